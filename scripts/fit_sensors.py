#!/usr/bin/env python
"""
Fits SMPL-H to sensor readings without a trained model (em_pose_amd/nn/fitting.py; the descent loop runs in HIP,
csrc/sensor_fit.hip) and prints the metric table of the zero pose, of the fitter alone and, with `--refine`, of a
random-weight LGD model before and after a few descent steps from its estimate.  Beside the joint metrics stand the
per-vertex error of the surface and its Procrustes-aligned form (PVE, PA-PVE; eval/mesh_metrics.py): with few sensors
the fit drifts globally, and only the aligned figures tell a rotated but well-posed body from a wrongly posed one.
A second table holds the temporal columns of the joints (eval/temporal_metrics.py) for the same rows: the acceleration
error and the jitter of the estimate beside the jitter of the ground truth, each window a sequence of its own.
A third holds the skin distance of the readings (eval/surface_metrics.py): how far they are from the surface of the estimate
and of the ground truth, how many lie inside either, and how deep -- the figure that needs no ground truth.  (On the
stand-in body, whose surface may intersect itself, the inside columns follow the parity rule and mean little.)

    python scripts/fit_sensors.py --synthetic [--n_markers 6|12] [--steps K] [--refine] [--windows B] [--frames F]
                                  [--smooth {window,one_euro} [--smooth_sigma S] [--smooth_min_cutoff F --smooth_beta B]]

`--smooth` adds a fourth table: the temporal columns, MPJPE and MPJAE of every row, raw and after the filter
(eval/smoothing.py); the first three tables are what they are without it.

`--synthetic` needs no data: `synthetic.make_windows` on the stand-in body model.  The script exits non-zero if the
objective of what the fitter returns exceeds, for any window, the objective at its init.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from em_pose_amd import synthetic  # noqa: E402
from em_pose_amd.bodymodels.smpl import SMPLLayer  # noqa: E402
from em_pose_amd.data.data import SyntheticBatch  # noqa: E402
from em_pose_amd.eval.mesh_metrics import VertexErrorEngine  # noqa: E402
from em_pose_amd.eval.metrics import MetricsEngine  # noqa: E402
from em_pose_amd.eval.surface_metrics import SkinDistanceEngine  # noqa: E402
from em_pose_amd.eval.smoothing import OneEuroFilter, gaussian_taps, smooth_model_output, window_filter  # noqa: E402
from em_pose_amd.eval.temporal_metrics import TemporalMetricsEngine  # noqa: E402
from em_pose_amd.helpers.configuration import lgd_config  # noqa: E402
from em_pose_amd.nn.fitting import SensorFitter  # noqa: E402
from em_pose_amd.nn.models import create_model  # noqa: E402


def synthetic_batch(net, n_windows, n_frames, device):
    def sensors(poses, betas, o_r, o_t):
        t = lambda a: torch.from_numpy(a).to(device)
        pos, ori, _ = net.get_estimated_real_markers(t(poses), t(betas), t(o_r), t(o_t), frames_per_window=1)
        return pos.cpu().numpy(), ori.cpu().numpy()
    return SyntheticBatch(synthetic.make_windows(n_windows, n_frames, 2024, sensors), device=device)


COLUMNS = ('MPJPE [mm]', 'PA-MPJPE [mm]', 'MPJAE [deg]', 'PVE [mm]', 'PA-PVE [mm]')
HEAD = '{:<22s} {:>12s} {:>15s} {:>13s} {:>10s} {:>13s}'
TEMPORAL_COLUMNS = ('Accel [m/s^2]', 'Jitter [m/s^3]', 'Jitter GT [m/s^3]')
TEMPORAL_HEAD = '{:<22s} {:>15s} {:>16s} {:>19s}'


def row(smpl, batch, name, out):
    m = {}
    for eng in (MetricsEngine(smpl), VertexErrorEngine(smpl, procrustes=True)):
        eng.compute(batch.poses_body, batch.shapes, out['pose_hat'], out['shape_hat'], batch.seq_lengths,
                    batch.poses_root, out['root_ori_hat'])
        m.update(eng.get_metrics())
    return HEAD.format(name, *['{:.2f}'.format(m[k]) if 'deg' in k else '{:.1f}'.format(m[k]) for k in COLUMNS])


def temporal_row(smpl, batch, name, out):
    eng = TemporalMetricsEngine(smpl)
    eng.compute(batch.poses_body, batch.shapes, out['pose_hat'], out['shape_hat'], batch.seq_lengths, batch.poses_root,
                out['root_ori_hat'])
    m = eng.get_metrics()
    return TEMPORAL_HEAD.format(name, *['{:.1f}'.format(m[k]) for k in TEMPORAL_COLUMNS])


SKIN_HEAD = '{:<22s} {:>15s} {:>18s} {:>11s} {:>14s} {:>11s}'


def skin_row(smpl, batch, name, out):
    eng = SkinDistanceEngine(smpl)
    eng.compute(batch.poses_body, batch.shapes, out['pose_hat'], out['shape_hat'], batch.seq_lengths, batch.poses_root,
                out['root_ori_hat'], marker_pos=batch.marker_pos_synth, marker_masks=batch.marker_masks)
    m = eng.get_metrics()
    return SKIN_HEAD.format(name, *['{:.1f}'.format(m[k]) for k in SkinDistanceEngine.COLUMNS])


SMOOTH_COLUMNS = TEMPORAL_COLUMNS + ('MPJPE [mm]', 'MPJAE [deg]')
SMOOTH_HEAD = '{:<34s} {:>15s} {:>16s} {:>19s} {:>12s} {:>13s}'


def smooth_row(smpl, batch, name, out):
    """`--smooth`: the temporal columns, MPJPE and MPJAE of an estimate, raw or filtered."""
    m = {}
    for eng in (TemporalMetricsEngine(smpl), MetricsEngine(smpl)):
        eng.compute(batch.poses_body, batch.shapes, out['pose_hat'], out['shape_hat'], batch.seq_lengths, batch.poses_root,
                    out['root_ori_hat'])
        m.update(eng.get_metrics())
    return SMOOTH_HEAD.format(name, *['{:.2f}'.format(m[k]) if 'deg' in k else '{:.1f}'.format(m[k])
                                      for k in SMOOTH_COLUMNS])


def smoothing_filter(args):
    """(a `filt` of `smooth_model_output`, its label).  Every window is a sequence of its own, so the One-Euro filter
    starts fresh on every call."""
    if args.smooth == 'window':
        return window_filter(gaussian_taps(args.smooth_sigma)), 'window, sigma {:g}'.format(args.smooth_sigma)
    return (OneEuroFilter(22, 10, min_cutoff=args.smooth_min_cutoff, beta=args.smooth_beta),
            'one-euro, {:g} Hz, beta {:g}'.format(args.smooth_min_cutoff, args.smooth_beta))


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument('--smooth', default=None, choices=['window', 'one_euro'],
                   help='a fourth table: the temporal columns, MPJPE and MPJAE of every row raw and after a filter of '
                        'eval/smoothing.py (window: zero-phase Gaussian; one_euro: the causal One-Euro filter)')
    p.add_argument('--smooth_sigma', type=float, default=2.0, help='--smooth window: sigma of the Gaussian, frames')
    p.add_argument('--smooth_min_cutoff', type=float, default=1.0, help='--smooth one_euro: cut-off at rest, Hz')
    p.add_argument('--smooth_beta', type=float, default=0.0, help='--smooth one_euro: rise of the cut-off with the speed')
    p.add_argument('--synthetic', action='store_true', help='synthetic windows on the stand-in body model')
    p.add_argument('--n_markers', type=int, default=12, choices=(6, 12))
    p.add_argument('--steps', type=int, default=30)
    p.add_argument('--lr', type=float, default=0.05)
    p.add_argument('--refine', action='store_true', help='also polish the estimate of a random-weight LGD model')
    p.add_argument('--windows', type=int, default=16)
    p.add_argument('--frames', type=int, default=32)
    p.add_argument('--device', default='cuda:0')
    args = p.parse_args()
    if not args.synthetic:
        raise SystemExit('only --synthetic readings are wired up: real recordings go through scripts/evaluate_real.py')
    device = torch.device(args.device)
    smpl = SMPLLayer(synthetic.make_model())
    torch.manual_seed(0)
    net = create_model(lgd_config(args.n_markers, True, 4, hidden=64, rnn_hidden=64), smpl).to(device).eval()
    batch = synthetic_batch(net, args.windows, args.frames, device)
    fitter = SensorFitter(net, num_steps=args.steps, lr=args.lr)
    zero = SensorFitter(net, num_steps=0)(batch)
    fit = fitter(batch)
    print(HEAD.format('', *COLUMNS))
    print(row(smpl, batch, 'zero init', zero))
    print(row(smpl, batch, 'fitter, {} steps'.format(args.steps), fit))
    checks = [('fitter', fit['objective'])]
    shown = [('zero init', zero), ('fitter, {} steps'.format(args.steps), fit)]
    if args.refine:
        with torch.no_grad():
            est = net(batch)
        polished = fitter(batch, init=est)
        print(row(smpl, batch, 'LGD (random weights)', est))
        print(row(smpl, batch, 'LGD + {} steps'.format(args.steps), polished))
        checks.append(('polish', polished['objective']))
        shown += [('LGD (random weights)', est), ('LGD + {} steps'.format(args.steps), polished)]
    print(TEMPORAL_HEAD.format('', *TEMPORAL_COLUMNS))
    for name, out in shown:
        print(temporal_row(smpl, batch, name, out))
    print(SKIN_HEAD.format('', *SkinDistanceEngine.COLUMNS))
    for name, out in shown:
        print(skin_row(smpl, batch, name, out))
    if args.smooth:
        filt, label = smoothing_filter(args)
        valid = MetricsEngine.valid_frames(batch.seq_lengths, batch.poses_body.shape[0], batch.poses_body.shape[1])
        print(SMOOTH_HEAD.format('', *SMOOTH_COLUMNS))
        for name, out in shown:
            print(smooth_row(smpl, batch, name, out))
            print(smooth_row(smpl, batch, '  + ' + label, smooth_model_output(out, valid.to(device), smpl, filt)))
    worse = 0
    for name, rows in checks:
        rows = rows.cpu()
        ratio = rows[-1] / rows[0]
        print('{}: objective returned / at the init: min {:.3f}, max {:.3f}'.format(name, float(ratio.min()),
                                                                                   float(ratio.max())))
        worse += int((rows[-1] > rows[0]).sum())
    if worse:
        raise SystemExit('{} window(s) ended above their start'.format(worse))


if __name__ == '__main__':
    main()
