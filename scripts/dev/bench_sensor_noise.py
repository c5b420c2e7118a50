#!/usr/bin/env python
"""
Times the sensor-noise step (em_pose_amd/data/noise_functions.py: host draws + one launch of empose_sensor_noise) against
a torch restatement of the reference's form of it -- the same host draws, then a Python loop over the batch entries with
three indexed device writes each (reference noise_functions.py:98-106,156-163) -- on the same GPU, at 12 x 32 and
256 x 32 windows of 12 sensors, for both modes.  Per variant: 10 warm-up calls, then 40 timed calls, each measured with
device events and with the host clock around the call plus a final synchronisation; the medians are printed.

    python scripts/dev/bench_sensor_noise.py [--out profiles/sensor_noise_mi355x.txt]
"""
import argparse
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from em_pose_amd.data import noise_functions as NF  # noqa: E402
from em_pose_amd.helpers.configuration import CONSTANTS as C  # noqa: E402


class LoopSpherical(NF.SphericalMarkerNoise):
    """The reference's write step in torch: per batch entry three indexed `+=`."""

    def __call__(self, batch, **kwargs):
        markers = batch.marker_pos_synth
        n, f, m = markers.shape[0], markers.shape[1], markers.shape[-1] // 3
        ms = markers.reshape(n, f, m, 3)
        window_len, plan = self.plan(n, f, m)
        h = plan.host
        dev = markers.device
        m_ids, sf = h['sensor'].long().to(dev), h['start'].long().to(dev)
        ef = sf + window_len
        thigh = torch.norm(ms[0, f // 2, C.THIGH_UPPER_IDX] - ms[0, 0, C.THIGH_LOWER_IDX])
        r = h['u_r'].to(dev) * self.max_r * thigh / 2
        thetas, phis = h['theta'].to(dev), h['phi'].to(dev)
        xs, ys, zs = r * torch.cos(thetas) * torch.sin(phis), r * torch.sin(thetas) * torch.cos(phis), r * torch.cos(phis)
        out = ms.clone()
        for i in range(n):
            out[i, sf[i]:ef[i], m_ids, 0] += xs[i]
            out[i, sf[i]:ef[i], m_ids, 1] += ys[i]
            out[i, sf[i]:ef[i], m_ids, 2] += zs[i]
        batch.marker_pos_noisy = out.reshape(n, f, -1)
        return batch


class LoopSuppression(NF.MarkerSuppressionNoise):
    """The reference's write step in torch: per batch entry three indexed assignments (the plan stays on the host, as the
    reference's does)."""

    def __call__(self, batch, **kwargs):
        markers = batch.marker_pos_synth
        n, f, m = markers.shape[0], markers.shape[1], markers.shape[-1] // 3
        window_len, plan = self.plan(n, f)
        ids, sf = plan.host['sensor'].long().to(markers.device), plan.host['start'].long()
        ef = sf + window_len
        outs = [markers.reshape(n, f, m, 3).clone(), batch.marker_ori_synth.reshape(n, f, m, 3, 3).clone(),
                batch.marker_normal_synth.reshape(n, f, m, 3).clone()]
        for i in range(n):
            for o in outs:
                o[i, sf[i]:ef[i], ids[i]] = self.mask_value
        batch.marker_pos_noisy, batch.marker_ori_noisy, batch.marker_normal_noisy = (o.reshape(n, f, -1) for o in outs)
        return batch


def timed(fn, batch, calls=40, warmup=10):
    ev, wall = [], []
    for it in range(warmup + calls):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        fn(batch)
        b.record()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if it >= warmup:
            ev.append(a.elapsed_time(b))
            wall.append((t1 - t0) * 1e3)
    return float(np.median(ev)), float(np.median(wall))


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--out', default=None)
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('needs an MI355X: a timing without the GPU says nothing')
    dev = torch.device('cuda:0')
    lines = ['sensor-noise step on {}: median of 40 calls after 10 warm-up calls, milliseconds'.format(
        torch.cuda.get_device_name(0)),
        '{:<12} {:<10} {:>14} {:>14} {:>14} {:>14}'.format('mode', 'windows', 'kernel events', 'kernel wall', 'loop events',
                                                           'loop wall')]
    for n, f in ((12, 32), (256, 32)):
        g = torch.Generator().manual_seed(n)
        batch = types.SimpleNamespace(marker_pos_synth=torch.randn(n, f, 36, generator=g).to(dev),
                                      marker_ori_synth=torch.randn(n, f, 108, generator=g).to(dev),
                                      marker_normal_synth=torch.randn(n, f, 36, generator=g).to(dev))
        pairs = (('spherical', NF.SphericalMarkerNoise(0.5, 0.25, 1), LoopSpherical(0.5, 0.25, 1)),
                 ('suppression', NF.MarkerSuppressionNoise(0.25, 1, 0.0), LoopSuppression(0.25, 1, 0.0)))
        for mode, kernel, loop in pairs:
            # the same seeds: the same plans; the outputs agree before anything is timed
            torch.manual_seed(0)
            a = kernel(types.SimpleNamespace(**vars(batch)))
            torch.manual_seed(0)
            b = loop(types.SimpleNamespace(**vars(batch)))
            err = float((a.marker_pos_noisy - b.marker_pos_noisy).abs().max())
            assert err <= 1e-6, err
            k_ev, k_wall = timed(kernel, batch)
            l_ev, l_wall = timed(loop, batch)
            lines.append('{:<12} {:<10} {:>14.4f} {:>14.4f} {:>14.4f} {:>14.4f}'.format(
                mode, '{} x {}'.format(n, f), k_ev, k_wall, l_ev, l_wall))
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(text)


if __name__ == '__main__':
    main()
