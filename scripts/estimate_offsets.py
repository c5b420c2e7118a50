#!/usr/bin/env python
"""
Estimates the per-subject sensor offsets from calibration recordings (em_pose_amd/data/offsets.py; the estimator runs in
HIP, csrc/offset_stats.hip) and writes one `<subject>_offsets.npz` per subject -- the files `scripts/train.py
--offset_files`, `scripts/evaluate_real.py` and `SampleMarkersWithOffsets` read.

    python scripts/estimate_offsets.py --recordings DIR --out DIR [--smpl_model model.npz] [--subject_from_id REGEX]
    python scripts/estimate_offsets.py --synthetic --out DIR
    python scripts/estimate_offsets.py --recordings DIR --out DIR --search_placement [--exclude_hands]

`--recordings`: a directory of `*_clean.npz` recordings (real sensor readings with ground-truth SMPL parameters).  The
recordings are grouped by subject: the part of the recording id before the first `_`, or the first group (or the whole
match) of `--subject_from_id`.  `--synthetic` needs no data: a few `synthetic.make_sequence` recordings of two subjects on
the stand-in body model.  Per sensor the script prints the number of frames, |means| in mm, sqrt(trace covs) in mm and
the spread of the rotational offsets in degrees.

`--search_placement` first searches the mesh for the sites of the sensors (em_pose_amd/data/placement.py; the search runs in
HIP, csrc/placement.hip), all recordings pooled: per sensor it prints the vertex the readings are closest to, its rms
distance in mm, the runner-up with its rms, and whether the site is CONSTANTS.VERTEX_IDS[m]; below that table, per sensor,
the mean distance of the readings to the ground-truth SURFACE (eval/surface_metrics.py) beside the rms to the site -- a
site whose rms is far above the skin distance is a vertex that is not under the strap.  The offsets are then
estimated at the found sites and the files carry them as `vertex_ids`.  `--exclude_hands` leaves the vertices skinned to
the finger joints out of the search.
"""
import argparse
import glob
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from em_pose_amd import synthetic  # noqa: E402
from em_pose_amd.bodymodels.smpl import SMPLLayer  # noqa: E402
from em_pose_amd.data.data import RealSample  # noqa: E402
from em_pose_amd.data.offsets import estimate_offsets, save_offsets_npz  # noqa: E402


def subject_of(seq_id, pattern):
    if pattern is None:
        return str(seq_id).split('_', 1)[0]
    found = re.search(pattern, str(seq_id))
    if not found:
        raise SystemExit("--subject_from_id '{}' does not match recording id '{}'".format(pattern, seq_id))
    return found.group(1) if found.groups() else found.group(0)


def synthetic_recordings(smpl, device):
    """Two subjects, two and one recordings: every recording of a subject carries the subject's offsets."""
    from em_pose_amd.helpers.configuration import lgd_config
    from em_pose_amd.nn.models import create_model
    net = create_model(lgd_config(12, False, 1, hidden=32), SMPLLayer(smpl.model)).to(device).eval()
    rng = np.random.default_rng(0)
    samples, subjects = [], []
    for subject, seeds in (('synthA', (100, 101)), ('synthB', (102,))):
        t = rng.normal(0.0, 0.02, (1, 12, 3)).astype(np.float32)
        r = synthetic._exp_so3(rng.normal(0.0, 0.1, (1, 12, 3))).astype(np.float32)

        def sensors(poses, betas, o_r, o_t, t=t, r=r):
            pos, ori, _ = net.get_estimated_real_markers(torch.from_numpy(poses).to(device),
                                                         torch.from_numpy(betas).to(device), torch.from_numpy(r).to(device),
                                                         torch.from_numpy(t).to(device), frames_per_window=poses.shape[0])
            return pos.cpu().numpy(), ori.cpu().numpy()
        for k, seed in enumerate(seeds):
            d = synthetic.make_sequence(synthetic.README_SEQUENCE_LENGTHS[seed - 100], seed, sensors)
            samples.append(RealSample('%s_%02d' % (subject, k), d['sensor_pos'], d['sensor_oris'],
                                      d['sensor_masks'].astype(np.float32), d['smpl_poses'], d['smpl_shape'],
                                      d['smpl_trans'], {'means': None, 'covs': None, 'r': None}))
            subjects.append(subject)
    return samples, subjects


def search_sites(smpl, samples, exclude_hands, device):
    """The sites of the sensors, all recordings pooled, printed per sensor; a sensor without a site ends the script."""
    from em_pose_amd.data.placement import candidates_excluding_bones, search_placement
    from em_pose_amd.helpers.configuration import CONSTANTS
    candidates = None
    if exclude_hands:
        candidates = candidates_excluding_bones(smpl, range(CONSTANTS.N_JOINTS + 1, smpl.n_joints))
        print('searching {} of {} vertices (hands excluded)'.format(len(candidates), smpl.n_vertices))
    found = search_placement(smpl, samples, candidates=candidates, device=device)['all']
    print('placement of {} sensors from {} recording(s)'.format(len(found['vertex_ids']), len(samples)))
    print('  {:>6} {:>8} {:>8} {:>10} {:>10} {:>14} {:>10}'.format('sensor', 'n', 'site', 'rms mm', 'runner-up', 'runner-up mm',
                                                                  'default'))
    for m, site in enumerate(found['vertex_ids']):
        default = CONSTANTS.VERTEX_IDS[m] if m < len(CONSTANTS.VERTEX_IDS) else None
        print('  {:>6} {:>8} {:>8} {:>10.2f} {:>10} {:>14.2f} {:>10}'.format(
            m, int(found['counts'][m]), int(site), float(found['rms_mm'][m]), int(found['runner_up_ids'][m]),
            float(found['runner_up_rms_mm'][m]), 'same' if default == int(site) else 'was {}'.format(default)))
    print('  {:>6} {:>10} {:>10}'.format('sensor', 'skin mm', 'rms mm'))
    for m in range(len(found['vertex_ids'])):
        print('  {:>6} {:>10.2f} {:>10.2f}'.format(m, float(found['skin_mm'][m]), float(found['rms_mm'][m])))
    if (found['vertex_ids'] < 0).any():
        raise SystemExit('sensors {} were read in no frame: no site, no offsets'.format(
            np.nonzero(found['vertex_ids'] < 0)[0].tolist()))
    return [int(v) for v in found['vertex_ids']]


def arg_parser():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument('--recordings', default=None, help='directory of *_clean.npz recordings')
    p.add_argument('--out', required=True, help='directory for the <subject>_offsets.npz files')
    p.add_argument('--smpl_model', default=None, help='SMPL-H model.npz (default: the synthetic stand-in body model)')
    p.add_argument('--subject_from_id', default=None, metavar='REGEX',
                   help='the subject of a recording: first group (or the match) of REGEX in its id; default: the id up to '
                        'the first "_"')
    p.add_argument('--synthetic', action='store_true', help='synthetic recordings on the stand-in body model')
    p.add_argument('--search_placement', action='store_true',
                   help='search the mesh for the sites of the sensors first and estimate the offsets there')
    p.add_argument('--exclude_hands', action='store_true',
                   help='with --search_placement: leave out the vertices skinned to the finger joints')
    p.add_argument('--device', default='cuda:0')
    return p


def main():
    args = arg_parser().parse_args()
    if args.exclude_hands and not args.search_placement:
        raise SystemExit('--exclude_hands goes with --search_placement')
    if not args.synthetic and not args.recordings:
        raise SystemExit('pass --recordings DIR or --synthetic')
    if not torch.cuda.is_available():
        raise SystemExit('the estimator runs in HIP and needs an MI355X; there is no CPU path')
    device = torch.device(args.device)
    smpl = SMPLLayer(args.smpl_model if args.smpl_model else synthetic.make_model()).to(device)
    if args.synthetic:
        samples, subjects = synthetic_recordings(smpl, device)
    else:
        files = sorted(glob.glob(os.path.join(args.recordings, '*_clean.npz')))
        if not files:
            raise SystemExit('no *_clean.npz files in {}'.format(args.recordings))
        samples = [RealSample.from_npz_clean(f) for f in files]
        subjects = [subject_of(s.id, args.subject_from_id) for s in samples]
    vertex_ids = search_sites(smpl, samples, args.exclude_hands, device) if args.search_placement else None
    estimates = estimate_offsets(smpl, samples, subjects=subjects, vertex_ids=vertex_ids, device=device)
    os.makedirs(args.out, exist_ok=True)
    for subject, est in estimates.items():
        path = os.path.join(args.out, '{}_offsets.npz'.format(subject))
        save_offsets_npz(path, est)
        n_rec = sum(1 for s in subjects if s == subject)
        print('{}: {} recording(s) -> {}'.format(subject, n_rec, path))
        print('  {:>6} {:>8} {:>12} {:>18} {:>12}'.format('sensor', 'n', '|means| mm', 'sqrt(tr covs) mm', 'spread deg'))
        for m in range(len(est['counts'])):
            print('  {:>6} {:>8} {:>12.2f} {:>18.2f} {:>12.2f}'.format(
                m, int(est['counts'][m]), 1e3 * float(np.linalg.norm(est['means'][m])),
                1e3 * float(np.sqrt(np.trace(est['covs'][m]))), float(est['r_spread_deg'][m])))


if __name__ == '__main__':
    main()
