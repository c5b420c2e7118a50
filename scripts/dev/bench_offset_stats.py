#!/usr/bin/env python
"""
Times the per-subject offset estimator (em_pose_amd/data/offsets.py, csrc/offset_stats.hip) on the shape of the EM-POSE
test set -- 36 recordings with the frame counts of `synthetic.README_SEQUENCE_LENGTHS` (54 030 frames), pooled into 9
subjects of 4 recordings, 12 sensors -- on the V = 6890 synthetic body model:

  offset_stats       the two launches alone, on sub-mesh vertices and readings that are already on the device
  torch restatement  the same statistics in float32 torch on the same GPU: the sensor frames from the existing
                     virtual-sensor kernel, then o = ori^T (p - pos), Q = ori^T R, masked sums per subject and
                     torch.linalg.svd
  estimate_offsets   end to end from numpy recordings: normalisation, uploads, root frames, sub-mesh, launch, download

Per row: 10 warm-up calls, then 40 timed calls, each measured with device events and with the host clock around the call
plus a final synchronisation; the medians are printed.  The table is measured three times in turn (rounds); the spread of
a median over the rounds is the run-to-run spread a difference has to exceed.  Before anything is timed the restatement
and the kernel are compared.

    python scripts/dev/bench_offset_stats.py [--out profiles/offset_stats_mi355x.txt]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from em_pose_amd import synthetic  # noqa: E402
from em_pose_amd.bodymodels.smpl import SMPLLayer  # noqa: E402
from em_pose_amd.data.data import RealSample  # noqa: E402
from em_pose_amd.data.offsets import estimate_offsets, offset_stats  # noqa: E402
from em_pose_amd.data.virtual_sensors import VirtualMarkerHelper  # noqa: E402
from em_pose_amd.helpers.configuration import CONSTANTS as C  # noqa: E402

ROUNDS = 3
PER_SUBJECT = 4


def torch_restatement(helper, ids, vertices, pos_r, ori_r, masks, groups):
    pos, ori, _ = helper._forward(vertices, ids)
    ot = ori.transpose(-1, -2)
    valid = (masks == 1).float()
    o = torch.matmul(ot, (pos_r - pos)[..., None])[..., 0] * valid[..., None]
    Q = torch.matmul(ot, ori_r) * valid[..., None, None]
    means, covs, rs = [], [], []
    for first, n in groups:
        sl = slice(first, first + n)
        cnt = valid[sl].sum(dim=0)
        mu = o[sl].sum(dim=0) / cnt[:, None]
        d = (o[sl] - mu) * valid[sl][..., None]
        covs.append(torch.einsum('tmi,tmj->mij', d, d) / (cnt - 1)[:, None, None])
        U, S, Vh = torch.linalg.svd(Q[sl].sum(dim=0) / cnt[:, None, None])
        sign = torch.det(torch.matmul(U, Vh))
        U = torch.cat([U[..., :2], U[..., 2:] * sign[:, None, None]], dim=-1)
        means.append(mu)
        rs.append(torch.matmul(U, Vh))
    return torch.stack(means), torch.stack(covs), torch.stack(rs)


def timed(fn, calls=40, warmup=10):
    ev, wall = [], []
    for it in range(warmup + calls):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        fn()
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
    smpl = SMPLLayer(synthetic.make_model()).to(dev)
    ids = list(C.VERTEX_IDS)
    sub = smpl.sub_mesh(ids)
    helper, local = VirtualMarkerHelper(sub), sub.local_ids(ids)
    lengths = synthetic.README_SEQUENCE_LENGTHS
    rng = np.random.default_rng(0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)

    # recordings of the forward model: the subject's offsets on the sub-mesh sensors, 5 mm and 2 degrees of noise
    samples, subjects = [], []
    for i, n in enumerate(lengths):
        if i % PER_SUBJECT == 0:
            t = rng.normal(0.0, 0.02, (12, 3))
            r0 = synthetic._exp_so3(rng.normal(0.0, 0.1, (12, 3)))
        w = synthetic.make_windows(1, n, 100 + i)
        poses, shape = w['poses'][0], w['shapes'][0]
        with torch.no_grad():
            v, _ = sub(poses_body=up(poses[:, 3:]), betas=up(np.repeat(shape[None], n, axis=0)), poses_root=up(poses[:, :3]))
            pos, ori, _ = helper._forward(v, local)
        pos, ori = pos.cpu().numpy().astype(np.float64), ori.cpu().numpy().astype(np.float64)
        pos = pos + (ori @ t[None, :, :, None])[..., 0] + rng.normal(0.0, 0.005, pos.shape)
        ori = ori @ r0[None] @ synthetic._exp_so3(rng.normal(0.0, np.deg2rad(2.0), pos.shape))
        masks = (rng.uniform(size=(n, 12)) > 0.002).astype(np.float32)
        samples.append(RealSample('s%02d_%02d' % (i // PER_SUBJECT, i), pos.astype(np.float32), ori.astype(np.float32),
                                  masks, poses, shape, np.zeros((n, 3), np.float32), {'means': None, 'covs': None, 'r': None}))
        subjects.append('s%02d' % (i // PER_SUBJECT))

    # the device inputs of the launch alone: what estimate_offsets builds on its way
    total = int(sum(lengths))
    per_subject = [int(sum(lengths[i:i + PER_SUBJECT])) for i in range(0, len(lengths), PER_SUBJECT)]
    groups = [(int(sum(per_subject[:g])), n) for g, n in enumerate(per_subject)]
    poses = np.concatenate([s.smpl_poses for s in samples])
    betas = np.concatenate([np.repeat(s.smpl_shape[None], s.n_frames, axis=0) for s in samples])
    with torch.no_grad():
        vertices, _ = sub(poses_body=up(poses[:, 3:]), betas=up(betas), poses_root=up(poses[:, :3]))
    pos_r = up(np.concatenate([s.marker_pos_real.reshape(-1, 12, 3) for s in samples]))
    ori_r = up(np.concatenate([s.marker_ori_real.reshape(-1, 12, 3, 3) for s in samples]))
    masks = up(np.concatenate([s.marker_masks for s in samples]))

    ours = offset_stats(helper, vertices, local, pos_r, ori_r, masks, groups)
    theirs = torch_restatement(helper, local, vertices, pos_r, ori_r, masks, groups)
    diff = [float((ours[k] - w).abs().max()) for k, w in zip(('means', 'covs', 'r'), theirs)]
    assert diff[0] <= 1e-6 and diff[1] <= 1e-8 and diff[2] <= 1e-5, diff
    est = estimate_offsets(smpl, samples, subjects=subjects)
    assert len(est) == len(groups) and all(np.array_equal(e['counts'], ours['counts'][g].cpu().numpy())
                                           for g, e in enumerate(est.values()))

    rows = (('offset_stats', lambda: offset_stats(helper, vertices, local, pos_r, ori_r, masks, groups)),
            ('torch restatement', lambda: torch_restatement(helper, local, vertices, pos_r, ori_r, masks, groups)),
            ('estimate_offsets', lambda: estimate_offsets(smpl, samples, subjects=subjects)))
    res = {name: [] for name, _ in rows}
    for _ in range(ROUNDS):
        for name, fn in rows:
            res[name].append(timed(fn))
    fmt = lambda x: '{:.4f} [{:.4f} .. {:.4f}]'.format(float(np.median(x)), min(x), max(x))
    lines = ['per-subject offset estimation, {} recordings / {} frames / {} subjects, 12 sensors, V = 6890 (sub-mesh of {}), '
             'on {} ({}):'.format(len(lengths), total, len(groups), len(sub.needed), torch.cuda.get_device_name(0),
                                  torch.cuda.get_device_properties(0).gcnArchName),
             'median of 40 calls after 10 warm-up calls, milliseconds; median over {} rounds [lowest .. highest round]'.format(ROUNDS),
             'kernel against the torch restatement, largest differences: means {:.3e} covs {:.3e} r {:.3e}'.format(*diff),
             '{:<20} {:>32} {:>32}'.format('', 'events', 'wall')]
    for name, _ in rows:
        lines.append('{:<20} {:>32} {:>32}'.format(name, fmt([r[0] for r in res[name]]), fmt([r[1] for r in res[name]])))
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(text)


if __name__ == '__main__':
    main()
