#!/usr/bin/env python
"""
Times the sensor placement search (em_pose_amd/data/placement.py, csrc/placement.hip) on the shape of the EM-POSE test
set -- 36 recordings with the frame counts of `synthetic.README_SEQUENCE_LENGTHS` (54 030 frames), pooled, 12 sensors --
over the whole V = 6890 synthetic body model, in slabs of 1024 frames:

  search_placement    end to end from numpy recordings: normalisation, uploads, root frames, the slab loop (mesh forward,
                      accumulation), finish, download
  mesh forwards       the `SMPLLayer.forward` calls of the slab loop alone
  placement kernels   the accumulation and finish calls of the slab loop alone, on one mesh buffer that every slab reuses
                      (their time does not depend on the values)
  torch restatement   the same slab loop with `((p[:, :, None] - v[:, None]) ** 2).sum(-1)`, masked, accumulated in
                      float64, then the division and `argmin`: end to end from the same device inputs (without the host
                      prologue, which it would share), and its scoring alone on the reused mesh buffer

Per row: 3 warm-up calls, then 10 timed calls, each measured with device events and with the host clock around the call
plus a final synchronisation; the medians are printed.  The table is measured three times in turn (rounds); the spread of
a median over the rounds is the run-to-run spread a difference has to exceed.  Peak allocation: the high-water mark of
torch's allocator over one call, above what was allocated before it.  Before anything is timed the restatement and the
kernel are compared.

    python scripts/dev/bench_placement_search.py [--out profiles/placement_search_mi355x.txt]
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
from em_pose_amd.data.offsets import pooled_recordings, root_normalized_poses  # noqa: E402
from em_pose_amd.data.placement import placement_finish, placement_scores, search_placement  # noqa: E402
from em_pose_amd.data.virtual_sensors import VirtualMarkerHelper  # noqa: E402
from em_pose_amd.helpers.configuration import CONSTANTS as C  # noqa: E402

ROUNDS = 3
SLAB = 1024


def timed(fn, calls=10, warmup=3):
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


def peak_mib(fn):
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - before) / 2.0 ** 20


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

    # recordings of the forward model: offsets on the sensors at CONSTANTS.VERTEX_IDS, 5 mm of noise
    samples = []
    t = rng.normal(0.0, 0.01, (12, 3))
    for i, n in enumerate(lengths):
        w = synthetic.make_windows(1, n, 100 + i)
        poses, shape = w['poses'][0], w['shapes'][0]
        with torch.no_grad():
            v, _ = sub(poses_body=up(poses[:, 3:]), betas=up(np.repeat(shape[None], n, axis=0)), poses_root=up(poses[:, :3]))
            pos, ori, _ = helper._forward(v, local)
        pos, ori = pos.cpu().numpy().astype(np.float64), ori.cpu().numpy().astype(np.float64)
        pos = pos + (ori @ t[None, :, :, None])[..., 0] + rng.normal(0.0, 0.005, pos.shape)
        masks = (rng.uniform(size=(n, 12)) > 0.002).astype(np.float32)
        samples.append(RealSample('s_%02d' % i, pos.astype(np.float32), ori.astype(np.float32), masks, poses, shape,
                                  np.zeros((n, 3), np.float32), {'means': None, 'covs': None, 'r': None}))
    total = int(sum(lengths))

    # the device inputs of the slab loop: what search_placement builds on its way
    rec = pooled_recordings(smpl, samples, None, 12, False, dev, 'bench')
    with torch.no_grad():
        poses_d = root_normalized_poses(smpl, rec, dev)
    betas_d, pos_d, masks_d = up(rec['betas']), up(rec['pos']), up(rec['masks'])
    slabs = [slice(at, min(at + SLAB, total)) for at in range(0, total, SLAB)]
    buffer = smpl(poses_body=poses_d[slabs[0], 3:], betas=betas_d[slabs[0]], poses_root=poses_d[slabs[0], :3])[0]

    def forward(sl):
        return smpl(poses_body=poses_d[sl, 3:], betas=betas_d[sl], poses_root=poses_d[sl, :3])[0]

    def forwards():
        with torch.no_grad():
            for sl in slabs:
                forward(sl)

    def kernels():
        sums = counts = None
        for sl in slabs:
            sums, counts = placement_scores(buffer[:sl.stop - sl.start], pos_d[sl], masks_d[sl], sums, counts)
        return placement_finish(sums, counts)

    def torch_scores(v, sl, sums, counts):
        valid = masks_d[sl] == 1
        d2 = ((pos_d[sl][:, :, None] - v[:, None]) ** 2).sum(-1)            # (T, 12, V) float32
        sums += (d2 * valid[..., None]).double().sum(dim=0)
        counts += valid.sum(dim=0)

    def torch_finish(sums, counts):
        score = (sums / counts[:, None]).float()
        return score, score.argmin(dim=1)

    def torch_search(mesh):
        with torch.no_grad():
            sums = torch.zeros(12, smpl.n_vertices, dtype=torch.float64, device=dev)
            counts = torch.zeros(12, dtype=torch.int64, device=dev)
            for sl in slabs:
                v = mesh(sl)
                torch_scores(v, sl, sums, counts)
                del v
            return torch_finish(sums, counts)

    ours = search_placement(smpl, samples, slab=SLAB)['all']
    score_t, best_t = torch_search(forward)
    score_t, best_t = score_t.cpu().numpy(), best_t.cpu().numpy()
    rel = float((np.abs(ours['score'] - score_t) / score_t).max())
    assert np.array_equal(ours['vertex_ids'], best_t) and rel <= 1e-5, (ours['vertex_ids'], best_t, rel)

    rows = (('search_placement', lambda: search_placement(smpl, samples, slab=SLAB)),
            ('  mesh forwards', forwards),
            ('  placement kernels', kernels),
            ('torch restatement', lambda: torch_search(forward)),
            ('  its scoring', lambda: torch_search(lambda sl: buffer[:sl.stop - sl.start])))
    res = {name: [] for name, _ in rows}
    for _ in range(ROUNDS):
        for name, fn in rows:
            res[name].append(timed(fn))
    peaks = {name: peak_mib(fn) for name, fn in rows}
    fmt = lambda x: '{:.3f} [{:.3f} .. {:.3f}]'.format(float(np.median(x)), min(x), max(x))
    lines = ['sensor placement search, {} recordings / {} frames pooled, 12 sensors, all V = 6890 vertices, {} slabs of at most '
             '{} frames, on {} ({}):'.format(len(lengths), total, len(slabs), SLAB, torch.cuda.get_device_name(0),
                                            torch.cuda.get_device_properties(0).gcnArchName),
             'median of 10 calls after 3 warm-up calls, milliseconds; median over {} rounds [lowest .. highest round]; peak '
             'allocation of one call in MiB'.format(ROUNDS),
             'sites found: {} (generated at CONSTANTS.VERTEX_IDS: {})'.format(
                 ours['vertex_ids'].tolist(), ours['vertex_ids'].tolist() == ids),
             'kernel against the torch restatement: same sites, largest relative difference of a score {:.3e}'.format(rel),
             '{:<22} {:>34} {:>34} {:>12}'.format('', 'events', 'wall', 'peak MiB')]
    for name, _ in rows:
        lines.append('{:<22} {:>34} {:>34} {:>12.1f}'.format(name, fmt([r[0] for r in res[name]]),
                                                             fmt([r[1] for r in res[name]]), peaks[name]))
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(text)


if __name__ == '__main__':
    main()
