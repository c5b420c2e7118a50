#!/usr/bin/env python
"""
Times the Procrustes-aligned per-vertex error (PA-PVE) between two bodies on the V = 6890 synthetic body model, at 16 384
frames (one slab) and at 54 030 frames (the frame count of the EM-POSE test set, `synthetic.README_SEQUENCE_LENGTHS`):

  vertex_error pa  SMPLLayer.vertex_error(procrustes=True): two sweeps of the fused pair kernel around a per-frame 3 x 3
                   solve, no mesh written (csrc/mesh_err.hip)
  vertex_error     SMPLLayer.vertex_error alone -- the floor: one of the two sweeps
  composition      what anyone would write without it: SMPLLayer.forward for each body, centring, a batched
                   torch.linalg.svd on the device, alignment, norm and mean -- two meshes of 83 KB per frame written

Per row: 10 warm-up calls, then 40 timed calls, each measured with device events and with the host clock around the call
plus a final synchronisation; the medians are printed.  A row whose first call takes more than a quarter of a second is
timed with 2 + 5 calls instead, and its line says so.  The table is measured three times in turn (rounds); the spread of
a median over the rounds is the run-to-run spread a difference has to exceed.  The peak allocated bytes of a call
(torch.cuda.max_memory_allocated above what the inputs hold) are measured on one further call per row.  Before anything
is timed the routes are compared.

    python scripts/dev/bench_vertex_error_pa.py [--out profiles/vertex_error_pa_mi355x.txt]
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

ROUNDS = 3
FRAMES = (16384, int(sum(synthetic.README_SEQUENCE_LENGTHS)))


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


def first_call_ms(fn):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return int(peak)


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--out', default=None)
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('needs an MI355X: a timing without the GPU says nothing')
    dev = torch.device('cuda:0')
    smpl = SMPLLayer(synthetic.make_model()).to(dev)
    V = smpl.n_vertices
    lines = ['Procrustes-aligned per-vertex error between two bodies, V = {}, on {} ({}):'.format(
                 V, torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).gcnArchName),
             'median of 40 calls after 10 warm-up calls, milliseconds; median over {} rounds [lowest .. highest round]; '
             'peak: bytes allocated by one call above its inputs'.format(ROUNDS)]
    fmt = lambda x: '{:.4f} [{:.4f} .. {:.4f}]'.format(float(np.median(x)), min(x), max(x))
    for n in FRAMES:
        g = torch.Generator().manual_seed(n)
        rnd = lambda cols, s: (torch.randn(n, cols, generator=g) * s).to(dev)
        pose, root, betas = rnd(63, 0.4), rnd(3, 0.5), rnd(10, 1.0)
        pose_h, root_h, betas_h = pose + rnd(63, 0.05), root + rnd(3, 0.02), betas + rnd(10, 0.3)

        def fused():
            return smpl.vertex_error(pose, betas, pose_h, betas_h, poses_root=root, poses_root_hat=root_h)

        def fused_pa():
            return smpl.vertex_error(pose, betas, pose_h, betas_h, poses_root=root, poses_root_hat=root_h,
                                     procrustes=True)

        def composition():
            # eval/metrics.py procrustes_align in torch, float32, over the vertices
            with torch.no_grad():
                x, _ = smpl(pose, betas, poses_root=root)
                y, _ = smpl(pose_h, betas_h, poses_root=root_h)
                mu_x, mu_y = x.mean(dim=1, keepdim=True), y.mean(dim=1, keepdim=True)
                x0, y0 = x - mu_x, y - mu_y
                norm_x = x0.pow(2).sum(dim=(1, 2), keepdim=True).sqrt()
                norm_y = y0.pow(2).sum(dim=(1, 2), keepdim=True).sqrt()
                x0, y0 = x0 / norm_x, y0 / norm_y
                u, s_, vt = torch.linalg.svd(x0.transpose(1, 2) @ y0)
                v = vt.transpose(1, 2).clone()
                sign = torch.sign(torch.linalg.det(v @ u.transpose(1, 2)))
                v[:, :, -1] *= sign[:, None]
                s_ = torch.cat([s_[:, :2], s_[:, 2:] * sign[:, None]], dim=1)
                z = norm_x * s_.sum(dim=1)[:, None, None] * (y0 @ (v @ u.transpose(1, 2))) + mu_x
                return torch.linalg.norm(x - z, dim=-1).mean(dim=1)

        diff = float((fused_pa()[:, 2] / V - composition().double()).abs().max())
        assert diff <= 1e-5, diff
        assert torch.equal(fused_pa()[:, :2], fused())
        rows = (('vertex_error pa', fused_pa), ('vertex_error', fused), ('composition', composition))
        res = {name: [] for name, _ in rows}
        calls = {name: (40, 10) if first_call_ms(fn) <= 250.0 else (5, 2) for name, fn in rows}
        for _ in range(ROUNDS):
            for name, fn in rows:
                res[name].append(timed(fn, *calls[name]))
        lines.append('{} frames; per-frame mean aligned distance, fused against the composition, largest difference '
                     '{:.3e} m'.format(n, diff))
        lines.append('{:<16} {:>32} {:>32} {:>16}'.format('', 'events', 'wall', 'peak bytes'))
        for name, fn in rows:
            note = '' if calls[name][0] == 40 else '   ({} calls after {})'.format(*calls[name])
            lines.append('{:<16} {:>32} {:>32} {:>16d}{}'.format(name, fmt([r[0] for r in res[name]]),
                                                                fmt([r[1] for r in res[name]]), peak_bytes(fn), note))
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(text)


if __name__ == '__main__':
    main()
