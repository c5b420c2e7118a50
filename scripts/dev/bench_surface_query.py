#!/usr/bin/env python
"""
Times the point-to-mesh query (em_pose_amd/eval/surface_metrics.py, csrc/surface_query.hip) on the V = 6890 synthetic body
model with 12 readings a frame, at T = 1024 frames (one slab) and at T = 54 030 (the EM-POSE test set):

  query, inside         `closest_point_on_mesh(..., inside=True)` on a mesh buffer that is already on the device
  query, distance only  the same with `inside=False`
  surface_distance      `SMPLLayer.surface_distance` end to end from poses and shapes: the mesh forwards in slabs of 1024
                        frames and a query per slab, with the inside test
  torch restatement     the distance alone (no inside test) by the same Voronoi-region rules on (frames, 12, F) tensors in
                        float32 torch on the same GPU, in chunks of 32 frames so that it fits, from the same mesh buffer

Per row: warm-up calls, then timed calls (3 + 10 for the kernel rows, 1 + 3 for the restatement), each measured with device
events and with the host clock around the call plus a final synchronisation; the medians are printed.  The table is
measured three times in turn (rounds); the spread of a median over the rounds is the run-to-run spread a difference has to
exceed.  Peak allocation: the high-water mark of torch's allocator over one call, above what was allocated before it.
Before anything is timed the restatement and the kernel are compared at T = 1024.

    python scripts/dev/bench_surface_query.py [--out profiles/surface_query_mi355x.txt]
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
from em_pose_amd.eval.surface_metrics import closest_point_on_mesh  # noqa: E402

ROUNDS = 3
SLAB = 1024
CHUNK = 32
Q = 12


def timed(fn, calls, warmup):
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


def torch_distance(vertices, faces, points):
    """dist (T, Q): the closest point by Voronoi regions on (chunk, Q, F) tensors, float32."""
    dot = lambda u, v: (u * v).sum(-1)
    out = []
    for at in range(0, vertices.shape[0], CHUNK):
        v, p = vertices[at:at + CHUNK], points[at:at + CHUNK, :, None]
        a, b, c = v[:, faces[:, 0]][:, None], v[:, faces[:, 1]][:, None], v[:, faces[:, 2]][:, None]
        ab, ac, ap, bp, cp = b - a, c - a, p - a, p - b, p - c
        d1, d2, d3, d4, d5, d6 = dot(ab, ap), dot(ac, ap), dot(ab, bp), dot(ac, bp), dot(ab, cp), dot(ac, cp)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        quot = lambda num, den: torch.where(den > 0, num / den.clamp_min(1e-38), torch.zeros_like(num))
        s = va.clamp_min(0) + vb.clamp_min(0) + vc.clamp_min(0)
        v_in, w_in = quot(vb.clamp_min(0), s), quot(vc.clamp_min(0), s)
        point = a + v_in[..., None] * ab + w_in[..., None] * ac
        t_bc = quot(d4 - d3, (d4 - d3) + (d5 - d6))
        regions = (((va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0), b + t_bc[..., None] * (c - b)),
                   ((vb <= 0) & (d2 >= 0) & (d6 <= 0), a + quot(d2, d2 - d6)[..., None] * ac),
                   ((d6 >= 0) & (d5 <= d6), c.expand_as(point)),
                   ((vc <= 0) & (d1 >= 0) & (d3 <= 0), a + quot(d1, d1 - d3)[..., None] * ab),
                   ((d3 >= 0) & (d4 <= d3), b.expand_as(point)),
                   ((d1 <= 0) & (d2 <= 0), a.expand_as(point)))
        for region, pt in regions:                              # the last one written wins: the first of the rule's order
            point = torch.where(region[..., None], pt, point)
        out.append(((p - point) ** 2).sum(-1).min(dim=-1).values.sqrt())
    return torch.cat(out)


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--out', default=None)
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('needs an MI355X: a timing without the GPU says nothing')
    dev = torch.device('cuda:0')
    smpl = SMPLLayer(synthetic.make_model()).to(dev)
    faces = smpl.surface_faces(dev)
    faces_long = faces.dev.long()
    rng = np.random.default_rng(0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    lines, checked = [], None
    for total in (SLAB, int(sum(synthetic.README_SEQUENCE_LENGTHS))):
        w = synthetic.make_windows(1, total, 100)
        poses, betas = up(w['poses'][0]), up(np.repeat(w['shapes'], total, axis=0))
        with torch.no_grad():
            mesh = torch.cat([smpl(poses_body=poses[at:at + SLAB, 3:], betas=betas[at:at + SLAB],
                                   poses_root=poses[at:at + SLAB, :3])[0] for at in range(0, total, SLAB)])
        sites = rng.choice(smpl.n_vertices, size=Q, replace=False)
        points = (mesh[:, sites] + up(rng.normal(0.0, 0.015, size=(total, Q, 3)))).contiguous()
        if checked is None:
            ours = closest_point_on_mesh(mesh, faces, points).dist
            checked = float((ours - torch_distance(mesh, faces_long, points)).abs().max())
            assert checked <= 2e-6, checked
        rows = (('query, inside', lambda: closest_point_on_mesh(mesh, faces, points, inside=True), 10, 3),
                ('query, distance only', lambda: closest_point_on_mesh(mesh, faces, points, inside=False), 10, 3),
                ('surface_distance', lambda: smpl.surface_distance(points, poses[:, 3:], betas, poses_root=poses[:, :3],
                                                                   slab=SLAB), 10, 3),
                ('torch restatement', lambda: torch_distance(mesh, faces_long, points), 3, 1))
        res = {name: [] for name, _, _, _ in rows}
        for _ in range(ROUNDS):
            for name, fn, calls, warmup in rows:
                res[name].append(timed(fn, calls, warmup))
        peaks = {name: peak_mib(fn) for name, fn, _, _ in rows}
        fmt = lambda x: '{:.3f} [{:.3f} .. {:.3f}]'.format(float(np.median(x)), min(x), max(x))
        lines.append('T = {} frames ({:.1f} MiB of vertices):'.format(total, mesh.numel() * 4 / 2.0 ** 20))
        lines.append('{:<22} {:>36} {:>36} {:>12}'.format('', 'events', 'wall', 'peak MiB'))
        for name, _, _, _ in rows:
            lines.append('{:<22} {:>36} {:>36} {:>12.1f}'.format(name, fmt([r[0] for r in res[name]]),
                                                                 fmt([r[1] for r in res[name]]), peaks[name]))
        del mesh, points
    head = ['point-to-mesh query, V = {}, F = {}, Q = {} readings a frame, on {} ({}):'.format(
                smpl.n_vertices, len(faces), Q, torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).gcnArchName),
            'median of the timed calls (10 after 3 warm-up calls; the restatement 3 after 1), milliseconds; median over {} '
            'rounds [lowest .. highest round]; peak allocation of one call in MiB'.format(ROUNDS),
            'surface_distance: mesh forwards in slabs of {} frames + a query per slab; torch restatement: distance only, '
            'float32, chunks of {} frames'.format(SLAB, CHUNK),
            'kernel against the torch restatement at T = {}: largest difference of a distance {:.3e} m'.format(SLAB, checked)]
    text = '\n'.join(head + lines) + '\n'
    print(text, end='')
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(text)


if __name__ == '__main__':
    main()
