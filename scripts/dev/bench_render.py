#!/usr/bin/env python
"""
Times the mesh renderer (em_pose_amd/vis MeshRenderer.render -> empose_render_meshes, csrc/raster.hip) on the V = 6890
synthetic body model: T = 256 frames at 256 x 256 and at 512 x 512 pixels, smooth shading, face ids and depth returned.

  render            MeshRenderer.render on vertices and normals that are already there: the three launches per slab
  forward + normals SMPLLayer.forward plus SMPLLayer.vertex_normals for the same frames -- the yardstick: what it costs to
                    have something to draw

Per row: 10 warm-up calls, then 40 timed calls, each measured with device events and with the host clock around the call
plus a final synchronisation; the medians are printed.  The table is measured three times in turn (rounds); the spread of
a median over the rounds is the run-to-run spread a difference has to exceed.

    python scripts/dev/bench_render.py [--out profiles/render_mi355x.txt]

The split of a call over its three launches comes from a kernel trace, taken in a run of its own so that the tracing
does not touch the timings above:

    rocprofv3 --kernel-trace --stats -d <dir> -o trace --output-format csv -- python scripts/dev/bench_render.py --once 512
    python scripts/dev/bench_render.py --kernel_stats <dir>/.../trace_kernel_stats.csv --once 512 --out profiles/render_mi355x.txt

(the second command appends the rows of the raster kernels to the file).
"""
import argparse
import csv
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

ROUNDS = 3
T = 256
SIZES = (256, 512)
ONCE_CALLS = 20


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


def append_kernel_stats(path, size, out):
    rows = [r for r in csv.DictReader(open(path)) if 'raster_' in r.get('Name', '')]
    if not rows:
        raise SystemExit('no raster kernels in ' + path)
    total = sum(float(r['TotalDurationNs']) for r in rows)
    lines = ['', 'kernel trace of {} calls at {} x {} (T = {}), a run of its own: share of the three launches'.format(
        ONCE_CALLS + 1, size, size, T)]
    for r in sorted(rows, key=lambda r: r['Name']):
        name = re.search(r'raster_\w+', r['Name']).group(0)
        lines.append('{:<24} {:>6} launches {:>12.1f} us each {:>7.1f} %'.format(
            name, r['Calls'], float(r['AverageNs']) / 1e3, 100.0 * float(r['TotalDurationNs']) / total))
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if out:
        with open(out, 'a') as fh:
            fh.write(text)


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--out', default=None)
    p.add_argument('--once', type=int, default=0, metavar='SIZE',
                   help='No timing: one warm-up call and {} calls at SIZE x SIZE (to run under a kernel trace).'.format(ONCE_CALLS))
    p.add_argument('--kernel_stats', default=None, metavar='CSV',
                   help='Append the raster kernels of a rocprofv3 kernel_stats CSV (taken with --once SIZE) to --out; no GPU work.')
    args = p.parse_args()
    if args.kernel_stats:
        return append_kernel_stats(args.kernel_stats, args.once, args.out)
    if not torch.cuda.is_available():
        raise SystemExit('needs an MI355X: a timing without the GPU says nothing')
    from em_pose_amd import synthetic
    from em_pose_amd.bodymodels.smpl import SMPLLayer
    from em_pose_amd.vis import MeshRenderer, fit_camera
    dev = torch.device('cuda:0')
    smpl = SMPLLayer(synthetic.make_model()).to(dev)
    V = smpl.n_vertices
    g = torch.Generator().manual_seed(T)
    rnd = lambda cols, s: (torch.randn(T, cols, generator=g) * s).to(dev)
    pose, root, betas = rnd(63, 0.2), rnd(3, 0.3), rnd(10, 1.0)

    def forward():
        with torch.no_grad():
            v, j = smpl(pose, betas, poses_root=root)
            return v, smpl.vertex_normals(v), j
    vertices, normals, joints = forward()

    def renderer(size):
        return MeshRenderer(smpl, size, size, camera=fit_camera(joints, size, size))
    if args.once:
        r = renderer(args.once)
        for _ in range(ONCE_CALLS + 1):
            r.render(vertices, normals=normals, return_buffers=True)
        torch.cuda.synchronize()
        return
    lines = ['Mesh rendering, V = {}, {} faces, T = {} frames, on {} ({}):'.format(
                 V, smpl.faces.shape[0], T, torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).gcnArchName),
             'median of 40 calls after 10 warm-up calls, milliseconds per call; median over {} rounds [lowest .. highest '
             'round]; per frame: the events median / {}'.format(ROUNDS, T)]
    fmt = lambda x: '{:.4f} [{:.4f} .. {:.4f}]'.format(float(np.median(x)), min(x), max(x))
    rows = [('forward + normals', forward)]
    for size in SIZES:
        r = renderer(size)
        covered = float((r.render(vertices, normals=normals, return_buffers=True)[1] >= 0).float().mean())
        rows.append(('render {0} x {0}'.format(size), lambda r=r: r.render(vertices, normals=normals, return_buffers=True)))
        lines.append('{0} x {0}: {1:.1f} % of the pixels covered'.format(size, 100 * covered))
    res = {name: [] for name, _ in rows}
    for _ in range(ROUNDS):
        for name, fn in rows:
            res[name].append(timed(fn))
    lines.append('{:<20} {:>32} {:>32} {:>14}'.format('', 'events', 'wall', 'ms per frame'))
    for name, _ in rows:
        ev = [x[0] for x in res[name]]
        lines.append('{:<20} {:>32} {:>32} {:>14.5f}'.format(name, fmt(ev), fmt([x[1] for x in res[name]]),
                                                            float(np.median(ev)) / T))
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(text)


if __name__ == '__main__':
    main()
