#!/usr/bin/env python
"""
Times the overlay ray caster (em_pose_amd/vis draw_primitives -> empose_render_overlay, csrc/overlay.hip) on the V = 6890
synthetic body model: T = 256 frames at 256 x 256 and at 512 x 512 pixels with the full overlay of a frame -- 51 bones +
52 joints + 12 x 4 sensor primitives + 12 residuals = 175 primitives -- drawn over the rendered mesh with its depth and
hidden_alpha = 0.6, prim_id and prim_depth returned.

  draw_primitives              the two launches per slab, on images, depths and primitives that are already there
  draw_primitives, full boxes  the same call in a LAB BUILD of the library whose set-up kernel gives every primitive the
                               whole image as its box (-DEMPOSE_OVERLAY_FULL_BOXES, this script only): what the binning buys
  render                       MeshRenderer.render of the same frames -- the yardstick (profiles/render_mi355x.txt)

Per row: 10 warm-up calls, then 40 timed calls, each measured with device events and with the host clock around the call
plus a final synchronisation; the medians are printed.  The table is measured three times in turn (rounds); the spread of
a median over the rounds is the run-to-run spread a difference has to exceed.

    python scripts/dev/bench_overlay.py --build_lab          # no GPU needed: scripts/dev/bin/libempose_hip_fullboxes.so
    python scripts/dev/bench_overlay.py [--out profiles/overlay_mi355x.txt]

Without the lab build the second row is left out.  The lab library is measured in a child process (EMPOSE_LIB_PATH).
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

ROUNDS = 3
T = 256
SIZES = (256, 512)
LAB_LIB = os.path.join(ROOT, 'scripts', 'dev', 'bin', 'libempose_hip_fullboxes.so')


def build_lab():
    """overlay.hip with whole-image boxes, linked with the in-tree objects of every other source."""
    from em_pose_amd import build as B
    B.build()
    srcs = B.sources()
    if any(not os.path.exists(s[:-4] + '.o') for s in srcs):
        B.build(force=True)
    os.makedirs(os.path.dirname(LAB_LIB), exist_ok=True)
    lab_obj = os.path.join(os.path.dirname(LAB_LIB), 'overlay_fullboxes.o')
    hipcc = B._hipcc()
    subprocess.run([hipcc] + B.FLAGS + ['-DEMPOSE_OVERLAY_FULL_BOXES', '-c', os.path.join(B.CSRC, 'overlay.hip'), '-o', lab_obj],
                   check=True)
    objs = [lab_obj if os.path.basename(s) == 'overlay.hip' else s[:-4] + '.o' for s in srcs]
    subprocess.run([hipcc, '--offload-arch=' + B.ARCH, '-shared', '-fPIC', '-o', LAB_LIB] + objs, check=True)
    print('built', LAB_LIB)


def timed(fn, calls=40, warmup=10):
    import torch
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


def measure(with_render):
    """{row: [(events ms, wall ms)] * ROUNDS}, and notes on the scene."""
    import torch
    from em_pose_amd import synthetic
    from em_pose_amd.bodymodels.smpl import SMPLLayer
    from em_pose_amd.bodymodels.tables import model_parents
    from em_pose_amd.data.virtual_sensors import VirtualMarkerHelper
    from em_pose_amd.helpers.configuration import CONSTANTS as C
    from em_pose_amd.vis import (MeshRenderer, Primitives, draw_primitives, fit_camera, residual_primitives,
                                 sensor_primitives, skeleton_primitives)
    dev = torch.device('cuda:0')
    smpl = SMPLLayer(synthetic.make_model()).to(dev)
    g = torch.Generator().manual_seed(T)
    rnd = lambda *shape, s=1.0: (torch.randn(*shape, generator=g) * s).to(dev)
    pose, root, betas = rnd(T, 63, s=0.2), rnd(T, 3, s=0.3), rnd(T, 10)
    with torch.no_grad():
        vertices, joints = smpl(pose, betas, poses_root=root)
        normals = smpl.vertex_normals(vertices)
        pos, ori, _ = VirtualMarkerHelper(smpl).get_virtual_pos_and_rot(vertices, C.VERTEX_IDS)
    readings = pos + rnd(T, 12, 3, s=0.03)
    prims = Primitives.cat(skeleton_primitives(joints, model_parents(smpl.model)), sensor_primitives(readings, ori),
                           residual_primitives(readings, pos))
    rows, notes = [], ['{} primitives a frame'.format(prims.n_primitives)]
    for size in SIZES:
        cam = fit_camera(joints, size, size)
        r = MeshRenderer(smpl, size, size, camera=cam)
        rgb, _, depth = r.render(vertices, normals=normals, return_buffers=True)
        _, prim_id, _ = draw_primitives(rgb.clone(), prims, cam, depth=depth, hidden_alpha=0.6, return_buffers=True)
        notes.append('{0} x {0}: {1:.2f} % of the pixels hit by a primitive'.format(size, 100 * float((prim_id >= 0).float().mean())))
        rows.append(('draw_primitives {0} x {0}'.format(size),
                     lambda rgb=rgb, cam=cam, depth=depth: draw_primitives(rgb, prims, cam, depth=depth, hidden_alpha=0.6,
                                                                           return_buffers=True)))
        if with_render:
            rows.append(('render {0} x {0}'.format(size),
                         lambda r=r: r.render(vertices, normals=normals, return_buffers=True)))
    res = {name: [] for name, _ in rows}
    for _ in range(ROUNDS):
        for name, fn in rows:
            res[name].append(timed(fn))
    return res, notes


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--out', default=None)
    p.add_argument('--build_lab', action='store_true', help='Build the lab library with whole-image boxes and stop (no GPU needed).')
    p.add_argument('--child', action='store_true', help='(internal) measure draw_primitives alone and print JSON')
    args = p.parse_args()
    if args.build_lab:
        return build_lab()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('needs an MI355X: a timing without the GPU says nothing')
    if args.child:
        res, _ = measure(False)
        print('RESULT ' + json.dumps(res))
        return
    res, notes = measure(True)
    if os.path.exists(LAB_LIB):
        env = dict(os.environ, EMPOSE_LIB_PATH=LAB_LIB)
        out = subprocess.run([sys.executable, os.path.abspath(__file__), '--child'], env=env, stdout=subprocess.PIPE,
                             universal_newlines=True, check=True).stdout
        lab = json.loads([l for l in out.splitlines() if l.startswith('RESULT ')][-1][len('RESULT '):])
        for name, v in lab.items():
            res[name + ', full boxes'] = [tuple(x) for x in v]
    lines = ['Overlay ray caster, T = {} frames over the rendered V = 6890 mesh, on {} ({}):'.format(
                 T, torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).gcnArchName)] + notes + [
             'median of 40 calls after 10 warm-up calls, milliseconds per call; median over {} rounds [lowest .. highest '
             'round]; per frame: the events median / {}'.format(ROUNDS, T),
             '(render of the same frames before this kernel existed, profiles/render_mi355x.txt: 2.23 ms at 256 x 256, 7.25 ms '
             'at 512 x 512)']
    fmt = lambda x: '{:.4f} [{:.4f} .. {:.4f}]'.format(float(np.median(x)), min(x), max(x))
    lines.append('{:<40} {:>32} {:>32} {:>14}'.format('', 'events', 'wall', 'ms per frame'))
    for name in sorted(res, key=lambda n: (n.split(' x ')[-1].split(',')[0], n)):
        ev = [x[0] for x in res[name]]
        lines.append('{:<40} {:>32} {:>32} {:>14.5f}'.format(name, fmt(ev), fmt([x[1] for x in res[name]]),
                                                            float(np.median(ev)) / T))
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(text)


if __name__ == '__main__':
    main()
