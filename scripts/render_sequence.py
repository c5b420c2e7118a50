#!/usr/bin/env python
"""
Render a sequence of SMPL-H parameters to images on the GPU (em_pose_amd/vis: a z-buffer rasteriser in HIP; no display,
no OpenGL).

    python scripts/render_sequence.py --synthetic --out renders/            # a synthetic recording, synthetic body model
    python scripts/render_sequence.py --npz poses.npz --out renders/        # AMASS-style parameters (needs SMPL_MODELS)
    python scripts/render_sequence.py --npz gt.npz --side_by_side est.npz --out renders/

An AMASS-style file holds `poses` (T, >= 66: root, then 21 body joints, axis-angle), `betas` (>= 10) and optionally
`trans` (T, 3); `smpl_poses` / `smpl_shape` / `smpl_trans` of a `*_clean.npz` recording are read as well.  With
`--side_by_side` the first body is drawn in grey on the left and the second on the right, coloured by its per-vertex
distance to the first.  `--skeleton` draws the joints and bones into every body and `--sensors` the virtual sensors of
the rendered body (VirtualMarkerHelper at the 12 sensor vertices) as tripods, both by the overlay ray caster
(em_pose_amd/vis/overlay.py); `--xray ALPHA` is how much of them shows through the surface that hides them (default 0.6
with --skeleton, which lies inside the body, else 0).  Images are PNG where PIL is installed, binary PPM otherwise.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def load_npz(path, device):
    z = np.load(path)
    pick = lambda *names: next((z[n] for n in names if n in z.files), None)
    poses, betas, trans = pick('poses', 'smpl_poses'), pick('betas', 'smpl_shape'), pick('trans', 'smpl_trans')
    if poses is None or betas is None:
        raise SystemExit('{}: needs `poses` and `betas` (or `smpl_poses` and `smpl_shape`)'.format(path))
    poses = torch.from_numpy(np.asarray(poses, dtype=np.float32)).to(device)
    body = {'poses_root': poses[:, :3].contiguous(), 'poses_body': poses[:, 3:66].contiguous(),
            'betas': torch.from_numpy(np.asarray(betas, dtype=np.float32).reshape(1, -1)[:, :10].copy()).to(device)}
    if trans is not None:
        body['trans'] = torch.from_numpy(np.asarray(trans, dtype=np.float32)).to(device)
    return body


def synthetic_body(n_frames, seed, device, perturb=0.0):
    from em_pose_amd import synthetic
    rec = synthetic.make_windows(1, n_frames, seed)     # (what make_sequence records, without the sensor readings)
    poses = rec['poses'][0].astype(np.float32)
    if perturb:
        poses = poses + np.random.default_rng(seed + 1).normal(0.0, perturb, size=poses.shape).astype(np.float32)
    poses = torch.from_numpy(poses).to(device)
    return {'poses_root': poses[:, :3].contiguous(), 'poses_body': poses[:, 3:].contiguous(),
            'betas': torch.from_numpy(rec['shapes'].reshape(1, -1).astype(np.float32)).to(device)}


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument('--synthetic', action='store_true', help='Render a synthetic.make_sequence recording on the synthetic body model.')
    p.add_argument('--npz', default=None, help='AMASS-style parameter file to render.')
    p.add_argument('--side_by_side', default=None, metavar='NPZ', nargs='?', const='perturbed',
                   help='A second parameter file drawn beside the first (with --synthetic no file: the same motion, perturbed).')
    p.add_argument('--out', required=True, help='Directory the images are written into.')
    p.add_argument('--frames', type=int, default=120, help='--synthetic: frames of the recording.')
    p.add_argument('--seed', type=int, default=100)
    p.add_argument('--stride', type=int, default=1, help='Write every stride-th frame.')
    p.add_argument('--width', type=int, default=256)
    p.add_argument('--height', type=int, default=256)
    p.add_argument('--shading', default='smooth', choices=['smooth', 'flat'])
    p.add_argument('--skeleton', action='store_true', help='Draw the skeleton: a capsule per bone, a sphere per joint.')
    p.add_argument('--sensors', action='store_true', help='Draw the virtual sensors of the rendered body as tripods.')
    p.add_argument('--xray', type=float, default=None, metavar='ALPHA',
                   help='How much of an overlay shows through the surface that hides it, 0 .. 1 (default 0.6 with --skeleton, else 0).')
    p.add_argument('--sheet', type=int, default=0, metavar='COLUMNS', help='Also write one contact sheet with this many columns.')
    args = p.parse_args()
    if args.synthetic == (args.npz is not None):
        raise SystemExit('pass exactly one of --synthetic and --npz FILE')
    if args.npz is not None and args.side_by_side == 'perturbed':
        raise SystemExit('--side_by_side needs a second parameter file beside --npz')
    if not torch.cuda.is_available():
        raise SystemExit('render_sequence.py renders with a HIP kernel and needs an MI355X; there is no CPU fallback')
    device = torch.device('cuda', 0)
    from em_pose_amd.bodymodels.smpl import SMPLLayer, create_default_smpl_model
    from em_pose_amd.vis import MeshRenderer, contact_sheet, fit_camera, save_frames, save_image
    from em_pose_amd.vis.compare import render_comparison
    xray = args.xray if args.xray is not None else (0.6 if args.skeleton else 0.0)
    if not 0.0 <= xray <= 1.0:
        raise SystemExit('--xray must lie inside [0, 1]')
    if args.synthetic:
        from em_pose_amd import synthetic
        layer = SMPLLayer(synthetic.make_model()).to(device)
        body = synthetic_body(args.frames, args.seed, device)
        other = synthetic_body(args.frames, args.seed, device, perturb=0.05) if args.side_by_side else None
    else:
        layer = create_default_smpl_model(device)
        body = load_npz(args.npz, device)
        other = load_npz(args.side_by_side, device) if args.side_by_side else None
        if other is not None and other['poses_body'].shape[0] != body['poses_body'].shape[0]:
            raise SystemExit('--side_by_side: both files need the same number of frames')
    stride = max(args.stride, 1)
    cut = lambda d: {k: (v[::stride].contiguous() if k != 'betas' else v) for k, v in d.items()}
    renderer = MeshRenderer(layer, args.width, args.height)

    def overlays_of(vertices, joints):
        """The overlays of posed bodies: the skeleton from the joints, the virtual sensors from the mesh."""
        from em_pose_amd.bodymodels.tables import model_parents
        from em_pose_amd.data.virtual_sensors import VirtualMarkerHelper
        from em_pose_amd.helpers.configuration import CONSTANTS as C
        from em_pose_amd.vis import sensor_primitives, skeleton_primitives
        out = []
        if args.skeleton:
            out.append(skeleton_primitives(joints, model_parents(layer.model)))
        if args.sensors:
            pos, ori, _ = VirtualMarkerHelper(layer).get_virtual_pos_and_rot(vertices, C.VERTEX_IDS)
            out.append(sensor_primitives(pos, ori))
        return out or None

    def overlays_all(d):
        if not (args.skeleton or args.sensors):
            return None
        T = d['poses_body'].shape[0]
        parts = []
        with torch.no_grad():
            for t0 in range(0, T, 64):
                parts.append(overlays_of(*layer(**{k: (v[t0:t0 + 64] if v.shape[0] == T else v) for k, v in d.items()})))
        from em_pose_amd.vis import Primitives
        whole = [Primitives.cat(p) for p in parts]
        return Primitives(torch.cat([p.a for p in whole]), torch.cat([p.b for p in whole]),
                          torch.cat([p.radius if p.radius.dim() == 2 else p.radius.expand(p.n_frames, -1) for p in whole]),
                          whole[0].colors)

    if other is not None:
        body, other = cut(body), cut(other)
        rgb = render_comparison(renderer, body, other, overlays=overlays_all(body), overlays_hat=overlays_all(other),
                                hidden_alpha=xray)
    else:
        body = cut(body)
        T = body['poses_body'].shape[0]
        parts = []
        with torch.no_grad():          # one fixed camera that keeps the whole sequence in view
            renderer.camera = fit_camera(layer.fk_joints(**body), args.width, args.height)
        for t0 in range(0, T, 64):
            part = {k: (v[t0:t0 + 64] if k != 'betas' else v) for k, v in body.items()}
            parts.append(renderer.render_bodies(normals=args.shading, hidden_alpha=xray,
                                                overlays=overlays_of if args.skeleton or args.sensors else None, **part))
        rgb = torch.cat(parts)
    paths = save_frames(args.out, rgb, step=stride)
    if args.sheet > 0 and len(paths):
        save_image(os.path.join(args.out, 'sheet'), contact_sheet(list(rgb.cpu().numpy()), args.sheet))
    print('{} frames written to {}'.format(len(paths), args.out))


if __name__ == '__main__':
    main()
