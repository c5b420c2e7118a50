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
distance to the first.  Images are PNG where PIL is installed, binary PPM otherwise.
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
    if other is not None:
        rgb = render_comparison(renderer, cut(body), cut(other))
    else:
        body = cut(body)
        T = body['poses_body'].shape[0]
        parts = []
        with torch.no_grad():          # one fixed camera that keeps the whole sequence in view
            renderer.camera = fit_camera(layer.fk_joints(**body), args.width, args.height)
        for t0 in range(0, T, 64):
            part = {k: (v[t0:t0 + 64] if k != 'betas' else v) for k, v in body.items()}
            parts.append(renderer.render_bodies(normals=args.shading, **part))
        rgb = torch.cat(parts)
    paths = save_frames(args.out, rgb, step=stride)
    if args.sheet > 0 and len(paths):
        save_image(os.path.join(args.out, 'sheet'), contact_sheet(list(rgb.cpu().numpy()), args.sheet))
    print('{} frames written to {}'.format(len(paths), args.out))


if __name__ == '__main__':
    main()
