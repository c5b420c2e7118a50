"""Ground truth beside an estimate, frame by frame: what `scripts/evaluate_real.py --visualize` and
`scripts/render_sequence.py --side_by_side` write."""
import torch

from em_pose_amd.vis.camera import fit_camera
from em_pose_amd.vis.renderer import error_colors


def render_comparison(renderer, body, body_hat, max_mm=100.0, frames_per_call=64):
    """`body`, `body_hat`: dicts with poses_body (T, 63), betas (T, 10) or (1, 10), and optionally poses_root, trans,
    on the device.  -> uint8 (T, H, 2 W, 3): the first body in the renderer's colour on the left, the second on the
    right, coloured by its per-vertex distance to the first (`error_colors`).  Both halves share one camera: the
    renderer's, or one fitted to the first body's joints over all T frames."""
    layer = renderer.layer
    T = body['poses_body'].shape[0]
    frames = lambda d, s: {k: (v[s] if v is not None and v.shape[0] == T else v) for k, v in d.items()}
    camera = renderer.camera
    if camera is None:
        with torch.no_grad():
            camera = fit_camera(layer.fk_joints(**body), renderer.width, renderer.height)
    out = []
    with torch.no_grad():
        for t0 in range(0, T, frames_per_call):
            s = slice(t0, min(t0 + frames_per_call, T))
            v, _ = layer(**frames(body, s))
            v_hat, _ = layer(**frames(body_hat, s))
            left = renderer.render(v, camera=camera)
            right = renderer.render(v_hat, colors=error_colors(v, v_hat, max_mm), camera=camera)
            out.append(torch.cat([left, right], dim=2))
    if not out:
        return torch.empty(0, renderer.height, 2 * renderer.width, 3, dtype=torch.uint8,
                           device=body['poses_body'].device)
    return torch.cat(out)
