"""Ground truth beside an estimate, frame by frame: what `scripts/evaluate_real.py --visualize` and
`scripts/render_sequence.py --side_by_side` write."""
import torch

from em_pose_amd.vis.camera import fit_camera
from em_pose_amd.vis.renderer import error_colors


def render_comparison(renderer, body, body_hat, max_mm=100.0, frames_per_call=64, overlays=None, overlays_hat=None,
                      hidden_alpha=0.0):
    """`body`, `body_hat`: dicts with poses_body (T, 63), betas (T, 10) or (1, 10), and optionally poses_root, trans,
    on the device.  -> uint8 (T, H, 2 W, 3): the first body in the renderer's colour on the left, the second on the
    right, coloured by its per-vertex distance to the first (`error_colors`).  Both halves share one camera: the
    renderer's, or one fitted to the first body's joints over all T frames.  `overlays` / `overlays_hat`:
    `vis.overlay.Primitives` of all T frames (or lists of them) drawn into the left / right half."""
    from em_pose_amd.vis.overlay import Primitives
    overlays = Primitives.cat(overlays) if overlays is not None else None
    overlays_hat = Primitives.cat(overlays_hat) if overlays_hat is not None else None
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
            left = renderer.render(v, camera=camera, overlays=overlays.frames(s) if overlays is not None else None,
                                   hidden_alpha=hidden_alpha)
            right = renderer.render(v_hat, colors=error_colors(v, v_hat, max_mm), camera=camera,
                                    overlays=overlays_hat.frames(s) if overlays_hat is not None else None,
                                    hidden_alpha=hidden_alpha)
            out.append(torch.cat([left, right], dim=2))
    if not out:
        return torch.empty(0, renderer.height, 2 * renderer.width, 3, dtype=torch.uint8,
                           device=body['poses_body'].device)
    return torch.cat(out)


def sensor_overlays(net, readings_pos, readings_ori, masks, poses_hat, shape_hat, offset_r, offset_t):
    """What `scripts/evaluate_real.py --visualize_sensors` draws, as (overlays, overlays_hat) for `render_comparison`.
    readings_pos (T, M * 3), readings_ori (T, M * 9), masks (T, M) or None: the readings as the batch holds them, i.e.
    in the frame in which the model's reconstruction energy compares them with the virtual sensors -- the body with its
    root orientation relative to the first frame and no translation, which is the body `render_comparison` shows on both
    sides; nothing has to move.  poses_hat (T, 66), shape_hat (1 or T, 10), offset_r (1, M, 3, 3), offset_t (1, M, 3): the
    estimate, whose virtual sensors (offsets applied, `net.get_estimated_real_markers`) are drawn on the right in lighter
    colours together with a capsule from each reading to its virtual sensor.  A model without virtual sensors (the ResNet
    baseline) gets the readings on both sides and nothing else.  Missing readings (mask 0) are left out."""
    from em_pose_amd.vis.overlay import residual_primitives, sensor_primitives
    T = readings_pos.shape[0]
    pos = readings_pos.reshape(T, -1, 3).float()
    ori = readings_ori.reshape(T, pos.shape[1], 3, 3).float()
    readings = sensor_primitives(pos, ori, mask=masks)
    if T == 0 or not hasattr(net, 'get_estimated_real_markers'):
        return [readings], [readings]
    with torch.no_grad():
        pos_hat, ori_hat, _ = net.get_estimated_real_markers(poses_hat.float(), shape_hat.float().expand(T, -1),
                                                             offset_r[:1], offset_t[:1], frames_per_window=T)
    virtual = sensor_primitives(pos_hat, ori_hat, axis_length=0.05, origin_radius=0.012, color=(0.95, 0.95, 0.95))
    return [readings], [readings, virtual, residual_primitives(pos, pos_hat, mask=masks)]
