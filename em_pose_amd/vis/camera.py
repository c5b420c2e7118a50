"""
Cameras of the mesh renderer (em_pose_amd/vis/renderer.py; the convention of csrc/raster.hip):

    p_c = R p + t,   the camera looks along +z,   x = fx X / Z + cx,   y = fy Y / Z + cy,   image y points down,

and the pixel of row i, column j has its centre at (j + 0.5, i + 0.5).  Host code, NumPy float64; the renderer rounds to
float32 once.
"""
import collections

import numpy as np

# R (3, 3) and t (3,) for one camera of all frames, or (T, 3, 3) and (T, 3) for one per frame.
Camera = collections.namedtuple('Camera', 'R t fx fy cx cy near')


def _unit(v, what):
    v = np.asarray(v, dtype=np.float64)
    n = np.linalg.norm(v)
    if not n > 0:
        raise ValueError(what + ' has no direction')
    return v / n


def look_at(eye, target, up=(0.0, 1.0, 0.0)):
    """(R, t) of a camera at `eye` that looks at `target`: the rows of R are right, down and forward in world
    coordinates (orthonormal, right-handed) and t = -R eye."""
    eye = np.asarray(eye, dtype=np.float64)
    forward = _unit(np.asarray(target, dtype=np.float64) - eye, 'target - eye')
    right = _unit(np.cross(forward, np.asarray(up, dtype=np.float64)), 'forward x up')
    down = np.cross(forward, right)
    R = np.stack([right, down, forward])
    return R, -R @ eye


def pinhole(width, height, fov_y_deg=40.0, near=0.05):
    """A camera at the origin with square pixels, the principal point at the image centre and the given vertical field
    of view."""
    if not 0.0 < fov_y_deg < 180.0:
        raise ValueError('fov_y_deg must lie inside (0, 180)')
    f = 0.5 * height / np.tan(np.deg2rad(fov_y_deg) / 2.0)
    return Camera(np.eye(3), np.zeros(3), float(f), float(f), width / 2.0, height / 2.0, float(near))


def project(camera, points):
    """(x, y, Z) of world points (..., 3) under a single camera; for the tests and for `fit_camera`."""
    p = np.asarray(points, dtype=np.float64) @ np.asarray(camera.R, dtype=np.float64).T + np.asarray(camera.t)
    return np.stack([camera.fx * p[..., 0] / p[..., 2] + camera.cx, camera.fy * p[..., 1] / p[..., 2] + camera.cy,
                     p[..., 2]], axis=-1)


def fit_camera(joints, width, height, fov_y_deg=40.0, margin=0.15, direction=(0.25, 0.1, 1.0), up=(0.0, 1.0, 0.0),
               near=0.05):
    """One fixed camera for a whole sequence: it looks at the centre of the joints' bounding box from `direction` (world
    coordinates, from the target towards the eye), from the smallest distance at which every joint of every frame
    projects inside the image shrunk by `margin` (a fraction of each half-extent, room for the flesh around the joints)
    and lies beyond `near`.
    :param joints: (..., 3) array or tensor, all frames of the sequence."""
    if hasattr(joints, 'detach'):
        joints = joints.detach().cpu().numpy()
    pts = np.asarray(joints, dtype=np.float64).reshape(-1, 3)
    if pts.shape[0] == 0 or not np.isfinite(pts).all():
        raise ValueError('fit_camera needs at least one joint and finite coordinates')
    if not 0.0 <= margin < 1.0:
        raise ValueError('margin must lie inside [0, 1)')
    cam = pinhole(width, height, fov_y_deg, near)
    target = 0.5 * (pts.min(axis=0) + pts.max(axis=0))
    d = _unit(direction, 'direction')
    R, _ = look_at(target + d, target, up)
    q = (pts - target) @ R.T     # camera axes, origin at the target: the eye sits at (0, 0, -dist)
    half_w, half_h = (1.0 - margin) * width / 2.0, (1.0 - margin) * height / 2.0
    dist = max(np.max(cam.fx * np.abs(q[:, 0]) / half_w - q[:, 2]), np.max(cam.fy * np.abs(q[:, 1]) / half_h - q[:, 2]),
               np.max(2.0 * near - q[:, 2]), 1e-3)
    dist *= 1.0 + 1e-9           # (the bound is met with equality by one joint: keep it inside after rounding)
    R, t = look_at(target + d * dist, target, up)
    return cam._replace(R=R, t=t)
