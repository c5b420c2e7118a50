"""
Overlays in rendered frames: a skeleton, sensor tripods and residuals as capsules and spheres, drawn on the device by
empose_render_overlay (csrc/overlay.hip, a per-pixel analytic ray caster in HIP; include/empose_hip.h states its
definition) into the images `MeshRenderer` produced and depth-tested against the mesh.

The builders (`skeleton_primitives`, `sensor_primitives`, `residual_primitives`) are plain torch on the device of their
inputs.  `draw_primitives` has no CPU path: tensors on the CPU raise `EmposeError`, as everywhere else in the package.
"""
import numpy as np
import torch

from em_pose_amd import _lib

BONE, SENSOR, RESIDUAL = (0.95, 0.85, 0.25), (0.15, 0.15, 0.15), (0.85, 0.10, 0.75)
AXES = ((0.9, 0.1, 0.1), (0.1, 0.7, 0.1), (0.1, 0.2, 0.9))       # the columns of a rotation: red, green, blue


class Primitives(object):
    """P capsules in each of T frames: a, b (T, P, 3) world coordinates (a == b: a sphere), radius (P,) or (T, P) (a
    primitive whose radius is not > 0 in a frame is skipped there), colors (P, 3) in [0, 1]."""

    def __init__(self, a, b, radius, colors):
        a, b = torch.as_tensor(a).float(), torch.as_tensor(b).float()
        if a.dim() != 3 or a.shape[2] != 3 or a.shape != b.shape:
            raise ValueError('a and b must both be (T, P, 3)')
        T, P = int(a.shape[0]), int(a.shape[1])
        radius = torch.as_tensor(radius, device=a.device).float()
        if radius.dim() == 0:
            radius = radius.expand(P)
        if tuple(radius.shape) not in ((P,), (T, P)):
            raise ValueError('radius must be a number, (P,) or (T, P)')
        colors = torch.as_tensor(colors, device=a.device).float()
        if tuple(colors.shape) == (3,):
            colors = colors.expand(P, 3)
        if tuple(colors.shape) != (P, 3):
            raise ValueError('colors must be an RGB triple or (P, 3)')
        self.a, self.b, self.radius, self.colors = a, b, radius, colors

    @property
    def n_frames(self):
        return int(self.a.shape[0])

    @property
    def n_primitives(self):
        return int(self.a.shape[1])

    @staticmethod
    def cat(*prims):
        """The primitives of all arguments (lists are flattened, None is left out), in order, frame by frame."""
        flat = []
        for p in prims:
            flat.extend(p if isinstance(p, (list, tuple)) else [p])
        flat = [p for p in flat if p is not None]
        if not flat:
            raise ValueError('nothing to concatenate')
        T = flat[0].n_frames
        if any(p.n_frames != T for p in flat):
            raise ValueError('all primitives need the same number of frames')
        per_frame = any(p.radius.dim() == 2 for p in flat)
        radius = [p.radius if p.radius.dim() == 2 or not per_frame else p.radius.unsqueeze(0).expand(T, -1) for p in flat]
        return Primitives(torch.cat([p.a for p in flat], dim=1), torch.cat([p.b for p in flat], dim=1),
                          torch.cat(radius, dim=-1), torch.cat([p.colors for p in flat], dim=0))

    def frames(self, s):
        """The primitives of the frames of slice `s`."""
        return Primitives(self.a[s], self.b[s], self.radius[s] if self.radius.dim() == 2 else self.radius, self.colors)


def skeleton_primitives(joints, parents, bone_radius=0.012, joint_radius=0.02, color=BONE):
    """joints (T, J, 3); parents: J indices, the root's negative (or its own).  A capsule per bone (from the parent to
    the joint), then a sphere per joint."""
    joints = torch.as_tensor(joints).float()
    parents = [int(p) for p in np.asarray(parents).reshape(-1)[:joints.shape[1]]]
    bones = [(p, j) for j, p in enumerate(parents) if 0 <= p != j]
    src = torch.tensor([p for p, _ in bones], dtype=torch.long, device=joints.device)
    dst = torch.tensor([j for _, j in bones], dtype=torch.long, device=joints.device)
    a = torch.cat([joints[:, src], joints], dim=1)
    b = torch.cat([joints[:, dst], joints], dim=1)
    radius = torch.tensor([bone_radius] * len(bones) + [joint_radius] * joints.shape[1], device=joints.device)
    return Primitives(a, b, radius, color)


def _present(pos, mask, mask_value):
    """(T, M) bool: the sensors that are drawn."""
    keep = torch.ones(pos.shape[:2], dtype=torch.bool, device=pos.device)
    if mask is not None:
        keep &= torch.as_tensor(mask, device=pos.device).reshape(pos.shape[:2]) > 0
    if mask_value is not None:
        keep &= ~(pos == mask_value).all(dim=-1)
    return keep & torch.isfinite(pos).all(dim=-1)


def sensor_primitives(pos, ori, mask=None, axis_length=0.08, axis_radius=0.004, origin_radius=0.015, color=SENSOR,
                      mask_value=None):
    """pos (T, M, 3), ori (T, M, 3, 3): a sphere at each reading, then three capsules along the columns of its rotation in
    red, green and blue (4 M primitives: the M spheres first).  Radius 0, i.e. not drawn, where `mask` (T, M) is false
    and where all three coordinates of a reading equal `mask_value` (the value missing sensors read in the batch)."""
    pos = torch.as_tensor(pos).float()
    T, M = int(pos.shape[0]), int(pos.shape[1])
    ori = torch.as_tensor(ori, device=pos.device).float().reshape(T, M, 3, 3)
    keep = _present(pos, mask, mask_value).float()
    tips = pos.unsqueeze(2) + axis_length * ori.transpose(2, 3)          # (T, M, 3 axes, 3)
    a = torch.cat([pos] + [pos] * 3, dim=1)
    b = torch.cat([pos] + [tips[:, :, k] for k in range(3)], dim=1)
    radius = torch.cat([keep * origin_radius] + [keep * axis_radius] * 3, dim=1)
    colors = torch.tensor([list(color)] * M + [list(c) for c in AXES for _ in range(M)], device=pos.device)
    return Primitives(a, b, radius, colors)


def residual_primitives(pos, pos_hat, mask=None, radius=0.005, color=RESIDUAL, mask_value=None):
    """A capsule from each reading pos (T, M, 3) to its virtual sensor pos_hat (T, M, 3); radius 0 where the reading is
    masked (as `sensor_primitives`)."""
    pos = torch.as_tensor(pos).float()
    pos_hat = torch.as_tensor(pos_hat, device=pos.device).float()
    if pos_hat.shape != pos.shape:
        raise ValueError('pos and pos_hat must both be (T, M, 3)')
    return Primitives(pos, pos_hat, _present(pos, mask, mask_value).float() * radius, color)


def draw_primitives(rgb, prims, camera, depth=None, hidden_alpha=0.0, light=(0.0, 0.0, -1.0), ambient=0.3,
                    return_buffers=False, slab_frames=0):
    """Draws `prims` into `rgb` IN PLACE.
    :param rgb: (T, H, W, 3) uint8 on the device, contiguous.
    :param camera: the `vis.camera.Camera` the frames were rendered with.
    :param depth: None, or the mesh depth (T, H, W) float32 of `MeshRenderer.render(..., return_buffers=True)`: a
      primitive shows where it is nearer than the mesh, strictly.
    :param hidden_alpha: how much of a primitive shows where the mesh hides it: 0 not at all, 1 as if there were no mesh.
    :return: rgb; with `return_buffers` also prim_id int32 (T, H, W), -1 where no primitive covers the pixel, and
      prim_depth float32 (T, H, W), +inf there -- both regardless of the mesh.
    """
    if not torch.is_tensor(rgb) or not rgb.is_cuda:
        raise _lib.EmposeError('draw_primitives needs GPU tensors; there is no CPU fallback')
    if rgb.dim() != 4 or rgb.shape[3] != 3 or rgb.dtype != torch.uint8 or not rgb.is_contiguous():
        raise ValueError('rgb must be a contiguous (T, H, W, 3) uint8 tensor')
    dev = rgb.device
    T, H, W = int(rgb.shape[0]), int(rgb.shape[1]), int(rgb.shape[2])
    P = prims.n_primitives
    if prims.n_frames != T:
        raise ValueError('{} frames of primitives for {} images'.format(prims.n_frames, T))
    if P > _lib.OVERLAY_MAX_PRIMS:
        raise ValueError('at most {} primitives a frame'.format(_lib.OVERLAY_MAX_PRIMS))
    if not 0.0 <= hidden_alpha <= 1.0:
        raise ValueError('hidden_alpha must lie inside [0, 1]')
    prim_id = torch.full((T, H, W), -1, dtype=torch.int32, device=dev) if return_buffers else None
    prim_depth = torch.full((T, H, W), float('inf'), dtype=torch.float32, device=dev) if return_buffers else None
    if T == 0 or P == 0:
        return (rgb, prim_id, prim_depth) if return_buffers else rgb
    for x in (prims.a, prims.b, prims.radius, prims.colors):
        if not x.is_cuda:
            raise _lib.EmposeError('draw_primitives needs GPU tensors; there is no CPU fallback')
    a, b = prims.a.detach().to(dev).contiguous(), prims.b.detach().to(dev).contiguous()
    radius, colors = prims.radius.detach().to(dev).contiguous(), prims.colors.detach().to(dev).contiguous()
    if depth is not None:
        if not depth.is_cuda:
            raise _lib.EmposeError('draw_primitives needs GPU tensors; there is no CPU fallback')
        if tuple(depth.shape) != (T, H, W) or depth.dtype != torch.float32:
            raise ValueError('depth must be (T, H, W) float32')
        depth = depth.contiguous()
    cam_R = torch.as_tensor(np.asarray(camera.R, dtype=np.float32), device=dev).contiguous()
    cam_t = torch.as_tensor(np.asarray(camera.t, dtype=np.float32), device=dev).contiguous()
    per_frame = cam_R.dim() == 3
    if tuple(cam_R.shape) != ((T, 3, 3) if per_frame else (3, 3)) or \
            tuple(cam_t.shape) != ((T, 3) if per_frame else (3,)):
        raise ValueError('camera R / t must be (3, 3) / (3,) or (T, 3, 3) / (T, 3)')

    d = _lib.OverlayDesc()
    d.T, d.P, d.H, d.W = T, P, H, W
    d.seg_a, d.seg_b, d.radius, d.radius_per_frame = _lib.dptr(a), _lib.dptr(b), _lib.dptr(radius), int(radius.dim() == 2)
    d.colors = _lib.dptr(colors)
    d.cam_R, d.cam_t, d.camera_per_frame = _lib.dptr(cam_R), _lib.dptr(cam_t), int(per_frame)
    d.fx, d.fy, d.cx, d.cy, d.near = camera.fx, camera.fy, camera.cx, camera.cy, camera.near
    d.light[:], d.ambient, d.hidden_alpha = tuple(light), float(ambient), float(hidden_alpha)
    d.mesh_depth, d.slab_frames = _lib.dptr(depth), int(slab_frames)
    d.rgb, d.prim_id, d.prim_depth = _lib.dptr(rgb), _lib.dptr(prim_id), _lib.dptr(prim_depth)
    lib = _lib.lib()
    with torch.cuda.device(dev):
        ws_bytes = lib.empose_render_overlay_workspace_bytes(T, P, H, W)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        _lib.check(lib.empose_render_overlay(_lib.C.byref(d), _lib.dptr(ws), ws_bytes, _lib.current_stream()))
    return (rgb, prim_id, prim_depth) if return_buffers else rgb
