"""
Headless rendering of posed body meshes on the device: `MeshRenderer` around empose_render_meshes (csrc/raster.hip, a
z-buffer rasteriser in HIP; include/empose_hip.h states its definition).  An Instinct card has no graphics pipeline and
no display, so nothing here needs one: meshes that are already on the device become uint8 images on the device.

There is no CPU path: tensors on the CPU raise `EmposeError`, as everywhere else in the package.
"""
import numpy as np
import torch

from em_pose_amd import _lib
from em_pose_amd.vis.camera import fit_camera

GREY = (0.7, 0.7, 0.7)


class MeshRenderer(object):
    def __init__(self, layer, width, height, camera=None, light=(0.0, 0.0, -1.0), ambient=0.3,
                 background=(1.0, 1.0, 1.0), color=GREY):
        """
        :param layer: an `SMPLLayer` (its `faces`; `forward` and `vertex_normals` for `render_bodies`).
        :param camera: a `vis.camera.Camera`; None: `fit_camera` on the joints of the first `render_bodies` call (a call
          of `render` then needs a camera of its own).
        :param light: direction in camera space; shading is two-sided, ambient + (1 - ambient) |n . l|.
        """
        if not (0 < width <= _lib.RENDER_MAX_IMAGE and 0 < height <= _lib.RENDER_MAX_IMAGE):
            raise ValueError('the image must be between 1 x 1 and {0} x {0}'.format(_lib.RENDER_MAX_IMAGE))
        self.layer, self.width, self.height = layer, int(width), int(height)
        self.camera, self.light, self.ambient = camera, tuple(light), float(ambient)
        self.background, self.color = tuple(background), tuple(color)
        self.slab_frames = 0          # 0: the library's choice (tests cut slabs short with it)
        self._faces_host = None
        self._faces_dev = None

    def _faces(self, device):
        if self._faces_host is None:
            self._faces_host = np.ascontiguousarray(self.layer.faces.detach().cpu().numpy().astype(np.int32))
        if self._faces_dev is None or self._faces_dev.device != device:
            self._faces_dev = torch.from_numpy(self._faces_host).to(device)
        return self._faces_host, self._faces_dev

    def render(self, vertices, normals='smooth', colors=None, return_buffers=False, camera=None, overlays=None,
               hidden_alpha=0.0):
        """
        :param vertices: (T, V, 3) float32 on the device.
        :param normals: 'smooth' (`layer.vertex_normals(vertices)`), 'flat' (face normals) or a (T, V, 3) tensor of
          un-normalised vertex normals.
        :param colors: None (the renderer's colour), an RGB triple, (V, 3) or (T, V, 3), values in [0, 1].
        :return: rgb uint8 (T, H, W, 3) on the device; with `return_buffers` also face_id int32 (T, H, W), -1 where no
          face covers the pixel, and depth float32 (T, H, W), +inf there.
        :param overlays: None, or `vis.overlay.Primitives` (or a list of them) of the same T frames, drawn into the
          images with `vis.overlay.draw_primitives` and depth-tested against the mesh; face_id and depth stay the mesh's.
        :param hidden_alpha: how much of an overlay shows through the mesh that hides it (0: not at all).
        """
        if overlays is not None:
            from em_pose_amd.vis.overlay import Primitives, draw_primitives
            rgb, face_id, depth = self.render(vertices, normals=normals, colors=colors, return_buffers=True, camera=camera)
            if rgb.shape[0]:
                draw_primitives(rgb, Primitives.cat(overlays), camera if camera is not None else self.camera, depth=depth,
                                hidden_alpha=hidden_alpha, light=self.light, ambient=self.ambient,
                                slab_frames=self.slab_frames)
            return (rgb, face_id, depth) if return_buffers else rgb
        if not torch.is_tensor(vertices) or not vertices.is_cuda:
            raise _lib.EmposeError('MeshRenderer needs GPU tensors; there is no CPU fallback')
        if vertices.dim() != 3 or vertices.shape[2] != 3:
            raise ValueError('vertices must be (T, V, 3)')
        camera = camera if camera is not None else self.camera
        if camera is None:
            raise ValueError('no camera: pass one here or to the constructor (vis.camera.fit_camera makes one)')
        dev = vertices.device
        T, V = int(vertices.shape[0]), int(vertices.shape[1])
        H, W = self.height, self.width
        rgb = torch.empty(T, H, W, 3, dtype=torch.uint8, device=dev)
        face_id = torch.empty(T, H, W, dtype=torch.int32, device=dev) if return_buffers else None
        depth = torch.empty(T, H, W, dtype=torch.float32, device=dev) if return_buffers else None
        if T == 0:
            return (rgb, face_id, depth) if return_buffers else rgb
        vertices = vertices.detach().contiguous().float()
        if isinstance(normals, str):
            if normals not in ('smooth', 'flat'):
                raise ValueError("normals must be 'smooth', 'flat' or a tensor")
            normals = self.layer.vertex_normals(vertices) if normals == 'smooth' else None
        if normals is not None:
            if not normals.is_cuda:
                raise _lib.EmposeError('MeshRenderer needs GPU tensors; there is no CPU fallback')
            if tuple(normals.shape) != (T, V, 3):
                raise ValueError('normals must be (T, V, 3)')
            normals = normals.detach().contiguous().float()
        colors, mode = self._colors(colors, T, V, dev)
        cam_R = torch.as_tensor(np.asarray(camera.R, dtype=np.float32), device=dev).contiguous()
        cam_t = torch.as_tensor(np.asarray(camera.t, dtype=np.float32), device=dev).contiguous()
        per_frame = cam_R.dim() == 3
        if tuple(cam_R.shape) != ((T, 3, 3) if per_frame else (3, 3)) or \
                tuple(cam_t.shape) != ((T, 3) if per_frame else (3,)):
            raise ValueError('camera R / t must be (3, 3) / (3,) or (T, 3, 3) / (T, 3)')
        faces_host, faces = self._faces(dev)

        d = _lib.RenderDesc()
        d.T, d.V, d.n_faces, d.H, d.W = T, V, int(faces_host.shape[0]), H, W
        d.vertices, d.faces, d.faces_host = _lib.dptr(vertices), _lib.dptr(faces), _lib.iptr(faces_host)
        d.normals, d.colors, d.color_mode = _lib.dptr(normals), _lib.dptr(colors), mode
        d.cam_R, d.cam_t, d.camera_per_frame = _lib.dptr(cam_R), _lib.dptr(cam_t), int(per_frame)
        d.fx, d.fy, d.cx, d.cy, d.near = camera.fx, camera.fy, camera.cx, camera.cy, camera.near
        d.light[:], d.ambient, d.background[:] = self.light, self.ambient, self.background
        d.slab_frames = self.slab_frames
        d.rgb, d.face_id, d.depth = _lib.dptr(rgb), _lib.dptr(face_id), _lib.dptr(depth)
        lib = _lib.lib()
        with torch.cuda.device(dev):
            ws_bytes = lib.empose_render_workspace_bytes(T, V, H, W)
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            _lib.check(lib.empose_render_meshes(_lib.C.byref(d), _lib.dptr(ws), ws_bytes, _lib.current_stream()))
        return (rgb, face_id, depth) if return_buffers else rgb

    def _colors(self, colors, T, V, dev):
        if colors is None:
            colors = self.color
        if not torch.is_tensor(colors):
            colors = torch.tensor(np.asarray(colors, dtype=np.float32), device=dev)
        if not colors.is_cuda:
            raise _lib.EmposeError('MeshRenderer needs GPU tensors; there is no CPU fallback')
        colors = colors.detach().contiguous().float()
        modes = {(3,): _lib.RENDER_COLOR_UNIFORM, (V, 3): _lib.RENDER_COLOR_VERTEX, (T, V, 3): _lib.RENDER_COLOR_FRAME}
        if tuple(colors.shape) not in modes:
            raise ValueError('colors must be an RGB triple, (V, 3) or (T, V, 3)')
        return colors, modes[tuple(colors.shape)]

    def render_bodies(self, poses_body, betas, poses_root=None, trans=None, normals='smooth', colors=None,
                      return_buffers=False, camera=None, overlays=None, hidden_alpha=0.0):
        """`layer.forward` and, for smooth shading, `layer.vertex_normals`, then `render`.  Without a camera anywhere,
        the first call fits one to its joints and keeps it.  `overlays`: as `render`, or a function of (vertices, joints)
        that returns them."""
        if not poses_body.is_cuda:
            raise _lib.EmposeError('MeshRenderer needs GPU tensors; there is no CPU fallback')
        with torch.no_grad():
            vertices, joints = self.layer(poses_body=poses_body, betas=betas, poses_root=poses_root, trans=trans)
        if camera is None and self.camera is None:
            self.camera = fit_camera(joints, self.width, self.height)
        if callable(overlays):
            overlays = overlays(vertices, joints)
        return self.render(vertices, normals=normals, colors=colors, return_buffers=return_buffers, camera=camera,
                           overlays=overlays, hidden_alpha=hidden_alpha)


def error_colors(vertices, vertices_hat, max_mm=100.0):
    """Per-vertex colours (..., V, 3) in [0, 1] from the distance between two meshes (..., V, 3) in metres: a ramp from
    blue-grey at 0 over yellow at max_mm / 2 to red at max_mm and beyond.  Plain torch, on the device of its inputs."""
    d = (vertices_hat - vertices).norm(dim=-1).mul(1000.0 / max_mm).clamp(0.0, 1.0).unsqueeze(-1)
    lo = torch.tensor([0.55, 0.65, 0.80], dtype=d.dtype, device=d.device)
    mid = torch.tensor([0.95, 0.85, 0.25], dtype=d.dtype, device=d.device)
    hi = torch.tensor([0.85, 0.10, 0.10], dtype=d.dtype, device=d.device)
    first = lo + (mid - lo) * (d * 2.0)
    second = mid + (hi - mid) * (d * 2.0 - 1.0)
    return torch.where(d < 0.5, first, second)
