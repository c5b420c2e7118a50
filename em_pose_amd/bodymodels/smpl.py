"""
SMPL-H layer (mirror of reference empose/bodymodels/smpl.py:24-165) backed by the HIP full-mesh kernels.

`SMPLLayer(...)(poses_body, betas, poses_root=None, trans=None, normalize_root=False, window_size=None)` returns
`(vertices (N,V,3), joints (N,52,3))` exactly as the reference (`body.v`, `body.Jtr`, smpl.py:121-122): the 30 hand
joints have zero pose (smpl.py:99) and ride rigidly on the wrists.  Like the reference's, the layer is differentiable:
when grad is enabled and one of `poses_body`, `betas`, `poses_root`, `trans` requires grad, the outputs carry a
`grad_fn` whose backward is empose_mesh_vjp (the full-mesh vector-Jacobian product in HIP, recomputing the forward from
the saved poses and betas; single backward only).  Otherwise the call is the plain forward, no autograd node.
`fk_joints` stays forward-only.  `normalize_root=True` re-expresses the sequence in the frame of its first root
orientation and position (reference smpl.py:112-119) with the root-frame kernel (csrc/root_frame.hip) in front of the mesh
kernels; under autograd it is a node of its own in front of the mesh node, with empose_root_frame_vjp as its backward.
`sub_mesh(vertex_ids)` gives the same layer on the vertices the virtual sensors at `vertex_ids` read (`SubMeshLayer`).
`vertex_error(...)` is not in the reference: the per-frame sums of the per-vertex distance between two bodies and of its
square, from one fused kernel that writes neither mesh (csrc/mesh_err.hip; eval/mesh_metrics.py turns them into PVE).
Differences to the reference, on purpose:
  * `normalize_root=True`: the exponential map follows `rodrigues_convention`, the logarithm is accurate up to pi, and
    the backward is the derivative of the exact maps, finite at the first frame, where the reference's acos-based
    `so3_log_map` yields 0 * inf.  The translation keeps the shape (N, 3) for N = 1 too, where
    the reference's `.squeeze()` collapses it.
  * the LGD loop itself never calls this layer: `IterativeErrorFeedback` evaluates only the sensor sub-mesh.
  * `rodrigues_convention` ('smplx' | 'so3') selects how the axis-angle map guards the angle at zero; the fork that
    holds the reference's arithmetic is not available, so the choice is explicit (include/empose_hip.h).

Buffers live under `self.bm` with the names of the third-party `BodyModel` (`f, v_template, shapedirs, posedirs,
J_regressor, weights`) so that `state_dict` keys of released checkpoints (`smpl.bm.*`) match.
"""
import os

import numpy as np
import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from em_pose_amd import _lib
from em_pose_amd.bodymodels import tables as TB
from em_pose_amd.helpers.configuration import CONSTANTS as C


def load_model_npz(path_or_dict):
    """Read the arrays of an SMPL-H `model.npz` (or take an equivalent dict)."""
    src = path_or_dict if isinstance(path_or_dict, dict) else np.load(path_or_dict, allow_pickle=True)
    keys = ('v_template', 'f', 'shapedirs', 'posedirs', 'J_regressor', 'weights', 'kintree_table')
    model = {k: np.asarray(src[k]) for k in keys}
    if model['posedirs'].ndim != 3 or model['posedirs'].shape[2] != 459:
        raise ValueError('expected SMPL-H posedirs of shape (V,3,459), got {}'.format(model['posedirs'].shape))
    if model['J_regressor'].shape[0] != 52:
        raise ValueError('expected a 52-joint SMPL-H model')
    return model


class _BodyModelBuffers(nn.Module):
    """Holds the model arrays under the third-party module's buffer names and layouts."""

    def __init__(self, model, num_betas):
        super(_BodyModelBuffers, self).__init__()
        t = lambda a: torch.from_numpy(np.array(a, dtype=np.float32))     # own memory: `model` must not alias buffers
        self.register_buffer('f', torch.from_numpy(np.array(model['f'], dtype=np.int64)))
        self.register_buffer('v_template', t(model['v_template'])[None])
        self.register_buffer('shapedirs', t(model['shapedirs'][:, :, :num_betas]))
        pd = np.asarray(model['posedirs'], dtype=np.float32)
        self.register_buffer('posedirs', t(pd.reshape(pd.shape[0] * 3, -1).T).contiguous())
        self.register_buffer('J_regressor', t(model['J_regressor']))
        self.register_buffer('weights', t(model['weights']))
        # The fork registers its default pose/shape as nn.Parameters (169 values, reference README.md:228).
        self.trans = nn.Parameter(torch.zeros(1, 3))
        self.root_orient = nn.Parameter(torch.zeros(1, 3))
        self.pose_body = nn.Parameter(torch.zeros(1, 63))
        self.pose_hand = nn.Parameter(torch.zeros(1, 90))
        self.betas = nn.Parameter(torch.zeros(1, num_betas))


class SMPLLayer(nn.Module):
    def __init__(self, smpl_path, device=None, vposer_path=None, rodrigues_convention='smplx', arithmetic='f32'):
        super(SMPLLayer, self).__init__()
        if vposer_path is not None:
            raise NotImplementedError('VPoser is not part of the LGD path')
        if rodrigues_convention not in _lib.RODRIGUES:
            raise ValueError('rodrigues_convention must be one of {}'.format(sorted(_lib.RODRIGUES)))
        self.rodrigues_convention = rodrigues_convention
        if arithmetic not in ('f32', 'bf16x3'):
            raise ValueError("arithmetic must be 'f32' (exact fp32 matrix cores, the default) or 'bf16x3'")
        self.arithmetic = arithmetic   # 'bf16x3': blend-shape contraction in split bf16 (explicit opt-in, not the reference's)
        self.num_betas = C.N_SHAPE_PARAMS
        self.model = load_model_npz(smpl_path)
        self.bm = _BodyModelBuffers(self.model, self.num_betas)
        self._faces = None
        self._vertex_faces = None
        self._mesh = None  # (handle, device index)
        self.tables_version = 0   # bumped when the arrays change: holders of tables derived from `self.model` rebuild
        # A released `model.pth` carries the body model as `smpl.bm.*` buffers and the reference's network computes with
        # THOSE after `load_state_dict` (reference eval/helpers.py:131-137), whatever `model.npz` was read at construction.
        self.register_load_state_dict_post_hook(lambda module, incompatible: module._adopt_buffers())

    def _adopt_buffers(self):
        """Make the kernel tables follow the `bm` buffers (after load_state_dict).  No-op when they already agree."""
        bm, m, nb = self.bm, self.model, self.num_betas
        V = bm.v_template.shape[1]
        new = {'v_template': bm.v_template[0], 'shapedirs': bm.shapedirs, 'J_regressor': bm.J_regressor,
               'weights': bm.weights, 'posedirs': bm.posedirs.t().reshape(V, 3, -1), 'f': bm.f}
        new = {k: v.detach().cpu().numpy() for k, v in new.items()}
        old = {k: (np.asarray(m[k])[:, :, :nb] if k == 'shapedirs' else np.asarray(m[k])) for k in new}
        if all(old[k].shape == new[k].shape and np.array_equal(old[k].astype(new[k].dtype), new[k]) for k in new):
            return
        model = dict(m)
        model.update(new)
        self.model = model
        self._faces = self._vertex_faces = None
        self._release()
        self.tables_version += 1

    # -- topology ----------------------------------------------------------------------------------------------
    @property
    def n_vertices(self):
        return self.model['v_template'].shape[0]

    @property
    def faces(self):
        if self._faces is None:
            self._faces = self.bm.f.to(dtype=torch.int32)
        return self._faces

    def vertex_faces(self, n_vertices):
        if self._vertex_faces is None:
            vf = TB.vertex_faces_table(self.model['f'], n_vertices)
            self._vertex_faces = torch.from_numpy(vf).to(dtype=torch.long, device=self.bm.f.device)
        return self._vertex_faces

    def vertex_normals(self, vertices, output_vertex_ids=None):
        """Un-normalised vertex normals of posed meshes (N, V, 3) -> (N, V, 3), or (N, len(ids), 3) for the given vertex
        ids (reference smpl.py:69-79)."""
        from em_pose_amd.data.virtual_sensors import VirtualMarkerHelper
        if getattr(self, '_normal_helper', None) is None:
            self._normal_helper = VirtualMarkerHelper(self)
        ids = list(range(vertices.shape[1])) if output_vertex_ids is None else [int(i) for i in output_vertex_ids]
        return self._normal_helper.get_vertex_normals(vertices, ids)

    # -- HIP full-mesh evaluation -----------------------------------------------------------------------------
    @property
    def n_joints(self):
        return int(np.asarray(self.model['J_regressor']).shape[0])

    def _mesh_handle(self, device):
        key = (device.index, self.rodrigues_convention, self.arithmetic)
        if self._mesh is not None and self._mesh[1] == key:
            return self._mesh[0]
        self._release()
        tab = self._mesh_tables()
        desc = _lib.MeshDesc()
        desc.n_vertices, desc.j_off, desc.ncp, desc.kb = tab['n_vertices'], tab['j_off'], tab['ncp'], tab['kb']
        desc.wc, desc.skin_idx = _lib.fptr(tab['wc']), _lib.iptr(tab['skin_idx'])
        desc.skin_w, desc.parents = _lib.fptr(tab['skin_w']), _lib.iptr(tab['parents'])
        desc.n_joints, desc.rodrigues = tab['n_joints'], _lib.RODRIGUES[self.rodrigues_convention]
        desc.with_bf16x3 = int(self.arithmetic == 'bf16x3')
        handle = _lib.C.c_void_p()
        with torch.cuda.device(device):
            _lib.check(_lib.lib().empose_mesh_create(_lib.C.byref(desc), _lib.C.byref(handle)))
        self._mesh = (handle, key)
        return handle

    def _mesh_tables(self):
        return TB.build_full_mesh_tables(self.model, self.num_betas)

    def sub_mesh(self, vertex_ids):
        """The layer restricted to what the virtual sensors at `vertex_ids` read of the mesh (`SubMeshLayer`), cached
        per id tuple."""
        key = tuple(int(v) for v in vertex_ids)
        cache = self.__dict__.setdefault('_sub_meshes', {})
        if key not in cache:
            cache[key] = SubMeshLayer(self, key)
        return cache[key]

    def _release(self):
        if self._mesh is not None:
            _lib.lib().empose_mesh_destroy(self._mesh[0])
            self._mesh = None

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass

    def _fk(self, poses_body, betas, poses_root=None, trans=None, normalize_root=False):
        assert poses_body.shape[1] >= C.N_JOINTS * 3
        if not poses_body.is_cuda:
            raise _lib.EmposeError('SMPLLayer needs GPU tensors; there is no CPU fallback')
        if torch.is_grad_enabled() and any(t is not None and t.requires_grad
                                           for t in (poses_body, betas, poses_root, trans)):
            if normalize_root:
                if poses_root is None:
                    poses_root = torch.zeros(poses_body.shape[0], 3, dtype=torch.float32, device=poses_body.device)
                poses_root, trans = _RootFrame.apply(_lib.RODRIGUES[self.rodrigues_convention], poses_root, trans)
            return _MeshFK.apply(self, poses_body, betas, poses_root, trans)
        poses, betas, trans = self._pack(poses_body, betas, poses_root, trans)
        if normalize_root:
            # one segment of N frames, on the packed rows in place of their first three columns
            root, trans = root_frame_fwd(poses, trans, poses.shape[0], _lib.RODRIGUES[self.rodrigues_convention])
            poses[:, :3] = root
        return self._fk_packed(poses, betas, trans)

    def _pack(self, poses_body, betas, poses_root, trans):
        """The kernel's inputs: poses [N][66] (root first), betas [N][10], trans [N][3] or None."""
        n, dev = poses_body.shape[0], poses_body.device
        if poses_root is None:
            poses_root = torch.zeros(n, 3, dtype=torch.float32, device=dev)
        if betas.dim() == 1 or betas.shape[0] == 1:
            betas = betas.reshape(1, -1).repeat(n, 1)
        betas = betas[:, :self.num_betas].contiguous().float()
        poses = torch.cat([poses_root.float(), poses_body[:, :C.N_JOINTS * 3].float()], dim=1).contiguous()
        trans = trans.contiguous().float() if trans is not None else None
        return poses, betas, trans

    def _fk_packed(self, poses, betas, trans):
        n, dev = poses.shape[0], poses.device
        lib = _lib.lib()
        with torch.cuda.device(dev):
            handle = self._mesh_handle(dev)
            vertices = torch.empty(n, self.n_vertices, 3, dtype=torch.float32, device=dev)
            joints = torch.empty(n, self.n_joints, 3, dtype=torch.float32, device=dev)
            ws_bytes = lib.empose_mesh_workspace_bytes(handle, n)
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            fwd = lib.empose_mesh_vertices_fwd_bf16x3 if self.arithmetic == 'bf16x3' else lib.empose_mesh_vertices_fwd
            _lib.check(fwd(handle, n, _lib.dptr(poses), _lib.dptr(betas), _lib.dptr(trans),
                                                    _lib.dptr(vertices), _lib.dptr(joints), _lib.dptr(ws), ws_bytes,
                                                    _lib.current_stream()))
        return vertices, joints

    def _vjp_packed(self, poses, betas, d_vertices, d_joints, want_trans):
        """empose_mesh_vjp: (g_poses [N][66], g_betas [N][10], g_trans [N][3] or None) for the cotangents (either may
        be None)."""
        n, dev = poses.shape[0], poses.device
        lib = _lib.lib()
        with torch.cuda.device(dev):
            handle = self._mesh_handle(dev)
            g_poses = torch.empty(n, 66, dtype=torch.float32, device=dev)
            g_betas = torch.empty(n, self.num_betas, dtype=torch.float32, device=dev)
            g_trans = torch.empty(n, 3, dtype=torch.float32, device=dev) if want_trans else None
            ws_bytes = lib.empose_mesh_vjp_workspace_bytes(handle, n)
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            _lib.check(lib.empose_mesh_vjp(handle, n, _lib.dptr(poses), _lib.dptr(betas), _lib.dptr(d_vertices),
                                           _lib.dptr(d_joints), _lib.dptr(g_poses), _lib.dptr(g_betas),
                                           _lib.dptr(g_trans), _lib.dptr(ws), ws_bytes, _lib.current_stream()))
        return g_poses, g_betas, g_trans

    def fk_joints(self, poses_body, betas, poses_root=None, trans=None):
        """The 22 posed body joints only (no vertices): forward kinematics for the metrics, (N,22,3) contiguous
        (= `fk(...)[1][:, :22]`, what reference eval/metrics.py:223-228 keeps)."""
        if not poses_body.is_cuda:
            raise _lib.EmposeError('SMPLLayer needs GPU tensors; there is no CPU fallback')
        n, dev = poses_body.shape[0], poses_body.device
        if poses_root is None:
            poses_root = torch.zeros(n, 3, dtype=torch.float32, device=dev)
        if betas.dim() == 1 or betas.shape[0] == 1:
            betas = betas.reshape(1, -1).repeat(n, 1)
        betas = betas[:, :self.num_betas].contiguous().float()
        poses = torch.cat([poses_root.float(), poses_body[:, :C.N_JOINTS * 3].float()], dim=1).contiguous()
        trans = trans.contiguous().float() if trans is not None else None
        lib = _lib.lib()
        with torch.cuda.device(dev):
            handle = self._mesh_handle(dev)
            joints = torch.empty(n, self.n_joints, 3, dtype=torch.float32, device=dev)
            ws_bytes = lib.empose_mesh_workspace_bytes(handle, n)
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            _lib.check(lib.empose_mesh_joints_fwd(handle, n, _lib.dptr(poses), _lib.dptr(betas), _lib.dptr(trans),
                                                  _lib.dptr(joints), _lib.dptr(ws), ws_bytes, _lib.current_stream()))
        return joints[:, :C.N_JOINTS + 1].contiguous()

    def vertex_error(self, poses_body, betas, poses_body_hat, betas_hat, poses_root=None, poses_root_hat=None,
                     trans=None, trans_hat=None, procrustes=False):
        """Per-vertex error between the body (poses_body, betas, poses_root, trans) and the body (`*_hat`), N frames
        each, without writing either mesh (empose_mesh_vertex_error, csrc/mesh_err.hip): `sums` (N, 2) float64 on the
        device, per frame the sum over this layer's vertices of |v - v_hat| (metres) and of |v - v_hat|^2; a frame's
        mean per-vertex error is `sums[:, 0] / n_vertices`.  The inputs are packed as `forward` packs them (betas
        broadcast, the first 63 body columns, `num_betas` shape coefficients).  No autograd: the inputs are detached and
        the result never carries a `grad_fn`.  fp32 on the fp32 matrix cores whatever `arithmetic` the layer has;
        deterministic, and a frame's row depends on that frame alone.
        `procrustes=True`: `sums` (N, 4), the same two columns and then the same two sums after the similarity transform
        (rotation, scale, translation; the convention of PA-MPJPE) that best maps the `*_hat` vertices onto the others,
        PA-PVE -- two sweeps over both bodies around a per-frame 3 x 3 SVD in float64, still without a mesh
        (empose_mesh_vertex_error_pa)."""
        if not (poses_body.is_cuda and poses_body_hat.is_cuda):
            raise _lib.EmposeError('SMPLLayer needs GPU tensors; there is no CPU fallback')
        if poses_body_hat.shape[0] != poses_body.shape[0]:
            raise ValueError('both bodies need the same number of frames')
        det = lambda t: t.detach() if t is not None else None
        pa, ba, ta = self._pack(det(poses_body), det(betas), det(poses_root), det(trans))
        pb, bb, tb = self._pack(det(poses_body_hat), det(betas_hat), det(poses_root_hat), det(trans_hat))
        n, dev = pa.shape[0], pa.device
        lib = _lib.lib()
        with torch.cuda.device(dev):
            handle = self._mesh_handle(dev)
            sums = torch.empty(n, 4 if procrustes else 2, dtype=torch.float64, device=dev)
            ws_query = lib.empose_mesh_vertex_error_pa_workspace_bytes if procrustes else \
                lib.empose_mesh_vertex_error_workspace_bytes
            entry = lib.empose_mesh_vertex_error_pa if procrustes else lib.empose_mesh_vertex_error
            ws_bytes = ws_query(handle, n)
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            _lib.check(entry(handle, n, _lib.dptr(pa), _lib.dptr(ba), _lib.dptr(ta), _lib.dptr(pb), _lib.dptr(bb),
                             _lib.dptr(tb), _lib.dptr(sums), _lib.dptr(ws), ws_bytes, _lib.current_stream()))
        return sums

    def surface_faces(self, device):
        """The face table as `eval.surface_metrics.Faces` (host and device copy), cached per device and table version."""
        from em_pose_amd.eval.surface_metrics import Faces
        key = (self.tables_version, str(device))
        cache = self.__dict__.setdefault('_surface_faces', {})
        if key not in cache:
            for stale in [k for k in cache if k[0] != self.tables_version]:
                del cache[stale]
            cache[key] = Faces(np.asarray(self.model['f']), device)
        return cache[key]

    def surface_distance(self, points, poses_body, betas, poses_root=None, trans=None, mask=None, inside=True, slab=1024):
        """The distance of `points` (N, Q, 3) or (N, Q * 3), given in the frame of the posed body, to the body's surface,
        and whether they lie inside it (eval/surface_metrics.py, csrc/surface_query.hip): `SurfaceResult(dist (N, Q), face,
        bary, closest, inside)` on the device, `mask` (N, Q) as in `closest_point_on_mesh`.  The mesh is evaluated with
        `forward` in slabs of at most `slab` frames and each slab is queried at once, so the memory beyond the inputs and
        the outputs does not grow with N; the results equal the one-shot query of the whole mesh bit for bit.  The body
        inputs are packed as `forward` packs them.  No autograd."""
        from em_pose_amd.eval.surface_metrics import surface_distance
        return surface_distance(self, points, poses_body, betas, poses_root=poses_root, trans=trans, mask=mask,
                                inside=inside, slab=slab)

    def fk(self, poses_body, betas, poses_root=None, trans=None, normalize_root=False, window_size=None):
        # The reference slices long inputs into windows to bound memory (smpl.py:124-144); the HIP entry point already
        # processes slabs of 2048 frames internally, so `window_size` only has to be accepted.
        if window_size is not None and normalize_root:
            raise ValueError('Are you sure you want to use root normalization with windowed evaluation?')
        return self._fk(poses_body, betas, poses_root, trans, normalize_root)

    def forward(self, *args, **kwargs):
        return self.fk(*args, **kwargs)


class SubMeshLayer(object):
    """`SMPLLayer.sub_mesh(vertex_ids)`: the parent layer on the sensor sub-mesh -- the sensor vertices, their helper
    vertices and the corners of their incident faces (`needed`, ascending original ids; 84 of 6890 for the 12 sensors).
    `fk` / `forward` / `fk_joints` as the parent's, with `vertices` (N, len(needed), 3) and the same `joints` (N, 52, 3):
    the same kernels on a mesh handle of its own whose tables are the gathered rows of the parent's
    (bodymodels/tables.py build_sub_mesh_tables), so the full mesh is never written and, under autograd, its backward
    (empose_mesh_vjp on this handle) never sees a full-mesh cotangent.  The Rodrigues convention and `arithmetic` are the
    parent's; the tables are rebuilt when the parent's `tables_version` changes.  `model['f']`, `faces` and `n_vertices`
    describe the restricted mesh in local numbering, which is what `VirtualMarkerHelper` reads: use it with
    `local_ids(vertex_ids)`."""

    def __init__(self, parent, vertex_ids):
        self.parent, self.vertex_ids = parent, tuple(vertex_ids)
        self.num_betas = parent.num_betas
        self._mesh = None
        self._version = None
        self._sync()

    def _sync(self):
        if self._version != self.parent.tables_version:
            self._release()
            self._tables = TB.build_sub_mesh_tables(self.parent.model, self.vertex_ids, self.num_betas)
            self._model = {'f': self._tables['faces']}
            self._faces = None
            self._version = self.parent.tables_version

    rodrigues_convention = property(lambda self: self.parent.rodrigues_convention)
    arithmetic = property(lambda self: self.parent.arithmetic)

    @property
    def needed(self):
        """Original ids of the sub-mesh vertices, ascending (numpy int64)."""
        self._sync()
        return self._tables['needed']

    @property
    def model(self):
        self._sync()
        return self._model

    @property
    def n_vertices(self):
        return len(self.needed)

    @property
    def n_joints(self):
        self._sync()
        return self._tables['n_joints']

    @property
    def faces(self):
        self._sync()
        if self._faces is None:
            self._faces = torch.from_numpy(self._tables['faces']).to(dtype=torch.int32, device=self.parent.bm.f.device)
        return self._faces

    def local_ids(self, vertex_ids):
        """Positions in `needed` of original vertex ids; ValueError for one the sub-mesh does not hold."""
        ids = np.asarray([int(v) for v in vertex_ids], dtype=np.int64)
        loc = np.minimum(np.searchsorted(self.needed, ids), len(self.needed) - 1)
        if not np.array_equal(self.needed[loc], ids):
            raise ValueError('vertices {} are not part of the sub-mesh'.format(ids[self.needed[loc] != ids].tolist()))
        return [int(i) for i in loc]

    def _mesh_tables(self):
        return self._tables

    def _mesh_handle(self, device):
        self._sync()
        return SMPLLayer._mesh_handle(self, device)

    # the evaluation itself is the parent class's, on this object's handle and sizes
    _release, __del__ = SMPLLayer._release, SMPLLayer.__del__
    _fk, _pack, _fk_packed, _vjp_packed = SMPLLayer._fk, SMPLLayer._pack, SMPLLayer._fk_packed, SMPLLayer._vjp_packed
    fk_joints, fk = SMPLLayer.fk_joints, SMPLLayer.fk
    vertex_error = SMPLLayer.vertex_error   # the error over the sub-mesh vertices (`needed`), on this object's handle

    def forward(self, *args, **kwargs):
        return self.fk(*args, **kwargs)

    __call__ = forward


def root_frame_fwd(rows, trans, seg_len, rodrigues, flags=None):
    """empose_root_frame_fwd on `rows` (T, ld) float32 whose first three columns are the root axis-angle, in segments of
    `seg_len` frames: (root_out (T, 3), trans_out (T, 3) or None).  `trans` (T, 3) or None is rotated into the first
    frame and the first translation subtracted, unless `flags` says otherwise."""
    if flags is None:
        flags = (_lib.ROOT_FRAME_ROTATE | _lib.ROOT_FRAME_SUBTRACT) if trans is not None else 0
    n, dev = rows.shape[0], rows.device
    with torch.cuda.device(dev):
        root_out = torch.empty(n, 3, dtype=torch.float32, device=dev)
        trans_out = torch.empty(n, 3, dtype=torch.float32, device=dev) if flags else None
        _lib.check(_lib.lib().empose_root_frame_fwd(n, seg_len, rodrigues, _lib.dptr(rows), rows.shape[1],
                                                    _lib.dptr(trans) if flags else None, _lib.dptr(root_out),
                                                    _lib.dptr(trans_out), flags, _lib.current_stream()))
    return root_out, trans_out


class _RootFrame(torch.autograd.Function):
    """`normalize_root=True` under autograd, one segment of N frames: (poses_root, trans) -> their normalised versions;
    the backward is empose_root_frame_vjp on the saved inputs (single backward only)."""

    @staticmethod
    def forward(ctx, rodrigues, poses_root, trans):
        root = poses_root.contiguous().float()
        tr = trans.contiguous().float() if trans is not None else None
        ctx.rodrigues = rodrigues
        ctx.root_dtype = poses_root.dtype
        ctx.trans_dtype = trans.dtype if trans is not None else None
        ctx.save_for_backward(root, tr)
        ctx.set_materialize_grads(False)
        root_out, trans_out = root_frame_fwd(root, tr, root.shape[0], rodrigues)
        return root_out, trans_out

    @staticmethod
    @once_differentiable
    def backward(ctx, d_root, d_trans):
        if d_root is None and d_trans is None:
            return None, None, None
        root, tr = ctx.saved_tensors
        n, dev = root.shape[0], root.device
        flags = (_lib.ROOT_FRAME_ROTATE | _lib.ROOT_FRAME_SUBTRACT) if tr is not None else 0
        d_root = d_root.contiguous().float() if d_root is not None else None
        d_trans = d_trans.contiguous().float() if d_trans is not None and tr is not None else None
        lib = _lib.lib()
        with torch.cuda.device(dev):
            g_root = torch.empty(n, 3, dtype=torch.float32, device=dev)
            g_trans = torch.empty(n, 3, dtype=torch.float32, device=dev) if d_trans is not None else None
            ws_bytes = lib.empose_root_frame_vjp_workspace_bytes(n, n)
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            _lib.check(lib.empose_root_frame_vjp(n, n, ctx.rodrigues, _lib.dptr(root), 3, _lib.dptr(tr),
                                                 _lib.dptr(d_root), _lib.dptr(d_trans), _lib.dptr(g_root),
                                                 _lib.dptr(g_trans), flags, _lib.dptr(ws), ws_bytes,
                                                 _lib.current_stream()))
        g_root = g_root.to(ctx.root_dtype) if ctx.needs_input_grad[1] else None
        if tr is not None and ctx.needs_input_grad[2]:
            g_trans = g_trans.to(ctx.trans_dtype) if g_trans is not None else torch.zeros_like(tr, dtype=ctx.trans_dtype)
        else:
            g_trans = None
        return None, g_root, g_trans


class _MeshFK(torch.autograd.Function):
    """`SMPLLayer._fk` under autograd: the forward runs the HIP kernels as without grad; the backward is
    empose_mesh_vjp, which recomputes what it needs from the packed poses and betas (the only saved tensors)."""

    @staticmethod
    def forward(ctx, layer, poses_body, betas, poses_root, trans):
        poses, betas_p, trans_p = layer._pack(poses_body, betas, poses_root, trans)
        ctx.layer = layer
        ctx.save_for_backward(poses, betas_p)
        ctx.body_shape, ctx.body_dtype = tuple(poses_body.shape), poses_body.dtype
        ctx.betas_shape, ctx.betas_dtype = tuple(betas.shape), betas.dtype
        ctx.betas_broadcast = betas.dim() == 1 or betas.shape[0] == 1
        ctx.has_root, ctx.has_trans = poses_root is not None, trans is not None
        ctx.root_dtype = poses_root.dtype if poses_root is not None else None
        ctx.trans_dtype = trans.dtype if trans is not None else None
        ctx.set_materialize_grads(False)
        return layer._fk_packed(poses, betas_p, trans_p)

    @staticmethod
    @once_differentiable
    def backward(ctx, d_vertices, d_joints):
        if d_vertices is None and d_joints is None:
            return None, None, None, None, None
        poses, betas = ctx.saved_tensors
        dv = d_vertices.contiguous().float() if d_vertices is not None else None
        dj = d_joints.contiguous().float() if d_joints is not None else None
        g_poses, g_betas, g_trans = ctx.layer._vjp_packed(poses, betas, dv, dj, ctx.has_trans)
        nb = g_betas.shape[1]
        g_body = g_root = g_b = g_t = None
        if ctx.needs_input_grad[1]:
            g_body = torch.zeros(ctx.body_shape, dtype=ctx.body_dtype, device=poses.device)
            g_body[:, :C.N_JOINTS * 3] = g_poses[:, 3:]
        if ctx.needs_input_grad[2]:
            g_b = torch.zeros(ctx.betas_shape, dtype=ctx.betas_dtype, device=poses.device)
            if ctx.betas_broadcast:   # `_pack` repeated one row for every frame
                g_b.view(-1)[:nb] = g_betas.sum(dim=0)
            else:
                g_b[:, :nb] = g_betas
        if ctx.needs_input_grad[3] and ctx.has_root:
            g_root = g_poses[:, :3].to(ctx.root_dtype)
        if ctx.needs_input_grad[4] and ctx.has_trans:
            g_t = g_trans.to(ctx.trans_dtype)
        return None, g_body, g_b, g_root, g_t


def create_default_smpl_model(device=None, vposer_path=None):
    """Loads `$SMPL_MODELS/smplh_amass/neutral/model.npz` (reference smpl.py:24-28)."""
    device = C.DEVICE if device is None else device
    layer = SMPLLayer(os.path.join(C.SMPL_MODELS_DIR, 'smplh_amass/neutral/model.npz'), vposer_path=vposer_path)
    return layer.to(device=device, dtype=torch.float32)
