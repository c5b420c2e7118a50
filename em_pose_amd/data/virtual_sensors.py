"""
Virtual sensors on a posed mesh (mirror of reference empose/data/virtual_sensors.py:41-96), HIP-backed.

`VirtualMarkerHelper(smpl_model).get_virtual_pos_and_rot(vertices (N,V,3), vertex_ids)` returns
`(positions (N,M,3), orientations (N,M,3,3), un-normalised vertex normals (N,M,3))` like the reference.  The index
tables (faces incident to the sensor vertices, helper vertex = first other vertex of the first incident face) are
derived once per `vertex_ids` tuple and cached on the device, as the reference caches them with `lru_cache`.
Inside the LGD loop this class is not used: `IterativeErrorFeedback` evaluates the sensors straight from the sub-mesh.

Like the reference's, the call is differentiable: when grad is enabled and `vertices` requires grad, the outputs carry a
`grad_fn` whose backward is empose_virtual_sensors_vjp (the vector-Jacobian product in HIP, recomputing the forward from
the saved vertices; single backward only).  Otherwise the call is the plain forward, no autograd node.
"""
import numpy as np
import torch
from torch.autograd.function import once_differentiable

from em_pose_amd import _lib
from em_pose_amd.bodymodels import tables as TB


class VirtualMarkerHelper(object):
    def __init__(self, smpl_model):
        self.smpl_model = smpl_model
        self._cache = {}

    def _topology(self, vertex_ids):
        faces = np.asarray(self.smpl_model.model['f'], dtype=np.int64)
        sub_faces, vf_sub, helpers = TB.sensor_topology(faces, list(vertex_ids))
        return sub_faces, vf_sub, helpers

    def get_vertex_helpers(self, vertex_ids):
        return self._topology(tuple(vertex_ids))[2].tolist()

    def get_sub_faces(self, vertex_ids):
        sub_faces, vf_sub, _ = self._topology(tuple(vertex_ids))
        return torch.from_numpy(sub_faces).long(), torch.from_numpy(vf_sub).long()

    def _tables(self, vertex_ids, device):
        key = (tuple(vertex_ids), str(device))
        if key not in self._cache:
            sub_faces, vf_sub, helpers = self._topology(tuple(vertex_ids))
            deg = (vf_sub >= 0).sum(axis=1).astype(np.int32)
            max_deg = int(deg.max())
            faces = np.zeros((len(vertex_ids), max_deg, 3), dtype=np.int32)
            for m in range(len(vertex_ids)):
                faces[m, :deg[m]] = sub_faces[vf_sub[m, :deg[m]]]
            t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(device)
            self._cache[key] = (t(np.asarray(vertex_ids)), t(helpers), t(deg), t(faces), max_deg)
        return self._cache[key]

    def _reverse_tables(self, vertex_ids, n_vertices, device):
        """The tables of empose_virtual_sensors_vjp (include/empose_hip.h), from the same topology as `_tables`:
        (sub_faces, face_ptr, face_sensors, vf_ptr, vf_corner, vs_ptr, vs_role, touched) on `device`, cached alike."""
        key = ('vjp', tuple(vertex_ids), int(n_vertices), str(device))
        if key not in self._cache:
            sub_faces, vf_sub, helpers = self._topology(tuple(vertex_ids))
            ids = np.asarray(vertex_ids, dtype=np.int64)
            if max(int(sub_faces.max()), int(ids.max()), int(helpers.max())) >= n_vertices:
                raise ValueError('vertex ids outside the {} mesh vertices'.format(n_vertices))
            m_of, f_of = np.nonzero(vf_sub >= 0)            # ascending m, then the row's own order
            f_of = vf_sub[m_of, f_of]
            order = np.argsort(f_of, kind='stable')         # per sub-face, its sensors in ascending m
            face_sensors = m_of[order]
            face_ptr = np.concatenate([[0], np.cumsum(np.bincount(f_of, minlength=len(sub_faces)))])
            u = sub_faces.reshape(-1)
            vf_corner = np.argsort(u, kind='stable')        # entries f * 3 + k, ascending per vertex
            vf_ptr = np.concatenate([[0], np.cumsum(np.bincount(u, minlength=n_vertices))])
            roles = np.stack([ids, helpers], axis=1).reshape(-1)
            vs_role = np.argsort(roles, kind='stable')      # entries m * 2 + role, ascending per vertex
            vs_ptr = np.concatenate([[0], np.cumsum(np.bincount(roles, minlength=n_vertices))])
            touched = np.nonzero(np.diff(vf_ptr) + np.diff(vs_ptr))[0]
            t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(device)
            self._cache[key] = tuple(t(a) for a in (sub_faces, face_ptr, face_sensors, vf_ptr, vf_corner, vs_ptr,
                                                    vs_role, touched))
        return self._cache[key]

    def _forward(self, v, vertex_ids):
        """empose_virtual_sensors_fwd on fp32 contiguous vertices."""
        n, nv = v.shape[0], v.shape[1]
        center, helper, deg, faces, max_deg = self._tables(vertex_ids, v.device)
        m = len(vertex_ids)
        pos = torch.empty(n, m, 3, dtype=torch.float32, device=v.device)
        ori = torch.empty(n, m, 3, 3, dtype=torch.float32, device=v.device)
        nor = torch.empty(n, m, 3, dtype=torch.float32, device=v.device)
        with torch.cuda.device(v.device):
            _lib.check(_lib.lib().empose_virtual_sensors_fwd(n, nv, _lib.dptr(v), m, max_deg, _lib.dptr(center),
                                                             _lib.dptr(helper), _lib.dptr(deg), _lib.dptr(faces),
                                                             _lib.dptr(pos), _lib.dptr(ori), _lib.dptr(nor),
                                                             _lib.current_stream()))
        return pos, ori, nor

    def _vjp(self, v, vertex_ids, d_pos, d_ori, d_nor):
        """empose_virtual_sensors_vjp: d_vertices (N, V, 3) fp32 for the cotangents (any but not all may be None)."""
        n, nv = v.shape[0], v.shape[1]
        center, helper, deg, faces, max_deg = self._tables(vertex_ids, v.device)
        rev = self._reverse_tables(vertex_ids, nv, v.device)
        m, lib = len(vertex_ids), _lib.lib()
        with torch.cuda.device(v.device):
            d_v = torch.empty(n, nv, 3, dtype=torch.float32, device=v.device)
            ws_bytes = lib.empose_virtual_sensors_vjp_workspace_bytes(n, m)
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=v.device)
            _lib.check(lib.empose_virtual_sensors_vjp(n, nv, _lib.dptr(v), m, max_deg, _lib.dptr(center),
                                                      _lib.dptr(helper), _lib.dptr(deg), _lib.dptr(faces),
                                                      rev[0].shape[0], *[_lib.dptr(a) for a in rev[:7]],
                                                      rev[7].shape[0], _lib.dptr(rev[7]), _lib.dptr(d_pos), _lib.dptr(d_ori), _lib.dptr(d_nor),
                                                      _lib.dptr(d_v), _lib.dptr(ws), ws_bytes, _lib.current_stream()))
        return d_v

    def get_virtual_pos_and_rot(self, vertices, vertex_ids):
        if not vertices.is_cuda:
            raise _lib.EmposeError('VirtualMarkerHelper needs GPU tensors; there is no CPU fallback')
        if torch.is_grad_enabled() and vertices.requires_grad:
            return _VirtualSensorsFn.apply(self, vertices, tuple(int(i) for i in vertex_ids))
        return self._forward(vertices.contiguous().float(), vertex_ids)

    def get_vertex_normals(self, vertices, vertex_ids):
        """Un-normalised vertex normals (mean of the incident faces' (v1-v0)x(v2-v0)) at `vertex_ids`, (N, M, 3)
        (reference virtual_sensors.py:77-83)."""
        return self.get_virtual_pos_and_rot(vertices, vertex_ids)[2]


class _VirtualSensorsFn(torch.autograd.Function):
    """`get_virtual_pos_and_rot` under autograd: the forward is the same launch as without grad (bit-identical outputs);
    the backward is empose_virtual_sensors_vjp, which recomputes the forward from the saved vertices (the only saved
    tensor).  Unused outputs get no cotangent and cost nothing."""

    @staticmethod
    def forward(ctx, helper, vertices, vertex_ids):
        ctx.helper, ctx.vertex_ids = helper, vertex_ids
        ctx.save_for_backward(vertices)
        ctx.set_materialize_grads(False)
        return helper._forward(vertices.contiguous().float(), vertex_ids)

    @staticmethod
    @once_differentiable
    def backward(ctx, d_pos, d_ori, d_nor):
        if d_pos is None and d_ori is None and d_nor is None:
            return None, None, None
        (vertices,) = ctx.saved_tensors
        f32 = lambda t: t.contiguous().float() if t is not None else None
        d_v = ctx.helper._vjp(f32(vertices), ctx.vertex_ids, f32(d_pos), f32(d_ori), f32(d_nor))
        return None, d_v.to(vertices.dtype).reshape(vertices.shape), None
