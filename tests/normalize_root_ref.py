"""Float64 restatements of the root normalisation (reference bodymodels/smpl.py:112-119) shared by the
test_normalize_root*.py files, and thin callers of the two C entry points.  Not a test module."""
import ctypes as C
import os

import numpy as np
import torch

from oracle import torch_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
ROTATE, SUBTRACT = 1, 2   # EMPOSE_ROOT_FRAME_* (include/empose_hip.h)


def load_fixture():
    z = np.load(os.path.join(GOLDEN, 'normalize_root.npz'))
    out = {}
    for k in z.files:
        g, rest = k.split('/', 1)
        out.setdefault(g, {})[rest] = z[k]
    return out


# ---- forward, numpy float64 ------------------------------------------------------------------------------------------
def exp64(r, conv):
    """The guarded axis-angle map of the given convention in float64 (oracle.torch_ref.rodrigues), (n,3) -> (n,3,3)."""
    return R.rodrigues(torch.from_numpy(np.asarray(r, dtype=np.float64)), conv).numpy()


def log64(Rm):
    """Matrix logarithm (n,3,3) -> (n,3), accurate over [0, pi]: angle from atan2(|w| / 2, (tr - 1) / 2), w = vee(R - R^T);
    series of angle / sin(angle) below 1e-4; above pi - 0.1 the axis from the symmetric part, its sign from w."""
    Rm = np.asarray(Rm, dtype=np.float64)
    w = np.stack([Rm[:, 2, 1] - Rm[:, 1, 2], Rm[:, 0, 2] - Rm[:, 2, 0], Rm[:, 1, 0] - Rm[:, 0, 1]], -1)
    sn = 0.5 * np.linalg.norm(w, axis=1)
    cs = 0.5 * (np.trace(Rm, axis1=1, axis2=2) - 1.0)
    th = np.arctan2(sn, cs)
    k = np.where(th < 1e-4, 0.5 * (1 + th ** 2 / 6), 0.5 * th / np.where(sn > 0, sn, 1.0))
    out = w * k[:, None]
    near = th > np.pi - 0.1
    if near.any():
        B = 0.5 * (Rm[near] + np.swapaxes(Rm[near], 1, 2))
        c = cs[near]
        j = np.argmax(np.diagonal(B, axis1=1, axis2=2), axis=1)
        col = np.take_along_axis(B, j[:, None, None], axis=2)[:, :, 0]
        col[np.arange(len(j)), j] -= c
        n = col / np.linalg.norm(col, axis=1, keepdims=True)
        n *= np.where((n * w[near]).sum(1, keepdims=True) < 0, -1.0, 1.0)
        out[near] = n * th[near][:, None]
    return out


def normalize64(root, trans, seg_len, conv, flags=ROTATE | SUBTRACT):
    """(root_out, trans_out, Rn) in float64 for float32 inputs: segments of seg_len rows, the reference's order."""
    root = np.asarray(root, dtype=np.float64)
    Rm = exp64(root, conv).reshape(-1, seg_len, 3, 3)
    R0t = np.swapaxes(Rm[:, :1], -1, -2)
    Rn = (R0t @ Rm).reshape(-1, 3, 3)
    out = log64(Rn).reshape(-1, seg_len, 3)
    out[:, 0] = 0.0
    t = None
    if trans is not None and flags:
        t = np.asarray(trans, dtype=np.float64).reshape(-1, seg_len, 3)
        if flags & ROTATE:
            t = (R0t @ t[..., None])[..., 0]
        if flags & SUBTRACT:
            t = t - t[:, :1]
        t = t.reshape(-1, 3)
    return out.reshape(-1, 3), t, Rn


# ---- differentiable, torch (float64 truth, float32 control): exact maps through unit quaternions ---------------------
def _quat(r):
    tiny = torch.finfo(r.dtype).tiny
    th = torch.sqrt((r * r).sum(-1, keepdim=True) + tiny)
    return torch.cat([torch.cos(0.5 * th), r * (torch.sin(0.5 * th) / th)], dim=-1)


def _qmul(a, b):
    aw, av, bw, bv = a[..., :1], a[..., 1:], b[..., :1], b[..., 1:]
    return torch.cat([aw * bw - (av * bv).sum(-1, keepdim=True), aw * bv + bw * av + torch.cross(av, bv, dim=-1)], dim=-1)


def _qrot(q, x):
    """Rotate x by the unit quaternion q."""
    w, v = q[..., :1], q[..., 1:]
    t = 2.0 * torch.cross(v, x, dim=-1)
    return x + w * t + torch.cross(v, t, dim=-1)


def normalize_torch(root, trans, seg_len, flags=ROTATE | SUBTRACT):
    """The normalisation with the exact exponential and logarithm, well conditioned everywhere on [0, pi) including
    Rn = I: q_n = conj(q_0) q_t, log = 2 atan2(|v|, w) v / |v| with |v| = sqrt(v.v + tiny)."""
    n = root.shape[0]
    q = _quat(root).reshape(n // seg_len, seg_len, 4)
    q0c = q[:, :1] * torch.tensor([1.0, -1.0, -1.0, -1.0], dtype=root.dtype)
    qn = _qmul(q0c.expand_as(q), q)
    qn = qn * torch.where(qn[..., :1] < 0, -1.0, 1.0).to(root.dtype)
    v = qn[..., 1:]
    s = torch.sqrt((v * v).sum(-1, keepdim=True) + torch.finfo(root.dtype).tiny)
    out = (v * (2.0 * torch.atan2(s, qn[..., :1]) / s)).reshape(n, 3)
    t = None
    if trans is not None and flags:
        t = trans.reshape(n // seg_len, seg_len, 3)
        if flags & ROTATE:
            t = _qrot(q0c.expand_as(q), t)
        if flags & SUBTRACT:
            t = t - t[:, :1]
        t = t.reshape(n, 3)
    return out, t


def vjp_torch(dtype, root, trans, d_root, d_trans, seg_len, flags):
    """(g_root, g_trans or None) as float64 numpy: autograd through normalize_torch in `dtype` on the CPU."""
    t = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64)).to(dtype)
    r = t(root).requires_grad_(True)
    x = t(trans).requires_grad_(True) if trans is not None and flags else None
    out, tout = normalize_torch(r, x, seg_len, flags)
    loss = (out * 0).sum()
    if d_root is not None:
        loss = loss + (out * t(d_root)).sum()
    if d_trans is not None:
        loss = loss + (tout * t(d_trans)).sum()
    loss.backward()
    g = lambda a: a.grad.numpy().astype(np.float64) if a is not None and a.grad is not None else None
    return g(r), g(x)


def check_rows(name, got, g64, g32):
    """The bar of tests/test_mesh_vjp.py for cotangent comparisons, same constants: per row, the largest error is at most
    1e-4 x the row's largest |g64|, and at most 4 x the error of the float32 CPU control plus 1e-7 x the row's scale."""
    scale = np.abs(g64).max(axis=1)
    err = np.abs(got - g64).max(axis=1)
    err32 = np.abs(g32 - g64).max(axis=1)
    bad = np.nonzero((err > 1e-4 * scale) | (err > 4 * err32 + 1e-7 * scale))[0]
    assert bad.size == 0, '{}: rows {} err {} scale {} control {}'.format(
        name, bad[:8], err[bad[:8]], scale[bad[:8]], err32[bad[:8]])


# ---- the C entry points ----------------------------------------------------------------------------------------------
def run_fwd(rows, trans, seg_len, conv, flags):
    """rows (T, ld) and trans (T, 3) or None: CUDA float32 tensors -> (root_out, trans_out or None)."""
    from em_pose_amd import _lib
    T = rows.shape[0]
    root_out = torch.empty(T, 3, dtype=torch.float32, device=rows.device)
    trans_out = torch.empty(T, 3, dtype=torch.float32, device=rows.device) if flags else None
    _lib.check(_lib.lib().empose_root_frame_fwd(T, seg_len, _lib.RODRIGUES[conv], _lib.dptr(rows), rows.shape[1],
                                                _lib.dptr(trans), _lib.dptr(root_out), _lib.dptr(trans_out), flags,
                                                _lib.current_stream()))
    return root_out, trans_out


def run_vjp(rows, trans, d_root, d_trans, seg_len, conv, flags):
    from em_pose_amd import _lib
    lib = _lib.lib()
    T = rows.shape[0]
    g_root = torch.full((T, 3), float('nan'), dtype=torch.float32, device=rows.device)
    g_trans = torch.full((T, 3), float('nan'), dtype=torch.float32, device=rows.device) if d_trans is not None else None
    nbytes = lib.empose_root_frame_vjp_workspace_bytes(T, seg_len)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=rows.device)
    _lib.check(lib.empose_root_frame_vjp(T, seg_len, _lib.RODRIGUES[conv], _lib.dptr(rows), rows.shape[1],
                                         _lib.dptr(trans), _lib.dptr(d_root), _lib.dptr(d_trans), _lib.dptr(g_root),
                                         _lib.dptr(g_trans), flags, _lib.dptr(ws), C.c_size_t(nbytes),
                                         _lib.current_stream()))
    return g_root, g_trans
