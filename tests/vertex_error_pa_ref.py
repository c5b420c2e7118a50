"""
The Procrustes-aligned per-vertex error (PA-PVE) restated in NumPy / torch for the tests (no tests here): per frame the
distances |x_v - (s R y_v + t)| between the vertices x of body A and the vertices y of body B after the similarity
transform that best maps y onto x -- the convention of em_pose_amd.eval.metrics.procrustes_align (optimal rotation and
scale, the last singular vector and value flipped by sign(det)), written through the 17 moments the device kernel sums
(csrc/mesh_err.hip): with a = x - pivot_a, b = y - pivot_b the sums of a, b, a b^T, |a|^2, |b|^2.

Two forms:
  float64 throughout (`distances64`): the reference.
  float32 control with the kernel's error sources (`distances32`): float32 vertices and pivots, the moments summed in
  float32 over groups of 32 consecutive vertices and then in float64, the solve in float64, s R and the centroids
  rounded to float32, the aligned distances in float32.
`bodies` takes the vertices and the posed root joints (the kernel's pivots) from oracle.torch_ref.smpl_fk.
"""
import numpy as np
import torch

from oracle import torch_ref as R


def moments(a, b, group=None):
    """a, b (n, V, 3) -> (n, 17) float64: sums over V of a (3), b (3), a b^T (9, row-major), |a|^2, |b|^2 -- in float64
    of whatever a and b hold, or with `group` in the dtype of a and b over groups of `group` consecutive vertices
    (zero-padded) and in float64 over the groups."""
    per = np.concatenate([a, b, (a[..., :, None] * b[..., None, :]).reshape(a.shape[:2] + (9,)),
                          (a * a).sum(-1, keepdims=True), (b * b).sum(-1, keepdims=True)], axis=-1)
    if group is None:
        return per.astype(np.float64).sum(axis=1)
    n, V, _ = per.shape
    pad = (-V) % group
    per = np.concatenate([per, np.zeros((n, pad, 17), per.dtype)], axis=1).reshape(n, -1, group, 17)
    part = per[:, :, 0].copy()
    for i in range(1, group):                   # sequential in the moments' own precision
        part = part + per[:, :, i]
    assert part.dtype == a.dtype
    return part.astype(np.float64).sum(axis=1)


def solve(S, V, pivot_a, pivot_b):
    """Moments (n, 17) of V points about the pivots (n, 3) -> M (n, 3, 3) with aligned b = (y - c_b) M + c_a, and the
    centroids c_a, c_b (n, 3); float64."""
    S = np.asarray(S, dtype=np.float64)
    sa, sb, sab = S[:, 0:3], S[:, 3:6], S[:, 6:15].reshape(-1, 3, 3)
    A = sab - sa[:, :, None] * sb[:, None, :] / V
    normX = np.sqrt(S[:, 15] - (sa * sa).sum(1) / V)
    normY = np.sqrt(S[:, 16] - (sb * sb).sum(1) / V)
    A = A / (normX * normY)[:, None, None]
    U, s, Vt = np.linalg.svd(A)
    Vm = np.swapaxes(Vt, 1, 2).copy()
    sign = np.sign(np.linalg.det(Vm @ np.swapaxes(U, 1, 2)))
    Vm[:, :, -1] *= sign[:, None]
    s[:, -1] *= sign
    T = Vm @ np.swapaxes(U, 1, 2)
    M = (normX * s.sum(1) / normY)[:, None, None] * T
    return M, np.asarray(pivot_a, np.float64) + sa / V, np.asarray(pivot_b, np.float64) + sb / V


def align64(x, y, pivot_a=None, pivot_b=None):
    """y (n, V, 3) mapped onto x, float64: what procrustes_align(x, y) returns."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    pa = np.zeros((x.shape[0], 3)) if pivot_a is None else np.asarray(pivot_a, np.float64)
    pb = np.zeros((x.shape[0], 3)) if pivot_b is None else np.asarray(pivot_b, np.float64)
    M, ca, cb = solve(moments(x - pa[:, None], y - pb[:, None]), x.shape[1], pa, pb)
    return (y - cb[:, None]) @ M + ca[:, None]


def distances64(x, y, pivot_a=None, pivot_b=None):
    return np.linalg.norm(np.asarray(x, np.float64) - align64(x, y, pivot_a, pivot_b), axis=-1)


def distances32(x, y, pivot_a, pivot_b):
    """The control: float32 in, (n, V) float32 out."""
    x, y, pa, pb = (np.asarray(t, np.float32) for t in (x, y, pivot_a, pivot_b))
    M, ca, cb = solve(moments(x - pa[:, None], y - pb[:, None], group=32), x.shape[1], pa, pb)
    M, ca, cb = M.astype(np.float32), ca.astype(np.float32), cb.astype(np.float32)
    d = (x - ca[:, None]) - (y - cb[:, None]) @ M
    out = np.sqrt((d * d).sum(-1))
    assert out.dtype == np.float32
    return out


def bodies(model, conv, dtype, a, b, rows=None):
    """Bodies (pose, root, betas, trans or None) a and b through the oracle in `dtype`: vertices (n, V', 3) of both
    (V' = `rows` of the mesh, or all of it) and the posed root joints (n, 3) of both, numpy."""
    bm = R.BodyModelTensors(model, dtype=dtype, rodrigues_convention=conv)
    t = lambda x: None if x is None else torch.from_numpy(np.asarray(x, dtype=np.float64)).to(dtype)
    out = []
    for body in (a, b):
        v, j = R.smpl_fk(bm, t(body[0]), t(body[2]), t(body[1]), t(body[3]))
        if rows is not None:
            v = v[:, torch.from_numpy(np.asarray(rows, dtype=np.int64))]
        out.append((v.numpy(), j[:, 0].numpy()))
    return out[0][0], out[1][0], out[0][1], out[1][1]


def sums(d):
    """(n, V) -> (n, 2) float64: the per-frame sums of d and d^2 accumulated in d's own precision."""
    return np.stack([d.sum(axis=1), (d * d).sum(axis=1)], axis=1).astype(np.float64)
