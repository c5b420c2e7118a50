"""
Restatement of synthetic sensor sampling (empose_sample_sensors_fwd; reference data/transforms.py:132-226) in torch, in
whatever dtype the vertices have: the oracle's sensor frames (oracle/torch_ref.py virtual_pos_and_rot) plus the offset
formulas, differentiable, so float64 gives the reference values and gradients and float32 on the CPU the control.
"""
import numpy as np
import torch

from oracle import torch_ref as R

NONE, WINDOW, FRAME = 0, 1, 2   # EMPOSE_SAMPLE_LOCAL_* (include/empose_hip.h)
NAMES = ('pos', 'ori', 'nor', 'pos_synth', 'ori_synth', 'nor_synth')


def sample(vertices, faces, ids, f, mode, local=None, r=None):
    """vertices (n * f, V, 3) -> the six outputs (NAMES).  `local`: (n, M, 3) for WINDOW, (n * f, M, 3) for FRAME;
    `r`: (n, M, 3, 3) or None for the identity.  Arrays or tensors; computed in the dtype of `vertices`."""
    dt = vertices.dtype
    t, m = vertices.shape[0], len(ids)
    n = t // f
    c = lambda a: torch.as_tensor(np.asarray(a)).to(dt)
    pos, ori, nor = R.virtual_pos_and_rot(vertices, list(ids), R.sensor_tables(faces, list(ids)))
    pos_s = pos
    if mode == WINDOW:
        l = c(local).reshape(n, 1, m, 3).expand(n, f, m, 3).reshape(t, m, 3)
        pos_s = pos + torch.matmul(ori, l[..., None])[..., 0]
    elif mode == FRAME:
        pos_s = pos + torch.matmul(ori, c(local).reshape(t, m, 3)[..., None])[..., 0]
    ori_s = ori
    if r is not None:
        ori_s = torch.matmul(ori, c(r).reshape(n, 1, m, 3, 3).expand(n, f, m, 3, 3).reshape(t, m, 3, 3))
    return pos, ori, nor, pos_s, ori_s, ori_s[..., 2]


def sample_np(vertices, faces, ids, f, mode, local=None, r=None, dtype=torch.float64):
    """`sample` on a float array, evaluated in `dtype` on the CPU; dict of float64 arrays."""
    with torch.no_grad():
        outs = sample(torch.from_numpy(np.asarray(vertices)).to(dtype), faces, ids, f, mode, local, r)
    return {k: o.numpy().astype(np.float64) for k, o in zip(NAMES, outs)}


def d_vertices(vertices, faces, ids, f, mode, local, r, cots, dtype=torch.float64):
    """The cotangent of the vertices for cotangents `cots` (dict by NAMES, missing or None = not given), by autograd
    through `sample` in `dtype`; float64 array."""
    v = torch.from_numpy(np.asarray(vertices)).to(dtype).requires_grad_(True)
    outs = sample(v, faces, ids, f, mode, local, r)
    loss = 0
    for k, o in zip(NAMES, outs):
        if cots.get(k) is not None:
            loss = loss + (o * torch.from_numpy(np.asarray(cots[k])).to(dtype)).sum()
    loss.backward()
    return v.grad.numpy().astype(np.float64)


def check_rows(name, got, w64, w32):
    """The project's bar per frame row (tests/test_virtual_sensors_vjp.py): the largest error of a row is at most
    1e-4 x the row's largest |w64|, and at most 4 x the error of the float32 CPU control plus 1e-7 x that scale."""
    got, w64, w32 = (np.asarray(a, dtype=np.float64).reshape(a.shape[0], -1) for a in (got, w64, w32))
    scale = np.abs(w64).max(axis=1)
    err = np.abs(got - w64).max(axis=1)
    err32 = np.abs(w32 - w64).max(axis=1)
    bad = np.nonzero((err > 1e-4 * scale) | (err > 4 * err32 + 1e-7 * scale))[0]
    assert bad.size == 0, '{}: rows {} err {} scale {} control {}'.format(
        name, bad[:8], err[bad[:8]], scale[bad[:8]], err32[bad[:8]])


def irregular_mesh():
    """A small mesh with unequal vertex degrees: a closed fan of 7 triangles (center of degree 7, rim of degree 2), a
    triangle split at an inner point (degree 3) and an open fan of 4 triangles (a boundary vertex of degree 4), gently
    curved so that no normal vanishes.  (points (V, 3) float64, faces (F, 3) int64)"""
    ring = 7
    pts = [[0, 0, 0.1]] + [[np.cos(2 * np.pi * i / ring), np.sin(2 * np.pi * i / ring), 0.05 * np.sin(3 * i)]
                           for i in range(ring)]
    faces = [[0, 1 + i, 1 + (i + 1) % ring] for i in range(ring)]
    o = len(pts)
    pts += [[3, 0, 0], [4, 0, 0.1], [3.5, 1, 0], [3.5, 0.3, 0.2]]
    faces += [[o, o + 1, o + 3], [o + 1, o + 2, o + 3], [o + 2, o, o + 3]]
    o = len(pts)
    pts += [[6, 0, 0.05]] + [[6 + np.cos(a), np.sin(a), 0.1 * a] for a in np.linspace(0, 2.5, 5)]
    faces += [[o, o + 1 + i, o + 2 + i] for i in range(4)]
    return np.asarray(pts, dtype=np.float64), np.asarray(faces, dtype=np.int64)
