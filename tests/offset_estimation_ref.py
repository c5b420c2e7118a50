"""
Restatement of the per-subject offset estimator (empose_offset_stats, em_pose_amd/data/offsets.py) in torch and numpy: the
oracle's sensor frames (oracle/torch_ref.py virtual_pos_and_rot) in whatever dtype the vertices have, the per-frame
offsets o = ori^T (p - pos) and Q = ori^T R in that dtype, and the statistics of their float64 values in numpy.  float64
gives the reference values, float32 on the CPU the control of the per-frame outputs.  `forward` is the model the
estimator inverts: SampleMarkersWithOffsets at noise level -1, (pos + ori . t, ori . r0).

Mirrors tests/sample_sensors_ref.py, whose `check_rows` is the bar of the per-frame comparisons.
"""
import numpy as np
import torch

from oracle import torch_ref as R
from tests import helpers as H
from tests.sample_sensors_ref import check_rows, irregular_mesh  # noqa: F401  (re-exported for the tests)


def frames(vertices, faces, ids):
    """(pos (T, M, 3), ori (T, M, 3, 3)) of the virtual sensors, tensors in the dtype of `vertices`."""
    pos, ori, _ = R.virtual_pos_and_rot(vertices, list(ids), R.sensor_tables(faces, list(ids)))
    return pos, ori


def forward(vertices, faces, ids, t, r0, dtype=torch.float64):
    """Noise-free readings for offsets t (M, 3) or (T, M, 3) and r0 (M, 3, 3): float64 arrays (p, Rr)."""
    v = torch.from_numpy(np.asarray(vertices)).to(dtype)
    c = lambda a: torch.from_numpy(np.asarray(a)).to(dtype)
    with torch.no_grad():
        pos, ori = frames(v, faces, ids)
        t = c(t).expand(pos.shape)
        p = pos + torch.matmul(ori, t[..., None])[..., 0]
        Rr = torch.matmul(ori, c(r0))
    return p.numpy().astype(np.float64), Rr.numpy().astype(np.float64)


def per_frame(vertices, faces, ids, p, Rr, masks=None, dtype=torch.float64):
    """o (T, M, 3) and Q (T, M, 3, 3) evaluated in `dtype`, zeros where masks != 1; float64 arrays."""
    v = torch.from_numpy(np.asarray(vertices)).to(dtype)
    c = lambda a: torch.from_numpy(np.asarray(a)).to(dtype)
    with torch.no_grad():
        pos, ori = frames(v, faces, ids)
        ot = ori.transpose(-1, -2)
        o = torch.matmul(ot, (c(p) - pos)[..., None])[..., 0]
        Q = torch.matmul(ot, c(Rr))
    o, Q = o.numpy().astype(np.float64), Q.numpy().astype(np.float64)
    if masks is not None:
        valid = np.asarray(masks) == 1
        o, Q = o * valid[..., None], Q * valid[..., None, None]
    return o, Q


def statistics(o, Q, masks, groups):
    """The definition, in float64 numpy, from per-frame o and Q: dict of means (G, M, 3), covs (G, M, 3, 3),
    r (G, M, 3, 3), r_trace (G, M), counts (G, M) and the singular values `sing` (G, M, 3) of the mean of Q."""
    t, m = o.shape[:2]
    valid = np.ones((t, m), bool) if masks is None else np.asarray(masks) == 1
    g = len(groups)
    out = {'means': np.zeros((g, m, 3)), 'covs': np.zeros((g, m, 3, 3)), 'r': np.tile(np.eye(3), (g, m, 1, 1)),
           'r_trace': np.full((g, m), 3.0), 'counts': np.zeros((g, m), np.int64), 'sing': np.ones((g, m, 3))}
    for gi, (first, n_frames) in enumerate(groups):
        sl = slice(int(first), int(first) + int(n_frames))
        for mi in range(m):
            ok = valid[sl, mi]
            n = int(ok.sum())
            out['counts'][gi, mi] = n
            if n == 0:
                continue
            og, Qg = o[sl, mi][ok], Q[sl, mi][ok]
            out['means'][gi, mi] = og.mean(axis=0)
            if n >= 2:
                out['covs'][gi, mi] = np.cov(og, rowvar=False)
            U, S, Vt = np.linalg.svd(Qg.mean(axis=0))
            d = np.linalg.det(U @ Vt)
            out['r'][gi, mi] = U @ np.diag([1.0, 1.0, d]) @ Vt
            out['r_trace'][gi, mi] = S[0] + S[1] + d * S[2]
            out['sing'][gi, mi] = S
    return out


def estimate(vertices, faces, ids, p, Rr, masks, groups, dtype=torch.float64):
    """`per_frame` in `dtype`, then `statistics`: the dict of `statistics` plus local_frames and q_frames."""
    o, Q = per_frame(vertices, faces, ids, p, Rr, masks, dtype)
    out = statistics(o, Q, masks, groups)
    out['local_frames'], out['q_frames'] = o, Q
    return out


def exp_so3(r):
    """Rodrigues for rotation vectors (..., 3) -> (..., 3, 3), float64."""
    r = np.asarray(r, dtype=np.float64)
    a = np.maximum(np.linalg.norm(r, axis=-1, keepdims=True), 1e-12)
    k = r / a
    K = np.zeros(r.shape[:-1] + (3, 3))
    K[..., 0, 1], K[..., 0, 2] = -k[..., 2], k[..., 1]
    K[..., 1, 0], K[..., 1, 2] = k[..., 2], -k[..., 0]
    K[..., 2, 0], K[..., 2, 1] = -k[..., 1], k[..., 0]
    return np.eye(3) + np.sin(a)[..., None] * K + (1.0 - np.cos(a))[..., None] * (K @ K)


def posed_small(n, seed, noise=0.003, ids=None, min_cross=0.2):
    """Posed meshes of the small model (float32 CPU oracle) plus per-vertex noise, (n, 160, 3) float32.  With `ids` only
    frames whose sensor frames are well conditioned are kept: at every sensor the direction to the helper vertex is at
    least ~11 degrees away from the normal, |nh x s| >= min_cross in float64 (the recipe and the reason of
    tests/test_virtual_sensors_vjp.py: near that degeneracy the frame amplifies the rounding of the vertices by
    1 / |nh x s|, and which fp32 evaluation happens to round better decides a comparison with the float32 control)."""
    rng = np.random.default_rng(seed)
    model = H.small_model()
    bm = R.BodyModelTensors(model, dtype=torch.float32)
    t = lambda a: torch.from_numpy(a.astype(np.float32))
    kept = []
    while sum(len(k) for k in kept) < n:
        k = n if ids is None else n + n // 8 + 8
        with torch.no_grad():
            v, _ = R.smpl_fk(bm, t(rng.normal(0, 0.3, (k, 63))), t(rng.normal(0, 1, (k, 10))), t(rng.normal(0, 0.5, (k, 3))))
        v = (v.numpy() + rng.normal(0, noise, v.shape)).astype(np.float32)
        if ids is not None:
            v = v[min_cross_of(v, model['f'], ids) >= min_cross]
        kept.append(v)
    return np.ascontiguousarray(np.concatenate(kept)[:n])


def min_cross_of(vertices, faces, ids):
    """Per frame the smallest |nh x s| over the sensors, float64: nh the unit normal, s the unit direction to the helper."""
    v = torch.from_numpy(np.asarray(vertices)).double()
    sub_faces, vf_sub, helpers = R.sensor_tables(faces, list(ids))
    nor = R.vertex_normals_sub(v, torch.from_numpy(sub_faces), torch.from_numpy(vf_sub))
    nh = nor / nor.norm(dim=-1, keepdim=True)
    sd = v[:, helpers.tolist()] - v[:, list(ids)]
    sd = sd / sd.norm(dim=-1, keepdim=True)
    return torch.cross(nh, sd, dim=-1).norm(dim=-1).min(dim=1).values.numpy()


def small_ids():
    return [int(v) for v in H.load_case('train_lgdrnn12_n2')['meta']['vertex_ids']]


def noisy_readings(vertices, faces, ids, rng, pos_noise=0.005, rot_noise_deg=2.0):
    """Readings of the forward model with per-sensor offsets (t, r0) drawn as synthetic.make_windows draws them, plus
    isotropic position noise and rotation noise (R . exp(noise)): float32 (p, Rr), float64 (t, r0)."""
    m = len(ids)
    t = rng.normal(0.0, 0.02, (m, 3))
    r0 = exp_so3(rng.normal(0.0, 0.1, (m, 3)))
    p, Rr = forward(vertices, faces, ids, t, r0)
    p = p + rng.normal(0.0, pos_noise, p.shape)
    Rr = Rr @ exp_so3(rng.normal(0.0, np.deg2rad(rot_noise_deg), p.shape))
    return p.astype(np.float32), Rr.astype(np.float32), t, r0
