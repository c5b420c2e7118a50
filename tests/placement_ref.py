"""
Restatement of the sensor placement search (empose_placement_accumulate / _finish, em_pose_amd/data/placement.py) in
float64 numpy: per sensor m and candidate vertex c, over the n frames with mask == 1,

    score[m, c] = (1 / n) sum_f |p_f(m) - x_f(c)|^2,      site[m] = argmin_c score[m, c], the lowest c on an exact tie,

and score = +inf, site = -1 when n == 0.  The inputs are taken as they are (fp32 arrays are widened, not recomputed):
"float64 evaluated on the same fp32 inputs".
"""
import numpy as np

# The recordings of the end-to-end tests (tests/test_placement_cpu.py checks their precondition, tests/test_placement.py
# searches them): two subjects, 1 cm offsets.
E2E_LAYOUT = [('x', (150, 90)), ('y', (130,))]
E2E_SEED, E2E_OFFSET_SD = 91, 0.01


def scores(vertices, pos, masks=None, candidates=None, block=64):
    """(score (M, C) float64, site (M,) int64 vertex ids, counts (M,) int64) of vertices (T, V, 3), pos (T, M, 3),
    masks (T, M) or None, candidates an ascending id list or None (all V)."""
    v = np.asarray(vertices, dtype=np.float64)
    p = np.asarray(pos, dtype=np.float64)
    t, m = p.shape[:2]
    ids = np.arange(v.shape[1]) if candidates is None else np.asarray(candidates, dtype=np.int64)
    valid = np.ones((t, m), bool) if masks is None else np.asarray(masks) == 1
    counts = valid.sum(axis=0).astype(np.int64)
    total = np.zeros((m, len(ids)))
    for k in range(m):
        rows = np.nonzero(valid[:, k])[0]
        for at in range(0, len(rows), block):          # in blocks of frames: the (frames, C, 3) temporary stays small
            r = rows[at:at + block]
            d = p[r, k][:, None, :] - v[r][:, ids]
            total[k] += (d * d).sum(axis=-1).sum(axis=0)
    score = np.full((m, len(ids)), np.inf)
    read = counts > 0
    score[read] = total[read] / counts[read, None]
    site = np.where(read, ids[np.argmin(score, axis=1)], -1)      # argmin: the first of equal values
    return score, site.astype(np.int64), counts


def runner_up_gap(score):
    """Per sensor (second-best score) / (best score) of a table whose rows are finite."""
    s = np.sort(score, axis=1)
    return s[:, 1] / s[:, 0]


def recordings(model, ids, layout, seed, offset_sd=0.02, pos_noise=0.005):
    """`RealSample` recordings of a body model (dict of arrays) with sensors at `ids`, made on the CPU by the oracle.
    `layout`: (subject key, frames of each of its recordings) per subject.  A subject has its shape and its offsets
    (t ~ N(0, offset_sd), a rotational offset); a recording has random poses, a root orientation that does not start at
    the identity, a translation (both applied as `NormalizeRealMarkers` undoes them), `pos_noise` of isotropic position
    noise and 0.5 % of missing readings.  Returns (samples, subject keys)."""
    import torch

    from em_pose_amd.data.data import RealSample
    from em_pose_amd.data.transforms import matrix_to_rotvec
    from em_pose_amd.eval.metrics import rotvec_to_matrix
    from oracle import torch_ref as R
    from tests import offset_estimation_ref as REF
    rng = np.random.default_rng(seed)
    bm = R.BodyModelTensors(model, dtype=torch.float32)
    faces = np.asarray(model['f'], dtype=np.int64)
    t32 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32))
    samples, subjects = [], []
    for key, lengths in layout:
        betas = rng.normal(0, 1, 10).astype(np.float32)
        t, r0 = rng.normal(0.0, offset_sd, (len(ids), 3)), REF.exp_so3(rng.normal(0.0, 0.1, (len(ids), 3)))
        for k, f in enumerate(lengths):
            poses = np.concatenate([rng.normal(0, 0.5, (f, 3)), rng.normal(0, 0.3, (f, 63))], axis=1).astype(np.float32)
            poses[0, :3] = 0.0
            with torch.no_grad():
                v, _ = R.smpl_fk(bm, t32(poses[:, 3:]), t32(betas), t32(poses[:, :3]))
            p, Rr = REF.forward(v.numpy(), faces, ids, t, r0)
            p = p + rng.normal(0.0, pos_noise, p.shape)
            # moved as `NormalizeRealMarkers` undoes it: readings and root orientations turned by R0 about the origin,
            # then the translation
            R0 = REF.exp_so3(rng.normal(0, 0.7, 3))
            trans = rng.normal(0, 0.5, (f, 3)).astype(np.float32)
            poses[:, :3] = matrix_to_rotvec(R0 @ rotvec_to_matrix(poses[:, :3].astype(np.float64))).astype(np.float32)
            p, Rr = p @ R0.T + trans[:, None], R0 @ Rr
            masks = (rng.uniform(size=(f, len(ids))) > 0.005).astype(np.float32)
            samples.append(RealSample('{}_{:02d}'.format(key, k), p.astype(np.float32), Rr.astype(np.float32), masks, poses,
                                      betas, trans, {'means': None, 'covs': None, 'r': None}))
            subjects.append(key)
    return samples, subjects


def normalized_scene(model, samples):
    """What the search sees of `samples`, restated on the CPU: (vertices (T, V, 3), pos (T, M, 3), masks (T, M)) of the
    concatenated recordings in the frame of `NormalizeRealMarkers` -- a copy of every sample goes through it, the root
    orientations are taken relative to the sample's first, no translation -- the meshes by the float32 oracle."""
    import copy

    import torch

    from em_pose_amd.data.transforms import NormalizeRealMarkers, matrix_to_rotvec
    from em_pose_amd.eval.metrics import rotvec_to_matrix
    from oracle import torch_ref as R
    bm = R.BodyModelTensors(model, dtype=torch.float32)
    t32 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32))
    verts, pos, masks = [], [], []
    for s in samples:
        n = NormalizeRealMarkers()(copy.copy(s))
        rot = rotvec_to_matrix(np.asarray(s.smpl_poses[:, :3], dtype=np.float64))
        root = matrix_to_rotvec(rot[0].T @ rot)
        with torch.no_grad():
            v, _ = R.smpl_fk(bm, t32(s.smpl_poses[:, 3:66]), t32(s.smpl_shape), t32(root))
        m = n.marker_pos_real.shape[-1] // 3
        verts.append(v.numpy())
        pos.append(n.marker_pos_real.reshape(-1, m, 3))
        masks.append(np.asarray(s.marker_masks, dtype=np.float32))
    return np.concatenate(verts), np.concatenate(pos), np.concatenate(masks)


def full_mesh_scene(frames=64, seed=5, normal_offset=0.01):
    """The V = 6890 stand-in body model posed `frames` times by the float32 oracle, and readings at CONSTANTS.VERTEX_IDS
    moved `normal_offset` metres along the sensor normal: (vertices (T, 6890, 3) float32, pos (T, 12, 3) float32, ids)."""
    import torch

    from em_pose_amd import synthetic
    from em_pose_amd.helpers.configuration import CONSTANTS
    from oracle import torch_ref as R
    from tests import offset_estimation_ref as REF
    rng = np.random.default_rng(seed)
    model = synthetic.make_model()
    ids = [int(v) for v in CONSTANTS.VERTEX_IDS]
    bm = R.BodyModelTensors(model, dtype=torch.float32)
    t32 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32))
    with torch.no_grad():
        v, _ = R.smpl_fk(bm, t32(rng.normal(0, 0.3, (frames, 63))), t32(rng.normal(0, 1, (frames, 10))),
                         t32(rng.normal(0, 0.5, (frames, 3))))
    v = np.ascontiguousarray(v.numpy(), dtype=np.float32)
    t = np.tile([0.0, 0.0, normal_offset], (len(ids), 1))           # the third column of a sensor frame is its normal
    p, _ = REF.forward(v, np.asarray(model['f'], dtype=np.int64), ids, t, np.tile(np.eye(3), (len(ids), 1, 1)))
    return v, p.astype(np.float32), ids


def moment_score(means, covs, counts):
    """|means|^2 + (n - 1) / n trace(covs): what the offset statistics of a site say its score is."""
    n = np.asarray(counts, dtype=np.float64)
    return (np.asarray(means) ** 2).sum(axis=-1) + (n - 1.0) / n * np.trace(np.asarray(covs), axis1=-2, axis2=-1)
