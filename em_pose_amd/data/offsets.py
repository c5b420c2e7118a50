"""
Per-subject sensor offsets estimated from calibration recordings, HIP-backed (csrc/offset_stats.hip): the producer of
the `*_offsets.npz` files that `SampleMarkersWithOffsets`, `RealSample` and the training and evaluation scripts read.

The reference ships those files with its data release and documents them as "pre-defined estimated offsets"
(transforms.py:132-155, data.py:131-151); its estimator is not in its tree.  The definition here is this project's own
(DESIGN.md section 9), the inverse of `SampleMarkersWithOffsets` at noise level -1: per frame f and sensor m, with
(pos_f, ori_f) the virtual sensor on the ground-truth mesh and (p_f, R_f) the real reading in the same body frame,

    o_f = ori_f^T (p_f - pos_f)        Q_f = ori_f^T R_f

and per (subject, sensor), over the n frames in which the sensor is not missing (`mask == 1`),

    means = mean of o_f,   covs = their sample covariance (n - 1; zeros for n < 2),
    r     = the rotation closest to the mean of Q_f (chordal mean: U diag(1, 1, det(U V^T)) V^T of its SVD),
    r_spread_deg = degrees(acos((mean of trace(r^T Q_f) - 1) / 2)), how far the Q_f scatter around r.

  offset_stats       the launch, on device tensors
  estimate_offsets   recordings (`RealSample`, numpy form) -> {subject: offset set}
  save_offsets_npz   an offset set -> a file `load_offsets_npz` reads
"""
import copy
import warnings

import numpy as np
import torch

from em_pose_amd import _lib

GROUP_DTYPE = np.dtype([('first_frame', np.int32), ('n_frames', np.int32)])   # empose_offset_group
SPREAD_WARN_DEG = 45.0   # beyond it the chordal mean is poorly determined


def group_table(groups):
    """(G, 2) rows (first_frame, n_frames), or records of GROUP_DTYPE -> records of GROUP_DTYPE.  ValueError for a row
    that does not fit int32; everything else is checked by the C layer."""
    if isinstance(groups, np.ndarray) and groups.dtype == GROUP_DTYPE:
        return np.ascontiguousarray(groups)
    rows = np.asarray(groups, dtype=np.int64).reshape(-1, 2)
    if rows.size and (rows.min() < -2 ** 31 or rows.max() >= 2 ** 31):
        raise ValueError('group table entries must fit int32 (got {} .. {})'.format(rows.min(), rows.max()))
    table = np.zeros(len(rows), dtype=GROUP_DTYPE)
    table['first_frame'], table['n_frames'] = rows[:, 0], rows[:, 1]
    return table


def offset_stats(helper, vertices, vertex_ids, pos, ori, masks, groups, per_frame=False):
    """empose_offset_stats on fp32 CUDA tensors.  `helper`: the `VirtualMarkerHelper` of the mesh `vertices` (T, V, 3)
    live on, `vertex_ids` the M sensors in its numbering; `pos` (T, M, 3) and `ori` (T, M, 3, 3) the real readings in the
    frame of the vertices; `masks` (T, M), 1 where the sensor was read, or None; `groups` rows (first_frame, n_frames),
    ascending and not overlapping, one per subject.  Returns a dict of device tensors: means (G, M, 3), covs (G, M, 3, 3),
    r (G, M, 3, 3), r_trace (G, M), counts (G, M) int32 and, with `per_frame`, local_frames (T, M, 3) and q_frames
    (T, M, 3, 3) (zeros where a frame does not count or belongs to no group).  A bad group table raises `EmposeError`
    before anything is launched."""
    given = [t for t in (vertices, pos, ori, masks) if t is not None]
    if any(not t.is_cuda for t in given):
        raise _lib.EmposeError('offset_stats needs GPU tensors; there is no CPU fallback')
    f32 = lambda t: t.contiguous().float()
    t, nv, m = vertices.shape[0], vertices.shape[1], len(vertex_ids)
    dev = vertices.device
    v, pos, ori = f32(vertices), f32(pos).reshape(t, m, 3), f32(ori).reshape(t, m, 3, 3)
    masks = None if masks is None else f32(masks).reshape(t, m)
    table = group_table(groups)
    g = len(table)
    center, hlp, deg, faces, max_deg = helper._tables(vertex_ids, dev)
    lib = _lib.lib()
    with torch.cuda.device(dev):
        table_dev = torch.from_numpy(table.view(np.int32).reshape(g, 2).copy()).to(dev)
        new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
        out = {'means': new(g, m, 3), 'covs': new(g, m, 3, 3), 'r': new(g, m, 3, 3), 'r_trace': new(g, m),
               'counts': torch.empty(g, m, dtype=torch.int32, device=dev)}
        if per_frame:
            out['local_frames'] = torch.zeros(t, m, 3, dtype=torch.float32, device=dev)
            out['q_frames'] = torch.zeros(t, m, 3, 3, dtype=torch.float32, device=dev)
        ws_bytes = lib.empose_offset_stats_workspace_bytes(t, g, m)
        ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
        _lib.check(lib.empose_offset_stats(
            t, nv, _lib.dptr(v), m, max_deg, _lib.dptr(center), _lib.dptr(hlp), _lib.dptr(deg), _lib.dptr(faces),
            _lib.dptr(pos), _lib.dptr(ori), _lib.dptr(masks), g, table.ctypes.data, _lib.dptr(table_dev),
            _lib.dptr(out['means']), _lib.dptr(out['covs']), _lib.dptr(out['r']), _lib.dptr(out['r_trace']),
            _lib.dptr(out['counts']), _lib.dptr(out.get('local_frames')), _lib.dptr(out.get('q_frames')),
            _lib.dptr(ws), ws_bytes, _lib.current_stream()))
    return out


def r_spread_deg(r_trace):
    """The angle of the mean of trace(r^T Q_f): 0 when every frame's rotational offset equals r."""
    return np.degrees(np.arccos(np.clip((np.asarray(r_trace, dtype=np.float64) - 1.0) * 0.5, -1.0, 1.0)))


def pooled_recordings(smpl_model, samples, subjects, m, normalized, device, who):
    """What `estimate_offsets` and `search_placement` (data/placement.py) read of their recordings, a list of `RealSample`
    in numpy form with `m` sensors each: the samples pooled by subject key -- in the order of the keys' first appearance,
    in the given order within a key -- and concatenated along the frames.  Unless `normalized`, a copy of every sample
    goes through `NormalizeRealMarkers`; the caller's arrays are not modified.  Returns a dict: device, keys, firsts and
    per_subject (each key's first pooled frame and number of frames), lengths (frames per pooled sample) and the float32
    arrays poses (T, 66), betas (T, 10: the sample's shape in every frame), pos (T, m, 3), ori (T, m, 3, 3), masks (T, m).
    `who` names the caller in the errors."""
    from em_pose_amd.data.transforms import NormalizeRealMarkers
    from em_pose_amd.helpers.configuration import CONSTANTS as C
    samples = list(samples)
    if not samples:
        raise ValueError('{} needs at least one recording'.format(who))
    subjects = ['all'] * len(samples) if subjects is None else list(subjects)
    if len(subjects) != len(samples):
        raise ValueError('{} subject keys for {} samples'.format(len(subjects), len(samples)))
    device = torch.device(smpl_model.bm.f.device if device is None else device)
    if device.type != 'cuda':
        raise _lib.EmposeError('{} needs a GPU (got device {}); there is no CPU fallback'.format(who, device))

    keys = list(dict.fromkeys(subjects))
    order = [i for k in keys for i in range(len(samples)) if subjects[i] == k]   # pooled by subject, given order within
    if not normalized:
        samples = [NormalizeRealMarkers()(copy.copy(s)) for s in samples]
    for s in samples:
        if np.asarray(s.marker_pos_real).shape[-1] != m * 3:
            raise ValueError('recording {} has {} sensors, vertex_ids {}'.format(
                s.id, np.asarray(s.marker_pos_real).shape[-1] // 3, m))
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    per_subject = [sum(samples[i].n_frames for i in order if subjects[i] == k) for k in keys]
    return {
        'device': device, 'keys': keys, 'per_subject': per_subject,
        'firsts': np.concatenate([[0], np.cumsum(per_subject)[:-1]]),
        'lengths': [samples[i].n_frames for i in order],
        'poses': np.concatenate([f32(samples[i].smpl_poses)[:, :C.MAX_INDEX_ROOT_AND_BODY] for i in order]),
        'betas': np.concatenate([np.repeat(f32(samples[i].smpl_shape).reshape(1, -1), samples[i].n_frames, axis=0)
                                 for i in order]),
        'pos': np.concatenate([f32(samples[i].marker_pos_real).reshape(-1, m, 3) for i in order]),
        'ori': np.concatenate([f32(samples[i].marker_ori_real).reshape(-1, m, 3, 3) for i in order]),
        'masks': np.concatenate([f32(samples[i].marker_masks).reshape(-1, m) for i in order])}


def root_normalized_poses(smpl_model, rec, device):
    """The pooled poses of `pooled_recordings` on the device, the root orientations of every sample relative to its first
    (the root-frame kernel, one segment per sample): the frame `NormalizeRealMarkers` puts the readings in."""
    from em_pose_amd.bodymodels.smpl import root_frame_fwd
    poses_d = torch.from_numpy(rec['poses']).to(device)
    at = 0
    for n in rec['lengths']:
        if n > 0:
            seg = poses_d[at:at + n]
            seg[:, :3] = root_frame_fwd(seg, None, n, _lib.RODRIGUES[smpl_model.rodrigues_convention])[0]
        at += n
    return poses_d


def estimate_offsets(smpl_model, samples, subjects=None, vertex_ids=None, normalized=False, device=None,
                     per_frame=False):
    """
    The offset sets of the subjects of `samples`, a list of `RealSample` in numpy form (before `ToTensor`).

    `subjects`: one key per sample; samples with the same key are pooled, concatenated in the given order (default: all
    samples are one subject, key 'all').  Unless `normalized`, a copy of every sample goes through `NormalizeRealMarkers`;
    the caller's arrays are not modified.  The ground-truth mesh is evaluated on the sensor sub-mesh
    (`smpl_model.sub_mesh(vertex_ids)`) in the frame that transform puts the readings in: the root orientations relative
    to the sample's first (the root-frame kernel, one segment per sample), no translation, the sample's shape in every
    frame.  One `offset_stats` launch then covers all subjects.

    Returns {subject: {'means' (M, 3), 'covs' (M, 3, 3), 'r' (M, 3, 3), 'vertex_ids' (M,), 'counts' (M,),
    'r_spread_deg' (M,)}} as numpy arrays, with `per_frame` also 'local_frames' (n, M, 3) and 'q_frames' (n, M, 3, 3) of
    the subject's n pooled frames.  Warns, and does not fail, about a sensor with fewer than two counting frames or a
    spread above 45 degrees.  `vertex_ids` defaults to CONSTANTS.VERTEX_IDS.
    """
    from em_pose_amd.data.virtual_sensors import VirtualMarkerHelper
    from em_pose_amd.helpers.configuration import CONSTANTS as C
    vertex_ids = [int(v) for v in (C.VERTEX_IDS if vertex_ids is None else vertex_ids)]
    m = len(vertex_ids)
    rec = pooled_recordings(smpl_model, samples, subjects, m, normalized, device, 'estimate_offsets')
    device, keys, firsts, per_subject = rec['device'], rec['keys'], rec['firsts'], rec['per_subject']
    groups = np.stack([firsts, per_subject], axis=1)

    up = lambda a: torch.from_numpy(a).to(device)
    with torch.no_grad(), torch.cuda.device(device):
        poses_d = root_normalized_poses(smpl_model, rec, device)
        sub = smpl_model.sub_mesh(vertex_ids)
        vertices, _ = sub(poses_body=poses_d[:, 3:], betas=up(rec['betas']), poses_root=poses_d[:, :3])
        stats = offset_stats(VirtualMarkerHelper(sub), vertices, sub.local_ids(vertex_ids), up(rec['pos']), up(rec['ori']),
                             up(rec['masks']), groups, per_frame=per_frame)
        host = {k: v.cpu().numpy() for k, v in stats.items()}

    out = {}
    for g, key in enumerate(keys):
        est = {'means': host['means'][g], 'covs': host['covs'][g], 'r': host['r'][g],
               'vertex_ids': np.asarray(vertex_ids, dtype=np.int64), 'counts': host['counts'][g],
               'r_spread_deg': r_spread_deg(host['r_trace'][g]).astype(np.float32)}
        if per_frame:
            sl = slice(int(firsts[g]), int(firsts[g]) + int(per_subject[g]))
            est['local_frames'], est['q_frames'] = host['local_frames'][sl], host['q_frames'][sl]
        few = np.nonzero(est['counts'] < 2)[0]
        if few.size:
            warnings.warn('subject {}: sensors {} have fewer than two valid frames (counts {}); their offsets are not '
                          'estimated'.format(key, few.tolist(), est['counts'][few].tolist()))
        wide = np.nonzero(est['r_spread_deg'] > SPREAD_WARN_DEG)[0]
        if wide.size:
            warnings.warn('subject {}: the rotational offsets of sensors {} spread by {} degrees (above {}); their mean '
                          'rotation is poorly determined'.format(key, wide.tolist(),
                                                                 np.round(est['r_spread_deg'][wide], 1).tolist(),
                                                                 SPREAD_WARN_DEG))
        out[key] = est
    return out


def save_offsets_npz(path, estimate):
    """One subject's offset set as the `*_offsets.npz` file `load_offsets_npz` reads (means, covs, r, vertex_ids), plus
    counts and r_spread_deg, which readers ignore."""
    np.savez(path, means=np.asarray(estimate['means'], dtype=np.float32),
             covs=np.asarray(estimate['covs'], dtype=np.float32), r=np.asarray(estimate['r'], dtype=np.float32),
             vertex_ids=np.asarray(estimate['vertex_ids'], dtype=np.int64),
             counts=np.asarray(estimate['counts'], dtype=np.int32),
             r_spread_deg=np.asarray(estimate['r_spread_deg'], dtype=np.float32))
