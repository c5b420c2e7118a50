"""
Sensor placement search, HIP-backed (csrc/placement.hip): which vertices of the body mesh are the sensors strapped over?
The step before `estimate_offsets` (data/offsets.py), which takes its `vertex_ids` as given; the reference has no such
tool, its ids are its authors' strap placement (CONSTANTS.VERTEX_IDS).  The definition is this project's own (DESIGN.md
section 9): per sensor m and candidate vertex c, over the n frames of a group in which the sensor was read (`mask == 1`),
with p_f the real reading and x_f(c) the ground-truth vertex in the body frame `estimate_offsets` uses,

    score[m, c] = (1 / n) sum_f |p_f(m) - x_f(c)|^2   (m^2)      site[m] = argmin_c score[m, c], the lowest c on a tie

and score = +inf, site = -1 when n == 0.  The score needs no sensor frame, and it is what the offsets pay for a site:
score[m, c] = |means|^2 + (n - 1) / n trace(covs) of the offset statistics there.

  placement_scores             one slab of frames into the running sums, on device tensors
  placement_finish             the sums -> score, best, best_score
  search_placement             recordings (`RealSample`, numpy form) -> {key: placement}
  candidates_excluding_bones   the vertices that are not skinned to some bones (fingers, for instance)
"""
import warnings

import numpy as np
import torch

from em_pose_amd import _lib
from em_pose_amd.data.offsets import pooled_recordings, root_normalized_poses
from em_pose_amd.eval.surface_metrics import closest_point_on_mesh


class Candidates(object):
    """An ascending list of candidate vertex ids, on the host and on a device: what a search over part of the mesh hands
    to every launch.  `Candidates.of(None, device)` is None, the whole mesh."""

    def __init__(self, ids, device):
        ids = np.asarray(ids)
        if ids.ndim != 1 or ids.size == 0 or ids.dtype.kind not in 'iu':
            raise ValueError('candidates must be a non-empty one-dimensional list of vertex ids')
        if ids.min() < -2 ** 31 or ids.max() >= 2 ** 31:
            raise ValueError('candidate ids must fit int32 (got {} .. {})'.format(ids.min(), ids.max()))
        self.host = np.ascontiguousarray(ids, dtype=np.int32)
        self.dev = torch.from_numpy(self.host).to(device)

    @staticmethod
    def of(candidates, device):
        if candidates is None or isinstance(candidates, Candidates):
            return candidates
        return Candidates(candidates, device)

    def __len__(self):
        return len(self.host)


def _need_gpu(who, tensors):
    if any(t is not None and not t.is_cuda for t in tensors):
        raise _lib.EmposeError('{} needs GPU tensors; there is no CPU fallback'.format(who))


def placement_scores(vertices, pos, masks, sums=None, counts=None, candidates=None):
    """empose_placement_accumulate on CUDA tensors: one slab of one group.  `vertices` (T, V, 3) the ground-truth mesh,
    `pos` (T, M, 3) the real readings in its frame, `masks` (T, M), 1 where the sensor was read, or None; `candidates` an
    ascending list of vertex ids (or a `Candidates`), None for all V.  Adds the slab to the running `sums` (M, C) float64
    and `counts` (M,) int32 -- new zeros when None, a group's first slab -- and returns them.  A candidate list that is not
    ascending within [0, V) raises `EmposeError` before anything is launched."""
    _need_gpu('placement_scores', (vertices, pos, masks, sums, counts))
    t, nv = vertices.shape[0], vertices.shape[1]
    dev = vertices.device
    f32 = lambda x: x.contiguous().float()
    v = f32(vertices)
    pos = f32(pos).reshape(t, -1, 3)
    m = pos.shape[1]
    masks = None if masks is None else f32(masks).reshape(t, m)
    cand = Candidates.of(candidates, dev)
    c = nv if cand is None else len(cand)
    lib = _lib.lib()
    with torch.cuda.device(dev):
        if sums is None:
            sums = torch.zeros(m, c, dtype=torch.float64, device=dev)
        if counts is None:
            counts = torch.zeros(m, dtype=torch.int32, device=dev)
        if tuple(sums.shape) != (m, c) or sums.dtype != torch.float64 or tuple(counts.shape) != (m,) or \
                counts.dtype != torch.int32:
            raise ValueError('sums must be ({}, {}) float64 and counts ({},) int32'.format(m, c, m))
        ws_bytes = lib.empose_placement_workspace_bytes(t, m, c)
        ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
        _lib.check(lib.empose_placement_accumulate(
            t, nv, _lib.dptr(v), m, _lib.dptr(pos), _lib.dptr(masks), c,
            None if cand is None else cand.host.ctypes.data, None if cand is None else _lib.dptr(cand.dev),
            _lib.dptr(sums), _lib.dptr(counts), _lib.dptr(ws), ws_bytes, _lib.current_stream()))
    return sums, counts


def placement_finish(sums, counts, candidates=None):
    """empose_placement_finish: the running sums of `placement_scores` -> (score (M, C) float32, best (M,) int32, the
    winning candidates' vertex ids, best_score (M,) float32) on the device; +inf and -1 for a sensor that was never
    read.  `candidates`: what the sums were accumulated with."""
    _need_gpu('placement_finish', (sums, counts))
    m, c = sums.shape
    dev = sums.device
    cand = Candidates.of(candidates, dev)
    if cand is not None and len(cand) != c:
        raise ValueError('{} candidates for sums of {} columns'.format(len(cand), c))
    if sums.dtype != torch.float64 or counts.dtype != torch.int32 or tuple(counts.shape) != (m,):
        raise ValueError('sums must be float64 and counts ({},) int32'.format(m))
    with torch.cuda.device(dev):
        score = torch.empty(m, c, dtype=torch.float32, device=dev)
        best = torch.empty(m, dtype=torch.int32, device=dev)
        best_score = torch.empty(m, dtype=torch.float32, device=dev)
        _lib.check(_lib.lib().empose_placement_finish(
            m, c, _lib.dptr(sums.contiguous()), _lib.dptr(counts.contiguous()),
            None if cand is None else _lib.dptr(cand.dev), _lib.dptr(score), _lib.dptr(best), _lib.dptr(best_score),
            _lib.current_stream()))
    return score, best, best_score


def candidates_excluding_bones(model, bones):
    """The vertices of a body model (an `SMPLLayer`, or its dict of arrays) whose largest skinning weight is not on one
    of `bones` (joint indices): an ascending int32 list for `candidates`.  Host numpy."""
    arrays = getattr(model, 'model', model)
    weights = np.asarray(arrays['weights'])
    bones = np.asarray(list(bones), dtype=np.int64).reshape(-1)
    if bones.size and (bones.min() < 0 or bones.max() >= weights.shape[1]):
        raise ValueError('bones must be within [0, {})'.format(weights.shape[1]))
    return np.nonzero(~np.isin(np.argmax(weights, axis=1), bones))[0].astype(np.int32)


def search_placement(smpl_model, samples, subjects=None, per_subject=False, candidates=None, normalized=False, slab=1024,
                     device=None):
    """
    The sites of the sensors of `samples`, a list of `RealSample` in numpy form (before `ToTensor`): the recordings
    `estimate_offsets` reads, in its frame conventions (`NormalizeRealMarkers` on a copy unless `normalized`, root
    orientations relative to each sample's first, no translation, the sample's shape in every frame).

    By default all recordings are pooled into one placement under the key 'all': a model holds one `vertex_ids` for
    everybody.  `per_subject=True`: one placement per key of `subjects` (one key per sample; default: all 'all'), for
    analysis.  `candidates`: an ascending list of vertex ids to search (`candidates_excluding_bones`), default the whole
    mesh.  The full mesh is evaluated with `smpl_model.forward` in slabs of at most `slab` frames that never cross a
    group, so the memory beyond the inputs and the (M, C) tables does not grow with the number of frames.

    Returns {key: {'vertex_ids' (M,) int64, 'rms_mm' (M,), 'runner_up_ids' (M,) int64, 'runner_up_rms_mm' (M,),
    'counts' (M,) int32, 'score' (M, C) float32, 'skin_mm' (M,)}} as numpy arrays: the site, the root of its score in
    millimetres, the second-best candidate and its rms (-1 and inf where there is none), the counting frames, the whole
    table, and per sensor the mean distance of its counting readings to the ground-truth SURFACE in millimetres (inf
    without one; eval/surface_metrics.py, one more query on each slab's mesh, the whole mesh whatever `candidates` is).
    A site whose `rms_mm` is far above `skin_mm` is a vertex that is not under the strap.  Warns, and does not fail, about
    a sensor with no counting frame (site -1) and about two sensors on the same vertex.
    """
    samples = list(samples)
    if not samples:
        raise ValueError('search_placement needs at least one recording')
    if slab < 1:
        raise ValueError('slab must be at least one frame')
    m = np.asarray(samples[0].marker_pos_real).shape[-1] // 3
    if not per_subject:
        subjects = None
    rec = pooled_recordings(smpl_model, samples, subjects, m, normalized, device, 'search_placement')
    device = rec['device']
    out = {}
    up = lambda a: torch.from_numpy(a).to(device)
    with torch.no_grad(), torch.cuda.device(device):
        cand = Candidates.of(candidates, device)
        faces = smpl_model.surface_faces(device)
        poses_d = root_normalized_poses(smpl_model, rec, device)
        betas_d, pos_d, masks_d = up(rec['betas']), up(rec['pos']), up(rec['masks'])
        c = smpl_model.n_vertices if cand is None else len(cand)
        for key, first, n in zip(rec['keys'], rec['firsts'], rec['per_subject']):
            sums = torch.zeros(m, c, dtype=torch.float64, device=device)
            counts = torch.zeros(m, dtype=torch.int32, device=device)
            skin = torch.zeros(m, dtype=torch.float64, device=device)
            for at in range(int(first), int(first) + int(n), int(slab)):
                sl = slice(at, min(at + int(slab), int(first) + int(n)))
                vertices, _ = smpl_model(poses_body=poses_d[sl, 3:], betas=betas_d[sl], poses_root=poses_d[sl, :3])
                placement_scores(vertices, pos_d[sl], masks_d[sl], sums, counts, cand)
                read = masks_d[sl] == 1.0
                dist = closest_point_on_mesh(vertices, faces, pos_d[sl], read).dist
                skin += torch.where(read, dist.double(), torch.zeros_like(skin)).sum(dim=0)
                del vertices
            score, best, _ = placement_finish(sums, counts, cand)
            out[key] = _placement(key, score.cpu().numpy(), best.cpu().numpy(), counts.cpu().numpy(),
                                  None if cand is None else cand.host)
            n_read = out[key]['counts'].astype(np.float64)
            with np.errstate(divide='ignore', invalid='ignore'):
                out[key]['skin_mm'] = np.where(n_read > 0, 1e3 * skin.cpu().numpy() / n_read, np.inf).astype(np.float32)
    return out


def _placement(key, score, best, counts, cand_host):
    """The result of one group on the host: the runner-up from the table, the warnings."""
    m, c = score.shape
    ids = np.arange(c, dtype=np.int64) if cand_host is None else cand_host.astype(np.int64)
    runner_ids = np.full(m, -1, dtype=np.int64)
    runner = np.full(m, np.inf, dtype=np.float32)
    for k in range(m):
        if best[k] < 0 or c < 2:
            continue
        rest = score[k].copy()
        rest[np.searchsorted(ids, best[k])] = np.inf
        second = int(np.argmin(rest))            # the first of equal scores: the lowest id
        if np.isfinite(rest[second]):
            runner_ids[k], runner[k] = ids[second], rest[second]
    best_score = np.array([score[k, np.searchsorted(ids, best[k])] if best[k] >= 0 else np.inf for k in range(m)],
                          dtype=np.float32)
    unread = np.nonzero(counts == 0)[0]
    if unread.size:
        warnings.warn('placement {}: sensors {} were read in no frame; they have no site'.format(key, unread.tolist()))
    found = best[best >= 0]
    twice = sorted(set(int(v) for v in found if (found == v).sum() > 1))
    if twice:
        warnings.warn('placement {}: more than one sensor landed on vertices {} (sites {})'.format(
            key, twice, best.tolist()))
    return {'vertex_ids': best.astype(np.int64), 'rms_mm': (1e3 * np.sqrt(best_score)).astype(np.float32),
            'runner_up_ids': runner_ids, 'runner_up_rms_mm': (1e3 * np.sqrt(runner)).astype(np.float32),
            'counts': counts.astype(np.int32), 'score': score}
