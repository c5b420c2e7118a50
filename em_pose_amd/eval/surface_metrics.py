"""
Skin distance of sensor readings: how far is a reading from the surface of a body, and is it inside the body?  The one
quality figure of an estimate that needs no ground truth -- an EM sensor is strapped on top of the skin, so a reading inside
the estimated body proves the estimate wrong -- and the diagnostic the placement search and the sensor fit lacked (a
distance to the surface, not to a vertex).  This is this project's addition: the reference has no geometric query, and
both definitions are the project's own (include/empose_hip.h):

  closest point  per query p and face f the closest point c(p, f) of the closed triangle, fp32, by Voronoi regions
                 (Ericson 5.1.5); the result is the face with the lowest fp32 |p - c|^2, the lowest face id on an exact tie.
  inside         the parity of the faces the ray from p along +z crosses, float64 predicates under a half-open rule that
                 counts a ray through a shared edge or vertex once.  On a mesh that is not closed, or whose surface
                 intersects itself, the flag is still defined by the rule but means nothing -- the synthetic stand-in body
                 is a closed grid mesh whose embedding may intersect itself; the licensed body is closed and simple.

  closest_point_on_mesh        (T, V, 3) meshes, one face table, (T, Q, 3) points -> SurfaceResult of device tensors
  SMPLLayer.surface_distance   the same against the posed body, the mesh evaluated slab by slab (bodymodels/smpl.py)
  SkinDistanceEngine           the table columns over an evaluation, mergeable like the other engines
  batch_readings               the readings a preprocessed batch holds, for the engine

One HIP kernel (csrc/surface_query.hip), a workgroup per frame and block of 12 queries with the frame's vertices in LDS.
There is no CPU path: CPU tensors raise `EmposeError`.  Results are bit-identical across calls and do not depend on the
other frames, the other queries or the slab.
"""
from collections import namedtuple

import numpy as np
import torch

from em_pose_amd import _lib
from em_pose_amd.eval.metrics import MetricsEngine

SurfaceResult = namedtuple('SurfaceResult', ['dist', 'face', 'bary', 'closest', 'inside'])


class Faces(object):
    """A face table (F, 3) on the host and on a device: the host copy is what every call checks against [0, V) before
    anything is launched.  `Faces.of(faces, device)` passes a `Faces` through."""

    def __init__(self, faces, device):
        if torch.is_tensor(faces):
            faces = faces.detach().cpu().numpy()
        faces = np.asarray(faces)
        if faces.ndim != 2 or faces.shape[1] != 3 or faces.shape[0] == 0 or faces.dtype.kind not in 'iu':
            raise ValueError('faces must be a non-empty (F, 3) table of vertex ids')
        if faces.shape[0] > _lib.SURFACE_MAX_FACES:
            raise ValueError('{} faces: more than the {} a query takes'.format(faces.shape[0], _lib.SURFACE_MAX_FACES))
        if faces.min() < 0 or faces.max() >= 2 ** 31:
            raise ValueError('face indices must be non-negative and fit int32 (got {} .. {})'
                             .format(faces.min(), faces.max()))
        self.host = np.ascontiguousarray(faces, dtype=np.int32)
        self.dev = torch.from_numpy(self.host).to(device)

    @staticmethod
    def of(faces, device):
        return faces if isinstance(faces, Faces) else Faces(faces, device)

    def __len__(self):
        return self.host.shape[0]


def _query_into(vertices, faces, points, mask, out):
    """One launch: `out` a SurfaceResult of contiguous tensors for these T frames (`inside` None: not wanted)."""
    t, nv = vertices.shape[0], vertices.shape[1]
    q = points.shape[1]
    desc = _lib.SurfaceDesc()
    desc.T, desc.V, desc.F, desc.Q = t, nv, len(faces), q
    desc.vertices, desc.points, desc.mask = _lib.dptr(vertices), _lib.dptr(points), _lib.dptr(mask)
    desc.faces_host, desc.faces_dev = _lib.iptr(faces.host), _lib.dptr(faces.dev)
    desc.want_inside = int(out.inside is not None)
    desc.dist, desc.face, desc.bary = _lib.dptr(out.dist), _lib.dptr(out.face), _lib.dptr(out.bary)
    desc.closest, desc.inside = _lib.dptr(out.closest), _lib.dptr(out.inside)
    lib = _lib.lib()
    ws_bytes = lib.empose_surface_query_workspace_bytes(t, nv, len(faces), q)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=vertices.device) if ws_bytes else None
    _lib.check(lib.empose_surface_query(_lib.C.byref(desc), _lib.dptr(ws), ws_bytes, _lib.current_stream()))


def _outputs(t, q, inside, device):
    return SurfaceResult(torch.empty(t, q, dtype=torch.float32, device=device),
                         torch.empty(t, q, dtype=torch.int32, device=device),
                         torch.empty(t, q, 3, dtype=torch.float32, device=device),
                         torch.empty(t, q, 3, dtype=torch.float32, device=device),
                         torch.empty(t, q, dtype=torch.uint8, device=device) if inside else None)


def _points_and_mask(points, mask, t):
    if points.shape[0] != t:
        raise ValueError('{} frames of points for {} frames of vertices'.format(points.shape[0], t))
    points = points.detach().float().reshape(t, -1, 3).contiguous()
    q = points.shape[1]
    if q == 0:
        raise ValueError('no query points')
    if mask is not None:
        if mask.numel() != t * q:
            raise ValueError('mask must hold one value per point ({} x {})'.format(t, q))
        mask = mask.detach().float().reshape(t, q).contiguous()
    return points, mask


def closest_point_on_mesh(vertices, faces, points, mask=None, inside=False):
    """empose_surface_query on GPU tensors.  `vertices` (T, V, 3), `faces` (F, 3) integers (or a `Faces`), `points`
    (T, Q, 3) in the frame of the vertices, `mask` (T, Q) or None: a point whose mask is 0 is not queried.  Returns
    `SurfaceResult(dist (T, Q) float32, face (T, Q) int32, bary (T, Q, 3), closest (T, Q, 3), inside (T, Q) bool or None
    when not asked for)` on the device; a masked point gives +inf, -1, zeros and False, and its coordinates, NaN included,
    reach nothing.  T at most 2^22 per call, V at most 2^24, F at most 2^26, Q at most 4096: more raises, nothing is
    truncated.  A face index outside [0, V) raises `EmposeError` before anything is launched.  No autograd."""
    tensors = (vertices, points, mask)
    if any(x is not None and not x.is_cuda for x in tensors):
        raise _lib.EmposeError('closest_point_on_mesh needs GPU tensors; there is no CPU fallback')
    if vertices.dim() != 3 or vertices.shape[2] != 3:
        raise ValueError('vertices must be (T, V, 3)')
    t, dev = vertices.shape[0], vertices.device
    vertices = vertices.detach().float().contiguous()
    points, mask = _points_and_mask(points, mask, t)
    faces = Faces.of(faces, dev)
    with torch.cuda.device(dev):
        out = _outputs(t, points.shape[1], inside, dev)
        _query_into(vertices, faces, points, mask, out)
    return out._replace(inside=None if out.inside is None else out.inside.bool())


def surface_distance(smpl_model, points, poses_body, betas, poses_root=None, trans=None, mask=None, inside=True,
                     slab=1024):
    """`SMPLLayer.surface_distance` (see there)."""
    if not (poses_body.is_cuda and points.is_cuda):
        raise _lib.EmposeError('surface_distance needs GPU tensors; there is no CPU fallback')
    if slab < 1:
        raise ValueError('slab must be at least one frame')
    t, dev = poses_body.shape[0], poses_body.device
    points, mask = _points_and_mask(points, mask, t)
    per_frame = lambda x: x is not None and x.dim() == 2 and x.shape[0] == t and t > 1
    cut = lambda x, sl: x[sl] if per_frame(x) else x
    faces = smpl_model.surface_faces(dev)
    with torch.no_grad(), torch.cuda.device(dev):
        out = _outputs(t, points.shape[1], inside, dev)
        for at in range(0, t, int(slab)):
            sl = slice(at, min(at + int(slab), t))
            vertices, _ = smpl_model(poses_body=poses_body[sl], betas=cut(betas, sl), poses_root=cut(poses_root, sl),
                                     trans=cut(trans, sl))
            part = SurfaceResult(*[None if x is None else x[sl] for x in out])
            _query_into(vertices, faces, points[sl], None if mask is None else mask[sl], part)
            del vertices
    return out._replace(inside=None if out.inside is None else out.inside.bool())


def batch_readings(batch):
    """(marker_pos, marker_masks) of a batch after preprocessing: the real readings where it holds them (`RealBatch`), else
    the noisy or the plain synthetic ones (`AMASSBatch`, `SyntheticBatch`; their masks are None: every reading counts)."""
    for name in ('marker_pos_real', 'marker_pos_noisy', 'marker_pos_synth'):
        pos = getattr(batch, name, None)
        if pos is not None:
            return pos, getattr(batch, 'marker_masks', None)
    raise ValueError('the batch holds no sensor readings')


class SkinDistanceEngine(object):
    """
    `SkinDistanceEngine(smpl_model)` takes the arguments of `VertexErrorEngine.compute` plus the readings: `marker_pos`
    (N, F, M * 3) and `marker_masks` (N, F, M) as the batch holds them (`marker_pos_real`, `marker_masks`), i.e. in the
    frame in which the reconstruction energy compares them with the virtual sensors -- the body with its root orientation
    relative to the first frame and no translation, the convention of `vis.compare.sensor_overlays` and
    `data.offsets.estimate_offsets`.  A reading counts when its mask is 1 and its frame lies within `seq_lengths` (and
    within `valid`, when given); `frame_mask`, which drops whole frames for the other engines, is accepted and not used:
    the readings that exist are the ones to measure.

    Per `compute` two queries (`SMPLLayer.surface_distance`): the readings against the estimate and against the ground
    truth.  Per frame the host keeps one float64 row (readings, sum of distances to the estimate, readings inside it, sum
    of the distances of those, sum of distances to the ground truth, readings inside it), summed over the frame's sensors
    in ascending order; these rows are the mergeable state (`state` / `merge` / `gather`).  `get_metrics`:
      'Skin dist [mm]'     mean unsigned distance of the readings to the estimate's surface
      'Skin dist GT [mm]'  the same to the ground-truth body
      'Inside [%]'         share of the readings inside the estimate
      'Inside GT [%]'      ... inside the ground-truth body
      'Depth [mm]'         mean distance of the readings inside the estimate, 0 when there are none
    NaN without a single reading.  'Inside' is the parity flag and means something on a closed, simple surface only.
    """
    WIDTH = 6
    COLUMNS = ('Skin dist [mm]', 'Skin dist GT [mm]', 'Inside [%]', 'Inside GT [%]', 'Depth [mm]')

    def __init__(self, smpl_model, slab=1024):
        self.smpl_model = smpl_model
        self.slab = int(slab)
        self.reset()

    def reset(self):
        self._sums = []       # host rows, (m, 6) float64 each
        self._pending = []    # device (count, dist_hat, inside_hat, dist, inside) of `compute` calls not read yet

    @property
    def sums(self):
        self._flush()
        return self._sums

    # ---- accumulation -------------------------------------------------------------------------------------------
    def compute(self, pose, shape, pose_hat, shape_hat=None, seq_lengths=None, pose_root=None, pose_root_hat=None,
                frame_mask=None, valid=None, marker_pos=None, marker_masks=None):
        if marker_pos is None:
            raise ValueError('SkinDistanceEngine.compute needs the readings (marker_pos)')
        n, f = pose.shape[0], pose.shape[1]
        shape_hat = shape if shape_hat is None else shape_hat
        frames = valid if valid is not None else MetricsEngine._mask(seq_lengths, n, f, None, pose.device)
        flat = lambda t: t.reshape(n * f, -1)
        per_frame = lambda s_: flat(s_) if s_.dim() == 3 else flat(s_.unsqueeze(1).expand(n, f, s_.shape[-1]))
        points = marker_pos.reshape(n * f, -1, 3).float()
        m = points.shape[1]
        count = frames.reshape(n * f, 1).expand(n * f, m)
        if marker_masks is not None:
            count = torch.logical_and(count, marker_masks.reshape(n * f, m) == 1)
        count = count.float().contiguous()
        root_f = None if pose_root is None else flat(pose_root)
        root_hat_f = None if pose_root is None else flat(pose_root_hat)
        hat = self.smpl_model.surface_distance(points, flat(pose_hat), per_frame(shape_hat), poses_root=root_hat_f,
                                               mask=count, inside=True, slab=self.slab)
        gt = self.smpl_model.surface_distance(points, flat(pose), per_frame(shape), poses_root=root_f, mask=count,
                                              inside=True, slab=self.slab)
        self._pending.append((count, hat.dist, hat.inside, gt.dist, gt.inside))

    @staticmethod
    def rows_from(count, dist_hat, inside_hat, dist, inside):
        """Host arithmetic of one `compute`: (T, M) arrays -> (frames with a reading, 6) float64, the sensors summed in
        ascending order."""
        on = np.asarray(count) != 0
        rows = np.zeros((on.shape[0], SkinDistanceEngine.WIDTH), dtype=np.float64)
        d_hat = np.where(on, np.asarray(dist_hat, dtype=np.float64), 0.0)
        d_gt = np.where(on, np.asarray(dist, dtype=np.float64), 0.0)
        in_hat = on & (np.asarray(inside_hat) != 0)
        in_gt = on & (np.asarray(inside) != 0)
        for k in range(on.shape[1]):
            rows[:, 0] += on[:, k]
            rows[:, 1] += d_hat[:, k]
            rows[:, 2] += in_hat[:, k]
            rows[:, 3] += np.where(in_hat[:, k], d_hat[:, k], 0.0)
            rows[:, 4] += d_gt[:, k]
            rows[:, 5] += in_gt[:, k]
        return rows[rows[:, 0] > 0]

    def _flush(self):
        pending, self._pending = self._pending, []
        for parts in pending:
            rows = self.rows_from(*[p.cpu().numpy() for p in parts])
            if rows.shape[0]:
                self._sums.append(rows)

    # ---- mergeable state ------------------------------------------------------------------------------------------
    def state(self):
        return {'sums': np.concatenate(self.sums, axis=0) if self.sums else np.zeros((0, self.WIDTH))}

    def merge(self, state):
        rows = np.asarray(state['sums'], dtype=np.float64).reshape(-1, self.WIDTH)
        if rows.shape[0]:
            self.sums.append(rows)

    def gather(self, group=None, device=None, force=False):
        """Combine the rows of all ranks (torch.distributed), concatenated in rank order, as `VertexErrorEngine.gather`."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()) or (dist.get_world_size(group) == 1 and not force):
            return self
        world = dist.get_world_size(group)
        dev = torch.device('cpu') if device is None else device
        mine = torch.from_numpy(self.state()['sums']).to(dev)
        count = torch.tensor([mine.shape[0]], dtype=torch.int64, device=dev)
        counts = [torch.zeros_like(count) for _ in range(world)]
        dist.all_gather(counts, count, group=group)
        counts = [int(c.item()) for c in counts]
        padded = torch.zeros(max(max(counts), 1), self.WIDTH, dtype=torch.float64, device=dev)
        padded[:mine.shape[0]] = mine
        parts = [torch.zeros_like(padded) for _ in range(world)]
        dist.all_gather(parts, padded, group=group)
        merged = np.concatenate([p[:c].cpu().numpy() for p, c in zip(parts, counts)], axis=0)
        self.reset()
        self.merge({'sums': merged})
        return self

    # ---- reduction ------------------------------------------------------------------------------------------------
    @staticmethod
    def metrics_from_rows(rows):
        out = {name: float('nan') for name in SkinDistanceEngine.COLUMNS}
        rows = np.asarray(rows, dtype=np.float64).reshape(-1, SkinDistanceEngine.WIDTH)
        n, d_hat, n_in, depth, d_gt, n_in_gt = rows.sum(axis=0)   # one reduction over the rows in their order
        if n > 0:
            out['Skin dist [mm]'] = float(1e3 * d_hat / n)
            out['Skin dist GT [mm]'] = float(1e3 * d_gt / n)
            out['Inside [%]'] = float(1e2 * n_in / n)
            out['Inside GT [%]'] = float(1e2 * n_in_gt / n)
            out['Depth [mm]'] = float(1e3 * depth / n_in) if n_in > 0 else 0.0
        return out

    def get_metrics(self):
        return self.metrics_from_rows(np.concatenate(self.sums, axis=0) if self.sums else np.zeros((0, self.WIDTH)))

    @staticmethod
    def to_pretty_string(metrics, model_name):
        from tabulate import tabulate
        return tabulate([[model_name] + list(metrics.values())], headers=['Model'] + list(metrics.keys()))
