"""
Temporal metrics: the acceleration error and the jitter (mean jerk) of an estimate over sequences -- what the per-frame
columns of `MetricsEngine` (MPJPE, PA-MPJPE, MPJAE) and `VertexErrorEngine` (PVE) cannot see.  An estimate that trembles by
a centimetre around the truth has the MPJPE of one that is steadily a centimetre off; the recurrent model (LGD-RNN against
LGD) exists for the difference.

These metrics are this project's addition: the reference has no temporal metric.  The definitions below are this project's
own; the columns follow the conventions of the reference's other columns.

For a point x[t] (metres) at `fps` frames per second (default `C.FPS` = 60), with backward stencils, so that a chunked
driver only ever needs context on the left:
  acc[t]  = (x[t] - 2 x[t-1] + x[t-2]) fps^2               defined where frames t-2 .. t all count
  jerk[t] = (x[t] - 3 x[t-1] + 3 x[t-2] - x[t-3]) fps^3    defined where frames t-3 .. t all count
A frame counts exactly when `MetricsEngine` counts it (inside `seq_lengths`, no sensor missing).  A stencil never reaches
across a frame that does not count and never across two sequences.  Per (frame, point): |acc_gt - acc_hat| (m/s^2),
|jerk_hat| and |jerk_gt| (m/s^3) -- real ground truth has jitter of its own, and the estimate's figure means little without
it.  One HIP kernel produces them (`empose_temporal_rows`, csrc/temporal.hip: fp32 in, float64 arithmetic).

`TemporalMetricsEngine(smpl_model)` takes the arguments of `MetricsEngine.compute` and `is_new_sequence`, with the meaning
it has in `net(chunk, is_new_sequence=)`: with False, batch row i continues row i of the previous call (the batched
driver's convention: the rows that go on are the first k).  The engine keeps the last three frames of every row on the
device and prepends them to the next call, so feeding a sequence in chunks accumulates the same rows, bit for bit, as
feeding it whole.  `get_metrics`:
  joints (the 22 of `fk_joints`):  'Accel [m/s^2]', 'Jitter [m/s^3]', 'Jitter GT [m/s^3]', each with its STD -- the mean over
      frames per joint, then over `EUCL_EVAL_JOINTS`; the STD is `np.std` over all selected (frame, joint) entries, as MPJPE.
      The frame sets differ: the frames where acc is defined, and those where jerk is.
  surface (`surface=True`, all vertices of the layer, or of a `SubMeshLayer`): 'V-Accel [m/s^2]', 'V-Jitter [m/s^3]',
      'V-Jitter GT [m/s^3]', each with its STD, from per-frame sums and sums of squares over the vertices in float64, as
      `VertexErrorEngine.get_metrics`.  Joint positions are blind to rotation about a bone's own axis; the vertices see it.
A family without a defined frame is NaN, not 0.  The accumulator is a mergeable value (`state` / `merge` / `gather`).
`compute_points` is the same bookkeeping on points the caller already has; on CPU tensors it takes the NumPy float64
path below (the same algorithm as the kernel), which is the only CPU path: `compute` on CPU tensors raises as the layer does.
"""
import numpy as np
import torch

from em_pose_amd import _lib
from em_pose_amd.eval.metrics import EUCL_EVAL_JOINTS, MetricsEngine
from em_pose_amd.helpers.configuration import CONSTANTS as C

LEAD = 3   # frames of context a stencil needs on the left

JOINT_KEYS = ('accel', 'jitter', 'jitter_gt')
SURFACE_KEYS = ('v_accel', 'v_jitter', 'v_jitter_gt')
JOINT_COLUMNS = ('Accel [m/s^2]', 'Accel STD', 'Jitter [m/s^3]', 'Jitter STD', 'Jitter GT [m/s^3]', 'Jitter GT STD')
SURFACE_COLUMNS = ('V-Accel [m/s^2]', 'V-Accel STD', 'V-Jitter [m/s^3]', 'V-Jitter STD', 'V-Jitter GT [m/s^3]',
                   'V-Jitter GT STD')


def temporal_rows_numpy(x_gt, x_hat, valid, fps):
    """The kernel's per-point form in NumPy float64: x_gt, x_hat (n, f, P, 3), valid (n, f) ->
    rows (n, f, 3 P) = |acc_gt - acc_hat| | |jerk_hat| | |jerk_gt| (0 where undefined), defined (n, f) uint8 (bit 0: acc,
    bit 1: jerk)."""
    g, h = np.asarray(x_gt, dtype=np.float64), np.asarray(x_hat, dtype=np.float64)
    v = np.asarray(valid).reshape(g.shape[:2]) != 0
    n, f, P = g.shape[:3]
    fps2, fps3 = float(fps) * float(fps), float(fps) * float(fps) * float(fps)
    rows = np.zeros((n, f, 3 * P))
    defined = np.zeros((n, f), dtype=np.uint8)
    norm = lambda d: np.sqrt((d * d).sum(axis=-1))
    with np.errstate(invalid='ignore', over='ignore'):   # a frame that does not count may hold anything
        if f >= 3:
            ok = v[:, 2:] & v[:, 1:-1] & v[:, :-2]
            acc = lambda x: ((x[:, 2:] - 2.0 * x[:, 1:-1]) + x[:, :-2]) * fps2
            rows[:, 2:, :P] = np.where(ok[..., None], norm(acc(g) - acc(h)), 0.0)
            defined[:, 2:] |= ok.astype(np.uint8) * _lib.TEMPORAL_ACC
        if f >= 4:
            ok = v[:, 3:] & v[:, 2:-1] & v[:, 1:-2] & v[:, :-3]
            jerk = lambda x: (((x[:, 3:] - 3.0 * x[:, 2:-1]) + 3.0 * x[:, 1:-2]) - x[:, :-3]) * fps3
            rows[:, 3:, P:2 * P] = np.where(ok[..., None], norm(jerk(h)), 0.0)
            rows[:, 3:, 2 * P:] = np.where(ok[..., None], norm(jerk(g)), 0.0)
            defined[:, 3:] |= ok.astype(np.uint8) * _lib.TEMPORAL_JERK
    return rows, defined


def temporal_rows(x_gt, x_hat, valid, fps, reduce=False):
    """`empose_temporal_rows` on device tensors: x_gt, x_hat (n, f, P, 3) float32, valid (n, f) ->
    rows (n, f, 3 P) float64 (`reduce`: (n, f, 6), per quantity the sum over the points and the sum of squares) and
    defined (n, f) uint8, both on the device; nothing waits for it."""
    n, f, P = x_gt.shape[:3]
    dev = x_gt.device
    x_gt, x_hat = x_gt.to(torch.float32).contiguous(), x_hat.to(torch.float32).contiguous()
    valid = valid.reshape(n, f).to(device=dev, dtype=torch.uint8).contiguous()
    rows = torch.empty(n, f, 6 if reduce else 3 * P, dtype=torch.float64, device=dev)
    defined = torch.empty(n, f, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().empose_temporal_rows(n, f, P, _lib.dptr(x_gt), _lib.dptr(x_hat), _lib.dptr(valid), float(fps),
                                                   1 if reduce else 0, _lib.dptr(rows), _lib.dptr(defined),
                                                   _lib.current_stream()))
    return rows, defined


class TemporalMetricsEngine(object):
    def __init__(self, smpl_model, fps=C.FPS, surface=False, slab_frames=1024):
        """`smpl_model`: an `SMPLLayer`, or a `SubMeshLayer` for the surface figures over its vertex subset (None: only
        `compute_points`).  `slab_frames`: with `surface`, the frames of mesh per body that are live at a time."""
        if not (float(fps) > 0.0 and np.isfinite(float(fps))):
            raise ValueError('fps must be positive and finite')
        if int(slab_frames) <= LEAD:
            raise ValueError('slab_frames must be above {}: a slab carries {} frames of lead-in'.format(LEAD, LEAD))
        self.smpl_model = smpl_model
        self.fps = float(fps)
        self.surface = bool(surface)
        self.slab_frames = int(slab_frames)
        self.eucl_idxs = [C.SMPL_JOINTS.index(j) for j in EUCL_EVAL_JOINTS]
        self.reset()

    @property
    def n_vertices(self):
        return int(self.smpl_model.n_vertices)

    @property
    def keys(self):
        return JOINT_KEYS + (SURFACE_KEYS if self.surface else ())

    def reset(self):
        self._store = {k: [] for k in JOINT_KEYS + SURFACE_KEYS}   # host rows per family
        self._groups = []     # calls not read yet: [[(rows, vrows or None, defined), ...] per sequence group]
        self._carry = None    # the last three frames of every row of the previous call
        self._points = None   # points per joint row (22 from `compute`)

    # ---- accumulation -------------------------------------------------------------------------------------------
    def _begin(self, kind, n, is_new_sequence):
        """The carried frames of this call's rows (None: a new sequence); opens a group of calls for a new sequence."""
        if is_new_sequence:
            self._carry = None
            self._groups.append([])
            return None
        carry = self._carry
        if carry is None:
            raise ValueError('is_new_sequence=False, but there is no previous call to continue')
        if carry['kind'] != kind:
            raise ValueError('is_new_sequence=False continues a `{}` call, not a `{}` call'.format(carry['kind'], kind))
        if n > carry['n']:
            raise ValueError('is_new_sequence=False with {} rows, the previous call had {}: the rows that go on are the '
                             'first k'.format(n, carry['n']))
        if not self._groups:          # the accumulators were read in the middle of the sequence
            self._groups.append([])
        return carry

    def _queue(self, rows, vrows, defined, points):
        if self._points is None:
            self._points = points
        elif self._points != points:
            raise ValueError('rows of {} points cannot join rows of {} points'.format(points, self._points))
        drop = lambda t: None if t is None else t[:, LEAD:]     # the prepended frames are not counted twice
        self._groups[-1].append((drop(rows), drop(vrows), drop(defined)))

    def compute_points(self, x_gt, x_hat, valid=None, is_new_sequence=True):
        """Points the caller already has: x_gt, x_hat (n, f, P, 3), valid (n, f) or None (every frame counts).  GPU
        tensors take the kernel, CPU tensors the NumPy float64 path.  Feeds the joint columns (all P points are averaged
        unless P is 22)."""
        n, f, P = int(x_gt.shape[0]), int(x_gt.shape[1]), int(x_gt.shape[2])
        if tuple(x_gt.shape) != (n, f, P, 3) or tuple(x_hat.shape) != (n, f, P, 3):
            raise ValueError('x_gt and x_hat must both be (n, f, P, 3)')
        dev = x_gt.device
        carry = self._begin('points', n, is_new_sequence)
        v = torch.ones(n, f, dtype=torch.bool, device=dev) if valid is None else valid.reshape(n, f).to(dev) != 0
        if carry is None:
            tail = [torch.zeros(n, LEAD, P, 3, dtype=torch.float32, device=dev)] * 2
            tail_v = torch.zeros(n, LEAD, dtype=torch.bool, device=dev)
        else:
            tail, tail_v = [t[:n] for t in carry['fields']], carry['valid'][:n]
        g = torch.cat([tail[0], x_gt.detach().to(torch.float32)], dim=1)
        h = torch.cat([tail[1], x_hat.detach().to(torch.float32)], dim=1)
        ev = torch.cat([tail_v, v], dim=1)
        self._carry = {'kind': 'points', 'n': n, 'fields': [g[:, -LEAD:], h[:, -LEAD:]], 'valid': ev[:, -LEAD:]}
        if dev.type == 'cuda':
            rows, defined = temporal_rows(g, h, ev, self.fps)
        else:
            rows, defined = temporal_rows_numpy(g.numpy(), h.numpy(), ev.numpy(), self.fps)
            rows, defined = torch.from_numpy(rows), torch.from_numpy(defined)
        self._queue(rows, None, defined, P)

    def compute(self, pose, shape, pose_hat, shape_hat=None, seq_lengths=None, pose_root=None, pose_root_hat=None,
                frame_mask=None, valid=None, is_new_sequence=True):
        """Same arguments as `MetricsEngine.compute`, same frames counted, plus `is_new_sequence` (module docstring).
        One `fk_joints` launch over ground truth and estimate together and one `empose_temporal_rows` launch; with
        `surface` the vertices of both bodies from the layer's forward, slab after slab.  The rows stay on the device
        until the accumulators are read: nothing here waits for the device."""
        if not (pose.is_cuda and pose_hat.is_cuda):
            raise _lib.EmposeError('TemporalMetricsEngine.compute needs GPU tensors; there is no CPU fallback '
                                   '(`compute_points` takes points on the CPU)')
        n, f, dev = int(pose.shape[0]), int(pose.shape[1]), pose.device
        carry = self._begin('pose', n, is_new_sequence)
        shape_hat = shape if shape_hat is None else shape_hat
        mask = valid if valid is not None else MetricsEngine._mask(seq_lengths, n, f, frame_mask, dev)
        mask = mask.reshape(n, f).to(dev) != 0
        per_frame = lambda s_: s_ if s_.dim() == 3 else s_.unsqueeze(1).expand(n, f, s_.shape[-1])
        zeros = torch.zeros(n, f, 3, dtype=torch.float32, device=dev)
        given = [pose[..., :C.N_JOINTS * 3], pose_hat[..., :C.N_JOINTS * 3], per_frame(shape), per_frame(shape_hat),
                 zeros if pose_root is None else pose_root, zeros if pose_root is None else pose_root_hat]
        given = [t.detach().to(torch.float32) for t in given]
        if carry is None:
            tail = [torch.zeros(n, LEAD, t.shape[-1], dtype=torch.float32, device=dev) for t in given]
            tail_v = torch.zeros(n, LEAD, dtype=torch.bool, device=dev)
        else:
            tail, tail_v = [t[:n] for t in carry['fields']], carry['valid'][:n]
        ext = [torch.cat([t, x], dim=1) for t, x in zip(tail, given)]
        ev = torch.cat([tail_v, mask], dim=1)
        fe = f + LEAD
        # the last three frames inside `seq_lengths`: frames lens .. lens + 2 of the extended rows (torch only, no sync)
        lens = torch.full((n,), f, dtype=torch.int64, device=dev) if seq_lengths is None else \
            seq_lengths.reshape(n).to(device=dev, dtype=torch.int64).clamp(0, f)
        at = lens[:, None] + torch.arange(LEAD, device=dev)[None, :]
        take = lambda t: t.gather(1, at[:, :, None].expand(n, LEAD, t.shape[-1]))
        self._carry = {'kind': 'pose', 'n': n, 'fields': [take(t) for t in ext], 'valid': ev.gather(1, at)}

        flat = lambda t: t.reshape(n * fe, -1)
        both = self.smpl_model.fk_joints(torch.cat([flat(ext[0]), flat(ext[1])]), torch.cat([flat(ext[2]), flat(ext[3])]),
                                         poses_root=torch.cat([flat(ext[4]), flat(ext[5])]))
        P = both.shape[1]
        rows, defined = temporal_rows(both[:n * fe].reshape(n, fe, P, 3), both[n * fe:].reshape(n, fe, P, 3), ev, self.fps)
        vrows = self._surface_rows(ext, ev, n, fe) if self.surface else None
        self._queue(rows, vrows, defined, P)

    def _surface_rows(self, ext, ev, n, fe):
        """(n, fe, 6) float64: the reduced rows over the layer's vertices, from at most `slab_frames` frames of mesh per
        body at a time.  Whole rows go into a slab when they fit; a longer row is cut in time with three frames of overlap.
        A frame's row depends only on its own four frames, so the result does not depend on `slab_frames`."""
        out = torch.empty(n, fe, 6, dtype=torch.float64, device=ev.device)

        def slab(r0, r1, t0, t1):
            cut = lambda t: t[r0:r1, t0:t1].reshape((r1 - r0) * (t1 - t0), -1)
            mesh = lambda p, s_, r: self.smpl_model(cut(p), cut(s_), poses_root=cut(r))[0].reshape(
                r1 - r0, t1 - t0, -1, 3)
            rows, _ = temporal_rows(mesh(ext[0], ext[2], ext[4]), mesh(ext[1], ext[3], ext[5]), ev[r0:r1, t0:t1], self.fps,
                                    reduce=True)
            return rows
        if fe <= self.slab_frames:
            per_slab = self.slab_frames // fe
            for r0 in range(0, n, per_slab):
                r1 = min(n, r0 + per_slab)
                out[r0:r1] = slab(r0, r1, 0, fe)
        else:
            for r in range(n):
                t0 = 0
                while True:
                    t1 = min(t0 + self.slab_frames, fe)
                    keep = 0 if t0 == 0 else LEAD     # the overlap is the lead-in of the next piece
                    out[r, t0 + keep:t1] = slab(r, r + 1, t0, t1)[0, keep:]
                    if t1 == fe:
                        break
                    t0 = t1 - LEAD
        return out

    def _flush(self):
        """Device rows of earlier calls -> the host accumulators.  Within a sequence group (a call with
        `is_new_sequence=True` and the calls that continue it) the rows are put in batch-row order, each row's frames in
        call order: what one call over the whole sequences leaves."""
        groups, self._groups = self._groups, []
        P = self._points
        for calls in groups:
            if not calls:
                continue
            host = [(r.cpu().numpy(), None if vr is None else vr.cpu().numpy(), d.cpu().numpy()) for r, vr, d in calls]
            for i in range(host[0][0].shape[0]):
                for rows, vrows, defined in host:
                    if i >= rows.shape[0]:
                        continue
                    acc = (defined[i] & _lib.TEMPORAL_ACC) != 0
                    jerk = (defined[i] & _lib.TEMPORAL_JERK) != 0
                    picks = [('accel', rows[i][acc][:, :P]), ('jitter', rows[i][jerk][:, P:2 * P]),
                             ('jitter_gt', rows[i][jerk][:, 2 * P:])]
                    if vrows is not None:
                        picks += [('v_accel', vrows[i][acc][:, 0:2]), ('v_jitter', vrows[i][jerk][:, 2:4]),
                                  ('v_jitter_gt', vrows[i][jerk][:, 4:6])]
                    for key, part in picks:
                        if part.shape[0]:
                            self._store[key].append(part)

    def _rows_of(self, key):
        self._flush()
        width = 2 if key in SURFACE_KEYS else (self._points or C.N_JOINTS + 1)
        parts = self._store[key]
        if len(parts) > 1:     # keep one block per family
            parts[:] = [np.concatenate(parts, axis=0)]
        return np.ascontiguousarray(parts[0]) if parts else np.zeros((0, width))

    # ---- mergeable state ------------------------------------------------------------------------------------------
    def state(self):
        """{'accel' (m_a, P), 'jitter' (m_j, P), 'jitter_gt' (m_j, P)} float64 per-point rows of the frames where acc /
        jerk is defined; with `surface` also 'v_accel' (m_a, 2), 'v_jitter' (m_j, 2), 'v_jitter_gt' (m_j, 2): per frame
        the sum over the vertices and the sum of squares."""
        return {k: self._rows_of(k) for k in self.keys}

    def merge(self, state):
        missing = [k for k in self.keys if k not in state]
        if missing:
            raise ValueError('the state lacks {}'.format(missing))
        parts = {k: np.asarray(state[k], dtype=np.float64) for k in self.keys}
        if any(v.ndim != 2 for v in parts.values()):
            raise ValueError('every family of a state is a (frames, width) array')
        if parts['jitter'].shape != parts['jitter_gt'].shape:
            raise ValueError("'jitter' and 'jitter_gt' count different frames")
        if self.surface and (parts['v_accel'].shape[0] != parts['accel'].shape[0] or
                             parts['v_jitter'].shape[0] != parts['jitter'].shape[0] or
                             parts['v_jitter_gt'].shape[0] != parts['jitter'].shape[0]):
            raise ValueError('the surface rows and the joint rows count different frames')
        self._flush()
        for k in JOINT_KEYS:
            if parts[k].shape[0]:
                if self._points is None:
                    self._points = parts[k].shape[1]
                elif self._points != parts[k].shape[1]:
                    raise ValueError('rows of {} points cannot join rows of {} points'.format(parts[k].shape[1],
                                                                                              self._points))
        for k, v in parts.items():
            if v.shape[0]:
                self._store[k].append(v)

    def gather(self, group=None, device=None, force=False):
        """Combine the rows of all ranks (torch.distributed), concatenated in rank order, as `MetricsEngine.gather`;
        `force` runs the collectives even in a group of one."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()) or (dist.get_world_size(group) == 1 and not force):
            return self
        world = dist.get_world_size(group)
        st = self.state()
        dev = torch.device('cpu') if device is None else device
        # (a rank without rows does not know the width: the widest of all ranks is everybody's)
        width = torch.tensor([self._points or 0], dtype=torch.int64, device=dev)
        widths = [torch.zeros_like(width) for _ in range(world)]
        dist.all_gather(widths, width, group=group)
        points = max(int(w.item()) for w in widths)
        merged = {}
        for key in self.keys:
            w = 2 if key in SURFACE_KEYS else max(points, 1)
            mine = torch.from_numpy(st[key]).to(dev)
            count = torch.tensor([mine.shape[0]], dtype=torch.int64, device=dev)
            counts = [torch.zeros_like(count) for _ in range(world)]
            dist.all_gather(counts, count, group=group)
            counts = [int(c.item()) for c in counts]
            padded = torch.zeros(max(max(counts), 1), w, dtype=torch.float64, device=dev)
            if mine.shape[0]:
                padded[:mine.shape[0]] = mine
            parts = [torch.zeros_like(padded) for _ in range(world)]
            dist.all_gather(parts, padded, group=group)
            merged[key] = np.concatenate([p[:c].cpu().numpy() for p, c in zip(parts, counts)], axis=0)
        self.reset()
        self.merge(merged)
        return self

    # ---- reduction ------------------------------------------------------------------------------------------------
    def get_metrics(self, eucl_idxs_select=True):
        nan = float('nan')
        out = {name: nan for name in JOINT_COLUMNS + (SURFACE_COLUMNS if self.surface else ())}
        for i, key in enumerate(JOINT_KEYS):
            a = self._rows_of(key)
            if a.shape[0]:
                select = eucl_idxs_select and a.shape[1] == C.N_JOINTS + 1
                idx = self.eucl_idxs if select else list(range(a.shape[1]))
                out[JOINT_COLUMNS[2 * i]] = float(np.mean(np.mean(a, axis=0)[idx]))
                out[JOINT_COLUMNS[2 * i + 1]] = float(np.std(a[:, idx]))
        if self.surface:
            for i, key in enumerate(SURFACE_KEYS):
                rows = self._rows_of(key)
                if rows.shape[0]:
                    count = float(rows.shape[0]) * self.n_vertices
                    mean = rows[:, 0].sum() / count
                    var = max(rows[:, 1].sum() / count - mean * mean, 0.0)
                    out[SURFACE_COLUMNS[2 * i]] = float(mean)
                    out[SURFACE_COLUMNS[2 * i + 1]] = float(np.sqrt(var))
        return out

    @staticmethod
    def to_pretty_string(metrics, model_name):
        from tabulate import tabulate
        return tabulate([[model_name] + list(metrics.values())], headers=['Model'] + list(metrics.keys()))
