"""
Mean per-vertex error, PVE (also MPVPE): the distance between the posed surface of the ground truth and of the estimate,
averaged over the vertices of the body model -- the surface counterpart of `MetricsEngine`'s MPJPE.  A wrong `shape_hat`
moves the 22 joints by millimetres and the surface by centimetres, so this is the figure that sees the shape.

This metric is this project's addition: the reference evaluates joints only (eval/metrics.py) and has nothing to pin a
vertex error to beyond the body model itself; the conventions below follow the reference's other columns.

`VertexErrorEngine(smpl_model)` takes the arguments of `MetricsEngine.compute` and counts the same frames.  Per frame
the device returns two numbers, the sum over the V vertices of |v - v_hat| and of |v - v_hat|^2
(`SMPLLayer.vertex_error`: one fused HIP kernel evaluates both bodies and keeps only the distance, neither mesh is
written).  These (frames, 2) float64 rows are the accumulator -- a mergeable value like `MetricsEngine`'s (`state` /
`merge` / `gather` for a sequence-sharded evaluation).  `get_metrics`:
  'PVE [mm]'  sum of all distances / (frames * V)
  'PVE STD'   the standard deviation over all (frame, vertex) distances, as the reference's STD columns are `np.std` over
              all entries -- here from the two moments, in float64: sqrt(sum d^2 / n - mean^2)
`VertexErrorEngine(smpl_model, procrustes=True)` adds the Procrustes-aligned error, PA-PVE (PA-MPVPE), as PA-MPJPE
stands beside MPJPE: the same distances after the similarity transform that best maps the estimate's vertices onto the
ground truth's (the convention of `eval/metrics.py procrustes_align`).  A globally rotated but correctly posed and shaped
body has a large PVE and a PA-PVE near zero.  Still one call to the layer per `compute` (`vertex_error(...,
procrustes=True)`, four numbers per frame); the second pair of columns is kept as 'sums_pa' beside an unchanged 'sums',
and `get_metrics` appends 'PA-PVE [mm]' and 'PA-PVE STD' with the conventions above.  Also this project's addition.
There is no CPU path: the layer refuses CPU tensors.
"""
import numpy as np
import torch

from em_pose_amd.eval.metrics import MetricsEngine


class VertexErrorEngine(object):
    def __init__(self, smpl_model, procrustes=False):
        """`smpl_model`: an `SMPLLayer`, or a `SubMeshLayer` for the error over its vertex subset."""
        self.smpl_model = smpl_model
        self.procrustes = bool(procrustes)
        self.reset()

    @property
    def n_vertices(self):
        return int(self.smpl_model.n_vertices)

    def reset(self):
        self._sums = []       # host rows, (m, 2) float64 each -- (m, 4) with `procrustes`: sums | sums_pa
        self._pending = []    # (device rows (n * f, 2), valid (n * f,) bool) of `compute` calls not read yet

    @property
    def sums(self):
        self._flush()
        return self._sums

    # ---- accumulation -------------------------------------------------------------------------------------------
    def compute(self, pose, shape, pose_hat, shape_hat=None, seq_lengths=None, pose_root=None, pose_root_hat=None,
                frame_mask=None, valid=None):
        """Same arguments as `MetricsEngine.compute`, same frames counted.  One launch over all n * f frames; the rows
        stay on the device with their `valid` mask and the valid ones are picked when the accumulator is first read, so
        nothing here waits for the device."""
        n, f = pose.shape[0], pose.shape[1]
        shape_hat = shape if shape_hat is None else shape_hat
        mask = valid if valid is not None else MetricsEngine._mask(seq_lengths, n, f, frame_mask, pose.device)
        flat = lambda t: t.reshape(n * f, -1)
        per_frame = lambda s_: flat(s_) if s_.dim() == 3 else flat(s_.unsqueeze(1).expand(n, f, s_.shape[-1]))
        root_f = None if pose_root is None else flat(pose_root)
        root_hat_f = None if pose_root is None else flat(pose_root_hat)
        kw = {'procrustes': True} if self.procrustes else {}
        rows = self.smpl_model.vertex_error(flat(pose), per_frame(shape), flat(pose_hat), per_frame(shape_hat),
                                            poses_root=root_f, poses_root_hat=root_hat_f, **kw)
        self._pending.append((rows, mask.reshape(n * f)))

    def _flush(self):
        pending, self._pending = self._pending, []
        for rows, valid in pending:
            idx = np.flatnonzero(valid.cpu().numpy())
            if idx.shape[0] == 0:
                continue
            if idx.shape[0] != rows.shape[0]:
                rows = rows.index_select(0, torch.from_numpy(idx).to(rows.device))
            self._sums.append(rows.cpu().numpy())

    # ---- mergeable state ------------------------------------------------------------------------------------------
    @property
    def _width(self):
        return 4 if self.procrustes else 2

    def state(self):
        rows = np.concatenate(self.sums, axis=0) if self.sums else np.zeros((0, self._width))
        if not self.procrustes:
            return {'sums': rows}
        return {'sums': np.ascontiguousarray(rows[:, :2]), 'sums_pa': np.ascontiguousarray(rows[:, 2:])}

    def merge(self, state):
        rows = np.asarray(state['sums'], dtype=np.float64).reshape(-1, 2)
        if self.procrustes:
            if 'sums_pa' not in state:
                raise ValueError("a state without 'sums_pa' cannot be merged into a Procrustes engine")
            rows_pa = np.asarray(state['sums_pa'], dtype=np.float64).reshape(-1, 2)
            if rows_pa.shape[0] != rows.shape[0]:
                raise ValueError("'sums' and 'sums_pa' count different frames")
            rows = np.concatenate([rows, rows_pa], axis=1)
        if rows.shape[0]:
            self.sums.append(rows)

    def gather(self, group=None, device=None, force=False):
        """Combine the rows of all ranks (torch.distributed), concatenated in rank order, as `MetricsEngine.gather`;
        `force` runs the collectives even in a group of one."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()) or (dist.get_world_size(group) == 1 and not force):
            return self
        world = dist.get_world_size(group)
        dev = torch.device('cpu') if device is None else device
        w = self._width
        mine = torch.from_numpy(np.concatenate(list(self.state().values()), axis=1)).to(dev)
        count = torch.tensor([mine.shape[0]], dtype=torch.int64, device=dev)
        counts = [torch.zeros_like(count) for _ in range(world)]
        dist.all_gather(counts, count, group=group)
        counts = [int(c.item()) for c in counts]
        padded = torch.zeros(max(max(counts), 1), w, dtype=torch.float64, device=dev)
        padded[:mine.shape[0]] = mine
        parts = [torch.zeros_like(padded) for _ in range(world)]
        dist.all_gather(parts, padded, group=group)
        merged = np.concatenate([p[:c].cpu().numpy() for p, c in zip(parts, counts)], axis=0)
        self.reset()
        self.merge({'sums': merged[:, :2], 'sums_pa': merged[:, 2:]} if self.procrustes else {'sums': merged})
        return self

    # ---- reduction ------------------------------------------------------------------------------------------------
    def get_metrics(self):
        # NaN, not 0, without a single accumulated row (as MetricsEngine: "0 mm" reads as a perfect score)
        names = ['PVE'] + (['PA-PVE'] if self.procrustes else [])
        out = {}
        for name in names:
            out[name + ' [mm]'] = out[name + ' STD'] = float('nan')
        if self.sums:
            rows = np.concatenate(self.sums, axis=0)
            count = float(rows.shape[0]) * self.n_vertices
            for i, name in enumerate(names):
                mean = rows[:, 2 * i].sum() / count
                var = max(rows[:, 2 * i + 1].sum() / count - mean * mean, 0.0)
                out[name + ' [mm]'] = float(mean * 1000.0)
                out[name + ' STD'] = float(np.sqrt(var) * 1000.0)
        return out

    @staticmethod
    def to_pretty_string(metrics, model_name):
        from tabulate import tabulate
        return tabulate([[model_name] + list(metrics.values())], headers=['Model'] + list(metrics.keys()))
