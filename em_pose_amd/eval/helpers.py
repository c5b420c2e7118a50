"""
Evaluation driver (mirror of reference empose/eval/helpers.py:30-200 and scripts/evaluate_real.py:24-101).

  window_generator        256-frame chunks of one recording (reference helpers.py:30-48)
  load_model              config.json + model.pth of a released model id (reference helpers.py:131-164)
  partition_sequences     NEW: whole recordings -> ranks, longest-processing-time-first (chunks of one
                          recording are serially dependent through the LSTM state and must stay on one GPU)
  evaluate_sequences      the per-recording loop of evaluate_real.py (state carry, first chunk's shape for the whole
                          recording, metrics on all frames / per recording)
  evaluate_sequences_batched, plan_rows   NEW: chunk c of all recordings as one ragged batch, and its plan of rows
"""
import collections
import contextlib
import glob
import os
import time
from collections import defaultdict

import numpy as np
import torch
from torch.nn.utils.rnn import pad_sequence

from em_pose_amd import _lib
from em_pose_amd.data.data import RealBatch
from em_pose_amd.eval.metrics import MetricsEngine
from em_pose_amd.helpers.configuration import CONSTANTS as C
from em_pose_amd.helpers.configuration import Configuration
from em_pose_amd.nn.models import IterativeErrorFeedback, create_model


def window_generator(batch, window_size):
    if window_size is None:
        yield batch
        return
    assert isinstance(batch, RealBatch)
    seq_len = batch.seq_length
    n_windows = seq_len // window_size + int(seq_len % window_size > 0)
    for i in range(n_windows):
        sf, ef = i * window_size, min((i + 1) * window_size, seq_len)
        lengths = torch.tensor([ef - sf], dtype=batch.seq_lengths.dtype, device=batch.seq_lengths.device)
        yield RealBatch(batch.ids, lengths, batch.poses[:, sf:ef], batch.shapes, batch.trans[:, sf:ef],
                        batch.marker_pos_real[:, sf:ef], batch.marker_ori_real[:, sf:ef], batch.marker_masks[:, sf:ef],
                        batch.offset_t, batch.offset_r)


def get_model_dir(experiment_dir, model_id):
    hits = glob.glob(os.path.join(experiment_dir, str(model_id) + '-*'))
    if len(hits) != 1:
        raise ValueError('expected exactly one model directory for id {} under {}, found {}'
                         .format(model_id, experiment_dir, len(hits)))
    return hits[0]


def load_model_weights(checkpoint_file, net, state_key='model_state_dict'):
    if not os.path.exists(checkpoint_file):
        raise ValueError('Could not find model checkpoint {}.'.format(checkpoint_file))
    ckpt = torch.load(checkpoint_file, map_location='cpu')[state_key]
    missing, unexpected = net.load_state_dict(ckpt, strict=False)
    bad = [k for k in list(missing) + list(unexpected) if not k.startswith('smpl.')]
    if bad:
        raise ValueError('checkpoint does not match the model: {}'.format(bad[:8]))


def get_all_offset_files():
    """{subject id: path} of the `*_offsets.npz` files of the real data set (reference helpers/utils.py:149-153)."""
    files = sorted(glob.glob(os.path.join(C.DATA_DIR_TEST, '*_offsets.npz')))
    return {os.path.split(f)[-1].split('_')[0]: f for f in files}


def sensor_vertex_ids():
    """The sensor sites of the asset tree: the `vertex_ids` of its offsets files (reference transforms.py:159, "the same
    for all offsets"), `C.VERTEX_IDS` when the tree has none.  On the licensed assets the two agree (the reference's
    network uses the constant, models.py:383, its preprocessing the files'); a tree around another mesh -- the 160-vertex
    one of tests/golden/eval_assets -- states its sites there."""
    ids = None
    for path in get_all_offset_files().values():
        here = [int(v) for v in np.load(path)['vertex_ids'].tolist()]
        if ids is not None and here != ids:
            raise ValueError('the offsets files under {} disagree about vertex_ids'.format(C.DATA_DIR_TEST))
        ids = here
    return list(C.VERTEX_IDS) if ids is None else ids


def load_model(model_id, device=None):
    """reference eval/helpers.py:148-164: config.json -> body model -> network -> model.pth (whose `smpl.bm.*` buffers
    replace what `model.npz` held, as `load_state_dict` does in the reference)."""
    from em_pose_amd.bodymodels.smpl import create_default_smpl_model
    device = C.DEVICE if device is None else device
    model_dir = get_model_dir(C.EXPERIMENT_DIR, model_id)
    config = Configuration.from_json(os.path.join(model_dir, 'config.json'))
    smpl = create_default_smpl_model(device)
    net = create_model(config, smpl)
    if hasattr(net, 'vertex_ids'):
        net.vertex_ids = sensor_vertex_ids()
    load_model_weights(os.path.join(model_dir, 'model.pth'), net)
    return net.to(device).eval(), config, model_dir


def get_model_config(model_id):
    """(Configuration, model directory) of a released model (reference eval/helpers.py:140-145)."""
    model_dir = get_model_dir(C.EXPERIMENT_DIR, model_id)
    return Configuration.from_json(os.path.join(model_dir, 'config.json')), model_dir


def evaluate(data_loader, net, preprocess_fn, metrics_engine, window_size=None, device=None, vertex_engine=None,
             temporal_engine=None, skin_engine=None):
    """
    Losses and metrics over a hold-out set (reference eval/helpers.py:51-111): every batch is normalised as a whole,
    cut into temporal chunks (`window_size`, single-recording `RealBatch`es only, as in the reference), preprocessed,
    run through the model with the LSTM state carried over the chunks, and fed to the metrics engine with the shape of
    the first chunk.  `vertex_engine` (optional, eval/mesh_metrics.py `VertexErrorEngine`) is reset and fed beside the
    metrics engine, with the same tensors and the first chunk's shape: the per-vertex error of the same frames.
    `temporal_engine` (optional, eval/temporal_metrics.py `TemporalMetricsEngine`) likewise, with `is_new_sequence` as the
    model gets it: the acceleration error and the jitter over the same frames, the stencils carried across the chunks.
    `skin_engine` (optional, eval/surface_metrics.py `SkinDistanceEngine`) likewise, with the chunk's readings
    (`batch_readings`): how far the readings are from the skin of the estimate and of the ground truth.
    :return: dict of loss values averaged over the samples of the set.
    """
    device = C.DEVICE if device is None else device
    net.eval()
    keep = getattr(net, 'keep_history', True)
    net.keep_history = True            # the loss values are computed from the iteration histories
    agg, n_samples = defaultdict(float), 0
    metrics_engine.reset()
    if vertex_engine is not None:
        vertex_engine.reset()
    if temporal_engine is not None:
        temporal_engine.reset()
    if skin_engine is not None:
        from em_pose_amd.eval.surface_metrics import batch_readings
        skin_engine.reset()
    try:
        with torch.no_grad():
            for b, abatch in enumerate(data_loader):
                abatch = preprocess_fn(abatch, mode='normalize_only')
                first_shape_hat, seq_vals, n_chunks, bs = None, defaultdict(float), 0, 0
                for i, achunk in enumerate(window_generator(abatch, window_size)):
                    chunk = preprocess_fn(achunk.to_gpu(device), mode='after_normalize', reset_rng=(i + b == 0))
                    out = net(chunk, is_new_sequence=(i == 0))
                    _, vals = net.backward(chunk, out)
                    for k, v in vals.items():
                        seq_vals[k] += v
                    pose_hat = out['pose_hat'] if out['pose_hat'] is not None else chunk.poses_body
                    if i == 0:
                        first_shape_hat = out['shape_hat'][:, 0] if out['shape_hat'] is not None else None
                    metrics_engine.compute(chunk.poses_body, chunk.shapes, pose_hat, first_shape_hat, chunk.seq_lengths,
                                           chunk.poses_root, out['root_ori_hat'], frame_mask=chunk.marker_masks)
                    if vertex_engine is not None:
                        vertex_engine.compute(chunk.poses_body, chunk.shapes, pose_hat, first_shape_hat,
                                              chunk.seq_lengths, chunk.poses_root, out['root_ori_hat'],
                                              frame_mask=chunk.marker_masks)
                    if temporal_engine is not None:
                        temporal_engine.compute(chunk.poses_body, chunk.shapes, pose_hat, first_shape_hat,
                                                chunk.seq_lengths, chunk.poses_root, out['root_ori_hat'],
                                                frame_mask=chunk.marker_masks, is_new_sequence=(i == 0))
                    if skin_engine is not None:
                        readings, reading_masks = batch_readings(chunk)
                        skin_engine.compute(chunk.poses_body, chunk.shapes, pose_hat, first_shape_hat,
                                            chunk.seq_lengths, chunk.poses_root, out['root_ori_hat'],
                                            frame_mask=chunk.marker_masks, marker_pos=readings,
                                            marker_masks=reading_masks)
                    n_chunks, bs = i + 1, chunk.batch_size
                for k, v in seq_vals.items():
                    agg[k] += v / n_chunks * bs
                n_samples += bs
    finally:
        net.keep_history = keep
    return {k: v / n_samples for k, v in agg.items()}


def compute_loss_and_metrics(data_loader, net, preprocess_fn, model_id, smpl_model=None, device=None,
                             vertex_error=False, vertex_error_procrustes=False, temporal=False,
                             temporal_surface=False, skin_distance=False):
    """reference eval/helpers.py:114-128.  `vertex_error` (not in the reference): also accumulate the per-vertex error
    (eval/mesh_metrics.py) and print it as a second table line, with `vertex_error_procrustes` the Procrustes-aligned
    error in the same line.  `temporal` (not in the reference): also accumulate the acceleration error and the jitter
    (eval/temporal_metrics.py) and print them as a further table line, with `temporal_surface` the surface columns in the
    same line.  `skin_distance` (not in the reference): also accumulate the distance of the readings to the skin of the
    estimate and of the ground truth (eval/surface_metrics.py) and print it as a further table line.  The returned values
    are the same either way."""
    if smpl_model is None:
        from em_pose_amd.bodymodels.smpl import create_default_smpl_model
        smpl_model = create_default_smpl_model(device)
    me = MetricsEngine(smpl_model)
    ve = None
    if vertex_error:
        from em_pose_amd.eval.mesh_metrics import VertexErrorEngine
        ve = VertexErrorEngine(smpl_model, procrustes=vertex_error_procrustes)
    te = None
    if temporal or temporal_surface:
        from em_pose_amd.eval.temporal_metrics import TemporalMetricsEngine
        te = TemporalMetricsEngine(smpl_model, surface=temporal_surface)
    se = None
    if skin_distance:
        from em_pose_amd.eval.surface_metrics import SkinDistanceEngine
        se = SkinDistanceEngine(smpl_model)
    losses = evaluate(data_loader, net, preprocess_fn, me, device=device, vertex_engine=ve, temporal_engine=te,
                      skin_engine=se)
    print('[LOSS] loss: {:.6f}'.format(losses['total_loss']))
    metrics = me.get_metrics()
    print(me.to_pretty_string(metrics, model_id))
    if ve is not None:
        print(ve.to_pretty_string(ve.get_metrics(), model_id))
    if te is not None:
        print(te.to_pretty_string(te.get_metrics(), model_id))
    if se is not None:
        print(se.to_pretty_string(se.get_metrics(), model_id))
    return losses, metrics


def partition_sequences(lengths, world_size):
    """
    Longest-processing-time-first assignment of recordings to ranks.
    :return: list (per rank) of sorted recording indices; deterministic for equal lengths.
    """
    order = sorted(range(len(lengths)), key=lambda i: (-int(lengths[i]), i))
    load = [0] * world_size
    parts = [[] for _ in range(world_size)]
    for i in order:
        r = min(range(world_size), key=lambda k: (load[k], k))
        parts[r].append(i)
        load[r] += int(lengths[i])
    return [sorted(p) for p in parts]


DEFER_FRAME_BUDGET = 65536   # evaluate_sequences: frames whose metrics may wait for one joint launch


def _check_async(dev):
    """After a synchronisation: a cooperative LSTM kernel that gave up on a poll poisoned its outputs with NaN and counted
    itself (include/empose_hip.h, empose_async_status) -- raise instead of averaging NaNs into the metrics table."""
    if torch.device(dev).type == 'cuda':
        _lib.check(_lib.lib().empose_async_status())


def _laps(host_times):
    """lap(key): (dev) the host seconds since the last lap, added to host_times[key] (None: nothing is measured)."""
    t = [time.perf_counter()]

    def lap(key):
        if host_times is not None:
            now = time.perf_counter()
            host_times[key], t[0] = host_times.get(key, 0.0) + now - t[0], now
    return lap


class _ChunkPipeline(object):
    """Chunks of a recording depend on each other only through the LSTM state, so chunk c + 1's packing + LSTM (current
    stream) runs beside chunk c's refinement iterations and metrics (a side stream, IterativeErrorFeedback.iter_stream);
    nothing in a driver's loop waits for the device.  Same results as one chunk after the other.  On the CPU, and for a
    model without the two-part forward, there is no side stream: everything runs where the caller is."""

    def __init__(self, net, device):
        self.net, self.dev, self.side = net, torch.device(device), None
        if isinstance(net, IterativeErrorFeedback) and self.dev.type == 'cuda' and not net.training:
            # one side stream per network, kept: a fresh stream per call may land on the hardware queue of the current
            # stream (measured: the first pass pipelined, later passes with their new streams did not)
            self.side = getattr(net, '_side_stream', None)
            if self.side is None or self.side.device != self.dev:
                self.side = net._side_stream = torch.cuda.Stream(device=self.dev)

    def __enter__(self):
        if self.side is not None:
            self.net.iter_stream = self.side
        return self

    def __exit__(self, *exc):
        if self.side is not None:
            self.net.iter_stream = None

    def forward(self, chunk, is_new_sequence):
        out = self.net(chunk, is_new_sequence=is_new_sequence)
        if self.side is not None and self.net.outputs_ready is None:
            # the forward did not go through the two-stream path (autograd forward of a `differentiable` net with grad
            # enabled): its outputs are on the current stream, the metrics are on the side stream
            self.side.wait_stream(torch.cuda.current_stream(self.dev))
        return out

    def metrics(self, chunk, *more):
        """Context of a chunk's metrics; the chunk (and `more`) live in memory of the current stream's pool."""
        if self.side is None:
            return contextlib.nullcontext()
        for t in (chunk.poses, chunk.shapes, chunk.seq_lengths) + more:
            t.record_stream(self.side)
        return torch.cuda.stream(self.side)

    def drain(self):
        if self.side is not None:
            torch.cuda.current_stream(self.dev).wait_stream(self.side)   # every chunk's outputs / rows are complete


def _recording_metrics(smpl_model, state, base, i):
    me = MetricsEngine(smpl_model)
    me.merge({key: v[base[i]:base[i + 1]] for key, v in state.items()})
    return me.get_metrics()


def _tables(smpl_model, ids, state, base, ready=None):
    """`state` of an engine with the rows in recording order, recording i owning rows base[i] .. base[i + 1] -> (overall
    engine, [(recording id, metrics dict)]); `ready[i]`: a recording's metrics where they are worked out already."""
    ready = [None] * len(ids) if ready is None else ready
    per_sequence = [(sid, ready[i] or _recording_metrics(smpl_model, state, base, i)) for i, sid in enumerate(ids)]
    me_all = MetricsEngine(smpl_model)
    me_all.merge(state)
    return me_all, per_sequence


def _flush_deferred(engine, deferred):
    # On the device path the metrics of the sequential driver are computed ONCE, over the frames of all chunks: a chunk
    # only leaves its tensors in `deferred` (the per-chunk forward-kinematics + metrics launches and the tensor plumbing
    # around them were 0.27 ms of host time per chunk, a quarter of a pass that is bound by the host).  Here:
    # one forward-kinematics launch and one metrics launch over the frames of the deferred chunks, in chunk order; shapes
    # per frame (ground truth: the recording's; estimate: the recording's first chunk's, evaluate_real.py:63-68).  Called
    # at the end of the pass and whenever DEFER_FRAME_BUDGET frames have piled up (each deferred chunk pins its staging
    # buffer and outputs, ~1.8 KB per frame; the rows of a flush stay on the device until the pass ends, 65 doubles per frame)
    if not deferred:
        return
    frames_of = lambda t: t.reshape(-1, t.shape[-1])
    cat = lambda k: torch.cat([frames_of(d[k]) for d in deferred]).unsqueeze(0)
    per_frame = lambda k, alt: torch.cat([(d[k] if d[k] is not None else d[alt]).reshape(1, -1)
                                          .expand(d[0].shape[1], -1) for d in deferred]).unsqueeze(0)
    engine.compute(cat(0), per_frame(1, 1), cat(2), per_frame(3, 1), None, cat(4), cat(5),
                   valid=torch.cat([d[6].reshape(-1) for d in deferred]).unsqueeze(0))
    del deferred[:]


def evaluate_sequences(net, batches, smpl_model, device, window_size=256, log=None, host_times=None):
    """
    :param batches: iterable of single-recording `RealBatch`es (root already normalised), on the CPU.
    :return: (overall MetricsEngine, [(recording id, metrics dict)], frames processed)
    """
    lap = _laps(host_times)
    ws = window_size if isinstance(net, IterativeErrorFeedback) else None
    # ONE engine collects the rows of every chunk of every recording (on the device, in call order); they are read back
    # once, after the last recording, and split by the per-recording counts of valid frames.  Reading them back per
    # recording (as the reference's two engines would) drains the two-stream pipeline 36 times: 3.3 ms each, 0.12 of the
    # 0.25 s of a pass.
    me_rows = MetricsEngine(smpl_model)
    ids, counts, frames = [], [], 0
    deferred, deferred_frames = [], 0    # (`_flush_deferred`)
    with _ChunkPipeline(net, device) as pipe:
        defer = pipe.side is not None and getattr(me_rows, 'angle_glob', False) and hasattr(smpl_model, 'fk_joints')
        for batch in batches:
            if log:
                log('Evaluate {} ({} frames)'.format(batch.ids[0], int(batch.seq_lengths[0])))
            ids.append(batch.ids[0])
            counts.append(0)
            # (Staging the whole recording on the device once and slicing views was measured slower: recordings have 36
            # different lengths, and every new size costs the caching allocator a ~50 ms hipMalloc/hipFree round.)
            for c, chunk in enumerate(window_generator(batch, ws)):
                frames += int(chunk.seq_lengths.sum())   # read while the lengths are still on the host
                # the frames that count, while lengths and masks are still on the host (no device kernels for it)
                valid = MetricsEngine.valid_frames(chunk.seq_lengths, chunk.batch_size, chunk.seq_length,
                                                   chunk.marker_masks)
                counts[-1] += int(valid.sum())
                lap('cut_chunk')
                chunk = chunk.to_gpu(device)
                lap('to_gpu')
                out = pipe.forward(chunk, is_new_sequence=(c == 0))
                lap('forward_enqueue')
                if c == 0:  # the first chunk's shape is used for the whole recording (evaluate_real.py:63-68)
                    first_shape_hat = out['shape_hat'][:, 0] if out['shape_hat'] is not None else None
                if defer and out['pose_hat'].is_cuda:
                    deferred.append((chunk.poses_body, chunk.shapes, out['pose_hat'], first_shape_hat, chunk.poses_root,
                                     out['root_ori_hat'], valid))
                    deferred_frames += chunk.seq_length
                    if deferred_frames >= DEFER_FRAME_BUDGET:   # bound what is kept alive: row order is unchanged
                        pipe.drain()
                        _flush_deferred(me_rows, deferred)
                        deferred_frames = 0
                else:
                    with pipe.metrics(chunk):
                        # the reference feeds the same chunk to two engines (evaluate_real.py:70-81); compute once per chunk
                        me_rows.compute(chunk.poses_body, chunk.shapes, out['pose_hat'], first_shape_hat,
                                        chunk.seq_lengths, chunk.poses_root, out['root_ori_hat'],
                                        frame_mask=chunk.marker_masks, valid=valid)
                lap('metrics_enqueue')
        pipe.drain()
        _flush_deferred(me_rows, deferred)
        st = me_rows.state()        # (reads the rows back: the device is in sync afterwards)
        _check_async(device)
        lap('wait_for_device_and_rows')
        me_all, per_sequence = _tables(smpl_model, ids, st, np.concatenate([[0], np.cumsum(counts, dtype=np.int64)]))
        lap('per_recording_metrics')
    return me_all, per_sequence, frames


RowPlan = collections.namedtuple('RowPlan', 'order lengths valid base total chunks lens dest')
RowPlanChunk = collections.namedtuple('RowPlanChunk', 'sf f k lens ended')


def plan_rows(lengths, valid_per_recording, window_size):
    """How the batched driver cuts its chunks and where every frame's metric row goes, from the recordings' lengths and
    their frames that count (per recording, bool (frames,)).  Batch row j is recording order[j]: `lengths`, `valid`, `dest`
    (rows, longest) and `lens` (chunks, rows) are per batch row, `base` is per recording, `ended` lists recordings."""
    n = len(lengths)
    # Longest recording first: the rows that still have frames in chunk c are then a PREFIX of the batch, so a chunk is
    # a slice [:k, sf:sf + f] of one padded block per field (no per-row cutting, padding and concatenating: that was
    # 47 of the 82 ms of a pass, all of it host time -- the device waits for the host in this driver).
    order = sorted(range(n), key=lambda i: (-lengths[i], i))
    sl = np.asarray([lengths[i] for i in order], dtype=np.int64)
    n_chunks = (int(sl[0]) + window_size - 1) // window_size
    valid = np.zeros((n, int(sl[0])), dtype=bool)
    for j, i in enumerate(order):
        valid[j, :sl[j]] = valid_per_recording[i]
    # Where every frame's row goes: recording i owns rows base[i] .. base[i + 1] of one block, its valid frames in
    # frame order (what the sequential driver accumulates, recording after recording); frames that do not count go to
    # a spare row past the end.
    base = np.zeros(n + 1, dtype=np.int64)
    base[1:][order] = valid.sum(axis=1)
    base = np.cumsum(base)
    total = int(base[-1])
    dest = np.where(valid, np.cumsum(valid, axis=1) - 1 + base[:-1][order][:, None], total)
    lens = np.clip(sl[None, :] - window_size * np.arange(n_chunks)[:, None], 0, window_size).astype(np.int32)
    rows = (lens > 0).sum(axis=1).tolist() + [0]     # per chunk, and none after the last
    chunks = [RowPlanChunk(c * window_size, int(lens[c, 0]), k, lens[c, :k], [order[j] for j in range(rows[c + 1], k)])
              for c, k in enumerate(rows[:-1])]
    return RowPlan(order, sl, valid, base, total, chunks, lens, dest)


class _PlacedRows(object):
    """The metric rows of a chunk are scattered on the device to where they belong in ONE block in recording order; a
    recording's rows go to the host (pinned memory, side stream) with the chunk it ends in, and its table row is worked
    out while the device runs the chunks after it -- the host part of the metrics (a third of a pass when it ran after the
    last chunk) is hidden behind the device, which is the bound of the batched driver (the LSTM's dependent steps)."""

    def __init__(self, plan, smpl_model, device):
        self.plan, self.smpl_model = plan, smpl_model
        self.dest = torch.from_numpy(np.ascontiguousarray(plan.dest)).pin_memory().to(device, non_blocking=True)
        self.rows = torch.empty(plan.total + 1, 65, dtype=torch.float64, device=device)
        self.rows_host = torch.empty(max(plan.total, 1), 65, dtype=torch.float64, pin_memory=True)
        r = self.rows_host.numpy()[:plan.total]   # (the view keeps the pinned block alive; torch caches it afterwards)
        self.state = {'eucl': r[:, :22], 'eucl_pa': r[:, 22:44], 'angle': r[:, 44:]}
        self.arrived = []                         # (event, recordings whose rows it brings), in chunk order
        self.ready = [None] * len(plan.order)     # per recording: its metrics

    def place(self, rows, ch):
        base = self.plan.base
        self.rows.index_copy_(0, self.dest[:ch.k, ch.sf:ch.sf + ch.f].reshape(-1), rows)
        for i in ch.ended:
            if base[i + 1] > base[i]:
                self.rows_host[base[i]:base[i + 1]].copy_(self.rows[base[i]:base[i + 1]], non_blocking=True)
        self.arrived.append((torch.cuda.current_stream().record_event(), ch.ended))

    def take_arrived(self, wait):
        while self.arrived and (wait or self.arrived[0][0].query()):
            ev, recs = self.arrived.pop(0)
            ev.synchronize()
            for i in recs:
                self.ready[i] = _recording_metrics(self.smpl_model, self.state, self.plan.base, i)


def _rows_in_recording_order(state, plan):
    """Host rows as the chunks left them (chunk after chunk, batch row after batch row) -> recording order."""
    of = lambda a, ch: a[:ch.k, ch.sf:ch.sf + ch.f]
    back = np.argsort(np.concatenate([of(plan.dest, ch)[of(plan.valid, ch)] for ch in plan.chunks]))
    return {key: v[back] if v.shape[0] else v for key, v in state.items()}     # (a family without rows stays without)


def _prepare_batched(batches, smpl_model, dev, window_size, lap):
    """-> the row plan, one padded block per field on the device (rows as in the plan), the engine, the placed rows."""
    lengths = [int(b.seq_lengths[0]) for b in batches]
    order = sorted(range(len(batches)), key=lambda i: (-lengths[i], i))   # (`plan_rows`, which comes after the upload)
    # (a recording a loader has pinned -- RealBatch.pin_memory -- goes up as ONE block, without staging and without
    # blocking the host: 36 copies per pass instead of 288)
    on_dev = [batches[i].device_fields(dev) for i in order]
    fields = ('poses', 'trans', 'marker_pos_real', 'marker_ori_real', 'marker_masks')
    packed = {k: pad_sequence([d[k][0] for d in on_dev], batch_first=True) for k in fields}
    packed.update({k: torch.cat([d[k] for d in on_dev]) for k in ('shapes', 'offset_t', 'offset_r')})
    del on_dev
    lap('upload_and_pack')
    # the frames that count -- inside the recording and every sensor present -- from the host copies of the masks
    # (numpy: a torch CPU op on a 36 x 256 x 12 block wakes the whole intra-op thread pool)
    valid = [(b.marker_masks[0].numpy() != 0).all(axis=-1) for b in batches]
    lap('valid_frames')
    plan = plan_rows(lengths, valid, window_size)
    packed['ids'] = [batches[i].ids[0] for i in plan.order]
    me_chunks = MetricsEngine(smpl_model)
    # placed: `compute` queues device rows (its device path); otherwise it accumulates on the host and the rows are
    # put into recording order after the loop
    placed = _PlacedRows(plan, smpl_model, dev) if me_chunks.queues_device_rows(dev) else None
    # the lengths of every chunk's rows in ONE pinned block and one copy that does not block (a pageable copy would make
    # the host wait for the stream; a pinned block per chunk asks the host allocator 14 times a pass, and a request it
    # cannot serve from its cache waits for the device)
    packed['lens'] = torch.from_numpy(plan.lens)
    if dev.type == 'cuda':
        packed['lens'] = packed['lens'].pin_memory().to(dev, non_blocking=True)
    lap('row_plan')
    return plan, packed, me_chunks, placed


def _run_batched_chunks(net, pipe, plan, packed, me_chunks, placed, lap):
    state, first_shape = None, None
    on_side = (placed.dest, placed.rows) if placed is not None else ()   # what the metrics stream uses beside the chunk
    for c, ch in enumerate(plan.chunks):
        cut = lambda name: packed[name][:ch.k, ch.sf:ch.sf + ch.f]
        chunk = RealBatch(packed['ids'][:ch.k], packed['lens'][c, :ch.k], cut('poses'), packed['shapes'][:ch.k],
                          cut('trans'), cut('marker_pos_real'), cut('marker_ori_real'), cut('marker_masks'),
                          packed['offset_t'][:ch.k], packed['offset_r'][:ch.k]).to_gpu(pipe.dev)
        if net.rnn_init and c > 0:   # the rows that go on are the first k of the previous chunk's
            net.rnn.final_state = (state[0][:, :ch.k].contiguous(), state[1][:, :ch.k].contiguous())
        lap('chunk_prep')
        out = pipe.forward(chunk, is_new_sequence=(c == 0))
        lap('forward_enqueue')
        if net.rnn_init:
            state = net.rnn.final_state
        with pipe.metrics(chunk, *on_side):
            if c == 0:   # the first chunk's shape estimate stands for the whole recording (evaluate_real.py:63-68)
                first_shape = out['shape_hat'][:, 0].contiguous()
            valid = torch.from_numpy(np.ascontiguousarray(plan.valid[:ch.k, ch.sf:ch.sf + ch.f]))
            queued = me_chunks.compute(chunk.poses_body, chunk.shapes, out['pose_hat'], first_shape[:ch.k],
                                       chunk.seq_lengths, chunk.poses_root, out['root_ori_hat'],
                                       frame_mask=chunk.marker_masks, valid=valid)
            if queued != (placed is not None):
                raise RuntimeError('MetricsEngine.compute %s device rows, the driver expected the opposite'
                                   % ('queued' if queued else 'did not queue'))
            if placed is not None:
                (rows, _, _), = me_chunks.take_device_rows()
                placed.place(rows, ch)
        lap('metrics_enqueue')
        if placed is not None:
            placed.take_arrived(wait=False)
        lap('per_recording_metrics')


def evaluate_sequences_batched(net, batches, smpl_model, device, window_size=256, host_times=None):
    """
    Same results as `evaluate_sequences`, but chunk c of ALL recordings runs as one ragged batch (rows = recordings
    that still have frames, `seq_lengths` = frames left in this chunk, LSTM state carried per row).  Windows are
    independent of each other in the model, so this only changes how much work one launch carries:
    36 recordings need 14 launches of the loop instead of 211.

    `host_times` (a dict, optional): seconds of host time per section of the pass (dev: where a slow pass spends it).
    """
    lap = _laps(host_times)
    assert isinstance(net, IterativeErrorFeedback)
    if len(batches) == 0:      # (a rank of a multi-GPU run that got no recording)
        return MetricsEngine(smpl_model), [], 0
    dev = torch.device(device)
    plan, packed, me_chunks, placed = _prepare_batched(batches, smpl_model, dev, window_size, lap)
    # rows shorter than the chunk are padded: average the shape over their valid frames only, which is what the
    # unpadded one-recording chunk of the sequential driver averages over
    was_valid_only, net.shape_avg_valid_only = net.shape_avg_valid_only, True
    try:
        with _ChunkPipeline(net, dev) as pipe:
            _run_batched_chunks(net, pipe, plan, packed, me_chunks, placed, lap)
            if placed is not None:
                placed.take_arrived(wait=True)     # (the last event is the end of the side stream's work)
                lap('wait_for_device')
            pipe.drain()
            if dev.type == 'cuda':
                torch.cuda.synchronize(dev)
                _check_async(dev)
            lap('wait_for_device')
            if placed is not None:
                rows, ready = placed.state, placed.ready
            else:   # one device-side gather of the valid rows, one copy to (cached) pinned host memory
                rows, ready = _rows_in_recording_order(me_chunks.state(), plan), None
                lap('merge_rows')
    finally:
        net.shape_avg_valid_only = was_valid_only
    # (a recording without a single frame never ended in a chunk: its empty table row is made here)
    me_all, per_sequence = _tables(smpl_model, [b.ids[0] for b in batches], rows, plan.base, ready)
    lap('per_recording_metrics')
    return me_all, per_sequence, int(plan.lengths.sum())
