"""
Temporal metrics on the device (empose_temporal_rows, csrc/temporal.hip; eval/temporal_metrics.py TemporalMetricsEngine).

The kernel against the float64 restatement (tests/temporal_ref.py) on the same float32 inputs, at every element of `rows`
and `defined`.  Both sides are float64 arithmetic on identical inputs, so the bound is derived, not measured: per entry
  |ours - ref| <= 64 x 2^-52 x 8 x max|x| x fps^k     (k = 2 for the acceleration block, 3 for the two jitter blocks),
fewer than 16 roundings at the magnitude of the largest intermediate; the reduced mode multiplies it by P for the sums and
by 2 P max_entry for the sums of squares.  `defined` matches exactly and what is written as 0 is exactly 0.

The engine end to end against float64 through the oracle (oracle/torch_ref.py smpl_fk, then the restatement).  The
tolerance is measured in the same test from existing code: eps = the largest distance between a joint of `fk_joints` (a
vertex of the layer's forward) and its float64 position over the inputs.  By the triangle inequality an acceleration entry
may differ by 2 x 4 x fps^2 x eps (two bodies) and a jitter entry by 8 x fps^3 x eps, plus the float64 term above.
8 x fps^3 x eps is the metric's fp32 noise floor.  Every check prints its figures before it asserts.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from em_pose_amd import _lib, synthetic
from em_pose_amd.bodymodels.smpl import SMPLLayer
from em_pose_amd.eval.metrics import MetricsEngine
from em_pose_amd.eval.temporal_metrics import TemporalMetricsEngine, temporal_rows
from oracle import torch_ref as R
from tests import helpers as H
from tests import temporal_ref as T

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FPS = 60.0
S = _lib.TEMPORAL_SEGMENT
U = 64 * 2.0 ** -52 * 8          # the derived float64 bound, per unit of max|x| fps^k
FRAMES = (1, 2, 3, 4, 5, 33, S - 1, S, S + 1, S + 3, S + 4)
_CASES = {}


def _case(n, f, P):
    """Smooth float32 inputs, ragged validity (3 % invalid, the last row all invalid when there is more than one) and
    the restatement, computed once per shape and left unchanged."""
    key = (n, f, P)
    if key not in _CASES:
        rng = np.random.default_rng(1000 * n + 10 * f + P)
        g, h = T.smooth_points(rng, n, f, P)
        v = T.ragged_valid(rng, n, f, dead_row=n - 1 if n > 1 else None)
        rows, defined = T.rows64(g, h, v, FPS)
        _CASES[key] = (g, h, v, rows, defined)
    return _CASES[key]


def _launch(g, h, v, reduce, fps=FPS):
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    rows, defined = temporal_rows(dev(g), dev(h), dev(v), fps, reduce=reduce)
    assert rows.dtype == torch.float64 and defined.dtype == torch.uint8
    return rows.cpu().numpy(), defined.cpu().numpy()


def _bounds(g, h, P):
    x = max(float(np.abs(g).max()), float(np.abs(h).max()))
    b = np.empty(3 * P)
    b[:P] = U * x * FPS ** 2
    b[P:] = U * x * FPS ** 3
    return b


# ---- the kernel against the restatement, at every element ---------------------------------------------------------------------
@pytest.mark.parametrize('P', [1, 22, 63, 64, 65, 160])
def test_per_point_rows_against_the_restatement(P):
    worst = 0.0
    for n in (1, 3):
        for f in FRAMES:
            g, h, v, want, want_def = _case(n, f, P)
            got, got_def = _launch(g, h, v, reduce=False)
            assert got.shape == (n, f, 3 * P) and np.array_equal(got_def, want_def), (n, f)
            ratio = np.abs(got - want) / _bounds(g, h, P)
            worst = max(worst, float(ratio.max()))
            assert (got[want == 0] == 0).all(), (n, f)           # what is written as 0 is exactly 0
            assert ratio.max() <= 1.0, (n, f, float(ratio.max()))
    print('per-point P={}: worst |ours - ref| / bound = {:.3e}'.format(P, worst))


def _check_reduced(g, h, v, want, want_def, P):
    got, got_def = _launch(g, h, v, reduce=True)
    n, f = v.shape
    assert got.shape == (n, f, 6) and np.array_equal(got_def, want_def)
    ref = T.reduced64(want)
    b = _bounds(g, h, P)
    top = want.reshape(n, f, 3, P).max(axis=(0, 1, 3))         # the largest entry of each quantity
    bound = np.empty(6)
    for q in range(3):
        bound[2 * q] = P * b[q * P]
        bound[2 * q + 1] = 2 * P * top[q] * b[q * P]
    undefined = np.repeat(np.stack([(want_def & T.ACC) == 0, (want_def & T.JERK) == 0, (want_def & T.JERK) == 0], -1), 2, -1)
    assert (got[undefined] == 0).all()
    ratio = np.abs(got - ref) / np.where(bound > 0, bound, 1.0)
    assert (np.abs(got - ref)[..., bound == 0] == 0).all()
    return float(ratio.max()), got


@pytest.mark.parametrize('P', [1, 22, 63, 64, 65, 160])
def test_reduced_rows_against_the_restatement(P):
    worst = 0.0
    for n in (1, 3):
        for f in FRAMES:
            g, h, v, want, want_def = _case(n, f, P)
            ratio, _ = _check_reduced(g, h, v, want, want_def, P)
            worst = max(worst, ratio)
            assert ratio <= 1.0, (n, f, ratio)
    print('reduced P={}: worst |ours - ref| / bound = {:.3e}'.format(P, worst))


def test_reduced_rows_over_the_full_mesh():
    """P = 6890: 27 tiles of 256 points, the last with 234; every wave adds several tiles."""
    g, h, v, want, want_def = _case(1, 8, 6890)
    ratio, _ = _check_reduced(g, h, v, want, want_def, 6890)
    print('reduced P=6890: worst |ours - ref| / bound = {:.3e}'.format(ratio))
    assert ratio <= 1.0


@pytest.mark.parametrize('P', [22, 300])
def test_reduced_row_is_the_sum_of_the_per_point_row_and_launches_repeat(P):
    g, h, v, want, want_def = _case(3, S + 4, P)
    points, d0 = _launch(g, h, v, reduce=False)
    again, d1 = _launch(g, h, v, reduce=False)
    assert np.array_equal(points, again) and np.array_equal(d0, d1)           # two launches, identical bits
    ratio, sums = _check_reduced(g, h, v, points, d0, P)                        # ... against the kernel's own points
    _, sums_again = _check_reduced(g, h, v, points, d0, P)
    assert np.array_equal(sums, sums_again)
    print('reduced against per-point P={}: worst ratio {:.3e}'.format(P, ratio))
    assert ratio <= 1.0


def test_known_answers_on_the_device():
    t = np.arange(8, dtype=np.float64)
    zero = np.zeros((1, 8, 2, 3), np.float32)
    x = zero.copy()
    x[0, :, 0, 0] = t ** 3
    x[0, :, 1, 2] = t ** 2
    ones = np.ones((1, 8), bool)
    rows, defined = _launch(x, zero, ones, reduce=False)
    assert defined[0].tolist() == [0, 0, 1, 3, 3, 3, 3, 3]
    assert np.array_equal(rows[0, 3:, 4], np.full(5, 6.0 * FPS ** 3))          # |jerk_gt| of t^3: 6 fps^3 exactly
    assert np.array_equal(rows[0, 2:, 0], (6.0 * t[2:] - 6.0) * FPS ** 2)
    assert np.array_equal(rows[0, 2:, 1], np.full(6, 2.0 * FPS ** 2))          # acc of t^2: 2 fps^2 exactly
    assert not rows[0, :, 5].any() and not rows[0, :, 2:4].any()               # jerk of t^2 is 0; the estimate is still
    rows, _ = _launch(zero, x, ones, reduce=False)
    assert np.array_equal(rows[0, 3:, 2], np.full(5, 6.0 * FPS ** 3)) and not rows[0, :, 4:].any()
    sums, _ = _launch(x, zero, ones, reduce=True)
    assert np.array_equal(sums[0, 3:, 4], np.full(5, 6.0 * FPS ** 3))
    assert np.array_equal(sums[0, 3:, 5], np.full(5, (6.0 * FPS ** 3) ** 2))
    # F < 3 is legal and defines nothing
    for f in (1, 2):
        rows, defined = _launch(x[:, :f], zero[:, :f], ones[:, :f], reduce=False)
        assert not rows.any() and not defined.any()


@pytest.mark.parametrize('reduce', [0, 1])
def test_every_element_is_written_and_nothing_past_the_end(reduce):
    n, f, P = 3, S + 4, 65
    g, h, v, _, want_def = _case(n, f, P)
    g, h = g.copy(), h.copy()
    g[~v], h[~v] = np.nan, np.inf                      # what a frame that does not count holds is never used
    width, guard = (6 if reduce else 3 * P), 5
    rows = torch.full((n * f + guard, width), float('nan'), dtype=torch.float64, device=DEV)
    defined = torch.full((n * f + guard,), 0xEE, dtype=torch.uint8, device=DEV)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    xg, xh, vv = dev(g), dev(h), dev(v.astype(np.uint8))
    _lib.check(_lib.lib().empose_temporal_rows(n, f, P, _lib.dptr(xg), _lib.dptr(xh), _lib.dptr(vv), FPS, reduce,
                                               _lib.dptr(rows), _lib.dptr(defined), _lib.current_stream()))
    rows, defined = rows.cpu().numpy(), defined.cpu().numpy()
    assert np.isfinite(rows[:n * f]).all() and np.isnan(rows[n * f:]).all()
    assert np.array_equal(defined[:n * f].reshape(n, f), want_def) and (defined[n * f:] == 0xEE).all()
    assert not rows[:n * f].reshape(n, f, width)[n - 1].any()          # the row without a counting frame


# ---- the engine against float64 through the oracle ----------------------------------------------------------------------------
def _trajectories(rng, n, f):
    """Smooth pose trajectories: the draws of tests/test_mesh_vjp.py (pose ~ N(0, 0.4), root ~ N(0, 0.5), betas ~ N(0, 1))
    modulated by sinusoids in time; the estimate is the truth plus N(0, 0.02) per frame."""
    t = np.arange(f)[None, :, None] / FPS
    wave = lambda d: 0.6 + 0.4 * np.sin(2 * np.pi * rng.uniform(0.5, 3.0, size=(n, 1, d)) * t +
                                        rng.uniform(0, 2 * np.pi, size=(n, 1, d)))
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    pose = f32(rng.normal(0, 0.4, size=(n, 1, 63)) * wave(63))
    root = f32(rng.normal(0, 0.5, size=(n, 1, 3)) * wave(3))
    shape = f32(rng.normal(0, 1, size=(n, 10)))
    pose_hat = f32(pose + rng.normal(0, 0.02, size=pose.shape))
    root_hat = f32(root + rng.normal(0, 0.02, size=root.shape))
    shape_hat = f32(shape + rng.normal(0, 0.3, size=shape.shape))
    return dict(pose=pose, pose_root=root, shape=shape, pose_hat=pose_hat, pose_root_hat=root_hat, shape_hat=shape_hat)


def _on_device(d):
    return {k: torch.from_numpy(v).to(DEV) for k, v in d.items()}


def _oracle64(model, d, rows=None):
    """float64 (vertices, joints) of both bodies, (n, f, ., 3) numpy."""
    bm = R.BodyModelTensors(model, dtype=torch.float64)
    n, f = d['pose'].shape[:2]
    t = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64))
    out = []
    for p, r, s in ((d['pose'], d['pose_root'], d['shape']), (d['pose_hat'], d['pose_root_hat'], d['shape_hat'])):
        v, j = R.smpl_fk(bm, t(p).reshape(n * f, -1), t(np.repeat(s, f, axis=0)), t(r).reshape(n * f, -1))
        if rows is not None:
            v = v[:, torch.from_numpy(np.asarray(rows, dtype=np.int64))]
        out.append((v.numpy().reshape(n, f, -1, 3), j[:, :22].numpy().reshape(n, f, 22, 3)))
    return out


def _layer_positions(layer, d):
    """What the existing layer gives for the same inputs: (vertices, joints) of both bodies, float64 numpy."""
    n, f = d['pose'].shape[:2]
    g = _on_device(d)
    flat = lambda t: t.reshape(n * f, -1)
    rep = lambda s: s.unsqueeze(1).expand(n, f, 10).reshape(n * f, 10)
    out = []
    for p, r, s in ((g['pose'], g['pose_root'], g['shape']), (g['pose_hat'], g['pose_root_hat'], g['shape_hat'])):
        v = layer(flat(p), rep(s), poses_root=flat(r))[0]
        j = layer.fk_joints(flat(p), rep(s), poses_root=flat(r))
        out.append((v.cpu().numpy().astype(np.float64).reshape(n, f, -1, 3),
                    j.cpu().numpy().astype(np.float64).reshape(n, f, 22, 3)))
    return out


def _validity(n, f):
    seq_lengths = torch.tensor([f, f - 7][:n])
    frame_mask = torch.ones(n, f, 12)
    frame_mask[0, 11, 4] = 0          # a frame with a missing sensor does not count
    return seq_lengths, frame_mask, MetricsEngine.valid_frames(seq_lengths, n, f, frame_mask).numpy()


@pytest.mark.parametrize('which', ['small', 'large'])
def test_engine_end_to_end_against_float64(which):
    model = H.small_model() if which == 'small' else synthetic.make_model()
    layer = SMPLLayer(model).to(DEV)
    V = model['v_template'].shape[0]
    n, f = 2, 40
    d = _trajectories(np.random.default_rng(31), n, f)
    seq_lengths, frame_mask, valid = _validity(n, f)
    eng = TemporalMetricsEngine(layer, surface=True, slab_frames=64)
    eng.compute(seq_lengths=seq_lengths.to(DEV), frame_mask=frame_mask.to(DEV), **_on_device(d))
    got = eng.state()
    ref, ours = _oracle64(model, d), _layer_positions(layer, d)
    dist = lambda a, b: float(np.linalg.norm(a - b, axis=-1).max())
    eps_j = max(dist(ours[b][1], ref[b][1]) for b in (0, 1))
    eps_v = max(dist(ours[b][0], ref[b][0]) for b in (0, 1))
    rows, defined = T.rows64(ref[0][1], ref[1][1], valid, FPS)
    assert int(((defined & T.ACC) != 0).sum()) == (40 - 2 - 3) + (33 - 2)
    assert int(((defined & T.JERK) != 0).sum()) == (40 - 3 - 4) + (33 - 3)
    want = T.families(rows, defined)
    x = max(np.abs(ref[0][1]).max(), np.abs(ref[1][1]).max())
    bars = {'accel': 2 * 4 * FPS ** 2 * eps_j + U * x * FPS ** 2, 'jitter': 8 * FPS ** 3 * eps_j + U * x * FPS ** 3}
    bars['jitter_gt'] = bars['jitter']
    print('{} model: eps joints {:.3e} m, vertices {:.3e} m; bounds accel {:.3e} m/s^2, jitter (8 fps^3 eps) {:.3e} m/s^3'
          .format(which, eps_j, eps_v, bars['accel'], 8 * FPS ** 3 * eps_j))
    for k in ('accel', 'jitter', 'jitter_gt'):
        assert got[k].shape == want[k].shape, k
        err = float(np.abs(got[k] - want[k]).max())
        print('  {}: largest {:.4e}, err {:.3e}, bound {:.3e}'.format(k, float(want[k].max()), err, bars[k]))
        assert err <= bars[k], k
    # the surface: per frame the sums over the vertices and the sums of squares
    vrows, vdef = T.rows64(ref[0][0], ref[1][0], valid, FPS)
    assert np.array_equal(vdef, defined)
    vsums = T.reduced64(vrows)
    xv = max(np.abs(ref[0][0]).max(), np.abs(ref[1][0]).max())
    vbars = (2 * 4 * FPS ** 2 * eps_v + U * xv * FPS ** 2, 8 * FPS ** 3 * eps_v + U * xv * FPS ** 3)
    print('  surface: V {}, bounds per vertex accel {:.3e} m/s^2, jitter (8 fps^3 eps) {:.3e} m/s^3'.format(
        V, vbars[0], 8 * FPS ** 3 * eps_v))
    acc, jerk = (defined & T.ACC) != 0, (defined & T.JERK) != 0
    for k, pick, q, b in (('v_accel', acc, 0, vbars[0]), ('v_jitter', jerk, 1, vbars[1]), ('v_jitter_gt', jerk, 2, vbars[1])):
        want_k = vsums[pick][:, 2 * q:2 * q + 2]
        top = float(vrows[..., q * V:(q + 1) * V].max())
        assert got[k].shape == want_k.shape, k
        err = np.abs(got[k] - want_k).max(axis=0)
        bound = (V * b, V * b * (2 * top + b))
        print('  {}: sums err {:.3e} bound {:.3e}; sums of squares err {:.3e} bound {:.3e}'.format(
            k, err[0], bound[0], err[1], bound[1]))
        assert err[0] <= bound[0] and err[1] <= bound[1], k
    m = eng.get_metrics()
    assert all(np.isfinite(x_) for x_ in m.values()) and len(m) == 12
    assert m['Jitter [m/s^3]'] > m['Jitter GT [m/s^3]'] > 0 and m['V-Jitter [m/s^3]'] > m['V-Jitter GT [m/s^3]'] > 0


# ---- chunks and slabs, bit for bit ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('chunk,second_len', [(7, 6), (16, 12)])
def test_chunked_compute_equals_whole_compute_bit_for_bit(chunk, second_len):
    layer = SMPLLayer(H.small_model()).to(DEV)
    n, f = 2, 40
    d = _on_device(_trajectories(np.random.default_rng(32), n, f))
    lens = [f, second_len]
    frame_mask = torch.ones(n, f, 12, device=DEV)
    frame_mask[0, 20, 3] = 0
    whole = TemporalMetricsEngine(layer)
    whole.compute(seq_lengths=torch.tensor(lens, device=DEV), frame_mask=frame_mask, **d)
    want = whole.state()
    assert want['accel'].shape == ((f - 2 - 3) + (second_len - 2), 22)
    eng = TemporalMetricsEngine(layer)
    calls = []
    for c, sf in enumerate(range(0, f, chunk)):
        ef = min(sf + chunk, f)
        k = sum(1 for n_ in lens if n_ > sf)
        cut = lambda key: d[key][:k, sf:ef]
        eng.compute(cut('pose'), d['shape'][:k], cut('pose_hat'), d['shape_hat'][:k],
                    torch.tensor([min(max(n_ - sf, 0), ef - sf) for n_ in lens[:k]], device=DEV), cut('pose_root'),
                    cut('pose_root_hat'), frame_mask=frame_mask[:k, sf:ef], is_new_sequence=(c == 0))
        calls.append(k)
    assert calls[0] == 2 and calls[1] == 1
    got = eng.state()
    for key in want:
        assert np.array_equal(got[key], want[key]), key
    with pytest.raises(ValueError):
        eng.compute(is_new_sequence=False, **d)             # more rows than the call before


def test_surface_rows_do_not_depend_on_the_slab_bit_for_bit():
    base = SMPLLayer(H.small_model()).to(DEV)
    ids = [int(v) for v in H.load_case('train_lgdrnn12_n2')['meta']['vertex_ids']]
    n, f = 2, 40
    d = _on_device(_trajectories(np.random.default_rng(33), n, f))
    lens = torch.tensor([f, 29], device=DEV)
    firsts = []
    for layer in (base, base.sub_mesh(ids)):
        states = []
        for slab in (5, 16, 1024):
            eng = TemporalMetricsEngine(layer, surface=True, slab_frames=slab)
            eng.compute(seq_lengths=lens, **d)
            states.append(eng.state())
        assert states[0]['v_accel'].shape == (38 + 27, 2) and states[0]['v_jitter'].shape == (37 + 26, 2)
        assert (states[0]['v_jitter'] > 0).all()
        for st in states[1:]:
            for key in states[0]:
                assert np.array_equal(st[key], states[0][key]), key
        firsts.append(states[0])
    # the sub-mesh layer gives the figures over its 60 vertices, not over the 160
    assert layer.n_vertices == 60 and (firsts[1]['v_accel'][:, 0] < firsts[0]['v_accel'][:, 0]).all()


# ---- the opt-in wiring ------------------------------------------------------------------------------------------------------------
def test_evaluate_with_a_temporal_engine_changes_nothing_else():
    from em_pose_amd.data.data import AMASSBatch, AMASSSample
    from em_pose_amd.data.transforms import ToTensor, get_end_to_end_preprocess_fn
    from em_pose_amd.eval.helpers import evaluate
    from em_pose_amd.helpers.configuration import lgd_config
    from em_pose_amd.nn.models import create_model
    case = H.load_case('train_lgdrnn12_n2')
    meta = case['meta']
    model, vids = H.small_model(), [int(v) for v in meta['vertex_ids']]
    smpl = SMPLLayer(model).to(DEV)
    cfg = lgd_config(int(meta['n_markers']), bool(meta['rnn']), int(meta['N']), hidden=32, rnn_hidden=32)
    net = create_model(cfg, SMPLLayer(model))
    net.load_state_dict(H.sd_to_torch(case['sd']), strict=False)
    net.vertex_ids = vids
    net = net.to(DEV).eval()
    rng = np.random.default_rng(9)
    offsets = {'means': rng.normal(0, 0.02, size=(12, 3)).astype(np.float32), 'covs': None,
               'r': np.tile(np.eye(3, dtype=np.float32), (12, 1, 1)), 'vertex_ids': np.asarray(vids)}
    fn = get_end_to_end_preprocess_fn(cfg, smpl, [offsets])
    batches = ((6, 4), (5,))

    def loader():
        r = np.random.default_rng(10)
        for lens in batches:
            yield AMASSBatch.from_sample_list([ToTensor()(AMASSSample(
                's', r.normal(0, 0.2, size=(n, 66)).astype(np.float32), r.normal(0, 1, size=10).astype(np.float32),
                np.zeros((n, 3), np.float32), 60.0)) for n in lens])
    plain, with_engine, te = MetricsEngine(smpl), MetricsEngine(smpl), TemporalMetricsEngine(smpl)
    te.merge({k: np.ones((3, 22)) for k in ('accel', 'jitter', 'jitter_gt')})     # `evaluate` resets the engine
    losses = evaluate(loader(), net, fn, plain, device=torch.device(DEV))
    losses_te = evaluate(loader(), net, fn, with_engine, device=torch.device(DEV), temporal_engine=te)
    assert losses == losses_te
    assert plain.get_metrics() == with_engine.get_metrics()
    for x, y in zip(plain.state().values(), with_engine.state().values()):
        assert np.array_equal(x, y)
    # the defined stencils, from the masks on the host: every batch is a new sequence, every sensor is present
    n_acc = n_jerk = 0
    for lens in batches:
        valid = np.arange(max(lens))[None, :] < np.asarray(lens)[:, None]
        _, defined = T.rows64(np.zeros(valid.shape + (1, 3)), np.zeros(valid.shape + (1, 3)), valid, FPS)
        n_acc, n_jerk = n_acc + int(((defined & T.ACC) != 0).sum()), n_jerk + int(((defined & T.JERK) != 0).sum())
    st = te.state()
    assert (n_acc, n_jerk) == (9, 6)
    assert st['accel'].shape == (n_acc, 22) and st['jitter'].shape == (n_jerk, 22) and st['jitter_gt'].shape == (n_jerk, 22)
    m = te.get_metrics()
    assert all(np.isfinite(v) and v > 0 for v in m.values())


def test_evaluate_real_script_prints_the_temporal_table_to_stderr():
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    res = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'evaluate_real.py'), '--synthetic',
                          '--max_sequences', '2', '--temporal'], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         timeout=600)
    out, err = res.stdout.decode(), res.stderr.decode()
    print(out)
    print(err)
    assert res.returncode == 0, err
    # stdout is what it is without the flag: the metric table and the throughput line, no temporal word
    lines = out.splitlines()
    assert len(lines) == 6 and 'MPJPE [mm]' in lines[0] and 'Overall average' in lines[4] and 'frames/s' in lines[5]
    assert 'Accel' not in out and 'Jitter' not in out
    table = [ln for ln in err.splitlines() if 'Accel [m/s^2]' in ln]
    assert len(table) == 1
    head = table[0]
    cols = ['Accel [m/s^2]', 'Accel STD', 'Jitter [m/s^3]', 'Jitter STD', 'Jitter GT [m/s^3]', 'Jitter GT STD']
    assert [head.index(c) for c in cols] == sorted(head.index(c) for c in cols)
    overall = [ln for ln in err.splitlines() if 'Overall average' in ln]
    assert len(overall) == 1
    values = [float(x) for x in overall[0].split('Overall average')[1].split()]
    assert len(values) == 6 and all(np.isfinite(x) and x > 0 for x in values)
