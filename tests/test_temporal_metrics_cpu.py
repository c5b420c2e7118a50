"""CPU checks of the temporal metrics (eval/temporal_metrics.py, empose_temporal_rows): the float64 restatement the GPU
tests compare against (tests/temporal_ref.py) and the engine's NumPy path give the known answers and agree on validity; the
engine's bookkeeping -- chunked feeding equals whole feeding bit for bit, state / merge / gather, the columns; and the
boundary: header, library and ctypes table agree, every refusal precedes the first launch and names its argument."""
import ctypes
import math
import os
import re
import socket

import numpy as np
import pytest
import torch

from em_pose_amd import _lib
from em_pose_amd.eval import temporal_metrics as TM
from em_pose_amd.eval.temporal_metrics import TemporalMetricsEngine
from em_pose_amd.helpers.configuration import CONSTANTS as C
from tests import temporal_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
FPS = 60.0
IMPLS = {'restatement': T.rows64, 'numpy path': TM.temporal_rows_numpy}


def _engine_rows(x_gt, x_hat, valid, chunk=None):
    """The engine's accumulated families from `compute_points` on CPU tensors, whole or in chunks of `chunk` frames; rows
    that have ended (no counting frame from the chunk's start on) leave the batch, as in the batched driver."""
    eng = TemporalMetricsEngine(None)
    g, h, v = torch.from_numpy(x_gt), torch.from_numpy(x_hat), torch.from_numpy(valid)
    f = g.shape[1]
    if chunk is None:
        eng.compute_points(g, h, v)
    else:
        lens = [int(np.flatnonzero(valid[i])[-1]) + 1 if valid[i].any() else 0 for i in range(g.shape[0])]
        assert lens == sorted(lens, reverse=True)
        for c, sf in enumerate(range(0, f, chunk)):
            k = max(1, sum(1 for n_ in lens if n_ > sf)) if c > 0 else g.shape[0]
            ef = min(sf + chunk, f)
            eng.compute_points(g[:k, sf:ef], h[:k, sf:ef], v[:k, sf:ef], is_new_sequence=(c == 0))
    return eng


# ---- known answers --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('impl', sorted(IMPLS))
def test_cubic_and_quadratic_known_answers(impl):
    t = np.arange(8, dtype=np.float64)
    zero = np.zeros((1, 8, 1, 3), np.float32)
    cubic, quad = zero.copy(), zero.copy()
    cubic[0, :, 0, 0] = t ** 3        # exact in float32
    quad[0, :, 0, 1] = t ** 2
    ones = np.ones((1, 8), bool)
    rows, defined = IMPLS[impl](cubic, zero, ones, FPS)
    assert defined[0].tolist() == [0, 0, 1, 3, 3, 3, 3, 3]
    assert np.array_equal(rows[0, 3:, 2], np.full(5, 6.0 * FPS ** 3))      # |jerk_gt| = 6 fps^3 exactly
    assert np.array_equal(rows[0, :3, 2], np.zeros(3)) and np.array_equal(rows[0, :, 1], np.zeros(8))
    assert np.array_equal(rows[0, 2:, 0], (6.0 * t[2:] - 6.0) * FPS ** 2)   # acc of t^3 by the backward stencil: 6 (t - 1)
    rows, defined = IMPLS[impl](zero, quad, ones, FPS)
    assert np.array_equal(rows[0, 2:, 0], np.full(6, 2.0 * FPS ** 2))      # |acc_gt - acc_hat| = 2 fps^2 exactly
    assert np.array_equal(rows[0, :, 1], np.zeros(8)) and np.array_equal(rows[0, :, 2], np.zeros(8))


def test_engine_numpy_path_gives_the_known_answers():
    t = np.arange(8, dtype=np.float64)
    x = np.zeros((1, 8, 2, 3), np.float32)
    x[0, :, 0, 0] = t ** 3
    x[0, :, 1, 2] = t ** 2
    eng = _engine_rows(x, np.zeros_like(x), np.ones((1, 8), bool))
    st = eng.state()
    assert st['accel'].shape == (6, 2) and st['jitter'].shape == (5, 2) and st['jitter_gt'].shape == (5, 2)
    assert np.array_equal(st['jitter_gt'], np.tile([6.0 * FPS ** 3, 0.0], (5, 1)))
    assert np.array_equal(st['accel'][:, 1], np.full(6, 2.0 * FPS ** 2))
    assert not st['jitter'].any()


# ---- validity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('impl', sorted(IMPLS))
def test_an_invalid_frame_removes_its_stencils_and_nothing_else(impl):
    rng = np.random.default_rng(0)
    f = 20
    g, h = T.smooth_points(rng, 1, f, 3)
    full, full_def = IMPLS[impl](g, h, np.ones((1, f), bool), FPS)
    assert full_def[0].tolist() == [0, 0, 1] + [3] * (f - 3)
    for k in (0, 1, 5, 17, 19):
        v = np.ones((1, f), bool)
        v[0, k] = False
        gk, hk = g.copy(), h.copy()
        gk[0, k], hk[0, k] = np.nan, np.inf          # what an invalid frame holds is never used
        rows, defined = IMPLS[impl](gk, hk, v, FPS)
        want = full_def.copy()
        want[0, k:k + 3] &= ~np.uint8(T.ACC)
        want[0, k:k + 4] &= ~np.uint8(T.JERK)
        assert np.array_equal(defined, want), k
        acc, jerk = (want[0] & T.ACC) != 0, (want[0] & T.JERK) != 0
        assert np.array_equal(rows[0, acc, :3], full[0, acc, :3]) and not rows[0, ~acc, :3].any()
        assert np.array_equal(rows[0, jerk, 3:], full[0, jerk, 3:]) and not rows[0, ~jerk, 3:].any()
        assert np.isfinite(rows).all()


@pytest.mark.parametrize('impl', sorted(IMPLS))
@pytest.mark.parametrize('f,n_acc,n_jerk', [(1, 0, 0), (2, 0, 0), (3, 1, 0), (4, 2, 1)])
def test_short_sequences_define_the_right_number_of_frames(impl, f, n_acc, n_jerk):
    g, h = T.smooth_points(np.random.default_rng(f), 2, f, 4)
    rows, defined = IMPLS[impl](g, h, np.ones((2, f), bool), FPS)
    assert rows.shape == (2, f, 12) and defined.shape == (2, f)
    for i in range(2):
        assert int(((defined[i] & T.ACC) != 0).sum()) == n_acc and int(((defined[i] & T.JERK) != 0).sum()) == n_jerk


@pytest.mark.parametrize('impl', sorted(IMPLS))
def test_a_stencil_never_reads_another_row(impl):
    rng = np.random.default_rng(2)
    g, h = T.smooth_points(rng, 3, 9, 5)
    v = T.ragged_valid(rng, 3, 9, rate=0.1)
    rows, defined = IMPLS[impl](g, h, v, FPS)
    for i in range(3):
        alone, alone_def = IMPLS[impl](g[i:i + 1], h[i:i + 1], v[i:i + 1], FPS)
        assert np.array_equal(alone[0], rows[i]) and np.array_equal(alone_def[0], defined[i])
    assert (defined[:, :2] == 0).all() and ((defined[:, 2] & T.JERK) == 0).all()     # a row starts from nothing
    g2 = g.copy()
    g2[0] += 1.0e3
    other, _ = IMPLS[impl](g2, h, v, FPS)
    assert np.array_equal(other[1:], rows[1:])


def test_numpy_path_equals_the_restatement():
    rng = np.random.default_rng(3)
    g, h = T.smooth_points(rng, 3, 41, 22)
    v = T.ragged_valid(rng, 3, 41, dead_row=1)
    rows, defined = TM.temporal_rows_numpy(g, h, v, FPS)
    want, want_def = T.rows64(g, h, v, FPS)
    assert np.array_equal(defined, want_def) and not defined[1].any()
    scale = 64 * 2.0 ** -52 * 8 * max(np.abs(g).max(), np.abs(h).max())
    assert np.abs(rows[..., :22] - want[..., :22]).max() <= scale * FPS ** 2
    assert np.abs(rows[..., 22:] - want[..., 22:]).max() <= scale * FPS ** 3
    assert not rows[defined == 0].any()


# ---- chunked feeding ----------------------------------------------------------------------------------------------------------
def _ragged_case():
    rng = np.random.default_rng(4)
    lens = [23, 11, 2]
    g, h = T.smooth_points(rng, 3, 23, 6)
    v = T.ragged_valid(rng, 3, 23, rate=0.08)
    for i, n_ in enumerate(lens):
        v[i, n_:] = False
        v[i, n_ - 1] = True
    return g, h, v


@pytest.mark.parametrize('chunk', [1, 2, 3, 5, 256])
def test_chunked_feeding_equals_whole_feeding_bit_for_bit(chunk):
    g, h, v = _ragged_case()
    whole = _engine_rows(g, h, v).state()
    rows, defined = T.rows64(g, h, v, FPS)
    want = T.families(*TM.temporal_rows_numpy(g, h, v, FPS))
    assert whole['accel'].shape[0] == int(((defined & T.ACC) != 0).sum()) > 10
    assert whole['jitter'].shape[0] == int(((defined & T.JERK) != 0).sum()) > 5
    for k in want:
        assert np.array_equal(whole[k], want[k]), k       # batch row after batch row, frames in order
    chunked = _engine_rows(g, h, v, chunk=chunk).state()
    for k in whole:
        assert np.array_equal(chunked[k], whole[k]), (chunk, k)


def test_a_row_shorter_than_three_frames_is_continued():
    rng = np.random.default_rng(5)
    g, h = T.smooth_points(rng, 2, 9, 3)
    v = np.ones((2, 9), bool)
    whole = _engine_rows(g, h, v).state()
    eng = TemporalMetricsEngine(None)
    tt = torch.from_numpy
    eng.compute_points(tt(g[:, :2]), tt(h[:, :2]), tt(v[:, :2]))
    assert eng.state()['accel'].shape == (0, 3)
    eng.reset()
    for c, (sf, ef) in enumerate(((0, 2), (2, 3), (3, 9))):
        eng.compute_points(tt(g[:, sf:ef]), tt(h[:, sf:ef]), tt(v[:, sf:ef]), is_new_sequence=(c == 0))
    for k, rows in eng.state().items():
        assert np.array_equal(rows, whole[k]), k
    assert whole['accel'].shape == (14, 3) and whole['jitter'].shape == (12, 3)


def test_a_new_sequence_starts_from_nothing_and_continuation_is_checked():
    rng = np.random.default_rng(6)
    g, h = T.smooth_points(rng, 2, 6, 3)
    tt = torch.from_numpy
    eng = TemporalMetricsEngine(None)
    with pytest.raises(ValueError, match='no previous call'):
        eng.compute_points(tt(g), tt(h), is_new_sequence=False)
    eng.compute_points(tt(g[:1]), tt(h[:1]))
    with pytest.raises(ValueError, match='first k'):
        eng.compute_points(tt(g), tt(h), is_new_sequence=False)          # more rows than the call before
    eng.compute_points(tt(g[:1]), tt(h[:1]))                              # a new sequence: the stencils start again
    st = eng.state()
    assert st['accel'].shape == (8, 3) and st['jitter'].shape == (6, 3)
    assert np.array_equal(st['accel'][:4], st['accel'][4:])
    with pytest.raises(ValueError, match='points'):
        eng.compute_points(tt(g[:, :, :2]), tt(h[:, :, :2]))
    eng.reset()
    with pytest.raises(ValueError, match='no previous call'):
        eng.compute_points(tt(g), tt(h), is_new_sequence=False)
    with pytest.raises(_lib.EmposeError):
        eng.compute(torch.zeros(1, 4, 63), torch.zeros(1, 10), torch.zeros(1, 4, 63))     # `compute` has no CPU path
    for bad in (dict(fps=0.0), dict(fps=float('inf')), dict(slab_frames=3)):
        with pytest.raises(ValueError):
            TemporalMetricsEngine(None, **bad)


# ---- columns, state, merge, gather ------------------------------------------------------------------------------------------
class _Layer(object):
    def __init__(self, n_vertices):
        self.n_vertices = n_vertices


def test_columns_and_nan_when_empty():
    eng = TemporalMetricsEngine(None)
    got = eng.get_metrics()
    assert list(got) == ['Accel [m/s^2]', 'Accel STD', 'Jitter [m/s^3]', 'Jitter STD', 'Jitter GT [m/s^3]', 'Jitter GT STD']
    assert all(math.isnan(x) for x in got.values())
    assert eng.fps == C.FPS == 60.0 and not eng.surface and eng.slab_frames == 1024
    assert list(eng.state()) == ['accel', 'jitter', 'jitter_gt'] and eng.state()['accel'].shape == (0, 22)
    surf = TemporalMetricsEngine(_Layer(7), surface=True)
    got = surf.get_metrics()
    assert list(got)[6:] == ['V-Accel [m/s^2]', 'V-Accel STD', 'V-Jitter [m/s^3]', 'V-Jitter STD', 'V-Jitter GT [m/s^3]',
                             'V-Jitter GT STD']
    assert len(got) == 12 and all(math.isnan(x) for x in got.values())
    assert list(surf.state()) == ['accel', 'jitter', 'jitter_gt', 'v_accel', 'v_jitter', 'v_jitter_gt']
    assert surf.state()['v_jitter'].shape == (0, 2)
    # three frames define an acceleration and no jerk: that family stays NaN
    g, h = T.smooth_points(np.random.default_rng(7), 1, 3, 22)
    eng.compute_points(torch.from_numpy(g), torch.from_numpy(h))
    got = eng.get_metrics()
    assert got['Accel [m/s^2]'] > 0 and math.isnan(got['Jitter [m/s^3]']) and math.isnan(got['Jitter GT STD'])
    assert 'Accel' in eng.to_pretty_string(got, 'model')


def test_get_metrics_against_numpy():
    rng = np.random.default_rng(8)
    g, h = T.smooth_points(rng, 3, 30, 22, noise=5e-3)
    v = T.ragged_valid(rng, 3, 30, rate=0.05)
    eng = _engine_rows(g, h, v)
    fam = T.families(*T.rows64(g, h, v, FPS))
    for select in (True, False):
        got, want = eng.get_metrics(eucl_idxs_select=select), T.joint_columns(fam, select)
        assert list(got) == list(want)
        for k in want:
            assert got[k] == pytest.approx(want[k], rel=1e-9), k
    assert eng.get_metrics()['Accel [m/s^2]'] != eng.get_metrics(eucl_idxs_select=False)['Accel [m/s^2]']
    assert eng.get_metrics()['Jitter [m/s^3]'] > eng.get_metrics()['Jitter GT [m/s^3]'] > 0
    # the surface columns from per-frame sums and sums of squares, as PVE
    V = 9
    d = np.abs(rng.normal(3.0, 1.0, size=(3, 12, V)))       # per-vertex values of the three quantities, 12 frames
    sums = lambda x: np.stack([x.sum(axis=1), (x * x).sum(axis=1)], axis=1)
    surf = TemporalMetricsEngine(_Layer(V), surface=True)
    surf.merge({'accel': np.ones((12, 22)), 'jitter': np.ones((10, 22)), 'jitter_gt': np.ones((10, 22)),
                'v_accel': sums(d[0]), 'v_jitter': sums(d[1, :10]), 'v_jitter_gt': sums(d[2, :10])})
    got = surf.get_metrics()
    for name, x in (('V-Accel [m/s^2]', d[0]), ('V-Jitter [m/s^3]', d[1, :10]), ('V-Jitter GT [m/s^3]', d[2, :10])):
        assert got[name] == pytest.approx(x.mean(), rel=1e-12)
        assert got[name.split(' [')[0] + ' STD'] == pytest.approx(np.std(x), rel=1e-9)
    with pytest.raises(ValueError, match='lacks'):
        surf.merge({'accel': np.ones((1, 22)), 'jitter': np.ones((1, 22)), 'jitter_gt': np.ones((1, 22))})
    with pytest.raises(ValueError, match='different frames'):
        surf.merge({'accel': np.ones((2, 22)), 'jitter': np.ones((1, 22)), 'jitter_gt': np.ones((1, 22)),
                    'v_accel': np.ones((1, 2)), 'v_jitter': np.ones((1, 2)), 'v_jitter_gt': np.ones((1, 2))})


def test_state_merge_round_trip_and_gather_in_a_group_of_one():
    import torch.distributed as dist
    rng = np.random.default_rng(9)
    g, h = T.smooth_points(rng, 2, 12, 22)
    tt = torch.from_numpy
    one, two, both = (TemporalMetricsEngine(None) for _ in range(3))
    one.compute_points(tt(g[:1]), tt(h[:1]))
    two.compute_points(tt(g[1:, :7]), tt(h[1:, :7]))
    both.compute_points(tt(g[:1]), tt(h[:1]))
    both.compute_points(tt(g[1:, :7]), tt(h[1:, :7]))
    one.merge(two.state())
    want = both.state()
    assert want['accel'].shape == (10 + 5, 22) and want['jitter'].shape == (9 + 4, 22)
    for k in want:
        assert one.state()[k].dtype == np.float64 and np.array_equal(one.state()[k], want[k]), k
    assert one.get_metrics() == both.get_metrics()
    fresh = TemporalMetricsEngine(None)
    fresh.merge(want)
    fresh.merge({k: np.zeros((0, 22)) for k in want})
    assert all(np.array_equal(fresh.state()[k], want[k]) for k in want)
    with pytest.raises(ValueError, match='different frames'):
        fresh.merge({'accel': want['accel'], 'jitter': want['jitter'], 'jitter_gt': want['jitter_gt'][:3]})
    assert one.gather() is one                                   # no process group: nothing to do
    assert not dist.is_initialized()
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    os.environ['MASTER_ADDR'], os.environ['MASTER_PORT'] = '127.0.0.1', str(port)
    dist.init_process_group('gloo', rank=0, world_size=1)
    try:
        assert one.gather() is one                               # a group of one: nothing to do
        got = one.gather(force=True).state()
        assert all(np.array_equal(got[k], want[k]) for k in want)
        empty = TemporalMetricsEngine(None).gather(force=True)
        assert empty.state()['jitter'].shape[0] == 0 and math.isnan(empty.get_metrics()['Accel [m/s^2]'])
    finally:
        dist.destroy_process_group()
    assert one.get_metrics() == both.get_metrics()


# ---- the boundary ---------------------------------------------------------------------------------------------------------------
def test_symbol_is_declared_exported_and_bound():
    text = open(os.path.join(ROOT, 'include', 'empose_hip.h')).read()
    assert int(re.search(r'#define\s+EMPOSE_TEMPORAL_SEGMENT\s+(\d+)', text).group(1)) == _lib.TEMPORAL_SEGMENT
    assert int(re.search(r'#define\s+EMPOSE_TEMPORAL_ACC\s+(\d+)', text).group(1)) == _lib.TEMPORAL_ACC == T.ACC
    assert int(re.search(r'#define\s+EMPOSE_TEMPORAL_JERK\s+(\d+)', text).group(1)) == _lib.TEMPORAL_JERK == T.JERK
    kernels = open(os.path.join(ROOT, 'em_pose_amd', 'csrc', 'data_kernels.h')).read()
    assert int(re.search(r'TEMPORAL_SEGMENT\s*=\s*(\d+)', kernels).group(1)) == _lib.TEMPORAL_SEGMENT
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    decl = re.search(r'int\s+empose_temporal_rows\s*\(([^)]*)\)', text).group(1)
    assert hasattr(_lib.lib(), 'empose_temporal_rows')
    assert len(decl.split(',')) == len(_lib.SIGNATURES['empose_temporal_rows'][1]) == 11
    assert _lib.SIGNATURES['empose_temporal_rows'][1][6] is ctypes.c_double


def test_refuses_bad_arguments_before_any_launch():
    lib = _lib.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)        # stands in for device pointers: never dereferenced on these paths

    def call(N=2, F=5, P=3, x_gt=p, x_hat=p, valid=p, fps=60.0, reduce=0, rows=p, defined=p):
        return lib.empose_temporal_rows(N, F, P, x_gt, x_hat, valid, fps, reduce, rows, defined, None)
    for arg in ('N', 'F', 'P'):
        for bad in (0, -1):
            assert call(**{arg: bad}) == EINVAL, arg
            assert arg.encode() + b' must be positive' in lib.empose_last_error(), lib.empose_last_error()
    for arg in ('x_gt', 'x_hat', 'valid', 'rows', 'defined'):
        assert call(**{arg: None}) == EINVAL, arg
        assert b'null ' + arg.encode() in lib.empose_last_error(), lib.empose_last_error()
    for bad in (0.0, -60.0, float('inf'), float('nan')):
        assert call(fps=bad) == EINVAL, bad
        assert b'fps' in lib.empose_last_error()
    for bad in (-1, 2):
        assert call(reduce=bad) == EINVAL, bad
        assert b'reduce' in lib.empose_last_error()
    assert call(N=1 << 16, F=1 << 16) == EINVAL
    assert b'N * F' in lib.empose_last_error()
