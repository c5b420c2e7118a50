"""CPU checks of the Procrustes-aligned per-vertex error (empose_mesh_vertex_error_pa, VertexErrorEngine(procrustes=True)):
the float64 restatement the GPU tests compare against (tests/vertex_error_pa_ref.py) is the joints' alignment, the
boundary -- header, library and ctypes table agree, every refusal precedes the first launch -- and the engine's host
logic on made-up rows."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from em_pose_amd import _lib
from em_pose_amd.eval.mesh_metrics import VertexErrorEngine
from em_pose_amd.eval.metrics import procrustes_align
from tests import vertex_error_pa_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENOMEM = -1, -3
NAMES = ('empose_mesh_vertex_error_pa_workspace_bytes', 'empose_mesh_vertex_error_pa')


# ---- the restatement is the joints' convention ----------------------------------------------------------------------------
@pytest.mark.parametrize('V', [5, 60, 161])
def test_restatement_equals_procrustes_align(V):
    rng = np.random.default_rng(V)
    n = 9
    X = rng.normal(0, 1, size=(n, V, 3))
    Y = rng.normal(0, 1, size=(n, V, 3))
    Y[:4] = 0.7 * X[:4] @ np.linalg.qr(rng.normal(size=(3, 3)))[0] + rng.normal(0, 0.05, size=(4, V, 3)) + 3.0
    want = procrustes_align(X, Y)
    for pivots in ((None, None), (X[:, 0], Y[:, 3])):        # the pivots change nothing
        got = P.align64(X, Y, *pivots)
        assert np.abs(got - want).max() <= 1e-12
        d = P.distances64(X, Y, *pivots)
        assert np.abs(d - np.linalg.norm(X - want, axis=-1)).max() <= 1e-12


def test_restatement_equals_procrustes_align_when_the_best_map_is_a_reflection():
    rng = np.random.default_rng(2)
    X = rng.normal(0, 1, size=(6, 40, 3))
    Y = X * np.array([1.0, 1.0, -1.0]) + rng.normal(0, 0.01, size=X.shape)     # a mirror image: det < 0 before the flip
    X0, Y0 = X - X.mean(1, keepdims=True), Y - Y.mean(1, keepdims=True)
    U, _, Vt = np.linalg.svd(np.swapaxes(X0, 1, 2) @ Y0)
    assert (np.linalg.det(np.swapaxes(Vt, 1, 2) @ np.swapaxes(U, 1, 2)) < 0).all()
    want = procrustes_align(X, Y)
    got = P.align64(X, Y)
    assert np.abs(got - want).max() <= 1e-12
    assert np.linalg.norm(X - got, axis=-1).mean() > 0.1       # a rotation cannot undo the mirror


def test_control_is_the_reference_up_to_float32():
    rng = np.random.default_rng(3)
    X = rng.normal(0, 0.3, size=(4, 70, 3)) + rng.normal(0, 1, size=(4, 1, 3))
    Y = X + rng.normal(0, 0.02, size=X.shape)
    d32 = P.distances32(X, Y, X[:, 0], Y[:, 0])
    assert d32.dtype == np.float32
    assert np.abs(d32 - P.distances64(X, Y)).max() < 2e-6


# ---- the boundary -----------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, 'include', 'empose_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    declared = set(re.findall(r'\b(empose_[a-z0-9_]+)\s*\(', text))
    lib = _lib.lib()
    for n in NAMES:
        assert n in declared, 'header does not declare ' + n
        assert hasattr(lib, n), 'library does not export ' + n
        assert n in _lib.SIGNATURES, 'ctypes table misses ' + n
    decl = re.search(r'int\s+empose_mesh_vertex_error_pa\s*\(([^)]*)\)', text).group(1)
    assert len(decl.split(',')) == len(_lib.SIGNATURES['empose_mesh_vertex_error_pa'][1]) == 12
    decl = re.search(r'size_t\s+empose_mesh_vertex_error_pa_workspace_bytes\s*\(([^)]*)\)', text).group(1)
    assert len(decl.split(',')) == len(_lib.SIGNATURES['empose_mesh_vertex_error_pa_workspace_bytes'][1]) == 2
    assert _lib.SIGNATURES['empose_mesh_vertex_error_pa_workspace_bytes'][0] is ctypes.c_size_t
    # the plain entry point keeps its twelve arguments
    assert len(_lib.SIGNATURES['empose_mesh_vertex_error'][1]) == 12


def _fakes():
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)            # stands in for device pointers: never dereferenced on these paths
    handle_buf = ctypes.create_string_buffer(512)    # a zeroed handle: only its sizes are read, all 0
    return buf, handle_buf, p, ctypes.cast(handle_buf, ctypes.c_void_p)


def test_refuses_bad_arguments_before_any_launch():
    lib = _lib.lib()
    buf, handle_buf, p, handle = _fakes()
    need = lib.empose_mesh_vertex_error_pa_workspace_bytes(handle, 4)
    assert need > 0

    def call(mesh=handle, T=4, poses_a=p, betas_a=p, poses_b=p, betas_b=p, sums=p, ws=p, size=None):
        return lib.empose_mesh_vertex_error_pa(mesh, T, poses_a, betas_a, None, poses_b, betas_b, None, sums, ws,
                                               ctypes.c_size_t(need if size is None else size), None)

    for arg, word in (('mesh', b'mesh'), ('poses_a', b'poses_a'), ('betas_a', b'betas_a'), ('poses_b', b'poses_b'),
                      ('betas_b', b'betas_b'), ('sums', b'sums'), ('ws', b'workspace')):
        assert call(**{arg: None}) == EINVAL, arg
        assert word in lib.empose_last_error(), (arg, lib.empose_last_error())
    for T in (0, -1):
        assert call(T=T) == EINVAL
        assert b'T must be positive' in lib.empose_last_error()
    assert call(size=need - 1) == ENOMEM
    assert b'workspace' in lib.empose_last_error()
    assert call(size=0) == ENOMEM


def test_workspace_query_is_zero_for_a_null_handle_and_bad_sizes():
    lib = _lib.lib()
    _, handle_buf, _, handle = _fakes()
    query = lib.empose_mesh_vertex_error_pa_workspace_bytes
    for T in (4, 0, -1):
        assert query(None, T) == 0
    assert query(handle, 0) == 0
    assert query(handle, -7) == 0
    assert 0 < query(handle, 100) < query(handle, 16384)
    # a slab bounds the scratch: more frames than one slab need no more
    assert query(handle, 16384) == query(handle, 16385) == query(handle, 100000)


# ---- the engine's bookkeeping -------------------------------------------------------------------------------------------------
class _Layer(object):
    def __init__(self, n_vertices):
        self.n_vertices = n_vertices


def _rows(d):
    return np.stack([d.sum(axis=1), (d * d).sum(axis=1)], axis=1)


def test_engine_keys_and_their_order_in_both_modes_and_nan_when_empty():
    plain, pa = VertexErrorEngine(_Layer(7)), VertexErrorEngine(_Layer(7), procrustes=True)
    assert not plain.procrustes and pa.procrustes
    got = plain.get_metrics()
    assert list(got) == ['PVE [mm]', 'PVE STD'] and all(math.isnan(v) for v in got.values())
    got = pa.get_metrics()
    assert list(got) == ['PVE [mm]', 'PVE STD', 'PA-PVE [mm]', 'PA-PVE STD']
    assert all(math.isnan(v) for v in got.values())
    assert list(plain.state()) == ['sums'] and plain.state()['sums'].shape == (0, 2)
    st = pa.state()
    assert list(st) == ['sums', 'sums_pa'] and st['sums'].shape == (0, 2) and st['sums_pa'].shape == (0, 2)


def test_engine_metrics_against_numpy_on_constructed_distances():
    rng = np.random.default_rng(0)
    V = 7
    d = np.abs(rng.normal(0.04, 0.02, size=(11, V)))          # per-vertex distances of 11 frames, metres
    d_pa = d * rng.uniform(0.1, 0.9, size=d.shape)            # ... and after the alignment
    eng = VertexErrorEngine(_Layer(V), procrustes=True)
    eng.merge({'sums': _rows(d[:4]), 'sums_pa': _rows(d_pa[:4])})
    eng.merge({'sums': np.zeros((0, 2)), 'sums_pa': np.zeros((0, 2))})
    eng.merge({'sums': _rows(d[4:]), 'sums_pa': _rows(d_pa[4:])})
    got = eng.get_metrics()
    assert list(got) == ['PVE [mm]', 'PVE STD', 'PA-PVE [mm]', 'PA-PVE STD']
    assert got['PVE [mm]'] == pytest.approx(d.mean() * 1000.0, rel=1e-12)
    assert got['PVE STD'] == pytest.approx(np.std(d) * 1000.0, rel=1e-9)
    assert got['PA-PVE [mm]'] == pytest.approx(d_pa.mean() * 1000.0, rel=1e-12)
    assert got['PA-PVE STD'] == pytest.approx(np.std(d_pa) * 1000.0, rel=1e-9)
    # the first two are what the plain engine makes of the same 'sums'
    plain = VertexErrorEngine(_Layer(V))
    plain.merge({'sums': eng.state()['sums']})
    assert plain.get_metrics() == {k: got[k] for k in ('PVE [mm]', 'PVE STD')}
    eng.reset()
    assert eng.state()['sums_pa'].shape == (0, 2) and math.isnan(eng.get_metrics()['PA-PVE [mm]'])


def test_engine_state_merge_round_trip_and_refusals():
    rng = np.random.default_rng(1)
    mk = lambda m: (_rows(rng.uniform(0, 0.1, size=(m, 9))), _rows(rng.uniform(0, 0.05, size=(m, 9))))
    (a0, a1), (b0, b1) = mk(5), mk(3)
    a, b, both = (VertexErrorEngine(_Layer(9), procrustes=True) for _ in range(3))
    a.merge({'sums': a0, 'sums_pa': a1})
    b.merge({'sums': b0, 'sums_pa': b1})
    both.merge({'sums': np.concatenate([a0, b0]), 'sums_pa': np.concatenate([a1, b1])})
    a.merge(b.state())
    st = a.state()
    assert st['sums'].dtype == np.float64 and st['sums_pa'].dtype == np.float64
    assert np.array_equal(st['sums'], np.concatenate([a0, b0])) and np.array_equal(st['sums_pa'], np.concatenate([a1, b1]))
    assert a.get_metrics() == both.get_metrics()
    fresh = VertexErrorEngine(_Layer(9), procrustes=True)
    fresh.merge(st)
    assert all(np.array_equal(fresh.state()[k], st[k]) for k in st)
    assert a.gather() is a and np.array_equal(a.state()['sums_pa'], st['sums_pa'])   # no process group: nothing to do
    # a state without the aligned rows does not go into a Procrustes engine, and leaves it as it was
    with pytest.raises(ValueError, match='sums_pa'):
        fresh.merge({'sums': a0})
    with pytest.raises(ValueError):
        fresh.merge({'sums': a0, 'sums_pa': b1})
    assert all(np.array_equal(fresh.state()[k], st[k]) for k in st)
    # the other way round is the plain engine's merge: it reads 'sums'
    plain = VertexErrorEngine(_Layer(9))
    plain.merge(st)
    assert list(plain.state()) == ['sums'] and np.array_equal(plain.state()['sums'], st['sums'])
