"""
The float64 restatement of the point-to-mesh query (tests/surface_query_ref.py) held to things known without it, the
tolerance of the GPU test measured from its float32 run, and what of em_pose_amd/eval/surface_metrics.py needs no GPU:
the engine's host arithmetic, the boundary of the C ABI and the argument and limit errors.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from em_pose_amd import _lib
from em_pose_amd.eval import surface_metrics as SM
from tests import helpers as H
from tests import surface_query_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
CONVEX = {'cube': R.cube, 'octahedron': R.octahedron, 'icosahedron': lambda: R.icosahedron(1)}


# ---- the restatement against what is known without it ---------------------------------------------------------------------
def test_helper_meshes_are_closed_and_have_the_stated_sizes():
    sizes = {'tetrahedron': (R.tetrahedron(), 4), 'cube': (R.cube(), 12), 'octahedron': (R.octahedron(), 8),
             'icosahedron': (R.icosahedron(1), 80), 'torus': (R.torus(24, 48), 2 * 24 * 48)}
    for name, ((v, f), n_faces) in sizes.items():
        assert f.shape == (n_faces, 3) and f.min() == 0 and f.max() == len(v) - 1, name
        edges = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
        directed = set(map(tuple, edges.tolist()))
        assert len(directed) == len(edges), name                                 # no directed edge twice
        assert all((b, a) in directed for a, b in directed), name                # every edge has its opposite: closed


@pytest.mark.parametrize('name', sorted(CONVEX))
def test_distance_and_inside_match_the_convex_polytope(name):
    v, f = CONVEX[name]()
    points = np.concatenate([R.random_queries(20, 3, scale=1.6), R.displaced_from_faces(v, f, 10, 0.05, 4),
                             R.displaced_from_faces(v, f, 10, -0.05, 5)])
    got = R.closest_point(v, f, points)
    want = R.convex_distance(v, f, points)
    assert np.abs(got['dist'] - want).max() < 1e-9, np.abs(got['dist'] - want).max()
    assert want.min() > 1e-4                                                      # no query on the surface
    assert np.array_equal(R.inside(v, f, points), R.convex_inside(v, f, points))
    # the reported point is on the reported face, at the reported distance, with the reported weights
    corners = v.astype(np.float64)[f[got['face']]]
    assert np.abs(np.einsum('qk,qkd->qd', got['bary'], corners) - got['closest']).max() < 1e-12
    assert np.abs(np.linalg.norm(points - got['closest'], axis=1) - got['dist']).max() < 1e-12
    assert (got['bary'] >= 0).all() and np.abs(got['bary'].sum(axis=1) - 1).max() < 1e-12


def test_inside_matches_the_analytic_torus_away_from_the_faceting_error():
    nu, nv = 24, 48
    v, f = R.torus(nu, nv)
    delta = 0.02
    assert R.torus_faceting_error(nu, nv) + 1e-4 < delta
    points = np.concatenate([R.torus_displaced(200, delta, 7), R.torus_displaced(200, -delta, 8),
                             R.random_queries(200, 9, scale=1.5)])
    signed = R.torus_signed_distance(points)
    far = np.abs(signed) > R.torus_faceting_error(nu, nv) + 1e-4
    assert far[:400].all() and far.sum() > 500
    assert np.array_equal(R.inside(v, f, points)[far], signed[far] < 0)
    # and the distance to the mesh is the analytic one up to the faceting error
    dist = R.closest_point(v, f, points)['dist']
    assert np.abs(dist - np.abs(signed)).max() < R.torus_faceting_error(nu, nv) + 1e-6


def test_half_open_rule_on_grazing_rays_of_the_cube_is_exact():
    v, f = R.cube()
    points, want = R.grazing_rays()
    assert np.array_equal(R.inside(v, f, points), want)
    # the same on a cube whose faces are listed in reverse and with their corners rotated
    f2 = np.roll(f[::-1], 1, axis=1)
    assert np.array_equal(R.inside(v, f2, points), want)


def test_zero_area_and_duplicated_faces_give_no_nan_and_the_lowest_id():
    v, f = R.degenerate_mesh()
    points = np.concatenate([R.special_queries(v, f), R.random_queries(40, 13, scale=2.5),
                             np.array([[0.75, 0.75, 2.0], [1.0, 1.0, 2.5], [0.5, 0.5, 2.0]], np.float32)])
    for dtype in (np.float32, np.float64):
        got = R.closest_point(v, f, points, dtype)
        assert all(np.isfinite(got[k]).all() for k in ('dist', 'bary', 'closest', 'all_dist'))
        assert (got['face'] != len(f) - 1).all()                                  # the copy of face 0 never beats it
        assert np.array_equal(got['all_dist'][:, 0], got['all_dist'][:, -1])
    assert got['dist'][-3:].tolist() == [0.0, 0.5, 0.0]


# ---- the tolerance of the GPU test ----------------------------------------------------------------------------------------
def test_tolerance_is_four_times_the_float32_error_of_the_restatement():
    worst_dist = worst_closest = 0.0
    for name, vertices, faces, points in R.gpu_cases():
        for k in range(vertices.shape[0]):
            r64 = R.closest_point(vertices[k], faces, points[k], np.float64)
            r32 = R.closest_point(vertices[k], faces, points[k], np.float32)
            scale = R.tolerance(points[k]) / R.TOL_M
            pick = np.arange(points.shape[1])
            worst_dist = max(worst_dist, (np.abs(r32['dist'].astype(np.float64) - r64['dist']) / scale).max())
            on_face = r64['all_closest'][pick, r32['face']]                       # float64 on the face float32 chose
            worst_closest = max(worst_closest, (np.abs(r32['closest'] - on_face).max(axis=1) / scale).max())
    print('float32 - float64: dist %.3g m, closest %.3g m' % (worst_dist, worst_closest))
    worst = max(worst_dist, worst_closest)
    assert R.TOL_MARGIN == 4.0 and R.TOL_MARGIN * worst <= R.TOL_M <= 2.0 * R.TOL_MARGIN * worst
    assert R.TOL_M < 2e-6                                                          # near 1e-6: the formulation does not cancel


# ---- the engine's host arithmetic -------------------------------------------------------------------------------------------
def test_engine_rows_and_columns():
    count = np.array([[1, 1, 0], [0, 0, 0], [1, 0, 1]], np.float32)
    inf = np.inf
    d_hat = np.array([[0.010, 0.020, inf], [inf, inf, inf], [0.030, inf, 0.005]], np.float32)
    in_hat = np.array([[1, 0, 0], [0, 0, 0], [0, 0, 1]], bool)
    d_gt = np.array([[0.004, 0.002, inf], [inf, inf, inf], [0.001, inf, 0.003]], np.float32)
    in_gt = np.zeros((3, 3), bool)
    rows = SM.SkinDistanceEngine.rows_from(count, d_hat, in_hat, d_gt, in_gt)
    f = lambda x: float(np.float32(x))
    assert rows.shape == (2, 6) and rows.dtype == np.float64                       # the frame without a reading is gone
    assert rows[0].tolist() == [2.0, f(0.010) + f(0.020), 1.0, f(0.010), f(0.004) + f(0.002), 0.0]
    assert rows[1].tolist() == [2.0, f(0.030) + f(0.005), 1.0, f(0.005), f(0.001) + f(0.003), 0.0]
    m = SM.SkinDistanceEngine.metrics_from_rows(rows)
    assert list(m) == ['Skin dist [mm]', 'Skin dist GT [mm]', 'Inside [%]', 'Inside GT [%]', 'Depth [mm]']
    assert m['Skin dist [mm]'] == pytest.approx(1e3 * (0.010 + 0.020 + 0.030 + 0.005) / 4, rel=1e-6)
    assert m['Skin dist GT [mm]'] == pytest.approx(1e3 * 0.010 / 4, rel=1e-6)
    assert m['Inside [%]'] == 50.0 and m['Inside GT [%]'] == 0.0
    assert m['Depth [mm]'] == pytest.approx(1e3 * (0.010 + 0.005) / 2, rel=1e-6)
    none_inside = rows.copy()
    none_inside[:, 2:4] = 0.0
    assert SM.SkinDistanceEngine.metrics_from_rows(none_inside)['Depth [mm]'] == 0.0
    assert all(np.isnan(x) for x in SM.SkinDistanceEngine.metrics_from_rows(np.zeros((0, 6))).values())


def test_engine_state_merge_and_pretty_string():
    rows = np.arange(24, dtype=np.float64).reshape(4, 6) + 1.0
    whole, a, b = (SM.SkinDistanceEngine(None) for _ in range(3))
    whole.merge({'sums': rows})
    a.merge({'sums': rows[:3]})
    b.merge({'sums': rows[3:]})
    a.merge(b.state())
    assert np.array_equal(a.state()['sums'], whole.state()['sums']) and a.get_metrics() == whole.get_metrics()
    a.merge({'sums': np.zeros((0, 6))})
    assert len(a.sums) == 2
    assert a.gather() is a                                                         # no process group: nothing to do
    text = SM.SkinDistanceEngine.to_pretty_string(whole.get_metrics(), 'model')
    assert 'Skin dist [mm]' in text and 'Depth [mm]' in text and 'model' in text
    a.reset()
    assert a.state()['sums'].shape == (0, 6)
    with pytest.raises(ValueError, match='marker_pos'):
        a.compute(torch.zeros(1, 2, 63), torch.zeros(1, 10), torch.zeros(1, 2, 63))


# ---- the boundary -----------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, 'include', 'empose_hip.h')).read()
    for name, value in (('FRAMES', _lib.SURFACE_MAX_FRAMES), ('VERTICES', _lib.SURFACE_MAX_VERTICES), ('FACES', _lib.SURFACE_MAX_FACES),
                        ('QUERIES', _lib.SURFACE_MAX_QUERIES)):
        assert eval(re.search(r'#define\s+EMPOSE_SURFACE_MAX_' + name + r'\s+(\(?[0-9< ]+\)?)', text).group(1)) == value
    end = re.search(r'\}\s*empose_surface_desc;', text).start()
    body = re.sub(r'/\*.*?\*/', '', text[text.rfind('typedef struct {', 0, end) + len('typedef struct {'):end], flags=re.S)
    names = [re.findall(r'([A-Za-z_][A-Za-z0-9_]*)\s*$', part.strip())[0]
             for decl in body.split(';') if decl.strip() for part in decl.split(',')]
    assert names == [f[0] for f in _lib.SurfaceDesc._fields_]
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    lib = _lib.lib()
    for n in ('empose_surface_query_workspace_bytes', 'empose_surface_query'):
        assert hasattr(lib, n) and n in _lib.SIGNATURES
    decl = re.search(r'int\s+empose_surface_query\s*\(([^)]*)\)', text).group(1)
    assert len(decl.split(',')) == len(_lib.SIGNATURES['empose_surface_query'][1]) == 4
    assert _lib.SIGNATURES['empose_surface_query_workspace_bytes'] == (ctypes.c_size_t, [ctypes.c_int] * 4)
    kernels = open(os.path.join(ROOT, 'em_pose_amd', 'csrc', 'surface_kernels.h')).read()
    assert int(re.search(r'SURFACE_MAX_Q\s*=\s*(\d+)', kernels).group(1)) == _lib.SURFACE_MAX_QUERIES


def test_bad_descriptors_are_refused_before_any_launch():
    lib = _lib.lib()
    buf = np.zeros(4096, np.float32)   # host memory: a launch would fault, a refusal never touches it
    p = ctypes.c_void_p(buf.ctypes.data)
    faces = np.array([[0, 1, 2], [2, 1, 3]], np.int32)

    def call(faces=faces, **change):
        d = _lib.SurfaceDesc()
        d.T, d.V, d.F, d.Q = 2, 4, len(faces), 3
        for name in ('vertices', 'faces_dev', 'points', 'dist', 'face', 'bary', 'closest', 'inside'):
            setattr(d, name, p)
        d.faces_host = _lib.iptr(faces)
        for k, v in change.items():
            setattr(d, k, v)
        return lib.empose_surface_query(ctypes.byref(d), None, 0, None)
    assert lib.empose_surface_query(None, None, 0, None) == EINVAL
    for name in ('T', 'V', 'F', 'Q'):
        for bad in (0, -1):
            assert call(**{name: bad}) == EINVAL, name
    for name in ('vertices', 'faces_dev', 'points', 'dist'):
        assert call(**{name: None}) == EINVAL, name
    assert call(faces_host=None) == EINVAL and b'host and its device' in lib.empose_last_error()
    assert call(want_inside=1, inside=None) == EINVAL and b'want_inside' in lib.empose_last_error()
    assert call(Q=_lib.SURFACE_MAX_QUERIES + 1) == EINVAL and b'Q = 4097 above the cap' in lib.empose_last_error()
    assert call(T=_lib.SURFACE_MAX_FRAMES + 1) == EINVAL and b'split the frames into slabs' in lib.empose_last_error()
    assert call(V=_lib.SURFACE_MAX_VERTICES + 1) == EINVAL and b'above the cap' in lib.empose_last_error()
    assert call(F=_lib.SURFACE_MAX_FACES + 1) == EINVAL and b'above the cap' in lib.empose_last_error()
    for bad, where in ((np.array([[0, 1, 2], [2, 1, 4]], np.int32), b'face 1'), (np.array([[0, -1, 2]], np.int32), b'face 0')):
        assert call(faces=bad) == EINVAL
        assert where in lib.empose_last_error() and b'outside [0, V = 4)' in lib.empose_last_error()
    assert lib.empose_surface_query_workspace_bytes(54030, 6890, 13776, 12) == 0  # combined inside the workgroup


def test_python_layer_refuses_cpu_tensors_and_bad_tables():
    from em_pose_amd.bodymodels.smpl import SMPLLayer
    v, pts = torch.zeros(2, 4, 3), torch.zeros(2, 5, 3)
    faces = np.array([[0, 1, 2]], np.int64)
    with pytest.raises(_lib.EmposeError, match='no CPU fallback'):
        SM.closest_point_on_mesh(v, faces, pts)
    smpl = SMPLLayer(H.small_model())
    with pytest.raises(_lib.EmposeError, match='no CPU fallback'):
        smpl.surface_distance(torch.zeros(2, 36), torch.zeros(2, 63), torch.zeros(1, 10))
    for bad in (np.zeros((0, 3), np.int64), np.zeros((2, 4), np.int64), np.zeros((2, 3), np.float32), np.zeros(3, np.int64)):
        with pytest.raises(ValueError, match='non-empty'):
            SM.Faces(bad, 'cpu')
    with pytest.raises(ValueError, match='non-negative'):
        SM.Faces(np.array([[0, 1, -2]]), 'cpu')
    with pytest.raises(ValueError, match='fit int32'):
        SM.Faces(np.array([[0, 1, 2 ** 31]]), 'cpu')
    table = SM.Faces(torch.tensor([[0, 1, 2], [2, 1, 3]]), 'cpu')
    assert len(table) == 2 and table.host.dtype == np.int32 and SM.Faces.of(table, 'cpu') is table
    assert smpl.surface_faces('cpu') is smpl.surface_faces('cpu')
    first = smpl.surface_faces('cpu')
    other = smpl.surface_faces('meta')                                             # a second device keeps the first's table
    assert smpl.surface_faces('cpu') is first and smpl.surface_faces('meta') is other
    smpl.tables_version += 1                                                       # new arrays: the stale tables go
    assert smpl.surface_faces('cpu') is not first and len(smpl.__dict__['_surface_faces']) == 1
    assert np.array_equal(smpl.surface_faces('cpu').host, np.asarray(H.small_model()['f'], np.int32))
    with pytest.raises(ValueError, match='frames of points'):
        SM._points_and_mask(torch.zeros(3, 5, 3), None, 2)
    with pytest.raises(ValueError, match='one value per point'):
        SM._points_and_mask(torch.zeros(2, 5, 3), torch.zeros(2, 4), 2)
