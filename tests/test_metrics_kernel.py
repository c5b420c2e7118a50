"""The device metrics kernel (`empose_metrics_rows`, csrc/metrics.hip) against the float64 reference of
tests/fuzz/fuzz_metrics.py: launch shapes around the 64-thread block, the output bound, argument checks, and a fixed-seed
slice of the randomized families (degenerate frames: near-planar / planar / collinear point sets, repeated singular
values, mirror images, large offsets, angles at 0 / 180 degrees and below the exp-map clamp, no poses, coincident joints).
The reference itself is tested on the CPU against the host metrics (eval/metrics.py) and against known answers."""
import ctypes

import numpy as np
import pytest

from em_pose_amd.eval.metrics import geodesic_degrees, local_to_global_rotations, procrustes_align, rotvec_to_matrix
from tests.fuzz import fuzz_metrics as FM

EMPOSE_EINVAL = -1


def _pose_pair(rng, T, scale=0.4):
    pg = rng.normal(0, scale, size=(T, 63))
    return pg, pg + rng.normal(0, 0.2, size=pg.shape)


# ---- the float64 reference (CPU) -------------------------------------------------------------------------------------
def test_reference_angles_match_host_metrics_above_the_clamp():
    """Above 1e-2 rad the clamped Rodrigues map is the exact one: the reference's angle columns equal the host metrics'
    global orientations (eval/metrics.py: rotvec_to_matrix, local_to_global_rotations, geodesic_degrees)."""
    rng = np.random.default_rng(11)
    pg, ph = _pose_pair(rng, 64)
    pg = pg.reshape(64, 21, 3)
    n = np.linalg.norm(pg, axis=-1, keepdims=True)
    pg = np.where(n < 0.02, pg * (0.02 / np.maximum(n, 1e-30)), pg).reshape(64, 63)   # every rotation above the clamp
    ph = ph.reshape(64, 21, 3)
    n = np.linalg.norm(ph, axis=-1, keepdims=True)
    ph = np.where(n < 0.02, ph * (0.02 / np.maximum(n, 1e-30)), ph).reshape(64, 63)
    X = FM.body_cloud(rng, 64)
    rows = FM.reference_rows(X, X + 0.01, pg, ph)
    zeros = np.zeros((64, 3))
    g = local_to_global_rotations(np.concatenate([zeros, pg], -1), FM.PARENTS)[:, 1:]
    gh = local_to_global_rotations(np.concatenate([zeros, ph], -1), FM.PARENTS)[:, 1:]
    np.testing.assert_allclose(rows[:, 44:], geodesic_degrees(g, gh), rtol=0, atol=1e-9)
    np.testing.assert_allclose(FM.exp_map_clamped(pg.reshape(-1, 3)), rotvec_to_matrix(pg.reshape(-1, 3)), atol=1e-15)
    # angles of a single turn: |r| in degrees, also at 180
    r = np.zeros((3, 63))
    r[0, 0:3] = [0.3, 0.0, 0.0]
    r[1, 0:3] = [0.0, 0.0, np.pi]
    r[2, 0:3] = [0.0, 0.05, 0.0]
    ang = FM.reference_rows(X[:3], X[:3], r, np.zeros_like(r))[:, 44]
    np.testing.assert_allclose(ang, np.degrees([0.3, np.pi, 0.05]), atol=1e-12)


def test_reference_procrustes_recovers_a_known_similarity_and_matches_host_alignment():
    """Y = (X R^T - t) / s exactly: every PA distance is zero (rounding only), while the Euclidean ones are not; a mirror
    image is NOT aligned (rotations only); on noisy frames the distances equal the host procrustes_align's."""
    rng = np.random.default_rng(12)
    T = 32
    X = FM.body_cloud(rng, T)
    Y = np.empty_like(X)
    for t in range(T):
        Y[t] = (X[t] @ FM.random_rotation(rng).T + rng.normal(0, 2.0, size=3)) / rng.uniform(0.3, 3.0)
    rows = FM.reference_rows(X, Y)
    assert rows[:, 22:44].max() < 1e-14 and rows[:, :22].min() > 1e-3
    mirror = FM.reference_rows(X, X * np.array([1.0, 1.0, -1.0]))
    assert mirror[:, 22:44].max() > 1e-2
    Yn = Y + rng.normal(0, 0.05, size=Y.shape)
    np.testing.assert_allclose(FM.reference_rows(X, Yn)[:, 22:44],
                               np.linalg.norm(X - procrustes_align(X, Yn), axis=-1), rtol=0, atol=1e-14)
    # a proper rotation: the aligned prediction of a noiseless similarity is X itself, whichever way Y was turned
    assert np.abs(procrustes_align(X, Y) - X).max() < 1e-13


def test_reference_nan_exactly_where_a_point_set_has_no_spread():
    rng = np.random.default_rng(13)
    for fam in FM.NAN_PA:
        X, Y, pg, ph = FM.make_case(fam, rng, 5)
        rows = FM.reference_rows(X, Y, pg, ph)
        assert np.isnan(rows[:, 22:44]).all() and np.isfinite(rows[:, :22]).all() and np.isfinite(rows[:, 44:]).all()
    X, Y, _, _ = FM.make_case('no_poses', rng, 5)
    assert (FM.reference_rows(X, Y)[:, 44:] == 0).all()


def test_clamp_family_tells_the_clamped_map_from_the_exact_one():
    """The 'angle_below_clamp' family is built so that a kernel WITHOUT the 1e-2 rad clamp fails it: on its co-axial
    chain frames the exact map's angles differ from the clamped ones by more than the angle bound."""
    rng = np.random.default_rng(14)
    X, Y, pg, ph = FM.make_case('angle_below_clamp', rng, 8)
    want = FM.reference_rows(X, Y, pg, ph)[:, 44:]
    exact = lambda p: FM.global_orientations(p, rodrigues=rotvec_to_matrix)[:, 1:]
    c = np.clip(((exact(pg) * exact(ph)).sum((-1, -2)) - 1.0) * 0.5, -1.0, 1.0)
    assert np.abs(np.degrees(np.arccos(c)) - want).max() > 3 * FM.TOL['angle']


def test_engine_reports_whether_compute_queued_device_rows():
    """MetricsEngine.queues_device_rows is the condition of compute's device path (what the batched driver reads to
    decide whether it places device rows), and compute returns what it did: on CPU tensors the host path, False."""
    import torch
    from em_pose_amd.eval.metrics import MetricsEngine

    class JointsOnly(object):
        def fk_joints(self, *a, **k):
            raise AssertionError('not on the CPU')

    assert MetricsEngine(JointsOnly()).queues_device_rows('cuda:0')
    assert not MetricsEngine(JointsOnly()).queues_device_rows('cpu')
    assert not MetricsEngine(None).queues_device_rows('cuda:0')
    rng = np.random.default_rng(16)
    pose = torch.from_numpy(rng.normal(0, 0.3, size=(2, 5, 63)))
    me = MetricsEngine(None)
    assert me.compute(pose, torch.zeros(2, 10), pose + 0.1, seq_lengths=torch.tensor([5, 3])) is False
    assert me.state()['angle'].shape == (8, 21) and not me.take_device_rows()


def test_every_family_generates_float32_frames_of_the_right_shape():
    rng = np.random.default_rng(15)
    for fam in FM.FAMILIES:
        X, Y, pg, ph = FM.make_case(fam, rng, 3)
        assert X.dtype == np.float32 and X.shape == (3, 22, 3) and Y.shape == (3, 22, 3), fam
        assert (pg is None) == (ph is None) == (fam == 'no_poses'), fam
        if pg is not None:
            assert pg.dtype == np.float32 and pg.shape == (3, 63), fam


# ---- the kernel (GPU) ------------------------------------------------------------------------------------------------
def _assert_rows(got, want, family='well_conditioned'):
    err = FM.case_errors(got, want, family)
    assert all(err[k] <= FM.TOL[k] for k in err), err


@pytest.mark.gpu
@pytest.mark.parametrize('T', [1, 63, 64, 65, 1000, 2 ** 17 + 3])
def test_launch_shapes_and_the_row_after_the_last_frame(T):
    """One thread per frame in blocks of 64: the frame counts around a block and a grid of 2049 blocks; a row of
    sentinels after the T x 65 output must come back untouched (bit for bit)."""
    rng = np.random.default_rng(T)
    X = FM.body_cloud(rng, T).astype(np.float32)
    Y = (X + rng.normal(0, 0.05, size=X.shape)).astype(np.float32)
    pg, ph = [p.astype(np.float32) for p in _pose_pair(rng, T)]
    sentinel = -1234.5
    got = FM.device_rows(X, Y, pg, ph, extra_rows=1, fill=sentinel)
    assert (got[T] == sentinel).all()
    _assert_rows(got[:T], FM.reference_rows(X, Y, pg, ph))


@pytest.mark.gpu
def test_argument_checks_refuse_and_launch_nothing():
    """EINVAL for T <= 0, exactly one pose pointer NULL, parents that are not topologically ordered (a parent at or
    after its child); nothing is written then."""
    import torch
    from em_pose_amd import _lib
    lib = _lib.lib()
    rng = np.random.default_rng(3)
    dev = torch.device('cuda:0')
    X = torch.from_numpy(FM.body_cloud(rng, 4).astype(np.float32)).to(dev)
    P = torch.from_numpy(rng.normal(0, 0.3, size=(4, 63)).astype(np.float32)).to(dev)
    rows = torch.full((4, 65), 7.0, dtype=torch.float64, device=dev)
    par = lambda p: (ctypes.c_int * 22)(*p)
    good = list(FM.PARENTS)
    call = lambda T, g, h, p: lib.empose_metrics_rows(T, _lib.dptr(X), _lib.dptr(X), g, h, par(p), _lib.dptr(rows),
                                                      _lib.current_stream())
    with torch.cuda.device(dev):
        assert call(4, _lib.dptr(P), _lib.dptr(P), good) == 0
        torch.cuda.synchronize()
        assert float(rows[:, 44:].abs().max()) <= FM.TOL['angle']    # same poses: zero angles (acos near 1: ~1e-6 deg)
        rows.fill_(7.0)
        bad_parents = [good[:5] + [5] + good[6:], good[:5] + [9] + good[6:], good[:21] + [21]]
        for args in [(0, _lib.dptr(P), _lib.dptr(P), good), (-3, _lib.dptr(P), _lib.dptr(P), good),
                     (4, _lib.dptr(P), None, good), (4, None, _lib.dptr(P), good)] + \
                    [(4, _lib.dptr(P), _lib.dptr(P), p) for p in bad_parents]:
            assert call(*args) == EMPOSE_EINVAL, args
        torch.cuda.synchronize()
    assert (rows == 7.0).all()


@pytest.mark.gpu
def test_fuzz_slice_every_family_within_absolute_bounds(capsys):
    """340 cases of tests/fuzz/fuzz_metrics.py (20 per family, 1..96 frames each) against the float64 reference at the
    absolute bounds of FM.TOL: 1e-12 m Euclidean, 1e-8 m after Procrustes, 1e-5 degrees; NaN in exactly the Procrustes
    columns of frames with coincident joints.  Before the one-sided Jacobi SVD (an eigen-decomposition of A^T A and
    u3 = A v3 / |A v3|) the near-planar and planar ground-truth families failed here."""
    r = FM.run(seed=7301, n_cases=20 * len(FM.FAMILIES), check=False)
    with capsys.disabled():
        print('\n[metrics fuzz slice] ' + FM.report(r), flush=True)
    assert r['n'] == 20 * len(FM.FAMILIES)
    assert not r['failures'], r['failures'][:5]
