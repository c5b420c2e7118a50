"""Resampling to 60 Hz on the device (csrc/resample.hip, em_pose_amd/data/resample.py): SQUAD for rotations against the
float64 restatement tests/resample_ref.py, the not-a-knot spline for positions against scipy.interpolate.CubicSpline,
the ragged batch, the dataset option, the transform and the converter.

Tolerances.  Rotations are compared as rotations, by the geodesic angle between float64 rotation matrices: 1e-6 rad.
Inputs are shared exactly, interior arithmetic is double on both sides, and the float32 rounding of the output vector is
at most 2^-24 * pi * sqrt(3) = 3.3e-7 rad; the tolerance is three times that.  Positions: 2.5e-7 * max(1, max|x|), four
times the float32 output rounding 2^-24 * |x|; the solve is in double.
"""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

from em_pose_amd import _lib
from em_pose_amd.data import resample as RS
from tests import helpers as H
from tests import resample_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROT_TOL = 1e-6
DEV = 'cuda:0'
AXIS = np.array([0.6, 0.0, 0.8])


def pos_tol(x):
    return 2.5e-7 * max(1.0, float(np.abs(x).max()))


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def geo(got, want):
    return float(RR.geodesic(got.detach().cpu().numpy().astype(np.float64), np.asarray(want, dtype=np.float64)).max())


@functools.lru_cache(maxsize=None)
def random_walk(F, J, seed=0):
    """Smooth rotation vectors: a random walk of sigma = 0.05 per frame from a random start, float32."""
    rng = np.random.default_rng(1000 * F + J + seed)
    r = rng.normal(0, 0.6, (1, J, 3)) + np.cumsum(rng.normal(0, 0.05, (F, J, 3)), axis=0)
    r = r.astype(np.float32)
    r.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def rotation_oracle(F, J, fps_in, fps_out, seed=0):
    return RR.resample_rotations(random_walk(F, J, seed), fps_in, fps_out)


@functools.lru_cache(maxsize=None)
def positions(F, C, seed=0):
    """Metre-scale trajectories with a 2 m offset, float32."""
    rng = np.random.default_rng(77 * F + C + seed)
    x = (2.0 + np.cumsum(rng.normal(0, 0.02, (F, C)), axis=0)).astype(np.float32)
    x.setflags(write=False)
    return x


def spline_oracle(x, fps_in, fps_out):
    from scipy.interpolate import CubicSpline
    n = x.shape[0]
    ts_in = np.arange(0, n / fps_in, 1 / fps_in)[:n]
    ts_out = np.arange(0, n / fps_in, 1 / fps_out)
    return CubicSpline(ts_in, np.asarray(x, dtype=np.float64), axis=0)(ts_out)


def write_amass_npz(path, n_frames, fps, seed):
    rng = np.random.default_rng(seed)
    poses = np.zeros((n_frames, 156))
    poses[:, :66] = (rng.normal(0, 0.3, (1, 66)) + np.cumsum(rng.normal(0, 0.02, (n_frames, 66)), axis=0))
    trans = 1.0 + np.cumsum(rng.normal(0, 0.01, (n_frames, 3)), axis=0)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez(path, poses=poses, betas=rng.normal(0, 0.5, 16), trans=trans, mocap_framerate=np.array(float(fps)),
             gender=np.array('female'))
    return poses[:, :66], trans


# ---- CPU ---------------------------------------------------------------------------------------------------------------
def test_output_length_is_np_arange_own_count():
    for fps_in in (60, 100, 120, 250):
        for fps_out in (30, 60):
            for f_in in range(2, 41):
                want = len(np.arange(0, f_in / fps_in, 1 / fps_out))
                assert RS.n_frames_out(f_in, fps_in, fps_out) == want
                table = RS.sequence_table([f_in, f_in], fps_in, fps_out)
                assert table['f_out'].tolist() == [want, want] and table['out_row'].tolist() == [0, want]
                assert table['in_row'].tolist() == [0, f_in]


def test_restatement_reproduces_its_knots():
    r = random_walk(9, 2)
    out = RR.resample_rotations(r, 120, 60)
    assert out.shape == (5, 2, 3)
    assert RR.geodesic(out, r[::2].astype(np.float64)).max() < 1e-12


def test_restatement_equals_the_closed_form_at_constant_angular_velocity():
    for f_in in (11, 7):
        r = (0.3 * np.arange(f_in))[:, None, None] * AXIS
        out = RR.resample_rotations(r, 100, 60)
        u = np.arange(out.shape[0]) / 60 * 100
        assert f_in != 7 or u[-1] > f_in - 1           # the last output frame lies past the last knot
        assert RR.geodesic(out, (0.3 * u)[:, None, None] * AXIS).max() < 1e-12


def test_converter_file_rules(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    try:
        import preprocess_amass as P
    finally:
        sys.path.pop(0)
    for rel in ('b/s2/walk_poses.npz', 'b/s1/run_poses.npz', 'a/x/jump_poses.npz', 'a/x/shape.npz', 'a/x/f_shape.npz',
                'a/x/MTR03_poses.npz', 'b/s1/WalkingStraightBackwards08_poses.npz', 'a/x/notes.txt', 'top_poses.npz'):
        path = tmp_path / rel
        path.parent.mkdir(parents=True, exist_ok=True)
        path.write_bytes(b'')
    assert P.amass_file_ids(str(tmp_path)) == ['top_poses.npz', 'a/x/jump_poses.npz', 'b/s1/run_poses.npz',
                                               'b/s2/walk_poses.npz']


def test_dataset_default_keeps_the_recorded_rate(tmp_path):
    from em_pose_amd.data.datasets import AMASSNpzDataset
    poses, trans = write_amass_npz(str(tmp_path / 'seq.npz'), 40, 120, 3)
    for data in (AMASSNpzDataset(str(tmp_path)), AMASSNpzDataset(str(tmp_path), resample_fps=None)):
        s = data[0]
        assert s.n_frames == 40 and s.fps == 120
        assert np.array_equal(s.poses, poses) and np.array_equal(s.trans, trans)


def test_refusals_come_before_any_gpu_work():
    lib = _lib.lib()
    buf = np.zeros(4096, np.float32)   # host memory: a launch would fault, a refusal never touches it
    p = ctypes.c_void_p(buf.ctypes.data)
    good = RS.sequence_table([5, 7], 100, 60)
    tp = lambda t: ctypes.c_void_p(t.ctypes.data)
    rot = lambda S=2, t=good, td=p, J=2, src=p, ld_in=6, rows=12, dst=p, ld_out=6, out=None: \
        lib.empose_resample_rotations(S, tp(t) if t is not None else None, td, J, src, ld_in, rows, dst, ld_out,
                                      int(good['f_out'].sum()) if out is None else out, None)
    pos = lambda S=2, t=good, td=p, J=2, src=p, ld_in=2, rows=12, dst=p, ld_out=2, out=None, ws=p, nb=4096: \
        lib.empose_resample_positions(S, tp(t) if t is not None else None, td, J, src, ld_in, rows, dst, ld_out,
                                      int(good['f_out'].sum()) if out is None else out, ws, nb, None)
    one = RS.sequence_table([5, 1], 100, 60)
    unpacked = good.copy()
    unpacked['out_row'][1] += 1
    slow = good.copy()
    slow['fps_in'][0] = 0.0
    for f in (rot, pos):
        assert f(t=None) == -1 and f(td=None) == -1 and f(src=None) == -1 and f(dst=None) == -1
        assert f(S=0) == -1 and f(J=0) == -1 and f(J=-1) == -1
        assert f(ld_in=1) == -1 and f(ld_out=1) == -1
        assert f(t=one) == -1
        assert b'at least two' in lib.empose_last_error()
        assert f(rows=11) == -1                       # the second sequence would read past the input
        assert f(t=unpacked) == -1 and f(out=3) == -1 and f(t=slow) == -1
    assert pos(ws=None) == -1 and pos(nb=8) == -1
    assert lib.empose_resample_positions_workspace_bytes(12, 2) >= 12 * 2 * 8
    assert lib.empose_resample_positions_workspace_bytes(0, 2) == 0


# ---- GPU, rotations ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_rotation_knots_are_reproduced():
    r = random_walk(9, 2)
    out = RS.resample_rotations(gpu(r), 120, 60)
    assert tuple(out.shape) == (5, 2, 3)
    err = geo(out, r[::2])
    print('knots: max geodesic error', err)
    assert err < ROT_TOL


@pytest.mark.gpu
@pytest.mark.parametrize('f_in', [11, 7])
def test_constant_rotation_about_a_fixed_axis_is_the_closed_form(f_in):
    r = ((0.3 * np.arange(f_in))[:, None, None] * AXIS).astype(np.float32)
    out = RS.resample_rotations(gpu(r), 100, 60)
    u = np.arange(out.shape[0]) / 60 * 100
    assert out.shape[0] == len(np.arange(0, f_in / 100, 1 / 60))
    assert f_in != 7 or u[-1] > f_in - 1               # 7 frames: the last output frame lies past the last knot
    err = geo(out, (0.3 * u)[:, None, None] * AXIS)
    print('constant rotation, F_in =', f_in, ': max geodesic error', err)
    assert err < ROT_TOL


@pytest.mark.gpu
@pytest.mark.parametrize('fps_in,f_in', [(100, 2), (100, 3), (100, 4), (100, 5), (100, 37), (250, 2), (250, 3), (250, 4),
                                         (250, 5), (250, 37), (30, 2), (30, 5)])
@pytest.mark.parametrize('J', [1, 22])
def test_smooth_random_rotations_against_the_restatement(fps_in, f_in, J):
    r = random_walk(f_in, J)
    want = rotation_oracle(f_in, J, fps_in, 60)
    ld_in, ld_out = 3 * J + 5, 3 * J + 2               # non-tight leading dimensions on both sides
    rows = torch.full((f_in, ld_in), float('nan'), device=DEV)
    rows[:, :3 * J] = gpu(r).reshape(f_in, 3 * J)
    out = RS.resample_rotation_rows(rows, J, RS.sequence_table([f_in], fps_in, 60), out_ld=ld_out)
    assert tuple(out.shape) == (want.shape[0], ld_out)
    err = geo(out[:, :3 * J].reshape(-1, J, 3), want)
    print('random walk', fps_in, f_in, J, ': max geodesic error', err)
    assert err < ROT_TOL
    tight = RS.resample_rotations(gpu(r), fps_in, 60)
    assert torch.equal(tight.reshape(-1, 3 * J), out[:, :3 * J])


@pytest.mark.gpu
def test_hemisphere_handling():
    # rotation vectors through |r| = pi: angles 0.8 pi -> 1.2 pi about one axis, 100 -> 60 Hz
    angle = np.linspace(0.8 * np.pi, 1.2 * np.pi, 11)
    r = (angle[:, None, None] * AXIS).astype(np.float32)
    out = RS.resample_rotations(gpu(r), 100, 60)
    u = np.arange(out.shape[0]) / 60 * 100
    e_ref, e_closed = geo(out, RR.resample_rotations(r, 100, 60)), geo(out, (0.8 * np.pi + 0.04 * np.pi * u)[:, None, None] * AXIS)
    print('through pi: against the restatement', e_ref, 'against the closed form', e_closed)
    assert e_ref < ROT_TOL and e_closed < ROT_TOL
    assert float(out.norm(dim=-1).max()) <= np.pi + 1e-6
    # every second vector replaced by its equivalent r (1 - 2 pi / |r|): the quaternion of the other sign
    base = random_walk(37, 22, seed=5).astype(np.float64)
    flipped = base.copy()
    norm = np.linalg.norm(base[1::2], axis=-1, keepdims=True)
    flipped[1::2] = base[1::2] * (1.0 - 2.0 * np.pi / norm)
    assert RR.geodesic(flipped, base).max() < 1e-12
    base32, flipped32 = base.astype(np.float32), flipped.astype(np.float32)
    got = RS.resample_rotations(gpu(flipped32), 100, 60)
    e_ref = geo(got, RR.resample_rotations(flipped32, 100, 60))
    # against the unflipped sequence: here the two float32 inputs are each other's equivalents only up to their own
    # rounding, so the strict statement is the one above; the same bar is held all the same
    e_same = geo(got, RS.resample_rotations(gpu(base32), 100, 60).cpu().numpy())
    print('alternating signs: against the restatement', e_ref, 'against the unflipped sequence', e_same)
    assert e_ref < ROT_TOL and e_same < ROT_TOL


@pytest.mark.gpu
def test_ragged_rotation_batch_is_bitwise_the_single_launches():
    seqs = [gpu(random_walk(f, 22)) for f in (2, 5, 37)]
    rates = [100, 250, 100]
    batch = RS.resample_rotations_batch(seqs, rates, 60)
    again = RS.resample_rotations_batch(seqs, rates, 60)
    for x, fps, b, b2 in zip(seqs, rates, batch, again):
        single = RS.resample_rotations(x, fps, 60)
        assert torch.equal(single.view(torch.int32), b.view(torch.int32))
        assert torch.equal(b.view(torch.int32), b2.view(torch.int32))


@pytest.mark.gpu
def test_rotation_refusals():
    x = gpu(random_walk(5, 2))
    with pytest.raises(_lib.EmposeError):
        RS.resample_rotations(x[:1], 100, 60)                  # one frame
    with pytest.raises(_lib.EmposeError):
        RS.resample_rotations(x.cpu(), 100, 60)                # no CPU fallback
    with pytest.raises(_lib.EmposeError):
        RS.resample_rotations(x[:, :0], 100, 60)               # J = 0
    with pytest.raises(_lib.EmposeError):
        RS.resample_positions(x.cpu().reshape(5, 6), 100, 60)
    with pytest.raises(_lib.EmposeError):
        RS.resample_positions(x.reshape(5, 6)[:1], 100, 60)
    same = RS.resample_rotations(x, 60, 60)                    # equal rates: the input itself
    assert same is x
    torch.cuda.synchronize()


# ---- GPU, positions ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('fps_in,f_in', [(100, 2), (100, 3), (100, 4), (100, 5), (100, 6), (100, 64), (250, 2), (250, 3),
                                         (250, 4), (250, 5), (250, 6), (250, 64), (120, 9)])
@pytest.mark.parametrize('C', [1, 3])
def test_positions_against_scipy(fps_in, f_in, C):
    x = positions(f_in, C)
    want = spline_oracle(x, fps_in, 60)
    out = RS.resample_positions(gpu(x), fps_in, 60)
    assert tuple(out.shape) == want.shape
    err = float(np.abs(out.cpu().numpy() - want).max())
    print('positions', fps_in, f_in, C, ': max error', err, 'tolerance', pos_tol(x))
    assert err <= pos_tol(x)
    if fps_in == 120:                                          # knots reproduced
        assert float(np.abs(out.cpu().numpy() - x[::2]).max()) <= pos_tol(x)
    # non-tight leading dimensions: the same bits
    rows = torch.full((f_in, C + 3), float('nan'), device=DEV)
    rows[:, :C] = gpu(x)
    wide = RS.resample_position_rows(rows, C, RS.sequence_table([f_in], fps_in, 60), out_ld=C + 1)
    assert torch.equal(wide[:, :C], out)


@pytest.mark.gpu
def test_a_cubic_polynomial_is_reproduced_with_its_extrapolated_last_frame():
    # a cubic in the knot index u = 100 t with dyadic coefficients: the float32 knots are exact, so nothing but the
    # arithmetic under test separates the result from the polynomial
    poly = lambda u: np.stack([2.0 + 0.25 * u - 0.125 * u ** 2 + 0.03125 * u ** 3, -1.0 + 0.0625 * u ** 3, 0.5 - 0.5 * u],
                              axis=-1)
    x = poly(np.arange(7.0)).astype(np.float32)
    assert np.array_equal(x.astype(np.float64), poly(np.arange(7.0)))
    out = RS.resample_positions(gpu(x), 100, 60).cpu().numpy()
    t_out = np.arange(0, 7 / 100, 1 / 60)
    assert out.shape[0] == len(t_out) == 5 and t_out[-1] * 100 > 6          # the last frame lies past the last knot
    err_scipy, err = np.abs(out - spline_oracle(x, 100, 60)).max(), np.abs(out - poly(t_out * 100)).max()
    print('cubic polynomial: max error against scipy', err_scipy, 'against the polynomial', err)
    assert err_scipy <= pos_tol(x) and err <= pos_tol(x)


@pytest.mark.gpu
def test_one_long_position_sequence_against_scipy():
    x = positions(5000, 3)
    out = RS.resample_positions(gpu(x), 120, 60).cpu().numpy()
    want = spline_oracle(x, 120, 60)
    assert out.shape == want.shape == (2500, 3)
    err = float(np.abs(out - want).max())
    print('5000 frames: max error', err, 'tolerance', pos_tol(x))
    assert err <= pos_tol(x)


@pytest.mark.gpu
def test_ragged_position_batch_is_bitwise_the_single_launches():
    seqs = [gpu(positions(f, 3)) for f in (2, 5, 37)]
    rates = [100, 250, 120]
    batch = RS.resample_positions_batch(seqs, rates, 60)
    again = RS.resample_positions_batch(seqs, rates, 60)
    for x, fps, b, b2 in zip(seqs, rates, batch, again):
        single = RS.resample_positions(x, fps, 60)
        assert torch.equal(single.view(torch.int32), b.view(torch.int32))
        assert torch.equal(b.view(torch.int32), b2.view(torch.int32))


# ---- GPU, end to end -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_dataset_resamples_once_to_60_hz(tmp_path):
    from em_pose_amd.data.datasets import AMASSNpzDataset
    poses, trans = write_amass_npz(str(tmp_path / 'seq.npz'), 40, 120, 3)
    data = AMASSNpzDataset(str(tmp_path), resample_fps=60)
    s = data[0]
    assert s.n_frames == 20 and s.fps == 60 and s.poses.shape == (20, 66) and s.trans.shape == (20, 3)
    p32 = poses.astype(np.float32)[::2].reshape(20, 22, 3)
    assert RR.geodesic(s.poses.reshape(20, 22, 3).astype(np.float64), p32.astype(np.float64)).max() < ROT_TOL
    assert np.abs(s.trans - trans.astype(np.float32)[::2]).max() <= pos_tol(trans)
    again = data[0]
    assert again is not s and again.poses is s.poses           # kept, not resampled again; the sample is a copy


@pytest.mark.gpu
def test_transform_recomputes_the_joints(tmp_path):
    from em_pose_amd.bodymodels.smpl import SMPLLayer
    from em_pose_amd.data.data import AMASSSample
    from em_pose_amd.data.transforms import ResampleSequence
    smpl = SMPLLayer(H.small_model()).to(DEV)
    poses, trans = write_amass_npz(str(tmp_path / 'seq.npz'), 12, 100, 4)
    betas = np.linspace(-0.5, 0.5, 10)
    sample = AMASSSample('x', poses, betas, trans, 100.0, joints=np.zeros((12, 66)))
    with pytest.raises(ValueError):
        ResampleSequence()(sample)                             # joints are recomputed: that needs the body model
    out = ResampleSequence(smpl_model=smpl)(sample)
    n = len(np.arange(0, 12 / 100, 1 / 60))
    assert out.fps == 60.0 and out.n_frames == n and out.joints.shape == (n, 66)
    p = gpu(out.poses)
    want = smpl.fk(p[:, 3:], gpu(betas).reshape(1, -1), poses_root=p[:, :3], trans=gpu(out.trans))[1][:, :22]
    assert np.abs(out.joints - want.reshape(n, 66).cpu().numpy()).max() <= 1e-5


@pytest.mark.gpu
def test_converter_writes_records_the_lmdb_dataset_reads(tmp_path):
    from em_pose_amd.bodymodels.smpl import SMPLLayer
    from em_pose_amd.data.datasets import LMDBDataset
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    try:
        import preprocess_amass as P
    finally:
        sys.path.pop(0)
    tree = tmp_path / 'amass'
    src = {'a/one_poses.npz': (14, 120), 'a/two_poses.npz': (9, 60), 'b/three_poses.npz': (11, 100)}
    raw = {rel: write_amass_npz(str(tree / rel), f, fps, 10 + k) for k, (rel, (f, fps)) in enumerate(src.items())}
    write_amass_npz(str(tree / 'a' / 'shape.npz'), 4, 120, 9)
    smpl = SMPLLayer(H.small_model()).to(DEV)
    records = P.convert_amass(str(tree), smpl, batch_size=2, device=DEV)
    P.save_records(str(tmp_path / 'out.npz'), records)
    data = LMDBDataset(P.load_records(str(tmp_path / 'out.npz')))
    assert len(data) == 3
    for k, rel in enumerate(sorted(src)):
        f, fps = src[rel]
        s = data[k]
        n = len(np.arange(0, f / fps, 1 / 60)) if fps != 60 else f
        assert s.id == rel and s.gender == 'female' and s.fps == 60.0
        assert s.n_frames == n and s.poses.shape == (n, 66) and s.trans.shape == (n, 3) and s.joints.shape == (n, 66)
        if fps == 60:                                          # passes through untouched
            assert np.array_equal(s.poses, raw[rel][0].astype(np.float32))
            assert np.array_equal(s.trans, raw[rel][1].astype(np.float32))
        p = gpu(s.poses)
        want = smpl.fk(p[:, 3:], gpu(s.shape).reshape(1, -1), poses_root=p[:, :3], trans=gpu(s.trans))[1][:, :22]
        # the joints-only and the full-mesh entry point run the same float32 chain; 1e-5 m is the float32 rounding of a
        # metre-scale joint (6e-8) through a chain of up to ten transforms, with a factor of ten to spare
        assert np.abs(s.joints - want.reshape(n, 66).cpu().numpy()).max() <= 1e-5
