"""
The pose filters without a GPU (csrc/smooth.hip, csrc/api_smooth.hip, eval/smoothing.py):
  - every refusal of `empose_smooth_window` / `empose_smooth_one_euro` happens before any GPU work and names its argument;
  - `gaussian_taps`;
  - properties of the float64 restatement the GPU tests compare against (tests/smooth_ref.py): R = 0 is the identity, a
    constant-velocity rotation about a fixed axis and a linear ramp are reproduced, One-Euro with beta = 0 is the
    closed-form first-order recursion, chunked feeding through the state equals whole feeding;
  - the condition of the generator: at every test shape every aligned quaternion dot product the restatement forms is at
    least 0.1 (the definitions are discontinuous at 0, where no tolerance could hold).
"""
import ctypes

import numpy as np
import pytest
import torch

from em_pose_amd import _lib
from em_pose_amd.eval import smoothing as SM
from tests import resample_ref as Q
from tests import smooth_ref as SR

EINVAL = -1
S = _lib.SMOOTH_SEGMENT


def _buffers():
    a, b = np.zeros(64, np.float32), np.zeros(64, np.float32)   # never read: every call below is refused
    return a, b, ctypes.c_void_p(a.ctypes.data), ctypes.c_void_p(b.ctypes.data)


def _taps(values):
    arr = (ctypes.c_double * len(values))(*values)
    return arr


def test_the_constants_of_the_binding_are_the_headers():
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'empose_hip.h')).read()
    value = lambda name: int(re.search(r'#define\s+' + name + r'\s+(\d+)', text).group(1))
    assert value('EMPOSE_SMOOTH_SEGMENT') == _lib.SMOOTH_SEGMENT
    assert value('EMPOSE_SMOOTH_MAX_RADIUS') == _lib.SMOOTH_MAX_RADIUS == 32
    assert value('EMPOSE_SMOOTH_STATE') == _lib.SMOOTH_STATE == SR.STATE == 6


def test_window_refuses_bad_arguments_without_a_gpu():
    lib = _lib.lib()
    keep = _buffers()
    p_in, p_out = keep[2], keep[3]
    good = dict(N=2, F=4, J=1, C=1, inp=p_in, ld_in=4, valid=None, R=1, taps=_taps([1.0, 0.5]), out=p_out, ld_out=4)

    def call(**change):
        a = dict(good, **change)
        return lib.empose_smooth_window(a['N'], a['F'], a['J'], a['C'], a['inp'], a['ld_in'], a['valid'], a['R'], a['taps'],
                                        a['out'], a['ld_out'], None)
    inf, nan = float('inf'), float('nan')
    for change, word in (
            (dict(N=0), b'N'), (dict(N=-1), b'N'), (dict(F=0), b'F'), (dict(F=-3), b'F'),
            (dict(J=-1), b'J'), (dict(C=-1), b'C'), (dict(J=0, C=0), b'J + C'),
            (dict(ld_in=3), b'ld_in'), (dict(ld_out=3), b'ld_out'),
            (dict(inp=None), b'in'), (dict(out=None), b'out'), (dict(taps=None), b'taps_host'),
            (dict(out=p_in), b'out == in'),
            (dict(R=-1), b'R'), (dict(R=33, taps=_taps([1.0] * 34)), b'R'),
            (dict(taps=_taps([1.0, -0.5])), b'taps_host[1]'), (dict(taps=_taps([1.0, nan])), b'taps_host[1]'),
            (dict(taps=_taps([1.0, inf])), b'taps_host[1]'), (dict(taps=_taps([inf, 0.5])), b'taps_host[0]'),
            (dict(taps=_taps([0.0, 0.5])), b'taps_host[0]'), (dict(taps=_taps([-1.0, 0.5])), b'taps_host[0]'),
            (dict(N=65536, F=32768), b'N * F')):
        assert call(**change) == EINVAL, change
        assert word in lib.empose_last_error(), (change, lib.empose_last_error())


def test_one_euro_refuses_bad_arguments_without_a_gpu():
    lib = _lib.lib()
    keep = _buffers()
    p_in, p_out = keep[2], keep[3]
    good = dict(N=2, F=4, J=1, C=1, inp=p_in, ld_in=4, valid=None, fps=60.0, min_cutoff=1.0, beta=0.0, d_cutoff=1.0,
                out=p_out, ld_out=4)

    def call(**change):
        a = dict(good, **change)
        return lib.empose_smooth_one_euro(a['N'], a['F'], a['J'], a['C'], a['inp'], a['ld_in'], a['valid'], a['fps'],
                                          a['min_cutoff'], a['beta'], a['d_cutoff'], None, None, a['out'], a['ld_out'], None)
    inf, nan = float('inf'), float('nan')
    cases = [(dict(N=0), b'N'), (dict(F=0), b'F'), (dict(J=-1), b'J'), (dict(C=-2), b'C'), (dict(J=0, C=0), b'J + C'),
             (dict(ld_in=3), b'ld_in'), (dict(ld_out=3), b'ld_out'), (dict(inp=None), b'in'), (dict(out=None), b'out'),
             (dict(out=p_in), b'out == in'), (dict(N=65536, F=32768), b'N * F')]
    for name in ('fps', 'min_cutoff', 'd_cutoff'):
        cases += [({name: bad}, name.encode()) for bad in (0.0, -1.0, inf, nan)]
    cases += [(dict(beta=bad), b'beta') for bad in (-0.1, inf, nan)]
    for change, word in cases:
        assert call(**change) == EINVAL, change
        assert word in lib.empose_last_error(), (change, lib.empose_last_error())


def test_cpu_tensors_raise():
    rows = torch.zeros(1, 4, 4)
    with pytest.raises(_lib.EmposeError):
        SM.smooth_window(rows, None, [1.0, 0.5], 1, 1)
    with pytest.raises(_lib.EmposeError):
        SM.OneEuroFilter(1, 1)(rows)
    out = {'root_ori_hat': torch.zeros(1, 4, 3), 'pose_hat': torch.zeros(1, 4, 63), 'shape_hat': torch.zeros(1, 4, 10)}
    with pytest.raises(_lib.EmposeError):
        SM.smooth_model_output(out, None, None, SM.window_filter([1.0]))


def test_gaussian_taps_values_and_radius_rule():
    w = SM.gaussian_taps(2.0)
    assert w.dtype == np.float64 and w.shape == (7,)                        # ceil(3 sigma) = 6
    assert np.allclose(w, np.exp(-np.arange(7.0) ** 2 / 8.0), rtol=1e-15, atol=0) and w[0] == 1.0
    assert SM.gaussian_taps(0.5).shape == (3,) and SM.gaussian_taps(1.01).shape == (5,)
    assert SM.gaussian_taps(20.0).shape == (33,)                            # capped at 32
    assert SM.gaussian_taps(2.0, radius=0).shape == (1,) and SM.gaussian_taps(2.0, radius=32).shape == (33,)
    for bad in (0.0, -1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError):
            SM.gaussian_taps(bad)
    for bad in (-1, 33):
        with pytest.raises(ValueError):
            SM.gaussian_taps(2.0, radius=bad)


def test_one_euro_filter_checks_its_parameters():
    for kw in (dict(fps=0.0), dict(min_cutoff=-1.0), dict(d_cutoff=float('nan')), dict(beta=-0.5)):
        with pytest.raises(ValueError):
            SM.OneEuroFilter(22, 10, **kw)
    with pytest.raises(ValueError):
        SM.OneEuroFilter(0, 0)
    f = SM.OneEuroFilter(22, 10)
    assert (f.fps, f.min_cutoff, f.beta, f.d_cutoff) == (60.0, 1.0, 0.0, 1.0)    # the paper's defaults at the project's rate


# ---- the restatement ------------------------------------------------------------------------------------------------------
def test_restatement_radius_zero_is_the_identity():
    rows, valid = SR.case(3, S + 1, 22, 10)
    v = valid
    out = SR.window64(rows, valid, [1.0], 22, 10)
    assert np.array_equal(out[v][:, 66:], rows[v][:, 66:].astype(np.float64))          # exact on channels: x * 1 / 1
    out = SR.window64(rows, valid, [0.7], 22, 10)                                      # (w0 x) / w0: two roundings
    assert np.abs(out[v][:, 66:] - rows[v][:, 66:].astype(np.float64)).max() <= 2 * 2.0 ** -52 * 2.0
    ang = Q.geodesic(out[v][:, :66].reshape(-1, 22, 3), rows[v][:, :66].astype(np.float64).reshape(-1, 22, 3))
    assert float(ang.max()) <= 1e-12
    assert float(np.linalg.norm(out[v][:, :66].reshape(-1, 3), axis=-1).max()) <= np.pi + 1e-12
    assert float(np.linalg.norm(rows[v][:, :66].reshape(-1, 3), axis=-1).max()) > np.pi    # the inputs do go beyond pi


def constant_velocity(f, J, C):
    """Rotations about fixed axes at constant angular velocity through |r| = pi, and linear ramps: float64 rows."""
    rng = np.random.default_rng(5)
    rows = np.empty((1, f, 3 * J + C))
    t = np.arange(f)[:, None]
    for j in range(J):
        u = rng.normal(size=3)
        u /= np.linalg.norm(u)
        q0 = Q.quat_exp(rng.normal(size=3))
        q = Q.quat_mul(q0[None], Q.quat_exp((0.5 * (2.6 + 0.03 * (j + 1) * t)) * u[None]))
        rows[0, :, 3 * j:3 * j + 3] = Q.quat_to_rotvec(q)
    rows[0, :, 3 * J:] = rng.uniform(-1, 1, size=(1, C)) + rng.uniform(-0.01, 0.01, size=(1, C)) * t
    return rows


def test_restatement_reproduces_constant_velocity_and_ramps():
    f, J, C = 2 * S + 33, 3, 2
    rows = constant_velocity(f, J, C)
    valid = np.ones((1, f), dtype=bool)
    valid[0, 40] = valid[0, 41] = valid[0, 100] = False     # runs of 40, 58 and the rest
    for R in (1, 8, 32):
        out = SR.window64(rows, valid, SM.gaussian_taps(max(R, 2) / 2.0, radius=R), J, C)
        ang = Q.geodesic(out[valid][:, :9].reshape(-1, 3, 3), rows[valid][:, :9].reshape(-1, 3, 3))
        lin = np.abs(out[valid][:, 9:] - rows[valid][:, 9:])
        print('R {}: rotation {:.3e} rad, ramp {:.3e}'.format(R, float(ang.max()), float(lin.max())))
        assert float(ang.max()) <= 1e-12 and float(lin.max()) <= 1e-12


def test_restatement_one_euro_with_beta_zero_is_the_first_order_recursion():
    rng = np.random.default_rng(9)
    f, fps, fc = 50, 60.0, 1.5
    x = rng.normal(size=(1, f, 1))
    out, state = SR.one_euro64(x, None, 0, 1, fps, fc, 0.0, 1.0)
    a = 1.0 / (1.0 + fps / (2.0 * np.pi * fc))
    want = np.empty(f)
    want[0] = x[0, 0, 0]
    for t in range(1, f):
        want[t] = want[t - 1] + a * (x[0, t, 0] - want[t - 1])
    assert np.abs(out[0, :, 0] - want).max() <= 1e-15
    # closed form: x^[t] = (1 - a)^t x[0] + a sum_{s=1..t} (1 - a)^(t-s) x[s]
    t = f - 1
    closed = (1 - a) ** t * x[0, 0, 0] + a * sum((1 - a) ** (t - s) * x[0, s, 0] for s in range(1, t + 1))
    assert abs(out[0, t, 0] - closed) <= 1e-13
    assert state.shape == (1, 1, 6) and state[0, 0, 0] == out[0, -1, 0] and state[0, 0, 5] == 1.0
    # a rotation about a fixed axis is the same recursion on the angle
    u = np.array([0.6, 0.0, 0.8])
    ang = 0.3 * rng.normal(size=f)
    out, _ = SR.one_euro64((ang[:, None] * u[None])[None], None, 1, 0, fps, fc, 0.0, 1.0)
    want[0] = ang[0]
    for t in range(1, f):
        want[t] = want[t - 1] + a * (ang[t] - want[t - 1])
    assert np.abs(out[0] - want[:, None] * u[None]).max() <= 1e-13


def test_restatement_chunked_feeding_equals_whole_feeding_and_an_invalid_frame_resets():
    rows, valid = SR.case(3, S + 1, 22, 10)
    whole, st_whole = SR.one_euro64(rows, valid, 22, 10, 60.0, 1.0, 0.5, 1.0)
    state, parts = None, []
    for t0 in range(0, S + 1, 7):
        o, state = SR.one_euro64(rows[:, t0:t0 + 7], valid[:, t0:t0 + 7], 22, 10, 60.0, 1.0, 0.5, 1.0, state=state)
        parts.append(o)
    assert np.array_equal(np.concatenate(parts, axis=1), whole, equal_nan=True) and np.array_equal(state, st_whole)
    assert not st_whole[1].any()                                 # the dead row leaves no state
    # after an invalid frame the filter starts again: the rest equals filtering the rest alone
    i, t = [(i, t) for i, t in zip(*np.nonzero(~valid)) if i != 1 and 0 < t < S - 2][0]
    alone, _ = SR.one_euro64(rows[i:i + 1, t + 1:], valid[i:i + 1, t + 1:], 22, 10, 60.0, 1.0, 0.5, 1.0)
    assert np.array_equal(alone[0], whole[i, t + 1:], equal_nan=True)


def test_generator_keeps_every_aligned_dot_product_away_from_zero():
    """Over every test shape of tests/test_smoothing.py, at the largest radius (smaller radii form a subset of its
    products) and in the One-Euro recursion with both values of beta."""
    lowest = {'window': 1.0, 'one_euro': 1.0}
    beyond_pi = 0
    for n in (1, 3):
        for f in SR.frames(S):
            for J, C in SR.JC:
                if J == 0:
                    continue
                rows, valid = SR.case(n, f, J, C)
                stats = []
                SR.window64(rows, valid, np.ones(33), J, C, stats=stats)
                lowest['window'] = min([lowest['window']] + stats)
                for beta in (0.0, 0.5):
                    stats = []
                    SR.one_euro64(rows, valid, J, C, 60.0, 1.0, beta, 1.0, stats=stats)
                    lowest['one_euro'] = min([lowest['one_euro']] + stats)
                with np.errstate(invalid='ignore'):
                    beyond_pi += int((np.linalg.norm(rows[..., :3 * J].reshape(n, f, J, 3), axis=-1) > np.pi).sum())
    print('lowest aligned dot product: window (R = 32) {:.4f}, one-euro {:.4f}; {} inputs longer than pi'.format(
        lowest['window'], lowest['one_euro'], beyond_pi))
    assert lowest['window'] >= 0.1 and lowest['one_euro'] >= 0.1
    assert beyond_pi > 100
