"""
Model-free sensor fitting without a GPU: the float64 restatement (tests/sensor_fit_ref.py) against finite differences
of its own objective, the descent it reaches on the very cases the GPU test uses, and the boundary of the C ABI -- struct
layout, workspace query and every refusal, all of which precede the first launch.
"""
import ctypes
import os
import re

import numpy as np
import pytest

from em_pose_amd import _lib
from tests import sensor_fit_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENOMEM = -1, -3


@pytest.fixture(scope='module')
def tab():
    return R.tables64()


# ---- the reference ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape_per_window', [True, False])
def test_reference_gradient_is_the_finite_difference_of_its_own_objective(tab, shape_per_window):
    """With zero moments, beta1 = beta2 = 0 and k = 0 a step stores the total gradient in m: data term (oracle) + pose
    prior + smoothness stencil, and for the shape the window sum + shape prior.  Central differences of J, h = 1e-6,
    on case A (ragged windows, a frame without data, a window of one live frame)."""
    case = R.make_case('A', 6)
    B, F, lens, idx, s = case['B'], case['F'], case['lens'], case['idx'], case['s']
    rng = np.random.default_rng(7)
    theta, beta = rng.normal(0, 0.2, (B, F, 66)), rng.normal(0, 0.5, (B, F, 10))
    if shape_per_window:
        beta = np.repeat(beta[:, :1], F, axis=1)
    prior = rng.normal(0, 0.2, (B, F, 66))
    hp = dict(R.HP, beta1=0.0, beta2=0.0, lambda_pose=0.3, lambda_shape=0.2, lambda_smooth=0.7)
    J = lambda th, be: R.objective_at(tab, th, be, case, hp, shape_per_window, prior)
    r = R.evaluate(tab, theta, beta, case['offset_r'], case['offset_t'], case['tgt'], idx, s)
    z = lambda w: np.zeros((B, F, w))
    o = R.step(theta, beta, r['g_theta'].reshape(B, F, 66), r['g_beta'].reshape(B, F, 10), r['pos'], r['ori'],
               case['tgt'], idx, s, lens, prior, z(66), z(66), z(10), z(10), 0, hp, shape_per_window)
    np.testing.assert_allclose(o['J'], J(theta, beta), rtol=1e-13)
    h = 1e-6
    picks = [(0, 0, 0), (0, 0, 7), (0, 4, 30), (0, 5, 12), (0, 5, 2), (0, 6, 65), (0, 7, 3), (1, 4, 9), (1, 3, 1),
             (2, 0, 20), (2, 0, 0)]        # window starts and ends, the frame without data (0, 5) and its neighbours
    for b, f, i in picks:
        d = np.zeros_like(theta)
        d[b, f, i] = h
        fd = (J(theta + d, beta)[b] - J(theta - d, beta)[b]) / (2 * h)
        assert abs(o['m_theta'][b, f, i] - fd) <= 1e-6 * max(1.0, abs(fd)), (b, f, i)
    assert (o['m_theta'][1, 5:] == 0).all() and (o['theta'][1, 5:] == theta[1, 5:]).all()     # padded frames
    for b, c in [(0, 0), (0, 9), (1, 4), (2, 3)]:
        d = np.zeros_like(beta)
        if shape_per_window:
            d[b, :, c] = h
            got = o['m_beta'][b, 0, c]
        else:
            d[b, 1 if b < 2 else 0, c] = h
            got = o['m_beta'][b, 1 if b < 2 else 0, c]
        fd = (J(theta, beta + d)[b] - J(theta, beta - d)[b]) / (2 * h)
        assert abs(got - fd) <= 1e-6 * max(1.0, abs(fd)), (b, c)


@pytest.mark.parametrize('n_markers', [12, 6])
@pytest.mark.parametrize('name', ['A', 'B'])
def test_reference_meets_the_descent_cap_on_the_cases_of_the_gpu_test(tab, name, n_markers):
    """Zero init, K = 30, lr 0.05: every window's returned J is at most 0.25 of its J at the init -- in float64 and in
    the float32 control.  Their trajectories are not compared: the early Adam steps are nearly lr sign(g), ill-conditioned
    element by element (after 30 steps the parameters of the two differ by up to 8e-2 rad, the ratios by up to 2.3 %)."""
    case = R.make_case(name, n_markers)
    ratios = {}
    for dtype in (np.float64, np.float32):
        rows = R.fit(tab, case, R.HP, 30, dtype=dtype)['objective']
        assert (rows[-1] <= rows[:-1].min(0)).all()                  # keep-best: the minimum over the iterates
        ratios[dtype] = rows[-1] / rows[0]
        assert (ratios[dtype] <= R.DESCENT_CAP).all(), (dtype, ratios[dtype])
    print('descent', name, n_markers, ratios[np.float64], ratios[np.float32])


@pytest.mark.parametrize('n_markers', [12, 6])
@pytest.mark.parametrize('name', ['A', 'B'])
def test_reference_smoothness_carries_the_frames_without_data(tab, name, n_markers):
    case = R.make_case(name, n_markers)
    frames = R.masked_with_live_neighbours(case)
    assert frames
    init = np.zeros((case['B'], case['F'], 66))
    free = R.fit(tab, case, dict(R.HP, lambda_smooth=0.0), 30, keep_best=False)['pose']
    tied = R.fit(tab, case, R.HP, 30, keep_best=False)['pose']
    for b, f in frames:
        assert (free[b, f] == 0).all(), (b, f)          # no data, no neighbours: it stays at its init exactly
        assert R.carried(tied, init, b, f), (b, f)


# ---- the boundary ----------------------------------------------------------------------------------------------------
def test_fit_io_layout_matches_the_header_field_order():
    text = open(os.path.join(ROOT, 'include', 'empose_hip.h')).read()
    end = re.search(r'\}\s*empose_fit_io;', text).start()
    start = text.rfind('typedef struct {', 0, end) + len('typedef struct {')
    body = re.sub(r'/\*.*?\*/', '', text[start:end], flags=re.S)
    names = []
    for decl in body.split(';'):
        for part in decl.strip().split(',') if decl.strip() else []:
            names.append(re.findall(r'([A-Za-z_][A-Za-z0-9_]*)\s*(?:\[[^\]]*\])*\s*$', part.strip())[0])
    assert names == [f[0] for f in _lib.FitIO._fields_]
    assert {'empose_sensor_fit', 'empose_sensor_fit_step', 'empose_sensor_fit_workspace_bytes'} <= set(_lib.SIGNATURES)


def _fakes():
    buf = np.zeros(64, np.float32)                       # never read: every call below is refused
    handle_buf = ctypes.create_string_buffer(1 << 16)    # a zeroed handle: only its sizes are read, all 0
    return buf, handle_buf, ctypes.c_void_p(buf.ctypes.data), ctypes.cast(handle_buf, ctypes.c_void_p)


def _io(p, **change):
    io = _lib.FitIO()
    io.B, io.F, io.K, io.ld_tgt = 2, 4, 3, 144
    for name, kind in _lib.FitIO._fields_:
        if kind is ctypes.c_void_p:
            setattr(io, name, p)
    for k, v in R.HP.items():
        setattr(io, k, v)
    io.shape_per_window, io.keep_best = 1, 1
    for k, v in change.items():
        setattr(io, k, v)
    return io


def test_workspace_query_is_zero_for_a_null_handle_and_bad_sizes():
    lib = _lib.lib()
    _, keep, _, handle = _fakes()
    assert lib.empose_sensor_fit_workspace_bytes(None, 2, 4) == 0
    for B, F in ((0, 4), (2, 0), (-1, 4), (2, -3)):
        assert lib.empose_sensor_fit_workspace_bytes(handle, B, F) == 0
    small, large = lib.empose_sensor_fit_workspace_bytes(handle, 2, 4), lib.empose_sensor_fit_workspace_bytes(handle, 2, 8)
    assert 0 < small < large


def test_every_refusal_precedes_the_first_launch_and_names_the_field():
    lib = _lib.lib()
    buf, keep, p, handle = _fakes()
    need = lib.empose_sensor_fit_workspace_bytes(handle, 2, 4)

    def fit(io, model=handle, ws=p, size=need):
        return lib.empose_sensor_fit(model, ctypes.byref(io) if io is not None else None, ws, ctypes.c_size_t(size), None)

    def refused(rc, code, word):
        assert rc == code, (word, rc)
        assert word.encode() in lib.empose_last_error(), (word, lib.empose_last_error())
    refused(fit(_io(p), model=None), EINVAL, 'model')
    refused(fit(None), EINVAL, 'io')
    refused(fit(_io(p), ws=None), EINVAL, 'workspace')
    refused(fit(_io(p), size=need - 1), ENOMEM, 'workspace')
    for name, word in (('tgt', 'tgt'), ('offset_r', 'offset_r'), ('offset_t', 'offset_t'), ('pose', 'pose'),
                       ('shape', 'shape'), ('joints', 'joints'), ('pos', 'pos'), ('ori', 'ori')):
        refused(fit(_io(p, **{name: None})), EINVAL, word)
    refused(fit(_io(p, B=0)), EINVAL, 'B and F')
    refused(fit(_io(p, F=-2)), EINVAL, 'B and F')
    refused(fit(_io(p, B=1 << 16, F=1 << 9)), EINVAL, 'B * F')
    refused(fit(_io(p, K=-1)), EINVAL, 'K')
    refused(fit(_io(p, ld_tgt=-1)), EINVAL, 'ld_tgt')
    for bad in (0.0, -0.05, float('nan'), float('inf')):
        refused(fit(_io(p, lr=bad)), EINVAL, 'lr')
        refused(fit(_io(p, lr_decay=bad)), EINVAL, 'lr_decay')
    for name in ('beta1', 'beta2'):
        for bad in (-0.1, 1.0, 1.5, float('nan')):
            refused(fit(_io(p, **{name: bad})), EINVAL, name)
    for name in ('eps', 'lambda_pose', 'lambda_shape', 'lambda_smooth'):
        for bad in (-1e-3, float('nan'), float('inf')):
            refused(fit(_io(p, **{name: bad})), EINVAL, name)

    def step(io=None, k=0, model=handle, **nulls):
        names = ('theta', 'beta', 'g_theta', 'g_beta', 'pos', 'ori', 's', 'm_theta', 'v_theta', 'm_beta', 'v_beta',
                 'theta_next', 'beta_next', 'energy', 'J', 'best_J', 'best_theta', 'best_beta')
        q = ctypes.c_void_p(buf.ctypes.data + 64)      # a second address: the next iterate is never the one read
        args = [None if n in nulls else (q if n in ('theta_next', 'beta_next') else p) for n in names]
        return lib.empose_sensor_fit_step(model, ctypes.byref(io if io is not None else _io(p)), k, *args, None)
    refused(step(model=None), EINVAL, 'model')
    refused(step(k=-1), EINVAL, 'k')
    refused(step(_io(p, lr=0.0)), EINVAL, 'lr')
    refused(step(_io(p, tgt=None)), EINVAL, 'tgt')
    for name in ('theta', 'beta', 'g_theta', 'g_beta', 'pos', 'ori', 's'):
        refused(step(**{name: 1}), EINVAL, 'null input')
    for name in ('m_theta', 'v_theta', 'm_beta', 'v_beta'):
        refused(step(**{name: 1}), EINVAL, 'moment')
    for name in ('theta_next', 'beta_next', 'J'):
        refused(step(**{name: 1}), EINVAL, 'null output')
    for name in ('best_J', 'best_theta', 'best_beta'):
        refused(step(**{name: 1}), EINVAL, 'go together')
    names_next = lib.empose_sensor_fit_step(handle, ctypes.byref(_io(p)), 0, *([p] * 18), None)    # theta_next == theta
    refused(names_next, EINVAL, 'theta_next')
