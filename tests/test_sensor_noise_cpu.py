"""Sensor-noise augmentation without a GPU: the float64 restatement of the write step against the fixture recorded from
the reference, the host draws against fresh generators driven in the reference's order, the selection table of the
factory, the opt-in switch of the preprocessing factory, and the refusals of the C entry point (all of them come before
any GPU work, so they run on host buffers that a launch would fault on)."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from em_pose_amd import _lib
from em_pose_amd.data import noise_functions as NF
from em_pose_amd.data.transforms import get_end_to_end_preprocess_fn
from em_pose_amd.helpers.configuration import CONSTANTS as CONST
from em_pose_amd.helpers.configuration import lgd_config
from tests import sensor_noise_ref as SN

EINVAL = -1


@pytest.fixture(scope='module')
def fx():
    return SN.load_fixture()


@pytest.mark.parametrize('name', SN.CASES)
def test_restatement_reproduces_the_reference(fx, name):
    assert tuple(fx['thigh_idx']) == SN.THIGH == (CONST.THIGH_UPPER_IDX, CONST.THIGH_LOWER_IDX)
    for call in fx['cases'][name]:
        got = SN.restate(fx['pos'], fx['ori'], fx['normal'], **SN.plan_of(call))
        err = SN.check_against_reference(fx, call, got)
        print('{}: displaced positions within {:.3e} of the reference'.format(name, err))
        if 'u_r' in call:   # the displacement is there at all
            assert np.abs(got[0] - fx['pos']).max() > 1e-3


def test_spherical_draws_follow_the_reference_order():
    n, f, m, k = 5, 16, 12, 3
    fn = NF.SphericalMarkerNoise(0.5, 0.3, k)
    g = torch.Generator().manual_seed(98052)

    def expect():
        ids = torch.randperm(m, generator=g)[:k]
        wl = int(0.3 * f)
        sf = torch.randint(0, f - wl + 1, (n,), generator=g)
        u_r = torch.rand(n, wl, k)                                  # the global generator
        theta = torch.rand((n, wl, k), generator=g) * np.pi * 2
        phi = torch.rand((n, wl, k), generator=g) * np.pi
        return wl, {'sensor': ids.to(torch.int32), 'start': sf.to(torch.int32), 'u_r': u_r, 'theta': theta, 'phi': phi}

    for call in range(2):   # the second call goes on where the first left the generators
        torch.manual_seed(1234 + call)
        wl, want = expect()
        torch.manual_seed(1234 + call)
        got_wl, plan = fn.plan(n, f, m)
        assert got_wl == wl == 4
        for key, w in want.items():
            assert plan.host[key].dtype == w.dtype and torch.equal(plan.host[key], w), (call, key)
    assert NF.SphericalMarkerNoise(2.0, 3.0, 1).max_r == 1.0 and NF.SphericalMarkerNoise(2.0, 3.0, 1).ws == 1.0
    with pytest.raises(ValueError, match='Temporal length'):
        NF.SphericalMarkerNoise(0.5, 0.0, 1)
    # the reference's early returns: no strength, no synthetic sensors
    batch = types.SimpleNamespace(marker_pos_synth=None, marker_pos_noisy=None)
    assert NF.SphericalMarkerNoise(0.0, 0.0, 1)(batch) is batch and NF.SphericalMarkerNoise(0.5, 0.5, 1)(batch) is batch
    assert batch.marker_pos_noisy is None


@pytest.mark.parametrize('n_in', [12, 6])
def test_suppression_draws_follow_the_reference_order(n_in):
    n, f, k = 5, 16, 2
    ids = torch.tensor(CONST.S_CONFIG_6 if n_in == 6 else list(range(12)))
    fn = NF.MarkerSuppressionNoise(0.3, k, 0.0, n_in)
    g = torch.Generator().manual_seed(8004)

    def expect():
        m_ids = torch.randint(0, len(ids), (n, k), generator=g)
        wl = int(0.3 * f)
        sf = torch.randint(0, f - wl + 1, (n,), generator=g)
        return wl, ids[m_ids].to(torch.int32), sf.to(torch.int32)

    def same(want):
        wl, plan = fn.plan(n, f)
        return wl == want[0] and torch.equal(plan.host['sensor'], want[1]) and torch.equal(plan.host['start'], want[2])

    first, second = expect(), expect()
    assert same(first) and same(second)
    assert not (torch.equal(first[1], second[1]) and torch.equal(first[2], second[2]))
    fn.reset_rng()
    assert same(first)
    # the call's reset_rng=True reseeds before it draws (it does so before it looks at the batch)
    cpu = types.SimpleNamespace(marker_pos_synth=torch.zeros(n, f, 36), marker_ori_synth=torch.zeros(n, f, 108),
                                marker_normal_synth=torch.zeros(n, f, 36))
    with pytest.raises(_lib.EmposeError, match='HIP path'):
        fn(cpu, reset_rng=True)
    assert same(first)
    with pytest.raises(AssertionError):
        NF.MarkerSuppressionNoise(0.3, 1, 0.0, 7)


def test_cpu_batches_are_refused():
    cpu = types.SimpleNamespace(marker_pos_synth=torch.zeros(2, 4, 36), marker_ori_synth=torch.zeros(2, 4, 108),
                                marker_normal_synth=torch.zeros(2, 4, 36))
    for fn in (NF.SphericalMarkerNoise(0.5, 0.5, 1), NF.MarkerSuppressionNoise(0.5, 1, 0.0)):
        with pytest.raises(_lib.EmposeError, match='no CPU fallback'):
            fn(cpu)


def test_get_noise_fn_selection_table():
    cfg = lambda n_markers=12, **kw: lgd_config(n_markers, True, 2, **kw)
    sph = cfg(spherical_noise_length=0.2, spherical_noise_strength=0.5, noise_num_markers=2)
    sup = cfg(suppression_noise_length=0.1, suppression_noise_value=-1.0, noise_num_markers=3, n_markers=6)
    fn = NF.get_noise_fn(sph, True)
    assert isinstance(fn, NF.SphericalMarkerNoise) and (fn.max_r, fn.ws, fn.num_markers) == (0.5, 0.2, 2)
    fn = NF.get_noise_fn(sup, True)
    assert isinstance(fn, NF.MarkerSuppressionNoise) and (fn.ws, fn.num_markers, fn.mask_value) == (0.1, 3, -1.0)
    assert fn.marker_ids.tolist() == CONST.S_CONFIG_6
    assert NF.get_noise_fn(cfg(), True) is NF.no_noise
    # without randomisation: nothing, except suppression for validation
    for c in (sph, sup, cfg()):
        assert NF.get_noise_fn(c, False) is NF.no_noise
    assert isinstance(NF.get_noise_fn(sup, False, is_valid=True), NF.MarkerSuppressionNoise)
    assert NF.get_noise_fn(sph, False, is_valid=True) is NF.no_noise
    assert NF.get_noise_fn(cfg(), False, is_valid=True) is NF.no_noise
    batch = object()
    assert NF.no_noise(batch, reset_rng=True) is batch
    with pytest.raises(AssertionError, match='one noise type'):
        NF.get_noise_fn(cfg(spherical_noise_length=0.2, spherical_noise_strength=0.5, suppression_noise_length=0.1), True)


def test_preprocess_factory_switch():
    cfg = lgd_config(12, True, 2, suppression_noise_length=0.1)
    with pytest.raises(NotImplementedError, match='device_noise=True'):
        get_end_to_end_preprocess_fn(cfg, None, [], randomize_if_configured=True)
    with pytest.raises(NotImplementedError):
        get_end_to_end_preprocess_fn(lgd_config(12, True, 2, spherical_noise_length=0.1, spherical_noise_strength=0.1),
                                     None, [], randomize_if_configured=True)
    with pytest.raises(AssertionError, match='one noise type'):   # the reference's assertion reaches the factory
        get_end_to_end_preprocess_fn(lgd_config(12, True, 2, spherical_noise_length=0.1, suppression_noise_length=0.1),
                                     None, [], randomize_if_configured=True, device_noise=True)
    offsets = {'means': np.zeros((12, 3), np.float32), 'covs': np.tile(np.eye(3, dtype=np.float32) * 1e-4, (12, 1, 1)),
               'r': np.tile(np.eye(3, dtype=np.float32), (12, 1, 1)),
               'vertex_ids': np.asarray(CONST.VERTEX_IDS)}
    make = lambda c, randomize: get_end_to_end_preprocess_fn(c, None, [offsets], randomize_if_configured=randomize,
                                                             device_noise=True)
    assert make(lgd_config(12, True, 2), True).noise_fn is None       # all lengths 0: the plain pipeline
    assert make(cfg, False).noise_fn is None                          # no randomisation: the plain pipeline
    assert isinstance(make(cfg, True).noise_fn, NF.MarkerSuppressionNoise)
    assert get_end_to_end_preprocess_fn(lgd_config(12, True, 2), None, [offsets], True).noise_fn is None


def test_abi_refusals_come_before_any_gpu_work():
    lib = _lib.lib()
    buf = np.zeros(4096, np.float32)   # host memory: a launch would fault, a refusal never touches it
    other = np.zeros(4096, np.float32)
    p, q = C.c_void_p(buf.ctypes.data), C.c_void_p(other.ctypes.data)
    start = np.asarray([0, 1, 2], np.int32)      # N = 3, F = 4, window_len = 2: starts in [0, 2]
    ids = np.asarray([[0, 1], [2, 3], [11, 11]], np.int32)   # K = 2, M = 12
    sp, ip = C.c_void_p(start.ctypes.data), C.c_void_p(ids.ctypes.data)

    def call(mode=SN.SUPPRESS, n=3, f=4, m=12, k=2, wl=2, sh=sp, ih=ip, sd=p, idv=p, u=p, th=p, ph=p, max_r=1.0, a=5, b=6,
             mask=0.0, pos=p, ori=p, nor=p, po=q, oo=q, no=q):
        return SN.call_abi(mode, n, f, m, k, wl, sh, ih, sd, idv, u, th, ph, max_r, a, b, mask, pos, ori, nor, po, oo, no)

    err = lambda: lib.empose_last_error()
    for mode in (SN.SPHERICAL, SN.SUPPRESS):
        for name in ('sh', 'ih', 'sd', 'idv', 'pos', 'po'):          # NULL required pointers
            assert call(mode=mode, **{name: None}) == EINVAL, name
        for name in ('n', 'f', 'm'):                                 # sizes
            assert call(mode=mode, **{name: 0}) == EINVAL and call(mode=mode, **{name: -3}) == EINVAL, name
        assert call(mode=mode, k=0) == EINVAL and call(mode=mode, k=13) == EINVAL and call(mode=mode, k=-1) == EINVAL
        assert b'affected sensors' in err()
        assert call(mode=mode, wl=-1) == EINVAL and call(mode=mode, wl=5) == EINVAL
        assert b'window_len' in err()
        assert call(mode=mode, po=p) == EINVAL                        # an output that is its input
        assert b'must not be' in err()
        # the host copy of the plan
        for bad in ([0, 3, 2], [-1, 0, 0]):
            s = np.asarray(bad, np.int32)
            assert call(mode=mode, sh=C.c_void_p(s.ctypes.data)) == EINVAL and b'start' in err()
        for bad in (12, -1):
            i = ids.copy()
            i[0, 1] = bad      # (spherical reads the first K entries)
            assert call(mode=mode, ih=C.c_void_p(i.ctypes.data)) == EINVAL and b'sensor id' in err()
    assert call(mode=2) == EINVAL and call(mode=-1) == EINVAL and b'mode' in err()
    # spherical: the thigh sensors and the draws
    for name in ('a', 'b'):
        assert call(mode=SN.SPHERICAL, **{name: 12}) == EINVAL and call(mode=SN.SPHERICAL, **{name: -1}) == EINVAL
        assert b'thigh' in err()
    for name in ('u', 'th', 'ph'):
        assert call(mode=SN.SPHERICAL, **{name: None}) == EINVAL and b'draws' in err()
    # suppression: all three buffers, none of them in place
    for name in ('ori', 'nor', 'oo', 'no'):
        assert call(**{name: None}) == EINVAL and b'orientation and normal' in err()
    assert call(oo=p) == EINVAL and call(no=p) == EINVAL
    # sizes one launch cannot cover are refused before the plan is read (these N entries do not exist)
    assert call(n=1 << 20, f=1 << 15) == EINVAL and b'too large' in err()
