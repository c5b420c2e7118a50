"""The sensor-noise kernel on the GPU: against what the unmodified reference wrote for recorded draws
(tests/golden/sensor_noise.npz), against the float64 restatement at the shapes where it can go wrong, repeated launches,
and the preprocessing factory end to end with one training step.

Bounds.  Suppression and every element a plan does not touch: bit-identical.  Displaced positions: 1e-6 absolute -- the
displacement is at most thigh / 2 < 0.3 m, device sinf / cosf are a few units in the last place and the build has no
fast-math, so the displacement is off by < 1e-7; rounding the sum at |x| < 4 adds <= 2.4e-7."""
import numpy as np
import pytest
import torch

from em_pose_amd.bodymodels.smpl import SMPLLayer
from em_pose_amd.data import noise_functions as NF
from em_pose_amd.helpers.configuration import CONSTANTS as CONST
from em_pose_amd.helpers.configuration import lgd_config
from tests import helpers as H
from tests import sensor_noise_ref as SN

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BOUND = 1e-6


@pytest.fixture(scope='module')
def fx():
    return SN.load_fixture()


@pytest.mark.parametrize('name', SN.CASES)
def test_kernel_reproduces_the_reference(fx, name):
    for call in fx['cases'][name]:
        got = SN.run_kernel(fx['pos'], fx['ori'], fx['normal'], **SN.plan_of(call))
        err = SN.check_against_reference(fx, call, got)
        print('{}: displaced positions within {:.3e} of the reference (bound {:.0e})'.format(name, err, BOUND))


def readings(rng, n, f, m=12):
    """Body-sized positions (|x| < 4, a thigh of about 0.4 m), orientations and normals of any values."""
    base = rng.uniform(-0.8, 0.8, size=(m, 3))
    base[5], base[6] = (-0.10, -0.30, 0.05), (-0.12, -0.72, 0.0)
    pos = (base[None, None] + rng.normal(0, 0.03, size=(n, f, m, 3))).reshape(n, f, m * 3).astype(np.float32)
    return pos, rng.normal(size=(n, f, m * 9)).astype(np.float32), rng.normal(size=(n, f, m * 3)).astype(np.float32)


def spherical_plan(rng, n, f, k, window_len, start=None, sensor=None):
    shape = (n, window_len, k)
    return dict(mode=SN.SPHERICAL, window_len=window_len, max_r=0.8,
                start=rng.integers(0, f - window_len + 1, size=n) if start is None else np.asarray(start),
                sensor=rng.permutation(12)[:k] if sensor is None else np.asarray(sensor),
                u_r=rng.uniform(size=shape).astype(np.float32),
                theta=(rng.uniform(size=shape) * 2 * np.pi).astype(np.float32),
                phi=(rng.uniform(size=shape) * np.pi).astype(np.float32))


def suppress_plan(rng, n, f, k, window_len, start=None, sensor=None, ids=range(12)):
    ids = np.asarray(list(ids))
    return dict(mode=SN.SUPPRESS, window_len=window_len, mask_value=-2.5,
                start=rng.integers(0, f - window_len + 1, size=n) if start is None else np.asarray(start),
                sensor=ids[rng.integers(0, len(ids), size=(n, k))] if sensor is None else np.asarray(sensor))


def check_against_restatement(inputs, plan):
    got = SN.run_kernel(*inputs, **plan)
    want = SN.restate(*inputs, **plan)
    n, f = inputs[0].shape[:2]
    hit = SN.affected(n, f, 12, plan['start'], plan['sensor'], plan['window_len'], plan['mode'])
    if plan['mode'] == SN.SUPPRESS:
        for g, w, x, c in zip(got, want, inputs, (3, 9, 3)):
            assert np.array_equal(g.astype(np.float64), w)
            g4 = g.reshape(n, f, 12, c)
            assert (g4[hit] == plan['mask_value']).all()
            assert np.array_equal(g4[~hit].view(np.int32), x.reshape(n, f, 12, c)[~hit].view(np.int32))   # bit copies
        return 0.0
    assert got[1] is None and got[2] is None
    g, w, x = (a.reshape(n, f, 12, 3) for a in (got[0], want[0], inputs[0]))
    assert np.array_equal(g[~hit].view(np.int32), x[~hit].view(np.int32))
    err = float(np.abs(g[hit].astype(np.float64) - w[hit]).max()) if hit.any() else 0.0
    print('displaced positions within {:.3e} of float64 (bound {:.0e})'.format(err, BOUND))
    assert err <= BOUND
    if hit.any():
        assert np.abs(g[hit] - x[hit]).max() > 1e-3   # ... and displaced at all
    return err


EDGES = {
    # (N, F) = (1, 1): a window of one frame (the thigh's frame F // 2 is frame 0) and an empty window (a pure copy)
    'one_frame': lambda r: (readings(r, 1, 1), [spherical_plan(r, 1, 1, 2, 1), suppress_plan(r, 1, 1, 2, 1)]),
    'empty_window': lambda r: (readings(r, 1, 1), [spherical_plan(r, 1, 1, 2, 0), suppress_plan(r, 1, 1, 2, 0)]),
    # the whole sequence: every start is 0
    'whole_sequence': lambda r: (readings(r, 3, 7), [spherical_plan(r, 3, 7, 3, 7), suppress_plan(r, 3, 7, 3, 7)]),
    # windows that end exactly at F
    'ends_at_F': lambda r: (readings(r, 3, 7), [spherical_plan(r, 3, 7, 2, 3, start=[4, 4, 0]),
                                                suppress_plan(r, 3, 7, 2, 3, start=[4, 0, 4])]),
    'all_sensors': lambda r: (readings(r, 3, 7), [spherical_plan(r, 3, 7, 12, 2), suppress_plan(r, 3, 7, 12, 2)]),
    # a sensor named twice inside one window
    'duplicate_ids': lambda r: (readings(r, 3, 7), [suppress_plan(r, 3, 7, 3, 2, sensor=[[4, 4, 9], [0, 11, 0], [7, 7, 7]]),
                                                    spherical_plan(r, 3, 7, 3, 2, sensor=[4, 9, 4])]),
    'six_sensor_ids': lambda r: (readings(r, 3, 7), [suppress_plan(r, 3, 7, 2, 3, ids=CONST.S_CONFIG_6)]),
    # several workgroups and a ragged tail: 5 * 67 * 12 * 15 floats over 256-thread blocks
    'several_blocks': lambda r: (readings(r, 5, 67), [spherical_plan(r, 5, 67, 3, 20), suppress_plan(r, 5, 67, 3, 20)]),
    # the size training runs at: 256 x 32 windows, 1.47 M floats in 5760 blocks
    'training_batch': lambda r: (readings(r, 256, 32), [spherical_plan(r, 256, 32, 1, 8), suppress_plan(r, 256, 32, 1, 8)]),
}


@pytest.mark.parametrize('edge', sorted(EDGES))
def test_edge_shapes_against_float64(edge):
    inputs, plans = EDGES[edge](np.random.default_rng(sorted(EDGES).index(edge)))
    for plan in plans:
        check_against_restatement(inputs, plan)
        if edge == 'empty_window':
            got = SN.run_kernel(*inputs, **plan)
            for g, x in zip(got, inputs):
                assert g is None or np.array_equal(g.view(np.int32), x.view(np.int32))


def test_repeated_launches_give_identical_bits():
    rng = np.random.default_rng(77)
    inputs = readings(rng, 5, 67)
    for plan in (spherical_plan(rng, 5, 67, 3, 20), suppress_plan(rng, 5, 67, 3, 20)):
        first = SN.run_kernel(*inputs, **plan)
        for _ in range(3):
            for a, b in zip(first, SN.run_kernel(*inputs, **plan)):
                assert a is None and b is None or np.array_equal(a.view(np.int32), b.view(np.int32))


# ---- end to end on the synthetic body model -------------------------------------------------------------------------------
def _amass_batch(n, f):
    from em_pose_amd.data.data import AMASSBatch, AMASSSample
    from em_pose_amd.data.transforms import ToTensor
    rng = np.random.default_rng(8)
    samples = [ToTensor()(AMASSSample('s%d' % i, rng.normal(0, 0.2, size=(f, 66)).astype(np.float32),
                                      rng.normal(0, 1, size=10).astype(np.float32),
                                      rng.normal(0, 1, size=(f, 3)).astype(np.float32), 60.0)) for i in range(n)]
    return AMASSBatch.from_sample_list(samples).to_gpu(torch.device(DEV))


@pytest.mark.parametrize('kind', ['suppress', 'spherical'])
def test_preprocessing_with_noise_and_a_training_step(kind):
    from em_pose_amd.data.transforms import get_end_to_end_preprocess_fn
    from em_pose_amd.nn.models import create_model
    n, f, k, mask = 4, 16, 2, -1.5
    noise = dict(suppression_noise_length=0.3, suppression_noise_value=mask, noise_num_markers=k) if kind == 'suppress' \
        else dict(spherical_noise_length=0.3, spherical_noise_strength=0.8, noise_num_markers=k)
    case = H.load_case('train_lgdrnn12_n2')
    model, vids = H.small_model(), [int(v) for v in case['meta']['vertex_ids']]
    cfg = lgd_config(12, True, 2, hidden=32, rnn_hidden=32, **noise)
    smpl = SMPLLayer(model).to(DEV)
    rng = np.random.default_rng(9)
    offsets = {'means': rng.normal(0, 0.02, size=(12, 3)).astype(np.float32),
               'covs': np.tile(np.eye(3, dtype=np.float32) * 1e-4, (12, 1, 1)),
               'r': np.tile(np.eye(3, dtype=np.float32), (12, 1, 1)), 'vertex_ids': np.asarray(vids)}
    fn = get_end_to_end_preprocess_fn(cfg, smpl, [offsets], randomize_if_configured=True, device_noise=True)
    twin = NF.get_noise_fn(cfg, True)   # a second object with the same seed: the plan the factory's object will draw
    torch.manual_seed(5)
    batch = fn(_amass_batch(n, f))
    # the same seeded pipeline without noise: what marker_*_synth must still be
    torch.manual_seed(5)
    clean = get_end_to_end_preprocess_fn(lgd_config(12, True, 2, hidden=32, rnn_hidden=32), smpl, [offsets],
                                         randomize_if_configured=True, device_noise=True)(_amass_batch(n, f))
    assert clean.marker_pos_noisy is None
    for x in ('pos', 'ori', 'normal'):
        assert torch.equal(getattr(batch, 'marker_%s_synth' % x), getattr(clean, 'marker_%s_synth' % x)), x
    wl = int(0.3 * f)
    plan = (twin.plan(n, f) if kind == 'suppress' else twin.plan(n, f, 12))[1].host
    synth = {x: getattr(batch, 'marker_%s_synth' % x) for x in ('pos', 'ori', 'normal')}
    inp = batch.get_inputs()
    assert inp['marker_pos'].data_ptr() == batch.marker_pos_noisy.data_ptr()
    hit = torch.from_numpy(SN.affected(n, f, 12, plan['start'].numpy(), plan['sensor'].numpy(), wl,
                                       SN.SUPPRESS if kind == 'suppress' else SN.SPHERICAL)).to(DEV)
    distinct = sum(len(set(row.tolist())) for row in plan['sensor'].reshape(n, -1)) if kind == 'suppress' else n * k
    assert int(hit.sum()) == wl * distinct
    if kind == 'suppress':
        for x, key, c in (('pos', 'marker_pos', 3), ('ori', 'marker_oris', 9), ('normal', 'marker_normals', 3)):
            got, src = inp[key].reshape(n, f, 12, c), synth[x].reshape(n, f, 12, c)
            assert inp[key].data_ptr() == getattr(batch, 'marker_%s_noisy' % x).data_ptr()
            masked = (got == mask).all(-1)
            assert torch.equal(masked, hit) and int(masked.sum()) == wl * distinct   # exactly N * wl * K sensors
            assert torch.equal(got[~hit], src[~hit]) and not (src == mask).any()     # marker_*_synth are unchanged
    else:
        assert batch.marker_ori_noisy is None and batch.marker_normal_noisy is None
        assert inp['marker_oris'].data_ptr() == batch.marker_ori_synth.data_ptr()
        got, src = inp['marker_pos'].reshape(n, f, 12, 3), synth['pos'].reshape(n, f, 12, 3)
        assert torch.equal(got[~hit], src[~hit]) and bool(((got[hit] - src[hit]).abs().amax(-1) > 0).all())
    net = create_model(cfg, SMPLLayer(model))
    net.vertex_ids = vids
    net = net.to(DEV).train()
    net.zero_grad()
    total, vals = net.backward(batch, net(batch))
    assert np.isfinite(vals['total_loss']) and vals['total_loss'] > 0


def test_call_does_not_wait_for_the_device():
    rng = np.random.default_rng(3)
    pos, ori, normal = (torch.from_numpy(a).to(DEV) for a in readings(rng, 4, 16))
    import types
    fns = (NF.SphericalMarkerNoise(0.5, 0.5, 2), NF.MarkerSuppressionNoise(0.5, 2, 0.0))
    for fn in fns:   # first calls: library load, pinned-memory pool
        fn(types.SimpleNamespace(marker_pos_synth=pos, marker_ori_synth=ori, marker_normal_synth=normal))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        outs = [fn(types.SimpleNamespace(marker_pos_synth=pos, marker_ori_synth=ori, marker_normal_synth=normal))
                for fn in fns]
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert outs[0].marker_pos_noisy.shape == pos.shape and outs[1].marker_ori_noisy.shape == ori.shape
