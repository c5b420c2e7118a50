"""
Per-vertex error between two bodies (SMPLLayer.vertex_error -> empose_mesh_vertex_error, csrc/mesh_err.hip;
eval/mesh_metrics.py VertexErrorEngine) against float64 through the oracle (oracle/torch_ref.py smpl_fk for both bodies,
per frame the sum over the vertices of |v_A - v_B| and of |v_A - v_B|^2).  The control is the same computation in float32
on the CPU.

The bar is launch-level ("no draw"), not a per-row comparison with the control.  With the sums
divided by V (mean distance, mean square of a frame):
  mean distance: the largest error over the launch's frames is at most 4 x the control's largest error of the launch
                 + 1e-7 x the largest |coordinate| of the launch;
  mean square:   the largest error is at most 4 x the control's largest + 1e-7 x the launch's largest mean square.
Inputs as tests/test_mesh_vjp.py (pose ~ N(0, 0.4), root ~ N(0, 0.5), betas ~ N(0, 1), trans ~ N(0, 1)); body B is A plus
N(0, 0.05) on the pose, N(0, 0.02) on the root, N(0, 0.3) on the betas and N(0, 0.02) on the translation.  Every check
prints its figures before it asserts.
"""
import os
import socket

import numpy as np
import pytest
import torch

from em_pose_amd import synthetic
from em_pose_amd.bodymodels import tables as TB
from em_pose_amd.bodymodels.smpl import SMPLLayer
from em_pose_amd.eval.mesh_metrics import VertexErrorEngine
from em_pose_amd.eval.metrics import MetricsEngine
from oracle import torch_ref as R
from tests import helpers as H

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
MESH_SLAB = 16384


@pytest.fixture(scope='module')
def big_model():
    return synthetic.make_model()


@pytest.fixture(scope='module')
def big_layer(big_model):
    return SMPLLayer(big_model).to(DEV)


def _small_ids():
    return [int(v) for v in H.load_case('train_lgdrnn12_n2')['meta']['vertex_ids']]


def _bodies(rng, n, with_trans=True, zero_frames=()):
    """(pose, root, betas, trans or None) of body A and of body B, float32 numpy."""
    pose = rng.normal(0, 0.4, size=(n, 63)).astype(np.float32)
    root = rng.normal(0, 0.5, size=(n, 3)).astype(np.float32)
    for f in zero_frames:
        pose[f] = 0
        root[f] = 0
    betas = rng.normal(0, 1, size=(n, 10)).astype(np.float32)
    trans = rng.normal(0, 1, size=(n, 3)).astype(np.float32) if with_trans else None
    pose_b = (pose + rng.normal(0, 0.05, size=pose.shape)).astype(np.float32)
    root_b = (root + rng.normal(0, 0.02, size=root.shape)).astype(np.float32)
    betas_b = (betas + rng.normal(0, 0.3, size=betas.shape)).astype(np.float32)
    trans_b = (trans + rng.normal(0, 0.02, size=trans.shape)).astype(np.float32) if with_trans else None
    return (pose, root, betas, trans), (pose_b, root_b, betas_b, trans_b)


def _oracle(model, conv, dtype, a, b, rows=None):
    """Per-vertex distances (n, V') in `dtype` through the oracle (V' = `rows` of the mesh, or all of it), and the
    largest |coordinate| of both bodies."""
    bm = R.BodyModelTensors(model, dtype=dtype, rodrigues_convention=conv)
    t = lambda x: None if x is None else torch.from_numpy(np.asarray(x, dtype=np.float64)).to(dtype)
    va, _ = R.smpl_fk(bm, t(a[0]), t(a[2]), t(a[1]), t(a[3]))
    vb, _ = R.smpl_fk(bm, t(b[0]), t(b[2]), t(b[1]), t(b[3]))
    if rows is not None:
        idx = torch.from_numpy(np.asarray(rows, dtype=np.int64))
        va, vb = va[:, idx], vb[:, idx]
    return (va - vb).norm(dim=-1), float(max(va.abs().max(), vb.abs().max()))


def _sums(d):
    """(n, 2) float64: the per-frame sums of d and d^2, accumulated in d's own precision."""
    return torch.stack([d.sum(dim=1), (d * d).sum(dim=1)], dim=1).to(torch.float64).numpy()


def _ours(layer, a, b):
    g = lambda x: None if x is None else torch.from_numpy(x).to(DEV)
    out = layer.vertex_error(g(a[0]), g(a[2]), g(b[0]), g(b[2]), poses_root=g(a[1]), poses_root_hat=g(b[1]),
                             trans=g(a[3]), trans_hat=g(b[3]))
    assert out.dtype == torch.float64 and tuple(out.shape) == (a[0].shape[0], 2) and out.is_cuda
    assert out.grad_fn is None and not out.requires_grad
    return out.cpu().numpy()


def _check(name, got, model, conv, a, b, rows=None):
    d64, coord = _oracle(model, conv, torch.float64, a, b, rows)
    d32, _ = _oracle(model, conv, torch.float32, a, b, rows)
    V = d64.shape[1]
    ref, ctl = _sums(d64) / V, _sums(d32) / V
    got = got / V
    err, err_c = np.abs(got - ref).max(axis=0), np.abs(ctl - ref).max(axis=0)
    bars = (4 * err_c[0] + 1e-7 * coord, 4 * err_c[1] + 1e-7 * ref[:, 1].max())
    print('{}: V {} frames {} mean distance {:.4f}..{:.4f} m |coord| {:.3f}; mean: err {:.3e} control {:.3e} bar {:.3e}; '
          'mean square: err {:.3e} control {:.3e} bar {:.3e} (largest {:.3e})'.format(
              name, V, got.shape[0], ref[:, 0].min(), ref[:, 0].max(), coord, err[0], err_c[0], bars[0], err[1],
              err_c[1], bars[1], ref[:, 1].max()))
    assert err[0] <= bars[0], name
    assert err[1] <= bars[1], name
    return d64


# ---- against float64 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('conv', ['smplx', 'so3'])
@pytest.mark.parametrize('with_trans', [False, True])
@pytest.mark.parametrize('n', [1, 31, 32, 33, 70])
def test_small_model_against_float64(n, with_trans, conv):
    """V = 160: five tiles for eight waves (three waves have none); block edges at 32 and 64 frames."""
    model = H.small_model()
    layer = SMPLLayer(model, rodrigues_convention=conv).to(DEV)
    a, b = _bodies(np.random.default_rng(100 + n), n, with_trans=with_trans)
    _check('small n={} trans={} {}'.format(n, with_trans, conv), _ours(layer, a, b), model, conv, a, b)


def test_sub_mesh_against_float64():
    """60 vertices: two tiles, 28 live lanes in the last one; the oracle's rows restricted to `needed`."""
    model = H.small_model()
    sub = SMPLLayer(model).to(DEV).sub_mesh(_small_ids())
    assert sub.n_vertices == 60
    a, b = _bodies(np.random.default_rng(7), 33)
    _check('sub-mesh n=33', _ours(sub, a, b), model, 'smplx', a, b, rows=sub.needed)


def test_many_bones_against_float64():
    """Up to six bones per vertex: the kernel's EXTRA form (the model of tests/test_mesh_vjp.py)."""
    model = dict(H.small_model())
    V = model['v_template'].shape[0]
    rng = np.random.default_rng(12)
    w = np.array(model['weights'], dtype=np.float64, copy=True)
    for v in range(0, V, 3):
        bones = rng.choice(22, size=6, replace=False)
        w[v] = 0
        w[v, bones] = rng.uniform(0.1, 1.0, size=6)
        w[v] /= w[v].sum()
    model['weights'] = w.astype(model['weights'].dtype)
    assert TB.build_full_mesh_tables(model)['kb'] == 6
    layer = SMPLLayer(model).to(DEV)
    a, b = _bodies(rng, 33)
    _check('six bones n=33', _ours(layer, a, b), model, 'smplx', a, b)


def test_large_model_against_float64(big_model, big_layer):
    """V = 6890: 216 tiles, the last with 10 live lanes, tiles split over grid.y; zero-pose frames included."""
    a, b = _bodies(np.random.default_rng(3), 70, with_trans=False, zero_frames=(0, 33, 69))
    _check('large n=70', _ours(big_layer, a, b), big_model, 'smplx', a, b)


def test_identical_bodies(big_model, big_layer):
    """B = A, the same tensors: every sum below 1e-6 x V metres, the rounding level of metre-scale fp32 coordinates."""
    a, _ = _bodies(np.random.default_rng(4), 70, with_trans=False)
    got = _ours(big_layer, a, a)
    V = big_model['v_template'].shape[0]
    print('identical bodies: largest sum of distances {:.3e} m, of squares {:.3e}; exact zeros: {}'.format(
        got[:, 0].max(), got[:, 1].max(), not got.any()))
    assert (got >= 0).all() and got.max() < 1e-6 * V


# ---- determinism and independence, bit for bit --------------------------------------------------------------------------
def _tiled(n):
    """n frames: 70 distinct ones, tiled (so no oracle is needed for a large launch), as device tensors."""
    a, b = _bodies(np.random.default_rng(11), 70)
    idx = torch.arange(n) % 70
    take = lambda body: [torch.from_numpy(x)[idx].contiguous().to(DEV) for x in body]
    return take(a), take(b)


def _launch(layer, a, b, sel=None):
    s = (lambda x: x) if sel is None else (lambda x: x[sel].contiguous())
    return layer.vertex_error(s(a[0]), s(a[2]), s(b[0]), s(b[2]), poses_root=s(a[1]), poses_root_hat=s(b[1]),
                              trans=s(a[3]), trans_hat=s(b[3]))


def test_deterministic_and_frames_independent():
    layer = SMPLLayer(H.small_model()).to(DEV)
    a, b = _tiled(70)
    full = _launch(layer, a, b)
    assert torch.equal(full, _launch(layer, a, b))
    assert float(full.min()) > 0
    for k in (0, 31, 32, 45, 63, 64, 69):
        alone = _launch(layer, a, b, torch.tensor([k], device=DEV))
        assert torch.equal(alone[0], full[k]), k
        sel = torch.arange(k - 32, k + 1, device=DEV) % 70          # frame k as the last of 33
        last = _launch(layer, a, b, sel)
        assert torch.equal(last[32], full[k]), k
        assert torch.equal(last, full[sel]), k


def test_slab_edge_bit_for_bit():
    layer = SMPLLayer(H.small_model()).to(DEV)
    n = MESH_SLAB + 33
    a, b = _tiled(n)
    full = _launch(layer, a, b)
    head = _launch(layer, a, b, slice(0, MESH_SLAB))
    tail = _launch(layer, a, b, slice(MESH_SLAB, n))
    assert tuple(full.shape) == (n, 2)
    assert torch.equal(full[:MESH_SLAB], head) and torch.equal(full[MESH_SLAB:], tail)
    assert torch.equal(full[:70], _launch(layer, a, b, slice(0, 70)))
    assert torch.equal(full[70:140], full[:70])                      # the tiled frames repeat


# ---- VertexErrorEngine ----------------------------------------------------------------------------------------------------
def _engine_batch(rng, n, f):
    a, b = _bodies(rng, n * f, with_trans=False)
    shape_a, shape_b = a[2].reshape(n, f, 10)[:, 0].copy(), b[2].reshape(n, f, 10)[:, 0].copy()   # one shape per sequence
    a = (a[0], a[1], np.repeat(shape_a, f, axis=0), None)
    b = (b[0], b[1], np.repeat(shape_b, f, axis=0), None)
    g = lambda x: torch.from_numpy(x).to(DEV)
    args = dict(pose=g(a[0]).reshape(n, f, 63), shape=g(shape_a), pose_hat=g(b[0]).reshape(n, f, 63),
                shape_hat=g(shape_b), pose_root=g(a[1]).reshape(n, f, 3), pose_root_hat=g(b[1]).reshape(n, f, 3))
    return a, b, args


def test_engine_counts_the_valid_frames_and_matches_float64():
    model = H.small_model()
    layer = SMPLLayer(model).to(DEV)
    rng = np.random.default_rng(21)
    n, f = 3, 12
    a, b, args = _engine_batch(rng, n, f)
    seq_lengths = torch.tensor([12, 7, 9])
    frame_mask = torch.ones(n, f, 12)
    frame_mask[0, 3, 5] = 0       # a frame with a missing sensor does not count
    frame_mask[2, 8, 0] = 0
    frame_mask[1, 10, 2] = 0      # (already past its sequence's end)
    valid = MetricsEngine.valid_frames(seq_lengths, n, f, frame_mask).reshape(-1).numpy()
    assert valid.sum() == 12 + 7 + 9 - 2
    eng = VertexErrorEngine(layer)
    eng.compute(seq_lengths=seq_lengths.to(DEV), frame_mask=frame_mask.to(DEV), **args)
    rows = eng.state()['sums']
    assert rows.shape == (int(valid.sum()), 2)
    assert np.array_equal(rows, _ours(layer, a, b)[valid])
    # the `valid` argument names the same frames
    other = VertexErrorEngine(layer)
    other.compute(valid=torch.from_numpy(valid).reshape(n, f), **args)
    assert np.array_equal(other.state()['sums'], rows)

    d64, coord = _oracle(model, 'smplx', torch.float64, a, b)
    d32, _ = _oracle(model, 'smplx', torch.float32, a, b)
    pick = torch.from_numpy(valid)
    d64, d32 = d64[pick].numpy(), d32[pick]
    got = eng.get_metrics()
    want = {'PVE [mm]': d64.mean() * 1e3, 'PVE STD': np.std(d64) * 1e3}
    # the control: float32 distances, float32 per-frame sums, the engine's reduction
    s32 = _sums(d32).sum(axis=0) / d64.size
    ctl = {'PVE [mm]': s32[0] * 1e3, 'PVE STD': np.sqrt(max(s32[1] - s32[0] ** 2, 0.0)) * 1e3}
    for k in want:
        err, err_c = abs(got[k] - want[k]), abs(ctl[k] - want[k])
        bar = 4 * err_c + 1e-7 * coord * 1e3
        print('engine {}: {:.6f} float64 {:.6f}; err {:.3e} control {:.3e} bar {:.3e} (mm)'.format(
            k, got[k], want[k], err, err_c, bar))
        assert err <= bar, k


def test_engine_merge_equals_one_engine_and_gather_in_a_group_of_one():
    import torch.distributed as dist
    layer = SMPLLayer(H.small_model()).to(DEV)
    rng = np.random.default_rng(22)
    _, _, first = _engine_batch(rng, 2, 5)
    _, _, second = _engine_batch(rng, 3, 4)
    lens = torch.tensor([5, 2], device=DEV)
    one, two, both = VertexErrorEngine(layer), VertexErrorEngine(layer), VertexErrorEngine(layer)
    one.compute(seq_lengths=lens, **first)
    two.compute(**second)
    both.compute(seq_lengths=lens, **first)
    both.compute(**second)
    one.merge(two.state())
    want = both.state()['sums']
    assert want.shape == (7 + 12, 2) and np.array_equal(one.state()['sums'], want)
    assert one.get_metrics() == both.get_metrics()
    assert not dist.is_initialized()
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    os.environ['MASTER_ADDR'], os.environ['MASTER_PORT'] = '127.0.0.1', str(port)
    dist.init_process_group('gloo', rank=0, world_size=1)
    try:
        assert one.gather() is one                                # a group of one: nothing to do
        assert np.array_equal(one.gather(force=True).state()['sums'], want)
        empty = VertexErrorEngine(layer).gather(force=True)
        assert empty.state()['sums'].shape == (0, 2)
    finally:
        dist.destroy_process_group()
    assert one.get_metrics() == both.get_metrics()


# ---- the opt-in wiring of the validation loop -----------------------------------------------------------------------------
def test_evaluate_with_a_vertex_engine_changes_nothing_else():
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

    def loader():
        r = np.random.default_rng(10)
        for lens in ((6, 4), (5,)):
            yield AMASSBatch.from_sample_list([ToTensor()(AMASSSample(
                's', r.normal(0, 0.2, size=(n, 66)).astype(np.float32), r.normal(0, 1, size=10).astype(np.float32),
                np.zeros((n, 3), np.float32), 60.0)) for n in lens])
    plain, with_engine, ve = MetricsEngine(smpl), MetricsEngine(smpl), VertexErrorEngine(smpl)
    ve.merge({'sums': np.ones((3, 2))})        # `evaluate` resets the engine, as it resets the metrics engine
    losses = evaluate(loader(), net, fn, plain, device=torch.device(DEV))
    losses_ve = evaluate(loader(), net, fn, with_engine, device=torch.device(DEV), vertex_engine=ve)
    assert losses == losses_ve
    assert plain.get_metrics() == with_engine.get_metrics()
    for x, y in zip(plain.state().values(), with_engine.state().values()):
        assert np.array_equal(x, y)
    rows = ve.state()['sums']
    assert rows.shape == (15, 2) and np.isfinite(rows).all() and (rows > 0).all()
    m = ve.get_metrics()
    assert 0 < m['PVE [mm]'] < 1000 and m['PVE STD'] > 0
