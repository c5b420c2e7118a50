"""
Procrustes-aligned per-vertex error (SMPLLayer.vertex_error(..., procrustes=True) -> empose_mesh_vertex_error_pa,
csrc/mesh_err.hip; VertexErrorEngine(procrustes=True)) against float64 through the oracle and the restatement of the
definition in tests/vertex_error_pa_ref.py.  The control is that file's float32 form, which has the kernel's error
sources: float32 vertices, float32 moments about the posed root joints over groups of 32 vertices, a float64 solve,
float32 transform and float32 aligned distances.

The bar is the launch-level bar of tests/test_vertex_error.py ("no draw"), on columns 2 and 3 divided by V:
  mean aligned distance: the largest error over the launch's frames is at most 4 x the control's largest error of the
                         launch + 1e-7 x the largest |coordinate| of the launch;
  mean square:           the largest error is at most 4 x the control's largest + 1e-7 x the launch's largest mean square.
Columns 0 and 1 are bit for bit empose_mesh_vertex_error's.  Inputs: tests/test_vertex_error.py `_bodies`.  Every check
prints its figures before it asserts.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from em_pose_amd import synthetic
from em_pose_amd.bodymodels import tables as TB
from em_pose_amd.bodymodels.smpl import SMPLLayer
from em_pose_amd.eval.mesh_metrics import VertexErrorEngine
from em_pose_amd.eval.metrics import MetricsEngine
from tests import helpers as H
from tests import vertex_error_pa_ref as P
from tests.test_vertex_error import MESH_SLAB, _bodies, _engine_batch, _small_ids, _tiled

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def big_model():
    return synthetic.make_model()


@pytest.fixture(scope='module')
def big_layer(big_model):
    return SMPLLayer(big_model).to(DEV)


def _ours(layer, a, b, procrustes=True):
    g = lambda x: None if x is None else torch.from_numpy(x).to(DEV)
    out = layer.vertex_error(g(a[0]), g(a[2]), g(b[0]), g(b[2]), poses_root=g(a[1]), poses_root_hat=g(b[1]),
                             trans=g(a[3]), trans_hat=g(b[3]), procrustes=procrustes)
    assert out.dtype == torch.float64 and tuple(out.shape) == (a[0].shape[0], 4 if procrustes else 2) and out.is_cuda
    assert out.grad_fn is None and not out.requires_grad
    return out.cpu().numpy()


def _reference(model, conv, a, b, rows=None):
    """float64 and control aligned distances (n, V'), the float64 plain distances, the largest |coordinate|."""
    x, y, _, _ = P.bodies(model, conv, torch.float64, a, b, rows)
    x32, y32, pa32, pb32 = P.bodies(model, conv, torch.float32, a, b, rows)
    assert x32.dtype == np.float32 and pa32.dtype == np.float32
    return (P.distances64(x, y), P.distances32(x32, y32, pa32, pb32), np.linalg.norm(x - y, axis=-1),
            float(max(np.abs(x).max(), np.abs(y).max())))


def _check(name, got, model, conv, a, b, rows=None):
    d64, d32, plain64, coord = _reference(model, conv, a, b, rows)
    V = d64.shape[1]
    ref, ctl = P.sums(d64) / V, P.sums(d32) / V
    got_pa = got[:, 2:] / V
    err, err_c = np.abs(got_pa - ref).max(axis=0), np.abs(ctl - ref).max(axis=0)
    bars = (4 * err_c[0] + 1e-7 * coord, 4 * err_c[1] + 1e-7 * ref[:, 1].max())
    print('{}: V {} frames {} mean aligned distance {:.4f}..{:.4f} m (plain {:.4f}..{:.4f}) |coord| {:.3f}; mean: err '
          '{:.3e} control {:.3e} bar {:.3e}; mean square: err {:.3e} control {:.3e} bar {:.3e} (largest {:.3e})'.format(
              name, V, got.shape[0], ref[:, 0].min(), ref[:, 0].max(), plain64.mean(axis=1).min(),
              plain64.mean(axis=1).max(), coord, err[0], err_c[0], bars[0], err[1], err_c[1], bars[1], ref[:, 1].max()))
    assert err[0] <= bars[0], name
    assert err[1] <= bars[1], name
    # the optimal similarity cannot do worse than the identity: in the mean square, up to the bar, on every frame
    plain_sq = (plain64 * plain64).mean(axis=1)
    assert (ref[:, 1] <= plain_sq).all(), name
    assert (got_pa[:, 1] <= plain_sq + bars[1]).all(), name
    assert (got[:, 3] / V <= got[:, 1] / V + 2 * bars[1]).all(), name


# ---- against float64 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('conv', ['smplx', 'so3'])
@pytest.mark.parametrize('with_trans', [False, True])
@pytest.mark.parametrize('n', [1, 31, 32, 33, 70])
def test_small_model_against_float64(n, with_trans, conv):
    """V = 160: five tiles for eight waves; block edges at 32 and 64 frames.  (With float32 transforms in the aligned
    sweep the single-frame launch [1-False-smplx] missed its mean-square bar, 9.4e-10 against 8.7e-10: the loss was in the
    float32 rotations and rest joints ahead of the sweep, and the float64 prologue of that sweep removed it.)"""
    model = H.small_model()
    layer = SMPLLayer(model, rodrigues_convention=conv).to(DEV)
    a, b = _bodies(np.random.default_rng(100 + n), n, with_trans=with_trans)
    _check('small n={} trans={} {}'.format(n, with_trans, conv), _ours(layer, a, b), model, conv, a, b)


def test_sub_mesh_against_float64():
    """60 vertices: two tiles, 28 live lanes in the last one; the alignment is that of the 60 vertices."""
    model = H.small_model()
    sub = SMPLLayer(model).to(DEV).sub_mesh(_small_ids())
    assert sub.n_vertices == 60
    a, b = _bodies(np.random.default_rng(7), 33)
    _check('sub-mesh n=33', _ours(sub, a, b), model, 'smplx', a, b, rows=sub.needed)


def _six_bone_model(rng):
    model = dict(H.small_model())
    V = model['v_template'].shape[0]
    w = np.array(model['weights'], dtype=np.float64, copy=True)
    for v in range(0, V, 3):
        bones = rng.choice(22, size=6, replace=False)
        w[v] = 0
        w[v, bones] = rng.uniform(0.1, 1.0, size=6)
        w[v] /= w[v].sum()
    model['weights'] = w.astype(model['weights'].dtype)
    assert TB.build_full_mesh_tables(model)['kb'] == 6
    return model


def test_many_bones_against_float64():
    """Up to six bones per vertex: the kernel's EXTRA form in both sweeps."""
    rng = np.random.default_rng(12)
    model = _six_bone_model(rng)
    layer = SMPLLayer(model).to(DEV)
    a, b = _bodies(rng, 33)
    _check('six bones n=33', _ours(layer, a, b), model, 'smplx', a, b)


def test_large_model_against_float64(big_model, big_layer):
    """V = 6890: 216 tiles, the last with 10 live lanes, tiles split over grid.y; zero-pose frames included."""
    a, b = _bodies(np.random.default_rng(3), 70, with_trans=False, zero_frames=(0, 33, 69))
    _check('large n=70', _ours(big_layer, a, b), big_model, 'smplx', a, b)


# ---- columns 0 and 1 are the plain call's ----------------------------------------------------------------------------------
def test_plain_columns_bit_for_bit(big_layer):
    small = SMPLLayer(H.small_model()).to(DEV)
    cases = (('small n=70', small, _bodies(np.random.default_rng(170), 70)),
             ('sub-mesh', small.sub_mesh(_small_ids()), _bodies(np.random.default_rng(7), 33)),
             ('large', big_layer, _bodies(np.random.default_rng(3), 70, with_trans=False, zero_frames=(0, 33, 69))))
    for name, layer, (a, b) in cases:
        pa, plain = _ours(layer, a, b), _ours(layer, a, b, procrustes=False)
        assert np.array_equal(pa[:, :2], plain), name


# ---- what the alignment is for ------------------------------------------------------------------------------------------------
def test_rigidly_moved_body(big_model, big_layer):
    """B is A with another root orientation and another translation: SMPL rotates about the root joint, so B is a rigid
    motion of A.  The plain error is large, the aligned one is rounding."""
    rng = np.random.default_rng(5)
    a, _ = _bodies(rng, 70)
    b = (a[0], (a[1] + rng.normal(0, 0.5, size=a[1].shape)).astype(np.float32), a[2],
         (a[3] + rng.normal(0, 0.3, size=a[3].shape)).astype(np.float32))
    got = _ours(big_layer, a, b)
    V = big_model['v_template'].shape[0]
    print('rigidly moved body: plain mean distance {:.4f}..{:.4f} m; aligned sums: largest of distances {:.3e} m, of '
          'squares {:.3e} (bound {:.3e})'.format(got[:, 0].min() / V, got[:, 0].max() / V, got[:, 2].max(),
                                                 got[:, 3].max(), 1e-6 * V))
    assert (got[:, 0] / V > 0.05).all()
    assert (got[:, 2:] >= 0).all() and got[:, 2:].max() < 1e-6 * V


def test_identical_bodies(big_model, big_layer):
    a, _ = _bodies(np.random.default_rng(4), 70, with_trans=False)
    got = _ours(big_layer, a, a)
    V = big_model['v_template'].shape[0]
    print('identical bodies: largest sum of distances {:.3e} m (aligned {:.3e}), of squares {:.3e} (aligned {:.3e})'
          .format(got[:, 0].max(), got[:, 2].max(), got[:, 1].max(), got[:, 3].max()))
    assert np.isfinite(got).all() and (got >= 0).all() and got.max() < 1e-6 * V


# ---- determinism and independence, bit for bit --------------------------------------------------------------------------
def _launch(layer, a, b, sel=None):
    s = (lambda x: x) if sel is None else (lambda x: x[sel].contiguous())
    return layer.vertex_error(s(a[0]), s(a[2]), s(b[0]), s(b[2]), poses_root=s(a[1]), poses_root_hat=s(b[1]),
                              trans=s(a[3]), trans_hat=s(b[3]), procrustes=True)


def test_deterministic_and_frames_independent():
    layer = SMPLLayer(H.small_model()).to(DEV)
    a, b = _tiled(70)
    full = _launch(layer, a, b)
    assert tuple(full.shape) == (70, 4)
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
    assert tuple(full.shape) == (n, 4)
    assert torch.equal(full[:MESH_SLAB], head) and torch.equal(full[MESH_SLAB:], tail)
    assert torch.equal(full[:70], _launch(layer, a, b, slice(0, 70)))
    assert torch.equal(full[70:140], full[:70])                      # the tiled frames repeat


# ---- VertexErrorEngine ----------------------------------------------------------------------------------------------------
def test_engine_counts_the_valid_frames_and_matches_float64():
    model = H.small_model()
    layer = SMPLLayer(model).to(DEV)
    rng = np.random.default_rng(21)
    n, f = 3, 12
    a, b, args = _engine_batch(rng, n, f)
    seq_lengths = torch.tensor([12, 7, 9])
    frame_mask = torch.ones(n, f, 12)
    frame_mask[0, 3, 5] = 0
    frame_mask[2, 8, 0] = 0
    frame_mask[1, 10, 2] = 0
    valid = MetricsEngine.valid_frames(seq_lengths, n, f, frame_mask).reshape(-1).numpy()
    assert valid.sum() == 12 + 7 + 9 - 2
    calls = []

    class Counting(object):        # the layer, with its calls counted: one per `compute`, not two
        n_vertices = layer.n_vertices

        def vertex_error(self, *x, **kw):
            calls.append(kw.get('procrustes', False))
            return layer.vertex_error(*x, **kw)
    eng, plain = VertexErrorEngine(Counting(), procrustes=True), VertexErrorEngine(layer)
    for e in (eng, plain):
        e.compute(seq_lengths=seq_lengths.to(DEV), frame_mask=frame_mask.to(DEV), **args)
    assert calls == [True]
    st = eng.state()
    assert list(st) == ['sums', 'sums_pa']
    assert st['sums'].shape == st['sums_pa'].shape == (int(valid.sum()), 2)
    assert np.array_equal(st['sums'], plain.state()['sums'])
    assert np.array_equal(np.concatenate([st['sums'], st['sums_pa']], axis=1), _ours(layer, a, b)[valid])

    d64, d32, _, coord = _reference(model, 'smplx', a, b)
    d64, d32 = d64[valid], d32[valid]
    got = eng.get_metrics()
    assert list(got) == ['PVE [mm]', 'PVE STD', 'PA-PVE [mm]', 'PA-PVE STD']
    assert {k: got[k] for k in ('PVE [mm]', 'PVE STD')} == plain.get_metrics()
    want = {'PA-PVE [mm]': d64.mean() * 1e3, 'PA-PVE STD': np.std(d64) * 1e3}
    s32 = P.sums(d32).sum(axis=0) / d64.size       # the control: float32 per-frame sums, the engine's reduction
    ctl = {'PA-PVE [mm]': s32[0] * 1e3, 'PA-PVE STD': np.sqrt(max(s32[1] - s32[0] ** 2, 0.0)) * 1e3}
    for k in want:
        err, err_c = abs(got[k] - want[k]), abs(ctl[k] - want[k])
        bar = 4 * err_c + 1e-7 * coord * 1e3
        print('engine {}: {:.6f} float64 {:.6f}; err {:.3e} control {:.3e} bar {:.3e} (mm)'.format(
            k, got[k], want[k], err, err_c, bar))
        assert err <= bar, k
    # merge carries both
    other = VertexErrorEngine(layer, procrustes=True)
    other.merge(st)
    assert other.get_metrics() == got


def test_evaluate_with_a_procrustes_vertex_engine():
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
    ve, ve_pa = VertexErrorEngine(smpl), VertexErrorEngine(smpl, procrustes=True)
    evaluate(loader(), net, fn, MetricsEngine(smpl), device=torch.device(DEV), vertex_engine=ve)
    evaluate(loader(), net, fn, MetricsEngine(smpl), device=torch.device(DEV), vertex_engine=ve_pa)
    st = ve_pa.state()
    assert st['sums_pa'].shape == (15, 2) and np.array_equal(st['sums'], ve.state()['sums'])
    m = ve_pa.get_metrics()
    print('evaluate: {}'.format(m))
    assert len(m) == 4 and all(np.isfinite(v) for v in m.values())
    assert 0 < m['PA-PVE [mm]'] <= m['PVE [mm]'] < 1000


# ---- the fitter's script ----------------------------------------------------------------------------------------------------
def test_fit_sensors_script_prints_the_surface_errors():
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    res = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'fit_sensors.py'), '--synthetic', '--steps', '10',
                          '--windows', '4', '--frames', '8'], env=env, stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, timeout=300)
    text = res.stdout.decode()
    print(text)
    assert res.returncode == 0, text
    lines = text.splitlines()
    head = [ln for ln in lines if 'MPJPE [mm]' in ln][0]
    assert head.index('PVE [mm]') < head.index('PA-PVE [mm]') and head.index('MPJAE [deg]') < head.index('PVE [mm]')
    for name in ('zero init', 'fitter, 10 steps'):
        cells = [ln for ln in lines if ln.startswith(name)][0][22:].split()
        assert len(cells) == 5
        pve, pa_pve = float(cells[3]), float(cells[4])
        assert 0 < pa_pve <= pve < 5000, (name, cells)
