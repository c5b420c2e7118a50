"""
The loss and bookkeeping kernels of the training step (csrc/train_glue.hip, csrc/train_loss.hip) against their float64 restatements
(tests/train_glue_ref.py), at every output element and within allowances derived from the kernels' rounding chains:
empose_lgd_losses (both kernels), empose_lgd_cotangent_step, empose_lgd_additive_update, empose_window_mean,
empose_axpby2d, empose_lgd_assemble_inputs, and one training step of the engine whose logged losses are recomputed from
its own histories.  Every output buffer is pre-filled with NaN, so an element a kernel does not write fails.
"""
import itertools

import numpy as np
import pytest
import torch

from em_pose_amd import _lib
from em_pose_amd.helpers.configuration import CONSTANTS
from oracle import torch_ref as R
from tests import elementwise as E
from tests import helpers as H
from tests import train_glue_ref as G

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SENTINEL = -7.5


def _idx(n_markers):
    return list(range(12)) if n_markers == 12 else list(CONSTANTS.S_CONFIG_6)


def _hold(name, got, want, allow, row_mod=64):
    got, want, allow = (t.reshape(-1, t.shape[-1]) if t.dim() != 2 else t for t in (got, want, allow))
    r = E.check(name, got.cpu(), want, allow, row_mod=row_mod, col_mod=max(1, min(32, want.shape[-1])))
    assert r.ok, r.message


def _same_bits(a, b):
    return bool((a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)).all())


# ---- (a) empose_lgd_losses -------------------------------------------------------------------------------------------
LOSS_SHAPES = [(1, 1, 1), (3, 16, 3), (5, 7, 2), (7, 99, 3)]   # 7 * 99 * 3 = 2079 items: the unrolled reduce loop + a tail


def _check_losses(name, io, got):
    want = G.losses64(io)
    allow = G.losses_allowance(io, want)
    print(name, 'loss_vals', got['loss_vals'].tolist(), 'err / allowance',
          ((got['loss_vals'].double() - want['loss_vals']).abs() / allow['loss_vals'].clamp_min(1e-300)).tolist())
    _hold(name + ' loss_vals', got['loss_vals'].reshape(1, 5), want['loss_vals'].reshape(1, 5),
          allow['loss_vals'].reshape(1, 5))
    for k in G.COTANGENTS:
        _hold('%s %s' % (name, k), got[k], want[k], allow[k], row_mod=io['F'])
    # exact zeros: padding frames everywhere, dropped frames and unread sensors in the reconstruction / FK cotangents
    padding, dropped = G.dead_rows(io)
    N1, T = io['n_hist'], io['B'] * io['F']
    assert (got['d_pose'][:, padding] == 0).all() and (got['d_shape'][:, padding] == 0).all(), name
    dead = padding | dropped
    assert (got['d_markers'][:, dead] == 0).all() and (got['d_markers_ori'][:, dead] == 0).all(), name
    assert (got['d_joints'][dead] == 0).all(), name
    unread = [m for m in range(12) if m not in io['marker_idx']]
    assert (got['d_markers'].reshape(N1, T, 12, 3)[:, :, unread] == 0).all(), name
    assert (got['d_markers_ori'].reshape(N1, T, 12, 9)[:, :, unread] == 0).all(), name
    if io['joints_gt'] is None:
        assert (got['d_joints'] == 0).all(), name      # zeros, not NaN
    # the L1 cotangent where hat == gt is exactly 0, as torch.sign
    assert (got['d_pose'][io['pose_hist'] == io['pose_gt'][None]] == 0).all(), name
    shape_gt = io['shape_gt'][:, None].expand(io['B'], io['F'], 10).reshape(1, T, 10)
    assert (got['d_shape'][io['shape_hist'] == shape_gt] == 0).all(), name
    return want


@pytest.mark.parametrize('masks', [None, 'ones', 'zeros'])
@pytest.mark.parametrize('n_markers', [12, 6])
@pytest.mark.parametrize('B,F,n_hist', LOSS_SHAPES)
def test_losses_and_cotangents_match_float64_at_every_element(B, F, n_hist, n_markers, masks):
    idx = _idx(n_markers)
    for ld_extra, lengths, fk in itertools.product((0, 76), (None, 'ragged'), (None, 0.0, 0.1)):
        io = G.make_loss_case(B, F, n_hist, n_markers, idx, ld_extra, lengths, masks, fk, seed=3)
        name = 'losses B%d F%d n%d m%d ld+%d %s %s fk=%s' % (B, F, n_hist, n_markers, ld_extra, lengths, masks, fk)
        got = G.run_losses(io, DEV)
        _check_losses(name, io, got)
        again = G.run_losses(io, DEV)
        for k in got:
            assert _same_bits(got[k], again[k]), (name, k, 'two launches differ')
        if masks == 'ones':        # the all-ones mask gives the bits of the NULL mask
            bare = G.run_losses(dict(io, marker_masks=None), DEV)
            for k in got:
                assert _same_bits(got[k], bare[k]), (name, k, 'all-ones mask differs from no mask')


@pytest.mark.parametrize('n_markers', [12, 6])
@pytest.mark.parametrize('B,F,n_hist', [(3, 16, 3), (5, 7, 2)])
def test_losses_ignore_what_padding_and_dropped_frames_hold(B, F, n_hist, n_markers):
    """NaN in the padding frames (f >= len) of every history and ground-truth array, and, separately, NaN in the sensor
    histories of the frames a missing sensor drops: every output keeps the bits of the clean run."""
    io = G.make_loss_case(B, F, n_hist, n_markers, _idx(n_markers), 76, 'ragged', 'zeros', 0.1, seed=5)
    clean = G.run_losses(io, DEV)
    _check_losses('clean', io, clean)
    padding, dropped = G.dead_rows(io)
    assert padding.any() and (dropped & ~padding).any()
    nan = float('nan')
    poisoned = dict(io)
    for k in ('pose_hist', 'shape_hist', 'markers_hist', 'markers_ori_hist'):
        poisoned[k] = io[k].clone()
        poisoned[k][:, padding] = nan
    for k in ('joints_final', 'pose_gt', 'joints_gt', 'inputs'):
        poisoned[k] = io[k].clone()
        poisoned[k][padding] = nan
    got = G.run_losses(poisoned, DEV)
    for k in clean:
        assert _same_bits(got[k], clean[k]), ('padding leaks into', k)
    poisoned = dict(io)
    for k in ('markers_hist', 'markers_ori_hist'):
        poisoned[k] = io[k].clone()
        poisoned[k][:, dropped] = nan
    got = G.run_losses(poisoned, DEV)
    for k in clean:
        assert _same_bits(got[k], clean[k]), ('dropped frames leak into', k)


# ---- (b) empose_lgd_cotangent_step -----------------------------------------------------------------------------------
def _guarded(rows, cols, fill, g=None):
    """(rows + 1, cols) device buffer: `fill` ('nan', 'randn') in the first rows, SENTINEL in the guard row."""
    t = torch.full((rows + 1, cols), SENTINEL, dtype=torch.float32)
    t[:rows] = float('nan') if fill == 'nan' else torch.randn(rows, cols, generator=g)
    return t


def _cotangent_case(B, F, first, with_g, shape_avg, with_pad, seed=0):
    g = torch.Generator().manual_seed(seed + 100 * F + B)
    T, d_in = B * F, 72
    ldx = d_in + 152
    rn = lambda *s: torch.randn(*s, generator=g)
    host = {'d_pose': rn(T, 66), 'd_shape': rn(T, 10), 'vp': rn(T, 66), 'vs': rn(T, 10), 'X': 50.0 * rn(T, ldx),
            'Dp': _guarded(T, 66, 'nan' if first else 'randn', g), 'Ds': _guarded(T, 10, 'nan' if first else 'randn', g),
            'dpad': _guarded(T, 68, 'nan'), 'dspad': _guarded(T, 12, 'nan')}
    dev = {k: v.to(DEV) for k, v in host.items()}
    step = 0.1
    # g_theta / g_beta: views into the [T][d_in + 152] rows, ld_g = ld_gb = ldx, as the engine passes them
    g_theta = dev['X'][:, d_in + 76:] if with_g else None
    g_beta = dev['X'][:, d_in + 142:] if with_g else None
    rc = G.run_cotangent_step(B, F, first, dev['d_pose'], dev['d_shape'], dev['vp'], dev['vs'], g_theta, ldx, g_beta, ldx,
                              dev['Dp'], dev['Ds'], step, shape_avg, dev['dpad'] if with_pad else None,
                              dev['dspad'] if with_pad else None)
    _lib.check(rc)
    torch.cuda.synchronize()
    args = (B, F, first, host['d_pose'], host['d_shape'], host['vp'], host['vs'],
            host['X'][:, d_in + 76:d_in + 142] if with_g else None, host['X'][:, d_in + 142:d_in + 152] if with_g else None,
            host['Dp'][:T], host['Ds'][:T], step, shape_avg)
    want = G.cotangent_step64(*args)
    mag = G.cotangent_step64(*args, magnitude=True)
    name = 'cotangent B%d F%d first%d g%d avg%d pad%d' % (B, F, first, with_g, shape_avg, with_pad)
    got = {k: dev[k].cpu() for k in ('Dp', 'Ds', 'dpad', 'dspad')}
    _hold(name + ' Dp', got['Dp'][:T], want[0], G.CHAIN_RUN * G.U * mag[0], row_mod=F)
    _hold(name + ' Ds', got['Ds'][:T], want[1], G.CHAIN_RUN * G.U * mag[1], row_mod=F)
    if with_pad:
        _hold(name + ' dpad', got['dpad'][:T, :66], want[2], G.CHAIN_RUN * G.U * mag[2], row_mod=F)
        chain = G.chain_mean(F) if shape_avg else G.CHAIN_RUN
        _hold(name + ' dspad', got['dspad'][:T, :10], want[3], chain * G.U * mag[3], row_mod=F)
        assert (got['dpad'][:T, 66:] == 0).all() and (got['dspad'][:T, 10:] == 0).all(), name   # written, although NaN before
    else:
        assert torch.isnan(got['dpad'][:T]).all() and torch.isnan(got['dspad'][:T]).all(), name
    for k in got:
        assert (got[k][T] == SENTINEL).all(), (name, k, 'guard row written')
    assert torch.equal(dev['X'].cpu(), host['X']), name


@pytest.mark.parametrize('B', [1, 5])
@pytest.mark.parametrize('F', [1, 3, 16, 37])   # F = 1: pose parts of 17, 17, 17, 15 entries; F = 37: 611 per part, not 256 k
def test_cotangent_step_matches_float64_and_writes_its_padding_columns(F, B):
    for first, with_g, shape_avg, with_pad in itertools.product((0, 1), (False, True), (0, 1), (False, True)):
        _cotangent_case(B, F, first, with_g, shape_avg, with_pad)


def test_cotangent_step_accepts_the_longest_window_its_shared_memory_holds():
    _cotangent_case(1, 1228, 1, True, 1, True)


# ---- (c) empose_lgd_additive_update ----------------------------------------------------------------------------------
@pytest.mark.parametrize('B', [1, 5])
@pytest.mark.parametrize('F', [1, 3, 16, 37])
def test_additive_update_matches_float64(F, B):
    T = B * F
    g = torch.Generator().manual_seed(F * 10 + B)
    pose, d_pose, shape, d_shape = (torch.randn(T, n, generator=g) for n in (66, 66, 10, 10))
    dev = [t.to(DEV) for t in (pose, d_pose, shape, d_shape)]
    for shape_avg, step in itertools.product((0, 1), (0.1, 1.0)):
        name = 'update B%d F%d avg%d step%g' % (B, F, shape_avg, step)
        pose_next, shape_next = G.run_additive_update(B, F, step, shape_avg, *dev)
        torch.cuda.synchronize()
        want = G.additive_update64(B, F, step, shape_avg, pose, d_pose, shape, d_shape)
        mag = G.additive_update64(B, F, step, shape_avg, pose, d_pose, shape, d_shape, magnitude=True)
        chain_s = G.chain_next(F) if shape_avg else G.CHAIN_NEXT
        _hold(name + ' pose_next', pose_next, want[0], G.CHAIN_NEXT * G.U * mag[0], row_mod=F)
        _hold(name + ' shape_next', shape_next, want[1], chain_s * G.U * mag[1], row_mod=F)
        if shape_avg:   # every frame of a window moved by the same amount: step * the float64 window mean
            moved = shape_next.cpu().double() - shape.double()
            _hold(name + ' shape_next - shape', moved, G.f32(step) * G.window_mean64(d_shape, F),
                  chain_s * G.U * mag[1], row_mod=F)


# ---- (d) empose_window_mean ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ld', [10, 12])
@pytest.mark.parametrize('windows', [1, 5])
@pytest.mark.parametrize('F', [1, 7, 32])
def test_window_mean_matches_float64_and_is_its_own_adjoint(F, windows, ld):
    T, Cc = F * windows, 10
    g = torch.Generator().manual_seed(F + windows)
    x, y = torch.randn(T, ld, generator=g), torch.randn(T, ld, generator=g)
    outs = []
    for src in (x, y):
        out = torch.full((T, ld), SENTINEL, dtype=torch.float32, device=DEV)
        G.run_window_mean(T, F, Cc, src.to(DEV), out)
        torch.cuda.synchronize()
        out = out.cpu()
        _hold('window mean F%d T%d ld%d' % (F, T, ld), out[:, :Cc], G.window_mean64(src[:, :Cc], F),
              F * G.U * G.window_mean_magnitude(src[:, :Cc], F), row_mod=F)
        assert (out[:, Cc:] == SENTINEL).all()
        outs.append(out[:, :Cc].double())
    # <mean(x), y> = <x, mean(y)>, each side within the summed allowances of its products
    x64, y64 = x[:, :Cc].double(), y[:, :Cc].double()
    lhs, rhs = float((outs[0] * y64).sum()), float((x64 * outs[1]).sum())
    slack = F * G.U * float((G.window_mean_magnitude(x64, F) * y64.abs()).sum()
                            + (x64.abs() * G.window_mean_magnitude(y64, F)).sum())
    assert abs(lhs - rhs) <= slack, (lhs, rhs, slack)


# ---- (e) empose_axpby2d ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rows,cols', [(1, 1), (5, 51), (1, 255), (257, 1)])   # rows * cols in {1, 255, 257}
def test_axpby2d_matches_float64_and_stays_inside_its_block(rows, cols):
    g = torch.Generator().manual_seed(rows + cols)
    alpha, beta = 0.3, -1.7
    wide = lambda extra: torch.randn(rows + 1, cols + extra, generator=g)
    for use_x, use_y in ((True, True), (False, True), (True, False)):
        x, y = (wide(3) if use_x else None), (wide(5) if use_y else None)
        out = torch.full((rows + 1, cols + 2), SENTINEL, dtype=torch.float32, device=DEV)
        G.run_axpby(rows, cols, alpha, None if x is None else x.to(DEV), beta, None if y is None else y.to(DEV), out)
        torch.cuda.synchronize()
        out = out.cpu()
        xs, ys = (None if x is None else x[:rows, :cols]), (None if y is None else y[:rows, :cols])
        like = torch.empty(rows, cols)
        _hold('axpby %dx%d x%d y%d' % (rows, cols, use_x, use_y), out[:rows, :cols], G.axpby64(alpha, xs, beta, ys, like),
              G.CHAIN_AXPBY * G.U * G.axpby64(alpha, xs, beta, ys, like, magnitude=True))
        assert (out[:rows, cols:] == SENTINEL).all() and (out[rows] == SENTINEL).all()
    # out aliasing x
    x, y = wide(3), wide(5)
    xd = x.to(DEV)
    G.run_axpby(rows, cols, alpha, xd, beta, y.to(DEV), xd)
    torch.cuda.synchronize()
    got = xd.cpu()
    like = torch.empty(rows, cols)
    _hold('axpby in place', got[:rows, :cols], G.axpby64(alpha, x[:rows, :cols], beta, y[:rows, :cols], like),
          G.CHAIN_AXPBY * G.U * G.axpby64(alpha, x[:rows, :cols], beta, y[:rows, :cols], like, magnitude=True))
    assert torch.equal(got[:rows, cols:], x[:rows, cols:]) and torch.equal(got[rows], x[rows])


# ---- (f) empose_lgd_assemble_inputs ----------------------------------------------------------------------------------
@pytest.mark.parametrize('T', [1, 48, 300])
@pytest.mark.parametrize('d_in', [72, 144])
def test_assemble_inputs_copies_exactly_and_leaves_the_gradient_columns(d_in, T):
    g = torch.Generator().manual_seed(d_in + T)
    x0, pose, shape = torch.randn(T, d_in, generator=g), torch.randn(T, 66, generator=g), torch.randn(T, 10, generator=g)
    X = torch.full((T + 1, d_in + 152), SENTINEL, dtype=torch.float32, device=DEV)
    G.run_assemble(T, d_in, x0.to(DEV), pose.to(DEV), shape.to(DEV), X)
    torch.cuda.synchronize()
    X = X.cpu()
    assert _same_bits(X[:T, :d_in + 76], G.assemble64(x0, pose, shape))
    assert (X[:T, d_in + 76:] == SENTINEL).all() and (X[T] == SENTINEL).all()


# ---- (g) the engine's wiring of empose_lgd_losses --------------------------------------------------------------------
@pytest.mark.parametrize('released', [True, False], ids=['shape_avg+fk', 'plain'])
def test_training_step_logs_the_losses_of_its_own_histories(released):
    """One engine step of a 6-sensor model on a batch with missing sensors: the logged loss values equal the float64
    losses of the step's own histories and the batch -- ld_inputs, marker_idx, the mask reshape and the weights as
    nn/train_engine.py passes them."""
    from em_pose_amd import synthetic
    from em_pose_amd.bodymodels.smpl import SMPLLayer
    from em_pose_amd.data.data import SyntheticBatch
    from em_pose_amd.helpers.configuration import lgd_config
    from em_pose_amd.nn.models import create_model

    class MaskedBatch(SyntheticBatch):
        def get_inputs(self, sf=None, ef=None, **kwargs):
            inp = super(MaskedBatch, self).get_inputs(sf, ef, **kwargs)
            inp['marker_masks'] = self.marker_masks[:, sf:ef]
            return inp
    model = H.small_model()
    bm = R.BodyModelTensors(model)
    vids = [int(v) for v in np.random.default_rng(5).choice(model['v_template'].shape[0], 12, replace=False)]
    tables = R.sensor_tables(model['f'], vids)

    def sensors(poses, betas, o_r, o_t):
        with torch.no_grad():
            p, o, _ = R.estimated_markers(bm, tables, vids, torch.from_numpy(poses), torch.from_numpy(betas),
                                          torch.from_numpy(o_r), torch.from_numpy(o_t))
        return p.numpy(), o.numpy()
    B, F, N = 3, 16, 2
    w = synthetic.make_windows(B, F, 3, sensors)
    torch.manual_seed(7)
    more = {} if released else {'m_average_shape': False, 'm_fk_loss': 0.0}
    net = create_model(lgd_config(6, True, N, hidden=32, rnn_hidden=32, **more), SMPLLayer(model))
    net.vertex_ids = vids
    net = net.to(DEV).train()
    assert net.n_markers == 6 and bool(net.shape_avg) == released and bool(net.do_fk) == released
    lens = torch.tensor([16, 11, 1], dtype=torch.int64, device=DEV)
    with torch.no_grad():
        _, _, jgt = R.estimated_markers(bm, tables, vids, torch.from_numpy(w['poses'].reshape(-1, 66)),
                                        torch.from_numpy(np.repeat(w['shapes'], F, axis=0)),
                                        torch.from_numpy(np.repeat(w['offset_r'], F, axis=0)),
                                        torch.from_numpy(np.repeat(w['offset_t'], F, axis=0)))
    masks = torch.ones(B, F, 12)
    masks[0, 2, 3] = 0.0      # a sensor the six do not include
    masks[0, 9, 0] = 0.0
    masks[1, 4:7, 7] = 0.0
    assert 3 not in net.marker_idxs and 0 in net.marker_idxs
    batch = MaskedBatch(w, lens, device=DEV)
    batch.marker_masks = masks.to(DEV)
    batch.joints_gt = jgt.reshape(B, F, -1).to(DEV).float()
    out = net(batch)
    assert net._engine is not None
    _, vals = net.backward(batch, out)
    torch.cuda.synchronize()
    T, nm = B * F, 6
    pos = batch.marker_pos_synth.cpu().reshape(T, 12, 3)[:, net.marker_idxs].reshape(T, 3 * nm)
    ori = batch.marker_ori_synth.cpu().reshape(T, 12, 9)[:, net.marker_idxs].reshape(T, 9 * nm)
    hist = lambda h, n: torch.stack([t.detach().cpu().float().reshape(T, n) for t in h])
    io = {'B': B, 'F': F, 'n_hist': N + 1, 'n_markers': nm, 'marker_idx': list(net.marker_idxs),
          'pose_hist': hist(net.pose_hat_history, 66), 'shape_hist': hist(net.shape_hat_history, 10),
          'markers_hist': hist(net.markers_hat_history, 36), 'markers_ori_hist': hist(net.markers_ori_hat_history, 108),
          'joints_final': net.joints_hat_history[-1].detach().cpu().float().reshape(T, 66),
          'pose_gt': batch.poses.cpu().reshape(T, 66), 'shape_gt': batch.shapes.cpu(),
          'joints_gt': batch.joints_gt.cpu().reshape(T, 66) if released else None,
          'inputs': torch.cat([pos, ori], dim=1), 'seq_lengths': lens.cpu(), 'marker_masks': masks.reshape(T, 12),
          'w_pose': net.pose_weight, 'w_shape': net.shape_weight, 'w_fk': net.fk_loss_weight if released else 0.0,
          'w_rec': net.r_weight}
    want = G.losses64(io)
    allow = G.losses_allowance(io, want)
    got = torch.tensor([vals[k] for k in G.LOSS_NAMES], dtype=torch.float64)
    print('engine losses', got.tolist(), want['loss_vals'].tolist())
    assert float(want['loss_vals'][2]) > 0 and (float(want['loss_vals'][3]) > 0) == released
    _hold('engine loss_vals', got.reshape(1, 5), want['loss_vals'].reshape(1, 5), allow['loss_vals'].reshape(1, 5))
