"""
Round 5 GPU tests (run with `-m gpu` on an MI355X).

  * the training step at the RELEASED width against fingerprints of the reference's own step
  * sampled-window parity at BASELINE configs[1]'s exact launch shape and across the T >= 16384 kernel switch (item 6)
"""
import os

import numpy as np
import pytest
import torch

from em_pose_amd import _lib, synthetic
from em_pose_amd.bodymodels.smpl import SMPLLayer
from em_pose_amd.helpers.configuration import CONSTANTS as CONST
from em_pose_amd.helpers.configuration import lgd_config
from em_pose_amd.nn.models import create_model
from oracle import torch_ref as R
from tests import helpers as H

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ATOL = 1e-4


def _load_fp(tag):
    z = np.load(os.path.join(H.GOLDEN, tag + '.npz'))
    return {k: z[k] for k in z.files}


@pytest.mark.parametrize('variant', ['default', 'epilogue_stats_side_streams', 'bn_kernels_one_stream'])
@pytest.mark.parametrize('tag', ['train_fp_lgdrnn12_n4_h512', 'train_fp_lgdrnn6_n2_h512'])
def test_full_width_training_step_matches_reference_fingerprints(tag, variant):
    """LGD-RNN-12 N=4 / LGD-RNN-6 N=2 with 2x512 update networks and a 2x512 LSTM, 12 windows x 32 frames (BASELINE
    configs[4]'s per-GPU batch), ragged lengths: the REFERENCE's train-mode forward + backward (models.py:485-688, with
    the in-forward deposits of :576) was run on these inputs and these weights (`tests.helpers.seeded_state_dict`, re-made
    here) and left, per parameter tensor, the max-abs, L2 norm, 8 seeded Gaussian projections and 256 seeded entries of
    its gradient, plus losses, outputs, BatchNorm running statistics -- and the SCATTER of each of those: the largest
    difference between any two of five fp32 realisations of the reference's own step (the recorded one and four draws
    with inputs and weights moved by one unit in the last place; N = 4 train-mode iterations amplify fp32 noise, the
    reference's FK loss alone moves by 2e-5 relative).  Tolerance rule of test_hip_parity.py:814:
    max(1e-4 of the tensor's scale, 4 x that scatter)."""
    from em_pose_amd.data.data import SyntheticBatch
    from em_pose_amd.nn.train_engine import LgdTrainEngine
    fp = _load_fp(tag)
    nm, N, seed = int(fp['meta/n_markers']), int(fp['meta/N']), int(fp['meta/seed'])
    lib = _lib.lib()
    saved = (LgdTrainEngine.two_streams_min_frames,)
    if variant == 'epilogue_stats_side_streams':      # what a 256-window step uses, forced onto these 384 frames
        _lib.check(lib.empose_set_option(b'train_epi', 2))
        LgdTrainEngine.two_streams_min_frames = 0
    elif variant == 'bn_kernels_one_stream':
        _lib.check(lib.empose_set_option(b'train_epi', 0))
        _lib.check(lib.empose_set_option(b'train_fused', 0))
        _lib.check(lib.empose_set_option(b'train_cols', 0))      # (default: the one-launch layers of train_cols.hip, paired)
    try:
        net = create_model(lgd_config(nm, True, N), SMPLLayer(H.small_model()))
        net.vertex_ids = [int(v) for v in fp['meta/vertex_ids']]
        missing, unexpected = net.load_state_dict(H.seeded_state_dict(net.state_dict(), seed), strict=False)
        assert not unexpected and all(k.startswith('smpl.') or k.endswith('num_batches_tracked') for k in missing)
        net = net.to(DEV).train()
        w = {k[3:]: v for k, v in fp.items() if k.startswith('in/')}
        batch = SyntheticBatch(w, torch.from_numpy(w['seq_lengths']).to(DEV), device=DEV)
        batch.joints_gt = torch.from_numpy(w['joints_gt']).to(DEV)
        net.zero_grad()
        out = net(batch)
        assert net._engine is not None
        if variant == 'epilogue_stats_side_streams':
            assert net._engine._use_side
        total, loss_vals = net.backward(batch, out)
        torch.cuda.synchronize()
    finally:
        LgdTrainEngine.two_streams_min_frames = saved[0]
    for k in ('pose_hat', 'root_ori_hat', 'shape_hat', 'joints_hat'):
        np.testing.assert_allclose(out[k].detach().cpu().numpy(), fp['out/' + k],
                                   atol=max(ATOL, 4.0 * float(fp['sens_out/' + k])), rtol=0, err_msg=k)
    for k in ('pose', 'shape', 'reconstruction', 'fk', 'total_loss'):
        assert loss_vals[k] == pytest.approx(float(fp['loss/' + k]), rel=1e-4, abs=max(1e-6, 4.0 * float(fp['sens_loss/' + k]))), k
    names = sorted({k.split('/')[1] for k in fp if k.startswith('grad/')})
    gmax = max(float(fp['grad/{}/max'.format(k)]) for k in names)
    params = dict(net.named_parameters())
    checked, worst, report, flips = 0, 0.0, [], []
    for k in names:
        g = params[k].grad
        assert g is not None, k
        mine = H.tensor_fingerprint(k, g)
        want = {f: fp['grad/{}/{}'.format(k, f)] for f in ('max', 'l2', 'n', 'proj', 'sample')}
        sens = {f: float(fp['sens/{}/{}'.format(k, f)]) for f in ('l2', 'proj', 'sample')}
        assert mine['n'] == int(want['n']), k
        scale = max(float(want['max']), 1e-4 * gmax)
        pre_bn_bias = k.endswith('.bias') and ('input_to_hidden' in k or '.layers.0.' in k or '.layers.4.' in k)
        if pre_bn_bias:      # mathematically zero in both implementations (a bias in front of a train-mode BatchNorm)
            assert mine['max'] < 1e-4 * gmax and float(want['max']) < 1e-4 * gmax, k
            continue
        # `sens` is a maximum over (10 pairs of realisations) x (entries compared): for a 256-entry sample that maximum sits
        # ~4.0 standard deviations out, for a single-element tensor (a PReLU slope: one sum over every activation of its
        # layer) only ~2.1 -- the same four-fold margin in standard deviations needs the ratio of the two as a factor
        n_e = min(mine['n'], H.N_SAMPLE)
        few = float(np.sqrt(np.log(10.0 * H.N_SAMPLE) / np.log(10.0 * n_e)))
        # (a one-element tensor's norm and its N_PROJ projections are that one element again, times constants: the same
        # single draw per pair of realisations, so the same factor -- round 6; the 8-projection factor understated it and the
        # footprint rule that used to wave single slopes through is gone)
        few_p = few if mine['n'] == 1 else float(np.sqrt(np.log(10.0 * H.N_SAMPLE) / np.log(10.0 * H.N_PROJ)))
        tol_e = max(1e-4 * scale, 4.0 * few * sens['sample'])
        tol_p = max(1e-4 * scale * np.sqrt(mine['n']), 4.0 * few_p * sens['proj'])
        tol_l = max(1e-4 * float(want['l2']), 4.0 * few_p * sens['l2'])
        e_s = float(np.abs(mine['sample'] - want['sample']).max())
        e_p = float(np.abs(mine['proj'] - want['proj']).max())
        e_l = abs(mine['l2'] - float(want['l2']))
        ratio = max(e_s / tol_e, e_p / tol_p, e_l / tol_l)
        # A PReLU branch flip: one activation of the 7.9 M of a step lies within rounding of zero and lands on the other side
        # (every change of a summation order moves a few; the reference's own five realisations differ by such flips too --
        # that is most of `sens`).  Its footprint is ONE entry of the per-column gradients of the BatchNorm in front of it, by
        # that element's cotangent -- not bounded by the scatter of five draws.  Round 6: accepted by PROOF, not by footprint
        # (tests/helpers.py::explain_by_prelu_flips): the fixture holds, per PReLU application of the reference's step, the
        # elements nearest to zero with their cotangents; the difference must be REPRODUCED -- entry, all projections, norm --
        # by one or two of those elements whose |z| lies within what the reference's own realisations move z by.
        if ratio > 1.0:
            slope_name = H.prelu_of_batch_norm(k.rsplit('.', 1)[0]) + '.weight' if (
                'batch_norm' in k or any(('.layers.%d.' % i) in k for i in (1, 5))) else None
            proof = None
            if slope_name is not None:
                proof = H.explain_by_prelu_flips(fp, k, g.detach().cpu().numpy(), want, tol_e, tol_p, tol_l,
                                                 float(params[slope_name].detach().cpu()))
            if proof is not None:
                flips.append((k, round(ratio, 2), [(c, r_, col, '%.1e' % z, '%.2e' % pr) for c, r_, col, z, pr in proof]))
                ratio = 0.0
        report.append((ratio, k, e_s, tol_e, e_p, tol_p, e_l, tol_l, scale, sens['sample']))
        worst = max(worst, report[-1][0])
        checked += 1
    report.sort(reverse=True)
    for r in report[:6]:
        print('  %5.2f %-52s entries %.2e / %.2e  proj %.2e / %.2e  l2 %.2e / %.2e  (scale %.2e, sens %.2e)' % r)
    bad = [r[1] for r in report if r[0] > 1.0]
    assert not bad, bad
    assert len(flips) <= 3, flips        # (of 56 tensors)
    if flips:
        print('  PReLU branch flips, each PROVEN by a recorded near-zero element (call, row, column, z, predicted difference): %s' % flips)
    assert checked >= 40, checked
    print('%s [%s]: %d gradient fingerprints, worst error / tolerance %.3f' % (tag, variant, checked, worst))
    for k, v in net.state_dict().items():
        if 'running_' in k:
            np.testing.assert_allclose(v.cpu().numpy(), fp['after/' + k], rtol=0, err_msg=k,
                                       atol=max(1e-5, 4.0 * float(fp['sens_after/' + k])))



# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def big_model():
    return synthetic.make_model()


def _randomize_bn(net, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=g) * 0.1)
                m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) + 0.5)


@pytest.mark.parametrize('B', [256, 512])
def test_config1_launch_shape_sampled_windows_vs_oracle(big_model, B):
    """BASELINE configs[1] at its own launch shape: LGD-12 WITHOUT the RNN (MLP init networks, reference models.py:517-526),
    N = 4, 2 x 512 MLPs, B = 256 windows x 32 frames = 8192 rows, V = 6890: fused update-network kernel + the general SMPL
    kernels + MLP init.  B = 512 crosses the T >= 16384 switch to the frame-per-lane SMPL kernels (api_model.hip) with MLP init.
    Eight windows sampled across workgroup boundaries against the oracle run on those windows alone."""
    torch.manual_seed(1614785570)
    net = create_model(lgd_config(12, False, 4), SMPLLayer(big_model))
    _randomize_bn(net, 1614785571)
    net = net.eval()
    bm = R.BodyModelTensors(big_model)
    tables = R.sensor_tables(big_model['f'], CONST.VERTEX_IDS)

    def fn(poses, betas, o_r, o_t):
        with torch.no_grad():
            p, o, _ = R.estimated_markers(bm, tables, CONST.VERTEX_IDS, torch.from_numpy(poses),
                                          torch.from_numpy(betas), torch.from_numpy(o_r), torch.from_numpy(o_t))
        return p.numpy(), o.numpy()
    F = 32
    pool = synthetic.make_windows(64, F, 2121, fn)
    pick = [0, 1, 3, 4, 127, 128, B // 2 + 1, B - 1]          # 128 rows = 4 windows per row block of the fused kernel
    keys = ('marker_pos', 'marker_oris', 'offset_t', 'offset_r')
    order = np.random.default_rng(B).permutation(B) % 64
    batch = {k: np.ascontiguousarray(pool[k][order]) for k in keys}
    sd = {k: v for k, v in net.state_dict().items() if not k.startswith('smpl.')}
    inp = {k: torch.from_numpy(batch[k][pick]) for k in keys}
    inp['marker_masks'] = None
    inp['seq_lengths'] = torch.full((len(pick),), F, dtype=torch.int64)
    want, _ = R.ief_forward(sd, bm, tables, CONST.VERTEX_IDS, inp, n_markers=12, N=4, rnn_init=False)
    net = net.to(DEV)
    res = net.forward_tensors(*(torch.from_numpy(batch[k]).to(DEV) for k in keys))
    torch.cuda.synchronize()
    pose = res['pose'][pick].cpu().numpy()
    np.testing.assert_allclose(pose[:, :, 3:], want['pose_hat'].numpy(), atol=ATOL)
    np.testing.assert_allclose(pose[:, :, :3], want['root_ori_hat'].numpy(), atol=ATOL)
    np.testing.assert_allclose(res['shape'][pick].cpu().numpy(), want['shape_hat'].numpy(), atol=ATOL)
    np.testing.assert_allclose(res['joints'][pick].cpu().numpy(), want['joints_hat'].numpy(), atol=ATOL)


# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('scale', [1.0, 30.0], ids=['unit_inputs', 'gradient_scale_inputs'])
def test_three_piece_bf16_update_nets_are_as_accurate_as_the_fp32_mfma_ones(scale):
    """mlp_fused_x3.hip forms every fp32 product from three bf16 pieces per operand (six bf16 MFMA products, fp32
    accumulation).  Claim: fp32-EQUIVALENT -- against a float64 evaluation of the same released-width networks (2 x 512,
    296 inputs, 66 / 10 outputs, random BatchNorm statistics) its error is no larger than that of the kernel built on the
    fp32 MFMA instruction (mlp_fused.hip), for O(1) inputs and for inputs at the scale of the gradient features (O(30)).
    Also: repeated launches are bit-identical (one wave per SIMD; scripts/dev/bf16_hazard_repro.md)."""
    T = 16384 + 64 + 7
    torch.manual_seed(11)
    net = create_model(lgd_config(12, False, 1), SMPLLayer(H.small_model()))
    _randomize_bn(net, 12)
    net.vertex_ids = synthetic.small_vertex_ids(160)
    net = net.to(DEV).eval()
    sd64 = {k: v.detach().cpu().double() for k, v in net.state_dict().items() if not k.startswith('smpl.')}
    g = torch.Generator().manual_seed(2)
    x = torch.randn(T, 296, generator=g) * scale
    rows = [0, 1, 63, 64, 8191, 16383, 16384, T - 1]
    with torch.no_grad():
        want_p = R.mlp_forward(sd64, 'pose_net_iter.', x[rows].double()).numpy()
        want_s = R.mlp_forward(sd64, 'shape_net_iter.', x[rows].double()).numpy()
    lib = _lib.lib()
    handle = net._ensure_handle(torch.device(DEV))
    xg = x.to(DEV)
    err, outs = {}, {}
    for x3 in (0, 1):
        _lib.check(lib.empose_set_option(b'mlp_x3', x3))
        reps = []
        for rep in range(3 if x3 else 1):
            dp, ds = torch.full((T, 66), 7.0, device=DEV), torch.full((T, 10), 7.0, device=DEV)
            nbytes = lib.empose_update_workspace_bytes(handle, T)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
            _lib.check(lib.empose_update_nets_fwd(handle, T, _lib.dptr(xg), 296, _lib.dptr(dp), _lib.dptr(ds), _lib.dptr(ws),
                                                  nbytes, _lib.current_stream()))
            torch.cuda.synchronize()
            reps.append((dp.cpu().numpy(), ds.cpu().numpy()))
        for r in reps[1:]:
            assert np.array_equal(r[0], reps[0][0]) and np.array_equal(r[1], reps[0][1])
        outs[x3] = reps[0]
        err[x3] = max(np.abs(reps[0][0][rows] - want_p).max(), np.abs(reps[0][1][rows] - want_s).max())
    out_scale = max(np.abs(want_p).max(), np.abs(want_s).max())
    print('update nets vs float64 (|out| <= %.2f): fp32 MFMA %.2e, three-piece bf16 %.2e; between them %.2e'
          % (out_scale, err[0], err[1], np.abs(outs[0][0] - outs[1][0]).max()))
    assert err[1] <= 1.5 * err[0] + 1e-7 * out_scale, err
    assert err[1] < 2e-5 * max(1.0, out_scale)
    assert np.abs(outs[0][0] - outs[1][0]).max() < 1e-4 * max(1.0, out_scale)


@pytest.mark.parametrize('B,F,In,Hd,L', [(1024, 8, 144, 512, 2), (300, 7, 72, 512, 2), (333, 5, 200, 192, 3), (257, 4, 144, 64, 1),
                                         (1000, 3, 36, 128, 4),
                                         # round 6, 17 .. 256 rows: lstm_mid_x3.hip (one / two row tiles, several row blocks)
                                         (36, 9, 72, 512, 2), (17, 5, 144, 512, 2), (32, 4, 144, 256, 2), (33, 3, 72, 64, 1),
                                         (100, 4, 144, 128, 3), (256, 3, 36, 512, 2)])
def test_three_piece_bf16_lstm_steps_are_as_accurate_as_the_fp32_mfma_ones(B, F, In, Hd, L):
    """lstm_x3.hip (the wavefront step of batches above 256 rows: weights and hidden states as three bf16 pieces in
    fragment order, six bf16 MFMA products per fp32 product, K split over the waves) against a float64 LSTM
    (reference nn/layers.py:133-157 semantics: ragged rows, carried state, zero-padded outputs): its error is no larger
    than that of the fp32-MFMA step kernel, outputs and final state; repeated runs are bit-identical."""
    from em_pose_amd.nn.layers import RNNLayer
    torch.manual_seed(B + F)
    layer = RNNLayer(In, Hd, L).eval()
    with torch.no_grad():
        for p in layer.lstm.parameters():
            p.mul_(2.0)
    x = torch.randn(B, F, In)
    lens = torch.randint(1, F + 1, (B,))
    lens[0], lens[-1] = F, 1
    h0, c0 = 0.5 * torch.randn(L, B, Hd), 0.5 * torch.randn(L, B, Hd)
    sd64 = {'lstm.' + k: v.detach().double() for k, v in layer.lstm.state_dict().items()}
    with torch.no_grad():
        want = {st is not None: R.lstm_forward(sd64, 'lstm.', x.double(), lens, None if st is None else (h0.double(), c0.double()),
                                               L, False) for st in (None, 1)}
    g = layer.to(DEV)
    err = {}
    lib = _lib.lib()
    for x3 in (0, 1, 2):       # 1 (the default): lstm_x3.hip, K-split waves; 2 (round 6, opt-in): lstm_rows_x3.hip, row-split waves
        _lib.check(lib.empose_set_option(b'lstm_x3', x3))
        worst, first = 0.0, None
        for rep in range(3 if x3 else 1):
            outs = []
            for carried in (False, True):
                g.init_state = (h0.to(DEV), c0.to(DEV)) if carried else None
                y = g(x.to(DEV), lens.to(DEV))
                torch.cuda.synchronize()
                wy, (wh, wc) = want[carried]
                got = (y.cpu(), g.final_state[0].cpu(), g.final_state[1].cpu())
                outs += [t.numpy() for t in got]
                worst = max(worst, float((got[0].double() - wy).abs().max()), float((got[1].double() - wh).abs().max()),
                            float((got[2].double() - wc).abs().max()))
            if first is None:
                first = outs
            else:
                for a_, b_ in zip(first, outs):
                    assert np.array_equal(a_, b_)
        err[x3] = worst
    print('lstm %s vs float64: fp32 MFMA %.2e, three-piece bf16 %.2e (K-split waves) %.2e (row-split waves)'
          % ((B, F, In, Hd, L), err[0], err[1], err[2]))
    assert err[1] <= 1.5 * err[0] + 2e-7 and err[1] < 1e-5
    assert err[2] <= 1.5 * err[0] + 2e-7 and err[2] < 1e-5
    g.release()


# ----------------------------------------------------------------------------------------------------------------------
# One-launch train-mode layers (csrc/train_cols.hip)
def _mlp_pair(in_dim, hidden, seed):
    from em_pose_amd.nn.layers import MLP
    torch.manual_seed(seed)
    nets = [MLP(in_dim, 66, hidden, num_layers=2), MLP(in_dim, 10, hidden, num_layers=2)]
    g = torch.Generator().manual_seed(seed + 1)
    for net in nets:
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                with torch.no_grad():
                    m.bias.copy_(0.3 * torch.randn(m.bias.shape, generator=g))
                    m.running_mean.copy_(0.1 * torch.randn(m.running_mean.shape, generator=g))
                    m.running_var.copy_(0.5 + torch.rand(m.running_var.shape, generator=g))
            if isinstance(m, torch.nn.PReLU):
                with torch.no_grad():
                    m.weight.fill_(0.1 + 0.3 * float(torch.rand(1, generator=g)))
    return [n.to(DEV).train() for n in nets]


def _run_mlp_train(nets, x, d_outs, M, pair, deferred=True, saves_from=None, after_forward=None, accumulate=0,
                   grads_init=None):
    """forward + reverse sweep of both networks through the C ABI; returns everything they write.  `saves_from`: the
    reverse sweep reads these saved activations instead of its own forward's (same PReLU branch decisions for two
    reverse paths under comparison: an activation within rounding of zero flips one element's branch otherwise).
    `after_forward`: called between the forward and the reverse sweep (tests/test_train_mlp_layout.py flips options there).
    `accumulate`, `grads_init`: the reverse sweep adds to these gradient tensors (per network, in the order of
    `_MlpView.parameter_list`) instead of writing into zeroed ones (tests/test_train_mlp_elementwise.py)."""
    import ctypes as C
    from em_pose_amd.nn.train_engine import _MlpView
    lib = _lib.lib()
    stream = _lib.current_stream()
    views = [_MlpView(n) for n in nets]
    for v in views:
        v.fix_layout(lib, M)
        v.pack_forward_x3(lib, stream, M)     # (round 6: three-piece copies of the weights for large M, option train_x3)
        # (paired call: as the engine prepares it -- no transposed copies when the reverse reads W itself; the single-network
        # calls get the copies: the same operand values through the other load path, so the two stay bit-identical)
        v.prepare_backward(lib, stream, M if pair else None)
    ps = [v.params() for v in views]
    ldx = x.shape[1]
    outs = [torch.zeros(M, 66, device=DEV), torch.zeros(M, 10, device=DEV)]
    saves = [torch.zeros(lib.empose_mlp_train_save_floats(C.byref(p), M), device=DEV) for p in ps]
    nbytes = max(lib.empose_mlp_train_pair_workspace_bytes(C.byref(ps[0]), C.byref(ps[1]), M), 16)
    ws = torch.empty(nbytes // 4 + 4, device=DEV)
    grads = [[torch.zeros_like(p) for p in v.parameter_list()] for v in views] if grads_init is None else grads_init
    gs = [v.grads(g) for v, g in zip(views, grads)]
    stashes = [torch.zeros(lib.empose_mlp_train_stash_floats(C.byref(p), M), device=DEV) for p in ps]
    lds = [d.shape[1] for d in d_outs]
    if pair:
        _lib.check(lib.empose_mlp_train_fwd_pair(C.byref(ps[0]), C.byref(ps[1]), M, _lib.dptr(x), ldx, _lib.dptr(outs[0]), 66,
                                                 _lib.dptr(outs[1]), 10, _lib.dptr(saves[0]), _lib.dptr(saves[1]),
                                                 _lib.dptr(ws), nbytes, stream))
        if after_forward is not None:
            after_forward()
        if saves_from is not None:
            fwd_saves = [t.clone() for t in saves]
            for t, src in zip(saves, saves_from):
                t.copy_(src)
        _lib.check(lib.empose_mlp_train_bwd_deferred_pair(
            C.byref(ps[0]), C.byref(ps[1]), M, _lib.dptr(x), ldx, _lib.dptr(d_outs[0]), lds[0], _lib.dptr(d_outs[1]), lds[1],
            _lib.dptr(saves[0]), _lib.dptr(saves[1]), C.byref(gs[0]), C.byref(gs[1]), accumulate, _lib.dptr(stashes[0]),
            _lib.dptr(stashes[1]), _lib.dptr(ws), nbytes, stream))
    else:
        for i in (0, 1):
            _lib.check(lib.empose_mlp_train_fwd(C.byref(ps[i]), M, _lib.dptr(x), ldx, _lib.dptr(outs[i]), outs[i].shape[1],
                                                _lib.dptr(saves[i]), _lib.dptr(ws), nbytes, stream))
        if after_forward is not None:
            after_forward()
        if saves_from is not None:
            fwd_saves = [t.clone() for t in saves]
            for t, src in zip(saves, saves_from):
                t.copy_(src)
        for i in (0, 1):
            if deferred:
                _lib.check(lib.empose_mlp_train_bwd_deferred(C.byref(ps[i]), M, _lib.dptr(x), ldx, _lib.dptr(d_outs[i]), lds[i],
                                                             _lib.dptr(saves[i]), C.byref(gs[i]), accumulate, _lib.dptr(stashes[i]),
                                                             _lib.dptr(ws), nbytes, stream))
            else:
                _lib.check(lib.empose_mlp_train_bwd(C.byref(ps[i]), M, _lib.dptr(x), ldx, _lib.dptr(d_outs[i]), lds[i],
                                                    _lib.dptr(saves[i]), C.byref(gs[i]), accumulate, _lib.dptr(ws), nbytes, stream))
    torch.cuda.synchronize()
    _lib.check(lib.empose_async_status())
    res = {'out': outs, 'save': saves if saves_from is None else fwd_saves, 'stash': stashes, 'grads': grads, 'views': views}
    res['bn'] = [[t.clone() for k, t in n.state_dict().items() if 'running_' in k or 'num_batches' in k] for n in nets]
    return res


@pytest.mark.parametrize('M,in_dim,hidden', [(384, 296, 512), (512, 296, 512), (100, 296, 512), (17, 152, 64),
                                             (48, 296, 32), (1, 152, 64)])
def test_one_launch_train_layers_equal_the_layer_by_layer_path(M, in_dim, hidden):
    """Training at up to 512 rows (the reference's 12 windows x 32 frames = 384): a layer's product + bias + train-mode
    BatchNorm + PReLU of BOTH update networks as one launch, forward and backward, its column statistics exchanged between
    the four row parts through tagged words (csrc/train_cols.hip, reference nn/layers.py:13-77 in training mode) -- against
    the product + BatchNorm launches of each network (option train_cols = 0): outputs, saved z / a / mean / rstd, running
    statistics, the layer cotangents and the BatchNorm / PReLU gradients, to rounding (another summation order; the batch
    variance by a pairwise update of the parts' centred sums).  The paired call and the two single-network calls run the
    same launches: bit-identical."""
    lib = _lib.lib()
    g = torch.Generator().manual_seed(M + hidden)
    def guarded(t):     # the array followed by NaNs: a read past its end (a lane of a ragged last k-block) poisons the result
        buf = torch.full((t.numel() + 256,), float('nan'), device=DEV)
        buf[:t.numel()] = t.reshape(-1).to(DEV)
        return buf[:t.numel()].view(t.shape)
    x = guarded(torch.randn(M, in_dim, generator=g))
    d_outs = [torch.zeros(M, 68), torch.zeros(M, 12)]
    d_outs[0][:, :66] = torch.randn(M, 66, generator=g)
    d_outs[1][:, :10] = torch.randn(M, 10, generator=g)
    d_outs = [guarded(d) for d in d_outs]
    res = {}
    for key, cols, pair, deferred in (('passes', 0, False, True), ('single', 1, False, True), ('pair', 1, True, True),
                                      ('passes_now', 0, False, False), ('single_now', 1, False, False)):
        nets = _mlp_pair(in_dim, hidden, 5)
        _lib.check(lib.empose_set_option(b'train_cols', cols))
        try:
            res[key] = _run_mlp_train(nets, x, d_outs, M, pair, deferred,
                                      saves_from=None if key == 'passes' else res['passes']['save'])
        finally:
            _lib.check(lib.empose_set_option(b'train_cols', 1))
    def flat(r, deferred=True):
        out = list(r['out']) + list(r['save']) + [t for b in r['bn'] for t in b]
        out += [t for gl in r['grads'] for t in gl]
        return out + (list(r['stash']) if deferred else [])
    for a, b in zip(flat(res['single']), flat(res['pair'])):
        assert torch.equal(a, b)
    if M == 1:       # one row: var = 0, rstd = 1 / sqrt(eps) amplifies rounding by 316 -- finite and paired == single is the check
        assert all(torch.isfinite(t).all() for t in flat(res['single']))
        return
    worst = 0.0
    for (want, got, deferred) in ((res['passes'], res['single'], True), (res['passes_now'], res['single_now'], False)):
        for idx, (a, b) in enumerate(zip(flat(want, deferred), flat(got, deferred))):
            assert torch.isfinite(b.float()).all()
            scale = max(1.0, float(a.abs().max()))
            err = float((a.double() - b.double()).abs().max()) / scale
            worst = max(worst, err)
            # (a bias in front of a train-mode BatchNorm has a mathematically zero gradient: both values are round-off of
            # sums of M terms)
            assert err < (1e-4 if a.ndim == 1 and a.numel() == hidden else 2e-5), (err, idx, a.shape, deferred)
    # the deferred sweeps left the weight gradients alone; the immediate ones formed them
    n_w = sum(float(t.abs().sum()) for t in res['single']['grads'][0][0:1])
    assert n_w == 0.0 and float(res['single_now']['grads'][0][0].abs().sum()) > 0.0
    print('one-launch layers M=%d %d->%d: worst relative difference to the layer-by-layer path %.2e' % (M, in_dim, hidden, worst))


# ----------------------------------------------------------------------------------------------------------------------
# LSTM steps of a few rows (csrc/lstm_fewrows.hip, lstm_fewrows_kernel; csrc/gemm_rec.hip, rec_fewrows_reg_kernel)
@pytest.mark.parametrize('B,F,In,H,L,bi', [(12, 32, 144, 512, 2, False), (4, 9, 60, 512, 2, False), (16, 7, 72, 64, 3, False),
                                          (6, 11, 60, 128, 2, True), (9, 5, 144, 256, 1, False)])
def test_lstm_steps_of_a_few_rows_equal_the_small_batch_kernels(B, F, In, H, L, bi):
    """From 4 to 16 rows a step is a launch of lstm_fewrows_kernel (a workgroup owns two hidden units, its 256 threads split
    K, the lanes' sums meet by a reduce-scatter): against the kernels it replaces there (lstm_small_kernel / the
    whole-sequence kernel, option lstm_fewrows = 0) -- outputs and final state, ragged rows, carried state over two chunks,
    both directions; another summation order, so to rounding.  Reference: nn/layers.py:133-157."""
    from em_pose_amd.nn.layers import RNNLayer
    torch.manual_seed(B + H)
    layer = RNNLayer(In, H, L, bidirectional=bi).eval()
    x = torch.randn(B, 2 * F, In)
    lens = torch.randint(1, 2 * F + 1, (B,))
    lens[0] = 2 * F
    res = {}
    for mode in (1, 0):
        _lib.check(_lib.lib().empose_set_option(b'lstm_fewrows', mode))
        g = layer.to(DEV)
        g.init_state = None
        outs = []
        for chunk in range(1 if bi else 2):
            sl = slice(chunk * F, (chunk + 1) * F) if not bi else slice(0, 2 * F)
            ln = (lens - chunk * F).clamp(1, F) if not bi else lens
            y = g(x[:, sl].contiguous().to(DEV), ln.to(DEV))
            if not bi:
                g.init_state = g.final_state
            outs += [y.cpu()] + ([g.final_state[0].cpu(), g.final_state[1].cpu()] if not bi else [])
        res[mode] = outs
        layer = g.cpu()
    _lib.check(_lib.lib().empose_set_option(b'lstm_fewrows', 1))
    worst = 0.0
    for a, b in zip(res[1], res[0]):
        assert torch.isfinite(a).all()
        worst = max(worst, float((a - b).abs().max()))
    assert worst < 2e-6, worst
    assert any(not torch.equal(a, b) for a, b in zip(res[1], res[0])) or H < 128    # (it IS another kernel)
    layer.release()


def test_lstm_training_forward_of_a_few_rows_and_its_reverse_equal_the_small_batch_kernels():
    """The training forward at the reference's batch (12 windows) on lstm_fewrows_kernel -- gates, cell states and incoming
    hidden states saved for the reverse sweep -- and the reverse recurrences on rec_fewrows_reg_kernel (K split over the
    waves, operands in registers): outputs, final state and every gradient against torch.nn.LSTM in float64."""
    from em_pose_amd.nn.layers import _LstmTrainFn
    torch.manual_seed(12)
    B, F, K, H, L = 12, 32, 144, 512, 2
    x = torch.randn(B, F, K, device=DEV)
    lens = torch.randint(1, F + 1, (B,), dtype=torch.int32)
    lens[3] = F
    h0, c0 = 0.5 * torch.randn(L, B, H, device=DEV), 0.5 * torch.randn(L, B, H, device=DEV)
    dy = torch.randn(B, F, H, device=DEV)
    ws = [0.05 * torch.randn(*shape, device=DEV) for l in range(L)
          for shape in ((4 * H, K if l == 0 else H), (4 * H, H), (4 * H,), (4 * H,))]
    wg = [w.clone().requires_grad_(True) for w in ws]
    xg = x.clone().requires_grad_(True)
    y, h_n, c_n = _LstmTrainFn.apply(xg, lens.to(DEV), h0, c0, L, *wg)
    (y * dy).sum().backward()
    torch.cuda.synchronize()
    got = [y.detach(), h_n, c_n, xg.grad] + [w.grad for w in wg]
    ref = torch.nn.LSTM(K, H, L, batch_first=True).double()
    with torch.no_grad():
        for l in range(L):
            for name, w in zip(('weight_ih_l%d', 'weight_hh_l%d', 'bias_ih_l%d', 'bias_hh_l%d'), ws[4 * l:4 * l + 4]):
                getattr(ref, name % l).copy_(w.double().cpu())
    xr = x.double().cpu().requires_grad_(True)
    packed = torch.nn.utils.rnn.pack_padded_sequence(xr, lens.long(), batch_first=True, enforce_sorted=False)
    out, (hn, cn) = ref(packed, (h0.double().cpu(), c0.double().cpu()))
    yr, _ = torch.nn.utils.rnn.pad_packed_sequence(out, batch_first=True, total_length=F)
    (yr * dy.double().cpu()).sum().backward()
    want = [yr.detach(), hn, cn, xr.grad] + [getattr(ref, n % l).grad for l in range(L)
                                             for n in ('weight_ih_l%d', 'weight_hh_l%d', 'bias_ih_l%d', 'bias_hh_l%d')]
    for a, b in zip(got, want):
        scale = max(1.0, float(b.abs().max()))
        assert float((a.double().cpu() - b).abs().max()) < 2e-5 * scale


@pytest.mark.provokes_poll_timeout
def test_mailbox_poll_of_the_one_launch_layers_gives_up_loudly():
    """spin_limit = 1: a row part that does not find the other parts' statistics at its first re-check gives up -- the call
    returns normally (the failure happens on the device), the outputs are poisoned with NaN, empose_async_status() reports
    EMPOSE_ETIMEOUT exactly then; with the normal limit the same call gives finite numbers again.  Nothing hangs."""
    lib = _lib.lib()
    M, in_dim, hidden = 384, 296, 512
    g = torch.Generator().manual_seed(3)
    x = torch.randn(M, in_dim, generator=g).to(DEV)
    d_outs = [torch.zeros(M, 68, device=DEV), torch.zeros(M, 12, device=DEV)]
    d_outs[0][:, :66] = torch.randn(M, 66, generator=g).to(DEV)
    d_outs[1][:, :10] = torch.randn(M, 10, generator=g).to(DEV)
    assert lib.empose_async_status() == 0
    timed_out = 0
    for attempt in range(12):
        nets = _mlp_pair(in_dim, hidden, 5)
        _lib.check(lib.empose_set_option(b'spin_limit', 1))
        try:
            res = _run_mlp_train(nets, x, d_outs, M, pair=True)
            status = 0
        except _lib.EmposeError as e:          # (_run_mlp_train checks the status after synchronising)
            assert 'error -4' in str(e) and 'timed out' in str(e)
            status = -4
        finally:
            _lib.check(lib.empose_set_option(b'spin_limit', 0))
        if status == -4:
            timed_out += 1
            assert lib.empose_async_status() == 0          # reported once
        else:
            assert all(torch.isfinite(t).all() for t in res['out'])
        if timed_out >= 2:
            break
    assert timed_out >= 1, 'spin_limit = 1 never made a mailbox poll give up: the test does not exercise the path'
    nets = _mlp_pair(in_dim, hidden, 5)
    res = _run_mlp_train(nets, x, d_outs, M, pair=True)       # back to normal
    assert all(torch.isfinite(t).all() for t in res['out'] + res['stash'])
