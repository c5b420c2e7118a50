"""
GPU tests: every element of everything the two update MLPs write in training mode (csrc/api_train.hip:
empose_mlp_train_fwd / _fwd_pair / _bwd / _bwd_deferred / _bwd_deferred_pair / _wgrad, through the C ABI) against float64,
each within its own derived allowance (tests/elementwise.py: mlp_train_fwd_reference, mlp_train_bwd_reference,
mlp_train_wgrad_reference; gamma = GAMMA_GEMM, u = 2^-24, elementwise roundings one unit in the last place each).  The
allowances themselves are tested without a GPU in tests/test_train_mlp_bounds.py.

Forward: every saved plane and statistic from the saved quantities the kernel computed it from (the pre-activation plane
from the saved activation below, mean / rstd from the saved plane, s / t from the saved statistics, a from both), both
outputs, the running statistics from their values before the call, num_batches_tracked + 1.
Reverse: the float64 sweep from that forward's own save buffer and d_out: the stash slots (deferred), every gradient.
Both networks are the 66- and 10-output pair of tests/test_hip_round5.py::_mlp_pair (num_layers = 2: six dense layers,
five of them hidden); x and d_out are followed by NaNs in memory, the padding columns of d_out are zero.

A case's id names the save layout and the launch family, and the case asserts both through
empose_mlp_train_save_layout and empose_mlp_train_uses_weight_t (0: the one-launch layers of train_cols.hip):
  cols     defaults, M <= 512: layout 1 on the one-launch layers.  pair: one call for both networks, W read by rows (no
           transposed copies); single: a call per network with the caller's W^T.  M = 2, 17: empty and ragged row parts;
           512: eight full 16-row tiles per part; 384 x 296 x 512 paired is the reference batch.
  passes   train_cols = train_fused = train_epi = 0: layout 1, GEMM + bn_prelu_*_kernel<R>, R = 4 / 8 / 12 / 16 / 24 / 32 at
           M = 100 / 200 / 384 / 512 / 700 / 1024; M = 1064: the three-pass BatchNorm kernels (9 row splits, the last of 40
           rows); hidden 96: a ragged 64-column block.
  fused    train_fused = 2: layout 2, the weight gradients read the re-formed a.
  epi      train_epi = 2 (100 rows) or the default (1064 rows): layout 3; train_x3 = 1: the view packed weight_x3 and
           weight_t_x3, so the hidden products are gemm_train_x3_kernel (the paired entry points: a view packs the transposed
           pieces only when it is prepared for a row count, and two networks of 1064 rows run one after the other there).
  shifted  x + 3: columns of layer 0 with |mean| of several standard deviations (the shifted one-pass variance of
           bn_stats_fwd_kernel at M = 1064, the uncentred reverse form of layout 3).
Weight gradients: `now` formed by the reverse sweep; `wgrad1` deferred + empose_mlp_train_wgrad over one application;
`wgrad2` over two different (x, d_out) applications of the same network -- one segmented product at M = 384 (M % 32 == 0),
one product per application, added, at M = 100; `acc`: accumulate = 1 onto random non-zero gradients.

Measured on the MI355X: worst err / allowance over all elements of both networks, per case and tensor group: planes (pre,
a, out) | statistics (mean, rstd, s, t, running) | dZ | dW | db | dgamma, dbeta, dslope; `control`: the float32 torch
evaluation on the CPU (tests/test_train_mlp_bounds.py) at the same shape and layout, same grouping.
    case                                                       on the GPU                                control (CPU, float32 torch)
    layout1_cols_pair_384x296x512_wgrad2                       0.31 | 0.38 | 0.18 | 0.12 | 0.06 | 0.07   0.41 | 0.35 | 0.17 | 0.10 | 0.07 | 0.09
    layout1_cols_single_100x296x512_wgrad2                     0.29 | 0.47 | 0.16 | 0.33 | 0.10 | 0.13   0.40 | 0.36 | 0.17 | 0.20 | 0.09 | 0.10
    layout1_cols_pair_2x152x64_wgrad1                          0.19 | 0.33 | 0.02 | 0.21 | 0.12 | 0.08   0.22 | 0.37 | 0.03 | 0.21 | 0.12 | 0.12
    layout1_cols_single_2x152x64_now                           0.19 | 0.33 | 0.00 | 0.21 | 0.12 | 0.08   0.22 | 0.37 | 0.03 | 0.21 | 0.12 | 0.12
    layout1_cols_pair_17x152x64_wgrad1_acc                     0.24 | 0.40 | 0.08 | 0.41 | 0.16 | 0.13   0.29 | 0.42 | 0.14 | 0.37 | 0.14 | 0.13
    layout1_cols_single_17x152x64_now_acc                      0.24 | 0.40 | 0.00 | 0.41 | 0.16 | 0.13   0.29 | 0.42 | 0.14 | 0.37 | 0.14 | 0.13
    layout1_cols_pair_512x152x64_wgrad1                        0.29 | 0.35 | 0.12 | 0.13 | 0.05 | 0.05   0.39 | 0.33 | 0.14 | 0.09 | 0.05 | 0.05
    layout1_cols_single_512x152x64_now                         0.29 | 0.35 | 0.00 | 0.13 | 0.05 | 0.05   0.39 | 0.33 | 0.14 | 0.09 | 0.05 | 0.05
    layout1_passes_100x152x64_now                              0.69 | 0.42 | 0.00 | 0.34 | 0.12 | 0.12   0.35 | 0.35 | 0.13 | 0.15 | 0.06 | 0.08
    layout1_passes_200x152x64_wgrad1                           0.72 | 0.43 | 0.17 | 0.21 | 0.10 | 0.10   0.35 | 0.34 | 0.12 | 0.11 | 0.07 | 0.07
    layout1_passes_384x152x64_now                              0.78 | 0.57 | 0.00 | 0.13 | 0.06 | 0.06   0.36 | 0.32 | 0.15 | 0.08 | 0.05 | 0.05
    layout1_passes_512x152x64_wgrad1                           0.30 | 0.47 | 0.14 | 0.10 | 0.06 | 0.06   0.39 | 0.33 | 0.14 | 0.09 | 0.05 | 0.05
    layout1_passes_700x152x64_now                              0.70 | 0.51 | 0.00 | 0.13 | 0.04 | 0.07   0.35 | 0.34 | 0.15 | 0.08 | 0.04 | 0.06
    layout1_passes_1024x152x64_wgrad1                          0.30 | 0.45 | 0.15 | 0.09 | 0.06 | 0.06   0.37 | 0.34 | 0.16 | 0.07 | 0.04 | 0.05
    layout1_passes_three_pass_bn_1064x152x64_now               0.31 | 0.35 | 0.00 | 0.09 | 0.04 | 0.05   0.39 | 0.38 | 0.16 | 0.07 | 0.05 | 0.05
    layout1_passes_100x152x96_wgrad1                           0.69 | 0.44 | 0.12 | 0.50 | 0.08 | 0.11   0.39 | 0.36 | 0.13 | 0.16 | 0.09 | 0.09
    layout1_passes_three_pass_bn_1064x152x96_now               0.30 | 0.40 | 0.00 | 0.11 | 0.05 | 0.05   0.38 | 0.37 | 0.16 | 0.08 | 0.05 | 0.05
    layout2_fused_100x152x64_wgrad2_acc                        0.66 | 0.48 | 0.17 | 0.60 | 0.07 | 0.09   0.20 | 0.46 | 0.13 | 0.13 | 0.06 | 0.08
    layout2_fused_384x296x512_wgrad2_acc                       0.75 | 0.49 | 0.38 | 0.45 | 0.10 | 0.10   0.12 | 0.49 | 0.17 | 0.10 | 0.07 | 0.09
    layout3_epi_100x152x64_now                                 0.59 | 0.46 | 0.00 | 0.40 | 0.08 | 0.09   0.46 | 0.46 | 0.13 | 0.15 | 0.06 | 0.08
    layout3_epi_1064x152x256_x3_0_now                          0.79 | 0.49 | 0.00 | 0.12 | 0.07 | 0.07   0.49 | 0.49 | 0.16 | 0.07 | 0.04 | 0.05
    layout3_epi_pair_1064x152x256_x3_1_wgrad1                  0.68 | 0.50 | 0.22 | 0.11 | 0.09 | 0.09   0.49 | 0.49 | 0.16 | 0.07 | 0.04 | 0.05
    layout1_passes_three_pass_bn_1064x152x64_shifted_wgrad1    0.31 | 0.32 | 0.16 | 0.11 | 0.04 | 0.04   0.38 | 0.38 | 0.16 | 0.07 | 0.05 | 0.04
    layout3_epi_pair_1064x152x256_x3_1_shifted_wgrad1          0.65 | 0.50 | 0.21 | 0.10 | 0.08 | 0.08   0.50 | 0.49 | 0.16 | 0.10 | 0.04 | 0.05
    layout1_cols_pair_512x152x64_shifted_wgrad1                0.32 | 0.35 | 0.14 | 0.12 | 0.05 | 0.06   0.41 | 0.35 | 0.14 | 0.08 | 0.05 | 0.05
(`control` of the wgrad2 and acc cases: one application, nothing accumulated.)  dZ 0.00: the sweep formed the weight
gradients itself and wrote no stash.  Undecided PReLU branches: at most one element of a plane (1 of 196608 twice, 1 of
51200 once, none elsewhere; the bound is 1e-4 of a plane).
Every element of every case is within its allowance; the worst is 0.79 (a plane of the fp32 tile products of layout 3 at
1064 x 152 x 256).  Two findings on the way, both about the derivation and neither a defect (tests/elementwise.py,
`mlp_train_fwd_reference` and `_bn_statistics`; docs/history.md):
  * the forward of bn_prelu_fwd_kernel<R> subtracts the UNROUNDED mean sum (1 / M) -- the compiler contracts the product
    into the difference -- and saves the rounded one: without the term |weight| rstd u |mean| a few elements with
    |y| << |weight xh| were up to 44 times over at M = 100, 200, 384, 700 and hidden 96, whole columns apart, and none at
    M = 512 and 1024 where 1 / M is a power of two.  With it those planes sit at 0.69 .. 0.78, the others at 0.30.
  * the shifted one-pass variance of the three-pass BatchNorm (M = 1064) put one rstd element at 1.005 of the unshifted
    form's allowance; with the same form on the plane shifted by its first row the statistics are at 0.32 .. 0.40 there.
The run's tail: profiles/train_mlp_elementwise_mi355x.txt.
"""
import ctypes as C

import pytest
import torch

from em_pose_amd import _lib
from tests import elementwise as E
from tests import test_train_mlp_bounds as B
from tests.test_hip_round5 import DEV, _mlp_pair, _run_mlp_train
from tests.test_train_mlp_layout import _set, _wgrad

pytestmark = pytest.mark.gpu
GAMMA = E.GAMMA_GEMM
OPTIONS = ('train_cols', 'train_fused', 'train_epi', 'train_x3')
PASSES = {'train_cols': 0, 'train_fused': 0, 'train_epi': 0}


def case(name, options, layout, cols, M, in_dim, hidden, pair=False, wgrad='now', accumulate=0, shift=0.0):
    return pytest.param(dict(options=options, layout=layout, cols=cols, M=M, in_dim=in_dim, hidden=hidden, pair=pair,
                             wgrad=wgrad, accumulate=accumulate, shift=shift), id=name)


CASES = [
    case('layout1_cols_pair_384x296x512_wgrad2', {}, 1, True, 384, 296, 512, pair=True, wgrad='wgrad2'),
    case('layout1_cols_single_100x296x512_wgrad2', {}, 1, True, 100, 296, 512, wgrad='wgrad2'),
    case('layout1_cols_pair_2x152x64_wgrad1', {}, 1, True, 2, 152, 64, pair=True, wgrad='wgrad1'),
    case('layout1_cols_single_2x152x64_now', {}, 1, True, 2, 152, 64),
    case('layout1_cols_pair_17x152x64_wgrad1_acc', {}, 1, True, 17, 152, 64, pair=True, wgrad='wgrad1', accumulate=1),
    case('layout1_cols_single_17x152x64_now_acc', {}, 1, True, 17, 152, 64, accumulate=1),
    case('layout1_cols_pair_512x152x64_wgrad1', {}, 1, True, 512, 152, 64, pair=True, wgrad='wgrad1'),
    case('layout1_cols_single_512x152x64_now', {}, 1, True, 512, 152, 64),
    case('layout1_passes_100x152x64_now', PASSES, 1, False, 100, 152, 64),
    case('layout1_passes_200x152x64_wgrad1', PASSES, 1, False, 200, 152, 64, wgrad='wgrad1'),
    case('layout1_passes_384x152x64_now', PASSES, 1, False, 384, 152, 64),
    case('layout1_passes_512x152x64_wgrad1', PASSES, 1, False, 512, 152, 64, wgrad='wgrad1'),
    case('layout1_passes_700x152x64_now', PASSES, 1, False, 700, 152, 64),
    case('layout1_passes_1024x152x64_wgrad1', PASSES, 1, False, 1024, 152, 64, wgrad='wgrad1'),
    case('layout1_passes_three_pass_bn_1064x152x64_now', PASSES, 1, False, 1064, 152, 64),
    case('layout1_passes_100x152x96_wgrad1', PASSES, 1, False, 100, 152, 96, wgrad='wgrad1'),
    case('layout1_passes_three_pass_bn_1064x152x96_now', PASSES, 1, False, 1064, 152, 96),
    case('layout2_fused_100x152x64_wgrad2_acc', {'train_cols': 0, 'train_fused': 2}, 2, False, 100, 152, 64, wgrad='wgrad2',
         accumulate=1),
    case('layout2_fused_384x296x512_wgrad2_acc', {'train_cols': 0, 'train_fused': 2}, 2, False, 384, 296, 512, wgrad='wgrad2',
         accumulate=1),
    case('layout3_epi_100x152x64_now', {'train_epi': 2}, 3, False, 100, 152, 64),
    case('layout3_epi_1064x152x256_x3_0_now', {'train_x3': 0}, 3, False, 1064, 152, 256),
    case('layout3_epi_pair_1064x152x256_x3_1_wgrad1', {'train_x3': 1}, 3, False, 1064, 152, 256, pair=True, wgrad='wgrad1'),
    case('layout1_passes_three_pass_bn_1064x152x64_shifted_wgrad1', PASSES, 1, False, 1064, 152, 64, wgrad='wgrad1', shift=3.0),
    case('layout3_epi_pair_1064x152x256_x3_1_shifted_wgrad1', {'train_x3': 1}, 3, False, 1064, 152, 256, pair=True, wgrad='wgrad1',
         shift=3.0),
    case('layout1_cols_pair_512x152x64_shifted_wgrad1', {}, 1, True, 512, 152, 64, pair=True, wgrad='wgrad1', shift=3.0),
]


def guarded(t):
    """The array followed by NaNs: a read past its end poisons the result."""
    buf = torch.full((t.numel() + 256,), float('nan'), device=DEV)
    buf[:t.numel()] = t.reshape(-1).to(DEV)
    return buf[:t.numel()].view(t.shape)


def inputs(c, application=0):
    x, d_outs = B.case_inputs(c['M'], c['in_dim'], c['shift'], seed=None if application == 0 else 1000 + c['M'])
    assert all(float(d[:, w:].abs().max()) == 0.0 for d, w in zip(d_outs, (66, 10)))      # padding columns zero
    return guarded(x), [guarded(d) for d in d_outs]


def written_gradients(view, grads):
    """The gradient tensors by the keys of mlp_train_bwd_reference."""
    out, it = {}, iter(grads)
    for l, (lin, bn, act) in enumerate(view.specs):
        out['dW%d' % l], out['db%d' % l] = next(it), next(it)
        if bn is not None:
            out['dgamma%d' % l], out['dbeta%d' % l], out['dslope%d' % l] = next(it), next(it), next(it)
    return out


def check_forward(c, net, layers, running, batches, x, res, i, tag, reports):
    L, M, H, layout = len(layers), c['M'], c['hidden'], c['layout']
    bn0 = net.dense_specs()[0][1]
    val, tol = E.mlp_train_fwd_reference(layers, x, res['save'][i], layout, GAMMA, bn0.eps, bn0.momentum, running)
    got = {'out': res['out'][i]}
    planes = E.mlp_train_save_planes(res['save'][i], layout, L, M, H)
    for l, (lin, bn, act) in enumerate(net.dense_specs()[:-1]):
        for name, t in planes[l].items():
            got['%s%d' % (name, l)] = t
        got['running_mean%d' % l], got['running_var%d' % l] = bn.running_mean, bn.running_var
        assert int(bn.num_batches_tracked) == batches[l] + 1, 'num_batches_tracked of layer %d' % l
    assert got.keys() == val.keys()
    reports.update({k + tag: r for k, r in B.check_all(got, val, tol, **c['tile']).items()})


def check_reverse(c, layers, x, d_out, res, i, tag, reports, init, with_weights):
    """One application's sweep: the stash (deferred) and every gradient it writes; returns the rows
    `mlp_train_wgrad_reference` takes, per layer."""
    L, M, H, layout = len(layers), c['M'], c['hidden'], c['layout']
    out_dim = layers[-1]['w'].shape[0]
    val, tol, info = E.mlp_train_bwd_reference(layers, x, res['save'][i], layout, d_out, GAMMA, init=init,
                                               rows_only=not with_weights)
    print(' %s: undecided PReLU branches per hidden layer %s of %d' % (tag, info['undecided_count'], M * H))
    assert max(info['undecided']) <= B.UNDECIDED_MAX, info['undecided']
    got = written_gradients(res['views'][i], res['grads'][i])
    if with_weights:
        assert float(res['stash'][i].abs().max()) == 0.0          # no stash passed: nothing may have been written
    else:
        slots = E.mlp_train_stash_planes(res['stash'][i], L, M, H, out_dim)
        got.update({'dZ%d' % l: slots[l] for l in range(L - 1)})
        got['d_out'] = slots[L - 1]
        for k, t in got.items():      # the deferred sweep leaves the weight gradients alone
            if k.startswith(('dW', 'db')) and not k.startswith('dbeta'):
                assert torch.equal(t, init[k]) if init is not None else float(t.abs().max()) == 0.0, k
    keys = sorted(k for k in val if k in got)
    assert set(val) - set(got) == ({k for k in val if k.startswith(('dZ', 'd_out'))} if with_weights else set())
    reports.update({k + tag: r for k, r in B.check_all(got, val, tol, keys=keys, **c['tile']).items()})
    return info['rows']


def check_weight_gradients(c, rows_of_apps, res, i, tag, reports, init):
    """dW, db of every layer over all applications against mlp_train_wgrad_reference."""
    got = written_gradients(res['views'][i], res['grads'][i])
    val, tol = {}, {}
    for l in range(len(rows_of_apps[0])):
        seed = None if init is None else (init['dW%d' % l], init['db%d' % l])
        val['dW%d' % l], tol['dW%d' % l], val['db%d' % l], tol['db%d' % l] = \
            E.mlp_train_wgrad_reference([rows[l] for rows in rows_of_apps], GAMMA, seed)
    reports.update({k + tag: r for k, r in B.check_all(got, val, tol, keys=sorted(val), **c['tile']).items()})


@pytest.mark.parametrize('c', CASES)
def test_every_element_of_everything_written_within_its_allowance(c, request):
    from em_pose_amd.nn.train_engine import _MlpView
    lib = _lib.lib()
    c = dict(c, tile=dict(row_mod=16, col_mod=16) if c['cols'] else dict(row_mod=64, col_mod=32))
    M, deferred, acc = c['M'], c['wgrad'] != 'now', c['accumulate']
    before = {name: lib.empose_get_option(name.encode()) for name in OPTIONS}
    reports = {}
    try:
        _set(lib, c['options'])
        nets = _mlp_pair(c['in_dim'], c['hidden'], B.NET_SEED)
        layers = [B.layers_of(n)[0] for n in nets]
        inits, grads_init = [None, None], None
        if acc:       # random non-zero gradients to add to: the first application's sweep and the weight-gradient call
            g = torch.Generator().manual_seed(M)
            grads_init = [[torch.randn(p.shape, generator=g).to(DEV) for p in _MlpView(n).parameter_list()] for n in nets]
            inits = [{k: t.clone() for k, t in written_gradients(_MlpView(n), gl).items()} for n, gl in zip(nets, grads_init)]
        apps = []
        for a in range(2 if c['wgrad'] == 'wgrad2' else 1):
            x, d_outs = inputs(c, a)
            running = [B.layers_of(n)[1] for n in nets]
            batches = [[int(s[1].num_batches_tracked) for s in n.dense_specs()[:-1]] for n in nets]
            res = _run_mlp_train(nets, x, d_outs, M, c['pair'], deferred, accumulate=acc if a == 0 else 0,
                                 grads_init=grads_init if a == 0 else None)
            rows = []
            for i, view in enumerate(res['views']):
                tag = ' app%d net%d' % (a, i)
                p = view.params()
                # the id's layout and launch family are the ones that ran
                assert p.save_layout == c['layout'] and lib.empose_mlp_train_save_layout(C.byref(p), M) == c['layout']
                assert lib.empose_mlp_train_uses_weight_t(C.byref(p), M) == (0 if c['cols'] else 1)
                assert (view.weight_t is None) == (c['cols'] and c['pair'])       # W read by rows only in the paired call
                if c['options'].get('train_x3') == 1:
                    assert view.weight_x3 is not None and all(t is not None for t in view.weight_x3[:-1])
                    assert view.weight_t_x3 is not None and all(t is not None for t in view.weight_t_x3[1:])
                elif c['options'].get('train_x3') == 0:
                    assert view.weight_x3 is None and view.weight_t_x3 is None
                check_forward(c, nets[i], layers[i], running[i], batches[i], x, res, i, tag, reports)
                rows.append(check_reverse(c, layers[i], x, d_outs[i], res, i, tag, reports, inits[i] if a == 0 else None,
                                          not deferred))
            apps.append((res, x, rows))
        if deferred:
            res = apps[0][0]
            _wgrad(res, apps[0][1], M, accumulate=acc, more=[(r, xk) for r, xk, _ in apps[1:]])
            for i in (0, 1):
                check_weight_gradients(c, [rows[i] for _, _, rows in apps], res, i, ' wgrad net%d' % i, reports, inits[i])
    finally:
        _set(lib, before)
    groups = B.by_group(reports)
    print('%-58s %s' % (request.node.callspec.id, ' | '.join('%.2f' % groups.get(name, 0.0) for name, _ in B.GROUPS)))
    bad = [r.message for r in reports.values() if not r.ok]
    assert not bad, '\n'.join(bad)
