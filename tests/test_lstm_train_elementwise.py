"""
GPU tests: every element of everything the training LSTM writes (csrc/api_lstm.hip: empose_lstm_train_fwd /
empose_lstm_train_bwd, through the C ABI) against float64, each within its own derived allowance (tests/elementwise.py:
lstm_gates_reference, lstm_bptt_reference; gamma = GAMMA_GEMM, u = 2^-24).  The allowances themselves are tested without
a GPU in tests/test_lstm_bptt_bounds.py.

Forward, per layer l and step t, rows with t < len: one float64 step from what the kernels themselves saved -- hprev[:, t],
the c plane at t - 1 (c0 at t = 0), the layer input (x, or plane y of the layer below) -- against the gate planes, the c
plane and the output at t.  Also: y == 0 exactly on padded steps; h_n / c_n carry the bits of the output / the c plane at
t = len - 1.
Reverse: every element of every output against the float64 sweep from that forward's own save buffer (so the forward's
error is no part of it).

Cases: the smallest shapes that take each branch; the id names the forward kernel (plan_lstm_f32 in
csrc/api_lstm.hip, by B and F) and the form of the reverse pass (carve_train_lstm / Bptt in csrc/api_lstm.hip,
rec_ksplit_applicable in csrc/gemm_rec.hip, gemm_fewrows_applicable in csrc/gemm_f32.hip), read off the dispatch code:
  forward   B <= 3 and F >= 4: lstm_persist_kernel (whole sequence, cooperative); else B <= 4 / 8 / 12 / 16:
            lstm_fewrows_kernel<4,2> / <8,2> / <12,2> / <16,1>; B <= 256: lstm_mid_kernel (32-row tiles: B = 17 is a second
            row tile of one row); above: lstm_chain_kernel, all units chained in one block from 192 tiles of 64 x 32
            (705 x 512: 12 x 16), spread below.
  reverse   L = 2 and 4H % 256 == 0: wavefront -- B <= 16 (and 4H <= 2048) on rec_fewrows_reg_kernel<4 / 8 / 12 / 16>, else,
            where the K-split applies (tiles of 64 x 64 times slices of 256 in [32, 1024], B > 16, at most 16 slices for the
            two segments), on rec_ksplit_kernel + rec_ksplit_reduce_kernel.  Otherwise layer after layer: the K-split pair
            with one segment; B <= 16 and 4H >= 1024: gemm_fewrows_kernel fused with the cell; else the plain GEMM and
            lstm_cell_bwd_kernel -- at B = 17, H = 256 (4 tiles x 4 slices = 16 < 32) with 4H = 1024.
Variants of two rows: no seq_lengths / h0 / c0 at all; no row reaching F; ldx = K + 4 with NaN in the padding columns
(every output bit-identical to the ldx = K run); dx, d_h0, d_c0 null.

Measured on the MI355X: worst err / allowance over all elements, per case.  Forward: gates | c | output; reverse: dx | dW
(w_ih, w_hh of all layers) | db | state (d_h0, d_c0); `control`: the float32 torch evaluation of the reverse sweep on the
CPU (tests/test_lstm_bptt_bounds.py), same grouping.
    B, F, K, H, L        forward on the GPU     reverse on the GPU          control (CPU, float32 torch)
    3, 4, 8, 256, 2      0.23 | 0.11 | 0.17     0.05 | 0.20 | 0.09 | 0.24   0.08 | 0.20 | 0.14 | 0.26
    4, 3, 8, 256, 2      0.26 | 0.16 | 0.19     0.04 | 0.21 | 0.09 | 0.21   0.06 | 0.26 | 0.14 | 0.23
    7, 3, 12, 256, 2     0.23 | 0.12 | 0.16     0.05 | 0.22 | 0.09 | 0.25   0.06 | 0.23 | 0.14 | 0.25
    12, 3, 8, 256, 1     0.24 | 0.13 | 0.15     0.08 | 0.31 | 0.10 | 0.25   0.13 | 0.31 | 0.10 | 0.31
    16, 3, 8, 256, 2     0.23 | 0.13 | 0.17     0.05 | 0.33 | 0.09 | 0.33   0.09 | 0.31 | 0.10 | 0.24
    17, 3, 8, 256, 2     0.49 | 0.25 | 0.21     0.06 | 0.28 | 0.09 | 0.24   0.09 | 0.28 | 0.12 | 0.29
    65, 3, 8, 256, 2     0.34 | 0.21 | 0.19     0.08 | 0.25 | 0.08 | 0.31   0.16 | 0.23 | 0.07 | 0.28
    65, 3, 8, 260, 1     0.31 | 0.21 | 0.20     0.13 | 0.25 | 0.08 | 0.31   0.20 | 0.22 | 0.08 | 0.36
    257, 2, 8, 256, 2    0.55 | 0.39 | 0.26     0.10 | 0.21 | 0.07 | 0.35   0.13 | 0.16 | 0.08 | 0.33
    705, 2, 8, 512, 2    0.69 | 0.37 | 0.29     0.10 | 0.27 | 0.06 | 0.39   0.15 | 0.14 | 0.05 | 0.36
    3, 4, 8, 16, 3       0.25 | 0.14 | 0.18     0.03 | 0.11 | 0.07 | 0.27   0.05 | 0.15 | 0.08 | 0.27
    5, 1, 8, 256, 2      0.11 | 0.05 | 0.07     0.03 | 0.23 | 0.16 | 0.27   0.05 | 0.25 | 0.15 | 0.25
  variants (3, 4, 8, 256, 2 and 65, 3, 8, 256, 2):
    no lengths, no state 0.43 | 0.29 | 0.25     0.04 | 0.25 | 0.10 | 0.06   and   0.55 | 0.35 | 0.30     0.09 | 0.38 | 0.07 | 0.21
    no row reaches F     0.22 | 0.10 | 0.15     0.05 | 0.23 | 0.10 | 0.24   and   0.33 | 0.19 | 0.16     0.08 | 0.27 | 0.09 | 0.31
    dx, d_h0, d_c0 null  dW 0.20, db 0.09                                   and   dW 0.25, db 0.08
The worst is 0.69 (a gate of the 705 x 512 case, lstm_chain_kernel: 5.5 u m against gamma = 8); the reverse pass stays
below 0.4 everywhere and next to the control.  No defect showed up: every element of every case within its allowance, y
exactly zero on padded steps, h_n / c_n the bits of the planes, the NaN padding of x never read.  The run's tail:
profiles/lstm_train_elementwise_mi355x.txt.
"""
import functools

import pytest
import torch

from tests import elementwise as E
from tests import test_lstm_bptt_bounds as T
from tests import test_lstm_train_driver as D

pytestmark = pytest.mark.gpu
DEV = D.DEV
GAMMA = E.GAMMA_GEMM

CASES = [pytest.param(3, 4, 8, 256, 2, id='persist_coop__wavefront_matvec4'),
         pytest.param(4, 3, 8, 256, 2, id='fewrows4x2__wavefront_matvec4'),
         pytest.param(7, 3, 12, 256, 2, id='fewrows8x2__wavefront_matvec8'),
         pytest.param(12, 3, 8, 256, 1, id='fewrows12x2__layers_matvec_fused_cell'),
         pytest.param(16, 3, 8, 256, 2, id='fewrows16x1__wavefront_matvec16'),
         pytest.param(17, 3, 8, 256, 2, id='mid_second_row_tile__layers_plain_gemm_cell_4h1024'),
         pytest.param(65, 3, 8, 256, 2, id='mid__wavefront_ksplit_two_segments'),
         pytest.param(65, 3, 8, 260, 1, id='mid__layers_ksplit_partial_slice'),
         pytest.param(257, 2, 8, 256, 2, id='chain_spread__wavefront_ksplit_f2'),
         pytest.param(705, 2, 8, 512, 2, id='chain_one_block_192_tiles__wavefront_ksplit_16_slices'),
         pytest.param(3, 4, 8, 16, 3, id='persist_coop__layers_plain_gemm_three_layers'),
         pytest.param(5, 1, 8, 256, 2, id='fewrows8x2_f1__wavefront_single_stage')]
VARIANT_ROWS = [pytest.param(3, 4, 8, 256, 2, id='persist_coop__wavefront_matvec4'),
                pytest.param(65, 3, 8, 256, 2, id='mid__wavefront_ksplit_two_segments')]


def lengths(inp):
    B, F = inp['B'], inp['F']
    return torch.full((B,), F, dtype=torch.long, device=DEV) if inp['lens'] is None else inp['lens'].long()


def check_forward(inp, fwd):
    """Every live element of the gate planes, the c plane and the output of every (layer, step), and the exact properties
    of y, h_n, c_n.  Returns the worst err / allowance of gates | c | output."""
    B, F, K, H, L = (inp[k] for k in 'BFKHL')
    lens = lengths(inp)
    planes = E.lstm_save_planes(fwd['save'], L, B, F, H)
    x = inp['x'][..., :K]
    worst = dict(gates=0.0, c=0.0, out=0.0)
    failures = []
    for l in range(L):
        w_ih, w_hh, b_ih, b_hh = inp['weights'][4 * l:4 * l + 4]
        layer_in = x if l == 0 else planes[l - 1]['y']
        out = fwd['y'] if l == L - 1 else planes[l]['y']
        for t in range(F):
            live = (t < lens)[:, None]
            c_prev = planes[l]['c'][:, t - 1] if t > 0 else inp['c0'][l] if inp['c0'] is not None else torch.zeros(B, H, device=DEV)
            h, c, e_h, e_c, gates, e_gates = E.lstm_gates_reference(w_ih, w_hh, b_ih.double() + b_hh.double(), layer_in[:, t],
                                                                    planes[l]['hprev'][:, t], c_prev, GAMMA)
            for key, got, want, tol in (('gates', planes[l]['gates'][:, t], gates, e_gates), ('c', planes[l]['c'][:, t], c, e_c),
                                        ('out', out[:, t], h, e_h)):
                # rows past their length are not held to the step (their place in the tile stays: rows are batch rows)
                want, tol = torch.where(live, want, got.double()), torch.where(live, tol, torch.ones_like(tol))
                r = E.check('layer %d step %d %s' % (l, t, key), got, want, tol, gamma=GAMMA, row_mod=64, col_mod=32)
                worst[key] = max(worst[key], r.worst)
                if not r.ok:
                    failures.append(r.message)
        last = (lens - 1)[:, None, None].expand(B, 1, H)
        assert torch.equal(fwd['h_n'][l], out.gather(1, last)[:, 0]), 'h_n of layer %d' % l
        assert torch.equal(fwd['c_n'][l], planes[l]['c'].gather(1, last)[:, 0]), 'c_n of layer %d' % l
    padded = torch.arange(F, device=DEV)[None, :] >= lens[:, None]
    assert bool((fwd['y'][padded] == 0).all()), 'y on padded steps'
    assert torch.isfinite(fwd['y']).all()
    print('forward  ' + '  '.join('%s %.2f' % kv for kv in worst.items()))
    assert not failures, '\n'.join(failures)
    return worst


def check_reverse(inp, fwd, bwd):
    """Every element of every tensor in `bwd` against the float64 sweep from fwd['save']."""
    val, tol = E.lstm_bptt_reference(inp['weights'], inp['x'][..., :inp['K']], inp['lens'], inp['c0'], fwd['save'], inp['dy'], GAMMA)
    assert set(bwd) <= set(val)
    reports = T.check_all(bwd, val, tol, keys=sorted(bwd))
    groups = {g: max([r.worst for k, r in reports.items() if k.startswith(pre)] or [0.0])
              for g, pre in (('dx', ('dx',)), ('dW', ('w_ih', 'w_hh')), ('db', ('b_ih', 'b_hh')), ('state', ('d_h0', 'd_c0')))}
    print('reverse  ' + '  '.join('%s %.2f' % kv for kv in groups.items()))
    bad = [r.message for r in reports.values() if not r.ok]
    assert not bad, '\n'.join(bad)
    return groups


@functools.lru_cache(maxsize=None)
def variant_run(B, F, K, H, L, lens, state):
    inp = D.inputs(B, F, K, H, L, lens=lens, state=state)
    fwd = D.forward(inp)
    return inp, fwd, D.backward(inp, fwd['save'])


@pytest.mark.parametrize('B,F,K,H,L', CASES)
def test_forward_every_saved_plane_and_output_within_its_allowance(B, F, K, H, L):
    check_forward(D.inputs(B, F, K, H, L), D.first_run(B, F, K, H, L)[0])


@pytest.mark.parametrize('B,F,K,H,L', CASES)
def test_reverse_every_output_within_its_allowance(B, F, K, H, L):
    fwd, bwd = D.first_run(B, F, K, H, L)
    assert len(bwd) == 4 * L + 3
    check_reverse(D.inputs(B, F, K, H, L), fwd, bwd)


@pytest.mark.parametrize('lens,state', [(None, False), ('short', True)], ids=['no_lengths_no_state', 'no_row_reaches_F'])
@pytest.mark.parametrize('B,F,K,H,L', VARIANT_ROWS)
def test_optional_inputs_and_short_batches(B, F, K, H, L, lens, state):
    inp, fwd, bwd = variant_run(B, F, K, H, L, lens, state)
    assert (inp['lens'] is None and inp['h0'] is None and inp['c0'] is None) if lens is None else int(inp['lens'].max()) == F - 1
    check_forward(inp, fwd)
    check_reverse(inp, fwd, bwd)


@pytest.mark.parametrize('B,F,K,H,L', VARIANT_ROWS)
def test_padding_columns_of_x_are_never_read(B, F, K, H, L):
    """ldx = K + 4, NaN in the four padding columns: every output finite and bit-identical to the ldx = K run."""
    inp = D.inputs(B, F, K, H, L)
    fwd, bwd = D.first_run(B, F, K, H, L)
    x = torch.full((B, F, K + 4), float('nan'), device=DEV)
    x[..., :K] = inp['x']
    wide = dict(inp, x=x, ldx=K + 4)
    fwd2 = D.forward(wide)
    bwd2 = D.backward(wide, fwd2['save'])
    for a, b in ((fwd, fwd2), (bwd, bwd2)):
        assert a.keys() == b.keys()
        for key in a:
            assert torch.isfinite(b[key]).all(), key
            assert torch.equal(a[key], b[key]), key


@pytest.mark.parametrize('B,F,K,H,L', VARIANT_ROWS)
def test_weight_gradients_without_the_optional_outputs(B, F, K, H, L):
    """dx, d_h0 and d_c0 null: the weight and bias gradients still within their allowances."""
    inp = D.inputs(B, F, K, H, L)
    fwd, _ = D.first_run(B, F, K, H, L)
    bare = D.backward(inp, fwd['save'], optional=False)
    assert len(bare) == 4 * L
    check_reverse(inp, fwd, bare)
