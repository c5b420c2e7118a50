"""
The fused update MLPs on TWO f16 pieces per operand (csrc/f16pair.h, mlp_fused_x3_kernel<PAIR16>, option `mlp_pair16`):
three v_mfma_f32_16x16x32_f16 per fp32 product under per-row / per-column power-of-two scales, against the six bf16
products of mlp_fused_x3_kernel<16> (`mlp_pair16 = 0`, the kernel this one replaces as the default).

Every output element of both nets is held to float64 within the allowance of tests/elementwise.py at GAMMA_MLP = 4, the
bar of tests/test_x3_elementwise.py, through the C ABI.  T = 8192 + 37 rows: 8192 is the smallest count at which two nets
take the one-launch path ((T + 63) / 64 * n_nets >= 256), the last block has 37 rows.

  1. hidden 512 (a wave per 128 columns), both arms, the arms differ in bits, a repeated launch does not;
  2. hidden 64 and 128: every hidden layer split over the waves by K;
  3. row i of x times 2^e(i), e cycling through -60 .. +60 within every 64-row block: every row still meets its (row-scaled)
     allowance -- the scale is per row, never per block; then one element inf and one NaN in two rows: every other row keeps
     its bits, the two rows are non-finite;
  4. a whole block of zero rows: the float64 result of zero input within the bar, nothing non-finite;
  5. column j of x times 2^(-12 + j mod 17), the spread of gradients beside sensor readings: no constant of its own -- the
     new arm's worst err / (u m) is at most max(4, 1.25 x that of `mlp_pair16 = 0` on the same inputs); the margin covers the
     draw-to-draw scatter of a maximum over 4 million elements.

Measured on the MI355X, worst err / (u m) over both nets against the bar of 4 (profiles/r11_gpu_tests_tail.log):
                                 mlp_pair16 = 1    mlp_pair16 = 0
    1. hidden 512                     0.739             0.875
    2. hidden 64                      0.740             0.660
       hidden 128                     0.793             0.658
    3. rows x 2^(-60 .. 60)           0.836             0.747
    4. zero rows                      0.739             0.875
    5. columns x 2^(-12 .. 4)         0.539             0.707
"""
import pytest
import torch

from em_pose_amd import _lib
from tests import elementwise as E
from tests.test_x3_shape16 import _set, _update_net, _update_nets_fwd

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GAMMA_MLP = 4
T_ROWS = 8192 + 37
ARMS = [('mlp_pair16=1', dict(mlp_x3=1, mlp_fused16=1, mlp_pair16=1)), ('mlp_pair16=0', dict(mlp_x3=1, mlp_fused16=1, mlp_pair16=0))]
_CACHE = {}


def _inputs(hidden):
    if ('x', hidden) not in _CACHE:
        g = torch.Generator().manual_seed(T_ROWS + hidden)
        _CACHE[('x', hidden)] = torch.randn(T_ROWS, 296, generator=g).to(DEV)
    return _CACHE[('x', hidden)]


def _refs(net, xg):
    sd = {k: v.detach() for k, v in net.state_dict().items() if not k.startswith('smpl.')}
    return [E.eval_mlp_reference(E.eval_mlp_layers(sd, p), xg, GAMMA_MLP) for p in ('pose_net_iter.', 'shape_net_iter.')]


def _run_arms(tag, net, xg, refs):
    """Both arms on `xg`: ({arm: outputs}, {arm: worst err / (u m)}, messages of the reports that fail)."""
    outs, worst, bad = {}, {}, []
    try:
        for arm, opts in ARMS:
            _set(**opts)
            outs[arm] = _update_nets_fwd(net, xg)
            worst[arm] = 0.0
            for name, got, (want, allow) in zip(('pose', 'shape'), outs[arm], refs):
                r = E.check('update nets %s %s %s' % (tag, arm, name), got, want, allow, GAMMA_MLP, col_mod=16)
                print(r.message.splitlines()[0])
                worst[arm] = max(worst[arm], r.ratio_um)
                if not r.ok:
                    bad.append(r.message)
    finally:
        _lib.lib().empose_reset_options()
    print('%s: worst err / (u m)  %s' % (tag, ',  '.join('%s %.3g' % kv for kv in worst.items())))
    return outs, worst, bad


def _fwd(net, xg, **opts):
    try:
        _set(**opts)
        return _update_nets_fwd(net, xg)
    finally:
        _lib.lib().empose_reset_options()


@pytest.mark.parametrize('hidden', [512, 64, 128])
def test_both_arms_every_element_within_its_allowance(hidden):
    net, xg = _update_net(hidden), _inputs(hidden)
    outs, _, bad = _run_arms('hidden=%d' % hidden, net, xg, _refs(net, xg))
    assert not bad, '\n'.join(bad)
    # the option selects another kernel: two f16 pieces and three bf16 pieces do not round alike over 8229 x 76 outputs
    assert not all(torch.equal(a_, b_) for a_, b_ in zip(outs['mlp_pair16=1'], outs['mlp_pair16=0']))
    for arm, opts in ARMS:                                # a repeated launch of an arm: the same bits
        for a_, b_ in zip(outs[arm], _fwd(net, xg, **opts)):
            assert torch.equal(a_, b_), arm


def test_rows_are_scaled_one_by_one_and_do_not_see_each_other():
    net = _update_net(512)
    i = torch.arange(T_ROWS, device=DEV)
    e = -60 + ((i % 64) * 120) // 63                      # -60 .. +60 within every 64-row block
    xg = _inputs(512) * torch.pow(torch.tensor(2.0, device=DEV), e.float())[:, None]
    outs, _, bad = _run_arms('rows x 2^(-60 .. 60)', net, xg, _refs(net, xg))
    assert not bad, '\n'.join(bad)
    # a non-finite value stays in its row: inf beside the block's smallest row, NaN beside its largest
    r_inf, r_nan = 64 * 5 + 1, 64 * 77 + 62
    xp = xg.clone()
    xp[r_inf, 17] = float('inf')
    xp[r_nan, 295] = float('nan')
    others = torch.ones(T_ROWS, dtype=torch.bool, device=DEV)
    others[[r_inf, r_nan]] = False
    for arm, opts in ARMS:
        for name, clean, got in zip(('pose', 'shape'), outs[arm], _fwd(net, xp, **opts)):
            assert torch.equal(got[others], clean[others]), (arm, name)
            assert not torch.isfinite(got[~others]).any(), (arm, name)


def test_a_block_of_zero_rows():
    net = _update_net(512)
    xg = _inputs(512).clone()
    xg[128:192] = 0.0                                     # a whole 64-row block
    xg[T_ROWS - 3] = 0.0                                  # and a row of the ragged last one
    outs, _, bad = _run_arms('zero rows', net, xg, _refs(net, xg))
    assert not bad, '\n'.join(bad)                        # (`check` counts a non-finite value as a violation)
    for got in outs['mlp_pair16=1']:
        assert torch.isfinite(got).all()
        assert torch.equal(got[128:192], got[128:129].expand(64, -1))   # the same input: the same bits in every row


def test_columns_spread_over_sixteen_binades_no_worse_than_three_bf16_pieces():
    net = _update_net(512)
    j = torch.arange(296, device=DEV)
    xg = _inputs(512) * torch.pow(torch.tensor(2.0, device=DEV), (-12 + j % 17).float())[None, :]
    _, worst, _ = _run_arms('columns x 2^(-12 .. 4)', net, xg, _refs(net, xg))
    assert worst['mlp_pair16=1'] <= max(4.0, 1.25 * worst['mlp_pair16=0']), worst
