"""
Large-batch LSTM steps with the operands the kernel produced itself on TWO f16 pieces (csrc/lstm_chain16_x3.hip
lstm_chain16_pair_kernel, csrc/f16pair.h, option `lstm_pair16`, the default; run with `-m gpu` on an MI355X).

The hidden state h = o tanh(c) lies in [-1, 1] and goes as split(h 2^14); weights as split(w s_n) with one power-of-two
scale per gate column; three f16 products instead of six bf16 ones.  The raw input of layer 0 and a caller's h0 are not
bounded: they stay on three bf16 pieces, their weights packed as the pieces of w s_n 2^14, and share the accumulator.

  * accuracy: every element of y, h_n, c_n against torch.nn.LSTM in float64, arms `lstm_pair16 = 1`, `= 0` and the fp32
    MFMA steps (`lstm_x3 = 0`), at the bar of tests/test_lstm_chain16.py: err <= 1.5 x the fp32 arm's + 2e-7 and < 1e-5;
    one step from a given state also per element within the allowance of tests/elementwise.py (GAMMA_LSTM = 4);
  * a caller's h0 beyond the f16 scale (entries to +-8, one row at 1e4): the same bar; inputs x 30 and x 1e-3: the same bar
    with the absolute ceiling scaled as fp32's own roundoff scales (test_input_magnitudes);
  * a NaN row of x leaves every other row's bits alone;
  * the same launch twice, and `lstm_skip_dead` 0 / 1, give the same bits; `lstm_pair16` 1 and 0 do not (the option selects
    something); the name round-trips and resets to 1 (no GPU needed);
  * LGD-RNN-12 at 257 windows x 32 frames, N = 2: pose / shape / joints of `lstm_pair16 = 1` against the fp32 steps differ by
    at most twice what `lstm_pair16 = 0` differs from them on the same input (two independent roundings of one quantity
    differ by at most the sum of both errors), and by less than the 1e-4 of bench.py's parity field.
"""
import pytest
import torch

from em_pose_amd import _lib
from tests import elementwise as E
from tests.test_lstm_chain16 import DEV, _float64, _forward, _inputs, _net, _rnn, _rnn_fwd, _set, _to_dev, _windows

ARMS = [('pair16=1', dict(lstm_x3=3, lstm_pair16=1)), ('pair16=0', dict(lstm_x3=3, lstm_pair16=0)), ('fp32', dict(lstm_x3=0))]
NAMES = ('y', 'h_n', 'c_n')
# H = 64, inputs 144 (nine 16-k steps: the last wide step is half) and 64; B = 257: the first chain batch, an odd number of
# 32-row tiles; F = 3: launches of one and of two units; one case at the width of the LGD models
SHAPES = [(144, 64, 257, 3), (64, 64, 257, 3), (144, 64, 320, 3), (144, 512, 257, 2)]


def _run_arms(layer, args, arms=ARMS):
    got = {}
    try:
        for tag, opts in arms:
            _lib.lib().empose_reset_options()
            _set(**opts)
            got[tag] = _rnn_fwd(layer, *args)
    finally:
        _lib.lib().empose_reset_options()
    return got


def _errors(got, want):
    return {tag: max(float((a_.cpu().double() - w_).abs().max()) for a_, w_ in zip(outs, want)) for tag, outs in got.items()}


def _hold_to_the_bar(tag, layer, ref, x, lens, h0, c0, ceiling=1e-5):
    want = _float64(ref, x, lens, h0, c0)
    got = _run_arms(layer, (_to_dev(x), _to_dev(lens, torch.int32), _to_dev(h0), _to_dev(c0)))
    err = _errors(got, want)
    print('lstm %s vs float64: %s' % (tag, ', '.join('%s %.2e' % kv for kv in err.items())))
    for arm, outs in got.items():
        for name, a_ in zip(NAMES, outs):
            assert torch.isfinite(a_).all(), (arm, name)          # (the outputs start as NaN: every element written)
    assert err['pair16=1'] <= 1.5 * err['fp32'] + 2e-7 and err['pair16=1'] < ceiling, err
    return got


@pytest.mark.gpu
@pytest.mark.parametrize('ragged', [False, True])
@pytest.mark.parametrize('state', [False, True])
@pytest.mark.parametrize('In,Hd,B,F', SHAPES)
def test_pair_steps_are_as_accurate_as_the_fp32_mfma_ones(In, Hd, B, F, state, ragged):
    layer, ref = _rnn(In, Hd)
    x, lens, h0, c0 = _inputs(In, Hd, B, F, state, ragged)
    got = _hold_to_the_bar('%s state=%s ragged=%s' % ((In, Hd, B, F), state, ragged), layer, ref, x, lens, h0, c0)
    # the option selects something: other pieces, other roundings
    assert not all(torch.equal(a_, b_) for a_, b_ in zip(got['pair16=1'], got['pair16=0']))


@pytest.mark.gpu
def test_one_pair_step_every_element_within_its_allowance():
    """F = 1 from a given (h0, c0), two layers: layer 0 all wide steps, layer 1 pair steps for the input (layer 0's new h,
    which carries its allowance) and wide ones for h0."""
    from tests.test_x3_elementwise import GAMMA_LSTM, _lstm_layer, _unit
    B, Hd, In, L = 257, 64, 144, 2
    layer = _lstm_layer(In, Hd, L, B + Hd + In)
    g = torch.Generator().manual_seed(B)
    x = torch.randn(B, 1, In, generator=g).to(DEV)
    h0, c0 = (0.5 * torch.randn(L, B, Hd, generator=g)).to(DEV), (0.5 * torch.randn(L, B, Hd, generator=g)).to(DEV)
    lens = torch.ones(B, dtype=torch.int64).to(DEV)
    refs, inp, e_in = [], x[:, 0], None
    for l in range(L):
        h1, c1, eh, ec = E.lstm_step_reference(*_unit(layer, l), inp, h0[l], c0[l], GAMMA_LSTM, e_x=e_in)
        refs.append((h1, c1, eh, ec))
        inp, e_in = h1, eh
    dev_layer = layer.to(DEV)
    reports = []
    try:
        for tag, opts in ARMS[:2]:
            _lib.lib().empose_reset_options()
            _set(**opts)
            dev_layer.init_state = (h0, c0)
            y = dev_layer(x, lens)
            torch.cuda.synchronize()
            hn, cn = dev_layer.final_state
            reports.append(E.check('lstm step %s y' % tag, y[:, 0], refs[-1][0], refs[-1][2], GAMMA_LSTM, col_mod=32))
            for l in range(L):
                reports.append(E.check('lstm step %s h_n[%d]' % (tag, l), hn[l], refs[l][0], refs[l][2], GAMMA_LSTM, col_mod=32))
                reports.append(E.check('lstm step %s c_n[%d]' % (tag, l), cn[l], refs[l][1], refs[l][3], GAMMA_LSTM, col_mod=32))
    finally:
        _lib.lib().empose_reset_options()
        dev_layer.release()
    for r in reports:
        print(r.message.splitlines()[0])
    bad = [r.message for r in reports if not r.ok]
    assert not bad, '\n'.join(bad)


@pytest.mark.gpu
@pytest.mark.parametrize('ragged', [False, True])
def test_a_callers_state_beyond_the_f16_scale(ragged):
    """h0 with entries up to +-8 and one row at 1e4: 1e4 x 2^14 is past f16 -- the wide first step is what takes it."""
    In, Hd, B, F = 144, 64, 257, 3
    layer, ref = _rnn(In, Hd)
    x, lens, h0, c0 = _inputs(In, Hd, B, F, True, ragged)
    h0 = h0 * (8.0 / h0.abs().max())
    h0[:, 64] = 1e4                                           # (a row that lives through every step when ragged)
    _hold_to_the_bar('h0 to 1e4, ragged=%s' % ragged, layer, ref, x, lens, h0, c0)


@pytest.mark.gpu
@pytest.mark.parametrize('scale', [30.0, 1e-3])
def test_input_magnitudes(scale):
    """The bar relative to the fp32 steps as everywhere.  The absolute ceiling of 1e-5 belongs to inputs of std 1: the gate
    sums of layer 0 have the magnitude m = sum |w| |x| ~ 144 x 0.08 x 0.8 x scale, and fp32's own roundoff u m grows with
    it (u m = 1.7e-5 at scale 30, before three steps add up in c), so the ceiling is 1e-5 x max(1, scale)."""
    In, Hd, B, F = 144, 64, 257, 3
    layer, ref = _rnn(In, Hd)
    x, lens, h0, c0 = _inputs(In, Hd, B, F, False, False)
    _hold_to_the_bar('x * %g' % scale, layer, ref, x * scale, lens, h0, c0, ceiling=1e-5 * max(1.0, scale))


@pytest.mark.gpu
def test_a_nan_row_stays_in_its_row():
    In, Hd, B, F = 144, 64, 257, 3
    layer, _ = _rnn(In, Hd)
    x, lens, h0, c0 = _inputs(In, Hd, B, F, False, False)
    bad = x.clone()
    bad[37] = float('nan')
    arm = ARMS[:1]
    clean = _run_arms(layer, (_to_dev(x), None, None, None), arm)['pair16=1']
    dirty = _run_arms(layer, (_to_dev(bad), None, None, None), arm)['pair16=1']
    keep = torch.ones(B, dtype=torch.bool, device=DEV)
    keep[37] = False
    for name, a_, b_ in zip(NAMES, clean, dirty):
        rows = 1 if name != 'y' else 0
        assert torch.isfinite(a_).all(), name
        assert torch.equal(a_.index_select(rows, keep.nonzero()[:, 0]), b_.index_select(rows, keep.nonzero()[:, 0])), name
        assert torch.isnan(b_.select(rows, 37)).any(), name


@pytest.mark.gpu
@pytest.mark.parametrize('case', ['fresh', 'fresh_ragged', 'given_state'])
def test_same_bits_twice_and_with_dead_work_skipped(case):
    In, Hd, B, F = 144, 64, 257, 3
    layer, _ = _rnn(In, Hd)
    x, lens, h0, c0 = _inputs(In, Hd, B, F, case == 'given_state', case == 'fresh_ragged')
    args = (_to_dev(x), _to_dev(lens, torch.int32), _to_dev(h0), _to_dev(c0))
    arms = [('skip=1', dict(lstm_x3=3, lstm_pair16=1, lstm_skip_dead=1)), ('skip=0', dict(lstm_x3=3, lstm_pair16=1, lstm_skip_dead=0)),
            ('again', dict(lstm_x3=3, lstm_pair16=1, lstm_skip_dead=1))]
    got = _run_arms(layer, args, arms)
    for name, a_, b_, c_ in zip(NAMES, got['skip=1'], got['skip=0'], got['again']):
        assert torch.isfinite(a_).all() and torch.isfinite(b_).all(), name
        assert a_.abs().max() > 0, name
        assert torch.equal(a_, b_), name
        assert torch.equal(a_, c_), name


def test_lstm_pair16_round_trips_and_resets_to_one():
    lib = _lib.lib()
    try:
        lib.empose_reset_options()
        assert lib.empose_get_option(b'lstm_pair16') == 1
        for v in (0, 7):
            assert lib.empose_set_option(b'lstm_pair16', v) == 0
            assert lib.empose_get_option(b'lstm_pair16') == v
        assert lib.empose_reset_options() == 0
        assert lib.empose_get_option(b'lstm_pair16') == 1
    finally:
        lib.empose_reset_options()


@pytest.mark.gpu
def test_lgd_forward_on_pair_steps_is_as_close_to_the_fp32_steps_as_three_pieces_are():
    net = _net()
    w = _windows(net, 257, 32, 13)
    got = {}
    try:
        for tag, opts in ARMS:
            _lib.lib().empose_reset_options()
            _set(**opts)
            got[tag] = _forward(net, w)
    finally:
        _lib.lib().empose_reset_options()
    diff = {}
    for tag in ('pair16=1', 'pair16=0'):
        for k in ('pose', 'shape', 'joints'):
            assert torch.isfinite(got[tag][k]).all(), (tag, k)
        diff[tag] = max(float((got[tag][k].double() - got['fp32'][k].double()).abs().max()) for k in ('pose', 'shape', 'joints'))
    print('LGD-RNN-12 257 x 32, N = 2, max |pose, shape, joints - fp32 steps|: lstm_pair16=1 %.3e, lstm_pair16=0 %.3e'
          % (diff['pair16=1'], diff['pair16=0']))
    assert diff['pair16=1'] <= 2.0 * diff['pair16=0'], diff
    assert diff['pair16=1'] < 1e-4, diff
