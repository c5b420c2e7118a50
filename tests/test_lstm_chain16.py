"""
Large-batch LSTM steps on the 16x16x32 bf16 MFMA, and the dead work the chain step kernels leave out (run with `-m gpu` on
an MI355X).

  * option `lstm_x3 = 3` (csrc/lstm_chain16_x3.hip): lstm_chain_x3_kernel with its products on v_mfma_f32_16x16x32_bf16,
    weights in the LSTM_MID16 order.  Held to torch.nn.LSTM in float64 at every element of y, h_n and c_n, with the bar of
    test_hip_round5 (test_three_piece_bf16_lstm_steps_are_as_accurate_as_the_fp32_mfma_ones): its error is at most 1.5 x
    that of the fp32-MFMA step kernel (`lstm_x3 = 0`) on the same inputs, plus the 2e-7 that test allows for the fp32 path's
    own rounding luck, and below 1e-5.
  * option `lstm_skip_dead` (csrc/api_lstm.hip x3_steps): the recurrent k-steps of a unit whose h_{t-1} is the zero state of
    a new sequence, and -- without seq_lengths -- the fp32 h_prev loads / h_next stores.  Both only leave work out: every
    output is compared BIT FOR BIT with the option at 0, for `lstm_x3 = 1` and `= 3`.

plan_lstm is internal to the library (no CPU entry point reaches it), so its choice per `lstm_x3` is covered through these
cases: B = 257 is the first batch on the chain path.
"""
import copy

import pytest
import torch

from em_pose_amd import _lib, synthetic
from em_pose_amd.bodymodels.smpl import SMPLLayer
from em_pose_amd.helpers.configuration import lgd_config
from em_pose_amd.nn.models import create_model

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
MODEL_SEED = 20240521
LAYERS = 2
_CACHE = {}


def _set(**options):
    for k, v in options.items():
        _lib.check(_lib.lib().empose_set_option(k.encode(), v))


def _rnn(In, Hd):
    """(the layer on the device, its nn.LSTM in float64 on the CPU); weights x 2 as in test_hip_round5, so that the gates
    leave the linear part of their non-linearities."""
    from em_pose_amd.nn.layers import RNNLayer
    key = ('rnn', In, Hd)
    if key not in _CACHE:
        torch.manual_seed(7 + In + Hd)
        layer = RNNLayer(In, Hd, LAYERS).eval()
        with torch.no_grad():
            for p in layer.lstm.parameters():
                p.mul_(2.0)
        ref = copy.deepcopy(layer.lstm).double()
        _CACHE[key] = (layer.to(DEV), ref)
    return _CACHE[key]


def _rnn_fwd(layer, x, lens, h0, c0):
    """empose_rnn_fwd as it is; the outputs start as NaN, so an element nobody wrote shows."""
    lib = _lib.lib()
    dev = torch.device(DEV)
    B, F, Hd = x.shape[0], x.shape[1], layer.hidden_size
    with torch.cuda.device(dev):
        handle = layer._ensure_handle(dev)
        y = torch.full((B, F, Hd), float('nan'), device=dev)
        h_n = torch.full((LAYERS, B, Hd), float('nan'), device=dev)
        c_n = torch.full((LAYERS, B, Hd), float('nan'), device=dev)
        nbytes = lib.empose_rnn_workspace_bytes(handle, B, F)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        _lib.check(lib.empose_rnn_fwd(handle, B, F, _lib.dptr(x), x.shape[2], _lib.dptr(lens), _lib.dptr(h0), _lib.dptr(c0),
                                      _lib.dptr(y), _lib.dptr(h_n), _lib.dptr(c_n), _lib.dptr(ws), nbytes,
                                      _lib.current_stream()))
        torch.cuda.synchronize()
    return y, h_n, c_n


def _inputs(In, Hd, B, F, state, ragged):
    """x of std 1; `state`: given h0 / c0; `ragged`: lengths in 1 .. F that include 1 and F (else none)."""
    g = torch.Generator().manual_seed(1000 * B + 10 * F + In)
    x = torch.randn(B, F, In, generator=g)
    h0 = 0.5 * torch.randn(LAYERS, B, Hd, generator=g) if state else None
    c0 = 0.5 * torch.randn(LAYERS, B, Hd, generator=g) if state else None
    lens = None
    if ragged:
        lens = torch.randint(1, F + 1, (B,), generator=g)
        lens[0], lens[1], lens[-1], lens[64] = F, 1, 1, F     # (the last row: alone in its workgroup at B = 257)
        assert set(lens.tolist()) == set(range(1, F + 1))
    return x, lens, h0, c0


def _float64(ref, x, lens, h0, c0):
    """torch.nn.LSTM in float64 on the CPU; ragged rows by pack / pad: zero outputs past a row's length, its final state
    that of its own last frame."""
    from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence
    F = x.shape[1]
    xt = x.double().transpose(0, 1).contiguous()
    st = None if h0 is None else (h0.double(), c0.double())
    with torch.no_grad():
        if lens is None:
            y, (h, c) = ref(xt, st)
        else:
            y, (h, c) = ref(pack_padded_sequence(xt, lens.cpu(), enforce_sorted=False), st)
            y, _ = pad_packed_sequence(y, total_length=F)
    return y.transpose(0, 1), h, c


def _to_dev(t, dtype=None):
    return None if t is None else (t if dtype is None else t.to(dtype)).to(DEV)


# H = 64, inputs 144 (nine 16-k steps: the last 32-k step is half) and 64; B = 257: the first batch on the chain path, nine
# 32-row tiles (odd), the last workgroup with one row; B = 320; F = 3: the first and last launches carry one unit, the middle
# ones two.  One case at the full width of the LGD models.
SHAPES = [(144, 64, 257, 3), (64, 64, 257, 3), (144, 64, 320, 3), (64, 64, 320, 3), (144, 512, 257, 2)]


@pytest.mark.parametrize('ragged', [False, True])
@pytest.mark.parametrize('state', [False, True])
@pytest.mark.parametrize('In,Hd,B,F', SHAPES)
def test_chain16_steps_are_as_accurate_as_the_fp32_mfma_ones(In, Hd, B, F, state, ragged):
    layer, ref = _rnn(In, Hd)
    x, lens, h0, c0 = _inputs(In, Hd, B, F, state, ragged)
    want = _float64(ref, x, lens, h0, c0)
    args = (_to_dev(x), _to_dev(lens, torch.int32), _to_dev(h0), _to_dev(c0))
    err, again = {}, None
    try:
        for x3 in (0, 3):
            _set(lstm_x3=x3)
            got = _rnn_fwd(layer, *args)
            for name, a_ in zip(('y', 'h_n', 'c_n'), got):
                assert torch.isfinite(a_).all(), (x3, name)
            err[x3] = max(float((a_.cpu().double() - w_).abs().max()) for a_, w_ in zip(got, want))
        again = _rnn_fwd(layer, *args)
    finally:
        _lib.lib().empose_reset_options()
    print('lstm %s state=%s ragged=%s vs float64: fp32 MFMA %.2e, 16x16x32 three-piece bf16 %.2e'
          % ((In, Hd, B, F), state, ragged, err[0], err[3]))
    assert err[3] <= 1.5 * err[0] + 2e-7 and err[3] < 1e-5, err
    for name, a_, b_ in zip(('y', 'h_n', 'c_n'), got, again):
        assert torch.equal(a_, b_), name           # the same launch repeated: the same bits


# ---- dead work -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['fresh', 'fresh_ragged', 'given_state'])
@pytest.mark.parametrize('x3', [1, 3])
def test_skipping_dead_work_leaves_the_same_bits(x3, case):
    """fresh: both removals active; fresh_ragged: only the zero-state k-steps; given_state: neither -- equal all the same."""
    In, Hd, B, F = 144, 64, 257, 3
    layer, _ = _rnn(In, Hd)
    x, lens, h0, c0 = _inputs(In, Hd, B, F, case == 'given_state', case == 'fresh_ragged')
    args = (_to_dev(x), _to_dev(lens, torch.int32), _to_dev(h0), _to_dev(c0))
    got = {}
    try:
        _set(lstm_x3=x3)
        for opt in (1, 0):
            _set(lstm_skip_dead=opt)
            got[opt] = _rnn_fwd(layer, *args)
        _set(lstm_skip_dead=1)
        again = _rnn_fwd(layer, *args)
    finally:
        _lib.lib().empose_reset_options()
    for name, a_, b_, c_ in zip(('y', 'h_n', 'c_n'), got[1], got[0], again):
        assert torch.isfinite(a_).all() and torch.isfinite(b_).all(), name    # (the outputs start as NaN: every element written)
        assert a_.abs().max() > 0, name
        assert torch.equal(a_, b_), name
        assert torch.equal(a_, c_), name
    if lens is None:
        assert torch.equal(got[1][1][-1], got[1][0][:, -1])     # the top layer's final hidden state is its last output


def _body_model():
    if 'model' not in _CACHE:
        _CACHE['model'] = synthetic.make_model()
    return _CACHE['model']


def _net(n_markers=12, N=2):
    """LGD-RNN-<n_markers> on the synthetic V = 6890 body model, as bench.build_net makes it."""
    key = ('net', n_markers, N)
    if key not in _CACHE:
        torch.manual_seed(MODEL_SEED)
        net = create_model(lgd_config(n_markers, True, N), SMPLLayer(_body_model()))
        g = torch.Generator().manual_seed(MODEL_SEED + 1)
        with torch.no_grad():
            for m in net.modules():
                if isinstance(m, torch.nn.BatchNorm1d):
                    m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=g) * 0.1)
                    m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) + 0.5)
        _CACHE[key] = net.eval().to(DEV)
    return _CACHE[key]


def _windows(net, B, F, seed):
    """Synthetic windows whose sensor readings come from the HIP body model itself (bench.make_inputs)."""
    key = ('win', B, F, seed)
    if key not in _CACHE:
        def sensors(poses, betas, o_r, o_t):
            pos, ori, _ = net.get_estimated_real_markers(torch.from_numpy(poses).to(DEV), torch.from_numpy(betas).to(DEV),
                                                         torch.from_numpy(o_r[::F].copy()).to(DEV),
                                                         torch.from_numpy(o_t[::F].copy()).to(DEV), frames_per_window=F)
            return pos.cpu().numpy(), ori.cpu().numpy()
        _CACHE[key] = synthetic.make_windows(B, F, seed, sensors)
    return _CACHE[key]


def _forward(net, w):
    args = [torch.from_numpy(w[k]).to(DEV) for k in ('marker_pos', 'marker_oris', 'offset_t', 'offset_r')]
    res = net.forward_tensors(*args)
    torch.cuda.synchronize()
    return res


def test_lgd_forward_with_dead_work_skipped_leaves_the_same_bits():
    """LGD-RNN-12, N = 2, 257 windows x 32 frames (new sequences, no lengths: both removals active in its LSTM): pose, shape,
    joints and the LSTM's final state with `lstm_skip_dead = 1` are the bits of `= 0`."""
    net = _net()
    w = _windows(net, 257, 32, 13)
    got = {}
    try:
        for opt in (1, 0):
            _set(lstm_skip_dead=opt)
            got[opt] = _forward(net, w)
    finally:
        _lib.lib().empose_reset_options()
    for k in ('pose', 'shape', 'joints'):
        assert torch.isfinite(got[0][k]).all() and torch.isfinite(got[1][k]).all(), k
        assert got[1][k].abs().max() > 0, k
        assert torch.equal(got[1][k], got[0][k]), k
    assert len(got[1]['state']) == len(got[0]['state']) > 0
    for a_, b_ in zip(got[1]['state'], got[0]['state']):
        assert torch.isfinite(a_).all() and torch.equal(a_, b_)
