"""
The three-piece kernels on the 16x16x32 form of the bf16 MFMA as the defaults (options `mlp_fused16`, `lstm_chain16`).

  * Update MLPs (csrc/mlp_fused_x3.hip, mlp_fused_x3_kernel<16>): every output element against float64 within the allowance
    of tests/elementwise.py at GAMMA_MLP = 4, the bar of tests/test_x3_elementwise.py, for `mlp_fused16 = 1`, `= 0` and the
    fp32 instruction (`mlp_x3 = 0`) on the same inputs.  T = 8192 + 64 + 7 rows: the smallest count at which two nets take
    the one-launch path (256 row blocks), with a last block of 7 rows; every row of every 64-row block is checked, which is
    what sees the single accumulator element a global store beside an in-flight MFMA corrupts.  Hidden widths 512 (a wave
    per 128 columns), 192 (one wave with half its columns, two with none) and 64 (every layer split over the waves by K);
    the first layer's K = 296 ends on a quarter of a 32-k step.
  * LSTM (csrc/api_lstm.hip plan_lstm): at the smallest chain batch the default options give the bits of `lstm_x3 = 3`,
    `lstm_chain16 = 0` gives other bits (lstm_chain_x3_kernel sums 16 k per instruction, not 32), and both are as accurate
    against float64 as the fp32 steps, at the bar of tests/test_lstm_chain16.py.
  * Both option names round-trip and reset to 1 (no GPU needed).
"""
import pytest
import torch

from em_pose_amd import _lib, synthetic
from em_pose_amd.bodymodels.smpl import SMPLLayer
from em_pose_amd.helpers.configuration import lgd_config
from em_pose_amd.nn.models import create_model
from tests import elementwise as E
from tests import helpers as H

DEV = 'cuda:0'
GAMMA_MLP = 4
T_ROWS = 8192 + 64 + 7
_CACHE = {}


def _set(**opts):
    for k, v in opts.items():
        _lib.check(_lib.lib().empose_set_option(k.encode(), int(v)))


def _update_net(hidden):
    """The update nets of LGD-12 (296 inputs, 2 x `hidden`, 66 / 10 outputs) with randomised BatchNorm statistics."""
    if ('net', hidden) not in _CACHE:
        from tests.test_hip_round5 import _randomize_bn
        torch.manual_seed(11 + hidden)
        net = create_model(lgd_config(12, False, 1, hidden=hidden), SMPLLayer(H.small_model()))
        _randomize_bn(net, 12)
        net.vertex_ids = synthetic.small_vertex_ids(160)
        _CACHE[('net', hidden)] = net.to(DEV).eval()
    return _CACHE[('net', hidden)]


def _case(hidden, scale):
    """(net, inputs, float64 outputs and allowances of both nets): computed once, shared, never written."""
    key = ('case', hidden, scale)
    if key not in _CACHE:
        net = _update_net(hidden)
        g = torch.Generator().manual_seed(T_ROWS + hidden)
        xg = (torch.randn(T_ROWS, 296, generator=g) * scale).to(DEV)
        sd = {k: v.detach() for k, v in net.state_dict().items() if not k.startswith('smpl.')}
        refs = [E.eval_mlp_reference(E.eval_mlp_layers(sd, p), xg, GAMMA_MLP) for p in ('pose_net_iter.', 'shape_net_iter.')]
        _CACHE[key] = (net, xg, refs)
    return _CACHE[key]


def _update_nets_fwd(net, xg):
    lib = _lib.lib()
    T = xg.shape[0]
    handle = net._ensure_handle(torch.device(DEV))
    dp, ds = torch.full((T, 66), float('nan'), device=DEV), torch.full((T, 10), float('nan'), device=DEV)
    nbytes = lib.empose_update_workspace_bytes(handle, T)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    _lib.check(lib.empose_update_nets_fwd(handle, T, _lib.dptr(xg), 296, _lib.dptr(dp), _lib.dptr(ds), _lib.dptr(ws),
                                          nbytes, _lib.current_stream()))
    torch.cuda.synchronize()
    return dp, ds


ARMS = [('mlp_fused16=1', dict(mlp_x3=1, mlp_fused16=1)), ('mlp_fused16=0', dict(mlp_x3=1, mlp_fused16=0)),
        ('mlp_x3=0', dict(mlp_x3=0))]


def _check_arms(hidden, scale, side=None):
    net, xg, refs = _case(hidden, scale)
    reports, outs = [], {}
    try:
        for tag, opts in ARMS:
            _set(**opts)
            if side is not None:
                H.queue_storing_kernels(*side)
            outs[tag] = _update_nets_fwd(net, xg)
            for name, got, (want, allow) in zip(('pose', 'shape'), outs[tag], refs):
                reports.append(E.check('update nets hidden=%d scale=%g %s %s' % (hidden, scale, tag, name), got, want, allow,
                                       GAMMA_MLP, col_mod=16 if tag == 'mlp_fused16=1' else 32))
        _set(mlp_x3=1, mlp_fused16=1)
        again = [_update_nets_fwd(net, xg) for _ in range(2)]
    finally:
        _lib.lib().empose_reset_options()
    for r in reports:
        print(r.message.splitlines()[0])
    bad = [r.message for r in reports if not r.ok]
    assert not bad, '\n'.join(bad)
    for rep in again:                                   # three launches of the new kernel: the same bits
        for a_, b_ in zip(outs['mlp_fused16=1'], rep):
            assert torch.equal(a_, b_)
    # the option selects another kernel: sums of 32 k per instruction against 16 do not round alike over 8263 x 76 outputs
    assert not all(torch.equal(a_, b_) for a_, b_ in zip(outs['mlp_fused16=1'], outs['mlp_fused16=0']))


@pytest.mark.gpu
@pytest.mark.parametrize('scale', [1.0, 30.0], ids=['unit_inputs', 'gradient_scale_inputs'])
@pytest.mark.parametrize('hidden', [512, 192, 64])
def test_update_nets_on_both_mfma_shapes_every_element_within_its_allowance(hidden, scale):
    _check_arms(hidden, scale)


@pytest.mark.gpu
def test_update_nets_on_both_mfma_shapes_within_their_allowance_beside_a_storing_stream():
    side = (torch.cuda.Stream(), torch.randn(1 << 26, device=DEV))
    torch.cuda.synchronize()
    _check_arms(512, 30.0, side=side)
    side[0].synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize('state,ragged', [(False, False), (True, True)], ids=['new_sequences', 'given_state_ragged'])
def test_lstm_default_is_the_16x16x32_chain_kernel(state, ragged):
    """B = 257, F = 3, In = 144, H = 64, two layers: one row in the last 64-row block, nine 32-row tiles, nine 16-k input
    steps (the last 32-k step is half)."""
    from tests.test_lstm_chain16 import _float64, _inputs, _rnn, _rnn_fwd, _to_dev
    In, Hd, B, F = 144, 64, 257, 3
    layer, ref = _rnn(In, Hd)
    x, lens, h0, c0 = _inputs(In, Hd, B, F, state, ragged)
    want = _float64(ref, x, lens, h0, c0)
    args = (_to_dev(x), _to_dev(lens, torch.int32), _to_dev(h0), _to_dev(c0))
    arms = {'default': dict(), 'lstm_x3=3': dict(lstm_x3=3), 'lstm_chain16=0': dict(lstm_chain16=0), 'fp32': dict(lstm_x3=0)}
    got, err = {}, {}
    try:
        for tag, opts in arms.items():
            _lib.lib().empose_reset_options()
            _set(**opts)
            got[tag] = _rnn_fwd(layer, *args)
            for name, a_ in zip(('y', 'h_n', 'c_n'), got[tag]):
                assert torch.isfinite(a_).all(), (tag, name)       # (the outputs start as NaN: every element written)
            err[tag] = max(float((a_.cpu().double() - w_).abs().max()) for a_, w_ in zip(got[tag], want))
    finally:
        _lib.lib().empose_reset_options()
    print('lstm default state=%s ragged=%s vs float64: %s' % (state, ragged, ', '.join('%s %.2e' % kv for kv in err.items())))
    for name, a_, b_ in zip(('y', 'h_n', 'c_n'), got['default'], got['lstm_x3=3']):
        assert torch.equal(a_, b_), name
    assert not all(torch.equal(a_, b_) for a_, b_ in zip(got['default'], got['lstm_chain16=0']))
    for tag in ('default', 'lstm_chain16=0'):
        assert err[tag] <= 1.5 * err['fp32'] + 2e-7, err


def test_shape_options_round_trip_and_reset_to_one():
    lib = _lib.lib()
    try:
        lib.empose_reset_options()
        for name in (b'mlp_fused16', b'lstm_chain16'):
            assert lib.empose_get_option(name) == 1, name
            assert lib.empose_set_option(name, 0) == 0, name
            assert lib.empose_get_option(name) == 0, name
            assert lib.empose_set_option(name, 7) == 0, name
            assert lib.empose_get_option(name) == 7, name
        assert lib.empose_reset_options() == 0
        for name in (b'mlp_fused16', b'lstm_chain16'):
            assert lib.empose_get_option(name) == 1, name
    finally:
        lib.empose_reset_options()
