"""
The global -> LDS staging of operand blocks (csrc/stage_block.h): every kernel that stages a row block through it, at the
edges of what it has to get right -- a leading dimension wider than the block, a last block of a few rows, pad columns that
must read as zeros whatever the LDS held before, and the K-major copy of a tile-layout block.

  * Update MLPs (mlp_fused_x3_kernel<16> / <32>, mlp_fused_kernel): the 296 input columns are a view into a buffer of 336
    columns and one row more whose other elements are NaN; T = 8192 + 64 + 7 rows (tests/test_x3_shape16.py: two nets on
    the one-launch path, a last block of 7 rows).  Every output element against float64 within the allowance of
    tests/elementwise.py at GAMMA = 4, on all three instructions; the row behind the outputs stays as it was; three
    launches give the same bits.  Hidden widths 64 (every layer split by K) and 512.
  * Zero fill: the 6-sensor nets have K0 = 224, which ends inside the 64-column quad the staging pads to.  A launch of the
    12-sensor nets on NaN rows first leaves NaN in the CUs' activation buffers; a pad column that is not written as zero
    then multiplies 0 x NaN into every output.
  * heads_rows_kernel (from 4096 rows on): LGD-RNN models with LSTM widths 128 and 512 at 463 windows of 9 frames (4167
    rows, a last block of 7).  The initial estimate against a float64 evaluation of the two head layers on the LSTM's
    output rows, at the bound of tests/test_hip_round3.py's heads test, 2e-6 of the largest value, for `rows_x3` = 1, 0.
    The LSTM output is taken from the same LSTM kernels through the recurrent layer's own entry point.
  * stage_a_tile (blend_t_gemm_rod_kernel): the frame-per-lane SMPL path forced (`smpl_tile` = 2, `smpl_fuse` = 1) at 203
    frames -- three tiles and one of 11 frames -- against the general path (`smpl_tile` = 0) at the bounds of
    tests/test_hip_round3.py::test_frame_per_lane_smpl_path, for both `rows_x3` values.
"""
import ctypes

import numpy as np
import pytest
import torch

from em_pose_amd import _lib, synthetic
from em_pose_amd.bodymodels.smpl import SMPLLayer
from em_pose_amd.helpers.configuration import CONSTANTS as CONST
from em_pose_amd.helpers.configuration import lgd_config
from em_pose_amd.nn.models import create_model
from tests import elementwise as E
from tests import helpers as H

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GAMMA_MLP = 4
T_ROWS = 8192 + 64 + 7
LD_X = 336
SENTINEL = -12345.0
ARMS = [('mlp_fused16=1', dict(mlp_x3=1, mlp_fused16=1)), ('mlp_fused16=0', dict(mlp_x3=1, mlp_fused16=0)),
        ('mlp_x3=0', dict(mlp_x3=0))]
_CACHE = {}


def _set(**opts):
    for k, v in opts.items():
        _lib.check(_lib.lib().empose_set_option(k.encode(), int(v)))


def _update_net(n_markers, hidden):
    """Update nets of an LGD model (12 sensors: 296 inputs, 6: 224; 2 x `hidden`; 66 / 10 outputs), BatchNorm randomised."""
    key = ('net', n_markers, hidden)
    if key not in _CACHE:
        from tests.test_hip_round5 import _randomize_bn
        torch.manual_seed(17 + hidden + n_markers)
        net = create_model(lgd_config(n_markers, False, 1, hidden=hidden), SMPLLayer(H.small_model()))
        _randomize_bn(net, 12)
        net.vertex_ids = synthetic.small_vertex_ids(160)
        _CACHE[key] = net.to(DEV).eval()
    return _CACHE[key]


def _case(n_markers, hidden):
    """(net, inputs (T, K0), float64 outputs and allowances of both nets): computed once, shared, never written."""
    key = ('case', n_markers, hidden)
    if key not in _CACHE:
        net = _update_net(n_markers, hidden)
        k0 = 12 * n_markers + 152
        g = torch.Generator().manual_seed(T_ROWS + hidden + n_markers)
        xg = torch.randn(T_ROWS, k0, generator=g).to(DEV)
        sd = {k: v.detach() for k, v in net.state_dict().items() if not k.startswith('smpl.')}
        refs = [E.eval_mlp_reference(E.eval_mlp_layers(sd, p), xg, GAMMA_MLP) for p in ('pose_net_iter.', 'shape_net_iter.')]
        _CACHE[key] = (net, xg, refs)
    return _CACHE[key]


def _update_nets_fwd(net, x, ldx):
    """`x`: a (T, K0) view with row stride `ldx`.  The outputs carry one row more than T, preset to SENTINEL."""
    lib = _lib.lib()
    T = x.shape[0]
    assert x.stride(0) == ldx and x.stride(1) == 1
    handle = net._ensure_handle(torch.device(DEV))
    dp, ds = torch.full((T + 1, 66), float('nan'), device=DEV), torch.full((T + 1, 10), float('nan'), device=DEV)
    dp[T], ds[T] = SENTINEL, SENTINEL
    nbytes = lib.empose_update_workspace_bytes(handle, T)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    _lib.check(lib.empose_update_nets_fwd(handle, T, ctypes.c_void_p(x.data_ptr()), ldx, _lib.dptr(dp), _lib.dptr(ds),
                                          _lib.dptr(ws), nbytes, _lib.current_stream()))
    torch.cuda.synchronize()
    return dp, ds


def _held(name, tag, outs, refs, T):
    reports = []
    for what, got, (want, allow) in zip(('pose', 'shape'), outs, refs):
        assert bool((got[T] == SENTINEL).all()), '%s %s %s: the row behind the output was written' % (name, tag, what)
        reports.append(E.check('%s %s %s' % (name, tag, what), got[:T], want, allow, GAMMA_MLP,
                               col_mod=16 if tag == 'mlp_fused16=1' else 32))
    return reports


def _assert_reports(reports):
    for r in reports:
        print(r.message.splitlines()[0])
    bad = [r.message for r in reports if not r.ok]
    assert not bad, '\n'.join(bad)


@pytest.mark.parametrize('hidden', [64, 512])
def test_update_nets_from_a_wider_buffer_with_a_last_block_of_seven_rows(hidden):
    net, xg, refs = _case(12, hidden)
    buf = torch.full((T_ROWS + 1, LD_X), float('nan'), device=DEV)
    buf[:T_ROWS, :296] = xg
    x = buf[:T_ROWS, :296]
    reports, outs = [], {}
    try:
        for tag, opts in ARMS:
            _set(**opts)
            outs[tag] = _update_nets_fwd(net, x, LD_X)
            reports += _held('ld 336 hidden=%d' % hidden, tag, outs[tag], refs, T_ROWS)
        _set(mlp_x3=1, mlp_fused16=1)
        again = [_update_nets_fwd(net, x, LD_X) for _ in range(2)]
    finally:
        _lib.lib().empose_reset_options()
    _assert_reports(reports)
    for rep in again:                                   # three launches of the default: the same bits
        for a_, b_ in zip(outs['mlp_fused16=1'], rep):
            assert torch.equal(a_[:T_ROWS], b_[:T_ROWS])
    assert bool(torch.isnan(buf[T_ROWS]).all()) and bool(torch.isnan(buf[:, 296:]).all())   # (the input is only read)


@pytest.mark.parametrize('hidden', [64, 512])
def test_pad_columns_are_zero_after_a_launch_that_left_nan_in_lds(hidden):
    net12 = _update_net(12, hidden)
    net6, xg, refs = _case(6, hidden)
    assert xg.shape[1] == 224
    x_nan = torch.full((T_ROWS, 296), float('nan'), device=DEV)
    reports = []
    try:
        for tag, opts in ARMS:
            _set(**opts)
            dp, _ = _update_nets_fwd(net12, x_nan, 296)          # NaN into every activation buffer of every CU
            assert bool(torch.isnan(dp[:T_ROWS]).all())
            reports += _held('K0 = 224 after NaN, hidden=%d' % hidden, tag, _update_nets_fwd(net6, xg, 224), refs, T_ROWS)
    finally:
        _lib.lib().empose_reset_options()
    _assert_reports(reports)


# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def big_model():
    return synthetic.make_model()


@pytest.mark.parametrize('width', [128, 512])
def test_init_heads_on_a_last_block_of_seven_rows_against_float64(big_model, width):
    from tests.test_hip_round3 import _Option
    torch.manual_seed(23 + width)
    net = create_model(lgd_config(12, True, 1, hidden=32, rnn_hidden=width), SMPLLayer(big_model)).eval().to(DEV)
    B, F = 463, 9
    T = B * F
    assert T >= 4096 and T % 64 == 7
    g = torch.Generator().manual_seed(29)
    pos, ori = torch.randn(B, F, 36, generator=g).to(DEV), torch.randn(B, F, 108, generator=g).to(DEV)
    off_t, off_r = (0.02 * torch.randn(B, 12, 3, generator=g)).to(DEV), torch.eye(3).expand(B, 12, 3, 3).contiguous().to(DEV)
    # the LSTM's output rows from the LSTM kernels themselves, then the two heads in float64
    y = net.rnn(torch.cat([pos, ori], dim=-1), torch.full((B,), F, dtype=torch.int32)).reshape(T, width).double()
    want = []
    for head in (net.pose_net_init, net.shape_net_init):
        want.append(y @ head.weight.detach().double().t() + head.bias.detach().double())
    if net.shape_avg:
        want[1] = want[1].reshape(B, F, -1).mean(dim=1, keepdim=True).expand(B, F, 10).reshape(T, 10)
    for rows_x3 in (1, 0):
        with _Option(b'rows_x3', rows_x3), _Option(b'heads_rows', 1):
            r = net.forward_tensors(pos, ori, off_t, off_r, keep_history=True)
            torch.cuda.synchronize()
        for name, got, w in zip(('pose', 'shape'), (r['hist']['pose'][0], r['hist']['shape'][0]), want):
            assert got.shape == w.shape and bool(torch.isfinite(got).all()), (name, rows_x3)
            err = float((got.double() - w).abs().max())
            bound = 2e-6 * max(1.0, float(w.abs().max()))
            print('init heads width=%d rows_x3=%d %s: max err %.3e (bound %.3e), last block %.3e'
                  % (width, rows_x3, name, err, bound, float((got.double() - w)[T - 7:].abs().max())))
            assert err <= bound, (name, rows_x3, err, bound)


@pytest.mark.parametrize('rows_x3', [1, 0])
def test_tile_layout_block_staged_as_it_lies_at_a_ragged_frame_count(big_model, rows_x3):
    from tests.test_hip_parity import _smpl_case, build_net
    from tests.test_hip_round3 import _Option, _sensors_call
    T, F = 203, 7                                       # three tiles of 64 frames and one of 11
    model, vids = big_model, CONST.VERTEX_IDS
    if 'smpl_case' not in _CACHE:
        _CACHE['smpl_case'] = _smpl_case(model, vids, T, F, 11, 12)
    theta, beta, off_r, off_t, tgt, scale, _ = _CACHE['smpl_case']
    net = build_net(lgd_config(12, False, 1, hidden=32), model, vids)
    handle = net._ensure_handle(torch.device(DEV))
    assert _lib.lib().empose_smpl_tile_supported(handle) == 1
    with _Option(b'rows_x3', rows_x3):
        with _Option(b'smpl_tile', 0):
            general = _sensors_call(handle, T, F, theta, beta, off_r, off_t, tgt, scale)
        with _Option(b'smpl_tile', 2), _Option(b'smpl_fuse', 1):
            tile = _sensors_call(handle, T, F, theta, beta, off_r, off_t, tgt, scale)
            again = _sensors_call(handle, T, F, theta, beta, off_r, off_t, tgt, scale)
    assert all(np.isfinite(x).all() for x in tile)
    for a_, b_ in zip(tile, again):
        assert np.array_equal(a_, b_)
    for k in (0, 2):                                    # positions, joints: element by element
        print('rows_x3=%d output %d: max |tile - general| %.3e' % (rows_x3, k, np.abs(tile[k] - general[k]).max()))
        np.testing.assert_allclose(tile[k], general[k], atol=2e-5)
    assert np.mean(np.abs(tile[1] - general[1]) > 1e-4) < 1e-4
    for k in (3, 4):                                    # gradients: the share a frame and a half may take, or 1 %
        sc = max(1.0, float(np.abs(general[k]).max()))
        share = np.mean(np.abs(tile[k] - general[k]) > 1e-3 * sc)
        print('rows_x3=%d gradient %d: share beyond 1e-3 x %.3g: %.3e' % (rows_x3, k, sc, share))
        assert share < max(1e-2, 1.5 / T)
    assert (tile[3][scale == 0] == 0).all()
