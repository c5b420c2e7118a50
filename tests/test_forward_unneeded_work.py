"""
Work the LGD forward skips because its result is never read (run with `-m gpu` on an MI355X).

  * option `last_pass_joints` (csrc/api_model.hip plan_smpl): an SMPL evaluation of the frame-per-lane path that is
    asked for joints only -- the last pass of a forward without histories -- multiplies only the rest-joint column tiles
    of the blend matrix and runs the chain alone;
  * option `lstm_state_direct` (csrc/api_lstm.hip run_lstm): new sequences get their zero hidden-state planes by one fill,
    and the last step of each layer stores h_n / c_n itself.

Both only leave work out or store a value a second time: every output is compared BIT FOR BIT with the option at 0.
"""
import pytest
import torch

from em_pose_amd import _lib, synthetic
from em_pose_amd.bodymodels.smpl import SMPLLayer
from em_pose_amd.helpers.configuration import lgd_config
from em_pose_amd.nn.models import create_model

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
MODEL_SEED = 20240521
_CACHE = {}


def _set(**options):
    for k, v in options.items():
        _lib.check(_lib.lib().empose_set_option(k.encode(), v))


def _body_model():
    if 'model' not in _CACHE:
        _CACHE['model'] = synthetic.make_model()
    return _CACHE['model']


def _net(n_markers, N=2):
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


def _forward(net, w, **kw):
    args = [torch.from_numpy(w[k]).to(DEV) for k in ('marker_pos', 'marker_oris', 'offset_t', 'offset_r')]
    res = net.forward_tensors(*args, **kw)
    torch.cuda.synchronize()
    return res


# B = 3 windows of F = 32 frames: T = 96, one full 64-frame tile and one half-filled one (the `valid` lanes of the chain,
# the GEMM's rows past the end); smpl_tile = 2 puts this size on the frame-per-lane path.
B_TILE, F_TILE = 3, 32


@pytest.mark.parametrize('n_markers', [12, 6])
def test_joints_only_last_pass_leaves_the_same_bits(n_markers):
    """LGD-RNN-12 / LGD-RNN-6, N = 2, no histories: pose, shape and joints with the reduced last pass (three column tiles of
    the blend product, chain-only tile kernel) are the bits of the full last pass."""
    net = _net(n_markers)
    w = _windows(_net(12), B_TILE, F_TILE, 11)
    got = {}
    try:
        _set(smpl_tile=2)
        assert _lib.lib().empose_smpl_tile_supported(net._ensure_handle(torch.device(DEV))) == 1
        for opt in (1, 0):
            _set(last_pass_joints=opt)
            got[opt] = _forward(net, w)
        _set(last_pass_joints=1)
        again = _forward(net, w)
    finally:
        _lib.lib().empose_reset_options()
    for k in ('pose', 'shape', 'joints'):
        assert torch.isfinite(got[0][k]).all() and torch.isfinite(got[1][k]).all(), k
        assert got[1][k].abs().max() > 0, k
        assert torch.equal(got[1][k], got[0][k]), k
        assert torch.equal(got[1][k], again[k]), k
    for a_, b_ in zip(got[1]['state'], got[0]['state']):
        assert torch.equal(a_, b_)


def test_last_pass_with_histories_takes_the_full_path():
    """The guard, not the kernel: when the sensor histories of the last pass are wanted, `last_pass_joints = 1` changes
    nothing -- through forward() with histories kept, every history tensor (marker positions and orientations included)
    and every output equals the `= 0` run bit for bit."""
    from em_pose_amd.data.data import SyntheticBatch
    net = _net(12)
    w = _windows(net, B_TILE, F_TILE, 11)
    names = ('pose_hat_history', 'shape_hat_history', 'joints_hat_history', 'markers_hat_history', 'markers_ori_hat_history')
    got = {}
    keep = net.keep_history
    try:
        _set(smpl_tile=2)
        net.keep_history = True
        for opt in (1, 0):
            _set(last_pass_joints=opt)
            out = net(SyntheticBatch(w, device=DEV))
            torch.cuda.synchronize()
            got[opt] = (out, {n: [h.clone() for h in getattr(net, n)] for n in names})
    finally:
        net.keep_history = keep
        _lib.lib().empose_reset_options()
    for k in got[1][0]:
        assert torch.isfinite(got[1][0][k]).all(), k
        assert torch.equal(got[1][0][k], got[0][0][k]), k
    for n in names:
        assert len(got[1][1][n]) == net.N + 1
        for i, (a_, b_) in enumerate(zip(got[1][1][n], got[0][1][n])):
            assert torch.isfinite(a_).all(), (n, i)
            assert torch.equal(a_, b_), (n, i)
    # the last entries are the last pass's: its sensors were evaluated
    assert got[1][1]['markers_hat_history'][-1].abs().max() > 0


# ---- LSTM final state ------------------------------------------------------------------------------------------------
IN, HID, LAYERS = 144, 512, 2   # the LSTM of the LGD-RNN-12 models


def _rnn():
    from em_pose_amd.nn.layers import RNNLayer
    if 'rnn' not in _CACHE:
        torch.manual_seed(7)
        layer = RNNLayer(IN, HID, LAYERS).eval()
        with torch.no_grad():
            for p in layer.lstm.parameters():
                p.mul_(2.0)
        _CACHE['rnn'] = layer.to(DEV)
    return _CACHE['rnn']


def _rnn_fwd(layer, x, lens, h0, c0):
    """empose_rnn_fwd as it is (RNNLayer.forward always passes lengths; the LGD forward of full windows passes none)."""
    lib = _lib.lib()
    dev = torch.device(DEV)
    B, F = x.shape[0], x.shape[1]
    with torch.cuda.device(dev):
        handle = layer._ensure_handle(dev)
        y = torch.full((B, F, HID), float('nan'), device=dev)
        h_n = torch.full((LAYERS, B, HID), float('nan'), device=dev)
        c_n = torch.full((LAYERS, B, HID), float('nan'), device=dev)
        nbytes = lib.empose_rnn_workspace_bytes(handle, B, F)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        _lib.check(lib.empose_rnn_fwd(handle, B, F, _lib.dptr(x), x.shape[2], _lib.dptr(lens), _lib.dptr(h0), _lib.dptr(c0),
                                      _lib.dptr(y), _lib.dptr(h_n), _lib.dptr(c_n), _lib.dptr(ws), nbytes,
                                      _lib.current_stream()))
        torch.cuda.synchronize()
    return y, h_n, c_n


def _direct_vs_copies(x, lens, h0, c0):
    got = {}
    try:
        for opt in (1, 0):
            _set(lstm_state_direct=opt)
            got[opt] = _rnn_fwd(_rnn(), x, lens, h0, c0)
    finally:
        _lib.lib().empose_reset_options()
    for name, a_, b_ in zip(('y', 'h_n', 'c_n'), got[1], got[0]):
        assert torch.isfinite(a_).all() and torch.isfinite(b_).all(), name    # (the outputs start as NaN: every element written)
        assert torch.equal(a_, b_), name
    return got[1]


# 320 rows: five 64-row tiles, 80 workgroup tiles -- a workgroup per (tile, layer); 1024 rows (the benchmark's): 256 tiles, a
# workgroup walks both layers of a launch.  F = 4: five step launches, both layers' last steps in different launches.
@pytest.mark.parametrize('B', [320, 1024])
@pytest.mark.parametrize('with_lengths', [False, True])
def test_lstm_final_state_of_new_sequences_is_stored_by_the_last_step(B, with_lengths):
    F = 4
    g = torch.Generator().manual_seed(B)
    x = torch.randn(B, F, IN, generator=g).to(DEV)
    lens = torch.full((B,), F, dtype=torch.int32, device=DEV) if with_lengths else None
    y, h_n, c_n = _direct_vs_copies(x, lens, None, None)
    assert torch.equal(h_n[-1], y[:, -1])      # the top layer's final hidden state is its last output
    assert c_n.abs().max() > 0


def test_lstm_final_state_carried_and_ragged():
    """Carried state keeps its copies and splits (the option does not apply); new sequences with ragged lengths take the
    direct path -- the step kernel rewrites the frozen state of rows past their length at every step, so the last step
    stores every row of h_n / c_n.  Both equal the `= 0` run bit for bit."""
    B, F = 320, 4
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, F, IN, generator=g).to(DEV)
    lens = torch.randint(1, F + 1, (B,), generator=g).to(torch.int32)
    lens[:4] = torch.tensor([1, 2, 3, 4], dtype=torch.int32)
    lens[-1], lens[64] = 1, F
    assert set(lens.tolist()) == {1, 2, 3, 4}
    lens = lens.to(DEV)
    h0 = (0.5 * torch.randn(LAYERS, B, HID, generator=g)).to(DEV)
    c0 = (0.5 * torch.randn(LAYERS, B, HID, generator=g)).to(DEV)
    _direct_vs_copies(x, lens, h0, c0)
    y, h_n, c_n = _direct_vs_copies(x, lens, None, None)
    rows = torch.arange(B, device=DEV)
    assert torch.equal(h_n[-1], y[rows, (lens - 1).long()])    # a row's final state is that of its own last frame
    assert (y[0, 1:] == 0).all()                               # ... and its outputs past it are zero padding


def test_lstm_workspace_carves_the_hidden_state_planes_back_to_back():
    """The single fill of `lstm_state_direct` relies on the 2 L hidden-state planes lying back to back in the workspace.
    run_lstm checks that against the carve on every call and fails with EMPOSE_EINVAL otherwise (the carve needs a device
    handle, so there is no CPU form of this test): a call on the direct path that returns OK has passed the check."""
    B, F = 320, 4
    x = torch.randn(B, F, IN, generator=torch.Generator().manual_seed(3)).to(DEV)
    try:
        _set(lstm_state_direct=1)
        y, h_n, c_n = _rnn_fwd(_rnn(), x, None, None, None)
    finally:
        _lib.lib().empose_reset_options()
    assert torch.isfinite(y).all() and torch.isfinite(h_n).all() and torch.isfinite(c_n).all()
