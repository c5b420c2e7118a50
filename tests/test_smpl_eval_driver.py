"""
The host driver of the LGD forward (csrc/api_model.hip: plan_smpl, run_smpl_eval, run_mlps), seen from outside: which
kernels it launches, how often, and which buffers it leaves alone (run with `-m gpu` on an MI355X).

The launch sequence is read off the profiler (`_lib.profile_read()`: launches per tag).  A forward of N iterations makes
N + 1 SMPL evaluations with the update nets between them; an evaluation is feature row, blend product and chain, and --
for the N evaluations that feed the update nets, when the model uses the gradient -- the transposed product and the
Rodrigues reverse.  On the fused frame-per-lane path the feature row and the Rodrigues reverse ride on the two products
and have no launches of their own.  The update nets take a launch per layer, or one launch for all layers once their
row panels fill the chip (T >= 8129 rows for two nets).

What nobody asked for is not written: on the frame-per-lane path the scratch sensor outputs of the workspace stay as
they were (NaN here), while the general kernel always writes them -- which also proves the test looks at the right bytes.
Body model: the 160-vertex stand-in of tests/golden/smpl_small.npz.
"""
import pytest
import torch

from em_pose_amd import _lib, synthetic
from em_pose_amd.bodymodels.smpl import SMPLLayer
from em_pose_amd.helpers.configuration import lgd_config
from em_pose_amd.nn.models import create_model
from tests import helpers as H

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
N = 2
TAGS = ('update_feat', 'blend_gemm', 'chain_sensors', 'blend_T_gemm', 'rodrigues_bwd', 'mlp_in_gemm', 'mlp_hidden_gemm',
        'mlp_out_gemm', 'mlp_fused', 'init_heads_gemm')
PATHS = {'general': dict(smpl_tile=0), 'tile_fused': dict(smpl_tile=2, smpl_fuse=1), 'tile_unfused': dict(smpl_tile=2, smpl_fuse=0)}
_CACHE = {}


def _net(use_gradient):
    """LGD-RNN-12, N = 2, 128-wide nets (whole 64s: every kernel variant applies) on the small body model."""
    if use_gradient not in _CACHE:
        torch.manual_seed(31 + use_gradient)
        cfg = lgd_config(12, True, N, hidden=128, rnn_hidden=128, m_use_gradient=bool(use_gradient))
        net = create_model(cfg, SMPLLayer(H.small_model()))
        net.vertex_ids = synthetic.small_vertex_ids(160)
        _CACHE[use_gradient] = net.to(DEV).eval()
    return _CACHE[use_gradient]


def _inputs(B, F):
    g = torch.Generator().manual_seed(B * 100 + F)
    r = lambda *s: torch.randn(*s, generator=g).to(DEV)
    return 0.3 * r(B, F, 36), r(B, F, 108), 0.05 * r(B, 12, 3), r(B, 12, 3, 3)


def _launches(net, B, F, **options):
    """Launches per tag of one forward (no histories) under `options`."""
    lib = _lib.lib()
    args = _inputs(B, F)
    try:
        for k, v in options.items():
            _lib.check(lib.empose_set_option(k.encode(), v))
        net.forward_tensors(*args)          # (handle, workspace and kernel attributes exist before the counted run)
        torch.cuda.synchronize()
        lib.empose_profile_enable(1)
        res = net.forward_tensors(*args)
        torch.cuda.synchronize()
        prof = _lib.profile_read()
    finally:
        lib.empose_profile_enable(0)
        lib.empose_reset_options()
    for k in ('pose', 'shape', 'joints'):
        assert torch.isfinite(res[k]).all(), k
    return {t: prof.get(t, (0.0, 0))[1] for t in TAGS}


def _layers(net):
    return sum(isinstance(m, torch.nn.Linear) for m in net.pose_net_iter.modules())


def _expected(path, use_gradient, layers, one_launch=False):
    fused = path == 'tile_fused'
    rev = N if use_gradient else 0
    want = {'update_feat': 0 if fused else N + 1, 'blend_gemm': N + 1, 'chain_sensors': N + 1, 'blend_T_gemm': rev,
            'rodrigues_bwd': 0 if fused else rev, 'init_heads_gemm': 1,
            'mlp_in_gemm': N, 'mlp_hidden_gemm': N * (layers - 2), 'mlp_out_gemm': N, 'mlp_fused': 0}
    if one_launch:
        want.update(mlp_in_gemm=0, mlp_hidden_gemm=0, mlp_out_gemm=0, mlp_fused=N)
    return want


# B = 12 windows of F = 8 frames: T = 96, one full 64-frame tile and a half-filled one.
@pytest.mark.parametrize('use_gradient', [1, 0])
@pytest.mark.parametrize('path', sorted(PATHS))
def test_launch_sequence_of_the_lgd_forward(path, use_gradient):
    net = _net(use_gradient)
    assert _lib.lib().empose_smpl_tile_supported(net._ensure_handle(torch.device(DEV))) == 1
    layers = _layers(net)
    assert layers >= 4
    got = _launches(net, 12, 8, **PATHS[path])
    assert got == _expected(path, use_gradient, layers)


def test_one_launch_update_nets_replace_the_layer_launches():
    """B = 128, F = 64: T = 8192 rows, 2 x 128 row panels -- both update nets, all layers, in one launch per iteration.
    Below 16384 frames the default `smpl_tile = 1` keeps the general SMPL path."""
    net = _net(1)
    assert _launches(net, 128, 64) == _expected('general', 1, _layers(net), one_launch=True)


def _scratch_sensor_outputs(net, T):
    """The scratch pos | ori | joints of the LGD workspace as float tensors (csrc/api_model.hip carve_lgd: x, scale,
    d_pose, d_shape, pos, ori, joints, ... -- every buffer rounded up to 256 bytes)."""
    up = lambda count: (count * 4 + 255) // 256 * 256
    d_x = 144 + 76 + (76 if net.use_gradient else 0)
    off = up(T * d_x) + up(T) + up(T * 66) + up(T * 10)
    out = []
    for cols in (36, 108, 66):
        out.append(net._workspace[off:off + T * cols * 4].view(torch.float32))
        off += up(T * cols)
    return out


# T = 96 (F = 8): a tile and a half; T = 70 (F = 7): a tile and six frames, no multiple of anything.
@pytest.mark.parametrize('B,F', [(12, 8), (10, 7)])
def test_unasked_sensor_outputs_are_not_written_on_the_frame_per_lane_path(B, F):
    net = _net(1)
    lib = _lib.lib()
    args = _inputs(B, F)
    net.forward_tensors(*args)              # allocates the workspace
    seen = {}
    try:
        for tile in (2, 0):
            _lib.check(lib.empose_set_option(b'smpl_tile', tile))
            torch.cuda.synchronize()
            net._workspace.fill_(255)       # every float a NaN
            res = net.forward_tensors(*args)
            torch.cuda.synchronize()
            assert torch.isfinite(res['joints']).all() and res['joints'].abs().max() > 0
            seen[tile] = [t.clone() for t in _scratch_sensor_outputs(net, B * F)]
    finally:
        lib.empose_reset_options()
    for name, t in zip(('pos', 'ori', 'joints'), seen[2]):
        assert torch.isnan(t).all(), name                    # frame-per-lane path: nobody asked, nothing written
    for name, t in zip(('pos', 'ori', 'joints'), seen[0]):
        assert torch.isfinite(t).all(), name                 # general path: its scratch copies, every element
