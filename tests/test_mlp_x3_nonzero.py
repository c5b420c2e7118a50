"""
Option `mlp_x3` is on at any non-zero value: `mlp_x3 = 2`, which used to select a kernel variant of its own, takes the
kernel of `mlp_x3 = 1` (csrc/api_model.hip plan_mlps), so the two update nets give the same bits.

T = 127 * 64 + 7 = 8135 rows: the smallest count at which two nets reach the 256 row panels of the one-launch path, with a
ragged last panel.  Hidden width 64 (every layer split over the waves by K) and 512 (a wave per 128 columns).
"""
import pytest
import torch

from em_pose_amd import _lib
from tests.test_x3_shape16 import DEV, _set, _update_net, _update_nets_fwd

T_ROWS = 127 * 64 + 7


@pytest.mark.gpu
@pytest.mark.parametrize('hidden', [64, 512])
def test_mlp_x3_two_gives_the_bits_of_mlp_x3_one(hidden):
    net = _update_net(hidden)
    g = torch.Generator().manual_seed(T_ROWS + hidden)
    xg = torch.randn(T_ROWS, 296, generator=g).to(DEV)
    outs = {}
    try:
        for value in (1, 2):
            _set(mlp_x3=value)
            outs[value] = _update_nets_fwd(net, xg)
    finally:
        _lib.lib().empose_reset_options()
    for name, one, two in zip(('pose', 'shape'), outs[1], outs[2]):
        assert torch.isfinite(one).all(), name            # (the outputs start as NaN: every element written)
        assert torch.equal(one, two), name
