"""
The allowances of tests/train_glue_ref.py on the CPU (no GPU), one case per kernel: an fp32 torch evaluation of the same
operation lies within them, and one element moved by twice its own allowance is rejected and named -- the bounds are
neither too tight for an honest fp32 evaluation nor vacuous.
"""
import torch

from em_pose_amd.helpers.configuration import CONSTANTS
from tests import elementwise as E
from tests import train_glue_ref as G


def _holds_and_catches(name, got32, want, allow, at):
    got32, want, allow = (t.reshape(-1, t.shape[-1]) for t in (got32, want, allow))
    r = E.check(name, got32, want, allow, col_mod=want.shape[-1])
    assert r.ok, r.message
    assert float(allow[at]) > 0, (name, at)
    bad = got32.double().clone()
    bad[at] = want[at] + 2.0 * float(allow[at])
    r_bad = E.check(name, bad, want, allow, col_mod=want.shape[-1])
    assert r_bad.n_bad == 1 and r_bad.worst_index == at, r_bad.message
    assert '(%d, %d): 1' % (at[0] % 64, at[1]) in r_bad.message, r_bad.message


def test_loss_allowances_hold_an_fp32_evaluation_and_catch_one_planted_element():
    for n_markers in (12, 6):
        idx = list(range(12)) if n_markers == 12 else list(CONSTANTS.S_CONFIG_6)
        io = G.make_loss_case(3, 16, 3, n_markers, idx, 76, 'ragged', 'zeros', 0.1, seed=1)
        want = G.losses64(io)
        allow = G.losses_allowance(io, want)
        got = G.losses_torch(io, torch.float32)
        for k, at in (('loss_vals', (0, 2)),) + tuple((k, None) for k in G.COTANGENTS):
            w, a, g = want[k], allow[k], got[k]
            w, a, g = (t.reshape(-1, t.shape[-1]) for t in (w, a, g))
            if at is None:        # the first element that is not an exact zero (padding, a dropped frame, hat == gt)
                at = tuple(int(v) for v in (a > 0).nonzero()[0])
            _holds_and_catches('%s n%d' % (k, n_markers), g, w, a, at)
        # the generator's promises, on which the zero checks of the GPU test rest
        padding, dropped = G.dead_rows(io)
        assert padding.any() and dropped.any() and (~(padding | dropped)).any()
        assert (want['d_markers'][:, padding | dropped] == 0).all() and (want['d_pose'][:, padding] == 0).all()
        assert (io['pose_hist'] == io['pose_gt'][None]).any()


def test_bookkeeping_allowances_hold_an_fp32_evaluation_and_catch_one_planted_element():
    B, F, T = 5, 16, 80
    g = torch.Generator().manual_seed(2)
    rn = lambda *s: torch.randn(*s, generator=g)
    # cotangent step
    args = (B, F, 0, rn(T, 66), rn(T, 10), rn(T, 66), rn(T, 10), 50 * rn(T, 66), 50 * rn(T, 10), rn(T, 66), rn(T, 10), 0.1, 1)
    want, mag = G.cotangent_step64(*args), G.cotangent_step64(*args, magnitude=True)
    d_pose, d_shape, vp, vs, g_theta, g_beta, Dp, Ds = args[3:11]
    inv_T, step = torch.tensor(1.0 / T), torch.tensor(0.1)
    Dp32 = inv_T * g_theta + (vp + (d_pose + Dp))
    Ds32 = inv_T * g_beta + (vs + (d_shape + Ds))
    mean32 = Ds32.reshape(B, F, 10).sum(1, keepdim=True).div(F).expand(B, F, 10).reshape(T, 10)
    _holds_and_catches('Dp', Dp32, want[0], G.CHAIN_RUN * G.U * mag[0], (5, 17))
    _holds_and_catches('Ds', Ds32, want[1], G.CHAIN_RUN * G.U * mag[1], (5, 7))
    _holds_and_catches('dpad', step * Dp32, want[2], G.CHAIN_RUN * G.U * mag[2], (5, 17))
    _holds_and_catches('dspad', step * mean32, want[3], G.chain_mean(F) * G.U * mag[3], (5, 7))
    # additive update
    pose, dp, shape, ds = rn(T, 66), rn(T, 66), rn(T, 10), rn(T, 10)
    want = G.additive_update64(B, F, 0.1, 1, pose, dp, shape, ds)
    mag = G.additive_update64(B, F, 0.1, 1, pose, dp, shape, ds, magnitude=True)
    m32 = ds.reshape(B, F, 10).sum(1, keepdim=True).div(F).expand(B, F, 10).reshape(T, 10)
    _holds_and_catches('pose_next', step * dp + pose, want[0], G.CHAIN_NEXT * G.U * mag[0], (5, 17))
    _holds_and_catches('shape_next', step * m32 + shape, want[1], G.chain_next(F) * G.U * mag[1], (5, 7))
    # window mean
    _holds_and_catches('window mean', m32, G.window_mean64(ds, F), F * G.U * G.window_mean_magnitude(ds, F), (5, 7))
    # axpby
    x, y = rn(7, 37), rn(7, 37)
    _holds_and_catches('axpby', torch.tensor(0.3) * x + torch.tensor(-1.7) * y, G.axpby64(0.3, x, -1.7, y, x),
                       G.CHAIN_AXPBY * G.U * G.axpby64(0.3, x, -1.7, y, x, magnitude=True), (5, 17))
    # assemble: a copy
    x0 = rn(T, 72)
    assert torch.equal(G.assemble64(x0, pose, shape)[:, 72:138], pose)
