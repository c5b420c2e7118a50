"""
The row maxima of mlp_fused_x3_kernel<PAIR16> (csrc/mlp_fused_x3.hip, csrc/f16pair.h): every layer scales a row of its
results by a power of two chosen from the row's largest finite magnitude, which the epilogue finds across the lanes of a
row group (DPP exchanges), across the four waves (one LDS atomic maximum per lane) and, in layers split by K, across 16
adjacent lanes.  A maximum that misses one lane, one row or one wave scales the row's largest element past f16's range:
the row goes non-finite, or far outside its allowance.

Construction.  T = 8192 + 37 rows, the smallest count on the one-launch path (tests/test_mlp_pair16.py).  Row r of the
input carries ONE element 2^12 times the others, at column k(r) = 101 r mod 296; the first layer of either update net gets
a selector entry W0[c(k), k] += 32 / |s_c| (its other entries are below 0.06; s_c is the scale of the layer's BatchNorm for
that column) for every input column k, so the first hidden layer's output in row r is dominated by the single column
c(k(r)): by a factor of at least 8 -- asserted on the float64 values below -- where a factor above 4 already overflows (the
scale puts the largest element it SAW in [2^14, 2^15), f16 ends at 2^16).  The pose net takes c(k) = k mod hidden, the shape net c(k) = hidden - 1 - k mod hidden; both run the same code, a
workgroup per (64 rows, net), so over the two nets
  * every hidden column is the dominant one at least once (296 input columns reach 512 only from both ends), and
  * every pair (row position within the 64-row block, wave that owns the dominant column) occurs at least once
    (hidden 512: a wave owns 128 columns; k(64 b + p) walks 37 values 8 apart over the blocks b);
both are asserted on the index tables.  Hidden 512 is the maximum across lanes, waves and the LDS atomic; 128 and 64 split
every layer by K (16 adjacent lanes own a row).  One more case has the dominant input elements and NO selector: the raw
input's maximum (p16_stage) with the dominant element in each of the 16 lane positions of a row group (a lane owns the
16-byte chunks l + 16 u of a row: position (k / 4) mod 16).

Every output element of both nets is held to float64 through tests/elementwise.py at GAMMA_MLP = 4, the bar of
tests/test_mlp_pair16.py, and every output must be finite.

Measured on the MI355X, worst err / (u m) over both nets against the bar of 4, and the smallest factor by which the
dominant element leads its row (profiles/r13_gpu_tests_tail.log):
    dominant column, hidden 512     0.557      84
                     hidden 128     0.594      72
                     hidden 64      1.07       72
    dominant input element          0.361
"""
import pytest
import torch

from em_pose_amd import _lib, synthetic
from em_pose_amd.bodymodels.smpl import SMPLLayer
from em_pose_amd.helpers.configuration import lgd_config
from em_pose_amd.nn.models import create_model
from tests import elementwise as E
from tests import helpers as H
from tests.test_x3_shape16 import _update_nets_fwd

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GAMMA_MLP = 4
T_ROWS = 8192 + 37
K_IN = 296
DOMINANT = 2.0 ** 12
SELECTOR = 32.0
PREFIXES = ('pose_net_iter.', 'shape_net_iter.')


def _k_of_row():
    return (101 * torch.arange(T_ROWS)) % K_IN


def _c_of_k(hidden):
    """Per net: the hidden column that input column k selects."""
    k = torch.arange(K_IN) % hidden
    return [k, hidden - 1 - k]


def _net(hidden, selector):
    """A net of its own, built like tests.test_x3_shape16._update_net (whose cached nets stay as they are)."""
    from tests.test_hip_round5 import _randomize_bn
    torch.manual_seed(1300 + hidden)
    net = create_model(lgd_config(12, False, 1, hidden=hidden), SMPLLayer(H.small_model()))
    _randomize_bn(net, 13)
    net.vertex_ids = synthetic.small_vertex_ids(160)
    if selector:
        sd = net.state_dict()                             # (tensors that share the parameters' and buffers' memory)
        with torch.no_grad():
            for prefix, c in zip(PREFIXES, _c_of_k(hidden)):
                w0 = sd[prefix + 'input_to_hidden.weight']
                assert tuple(w0.shape) == (hidden, K_IN) and float(w0.abs().max()) < 0.06
                # the layer's BatchNorm scales column c by s_c, anything in (0, 1.5): the entry makes up for it
                s = sd[prefix + 'batch_norm.weight'] / torch.sqrt(sd[prefix + 'batch_norm.running_var'] + 1e-5)
                assert float(s.abs().min()) > 0.0
                w0[c, torch.arange(K_IN)] += SELECTOR / s.abs()[c]
    return net.to(DEV).eval()


def _inputs(hidden):
    g = torch.Generator().manual_seed(T_ROWS + 13 * hidden)
    x = torch.randn(T_ROWS, K_IN, generator=g)
    big = DOMINANT * (1.0 + 0.5 * torch.rand(T_ROWS, generator=g)) * (1.0 - 2.0 * (torch.arange(T_ROWS) % 2))
    x[torch.arange(T_ROWS), _k_of_row()] = big
    return x.to(DEV)


def _check(tag, net, xg):
    sd = {k: v.detach() for k, v in net.state_dict().items() if not k.startswith('smpl.')}
    layers = [E.eval_mlp_layers(sd, p) for p in PREFIXES]
    refs = [E.eval_mlp_reference(l, xg, GAMMA_MLP) for l in layers]
    try:
        _lib.lib().empose_reset_options()                 # the default form: two f16 pieces
        outs = _update_nets_fwd(net, xg)
    finally:
        _lib.lib().empose_reset_options()
    bad = []
    for name, got, (want, allow) in zip(('pose', 'shape'), outs, refs):
        r = E.check('update nets %s %s' % (tag, name), got, want, allow, GAMMA_MLP, col_mod=16)
        print(r.message.splitlines()[0])
        if not r.ok:
            bad.append(r.message)
        assert torch.isfinite(got).all(), (tag, name)
    assert not bad, '\n'.join(bad)
    return layers


@pytest.mark.parametrize('hidden', [512, 128, 64])
def test_one_dominant_hidden_column_per_row_in_every_lane_row_and_wave(hidden):
    k_of_row, c_of_k = _k_of_row(), _c_of_k(hidden)
    # the cases the construction promises, on the index tables
    dominant = torch.cat([c[k_of_row] for c in c_of_k])
    assert torch.equal(torch.unique(dominant), torch.arange(hidden))
    if hidden > 128:
        pos = (torch.arange(T_ROWS) % 64).repeat(2)
        assert torch.unique(pos * 4 + dominant // 128).numel() == 64 * 4
    net, xg = _net(hidden, True), _inputs(hidden)
    layers = _check('dominant column, hidden=%d' % hidden, net, xg)
    # ... and on the values: the first hidden layer's dominant element is at least 8 times any other of its row
    rows = torch.arange(T_ROWS, device=DEV)
    for d, c in zip(layers, c_of_k):
        d0 = d[0]
        s, mean, beta = (t.to(DEV) for t in d0['bn'])
        z = s * (xg.double() @ d0['w'].to(DEV).t() + d0['b'].to(DEV) - mean) + beta
        h1 = torch.where(z >= 0, z, d0['slope'].to(DEV) * z).abs()
        col = c[k_of_row].to(DEV)
        top = h1[rows, col].clone()
        h1[rows, col] = 0.0
        margin = float((top / h1.max(dim=1).values).min())
        print('hidden=%d: the dominant element over the largest other of its row, smallest over the rows: %.1f' % (hidden, margin))
        assert margin >= 8.0


def test_one_dominant_input_element_per_row_in_every_lane_of_the_staging_row_group():
    lane = (_k_of_row() // 4) % 16
    for p in range(4):                                    # (a thread stages rows rg, rg + 16, rg + 32, rg + 48 of a block)
        assert torch.unique(lane[(torch.arange(T_ROWS) % 64) // 16 == p]).numel() == 16
    _check('dominant input element', _net(512, False), _inputs(512))
