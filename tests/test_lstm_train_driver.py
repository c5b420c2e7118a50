"""
GPU tests of the training LSTM's host driver (csrc/api_lstm.hip: empose_lstm_train_fwd / empose_lstm_train_bwd), called
through the C ABI: what the pieces shared by the two forms of the reverse pass -- the save-buffer view, the cell builder, the
batched tail -- must keep, whichever recurrence runs.  Ragged lengths and a carried state throughout.

The shapes are the smallest that take each branch of the reverse pass (carve_train_lstm in api_lstm.hip,
rec_ksplit_applicable in gemm_rec.hip / gemm_fewrows_applicable in gemm_f32.hip; B rows, 4H = 1024 deep recurrent products
of H columns):
  wavefront, matrix-vector   L = 2, B <= 16 and 1024 <= 4H <= 2048 (rec_fewrows_reg_kernel)
  wavefront, K-split         L = 2, B > 16, 4 slices of 256 x (2 x 4 tiles of 64 x 64) = 32 workgroups, the lower bound
                             (rec_ksplit_kernel + rec_ksplit_reduce_kernel, two units of one and two K segments)
  layer form, the same two   L = 1 (the wavefront needs two layers): gemm_fewrows_kernel fused with the cell; the same
                             K-split kernel pair with one unit of one segment
  layer form, partial slice  H = 260 (4H is no multiple of 256, so no wavefront either): K = 1040 is five slices, the last
                             16 wide; five column tiles, the last 4 wide; a second row tile of one row -- the slice mask and
                             both tile edges of the K-split pair
  layer form, plain GEMM     4H = 64: one K slice and fewer than 1024 deep, neither special product applies
Every output of every case is also held to torch.nn.LSTM in float64 (test_every_output_matches_float64_lstm).
"""
import ctypes as C
import functools

import pytest
import torch

from em_pose_amd import _lib

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

CASES = [pytest.param(5, 4, 8, 256, 2, id='wavefront_matrix_vector'),
         pytest.param(65, 3, 8, 256, 2, id='wavefront_ksplit'),
         pytest.param(5, 4, 8, 256, 1, id='layers_fused_matrix_vector_cell'),
         pytest.param(65, 3, 8, 256, 1, id='layers_ksplit_cell'),
         pytest.param(65, 3, 8, 260, 1, id='layers_ksplit_partial_slice'),
         pytest.param(3, 4, 8, 16, 3, id='layers_plain_gemm')]
PLANES = 7      # of [B][F][H] per layer in the save buffer: gates x 4, cell state, incoming hidden state, layer output
WEIGHT_KEYS = ('w_ih', 'w_hh', 'b_ih', 'b_hh')


@functools.lru_cache(maxsize=None)
def inputs(B, F, K, H, L, lens='ragged', state=True, dev=DEV):
    """The tensors of a case, the same draws whatever the options.  `lens`: 'ragged' (row 0 reaches F), 'short' (no row
    does: at most F - 1) or None (no seq_lengths); `state` False: neither h0 nor c0; `dev`: where the tensors live."""
    g = torch.Generator().manual_seed(1000 * B + 100 * F + H + L)
    rnd = lambda *shape: torch.randn(*shape, generator=g)
    drawn = torch.randint(1, F + 1, (B,), generator=g, dtype=torch.int32)
    drawn[0] = F
    if lens == 'short':
        drawn = torch.clamp(drawn, max=F - 1)
    weights = [(rnd(*shape) / H ** 0.5).to(dev) for l in range(L)
               for shape in ((4 * H, K if l == 0 else H), (4 * H, H), (4 * H,), (4 * H,))]
    x, h0, c0, dy = rnd(B, F, K), 0.5 * rnd(L, B, H), 0.5 * rnd(L, B, H), rnd(B, F, H)
    return dict(B=B, F=F, K=K, H=H, L=L, x=x.to(dev), lens=None if lens is None else drawn.to(dev),
                h0=h0.to(dev) if state else None, c0=c0.to(dev) if state else None, dy=dy.to(dev), weights=weights)


def _params(inp):
    p = _lib.LstmParams()
    p.num_layers, p.input_size, p.hidden_size = inp['L'], inp['K'], inp['H']
    for l in range(inp['L']):
        p.w_ih[l], p.w_hh[l], p.b_ih[l], p.b_hh[l] = [inp['weights'][4 * l + k].data_ptr() for k in range(4)]
    return p


def _workspace(p, B, F):
    nbytes = _lib.lib().empose_lstm_train_workspace_bytes(C.byref(p), B, F)
    return torch.empty(nbytes, dtype=torch.uint8, device=DEV), nbytes


def forward(inp):
    """empose_lstm_train_fwd into fresh buffers (the save buffer zeroed: the top layer's output plane is never written)."""
    lib, p = _lib.lib(), _params(inp)
    B, F, K, H, L = (inp[k] for k in 'BFKHL')
    out = dict(y=torch.empty(B, F, H, device=DEV), h_n=torch.empty(L, B, H, device=DEV), c_n=torch.empty(L, B, H, device=DEV),
               save=torch.zeros(lib.empose_lstm_train_save_floats(L, B, F, H), device=DEV))
    ws, nbytes = _workspace(p, B, F)
    _lib.check(lib.empose_lstm_train_fwd(C.byref(p), B, F, _lib.dptr(inp['x']), inp.get('ldx', K), _lib.dptr(inp['lens']),
                                         _lib.dptr(inp['h0']), _lib.dptr(inp['c0']), _lib.dptr(out['y']), _lib.dptr(out['h_n']),
                                         _lib.dptr(out['c_n']), _lib.dptr(out['save']), _lib.dptr(ws), nbytes,
                                         _lib.current_stream()))
    torch.cuda.synchronize()
    return out


def backward(inp, save, optional=True):
    """empose_lstm_train_bwd into fresh buffers; `optional`: dx and the cotangents of the initial state are asked for."""
    lib, p, g = _lib.lib(), _params(inp), _lib.LstmGrads()
    B, F, K, H, L = (inp[k] for k in 'BFKHL')
    out = {}
    for l in range(L):
        for k, key in enumerate(WEIGHT_KEYS):
            out['%s%d' % (key, l)] = t = torch.empty_like(inp['weights'][4 * l + k])
            getattr(g, key)[l] = t.data_ptr()
    if optional:
        out.update(dx=torch.empty(B, F, K, device=DEV), d_h0=torch.empty(L, B, H, device=DEV),
                   d_c0=torch.empty(L, B, H, device=DEV))
        for l in range(L):
            g.d_h0[l], g.d_c0[l] = out['d_h0'][l].data_ptr(), out['d_c0'][l].data_ptr()
    ws, nbytes = _workspace(p, B, F)
    _lib.check(lib.empose_lstm_train_bwd(C.byref(p), B, F, _lib.dptr(inp['x']), inp.get('ldx', K), _lib.dptr(inp['lens']),
                                         _lib.dptr(inp['c0']),
                                         _lib.dptr(save), _lib.dptr(inp['dy']), _lib.dptr(out.get('dx')), C.byref(g),
                                         _lib.dptr(ws), nbytes, _lib.current_stream()))
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def first_run(B, F, K, H, L):
    """One forward and one reverse pass with every optional output, shared by the tests of a case and left unchanged."""
    inp = inputs(B, F, K, H, L)
    fwd = forward(inp)
    return fwd, backward(inp, fwd['save'])


def _assert_same_bits(a, b):
    assert a.keys() == b.keys()
    for key in a:
        assert torch.isfinite(a[key]).all(), key
        assert torch.equal(a[key], b[key]), key


@pytest.mark.parametrize('B,F,K,H,L', CASES)
def test_optional_outputs_do_not_perturb_the_weight_gradients(B, F, K, H, L):
    """dx, d_h0 and d_c0 requested or all null: every dW and db bit-identical, and finite."""
    fwd, full = first_run(B, F, K, H, L)
    bare = backward(inputs(B, F, K, H, L), fwd['save'], optional=False)
    assert len(bare) == 4 * L
    _assert_same_bits(bare, {k: full[k] for k in bare})


@pytest.mark.parametrize('B,F,K,H,L', CASES)
def test_reverse_pass_reads_the_save_buffer_the_forward_wrote(B, F, K, H, L):
    """Forward then backward twice from the same inputs into fresh buffers: all outputs bit-identical.  And on the host:
    the output sequence of layer l -- plane `y` of its record in `save`, which the reverse pass reads as the input rows of
    layer l + 1 (the caller's y for the top layer) -- is the layer's own hidden state, so it equals plane `hprev` of the
    same record one step later, on rows within their length."""
    inp = inputs(B, F, K, H, L)
    fwd, bwd = first_run(B, F, K, H, L)
    fwd2 = forward(inp)
    _assert_same_bits(fwd, fwd2)
    _assert_same_bits(bwd, backward(inp, fwd2['save']))
    save = fwd['save'].view(L, PLANES, B, F, H).cpu()
    live_next = (torch.arange(1, F)[None, :] < inp['lens'].cpu()[:, None])    # [B][F - 1]: step t + 1 is within the row
    for l in range(L):
        y_l = save[l, 6] if l < L - 1 else fwd['y'].cpu()
        assert torch.equal(y_l[:, :-1][live_next], save[l, 5][:, 1:][live_next]), l
        assert torch.equal(save[l, 5][:, 0], inp['h0'][l].cpu()), l


@pytest.mark.parametrize('B,F,K,H,L', CASES[:2])
def test_wavefront_stays_within_tolerance_of_layer_after_layer(B, F, K, H, L):
    """Option bptt_wave = 0 on the two wavefront shapes: the tolerance of
    test_hip_round3.py::test_reverse_lstm_wavefront_equals_layer_after_layer (another summation order)."""
    fwd, wave = first_run(B, F, K, H, L)
    with _lib.option('bptt_wave', 0):
        layers = backward(inputs(B, F, K, H, L), fwd['save'])
    for key, a in layers.items():
        assert torch.isfinite(wave[key]).all(), key
        torch.testing.assert_close(wave[key], a, atol=2e-5 * max(1.0, float(a.abs().max())), rtol=1e-4, msg=key)


@functools.lru_cache(maxsize=None)
def float64_lstm(B, F, K, H, L):
    """torch.nn.LSTM in float64 on the CPU from the same inputs: packed sequences, the carried state with requires_grad,
    the loss (y * dy).sum() (the construction of test_hip_round5.py's training test).  Keys as in forward() / backward()."""
    inp = inputs(B, F, K, H, L)
    cpu64 = lambda t: t.double().cpu()
    ref = torch.nn.LSTM(K, H, L, batch_first=True).double()
    names = ('weight_ih_l%d', 'weight_hh_l%d', 'bias_ih_l%d', 'bias_hh_l%d')
    with torch.no_grad():
        for l in range(L):
            for k, name in enumerate(names):
                getattr(ref, name % l).copy_(cpu64(inp['weights'][4 * l + k]))
    x, h0, c0 = (cpu64(inp[k]).requires_grad_(True) for k in ('x', 'h0', 'c0'))
    packed = torch.nn.utils.rnn.pack_padded_sequence(x, inp['lens'].cpu().long(), batch_first=True, enforce_sorted=False)
    out, (h_n, c_n) = ref(packed, (h0, c0))
    y, _ = torch.nn.utils.rnn.pad_packed_sequence(out, batch_first=True, total_length=F)
    (y * cpu64(inp['dy'])).sum().backward()
    want = dict(y=y.detach(), h_n=h_n.detach(), c_n=c_n.detach(), dx=x.grad, d_h0=h0.grad, d_c0=c0.grad)
    for l in range(L):
        for key, name in zip(WEIGHT_KEYS, names):
            want['%s%d' % (key, l)] = getattr(ref, name % l).grad
    return want


@pytest.mark.parametrize('B,F,K,H,L', CASES)
def test_every_output_matches_float64_lstm(B, F, K, H, L):
    """y, h_n, c_n, dx, d_h0, d_c0 and every dW / db of the first run against torch.nn.LSTM in float64, whichever recurrence
    ran: at most 2e-5 * max(1, max |reference|) per tensor, the bound of
    test_hip_round5.py::test_lstm_training_forward_of_a_few_rows_and_its_reverse_equal_the_small_batch_kernels.
    (Measured when the test was written: the worst tensor, dW_ih of layer 0, uses 2.1 % of its bound.)"""
    fwd, bwd = first_run(B, F, K, H, L)
    got = dict(bwd, **{k: fwd[k] for k in ('y', 'h_n', 'c_n')})
    want = float64_lstm(B, F, K, H, L)
    assert got.keys() == want.keys()
    for key, b in want.items():
        err = float((got[key].double().cpu() - b).abs().max())
        bound = 2e-5 * max(1.0, float(b.abs().max()))
        print('%s: worst error %.3e, bound %.3e' % (key, err, bound))
        assert err < bound, key
