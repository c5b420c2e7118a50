"""
CPU tests of the per-element allowance that holds the training LSTM's reverse pass (tests/test_lstm_train_elementwise.py)
to float64: `elementwise.lstm_bptt_reference`, the sweep from the saved planes.  No GPU, nothing of the kernels.

  the oracle is right     fed the planes of a float64 forward it equals torch.nn.LSTM float64 autograd (packed ragged
                          sequences, h0 / c0 with requires_grad, loss (y * dy).sum(), dy non-zero on padded steps)
  not vacuous, not tight  a float32 torch evaluation of the same sweep from the same planes (the CONTROL: plain torch ops)
                          stays within half of every element's allowance at every shape of the GPU test
  it has teeth            the control with a fault injected fails the check, and the fault of one pre-activation gradient
                          off by 2^-12 stays invisible to the per-tensor bound 2e-5 max(1, max |ref|) it replaces
  one body                lstm_step_reference still returns the bits it returned before lstm_gates_reference shared its body

Worst err / allowance of the control per case and tensor group (dx | dW: w_ih and w_hh of all layers | db | state: d_h0 and
d_c0), as test_float32_control_stays_within_half_of_every_allowance prints it: 0.05 .. 0.36 over the fifteen shapes; per
case in the table of tests/test_lstm_train_elementwise.py, column `control`, next to what the kernels need.  The injected
faults, worst err / allowance: c0 dropped 7.6e5; one dG element off by 2^-12 (median magnitude of its row) 11.9, 34.5 and
2.2 at (5, 8, 8, 64, 2), (3, 4, 8, 256, 2), (65, 3, 8, 256, 2), where the per-tensor bound is used to 2 - 6 %; the last 16
recurrent terms dropped 2.7e4; dy of padded steps 1.1e8; b_hh of the other layer 1.3e6.
"""
import functools

import pytest
import torch

from tests import elementwise as E
from tests import test_lstm_train_driver as D

SHAPES = [(3, 4, 8, 256, 2), (4, 3, 8, 256, 2), (7, 3, 12, 256, 2), (12, 3, 8, 256, 1), (16, 3, 8, 256, 2),
          (17, 3, 8, 256, 2), (65, 3, 8, 256, 2), (65, 3, 8, 260, 1), (257, 2, 8, 256, 2), (705, 2, 8, 512, 2),
          (3, 4, 8, 16, 3), (5, 1, 8, 256, 2),
          # the shapes the allowance was prototyped at (longer sequences)
          (5, 8, 8, 64, 2), (65, 8, 8, 256, 2), (17, 6, 8, 260, 1)]
GAMMA = E.GAMMA_GEMM


def cpu_inputs(B, F, K, H, L, **kw):
    return D.inputs(B, F, K, H, L, dev='cpu', **kw)


def forward_planes(inp, dtype=torch.float64):
    """The training forward in plain torch at `dtype`: the flat save buffer (elementwise.lstm_save_planes) and the top
    layer's output, zero on padded steps; the state of a row is frozen past its length."""
    B, F, H, L = (inp[k] for k in 'BFHL')
    save = torch.zeros(L * E.LSTM_SAVE_PLANES * B * F * H, dtype=dtype)
    planes = E.lstm_save_planes(save, L, B, F, H)
    lens = torch.full((B,), F) if inp['lens'] is None else inp['lens'].long()
    layer_in = inp['x'].to(dtype)
    for l in range(L):
        w_ih, w_hh, b_ih, b_hh = (w.to(dtype) for w in inp['weights'][4 * l:4 * l + 4])
        h = torch.zeros(B, H, dtype=dtype) if inp['h0'] is None else inp['h0'][l].to(dtype)
        c = torch.zeros(B, H, dtype=dtype) if inp['c0'] is None else inp['c0'][l].to(dtype)
        out = torch.zeros(B, F, H, dtype=dtype)
        for t in range(F):
            live = (t < lens)[:, None]
            z = layer_in[:, t] @ w_ih.t() + h @ w_hh.t() + b_ih + b_hh
            i, f, g, o = torch.sigmoid(z[:, :H]), torch.sigmoid(z[:, H:2 * H]), torch.tanh(z[:, 2 * H:3 * H]), torch.sigmoid(z[:, 3 * H:])
            c_new = f * c + i * g
            h_new = o * torch.tanh(c_new)
            planes[l]['gates'][:, t] = torch.cat([i, f, g, o], dim=1)
            planes[l]['hprev'][:, t] = h
            c, h = torch.where(live, c_new, c), torch.where(live, h_new, h)
            planes[l]['c'][:, t] = c
            out[:, t] = torch.where(live, h_new, torch.zeros_like(h_new))
        planes[l]['y'][:] = out
        layer_in = out
    return save, layer_in


def over_rows(a, b, block=64):
    """A^T B (column sums of A without B), the rows in blocks of 64 whose partial results are added in order: the
    reductions over the B F rows are split over rows in the kernels too (csrc/gemm_atb.hip, atb_splits: a workgroup gets at
    least 64 rows), and 64 is the shortest range they hand out.  One product over all rows would leave the order, and with
    it the error of the longest chains, to the host BLAS and its thread count: the worst dW element of the 65 x 3 cases
    then moves between 0.44 and 0.51 of its allowance with 1, 8 or 16 threads."""
    acc = None
    for r0 in range(0, a.shape[0], block):
        part = a[r0:r0 + block].sum(0) if b is None else a[r0:r0 + block].t() @ b[r0:r0 + block]
        acc = part if acc is None else acc + part
    return acc


def control(inp, save, dtype=torch.float32, fault=None):
    """The reverse sweep in plain torch ops at `dtype` from the planes in `save`: values only, keys as
    lstm_bptt_reference.  `fault` injects one of the mistakes the allowance must catch:
      'c0'      c_prev = 0 instead of c0 at t = 0
      'dG'      one pre-activation gradient of the top layer times 1 + 2^-12: of the 4H of row 0 at the last step the one of
                median magnitude, a typical element and not a favourable one
      'k_tail'  the last 16 of the 4H terms of the recurrent product dropped
      'padded'  dy of a padded step taking part (it reaches the row's last live step as a carried dh)
      'b_hh'    b_hh's gradient taken from the other layer"""
    B, F, H, L = (inp[k] for k in 'BFHL')
    t_ = lambda v: v.to(dtype)
    planes = E.lstm_save_planes(save, L, B, F, H)
    lens = torch.full((B,), F) if inp['lens'] is None else inp['lens'].long()
    dy_l = t_(inp['dy'])
    out = dict(d_h0=torch.zeros(L, B, H, dtype=dtype), d_c0=torch.zeros(L, B, H, dtype=dtype))
    for l in range(L - 1, -1, -1):
        w_ih, w_hh = t_(inp['weights'][4 * l]), t_(inp['weights'][4 * l + 1])
        gates, c_all, hprev = (t_(planes[l][k]) for k in ('gates', 'c', 'hprev'))
        layer_in = t_(inp['x']) if l == 0 else t_(planes[l - 1]['y'])
        dG = torch.zeros(B, F, 4 * H, dtype=dtype)
        dc_in = torch.zeros(B, H, dtype=dtype)
        carry = torch.zeros(B, H, dtype=dtype)
        kk = 4 * H - 16 if fault == 'k_tail' else 4 * H
        for t in range(F - 1, -1, -1):
            live = (t < lens)[:, None]
            dh = dy_l[:, t]
            if t + 1 < F:
                dh = dh + dG[:, t + 1, :kk] @ w_hh[:kk]
            if fault == 'padded':
                dh = dh + carry
                carry = torch.where(live, torch.zeros_like(dh), dh)
            i, f, g, o = (gates[:, t, k * H:(k + 1) * H] for k in range(4))
            c_prev = c_all[:, t - 1] if t > 0 else t_(inp['c0'][l]) if inp['c0'] is not None and fault != 'c0' else torch.zeros_like(dc_in)
            tc = torch.tanh(c_all[:, t])
            d_o = dh * tc
            dc = dc_in + dh * o * (1 - tc * tc)
            step = torch.cat([dc * g * i * (1 - i), dc * c_prev * f * (1 - f), dc * i * (1 - g * g), d_o * o * (1 - o)], dim=1)
            if fault == 'dG' and l == L - 1 and t == F - 1:
                step[0, int(step[0].abs().argsort()[2 * H])] *= 1 + 2.0 ** -12
            dG[:, t] = torch.where(live, step, torch.zeros_like(step))
            dc_in = torch.where(live, dc * f, dc_in)
        out['d_c0'][l] = dc_in
        out['d_h0'][l] = dG[:, 0] @ w_hh
        rows = dG.reshape(B * F, 4 * H)
        out['w_ih%d' % l] = over_rows(rows, layer_in.reshape(B * F, -1))
        out['w_hh%d' % l] = over_rows(rows, hprev.reshape(B * F, -1))
        out['b_ih%d' % l] = over_rows(rows, None)
        out['b_hh%d' % l] = over_rows(rows, None)
        dy_l = (rows @ w_ih).view(B, F, -1)
    out['dx'] = dy_l
    if fault == 'b_hh':
        out['b_hh0'], out['b_hh1'] = out['b_hh1'], out['b_hh0']
    return out


def two_d(t):
    """check() classes 2-D outputs by tile position: [L][B][H] and [B][F][K] as rows of their last dimension."""
    return t.reshape(-1, t.shape[-1]) if t.dim() == 3 else t


def check_all(got, want, tol, keys=None):
    """E.check of every tensor: {key: Report}."""
    return {k: E.check(k, two_d(got[k]), two_d(want[k]), two_d(tol[k]), gamma=GAMMA) for k in (keys or want)}


def by_group(reports):
    """Worst ratio over dx | the dW | the db | the state cotangents."""
    groups = {'dx': ('dx',), 'dW': ('w_ih', 'w_hh'), 'db': ('b_ih', 'b_hh'), 'state': ('d_h0', 'd_c0')}
    return {g: max(r.worst for k, r in reports.items() if k.startswith(pre)) for g, pre in groups.items()}


@functools.lru_cache(maxsize=None)
def float32_case(B, F, K, H, L):
    """Inputs, the float32 planes of a float64 forward, and the reference from those planes: shared, left unchanged."""
    inp = cpu_inputs(B, F, K, H, L)
    save = forward_planes(inp)[0].float()
    return inp, save, E.lstm_bptt_reference(inp['weights'], inp['x'], inp['lens'], inp['c0'], save, inp['dy'], GAMMA)


# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,F,K,H,L', [(5, 6, 8, 32, 1), (5, 6, 8, 32, 2), (4, 5, 12, 20, 3)])
def test_reference_from_float64_planes_equals_float64_autograd(B, F, K, H, L):
    inp = cpu_inputs(B, F, K, H, L)
    assert int(inp['lens'].min()) < F and float(inp['dy'][inp['lens'].argmin(), F - 1].abs().min()) > 0   # dy on padded steps
    save, y = forward_planes(inp)
    val, _ = E.lstm_bptt_reference(inp['weights'], inp['x'], inp['lens'], inp['c0'], save, inp['dy'], GAMMA)

    ref = torch.nn.LSTM(K, H, L, batch_first=True).double()
    names = ('weight_ih_l%d', 'weight_hh_l%d', 'bias_ih_l%d', 'bias_hh_l%d')
    with torch.no_grad():
        for l in range(L):
            for k, name in enumerate(names):
                getattr(ref, name % l).copy_(inp['weights'][4 * l + k].double())
    x, h0, c0 = (inp[k].double().requires_grad_(True) for k in ('x', 'h0', 'c0'))
    packed = torch.nn.utils.rnn.pack_padded_sequence(x, inp['lens'].long(), batch_first=True, enforce_sorted=False)
    out, _ = ref(packed, (h0, c0))
    y_ref, _ = torch.nn.utils.rnn.pad_packed_sequence(out, batch_first=True, total_length=F)
    (y_ref * inp['dy'].double()).sum().backward()
    want = dict(dx=x.grad, d_h0=h0.grad, d_c0=c0.grad)
    for l in range(L):
        for key, name in zip(D.WEIGHT_KEYS, names):
            want['%s%d' % (key, l)] = getattr(ref, name % l).grad
    y_ref = y_ref.detach()
    assert float((y - y_ref).abs().max()) <= 1e-12 * float(y_ref.abs().max())
    assert val.keys() == want.keys()
    for key, b in want.items():
        assert float((val[key] - b).abs().max()) <= 1e-12 * float(b.abs().max()), key


@pytest.mark.parametrize('B,F,K,H,L', SHAPES)
def test_float32_control_stays_within_half_of_every_allowance(B, F, K, H, L):
    inp, save, (val, tol) = float32_case(B, F, K, H, L)
    reports = check_all(control(inp, save), val, tol)
    print('control (%d, %d, %d, %d, %d): ' % (B, F, K, H, L)
          + '  '.join('%s %.2f' % kv for kv in by_group(reports).items()))
    for key, r in reports.items():
        print('  ' + r.message)
        assert r.worst <= 0.5, r.message
        assert float(tol[key].min()) >= 0 and torch.isfinite(tol[key]).all(), key


@pytest.mark.parametrize('fault,shape', [('c0', (5, 8, 8, 64, 2)), ('dG', (5, 8, 8, 64, 2)), ('dG', (3, 4, 8, 256, 2)), ('dG', (65, 3, 8, 256, 2)),
                                         ('k_tail', (17, 6, 8, 260, 1)), ('k_tail', (65, 3, 8, 260, 1)),
                                         ('padded', (5, 8, 8, 64, 2)), ('b_hh', (5, 8, 8, 64, 2))])
def test_injected_fault_fails_the_check(fault, shape):
    inp, save, (val, tol) = float32_case(*shape)
    assert all(r.ok for r in check_all(control(inp, save), val, tol).values())      # the control itself passes
    bad = control(inp, save, fault=fault)
    reports = check_all(bad, val, tol)
    failed = sorted(k for k, r in reports.items() if not r.ok)
    print('%s at %s: over the allowance in %s; worst %s' % (fault, shape, failed, '  '.join('%s %.2f' % kv for kv in by_group(reports).items())))
    assert failed, fault
    if fault == 'dG':
        # the gap this closes: the bound of test_lstm_train_driver.py::test_every_output_matches_float64_lstm does not see it
        for key, b in val.items():
            err = float((bad[key].double() - b).abs().max())
            assert err < 2e-5 * max(1.0, float(b.abs().max())), key


def test_step_reference_keeps_its_bits_and_the_gates_reference_shares_them():
    """lstm_step_reference as it stood before the shared body (copied here, the parent's lines), on one random case."""
    def parent(w_ih, w_hh, bias, x, h, c, gamma, e_x=None, e_h=None, e_c=None):
        U, propagate, sigmoid_finish, tanh_finish = E.U, E.propagate, E.sigmoid_finish, E.tanh_finish
        x, h, c = (t.detach().double() for t in (x, h, c))
        w_ih, w_hh, bias = (t.detach().double().to(x.device) for t in (w_ih, w_hh, bias))
        H = w_hh.shape[1]
        z = x @ w_ih.t() + h @ w_hh.t() + bias
        ez = gamma * U * (x.abs() @ w_ih.abs().t() + h.abs() @ w_hh.abs().t() + bias.abs())
        if e_x is not None:
            ez = ez + propagate(e_x, w_ih)
        if e_h is not None:
            ez = ez + propagate(e_h, w_hh)
        zi, zf, zg, zo = (z[:, k * H:(k + 1) * H] for k in range(4))
        ei, ef, eg, eo = (ez[:, k * H:(k + 1) * H] for k in range(4))
        i, f, g, o = torch.sigmoid(zi), torch.sigmoid(zf), torch.tanh(zg), torch.sigmoid(zo)
        ei, ef, eo = (0.25 * e + sigmoid_finish(zz) for e, zz in ((ei, zi), (ef, zf), (eo, zo)))
        eg = eg + tanh_finish(zg)
        c_new = f * c + i * g
        e_c_new = f.abs() * (0 if e_c is None else e_c) + c.abs() * ef + g.abs() * ei + i.abs() * eg \
            + gamma * U * ((f * c).abs() + (i * g).abs())
        tc = torch.tanh(c_new)
        h_new = o * tc
        e_h_new = tc.abs() * eo + o.abs() * (e_c_new + tanh_finish(c_new)) + gamma * U * h_new.abs()
        return h_new, c_new, e_h_new, e_c_new

    g = torch.Generator().manual_seed(7)
    rnd = lambda *shape: torch.randn(*shape, generator=g)
    B, K, H = 9, 12, 20
    args = (rnd(4 * H, K) / H ** 0.5, rnd(4 * H, H) / H ** 0.5, rnd(4 * H), rnd(B, K), rnd(B, H), rnd(B, H), 8)
    errs = dict(e_x=1e-6 * rnd(B, K).abs().double(), e_h=1e-6 * rnd(B, H).abs().double(), e_c=1e-6 * rnd(B, H).abs().double())
    for kw in ({}, errs):
        for a, b in zip(E.lstm_step_reference(*args, **kw), parent(*args, **kw)):
            assert torch.equal(a, b)
    full = E.lstm_gates_reference(*args)
    for a, b in zip(full[:4], parent(*args)):
        assert torch.equal(a, b)
    gates, e_gates = full[4:]
    assert gates.shape == e_gates.shape == (B, 4 * H) and float(e_gates.min()) > 0
    z = args[3].double() @ args[0].double().t() + args[4].double() @ args[1].double().t() + args[2].double()
    assert torch.equal(gates[:, 2 * H:3 * H], torch.tanh(z[:, 2 * H:3 * H])) and torch.equal(gates[:, :H], torch.sigmoid(z[:, :H]))
