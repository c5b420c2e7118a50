"""
CPU tests of the per-element allowances that hold the training update MLPs (tests/test_train_mlp_elementwise.py) to
float64: `elementwise.mlp_train_fwd_reference` and `elementwise.mlp_train_bwd_reference`, both sweeps from the saved
planes.  No GPU, nothing of the kernels.

  the oracle is right     fed the planes of a float64 forward, the reverse sweep equals float64 torch.autograd through
                          nn.Linear / BatchNorm1d (train) / PReLU with loss (out * d_out).sum(), in all three save layouts;
                          the forward oracle equals the modules' outputs and updated running statistics
  not vacuous, not tight  a float32 plain-torch evaluation of forward and sweep from the same planes (the CONTROL; its row
                          reductions in 64-row blocks added in order, layout 1 with k (M dy - dbeta - xh dgamma), layouts 2
                          and 3 with c1 dyh + c3 y + c0) stays within half of every element's allowance at every shape of
                          the GPU grid, and the undecided PReLU branches within 1e-4 of every plane
  it has teeth            the control with one fault injected fails the check; the dZ fault stays invisible to the per-tensor
                          bound 2e-5 max(1, max |ref|) that held these outputs before

Worst err / allowance of the control over the twenty shapes of the grid and both networks, per tensor group, as
test_float32_control_stays_within_half_of_every_allowance prints it (per case in the table of
tests/test_train_mlp_elementwise.py, column `control`):
    planes 0.12 .. 0.50 | statistics 0.31 .. 0.49 | dZ 0.01 .. 0.17 | dW 0.06 .. 0.37 | db 0.04 .. 0.14 | dgamma, dbeta, dslope 0.04 .. 0.13
(planes and statistics reach 0.5 and no more by construction: `a` of layout 3, s and t are one to three roundings away
from saved numbers, each allowed one unit in the last place, `elementwise.ULP`.)  Accumulating onto random gradients:
dW 0.30, the rest unchanged.  Undecided branches: none at any shape of the grid with these seeds.
Two findings about the control, not the allowance: float32 products through `@` leave the order of the K terms to the host
BLAS, whose single chain per element reaches 4.8 u |a| |W|^T at K = 152, 0.60 of the allowance (`product`: torch.sum, 1.0 u);
and with u instead of one unit in the last place per elementwise rounding s = weight rstd, ONE rounding, sat at 0.91.
The forward's layout-1 `a` was at 0.36 .. 0.45 before its allowance got the term |weight| rstd u |mean| (the pass kernels'
unrounded mean, `mlp_train_fwd_reference`), 0.33 .. 0.41 after; the shifted form of `_bn_statistics` only widens columns
whose first row lies far from their mean and leaves the statistics' range, 0.31 .. 0.49, where it was.
The injected faults, worst err / allowance at 100 x 152 x 64 (the control itself: at most 0.46 there):
    one dZ element of the top hidden layer times 1 + 2^-12      15.1 (layouts 1 and 3), 29.7 at 384 x 296 x 512; the per-tensor
                                                                bound is used to 72 % and 44 % by it (most by db of the top
                                                                hidden layer, whose vectors of H get 1e-4 there)
    the wrong PReLU branch at one decided element               2.4e5
    dbeta missing one row                                       8.3e4
    dslope summing over y > 0 as well                           4.4e4
    the last 16 K-terms of one dX product dropped               2.0e5
    unbiased variance in rstd                                   6.0e3
    biased variance in running_var                              1.3e3
    accumulate ignored                                          7.9e6
    layout 2's a re-formed with the slope of the wrong layer    7.3e5
"""
import functools

import pytest
import torch

from tests import elementwise as E
from tests.test_lstm_bptt_bounds import over_rows

GAMMA = E.GAMMA_GEMM
EPS, MOMENTUM = 1e-5, 0.1
NET_SEED = 5

# (layout, M, in_dim, hidden, shift): every shape of the GPU test, once per formula (layout 1 serves the one-launch layers
# and the pass kernels alike); shift 3: the conditioning edge, x + 3
GRID = [(1, M, 152, 64, 0.0) for M in (2, 17, 100, 200, 384, 512, 700, 1024, 1064)] + \
       [(1, 100, 152, 96, 0.0), (1, 1064, 152, 96, 0.0), (1, 100, 296, 512, 0.0), (1, 384, 296, 512, 0.0),
        (2, 100, 152, 64, 0.0), (2, 384, 296, 512, 0.0), (3, 100, 152, 64, 0.0), (3, 1064, 152, 256, 0.0),
        (1, 1064, 152, 64, 3.0), (3, 1064, 152, 256, 3.0), (1, 512, 152, 64, 3.0)]
GROUPS = (('planes', ('pre', 'a', 'out')), ('statistics', ('mean', 'rstd', 's', 't', 'running_')),
          ('dZ', ('dZ', 'd_out')), ('dW', ('dW',)), ('db', ('db',)), ('dgamma, dbeta, dslope', ('dgamma', 'dbeta', 'dslope')))
UNDECIDED_MAX = 1e-4


def cpu_pair(in_dim, hidden, seed=NET_SEED):
    """The 66- and 10-output update networks of tests/test_hip_round5.py::_mlp_pair (same seeds, same draws), on the CPU."""
    from em_pose_amd.nn.layers import MLP
    torch.manual_seed(seed)
    nets = [MLP(in_dim, 66, hidden, num_layers=2), MLP(in_dim, 10, hidden, num_layers=2)]
    g = torch.Generator().manual_seed(seed + 1)
    for net in nets:
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                with torch.no_grad():
                    m.bias.copy_(0.3 * torch.randn(m.bias.shape, generator=g))
                    m.running_mean.copy_(0.1 * torch.randn(m.running_mean.shape, generator=g))
                    m.running_var.copy_(0.5 + torch.rand(m.running_var.shape, generator=g))
            if isinstance(m, torch.nn.PReLU):
                with torch.no_grad():
                    m.weight.fill_(0.1 + 0.3 * float(torch.rand(1, generator=g)))
    return [n.train() for n in nets]


def layers_of(net):
    """The dense layers as `elementwise` takes them, and the running statistics per hidden layer (clones)."""
    layers, running = [], []
    for lin, bn, act in net.dense_specs():
        layers.append({'w': lin.weight.detach().clone(), 'b': lin.bias.detach().clone(),
                       'bn': None if bn is None else (bn.weight.detach().clone(), bn.bias.detach().clone()),
                       'slope': None if act is None else act.weight.detach().clone()})
        if bn is not None:
            running.append((bn.running_mean.detach().clone(), bn.running_var.detach().clone()))
    return layers, running


def case_inputs(M, in_dim, shift=0.0, seed=None):
    """x [M][in_dim] (+ shift) and the padded cotangents of both outputs, padding columns zero; on the CPU."""
    g = torch.Generator().manual_seed(M + in_dim if seed is None else seed)
    x = torch.randn(M, in_dim, generator=g) + shift
    d_outs = [torch.zeros(M, 68), torch.zeros(M, 12)]
    d_outs[0][:, :66] = torch.randn(M, 66, generator=g)
    d_outs[1][:, :10] = torch.randn(M, 10, generator=g)
    return x, d_outs


def forward_planes(layers, x, layout, dtype=torch.float64):
    """The training forward in plain torch at `dtype`: (save buffer in `layout`, output)."""
    L, M, H = len(layers), x.shape[0], layers[0]['w'].shape[0]
    per_layer = (1 if layout == 2 else 2) * M * H + (2 if layout == 1 else 4) * H
    save = torch.zeros((L - 1) * per_layer, dtype=dtype)
    planes = E.mlp_train_save_planes(save, layout, L, M, H)
    h = x.to(dtype)
    for l, d in enumerate(layers):
        z = product(h, d['w'].to(dtype)) + d['b'].to(dtype)       # (no BLAS: its last bits depend on the machine, `product`)
        if d['bn'] is None:
            return save, z
        g, b = (t.to(dtype) for t in d['bn'])
        mean, var = z.mean(0), z.var(0, unbiased=False)
        rstd = 1.0 / torch.sqrt(var + E._f32(EPS))
        s = g * rstd
        t = b - mean * s
        y = g * ((z - mean) * rstd) + b if layout == 1 else s * z + t       # each layout in its kernels' own form
        h = torch.where(y > 0, y, d['slope'].to(dtype) * y)
        p = planes[l]
        p['pre'][:], p['mean'][:], p['rstd'][:] = z, mean, rstd
        if layout != 2:
            p['a'][:] = h
        if layout != 1:
            p['s'][:], p['t'][:] = s, t


def product(a, w):
    """a W^T in float32 with every element's K products added by torch.sum (vector lanes, then pairwise), the rows in chunks
    of at most 2^24 products.  A plain `a @ w.t()` leaves the order to the host BLAS, which chains the K terms of an element
    in one accumulator: at K = 152 its worst element is off by 4.8 u |a| |W|^T, 0.60 of the allowance, where this sum stays
    at 1.0 u |a| |W|^T -- and which order a BLAS takes depends on the machine and its thread count."""
    rows = max(1, (1 << 24) // (w.shape[0] * w.shape[1]))
    return torch.cat([(a[r0:r0 + rows, None, :] * w[None]).sum(-1) for r0 in range(0, a.shape[0], rows)])


def rows_product(a, b):
    """A^T B in float32: 64-row blocks added in order (`over_rows`, and why), every block summed by torch.sum."""
    acc = None
    for r0 in range(0, a.shape[0], 64):
        part = (a[r0:r0 + 64, :, None] * b[r0:r0 + 64, None, :]).sum(0)
        acc = part if acc is None else acc + part
    return acc


def control_forward(layers, x, save, layout, running, fault=None):
    """Every quantity of the forward in plain float32 torch ops from the saved quantities it is computed from, keys as
    mlp_train_fwd_reference.  Faults: 'var_unbiased' (rstd from the unbiased variance), 'running_biased' (running_var from
    the biased one), 'wrong_slope' (layout 2: a re-formed with the slope of the layer below the right one)."""
    L, M, H = len(layers), x.shape[0], layers[0]['w'].shape[0]
    planes = E.mlp_train_save_planes(save, layout, L, M, H)
    eps, mom = torch.tensor(EPS, dtype=torch.float32), torch.tensor(MOMENTUM, dtype=torch.float32)
    prelu = lambda y, slope: torch.where(y > 0, y, slope * y)
    out = {}
    for l, d in enumerate(layers):
        if l == 0:
            h = x.float()
        elif layout != 2:
            h = planes[l - 1]['a']
        else:
            slope = layers[l - 2 if fault == 'wrong_slope' and l >= 2 else l - 1]['slope']
            h = prelu(planes[l - 1]['s'] * planes[l - 1]['pre'] + planes[l - 1]['t'], slope)
        z = product(h, d['w']) + d['b']
        if d['bn'] is None:
            out['out'] = z
            break
        out['pre%d' % l] = z
        p = planes[l]
        z, ms, rs = p['pre'], p['mean'], p['rstd']
        g, b = d['bn']
        mean = over_rows(z, None) / M
        c = z - mean
        var = over_rows(c * c, None) / M
        unbiased = var * M / (M - 1) if M > 1 else var
        out['mean%d' % l] = mean
        out['rstd%d' % l] = 1.0 / torch.sqrt((unbiased if fault == 'var_unbiased' else var) + eps)
        if layout != 1:
            out['s%d' % l] = g * rs
            out['t%d' % l] = b - ms * out['s%d' % l]
        if layout == 1:
            out['a%d' % l] = prelu(g * ((z - ms) * rs) + b, d['slope'])
        elif layout == 3:
            out['a%d' % l] = prelu(p['s'] * z + p['t'], d['slope'])
        if running is not None:
            rm0, rv0 = running[l]
            out['running_mean%d' % l] = (1.0 - mom) * rm0 + mom * ms
            out['running_var%d' % l] = (1.0 - mom) * rv0 + mom * (var if fault == 'running_biased' else unbiased)
    return out


def control_backward(layers, x, save, layout, d_out, init=None, fault=None):
    """The reverse sweep in plain float32 torch ops from the planes in `save`, keys as mlp_train_bwd_reference; layout 1
    forms dZ as k (M dy - dbeta - xh dgamma), layouts 2 and 3 as c1 dyh + c3 y + c0.  Faults:
      'dZ'          one dZ element of the top hidden layer times 1 + 2^-12: of row 0 the one of median magnitude
      'branch'      the other PReLU branch at one clearly decided element of the top hidden layer (the largest |y| of row 0)
      'dbeta_row'   dbeta of the top hidden layer without its last row
      'dslope_pos'  dslope summing dA y over y > 0 as well
      'k_tail'      the last 16 of the H terms of the top hidden layer's dX product dropped
      'accumulate'  the initial gradient values ignored
      'wrong_slope' layout 2: a re-formed with the slope of the layer below the right one (the weight gradients read it)"""
    L, M, H = len(layers), x.shape[0], layers[0]['w'].shape[0]
    out_dim = layers[-1]['w'].shape[0]
    planes = E.mlp_train_save_planes(save, layout, L, M, H)
    prelu = lambda y, slope: torch.where(y > 0, y, slope * y)
    out = {'d_out': d_out.clone()}

    def put(key, v):
        out[key] = v + init[key] if init is not None and key in init and fault != 'accumulate' else v

    dY = d_out[:, :out_dim].float()
    for l in range(L - 1, -1, -1):
        if l == 0:
            h = x.float()
        elif layout != 2:
            h = planes[l - 1]['a']
        else:
            slope = layers[l - 2 if fault == 'wrong_slope' and l >= 2 else l - 1]['slope']
            h = prelu(planes[l - 1]['s'] * planes[l - 1]['pre'] + planes[l - 1]['t'], slope)
        put('dW%d' % l, rows_product(dY, h))
        put('db%d' % l, over_rows(dY, None))
        if l == 0:
            break
        w = layers[l]['w']
        top = l == L - 1          # this step holds the PReLU / BatchNorm reverse of the top hidden layer
        kk = w.shape[0] - 16 if fault == 'k_tail' and l == L - 2 else w.shape[0]
        dA = product(dY[:, :kk], w[:kk].t())
        j = l - 1
        p = planes[j]
        z, ms, rs = p['pre'], p['mean'], p['rstd']
        g, b = layers[j]['bn']
        slope = layers[j]['slope']
        xh = (z - ms) * rs
        y = g * xh + b if layout == 1 else p['s'] * z + p['t']
        pos = y > 0
        if fault == 'branch' and top:
            pos = pos.clone()
            c = int(y[0].abs().argmax())
            pos[0, c] = ~pos[0, c]
        dy = torch.where(pos, dA, slope * dA)
        term = dA * y if fault == 'dslope_pos' else torch.where(pos, torch.zeros_like(y), dA * y)
        put('dslope%d' % j, over_rows(term, None).sum().reshape(1))
        dbeta = over_rows(dy[:-1] if fault == 'dbeta_row' and top else dy, None)
        dgamma = over_rows(dy * xh, None)
        put('dbeta%d' % j, dbeta)
        put('dgamma%d' % j, dgamma)
        if layout == 1:
            dZ = (g * rs / M) * (M * dy - dbeta - xh * dgamma)
        else:
            c1 = g * rs
            c3 = -g * rs * rs * dgamma / M
            dZ = c1 * dy + (c3 * z + (-c1 * dbeta / M - c3 * ms))
        if fault == 'dZ' and l == L - 1:
            dZ[0, int(dZ[0].abs().argsort()[H // 2])] *= 1 + 2.0 ** -12
        out['dZ%d' % j] = dZ
        dY = dZ
    return out


def check_all(got, want, tol, keys=None, row_mod=64, col_mod=32):
    """E.check of every tensor (vectors as one row): {key: Report}."""
    two_d = lambda t: t.reshape(1, -1) if t.dim() == 1 else t
    return {k: E.check(k, two_d(got[k]), two_d(want[k]), two_d(tol[k]), gamma=GAMMA, row_mod=row_mod, col_mod=col_mod)
            for k in (keys or want)}


def by_group(reports):
    """Worst ratio over planes | statistics | dZ | dW | db | dgamma, dbeta, dslope (groups without a tensor left out)."""
    out = {}
    for name, prefixes in GROUPS:
        worst = [r.worst for k, r in reports.items() if k.startswith(prefixes)]
        if worst:
            out[name] = max(worst)
    return out


def init_grads(val, seed):
    """Random non-zero initial values for every gradient of a reverse sweep (accumulate = 1)."""
    g = torch.Generator().manual_seed(seed)
    return {k: torch.randn(v.shape, generator=g) for k, v in val.items() if not k.startswith(('dZ', 'd_out'))}


@functools.lru_cache(maxsize=None)
def float32_case(layout, M, in_dim, hidden, shift, net=0, accumulate=False):
    """Inputs, the float32 planes of a float64 forward in `layout`, and both references from those planes: shared, left
    unchanged."""
    layers, running = layers_of(cpu_pair(in_dim, hidden)[net])
    x, d_outs = case_inputs(M, in_dim, shift)
    save = forward_planes(layers, x, layout)[0].float()
    fwd = E.mlp_train_fwd_reference(layers, x, save, layout, GAMMA, EPS, MOMENTUM, running)
    init = None
    if accumulate:
        init = init_grads(E.mlp_train_bwd_reference(layers, x, save, layout, d_outs[net], GAMMA)[0], M)
    bwd = E.mlp_train_bwd_reference(layers, x, save, layout, d_outs[net], GAMMA, init=init)
    return dict(layers=layers, running=running, x=x, d_out=d_outs[net], save=save, fwd=fwd, bwd=bwd, init=init, layout=layout)


def run_control(c, fault=None):
    """{key: Report} of the control's forward and sweep on a `float32_case`."""
    got = control_forward(c['layers'], c['x'], c['save'], c['layout'], c['running'], fault)
    got.update(control_backward(c['layers'], c['x'], c['save'], c['layout'], c['d_out'], c['init'], fault))
    want, tol = dict(c['fwd'][0]), dict(c['fwd'][1])
    want.update(c['bwd'][0])
    tol.update(c['bwd'][1])
    assert got.keys() == want.keys()
    return got, check_all(got, want, tol)


# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('layout', [1, 2, 3])
@pytest.mark.parametrize('M,in_dim,hidden', [(9, 8, 12), (70, 12, 20)])
def test_references_from_float64_planes_equal_float64_autograd(M, in_dim, hidden, layout):
    nets = [n.double() for n in cpu_pair(in_dim, hidden)]
    x, d_outs = case_inputs(M, in_dim)
    for net, d_out in zip(nets, d_outs):
        layers, running = layers_of(net)
        out_dim = layers[-1]['w'].shape[0]
        save, out = forward_planes(layers, x, layout)
        val, tol = E.mlp_train_fwd_reference(layers, x, save, layout, GAMMA, EPS, MOMENTUM, running)
        g_val, g_tol, info = E.mlp_train_bwd_reference(layers, x, save, layout, d_out, GAMMA)
        assert max(info['undecided']) == 0.0

        h = x.double()
        for bn in (s[1] for s in net.dense_specs() if s[1] is not None):
            bn.eps, bn.momentum = E._f32(EPS), E._f32(MOMENTUM)
        pre, act_out = [], []
        for lin, bn, act in net.dense_specs():
            h = lin(h)
            if bn is not None:
                h.retain_grad()
                pre.append(h)
                h = act(bn(h))
                act_out.append(h)
        (h * d_out[:, :out_dim].double()).sum().backward()
        planes = E.mlp_train_save_planes(save, layout, len(layers), M, hidden)
        want = {'out': h.detach()}
        for l, (lin, bn, act) in enumerate(net.dense_specs()):
            want['dW%d' % l], want['db%d' % l] = lin.weight.grad, lin.bias.grad
            if bn is None:
                continue
            want['pre%d' % l], want['dZ%d' % l] = pre[l].detach(), pre[l].grad
            want['mean%d' % l] = pre[l].detach().mean(0)
            want['rstd%d' % l] = 1.0 / torch.sqrt(pre[l].detach().var(0, unbiased=False) + bn.eps)
            want['running_mean%d' % l], want['running_var%d' % l] = bn.running_mean, bn.running_var
            want['dgamma%d' % l], want['dbeta%d' % l], want['dslope%d' % l] = bn.weight.grad, bn.bias.grad, act.weight.grad
            if layout != 2:
                want['a%d' % l] = act_out[l].detach()
            assert int(bn.num_batches_tracked) == 1
        both = dict(val)
        both.update(g_val)
        for key, b in want.items():
            a = both[key]
            assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max())), key
        assert torch.equal(g_val['d_out'], d_out.double()) and float(g_tol['d_out'].abs().max()) == 0.0
        assert float((out - want['out']).abs().max()) <= 1e-12 * float(want['out'].abs().max())
        # the stash views and the save views address what MlpPlan lays out
        stash = torch.arange(M * ((len(layers) - 1) * hidden + d_out.shape[1]), dtype=torch.float64)
        slots = E.mlp_train_stash_planes(stash, len(layers), M, hidden, out_dim)
        assert [s.shape for s in slots] == [(M, hidden)] * (len(layers) - 1) + [d_out.shape]
        assert float(slots[-1][0, 0]) == M * (len(layers) - 1) * hidden and float(slots[1][0, 0]) == M * hidden
        assert planes[1]['pre'].data_ptr() - planes[0]['pre'].data_ptr() == 8 * save.numel() // (len(layers) - 1)


@pytest.mark.parametrize('layout,M,in_dim,hidden,shift', GRID)
def test_float32_control_stays_within_half_of_every_allowance(layout, M, in_dim, hidden, shift):
    for net in (0, 1):
        c = float32_case(layout, M, in_dim, hidden, shift, net)
        _, reports = run_control(c)
        info = c['bwd'][2]
        print('control layout %d %d x %d x %d shift %g net %d: %s; undecided branches %s'
              % (layout, M, in_dim, hidden, shift, net, '  '.join('%s %.2f' % kv for kv in by_group(reports).items()),
                 info['undecided_count']))
        assert max(info['undecided']) <= UNDECIDED_MAX, info['undecided']
        for tols in (c['fwd'][1], c['bwd'][1]):
            for key, t in tols.items():
                assert float(t.min()) >= 0 and torch.isfinite(t).all(), key
        for key, r in reports.items():
            assert r.worst <= 0.5, r.message


def test_float32_control_accumulating_stays_within_half_of_every_allowance():
    for layout in (1, 2, 3):
        c = float32_case(layout, 100, 152, 64, 0.0, 0, True)
        _, reports = run_control(c)
        print('control accumulating, layout %d: %s' % (layout, '  '.join('%s %.2f' % kv for kv in by_group(reports).items())))
        for key, r in reports.items():
            assert r.worst <= 0.5, r.message


FAULTS = [('dZ', (1, 100, 152, 64)), ('dZ', (3, 100, 152, 64)), ('dZ', (1, 384, 296, 512)), ('branch', (1, 100, 152, 64)),
          ('branch', (3, 100, 152, 64)), ('dbeta_row', (1, 100, 152, 64)), ('dslope_pos', (1, 100, 152, 64)),
          ('k_tail', (1, 100, 152, 64)), ('k_tail', (3, 100, 152, 64)), ('var_unbiased', (1, 100, 152, 64)),
          ('running_biased', (1, 100, 152, 64)), ('accumulate', (1, 100, 152, 64)), ('wrong_slope', (2, 100, 152, 64))]


@pytest.mark.parametrize('fault,shape', FAULTS)
def test_injected_fault_fails_the_check(fault, shape):
    c = float32_case(*shape, 0.0, 0, fault == 'accumulate')
    assert all(r.ok for r in run_control(c)[1].values())      # the control itself passes
    bad, reports = run_control(c, fault)
    failed = sorted(k for k, r in reports.items() if not r.ok)
    print('%s at %s: over the allowance in %s; worst %.3g' % (fault, shape, failed, max(r.worst for r in reports.values())))
    assert failed, fault
    if fault == 'dZ':
        # the gap this closes: the per-tensor bound of test_one_launch_train_layers_equal_the_layer_by_layer_path does not see it
        used, hidden = 0.0, shape[3]
        for key, b in c['bwd'][0].items():
            err = float((bad[key].double() - b).abs().max())
            rel = 1e-4 if b.ndim == 1 and b.numel() == hidden else 2e-5      # (as that test has it: vectors of H get 1e-4)
            used = max(used, err / (rel * max(1.0, float(b.abs().max()))))
        print('  the per-tensor bound 2e-5 max(1, max |ref|) is used to %.1f %%' % (100 * used))
        assert used < 1.0
