"""
Per-element error allowances for the kernels that form fp32 products on the bf16 matrix cores (three bf16 pieces per
operand, csrc/bf16x3.h) and for the fp32 GEMM family they are compared against (csrc/gemm_f32.hip, `gemm_reference`),
and the check that holds an output to them.

A global tolerance lets one wrong element hide below the worst honest rounding error of the whole output.  Here every
output element gets its own allowance from a float64 MAGNITUDE `m` -- the same operation evaluated on absolute values --
as `gamma * u * m` with u = 2^-24 and one constant gamma per kernel family, carried through the layers of a network as a
running bound (PReLU, sigmoid and tanh are Lipschitz; the errors of earlier layers pass a product root-sum-square,
`propagate`).  `check` reports the violations by
their position inside the kernels' tiles, (row mod 64, column mod 32) -- or mod 16 for the 16 x 16 x 32 instruction -- and
by coordinate for the mesh, so that a footprint such as one accumulator element of the MFMA (rows 5 / 37 of a 64-row
block, columns 16..31 of a 32-column tile) is recognisable from the failure message alone.

Everything here is float64 torch on whatever device the inputs are on; nothing needs a GPU.
"""
import collections

import torch

U = 2.0 ** -24


def _abs64(t):
    return t.detach().double().abs()


# ----------------------------------------------------------------------------------------------------------------------
# Linear / GEMM  y = A W^T + b
def linear_magnitude(a, w, b=None):
    m = _abs64(a) @ _abs64(w).t()
    return m if b is None else m + _abs64(b)


def propagate(e, w):
    """The error e (rows, K) of an input carried through y = x W^T, root-sum-square: sqrt(e^2 (W^2)^T).  The worst
    case |W| e grows about 5x per 512-wide layer (|W| row sums of the released initialisation) and is vacuous after
    two layers; the rounding errors of the layers below are independent of the signs of W, so their sum over K
    cancels like a random walk.  The local term of every layer stays the worst case gamma u m."""
    w = w.detach().double().to(e.device)
    return torch.sqrt((e * e) @ (w * w).t())


def linear_allowance(a, w, b, gamma, e_a=None):
    """|y - y64| <= gamma u (|A| |W|^T + |b|) (+ propagate(e_a, W) for an input that carries an error e_a)."""
    e = gamma * U * linear_magnitude(a, w, b)
    return e if e_a is None else e + propagate(e_a, w)


# ----------------------------------------------------------------------------------------------------------------------
# The fp32 GEMM family (csrc/gemm_f32.hip, v_mfma_f32_32x32x2_f32): the contract of empose_linear_f32_ex
#     C = act(scale (A W^T) + shift) (+ resid)
# act 0: none; act 1: PReLU(slope), the residual added AFTER it (skip connection of an MLP block); act 2: the residual
# added first, then ReLU (residual block).  One constant for the whole family, every kernel `launch_gemm` can pick, the
# strided split-K kernel and A^T B; measured values in the docstring of tests/test_gemm_elementwise.py.
GAMMA_GEMM = 8


def gemm_products(a, w):
    """(P, R) = (A W^T, sqrt(sum_k s_k^2)) in float64, s_k = sum_{j <= k} a_j w_j the partial sums of the k-ordered chain
    of each element: what every epilogue form of one shape shares.  K rank-one updates, no (M, N, K) tensor."""
    a, w = a.detach().double(), w.detach().double()
    s = torch.zeros(a.shape[0], w.shape[0], dtype=torch.float64, device=a.device)
    r2 = torch.zeros_like(s)
    for k in range(a.shape[1]):
        s.addr_(a[:, k], w[:, k])
        r2.addcmul_(s, s)
    return s, torch.sqrt(r2)


def gemm_reference(a, w, scale=None, shift=None, resid=None, act=0, slope=0.0, gamma=GAMMA_GEMM, products=None):
    """float64 result of the contract above and its per-element allowance
        gamma u L |scale| R  +  3 u (L (|scale| |P| + |shift|) + |resid|),
    P = A W^T, R = sqrt(sum_k s_k^2) over the partial sums s_k of the element's k-ordered chain (`gemm_products`),
    L = max(1, |slope|) for the PReLU (an error that moves an element across the kink still moves the result by at most
    L times itself), L = 1 otherwise (ReLU is 1-Lipschitz).

    Accumulation, root-sum-square: an fp32 chain rounds every partial sum s_k by at most u |s_k|, independently, so the
    roundings add like u sqrt(sum s_k^2) = u R.  Kernels that split K over waves or lanes (split-K, few-rows, A^T B's
    row splits) restart their partial sums and stay below the single chain.  Two coarser forms were measured on the
    MI355X first and do not fit under the family's cap of 8 with the factor 2 it keeps in hand: the worst case
    u |scale| |A| |W|^T of the three-piece families above (honest kernels reach 6.8 at elements whose terms align, among
    the 16 million of one case), and R averaged over the orders of k, sqrt(K (P^2 / 3 + Q / 6)) with Q = (A^2) (W^2)^T
    (5.2: the partial sums of single elements wander far from that average).
    Epilogue, worst case without gamma: the scale / shift, the slope product and the residual add round at most three
    times, each by u times a value the second term bounds."""
    p, r = gemm_products(a, w) if products is None else products
    f = lambda t: None if t is None else t.detach().double().to(p.device)
    scale, shift, resid = f(scale), f(shift), f(resid)
    z, m, acc = p, p.abs(), r
    if scale is not None:
        z, m, acc = z * scale, m * scale.abs(), acc * scale.abs()
    if shift is not None:
        z, m = z + shift, m + shift.abs()
    if act == 1:
        lip = max(1.0, abs(float(slope)))
        z, m, acc = torch.where(z >= 0, z, slope * z), lip * m, lip * acc
    if resid is not None:
        z, m = z + resid, m + resid.abs()
    if act == 2:
        z = torch.clamp(z, min=0.0)
    return z, gamma * U * acc + 3.0 * U * m


# ----------------------------------------------------------------------------------------------------------------------
# Update MLPs: Linear - BatchNorm - PReLU blocks, then a Linear (oracle/torch_ref.py::mlp_forward)
def eval_mlp_layers(sd, prefix, num_layers=2, eps=1e-5):
    """The dense layers of an eval-mode MLP in order: dicts of float64 weight, bias, BatchNorm (scale, mean, beta) or
    None, PReLU slope or None.  BatchNorm is the affine map s (z - mean) + beta, s = weight / sqrt(var + eps)."""
    def dense(lin, bn, act):
        d = {'w': sd[lin + 'weight'].double(), 'b': sd[lin + 'bias'].double(), 'bn': None, 'slope': None}
        if bn is not None:
            s = sd[bn + 'weight'].double() / torch.sqrt(sd[bn + 'running_var'].double() + eps)
            d['bn'] = (s, sd[bn + 'running_mean'].double(), sd[bn + 'bias'].double())
        if act is not None:
            d['slope'] = sd[act + 'weight'].double()
        return d
    out = [dense(prefix + 'input_to_hidden.', prefix + 'batch_norm.', prefix + 'activation_fn.')]
    for h in range(num_layers):
        base = prefix + 'hidden_layers.{}.layers.'.format(h)
        for k in range(2):
            out.append(dense(base + '{}.'.format(4 * k), base + '{}.'.format(4 * k + 1), base + '{}.'.format(4 * k + 2)))
    out.append(dense(prefix + 'hidden_to_output.', None, None))
    return out


def _prelu(y, slope):
    return torch.where(y >= 0, y, slope * y)


def eval_mlp_reference(layers, x, gamma, skip=False):
    """float64 output of the eval-mode MLP and its per-element allowance.  Layer by layer, with h the float64 activation,
    z = W h + b and the BatchNorm magnitude  m = |s| (|W| |h| + |b| + |mean|) + |beta|:
        e_l = max(1, |slope|) (|s| P(e_{l-1}, W) + gamma u m_l) + gamma u |h_l|,
    and for the output layer  e = P(e, W) + gamma u (|W| |h| + |b|), with P = `propagate`.  `skip`: the input of every
    hidden block (layer pairs (1, 2), (3, 4), ...) is added to its output, its allowance with it plus gamma u |sum|."""
    h = x.detach().double()
    e = torch.zeros_like(h)
    block_in = None
    for l, d in enumerate(layers):
        if skip and l % 2 == 1 and l < len(layers) - 1:
            block_in = (h, e)
        w, b = d['w'].to(h.device), d['b'].to(h.device)
        z = h @ w.t() + b
        mag = linear_magnitude(h, w, b)
        prop = propagate(e, w)
        if d['bn'] is not None:
            s, mean, beta = (t.to(h.device) for t in d['bn'])
            z = s * (z - mean) + beta
            mag = s.abs() * (mag + mean.abs()) + beta.abs()
            prop = s.abs() * prop
        if d['slope'] is not None:
            slope = d['slope'].to(h.device)
            lip = torch.clamp(slope.abs(), min=1.0)
            h_new = _prelu(z, slope)
            e = lip * (prop + gamma * U * mag) + gamma * U * h_new.abs()
        else:
            h_new = z
            e = prop + gamma * U * mag
        if skip and l >= 2 and l % 2 == 0 and l < len(layers) - 1:
            h_new = h_new + block_in[0]
            e = e + block_in[1] + gamma * U * h_new.abs()
        h = h_new
    return h, e


def train_mlp_reference(layers, x, gamma, eps=1e-5):
    """Train-mode forward (BatchNorm over the batch with its own statistics, biased variance): float64 output and
    allowance.  `layers`: dicts of w, b, bn = (weight, bias) or None, slope.  z = W h + b gets
    propagate(e, W) + gamma u (|W| |h| + |b|).  Per BatchNorm layer, with z's allowance
    e_z, r = 1 / sqrt(var + eps) and xh = (z - mean) r:
        mean:      e_mu = sqrt(rowmean(e_z^2) / M) + gamma u rowmean(|z|)          (the statistics' own error)
        rstd:      |dr| / r <= r^2 (sqrt(rowmean((z - mean)^2 e_z^2) / M) + |mean| e_mu + gamma u rowmean(z^2))
    The statistics are sums over the M rows of errors that are independent from row to row: root-sum-square, as in
    `propagate` (the worst case, rowmean(e_z), triples the allowance at every layer and is vacuous at the output).
        xh:        e_xh = r (e_z + e_mu + gamma u (|z| + |mean|)) + |xh| |dr| / r
        affine:    e_y = |weight| e_xh + gamma u (|weight| |xh| + |bias|),  PReLU: max(1, |slope|), + gamma u |h|."""
    h = x.detach().double()
    e = torch.zeros_like(h)
    gu = gamma * U
    for d in layers:
        w, b = d['w'].to(h.device), d['b'].to(h.device)
        z = h @ w.t() + b
        ez = propagate(e, w) + gu * linear_magnitude(h, w, b)
        if d['bn'] is not None:
            bw, bb = (t.to(h.device) for t in d['bn'])
            mean, var = z.mean(0), z.var(0, unbiased=False)
            r = 1.0 / torch.sqrt(var + eps)
            xh = (z - mean) * r
            M = z.shape[0]
            e_mu = torch.sqrt((ez * ez).mean(0) / M) + gu * z.abs().mean(0)
            dr_rel = r * r * (torch.sqrt(((z - mean) ** 2 * ez * ez).mean(0) / M) + mean.abs() * e_mu + gu * (z * z).mean(0))
            e_xh = r * (ez + e_mu + gu * (z.abs() + mean.abs())) + xh.abs() * dr_rel
            z = xh * bw + bb
            ez = bw.abs() * e_xh + gu * (bw.abs() * xh.abs() + bb.abs())
        if d['slope'] is not None:
            slope = d['slope'].to(h.device)
            h = _prelu(z, slope)
            e = torch.clamp(slope.abs(), min=1.0) * ez + gu * h.abs()
        else:
            h, e = z, ez
    return h, e


# ----------------------------------------------------------------------------------------------------------------------
# LSTM: one step from a known state (gate order i, f, g, o)
def sigmoid_finish(z):
    """Absolute error of the kernels' sigmoid rcp(1 + __expf(-z)): __expf carries a relative error of (|z| + 4) u (the
    rounding of z log2(e) and v_exp_f32), which reaches the result times s (1 - s); the sum and v_rcp_f32 add 2 u s."""
    s = torch.sigmoid(z)
    return s * (1 - s) * (z.abs() + 4) * U + 2 * U * s


def tanh_finish(z):
    """Absolute error of the kernels' tanh 1 - 2 rcp(1 + __expf(2z)): the relative error (2|z| + 4) u of __expf reaches
    the result times (1 - t^2) / 2; the sum, v_rcp_f32 and the final subtraction add at most 3 u."""
    t = torch.tanh(z)
    return (1 - t * t) * (z.abs() + 2) * U + 3 * U


def _lstm_step(w_ih, w_hh, bias, x, h, c, gamma, e_x=None, e_h=None, e_c=None):
    """The one body of `lstm_step_reference` and `lstm_gates_reference`: (h', c', e_h', e_c', gates, e_gates), the gates
    activated, i | f | g | o along the columns."""
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
    return h_new, c_new, e_h_new, e_c_new, torch.cat([i, f, g, o], dim=1), torch.cat([ei, ef, eg, eo], dim=1)


def lstm_step_reference(w_ih, w_hh, bias, x, h, c, gamma, e_x=None, e_h=None, e_c=None):
    """One LSTM step in float64 from (x, h, c) and its allowance.  The pre-activations get the GEMM bound
    gamma u (|W_ih| |x| + |W_hh| |h| + |b|) plus propagate(e_x, W_ih) + propagate(e_h, W_hh); the gates Lipschitz 1/4 (sigmoid)
    and 1 (tanh) plus the finish terms of the approximate __expf / rcp (sigmoid_finish, tanh_finish -- stated, not folded
    into gamma); then
        e_c' = |f| e_c + |c| e_f + |g| e_i + |i| e_g + gamma u (|f c| + |i g|)
        e_h' = |tanh c'| e_o + |o| (e_c' + tanh_finish(c')) + gamma u |h'|.
    Returns (h', c', e_h', e_c') in float64."""
    return _lstm_step(w_ih, w_hh, bias, x, h, c, gamma, e_x, e_h, e_c)[:4]


def lstm_gates_reference(w_ih, w_hh, bias, x, h, c, gamma):
    """`lstm_step_reference` from an exact state, with what the training forward saves for the reverse pass returned as
    well: (h', c', e_h', e_c', gates, e_gates), the activated gates i | f | g | o as (rows, 4H) and their allowances."""
    return _lstm_step(w_ih, w_hh, bias, x, h, c, gamma)


# ----------------------------------------------------------------------------------------------------------------------
# Training LSTM: the save buffer of empose_lstm_train_fwd and back-propagation through time from it
LSTM_SAVE_PLANES = 7


def lstm_save_planes(save, L, B, F, H):
    """Views into the save buffer (csrc/api_lstm.hip, LstmSave), per layer: `gates` [B][F][4H] activated i | f | g | o,
    `c` [B][F][H] after every step, `hprev` [B][F][H] the hidden state before every step, `y` [B][F][H] the layer's output
    (the top layer's goes to the caller's y; its plane is never written)."""
    bfh = B * F * H
    rec = save.reshape(L, LSTM_SAVE_PLANES * bfh)
    return [dict(gates=rec[l, :4 * bfh].view(B, F, 4 * H), c=rec[l, 4 * bfh:5 * bfh].view(B, F, H),
                 hprev=rec[l, 5 * bfh:6 * bfh].view(B, F, H), y=rec[l, 6 * bfh:].view(B, F, H)) for l in range(L)]


def lstm_bptt_reference(weights, x, lens, c0, save, dy, gamma):
    """The reverse sweep of the training LSTM (empose_lstm_train_bwd) in float64 FROM THE SAVED PLANES, and one allowance
    per output element.  `weights`: (w_ih, w_hh, b_ih, b_hh) per layer, flat; x [B][F][K]; `lens` [B] or None; `c0`
    [L][B][H] or None; `save` the flat save buffer; dy [B][F][H] the cotangent of the top layer's output.  The planes are
    exactly what the kernels read (activated gates, c after every step, hprev, the output of the layer below as layer
    input), converted to float64: the forward's error is no part of this, the sweep is linear in dy, and what remains is
    the roundoff of the reverse kernels alone.
    Returns (values, allowances), dicts with keys dx [B][F][K], d_h0, d_c0 [L][B][H], w_ih<l>, w_hh<l>, b_ih<l>, b_hh<l>.

    The allowance is a running bound, u = 2^-24, P = `propagate` (root-sum-square through the products), the local term of
    every product the worst case gamma u |A| |W|.  Per layer, top down, t = F-1 .. 0 (rows with t >= len: dG = 0 exactly,
    e = 0, dc unchanged):
        dh  = dy_l[t] + dG[t+1] W_hh        e_dh = e_dy_l[t] + P(e_dG[t+1], W_hh^T) + gamma u |dG[t+1]| |W_hh| + u |dh|
        tc  = tanh(c_t)  e_tc = 4 u (tanhf) s2 = 1 - tc^2,  e_s2 = 2 |tc| e_tc + 2 u
        d_o = dh tc                         e_do = |tc| e_dh + |dh| e_tc + u |d_o|
        dc  = dc_in + dh o s2               e_dc = e_dc_in + |o s2| e_dh + |dh o| e_s2 + 3 u |dh o s2| + u |dc|
        dG_i = dc g i (1 - i)               e = |g i (1 - i)| e_dc + u |dc g i| + 4 u |dG_i|
        dG_f = dc c_prev f (1 - f)          e = |c_prev f (1 - f)| e_dc + u |dc c_prev f| + 4 u |dG_f|
        dG_g = dc i (1 - g^2)               e = |i (1 - g^2)| e_dc + 2 u |dc i| + 4 u |dG_g|
        dG_o = d_o o (1 - o)                e = |o (1 - o)| e_do + u |d_o o| + 4 u |dG_o|
        dc_in <- dc f                       e <- |f| e_dc + u |dc f|
    (c_prev = c0 at t = 0, 0 without one; the u |.| terms beside the 4 u |dG| are the rounding of 1 - i, 1 - f, 1 - g^2 and
    1 - o, each at most u, or 2 u with the square, times what multiplies it.)  After the loop, over the rows (b, t):
        dW   = dG^T In        e = sqrt((e_dG^2)^T In^2) + gamma u |dG|^T |In|   (In = x, the y plane below, or hprev)
        db   = sum dG         e = sqrt(sum e_dG^2) + gamma u sum |dG|            (b_ih and b_hh both)
        dx_l = dG W_ih        e = P(e_dG, W_ih^T) + gamma u |dG| |W_ih|          (the e_dy of the layer below)
        d_h0 = dG[0] W_hh     the same form;      d_c0 = the final dc_in with its e."""
    L = len(weights) // 4
    B, F, _ = x.shape
    H = dy.shape[2]
    dev = x.device
    d64 = lambda t: t.detach().double().to(dev)
    gu = gamma * U
    lens = torch.full((B,), F, dtype=torch.long, device=dev) if lens is None else lens.to(dev).long()
    planes = lstm_save_planes(save, L, B, F, H)
    dy_l, e_dy_l = d64(dy), torch.zeros(B, F, H, dtype=torch.float64, device=dev)
    val, tol = {}, {}
    val['d_h0'], tol['d_h0'] = (torch.zeros(L, B, H, dtype=torch.float64, device=dev) for _ in range(2))
    val['d_c0'], tol['d_c0'] = (torch.zeros(L, B, H, dtype=torch.float64, device=dev) for _ in range(2))
    for l in range(L - 1, -1, -1):
        w_ih, w_hh = d64(weights[4 * l]), d64(weights[4 * l + 1])
        gates, c_all, hprev = (d64(planes[l][k]) for k in ('gates', 'c', 'hprev'))
        layer_in = d64(x) if l == 0 else d64(planes[l - 1]['y'])
        dG = torch.zeros(B, F, 4 * H, dtype=torch.float64, device=dev)
        e_dG = torch.zeros_like(dG)
        dc_in = torch.zeros(B, H, dtype=torch.float64, device=dev)
        e_dc_in = torch.zeros_like(dc_in)
        product = lambda g, e, w: (g @ w, propagate(e, w.t()) + gu * (g.abs() @ w.abs()))
        for t in range(F - 1, -1, -1):
            live = (t < lens)[:, None]
            dh, e_dh = dy_l[:, t], e_dy_l[:, t]
            if t + 1 < F:
                rec, e_rec = product(dG[:, t + 1], e_dG[:, t + 1], w_hh)
                dh, e_dh = dh + rec, e_dh + e_rec
            e_dh = e_dh + U * dh.abs()
            i, f, g, o = (gates[:, t, k * H:(k + 1) * H] for k in range(4))
            c_prev = c_all[:, t - 1] if t > 0 else (torch.zeros_like(dc_in) if c0 is None else d64(c0[l]))
            tc = torch.tanh(c_all[:, t])
            e_tc = 4 * U
            s2 = 1 - tc * tc
            e_s2 = 2 * tc.abs() * e_tc + 2 * U
            d_o = dh * tc
            e_do = tc.abs() * e_dh + dh.abs() * e_tc + U * d_o.abs()
            dc = dc_in + dh * o * s2
            e_dc = e_dc_in + (o * s2).abs() * e_dh + (dh * o).abs() * e_s2 + 3 * U * (dh * o * s2).abs() + U * dc.abs()
            dGi = dc * g * i * (1 - i)
            dGf = dc * c_prev * f * (1 - f)
            dGg = dc * i * (1 - g * g)
            dGo = d_o * o * (1 - o)
            e_i = (g * i * (1 - i)).abs() * e_dc + U * (dc * g * i).abs() + 4 * U * dGi.abs()
            e_f = (c_prev * f * (1 - f)).abs() * e_dc + U * (dc * c_prev * f).abs() + 4 * U * dGf.abs()
            e_g = (i * (1 - g * g)).abs() * e_dc + 2 * U * (dc * i).abs() + 4 * U * dGg.abs()
            e_o = (o * (1 - o)).abs() * e_do + U * (d_o * o).abs() + 4 * U * dGo.abs()
            zero = torch.zeros_like(dc)
            dG[:, t] = torch.cat([torch.where(live, v, zero) for v in (dGi, dGf, dGg, dGo)], dim=1)
            e_dG[:, t] = torch.cat([torch.where(live, v, zero) for v in (e_i, e_f, e_g, e_o)], dim=1)
            dc_in, e_dc_in = torch.where(live, dc * f, dc_in), torch.where(live, f.abs() * e_dc + U * (dc * f).abs(), e_dc_in)
        val['d_c0'][l], tol['d_c0'][l] = dc_in, e_dc_in
        val['d_h0'][l], tol['d_h0'][l] = product(dG[:, 0], e_dG[:, 0], w_hh)
        rows, e_rows = dG.reshape(B * F, 4 * H), e_dG.reshape(B * F, 4 * H)
        for key, a in (('w_ih', layer_in), ('w_hh', hprev)):
            a = a.reshape(B * F, -1)
            val['%s%d' % (key, l)] = rows.t() @ a
            tol['%s%d' % (key, l)] = torch.sqrt((e_rows * e_rows).t() @ (a * a)) + gu * (rows.abs().t() @ a.abs())
        for key in ('b_ih', 'b_hh'):
            val['%s%d' % (key, l)] = rows.sum(0)
            tol['%s%d' % (key, l)] = torch.sqrt((e_rows * e_rows).sum(0)) + gu * rows.abs().sum(0)
        dx_l, e_dx_l = product(rows, e_rows, w_ih)
        dy_l, e_dy_l = dx_l.view(B, F, -1), e_dx_l.view(B, F, -1)
    val['dx'], tol['dx'] = dy_l, e_dy_l
    return val, tol


# ----------------------------------------------------------------------------------------------------------------------
# Training update MLPs: the save buffer and the stash of empose_mlp_train_fwd / _bwd*, and both sweeps from them
#
# Roundings of elementwise operations are counted one by one, each as v = 2 u = 2^-23, one unit in the last place of its
# result: twice what a correctly rounded fp32 operation can be off by.  A float32 evaluation with correctly rounded
# operations (the control of tests/test_train_mlp_bounds.py) therefore stays within half of such an allowance by
# construction and not by luck -- with u per operation a quantity that is ONE rounding away from its inputs (s = weight
# rstd) sits at up to 1.0 of its allowance in the control --, and an operation the device evaluates to one unit and not
# half of one (v_rcp_f32, v_rsq_f32, v_sqrt_f32, where a compiler picks them for a quotient or a root) is covered.  Products
# and column sums keep gamma u |A| |W|, gamma = GAMMA_GEMM.
ULP = 2.0 * U
def mlp_train_save_planes(save, layout, L, M, H):
    """Views into the save buffer of one network (csrc/api_train.hip, MlpPlan), one dict per hidden layer (L dense layers,
    L - 1 hidden):
        layout 1 (passes, one-launch layers)   pre = z [M][H] | a [M][H] | mean [H] | rstd [H]
        layout 2 (fused)                       pre = y [M][H] | mean | rstd | s | t
        layout 3 (epi)                         pre = y [M][H] | a [M][H] | mean | rstd | s | t
    `pre` is the layer's product + bias (called z in layout 1, y in the others), `a` its activation after BatchNorm and
    PReLU, s = gamma rstd and t = beta - mean s the affine form of the BatchNorm."""
    n_planes = 1 if layout == 2 else 2
    vecs = ('mean', 'rstd') if layout == 1 else ('mean', 'rstd', 's', 't')
    rec = save.reshape(L - 1, n_planes * M * H + len(vecs) * H)
    out = []
    for l in range(L - 1):
        d = {'pre': rec[l, :M * H].view(M, H)}
        if layout != 2:
            d['a'] = rec[l, M * H:2 * M * H].view(M, H)
        for k, name in enumerate(vecs):
            d[name] = rec[l, n_planes * M * H + k * H:n_planes * M * H + (k + 1) * H]
        out.append(d)
    return out


def mlp_train_stash_planes(stash, L, M, H, out_dim):
    """Views into the stash of one application (deferred weight gradients): dZ_l [M][H] of every hidden layer, then the
    copy of d_out [M][(out_dim + 3) & ~3]."""
    op = (out_dim + 3) & ~3
    return [stash[l * M * H:(l + 1) * M * H].view(M, H) for l in range(L - 1)] + \
        [stash[(L - 1) * M * H:(L - 1) * M * H + M * op].view(M, op)]


def _f32(v):
    """A host float as the kernels receive it (eps and momentum travel as float)."""
    return float(torch.tensor(float(v), dtype=torch.float32))


def _mlp_layer_input(layers, x, planes, layout, l):
    """(h, e_h): what layer l's product and its weight gradient read, in float64 from the saved numbers.  x for layer 0
    and the saved activation plane in layouts 1 and 3, both exact (e_h None).  Layout 2 stores no activation: every consumer
    re-forms a = PReLU(s y + t) in fp32 from the saved y, s, t; here in float64 with
        e_h = max(1, |slope|) v (|s y| + |s y + t|) + v |a|
    (the product and the sum round once each, the slope product once; PReLU is continuous, so an element whose fp32 sign
    differs still moves by at most its Lipschitz constant times the error)."""
    if l == 0:
        return x.detach().double(), None
    p = planes[l - 1]
    if layout != 2:
        return p['a'].detach().double(), None
    slope = layers[l - 1]['slope'].detach().double().to(x.device)
    sy = p['s'].detach().double() * p['pre'].detach().double()
    yh = sy + p['t'].detach().double()
    a = _prelu(yh, slope)
    return a, torch.clamp(slope.abs(), min=1.0) * ULP * (sy.abs() + yh.abs()) + ULP * a.abs()


def _bn_statistics(z, eps, gamma):
    """mean, biased variance and rstd of the columns of a float64 plane, with the allowances of `train_mlp_reference` for
    an exact plane (e_z = 0): e_mu = gamma u rowmean(|z|); half the variance's, the bracket of |dr| / r there,
    h = |mean| e_mu + gamma u rowmean(z^2).
    The three-pass BatchNorm of large batches (csrc/bn_prelu.hip, bn_stats_fwd_kernel / bn_combine_fwd_kernel) sums the
    plane SHIFTED by its first row, k = z[0]: d = sum(z - k) / M, mean = k + d, var = sum((z - k)^2) / M - d^2.  That is
    the same one-pass form on z - k, so its allowances are the same expressions on z - k (plus one rounding for k + d):
    e_mu' = gamma u rowmean(|z - k|) + v |mean|,  h' = |d| gamma u rowmean(|z - k|) + gamma u rowmean((z - k)^2).  Where the
    first row of a column lies far from the column's mean these exceed e_mu and h (measured on the MI355X at 1064 x 152 x 64:
    one rstd element at 1.005 of r^3 h + 3 v r); each statistic gets the larger of its two forms, which covers both paths.
    Returns (mean, var, r, e_mu, h)."""
    gu = gamma * U
    mean, var = z.mean(0), z.var(0, unbiased=False)
    e_mu = gu * z.abs().mean(0)
    half = mean.abs() * e_mu + gu * (z * z).mean(0)
    zk = z - z[0]
    e_d = gu * zk.abs().mean(0)
    half_k = (mean - z[0]).abs() * e_d + gu * (zk * zk).mean(0)
    return mean, var, 1.0 / torch.sqrt(var + eps), torch.maximum(e_mu, e_d + ULP * mean.abs()), torch.maximum(half, half_k)


def mlp_train_fwd_reference(layers, x, save, layout, gamma, eps=1e-5, momentum=0.1, running=None):
    """Everything the training forward of one update MLP writes (empose_mlp_train_fwd / _fwd_pair), each quantity in
    float64 FROM THE SAVED QUANTITIES THE KERNEL COMPUTED IT FROM, and one allowance per element: the error of the layers
    below is no part of a layer's check.  `layers`: dicts of w, b, bn = (weight, bias) or None, slope, as
    `train_mlp_reference`; `save` the flat save buffer in `layout`; `running`: per hidden layer (running_mean,
    running_var) as they were BEFORE the call, or None.  Returns (values, allowances), dicts with keys pre<l>, mean<l>,
    rstd<l>, s<l>, t<l> (layouts 2, 3), a<l> (layouts 1, 3), running_mean<l>, running_var<l> per hidden layer l, and out.
    num_batches_tracked is the caller's: exactly + 1.

    u = 2^-24, v = 2 u (above), P = `propagate`, r = 1 / sqrt(var + eps), in the order of a layer:
        pre   = h W^T + b                       e = gamma u (|h| |W|^T + |b|) + P(e_h, W)     (h, e_h: `_mlp_layer_input`)
        mean, var of the SAVED pre plane z      e_mu = gamma u rowmean(|z|)
                                                e_var = 2 h,  h = |mean| e_mu + gamma u rowmean(z^2)
                                                (each the larger of this and its form on the plane shifted by its first row,
                                                `_bn_statistics`)
        rstd  = r                               e = r^3 h + 3 v r              (the sum with eps, the root and the quotient)
        s     = weight rstd                     e = v |s|                                     (from the saved rstd)
        t     = bias - mean s                   e = |mean| e_s + v (|mean s| + |t|)           (from the saved mean and rstd)
        a     = PReLU(y), with y recomputed from the saved plane and the saved statistics as the kernel does:
                layout 1: y = weight ((z - mean) rstd) + bias     e_y = v (3 |weight xh| + |y|) + |weight| rstd u |mean|
                          (xh = (z - mean) rstd: the difference, two products, the sum.  The last term: bn_prelu_fwd_kernel
                          holds mean = sum (1 / M) in a register, and the compiler contracts that product into the
                          difference, z - sum (1 / M) with ONE rounding: the forward's mean is the unrounded product, up to
                          u |mean| from the saved one, the same for all rows of a column.  Measured on the MI355X without
                          the term: a few elements with |y| << |weight xh| of the pass kernels at M = 100, 200, 384, 700
                          up to 44 times over, columns apart, none at M = 512 and 1024 where 1 / M is a power of two and the
                          product exact.  The reverse kernels read the saved mean: their branch value has no such term.)
                layout 3: y = s z + t                             e_y = v (|s z| + |y|)
                                                e = max(1, |slope|) e_y + v |a|
        out   = h W^T + b  from the last saved activation, as pre
        running_mean' = (1 - m) running_mean + m mean             e = v (2 |(1 - m) running_mean| + |m mean| + |.'|)
        running_var'  = (1 - m) running_var + m var M / (M - 1)   e = m M / (M - 1) e_var + v (2 |(1 - m) running_var| +
                        3 |m var M / (M - 1)| + |.'|)
    (the fp32 difference 1 - m and its product round once each, m times the statistic once, the sum once; the unbiased
    variance two more; mean is the saved one, var the float64 one of the saved plane.)"""
    dev = x.device
    d64 = lambda t: t.detach().double().to(dev)
    gu = gamma * U
    L, M, H = len(layers), x.shape[0], layers[0]['w'].shape[0]
    eps, mom = _f32(eps), _f32(momentum)
    planes = mlp_train_save_planes(save, layout, L, M, H)
    val, tol = {}, {}
    for l in range(L):
        h, e_h = _mlp_layer_input(layers, x, planes, layout, l)
        w, b = d64(layers[l]['w']), d64(layers[l]['b'])
        key = 'out' if l == L - 1 else 'pre%d' % l
        val[key] = h @ w.t() + b
        tol[key] = gu * linear_magnitude(h, w, b) + (0 if e_h is None else propagate(e_h, w))
        if l == L - 1:
            break
        p = planes[l]
        z, ms, rs = d64(p['pre']), d64(p['mean']), d64(p['rstd'])
        bw, bb = (d64(t) for t in layers[l]['bn'])
        slope = d64(layers[l]['slope'])
        mean, var, r, e_mu, half = _bn_statistics(z, eps, gamma)
        val['mean%d' % l], tol['mean%d' % l] = mean, e_mu
        val['rstd%d' % l], tol['rstd%d' % l] = r, r ** 3 * half + 3 * ULP * r
        if layout != 1:
            s = bw * rs
            t = bb - ms * s
            val['s%d' % l], tol['s%d' % l] = s, ULP * s.abs()
            val['t%d' % l], tol['t%d' % l] = t, ms.abs() * ULP * s.abs() + ULP * ((ms * s).abs() + t.abs())
        if layout != 2:
            if layout == 1:
                gx = bw * ((z - ms) * rs)
                y = gx + bb
                e_y = ULP * (3 * gx.abs() + y.abs()) + bw.abs() * rs * U * ms.abs()
            else:
                sy = d64(p['s']) * z
                y = sy + d64(p['t'])
                e_y = ULP * (sy.abs() + y.abs())
            a = _prelu(y, slope)
            val['a%d' % l], tol['a%d' % l] = a, torch.clamp(slope.abs(), min=1.0) * e_y + ULP * a.abs()
        if running is not None:
            rm0, rv0 = (d64(t) for t in running[l])
            fac = M / (M - 1.0) if M > 1 else 1.0
            keep, new_m, new_v = 1.0 - mom, mom * ms, mom * var * fac
            val['running_mean%d' % l] = keep * rm0 + new_m
            tol['running_mean%d' % l] = ULP * (2 * (keep * rm0).abs() + new_m.abs() + val['running_mean%d' % l].abs())
            val['running_var%d' % l] = keep * rv0 + new_v
            tol['running_var%d' % l] = mom * fac * 2 * half + ULP * (2 * (keep * rv0).abs() + 3 * new_v.abs()
                                                                    + val['running_var%d' % l].abs())
    return val, tol


def mlp_train_wgrad_reference(rows, gamma, init=None):
    """dW = dY^T In and db = sum dY of one layer over the rows of every application in `rows`, a list of (dY, e_dY, In,
    e_In or None) -- float64 values and their allowances -- with
        e_dW = sqrt((e_dY^2)^T In^2) + sqrt((dY^2)^T e_In^2) + gamma u |dY|^T |In|
        e_db = sqrt(sum e_dY^2) + gamma u sum |dY|
    (sums over rows whose errors are independent from row to row: root-sum-square, the local term the worst case, as
    `lstm_bptt_reference` has them).  `init` = (dW0, db0): accumulate onto these, one more rounding, v |result|.
    Returns (dW, e_dW, db, e_db)."""
    gu = gamma * U
    dY, e_dY, a = (torch.cat([r[k] for r in rows], dim=0) for k in range(3))
    dW = dY.t() @ a
    e_dW = torch.sqrt((e_dY * e_dY).t() @ (a * a)) + gu * (dY.abs().t() @ a.abs())
    if rows[0][3] is not None:
        e_a = torch.cat([r[3] for r in rows], dim=0)
        e_dW = e_dW + torch.sqrt((dY * dY).t() @ (e_a * e_a))
    db = dY.sum(0)
    e_db = torch.sqrt((e_dY * e_dY).sum(0)) + gu * dY.abs().sum(0)
    if init is not None:
        dW, db = dW + init[0].detach().double().to(dW.device), db + init[1].detach().double().to(dW.device)
        e_dW, e_db = e_dW + ULP * dW.abs(), e_db + ULP * db.abs()
    return dW, e_dW, db, e_db


def mlp_train_bwd_reference(layers, x, save, layout, d_out, gamma, init=None, rows_only=False):
    """The reverse sweep of one training update MLP (empose_mlp_train_bwd / _bwd_deferred / _bwd_deferred_pair, and the
    products of empose_mlp_train_wgrad) in float64 FROM THE SAVED PLANES and d_out, with a running allowance per element.
    `d_out` [M][(out + 3) & ~3], its padding columns zero; `init`: {key: tensor} of the gradients' values before the call
    when it accumulates, else None.  Returns (values, allowances, info): keys d_out (the stash copy, exact), dZ<l>
    (the stash slots), dgamma<l>, dbeta<l>, dslope<l> per hidden layer, dW<l>, db<l> per layer; info['undecided'] the
    share of undecided PReLU branches per hidden layer, info['rows'] per layer the (dY, e_dY, In, e_In) that
    `mlp_train_wgrad_reference` takes (`rows_only`: no dW / db formed here: several applications).  There is no dx.

    Top down, dY = d_out with e = 0; per layer l (P = `propagate`, u = 2^-24, v = 2 u as above):
        dW_l, db_l        `mlp_train_wgrad_reference` from dY_l and the layer's input (`_mlp_layer_input`)
        dA = dY_l W_l     e_dA = P(e_dY, W_l^T) + gamma u |dY_l| |W_l|
    then the PReLU and BatchNorm reverse of layer j = l - 1 from its saved plane z, mean, rstd (and s, t):
        xh = (z - mean) rstd                    e_xh = 2 v |xh|                               (difference, product)
        the branch value, as the kernels recompute it in fp32 (layout 1 and the one-launch layers: csrc/bn_prelu.hip,
        csrc/train_cols.hip; layouts 2 and 3: csrc/train_epilogue.h):
          layout 1:    y = weight xh + bias     e_y = v (3 |weight xh| + |y|)
          layouts 2, 3: y = s z + t             e_y = v (|s z| + |y|)
        UNDECIDED where |y| <= e_y: the fp32 value may lie on the other side.  No element is left out:
        dy = dA (y > 0) or slope dA             e_dy = lip e_dA + v |dy| + [undecided] |1 - slope| |dA|,
                                                lip = 1 / |slope| by the branch, max(1, |slope|) where undecided
        dslope = sum_{y <= 0} dA y              per term |y| e_dA + |dA| e_y + v |dA y| (undecided: |dA| (|y| + e_y) more,
                                                the term either way); the sum over all M H terms as below
        dbeta  = sum dy                         e = sqrt(sum e_dy^2) + gamma u sum |dy|
        dgamma = sum dy xh                      per term |xh| e_dy + |dy| e_xh + v |dy xh|; e = sqrt(sum e^2) + gamma u sum |dy xh|
        dZ_j = weight rstd (dy - dbeta / M - xh dgamma / M)
    The kernels form dZ in two ways: k (M dy - dbeta - xh dgamma) with k = weight rstd / M (layout 1), and
    c1 dyh + c3 z + c0 with per-column coefficients on the UNCENTRED plane, c1 = weight rstd, c3 = -weight rstd^2 dgamma /
    M, c0 = -c1 dbeta / M - c3 mean (layouts 2, 3).  One allowance from magnitudes covers both, with
    sp = rstd (|z| + |mean|) >= |xh| where the second form does not centre:
        e_dZ = |weight| rstd (e_dy + e_dbeta / M + sp e_dgamma / M + |dgamma| e_xh / M)
               + 8 v |weight| rstd (|dy| + |dbeta| / M + sp |dgamma| / M)
    8: the longest chain of roundings on one term, c3 mean in c0 (four in c3, the product, the difference in c0, two sums);
    the first form has at most 6 (k two, M dy, xh dgamma, two differences -- and the product with k).
    Column sums are over M rows of errors that are independent from row to row: root-sum-square plus gamma u sum |.|.  The
    bias in front of a train-mode BatchNorm has a mathematically zero gradient; db_j's allowance is exactly that sum.
    Accumulating adds the initial value with one rounding, v |result|."""
    dev = x.device
    d64 = lambda t: t.detach().double().to(dev)
    gu = gamma * U
    L, M, H = len(layers), x.shape[0], layers[0]['w'].shape[0]
    out_dim = layers[-1]['w'].shape[0]
    planes = mlp_train_save_planes(save, layout, L, M, H)
    val, tol = {'d_out': d64(d_out)}, {'d_out': torch.zeros(d_out.shape, dtype=torch.float64, device=dev)}
    info = {'undecided': [0.0] * (L - 1), 'undecided_count': [0] * (L - 1), 'rows': [None] * L}

    def put(key, v, e):
        if init is not None and key in init:
            v = v + d64(init[key])
            e = e + ULP * v.abs()
        val[key], tol[key] = v, e

    dY = d64(d_out)[:, :out_dim]
    e_dY = torch.zeros_like(dY)
    for l in range(L - 1, -1, -1):
        h, e_h = _mlp_layer_input(layers, x, planes, layout, l)
        info['rows'][l] = (dY, e_dY, h, e_h)
        if not rows_only:
            seed = None if init is None or 'dW%d' % l not in init else (init['dW%d' % l], init['db%d' % l])
            val['dW%d' % l], tol['dW%d' % l], val['db%d' % l], tol['db%d' % l] = \
                mlp_train_wgrad_reference([info['rows'][l]], gamma, seed)
        if l == 0:
            break
        w = d64(layers[l]['w'])
        dA = dY @ w
        e_dA = propagate(e_dY, w.t()) + gu * (dY.abs() @ w.abs())
        j = l - 1
        p = planes[j]
        z, ms, rs = d64(p['pre']), d64(p['mean']), d64(p['rstd'])
        bw, bb = (d64(t) for t in layers[j]['bn'])
        slope = d64(layers[j]['slope'])
        xh = (z - ms) * rs
        e_xh = 2 * ULP * xh.abs()
        if layout == 1:
            gx = bw * xh
            y = gx + bb
            e_y = ULP * (3 * gx.abs() + y.abs())
        else:
            sy = d64(p['s']) * z
            y = sy + d64(p['t'])
            e_y = ULP * (sy.abs() + y.abs())
        undecided = y.abs() <= e_y
        pos = y > 0
        info['undecided_count'][j] = int(undecided.sum())
        info['undecided'][j] = info['undecided_count'][j] / float(y.numel())
        one, zero = torch.ones_like(y), torch.zeros_like(y)
        dy = torch.where(pos, dA, slope * dA)
        lip = torch.where(undecided, torch.clamp(slope.abs(), min=1.0) * one, torch.where(pos, one, slope.abs() * one))
        e_dy = lip * e_dA + ULP * dy.abs() + torch.where(undecided, (1 - slope).abs() * dA.abs(), zero)
        term = torch.where(pos, zero, dA * y)
        e_term = y.abs() * e_dA + dA.abs() * e_y + ULP * (dA * y).abs()
        e_term = torch.where(undecided, e_term + dA.abs() * (y.abs() + e_y), torch.where(pos, zero, e_term))
        put('dslope%d' % j, term.sum().reshape(1), (torch.sqrt((e_term * e_term).sum()) + gu * term.abs().sum()).reshape(1))
        dbeta = dy.sum(0)
        e_dbeta = torch.sqrt((e_dy * e_dy).sum(0)) + gu * dy.abs().sum(0)
        prod = dy * xh
        e_prod = xh.abs() * e_dy + dy.abs() * e_xh + ULP * prod.abs()
        dgamma = prod.sum(0)
        e_dgamma = torch.sqrt((e_prod * e_prod).sum(0)) + gu * prod.abs().sum(0)
        put('dbeta%d' % j, dbeta, e_dbeta)
        put('dgamma%d' % j, dgamma, e_dgamma)
        k = (bw * rs).abs()
        sp = rs * (z.abs() + ms.abs())
        dZ = bw * rs * (dy - dbeta / M - xh * dgamma / M)
        e_dZ = k * (e_dy + e_dbeta / M + sp * e_dgamma / M + dgamma.abs() * e_xh / M) \
            + 8 * ULP * k * (dy.abs() + dbeta.abs() / M + sp * dgamma.abs() / M)
        val['dZ%d' % j], tol['dZ%d' % j] = dZ, e_dZ
        dY, e_dY = dZ, e_dZ
    return val, tol, info


# ----------------------------------------------------------------------------------------------------------------------
# Full mesh: x3 against the fp32-instruction kernel
def mesh_magnitude(bm, pose_body, betas, root, trans=None):
    """Per vertex coordinate (n, V, 3), float64:
        sum_j w_vj (|R_j| (|v_t| + |S| |beta| + |P| |f|) + |t_j|) + |trans|
    with R_j, t_j the skinning transforms and f the pose features of the float64 evaluation (as magnitudes only).  Both
    kernels share the forward kinematics; what differs is the blend-shape contraction and the skinning sums after it.
    Memory: about 200 bytes per (frame, vertex); callers chunk the frames."""
    from oracle import torch_ref as R
    dt, dev = torch.float64, pose_body.device
    n = pose_body.shape[0]
    pose_body, betas, root = (t.detach().to(dt) for t in (pose_body, betas, root))
    v_t = bm.v_template.to(dev, dt)[0]                         # (V, 3)
    S = bm.shapedirs.to(dev, dt)                               # (V, 3, 10)
    P = bm.posedirs.to(dev, dt)                                # (459, V*3)
    Wt = bm.weights.to(dev, dt)                                # (V, 52)
    Jreg = bm.J_regressor.to(dev, dt)
    full_pose = torch.cat([root, pose_body, torch.zeros(n, 90, dtype=dt, device=dev)], dim=1)
    v_shaped = v_t[None] + torch.einsum('bl,mkl->bmk', betas, S)
    J = torch.einsum('bik,ji->bjk', v_shaped, Jreg)
    n_j = J.shape[1]
    Rm = R.rodrigues(full_pose.reshape(-1, 3), getattr(bm, 'rodrigues_convention', 'smplx')).view(n, n_j, 3, 3)
    feat = (Rm[:, 1:] - torch.eye(3, dtype=dt, device=dev)).reshape(n, -1)
    rel = J.clone()
    rel[:, 1:] = J[:, 1:] - J[:, bm.parents[1:]]
    G = [None] * n_j
    for j in range(n_j):
        T = torch.zeros(n, 4, 4, dtype=dt, device=dev)
        T[:, :3, :3], T[:, :3, 3], T[:, 3, 3] = Rm[:, j], rel[:, j], 1.0
        G[j] = T if j == 0 else G[bm.parents[j]] @ T
    G = torch.stack(G, dim=1)
    Rj = G[:, :, :3, :3]
    tj = G[:, :, :3, 3] - (Rj @ J[..., None])[..., 0]
    base = v_t.abs()[None] + torch.einsum('bl,mkl->bmk', betas.abs(), S.abs()) \
        + (feat.abs() @ P.abs()).view(n, -1, 3)                # (n, V, 3)
    skin_r = (Wt.abs() @ Rj.abs().reshape(n, n_j, 9)).view(n, -1, 3, 3)      # sum_j w_vj |R_j|
    skin_t = Wt.abs() @ tj.abs()                                               # sum_j w_vj |t_j|
    out = (skin_r @ base[..., None])[..., 0] + skin_t
    if trans is not None:
        out = out + trans.detach().to(dt).abs()[:, None, :]
    return out


# ----------------------------------------------------------------------------------------------------------------------
class Report(object):
    """Result of `check`: `n_bad` violations, `worst` = the largest err / allowance and its `worst_index`, and the
    `message` with the violations counted by their place in the kernels' tiles."""

    def __init__(self, n_bad, worst, worst_index, ratio_um, message):
        self.n_bad, self.worst, self.worst_index, self.ratio_um, self.message = n_bad, worst, worst_index, ratio_um, message

    @property
    def ok(self):
        return self.n_bad == 0

    def __bool__(self):
        return self.ok


def _top(counter, k=12):
    return ', '.join('%s: %d' % (key, cnt) for key, cnt in counter.most_common(k))


def check(name, got, want, allowance, gamma=None, row_mod=64, col_mod=32):
    """Hold `got` to `want` (float64) within `allowance` at every element.  2-D outputs (rows, columns) are classed by
    (row mod `row_mod`, column mod `col_mod`); 3-D mesh outputs (frames, vertices, 3) by coordinate as well.  `gamma`
    (the family constant the allowance was built with) turns the worst ratio into the gamma it would have needed.
    Non-finite values are violations."""
    got64 = got.detach().double().to(want.device)
    err = (got64 - want).abs()
    err = torch.where(torch.isfinite(got64), err, torch.full_like(err, float('inf')))
    ratio = err / allowance.clamp_min(1e-300)
    bad = ratio > 1.0
    n_bad = int(bad.sum())
    flat = int(torch.argmax(torch.where(torch.isnan(ratio), torch.full_like(ratio, float('inf')), ratio)))
    idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(flat), ratio.shape))
    worst = float(ratio.reshape(-1)[flat])
    ratio_um = None if gamma is None else worst * gamma
    msg = ['%s: %d of %d elements over the allowance; worst err / allowance %.3g at %s (err %.3g, allowance %.3g%s)'
           % (name, n_bad, err.numel(), worst, idx, float(err[idx]), float(allowance[idx]),
              '' if gamma is None else ', i.e. err / (u m) = %.3g against gamma = %g' % (ratio_um, gamma))]
    if n_bad:
        where = bad.nonzero().cpu()
        if got.dim() == 3:        # mesh: (frame, vertex, coordinate)
            by_coord = collections.Counter(int(c) for c in where[:, 2])
            by_fv = collections.Counter((int(r) % row_mod, int(v) % col_mod) for r, v in where[:, :2])
            msg.append('  by coordinate: ' + _top(by_coord))
            msg.append('  by (frame mod %d, vertex mod %d): %s' % (row_mod, col_mod, _top(by_fv)))
        else:
            rows, cols = where[:, 0] % row_mod, (where[:, 1] % col_mod if where.shape[1] > 1 else where[:, 0] * 0)
            msg.append('  by (row mod %d, column mod %d): %s' % (row_mod, col_mod,
                                                                 _top(collections.Counter(zip(rows.tolist(), cols.tolist())))))
            msg.append('  by row mod %d: %s' % (row_mod, _top(collections.Counter(rows.tolist()))))
            msg.append('  by column mod %d: %s' % (col_mod, _top(collections.Counter(cols.tolist()), 32)))
    return Report(n_bad, worst, idx, ratio_um, '\n'.join(msg))
