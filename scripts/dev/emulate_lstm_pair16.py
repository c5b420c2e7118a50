"""Dev (numpy, CPU only): the arithmetic of the LSTM gate sums of lstm_chain16_pair_kernel (csrc/lstm_chain16_x3.hip, option
lstm_pair16), emulated with the model of emulate_pair16.py -- pieces rounded to nearest, a matrix instruction the exact sum of
its 32 k products added to the fp32 accumulator with one rounding, products in the kernels' order.  What differs from the
update MLPs: the A operand h lies in [-1, 1] under the FIXED scale 2^14 (no row maximum); gate column n has one scale s_n
from the concatenated [W_ih | W_hh]; an unbounded operand (the raw input, a caller's h0) stays on three bf16 pieces with its
weights packed as the pieces of w s_n 2^14, and adds into the same accumulator ("mixed").
Prints the worst |err| / sum_k |a_k w_k| over 64 x 128 outputs in units of u = 2^-24, next to the three-piece form.
Usage: python scripts/dev/emulate_lstm_pair16.py > profiles/r12_lstm_pair16_emulation_cpu.txt"""
import numpy as np

from emulate_pair16 import M, N, U, pieces_bf16, pieces_f16, pow2_scale

X3 = list(zip((2, 1, 0, 1, 0, 0), (0, 1, 2, 0, 1, 0)))       # bf16x3.h X3_PA / X3_PB
P16 = list(zip((1, 0, 0), (0, 1, 0)))                        # f16pair.h PA / PB
S_A = np.float32(2.0 ** 14)                                  # pair16::EXP_TOP


def chain(acc, a_pieces, w_pieces, order, step=32):
    for k0 in range(0, a_pieces[0].shape[1], step):
        for pa, pb in order:
            s = a_pieces[pa][:, k0:k0 + step].astype(np.float64) @ w_pieces[pb][:, k0:k0 + step].astype(np.float64).T
            acc = (acc.astype(np.float64) + s).astype(np.float32)
    return acc


def worst(got, a, w):
    ref = a.astype(np.float64) @ w.astype(np.float64).T
    mag = np.abs(a).astype(np.float64) @ np.abs(w).astype(np.float64).T
    return float((np.abs(got.astype(np.float64) - ref) / mag).max() / U)


def gate_sums(x, h, w_ih, w_hh):
    """(three-piece form, pair form) of [x | h] [W_ih | W_hh]^T; x may be None (layer >= 1 with the input as part of h)"""
    w_all = w_hh if x is None else np.concatenate([w_ih, w_hh], axis=1)
    sw = pow2_scale(w_all, 1)                                # one exponent per gate column, over both matrices
    zero = np.zeros((M, N), np.float32)
    x3 = zero if x is None else chain(zero, pieces_bf16(x), pieces_bf16(w_ih), X3)
    x3 = chain(x3, pieces_bf16(h), pieces_bf16(w_hh), X3)
    # wide steps: A as it is, W the pieces of w s_n 2^14; pair steps: split(h 2^14), split(w s_n)
    p = zero if x is None else chain(zero, pieces_bf16(x), pieces_bf16((w_ih * sw * S_A).astype(np.float32)), X3)
    p = chain(p, pieces_f16(h, S_A), pieces_f16(w_hh, sw), P16)
    p = ((p / sw.T).astype(np.float32) / S_A).astype(np.float32)     # exact: powers of two
    return x3, p


def main():
    rng = np.random.default_rng(12)
    g = lambda *s: rng.standard_normal(s).astype(np.float32)
    K = 512
    wn = lambda k: (g(N, k) / np.sqrt(k)).astype(np.float32)
    near1 = (np.sign(g(M, K)) * (1.0 - np.abs(g(M, K)) * 2.0 ** -12)).astype(np.float32)
    near1[:, ::7] = np.float32(1.0)
    near1[:, 3::7] = np.float32(-1.0)
    hidden = [('h = tanh(gaussian)', np.tanh(g(M, K)).astype(np.float32)),
              ('h uniform in (-1, 1)', rng.uniform(-1, 1, (M, K)).astype(np.float32)),
              ('every element of a row tiny (1e-6)', (1e-6 * g(M, K)).astype(np.float32)),
              ('elements near +-1 and at +-1', near1),
              ('h spread over 16 binades below 1', (rng.uniform(-1, 1, (M, K)) * np.exp2(-rng.integers(0, 16, (M, K)))).astype(np.float32))]
    print('worst |err| / sum|a||w| over %d x %d outputs, in u = 2^-24; h under the fixed 2^14, K = %d' % (M, N, K))
    print('%-52s %22s %20s' % ('operands', 'bf16 x 3, 6 products', 'f16 x 2, 3 products'))
    for name, h in hidden:
        w = wn(K)
        x3, p = gate_sums(None, h, None, w)
        print('%-52s %22.2f %20.2f' % (name, worst(x3, h, w), worst(p, h, w)))
    print()
    print('one gate column over [W_ih | W_hh]: x gaussian (K = 296, wide steps) + h = tanh(gaussian) (K = 512, pair steps)')
    for name, f_ih, f_hh in [('W_ih, W_hh of equal magnitude', 1.0, 1.0), ('W_ih 2^10 times W_hh', 2.0 ** 10, 1.0),
                             ('W_hh 2^10 times W_ih', 1.0, 2.0 ** 10)]:
        x, h = g(M, 296), np.tanh(g(M, K)).astype(np.float32)
        w_ih, w_hh = (wn(296) * f_ih).astype(np.float32), (wn(K) * f_hh).astype(np.float32)
        x3, p = gate_sums(x, h, w_ih, w_hh)
        a, w = np.concatenate([x, h], axis=1), np.concatenate([w_ih, w_hh], axis=1)
        print('%-52s %22.2f %20.2f' % (name, worst(x3, a, w), worst(p, a, w)))
    print()
    print('the weaker matrix alone against its own sum|a||w| (the column scale belongs to the other matrix): pair steps')
    for name, f in [('W_hh 2^-10 of the column maximum', 2.0 ** -10), ('W_hh 2^-14 of the column maximum', 2.0 ** -14)]:
        h, w_hh = np.tanh(g(M, K)).astype(np.float32), (wn(K) * f).astype(np.float32)
        sw = pow2_scale(wn(K), 1)
        p = chain(np.zeros((M, N), np.float32), pieces_f16(h, S_A), pieces_f16(w_hh, sw), P16)
        p = ((p / sw.T).astype(np.float32) / S_A).astype(np.float32)
        x3 = chain(np.zeros((M, N), np.float32), pieces_bf16(h), pieces_bf16(w_hh), X3)
        print('%-52s %22.2f %20.2f' % (name, worst(x3, h, w_hh), worst(p, h, w_hh)))
    print()
    print('a row of tiny h, absolute: its pieces under 2^14 are f16 subnormals below 2^-24 x 2^14 of 1, i.e. the worst')
    h = (1e-6 * g(M, K)).astype(np.float32)
    w = wn(K)
    _, p = gate_sums(None, h, None, w)
    print('absolute error of such a row\'s gate sum is %.2e (fp32 u of a gate sum of magnitude 1: %.2e)'
          % (float(np.abs(p.astype(np.float64) - h.astype(np.float64) @ w.astype(np.float64).T).max()), U))


if __name__ == '__main__':
    main()
