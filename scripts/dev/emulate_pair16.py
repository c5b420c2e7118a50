"""Dev (numpy, CPU only): the arithmetic of the update MLPs' three product forms, emulated -- fp32 operands as they are, three
bf16 pieces per operand with six products (csrc/bf16x3.h), two f16 pieces per operand under power-of-two row / column
scales with three products (csrc/f16pair.h).  Pieces are rounded to nearest; a matrix instruction is modelled as the exact
sum of its 32 k products added to the fp32 accumulator with one rounding, the products of an accumulator in the kernels'
order (the small ones first).  Prints the worst |err| / sum_k |a_k w_k| over 64 x 128 outputs in units of u = 2^-24.
This covers the arithmetic, not the hardware: tests/test_mlp_pair16.py holds the kernels themselves to float64.
Usage: python scripts/dev/emulate_pair16.py > profiles/r11_pair16_emulation_cpu.txt"""
import numpy as np

U = 2.0 ** -24
M, N = 64, 128


def bf16(x):
    """round-to-nearest-even bf16 of an fp32 array, as fp32"""
    b = np.asarray(x, np.float32).view(np.uint32).astype(np.uint64)
    b = (b + 0x7fff + ((b >> 16) & 1)) & 0xffff0000
    return b.astype(np.uint32).view(np.float32)


def f16(x):
    return np.asarray(x, np.float32).astype(np.float16).astype(np.float32)


def pieces_bf16(x):
    h = bf16(x)
    m = bf16(x - h)
    return [h, m, bf16(x - h - m)]


def pow2_scale(x, axis):
    """2^e per row (axis 1) / column with the scaled largest magnitude in [2^14, 2^15); 1 for an all-zero line"""
    m = np.abs(x).max(axis=axis, keepdims=True)
    e = np.where(m > 0, 14 - np.floor(np.log2(np.where(m > 0, m, 1.0))), 0.0)
    return np.exp2(e).astype(np.float32)


def pieces_f16(x, s):
    xs = (x * s).astype(np.float32)
    h = f16(xs)
    return [h, f16(xs - h)]


def mfma_chain(a_pieces, w_pieces, order, step=32):
    """acc <- fl32(acc + exact sum over the step's k of a_piece w_piece), per step the products in `order`"""
    K = a_pieces[0].shape[1]
    acc = np.zeros((M, N), np.float32)
    for k0 in range(0, K, step):
        for pa, pb in order:
            s = a_pieces[pa][:, k0:k0 + step].astype(np.float64) @ w_pieces[pb][:, k0:k0 + step].astype(np.float64).T
            acc = (acc.astype(np.float64) + s).astype(np.float32)
    return acc


def worst(got, a, w):
    ref = a.astype(np.float64) @ w.astype(np.float64).T
    mag = np.abs(a).astype(np.float64) @ np.abs(w).astype(np.float64).T
    return float((np.abs(got.astype(np.float64) - ref) / mag).max() / U)


def prelu(x, slope=0.01):
    return np.where(x >= 0, x, slope * x).astype(np.float32)


def main():
    rng = np.random.default_rng(11)
    g = lambda *s: rng.standard_normal(s).astype(np.float32)
    spread = lambda k: (g(M, k) * np.exp2(rng.integers(-8, 8, size=(M, k)))).astype(np.float32)
    cases = [('gaussian, 512', g(M, 512)), ('gaussian, 320', g(M, 320)), ('PReLU(0.01) of gaussian, 512', prelu(g(M, 512))),
             ('PReLU(0.01) of gaussian, 1024', prelu(g(M, 1024))), ('elements spread over 16 binades, 512', spread(512))]
    X3 = list(zip((2, 1, 0, 1, 0, 0), (0, 1, 2, 0, 1, 0)))       # bf16x3.h X3_PA / X3_PB
    P16 = list(zip((1, 0, 0), (0, 1, 0)))                        # f16pair.h PA / PB: lo hi, hi lo, hi hi
    print('worst |err| / sum|a||w| over %d x %d outputs, in u = 2^-24' % (M, N))
    print('%-40s %12s %22s %20s' % ('input, K', 'fp32 chain', 'bf16 x 3, 6 products', 'f16 x 2, 3 products'))
    for name, a in cases:
        w = (g(N, a.shape[1]) / np.sqrt(a.shape[1])).astype(np.float32)
        sa, sw = pow2_scale(a, 1), pow2_scale(w, 1)
        p16 = mfma_chain(pieces_f16(a, sa), pieces_f16(w, sw), P16)
        p16 = ((p16 / sw.T).astype(np.float32) / sa).astype(np.float32)          # exact: powers of two
        print('%-40s %12.2f %22.2f %20.2f' % (name, worst(mfma_chain([a], [w], [(0, 0)]), a, w),
                                              worst(mfma_chain(pieces_bf16(a), pieces_bf16(w), X3), a, w), worst(p16, a, w)))


if __name__ == '__main__':
    main()
