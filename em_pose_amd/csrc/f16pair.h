// fp32 values as TWO f16 pieces under a power-of-two scale, the operand format of mlp_fused_x3_kernel<PAIR16> and of
// lstm_chain16_pair_kernel:
//   hi = rn_f16(x s),  lo = rn_f16(x s - float(hi))          11 + 11 mantissa bits, 2^-24 relative: fp32's own roundoff
//   x w ~= (lo_x hi_w + hi_x lo_w + hi_x hi_w) / (s_x s_w)   three v_mfma_f32_16x16x32_f16 products, the small ones first;
// what is dropped (lo_x lo_w) is at 2^-24 of the product.  The three-piece bf16 format (bf16x3.h) needs six products for
// the same: with 8-bit pieces three of the nine cross products sit at 2^-16.
// f16 has a narrow exponent, hence the scale s = 2^e: ONE exponent per row of the A operand and one per output column of
// W, constant along K, so that it leaves the sum and is undone -- exactly -- on the accumulator.  e is chosen from the
// row's (column's) largest FINITE magnitude m so that m s lies in [2^14, 2^15): hi then never overflows, and an element
// 2^-24 of the largest still has a (subnormal) hi piece.  An all-zero row has e = 0; floor(log2 m) is clamped to
// +-EXP_CLAMP, which keeps s and 1 / s normal fp32 numbers.  A row that holds inf or NaN keeps its finite scale: its
// pieces, and with them its results, are non-finite, and no other row sees it.
// A second user with a FIXED scale: lstm_chain16_pair_kernel (lstm_chain16_x3.hip).  Its A operand is the hidden state
// h = o tanh(c) in [-1, 1]: s = 2^EXP_TOP for every row, no maximum to find (h s <= 2^14 cannot overflow; an element below
// 2^-24 of 1 has lost its lo piece, which is 2^-24 of what a gate sum is compared with).  Its weight columns are scaled as
// above, over the concatenated [W_ih | W_hh]; an operand that is not bounded (the raw input, a caller's h0) stays on three
// bf16 pieces against weights packed as the pieces of w s 2^EXP_TOP and adds into the same accumulator.
// Conversions are round to nearest (v_cvt_pk_f16_f32), never the round-toward-zero pack: truncated pieces are four times
// less accurate.  Internal, gfx950 only.
#pragma once
#include "bf16x3.h"

namespace empose {

typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2_t __attribute__((ext_vector_type(2)));

namespace pair16 {

constexpr int EXP_TOP = 14, EXP_CLAMP = 100;

// The three piece products of an accumulator in the order they are issued (piece 0 = hi, 1 = lo).
constexpr int PA[3] = {1, 0, 0}, PB[3] = {0, 1, 0};

// |y| as an integer that orders like the magnitude; 0 for inf and NaN (they do not take part in a maximum)
__host__ __device__ inline unsigned finite_abs_bits(float y) {
  const unsigned b = __builtin_bit_cast(unsigned, y) & 0x7fffffffu;
  return b < 0x7f800000u ? b : 0u;
}
// the exponent e of the scale for a largest finite magnitude with these bits
__host__ __device__ inline int scale_exp(unsigned max_bits) {
  if (max_bits == 0u) return 0;
  int fl = (int)(max_bits >> 23) - 127;
  fl = fl < -EXP_CLAMP ? -EXP_CLAMP : fl > EXP_CLAMP ? EXP_CLAMP : fl;
  return EXP_TOP - fl;
}
__host__ __device__ inline float pow2(int e) { return __builtin_bit_cast(float, (unsigned)(e + 127) << 23); }

// two scaled fp32 -> their (hi, lo) pieces, packed (element 0 in the low half)
__device__ __forceinline__ void split_pair(float x0, float x1, unsigned& hi, unsigned& lo) {
  const f16x2_t h = __builtin_convertvector(f32x2_t{x0, x1}, f16x2_t);
  const f32x2_t hf = __builtin_convertvector(h, f32x2_t);
  const f16x2_t l = __builtin_convertvector(f32x2_t{x0 - hf[0], x1 - hf[1]}, f16x2_t);
  hi = __builtin_bit_cast(unsigned, h);
  lo = __builtin_bit_cast(unsigned, l);
}
// the maximum of an integer over the 16 lanes of a row group
__device__ __forceinline__ unsigned max16(unsigned m) {
#pragma unroll
  for (int d = 1; d < 16; d <<= 1) {
    const unsigned o = (unsigned)__shfl_xor((int)m, d);
    m = o > m ? o : m;
  }
  return m;
}
}  // namespace pair16
}  // namespace empose
