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
// The same order without a compare per value, for the epilogues that look at every accumulator: the magnitude bits shifted
// left by one (the sign leaves) plus 2^24, in unsigned arithmetic -- ONE v_lshl_add_u32.  A finite magnitude lands in
// [KEY_ZERO, 2^32) in its own order; inf and NaN wrap to [0, KEY_ZERO) and lose every maximum that starts from KEY_ZERO,
// the key of 0.  key_bits undoes it, once per row: key_bits(max of keys) == max of finite_abs_bits.
constexpr unsigned KEY_ZERO = 0x01000000u;
__host__ __device__ inline unsigned finite_key(float y) { return (__builtin_bit_cast(unsigned, y) << 1) + KEY_ZERO; }
__host__ __device__ inline unsigned key_bits(unsigned key) { return (key - KEY_ZERO) >> 1; }

// A row group -- 16 adjacent lanes -- is a DPP row: a lane reads another's register in the instruction that uses it.
constexpr int DPP_XOR1 = 0xB1, DPP_XOR2 = 0x4E;                  // quad_perm:[1,0,3,2], quad_perm:[2,3,0,1]
constexpr int DPP_HALF_MIRROR = 0x141, DPP_MIRROR = 0x140;       // row_half_mirror (7 - i of 8), row_mirror (15 - i of 16)
// (Every lane of a row is written -- all four patterns are permutations, the users run with all lanes on -- so the `old`
// value is never seen; 0, a maximum's identity, is what lets the compiler fold the move into the v_max_u32 that uses it.)
template <int CTRL>
__device__ __forceinline__ unsigned dpp(unsigned v) {
  return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, false);
}
template <int CTRL>
__device__ __forceinline__ unsigned dpp_max(unsigned m) {
  const unsigned o = dpp<CTRL>(m);
  return o > m ? o : m;
}
// the maximum of an integer over the 16 lanes of a row group, in every lane: four v_max_u32_dpp
__device__ __forceinline__ unsigned max16(unsigned m) {
  return dpp_max<DPP_MIRROR>(dpp_max<DPP_HALF_MIRROR>(dpp_max<DPP_XOR2>(dpp_max<DPP_XOR1>(m))));
}
// The maxima of SIXTEEN integers over the 16 lanes of a row group as a reduce-scatter (lane_reduce.h): every step halves
// what a lane carries -- it keeps the half its lane bit selects and takes the partner's maximum of the same half -- and
// lane l15 returns the group's maximum of v[l15] (v is used up): 15 exchanges instead of 64.  The mirrors come first: a
// mirror's partner differs in the lower lane bits too, and has to hold the same half still.
__device__ __forceinline__ unsigned max16_scatter(unsigned (&v)[16], int l15) {
  const bool b3 = l15 & 8, b2 = l15 & 4, b1 = l15 & 2, b0 = l15 & 1;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const unsigned keep = b3 ? v[i + 8] : v[i], send = b3 ? v[i] : v[i + 8], got = dpp<DPP_MIRROR>(send);
    v[i] = got > keep ? got : keep;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const unsigned keep = b2 ? v[i + 4] : v[i], send = b2 ? v[i] : v[i + 4], got = dpp<DPP_HALF_MIRROR>(send);
    v[i] = got > keep ? got : keep;
  }
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const unsigned keep = b1 ? v[i + 2] : v[i], send = b1 ? v[i] : v[i + 2], got = dpp<DPP_XOR2>(send);
    v[i] = got > keep ? got : keep;
  }
  const unsigned keep = b0 ? v[1] : v[0], send = b0 ? v[0] : v[1], got = dpp<DPP_XOR1>(send);
  return got > keep ? got : keep;
}
}  // namespace pair16
}  // namespace empose
