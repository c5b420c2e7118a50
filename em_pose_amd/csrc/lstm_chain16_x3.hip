// lstm_chain_x3_kernel (lstm_x3.hip) with its products on v_mfma_f32_16x16x32_bf16 (option lstm_x3 = 3).
//
// Same workgroup (64 batch rows x 32 hidden units x 4 gates, walks layer 0 then layer 1), same K split over four waves that
// each keep the whole 64 x 128 tile in 128 registers, same operands from global memory in fragment order, no LDS and no
// barrier in the K loop, same finish.  The instruction is the only variable: where the chip holds its clock down under
// matrix load, the 16x16x32 shape has been seen to hold a higher one at equal cycles per FLOP.
//   * the tile is 4 x 8 accumulator tiles of 16 x 16; a k-step is 32 wide: K2_in = (ks_in + 1) / 2 steps of the input, then
//     ks_rec / 2 recurrent ones; wave w takes steps w, w + 4, ... of the unit;
//   * weights in the LSTM_MID16 order of lstm_mid16_x3.hip ([k-step of 32][4-unit block][piece], column = gate * 4 + unit):
//     the workgroup's 32 units are the blocks 8 jb .. 8 jb + 7;
//   * A fragments from the planes every other kernel writes ([32-row tile][k-step of 16][piece][lane (row, k half)][8]):
//     lane (r = lane & 15, q = lane >> 4) of 16-row tile rt16 reads row (rt16 & 1) * 16 + r, half q & 1 of 16-k step
//     2 k2 + (q >> 1) of 32-row tile rt16 >> 1.  An odd ks_in ends on a half step: the lanes of the half that does not exist
//     hold zero (selected, not multiplied away by the weights' zero padding: no 0 * Inf);
//   * per wave and step 12 A + 24 W fragment loads and 192 MFMAs; two fragment sets (2 x 144 registers), the next step's
//     loads pinned between this step's MFMAs -- the same look-ahead in k as lstm_chain_x3_kernel's step after next;
//   * partial sums meet in LDS as [wave][gate][unit][row] and are added in wave order; thread (row, 8 units) runs the cell.
// The sums are grouped differently from lstm_chain_x3_kernel (32 k per instruction): the two agree to rounding, not to the bit.
// One workgroup per CU, one wave per SIMD, stores only in the finish (bf16x3.h).
// Below it lstm_chain16_pair_kernel (option lstm_pair16, the default): the same step with the operands the kernel produced
// itself on two f16 pieces, three products instead of six.
#include <type_traits>

#include "f16pair.h"
#include "gemm_epilogue.h"
#include "launch.h"
#include "lstm_kernels.h"

namespace empose {

namespace lx16 {
constexpr int BM = 64, BU = 32, NT = 256, RT = 4, CB = 8;            // row tiles of 16, column blocks of 4 units x 4 gates
// a partial-sum column is PLD floats, gate q's columns are shifted by 4 q floats: the 16 lanes of a C tile that store
// together (column = lane & 15 = gate * 4 + unit) then spread over all banks two deep, which is what 256 bytes take anyway
constexpr int PLD = BM + 8, GSK = 4;
constexpr int WAVE_FLOATS = 4 * BU * PLD + 4 * GSK;
constexpr size_t LDS_BYTES = (size_t)4 * WAVE_FLOATS * sizeof(float);   // 147,712 bytes: one workgroup per CU
static_assert(LDS_BYTES > LDS_BYTES_PER_CU / 2 && LDS_BYTES <= LDS_BYTES_PER_CU, "one workgroup per CU");
__device__ __forceinline__ int col_off(int gate, int unit) { return (gate * BU + unit) * PLD + gate * GSK; }

// The finish of lstm_chain16_pair_kernel: lstm_chain16_x3_kernel's -- thread (row tid & 63, units j0 + 8 (tid >> 6) .. + 7)
// adds the four waves' partial sums in wave order, runs the cell and stores the state, the outputs and the new hidden values
// as the next step's A planes -- except that the sums carry 2^14 s_n, undone (exactly) by e_inv before the bias, and that
// the planes are the two f16 pieces of h 2^14, at the three-piece stride.  (Its own copy: with one template shared by both, the three-piece
// kernel's finish compiled to other instructions and its outputs were no longer the parent's bits -- most likely another
// contraction of the cell update into fused multiply-adds; profiles/r12_lstm_chain16_isa_vs_parent.txt.)
__device__ __forceinline__ void finish_pair(const LstmX3Args& a, const LstmX3Unit& U, const float* part, int tid, int m0, int j0,
                                       const f32x4 (&e_c)[2], const f32x4 (&e_hp)[2], const float (&e_bias)[4][8],
                                       const float (&e_inv)[4][8], int e_len) {
  const int H = a.H, B = a.B, F = a.F, t = U.t, KS_h = H / 16;
  const bool skip_h = a.skip_h_state != 0;
  const int f_row = tid & 63, f_ug = tid >> 6;
  const int g_row = m0 + f_row, g_unit = j0 + f_ug * 8;
  float hv[8], cv[8], yv[8];
  const bool live = t < e_len;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    float gsum[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float* ps = part + col_off(q, f_ug * 8 + e) + f_row;
      gsum[q] = ((ps[0] + ps[WAVE_FLOATS]) + ps[2 * WAVE_FLOATS]) + ps[3 * WAVE_FLOATS];
      gsum[q] *= e_inv[q][e];
    }
    const float g_i = fast_sigmoid(gsum[0] + e_bias[0][e]), g_f = fast_sigmoid(gsum[1] + e_bias[1][e]);
    const float g_g = fast_tanh(gsum[2] + e_bias[2][e]), g_o = fast_sigmoid(gsum[3] + e_bias[3][e]);
    const float c_old = e_c[e >> 2][e & 3], h_old = e_hp[e >> 2][e & 3];
    const float c_new = g_f * c_old + g_i * g_g;
    const float h_new = g_o * fast_tanh(c_new);
    cv[e] = live ? c_new : c_old;
    hv[e] = live ? h_new : (a.seq_lengths ? h_old : 0.f);
    yv[e] = live ? h_new : 0.f;
  }
  if (g_row < B) {
    const size_t hc = (size_t)g_row * H + g_unit;
    *reinterpret_cast<f32x4*>(U.c + hc) = f32x4{cv[0], cv[1], cv[2], cv[3]};
    *reinterpret_cast<f32x4*>(U.c + hc + 4) = f32x4{cv[4], cv[5], cv[6], cv[7]};
    // (skip_h: every row is live at every step and the last step stores h_final -- nobody reads h_next)
    if (!skip_h) {
      *reinterpret_cast<f32x4*>(U.h_next + hc) = f32x4{hv[0], hv[1], hv[2], hv[3]};
      *reinterpret_cast<f32x4*>(U.h_next + hc + 4) = f32x4{hv[4], hv[5], hv[6], hv[7]};
    }
    // the layer's last step: the same values once more, where the caller wants h_n / c_n
    if (U.h_final) {
      *reinterpret_cast<f32x4*>(U.h_final + hc) = f32x4{hv[0], hv[1], hv[2], hv[3]};
      *reinterpret_cast<f32x4*>(U.h_final + hc + 4) = f32x4{hv[4], hv[5], hv[6], hv[7]};
    }
    if (U.c_final) {
      *reinterpret_cast<f32x4*>(U.c_final + hc) = f32x4{cv[0], cv[1], cv[2], cv[3]};
      *reinterpret_cast<f32x4*>(U.c_final + hc + 4) = f32x4{cv[4], cv[5], cv[6], cv[7]};
    }
    if (U.y) {
      float* yo = U.y + ((size_t)g_row * F + t) * U.y_ld + U.y_col + g_unit;
      *reinterpret_cast<f32x4*>(yo) = f32x4{yv[0], yv[1], yv[2], yv[3]};
      *reinterpret_cast<f32x4*>(yo + 4) = f32x4{yv[4], yv[5], yv[6], yv[7]};
    }
    // the new hidden values as pieces, where the next step's (and the layer above's) A fragments expect them
    const int ks = g_unit >> 4, ln = (g_row & 31) + 32 * ((g_unit & 15) >> 3);
    unsigned short* o = U.a3_out + ((((size_t)(g_row >> 5)) * KS_h + ks) * 3) * FRAG + ln * 8;
    // (a row past its length carries the caller's h0 on: beyond 4 its pieces overflow -- in that row, which stays dead)
    const float s = pair16::pow2(pair16::EXP_TOP);
    unsigned hi[4], lo[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) pair16::split_pair(hv[2 * e] * s, hv[2 * e + 1] * s, hi[e], lo[e]);
    *reinterpret_cast<u32x4_t*>(o) = u32x4_t{hi[0], hi[1], hi[2], hi[3]};
    *reinterpret_cast<u32x4_t*>(o + FRAG) = u32x4_t{lo[0], lo[1], lo[2], lo[3]};
  }
}

// Which k-steps of 32 a wave of lstm_chain16_pair_kernel takes of a unit's NW wide (192 MFMAs) and NP pair (96) steps.
// Wide steps go round: wave w takes w, w + 4, ...; r = NW % 4 waves then hold one more than the others.  The first
// E = min(NP, 2 (4 - r)) pair steps level that -- two to each wave that is one wide step short, in turn -- and the rest go
// round again.  With r = 0 pair step j is wave j % 4's whatever NP is: the recurrent steps that lstm_skip_dead leaves out
// come last and move no other step to another wave.
struct WaveSteps {
  int r, E, n_wide, n_lev, n_pair;   // this wave's wide steps, levelling pair steps, all pair steps
  int wave;
  __host__ __device__ WaveSteps(int NW, int NP, int w) : r(NW & 3), wave(w) {
    E = r ? (NP < 2 * (4 - r) ? NP : 2 * (4 - r)) : 0;
    n_wide = (NW - w + 3) / 4;
    n_lev = (r && w >= r && E > w - r) ? (E - (w - r) + (4 - r) - 1) / (4 - r) : 0;
    n_pair = n_lev + (NP - E - w + 3) / 4;
  }
  __host__ __device__ int wide_step(int i) const { return wave + 4 * i; }
  __host__ __device__ int pair_step(int i) const { return i < n_lev ? (wave - r) + (4 - r) * i : E + wave + 4 * (i - n_lev); }
};
}  // namespace lx16

__global__ __launch_bounds__(lx16::NT) void lstm_chain16_x3_kernel(LstmX3Args a) {
  X3_EXCLUSIVE_SIMD();
  using namespace lx16;
  extern __shared__ __attribute__((aligned(16))) float part[];
  const int H = a.H, B = a.B, F = a.F;
  const int jb = blockIdx.x, JB4 = H / 4, j0 = jb * BU;
  const int m0 = blockIdx.y * BM, rt0 = blockIdx.y * 2;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, lq = lane >> 4;
  const int KS_h = H / 16;                                         // k-steps of 16 of a hidden-state plane
  const bool skip_h = a.skip_h_state != 0;
  // the finishing thread's element group: row f_row, units j0 + 8 f_ug .. + 7 (all four gates)
  const int f_row = tid & 63, f_ug = tid >> 6;
  const int g_row = m0 + f_row, g_rowc = g_row < B ? g_row : B - 1;
  const int g_unit = j0 + f_ug * 8;
  // lane (row l15, k quarter lq) of a 16 x 32 A fragment: half lq & 1 of k-step 2 k2 + (lq >> 1) of the 32-row tile's plane
  const int lane_off = (l15 + 32 * (lq & 1)) * 8;
  // (an odd number of 32-row tiles: the last workgroup's second tile does not exist in the piece planes -- it reads its
  // first tile again instead of one tile past the plane; those rows are >= B and never stored)
  const bool two_tiles = rt0 + 1 < (B + 31) / 32;

  const int u_beg = blockIdx.z * a.units_per_block;
  const int u_end = u_beg + a.units_per_block < a.n_units ? u_beg + a.units_per_block : a.n_units;
  for (int u = u_beg; u < u_end; ++u) {
    const LstmX3Unit& U = a.unit[u];
    const int KS_in = U.ks_in;
    const int K2_in = (KS_in + 1) / 2, K2 = K2_in + U.ks_rec / 2;   // k-steps of 32 (the input's last may be half)
    const int t = U.t;
    // ---- the state the finish reads besides the sums, fetched now (latency under the K loop)
    f32x4 e_c[2], e_hp[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    const int e_len = a.seq_lengths ? a.seq_lengths[g_rowc] : F;
    {
      const size_t hc = (size_t)g_rowc * H + g_unit;
      e_c[0] = *reinterpret_cast<const f32x4*>(U.c + hc);
      e_c[1] = *reinterpret_cast<const f32x4*>(U.c + hc + 4);
      if (!skip_h) {
        e_hp[0] = *reinterpret_cast<const f32x4*>(U.h_prev + hc);
        e_hp[1] = *reinterpret_cast<const f32x4*>(U.h_prev + hc + 4);
      }
    }

    f32x4 acc[RT][CB];
#pragma unroll
    for (int r = 0; r < RT; ++r)
#pragma unroll
      for (int cb = 0; cb < CB; ++cb) acc[r][cb] = f32x4{0.f, 0.f, 0.f, 0.f};

    // ---- the wave's k-steps of 32: g = wave + 4 i.  Fragments of step g: A from the input planes (g < K2_in) or the
    // recurrent ones, W from the matching matrix; everything is a wave-uniform base plus a lane offset.
    u32x4_t fa[2][RT][3], fw[2][CB][3];
    const int n_w = (K2 - wave + 3) / 4;
    const unsigned short* const p_in = U.a3_in; const unsigned short* const p_rec = U.a3_rec;
    const unsigned short* const p_wih = U.w3_ih; const unsigned short* const p_whh = U.w3_hh;
    // the half step of an odd input: k-step of 16 number KS_in does not exist
    const int g_half = (KS_in & 1) ? K2_in - 1 : -1;
    auto load = [&, p_in, p_rec, p_wih, p_whh](u32x4_t (&A)[RT][3], u32x4_t (&W)[CB][3], int i) {
      int g = wave + 4 * i;
      g = g < K2 ? g : K2 - 1;                      // (past the wave's last step: fetched, never multiplied)
      const bool in = g < K2_in;
      const int k2 = in ? g : g - K2_in, ksn = in ? KS_in : KS_h;
      // (the lanes of a half that does not exist address the first half -- inside the plane -- and are zeroed before use)
      const int ks = 2 * k2 + ((2 * k2 + 1 < ksn) ? (lq >> 1) : 0);
      x3_gptr_t ab = (x3_gptr_t)(in ? p_in : p_rec) + (((size_t)rt0 * ksn + ks) * 3) * FRAG + lane_off;
      x3_gptr_t wb = (x3_gptr_t)(in ? p_wih : p_whh) + ((((size_t)k2 * JB4 + jb * CB)) * 3) * FRAG + lane * 8;
      const size_t rt_stride = two_tiles ? (size_t)ksn * 3 * FRAG : 0;
#pragma unroll
      for (int r = 0; r < RT; ++r)
#pragma unroll
        for (int pc = 0; pc < 3; ++pc) A[r][pc] = *(x3_gvec_t)(ab + (r >> 1) * rt_stride + (r & 1) * 16 * 8 + pc * FRAG);
#pragma unroll
      for (int cb = 0; cb < CB; ++cb)
#pragma unroll
        for (int pc = 0; pc < 3; ++pc) W[cb][pc] = *(x3_gvec_t)(wb + (cb * 3 + pc) * FRAG);
    };
    // the half step: zero for the lanes of the half that does not exist.  Called BEFORE the loads that go between the step's
    // MFMAs, so that those and the MFMAs stay in one basic block (wave-uniform branch, one step of one wave per unit at most)
    auto fix_half = [&](u32x4_t (&A)[RT][3], int i) {
      if (wave + 4 * i == g_half) {
        const bool exists = (lq >> 1) == 0;
#pragma unroll
        for (int r = 0; r < RT; ++r)
#pragma unroll
          for (int pc = 0; pc < 3; ++pc) A[r][pc] = exists ? A[r][pc] : u32x4_t{0u, 0u, 0u, 0u};
      }
    };
    auto mma = [&](const u32x4_t (&A)[RT][3], const u32x4_t (&W)[CB][3]) {
#pragma unroll
      for (int p = 0; p < 6; ++p)
#pragma unroll
        for (int r = 0; r < RT; ++r)
#pragma unroll
          for (int cb = 0; cb < CB; ++cb)
            acc[r][cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, A[r][X3_PA[p]]),
                                                                 __builtin_bit_cast(bf16x8_t, W[cb][X3_PB[p]]), acc[r][cb], 0, 0, 0);
    };
    auto pattern = [&]() {   // 192 MFMAs with the 36 fragment loads of the next step between them
#pragma unroll
      for (int q = 0; q < 36; ++q) { SGB(SG_MFMA, 4); SGB(SG_VMEM_RD, 1); }
      SGB(SG_MFMA, 48);
    };
    load(fa[0], fw[0], 0);
    int i = 0;
    for (; i + 2 <= n_w; i += 2) {
      fix_half(fa[0], i);
      load(fa[1], fw[1], i + 1);
      mma(fa[0], fw[0]);
      pattern();
      fix_half(fa[1], i + 1);
      load(fa[0], fw[0], i + 2);
      mma(fa[1], fw[1]);
      pattern();
    }
    if (i < n_w) { fix_half(fa[0], i); mma(fa[0], fw[0]); }
    // (the 32 bias values do not fit beside two fragment sets and the accumulators: fetched here, where the fragment
    // registers are free, their latency under the LDS stores and the barrier)
    float e_bias[4][8];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const f32x4 b0 = *reinterpret_cast<const f32x4*>(U.bias + q * H + g_unit);
      const f32x4 b1 = *reinterpret_cast<const f32x4*>(U.bias + q * H + g_unit + 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) { e_bias[q][e] = b0[e]; e_bias[q][4 + e] = b1[e]; }
    }

    // ---- partial sums -> LDS as [wave][gate][unit][row]: the 16 x 16 C/D layout has rows 4 lq .. + 3 of column l15 in one
    // lane -- one 16-byte store; column gate * 4 + unit of block cb is unit cb * 4 + unit of the workgroup's 32
    if (u > u_beg) __syncthreads();   // the previous unit's finish has read its sums
    {
      float* pw = part + (size_t)wave * WAVE_FLOATS + col_off(l15 >> 2, l15 & 3) + 4 * lq;
#pragma unroll
      for (int cb = 0; cb < CB; ++cb)
#pragma unroll
        for (int r = 0; r < RT; ++r) *reinterpret_cast<f32x4*>(pw + cb * 4 * PLD + r * 16) = acc[r][cb];
    }
    __syncthreads();

    // ---- finish: thread (row, 8 units)
    float hv[8], cv[8], yv[8];
    const bool live = t < e_len;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float gsum[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float* ps = part + col_off(q, f_ug * 8 + e) + f_row;
        gsum[q] = ((ps[0] + ps[WAVE_FLOATS]) + ps[2 * WAVE_FLOATS]) + ps[3 * WAVE_FLOATS];
      }
      const float g_i = fast_sigmoid(gsum[0] + e_bias[0][e]), g_f = fast_sigmoid(gsum[1] + e_bias[1][e]);
      const float g_g = fast_tanh(gsum[2] + e_bias[2][e]), g_o = fast_sigmoid(gsum[3] + e_bias[3][e]);
      const float c_old = e_c[e >> 2][e & 3], h_old = e_hp[e >> 2][e & 3];
      const float c_new = g_f * c_old + g_i * g_g;
      const float h_new = g_o * fast_tanh(c_new);
      cv[e] = live ? c_new : c_old;
      hv[e] = live ? h_new : (a.seq_lengths ? h_old : 0.f);
      yv[e] = live ? h_new : 0.f;
    }
    if (g_row < B) {
      const size_t hc = (size_t)g_row * H + g_unit;
      *reinterpret_cast<f32x4*>(U.c + hc) = f32x4{cv[0], cv[1], cv[2], cv[3]};
      *reinterpret_cast<f32x4*>(U.c + hc + 4) = f32x4{cv[4], cv[5], cv[6], cv[7]};
      // (skip_h: every row is live at every step and the last step stores h_final -- nobody reads h_next)
      if (!skip_h) {
        *reinterpret_cast<f32x4*>(U.h_next + hc) = f32x4{hv[0], hv[1], hv[2], hv[3]};
        *reinterpret_cast<f32x4*>(U.h_next + hc + 4) = f32x4{hv[4], hv[5], hv[6], hv[7]};
      }
      // the layer's last step: the same values once more, where the caller wants h_n / c_n
      if (U.h_final) {
        *reinterpret_cast<f32x4*>(U.h_final + hc) = f32x4{hv[0], hv[1], hv[2], hv[3]};
        *reinterpret_cast<f32x4*>(U.h_final + hc + 4) = f32x4{hv[4], hv[5], hv[6], hv[7]};
      }
      if (U.c_final) {
        *reinterpret_cast<f32x4*>(U.c_final + hc) = f32x4{cv[0], cv[1], cv[2], cv[3]};
        *reinterpret_cast<f32x4*>(U.c_final + hc + 4) = f32x4{cv[4], cv[5], cv[6], cv[7]};
      }
      if (U.y) {
        float* yo = U.y + ((size_t)g_row * F + t) * U.y_ld + U.y_col + g_unit;
        *reinterpret_cast<f32x4*>(yo) = f32x4{yv[0], yv[1], yv[2], yv[3]};
        *reinterpret_cast<f32x4*>(yo + 4) = f32x4{yv[4], yv[5], yv[6], yv[7]};
      }
      // the new hidden values as pieces, where the next step's (and the layer above's) A fragments expect them
      const Pieces q = split8(hv[0], hv[1], hv[2], hv[3], hv[4], hv[5], hv[6], hv[7]);
      const int ks = g_unit >> 4, ln = (g_row & 31) + 32 * ((g_unit & 15) >> 3);
      unsigned short* o = U.a3_out + ((((size_t)(g_row >> 5)) * KS_h + ks) * 3) * FRAG + ln * 8;
#pragma unroll
      for (int pc = 0; pc < 3; ++pc) *reinterpret_cast<u32x4_t*>(o + pc * FRAG) = q.p[pc];
    }
  }
}

// The same step with every operand the kernel produced itself on TWO f16 pieces (f16pair.h; option lstm_pair16).
//
// h = o tanh(c) lies in [-1, 1]: under the FIXED scale 2^14 it never overflows f16, so the finish needs no row maximum (it
// could not form one: a row's units are spread over H / 32 workgroups).  Each gate column n has one power-of-two scale s_n,
// chosen at packing from the column's largest magnitude over [W_ih | W_hh] -- one matrix as far as the sum goes.  A unit's
// k-steps of 32 are of two kinds, each part (input / recurrent) wholly of one (LstmX3Unit::in_pair, rec_pair):
//   * pair step: 8 A + 16 W fragments, 96 v_mfma_f32_16x16x32_f16 in the pair16::PA / PB order; A pieces split(h 2^14), W
//     pieces split(w s_n).  h_{t-1} of the layer and the layer below's h_t;
//   * wide step: lstm_chain16_x3_kernel's 12 + 24 fragments and 192 bf16 MFMAs; A the three bf16 pieces of the operand as it
//     is, W those of w s_n 2^14 (exact before the split; bf16 has fp32's exponents).  Layer 0's raw input, and the recurrent
//     operand of a layer's first step where the caller gave h0 -- neither is bounded.
// Both accumulate sum 2^14 s_n (a w) into the same registers; the finish multiplies by 2^-14 / s_n.
// Pair planes and pair weights keep the three-piece stride (third slot unused): the addresses of the two kinds are the same,
// and the step that is fetched across the seam of the two loops is an ordinary load of the first loop.
// A wave runs its wide steps in one loop and its pair steps in the next (lx16::WaveSteps says which; the unit's sums do not
// depend on the order), both of lstm_chain16_x3_kernel's shape: two fragment sets, the next step's loads pinned between
// this step's MFMAs in one basic block, the first pair step fetched under the last wide one.  An odd wide step left over
// shares its round of the two sets with the first pair step, so that the pair loop always starts from set 0.  Grid, tile,
// LDS meeting and finish as above.
__global__ __launch_bounds__(lx16::NT) void lstm_chain16_pair_kernel(LstmX3Args a) {
  X3_EXCLUSIVE_SIMD();
  using namespace lx16;
  extern __shared__ __attribute__((aligned(16))) float part[];
  const int H = a.H, B = a.B, F = a.F;
  const int jb = blockIdx.x, JB4 = H / 4, j0 = jb * BU;
  const int m0 = blockIdx.y * BM, rt0 = blockIdx.y * 2;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, lq = lane >> 4;
  const int KS_h = H / 16;
  const bool skip_h = a.skip_h_state != 0;
  const int g_row = m0 + (tid & 63), g_rowc = g_row < B ? g_row : B - 1;
  const int g_unit = j0 + (tid >> 6) * 8;
  const int lane_off = (l15 + 32 * (lq & 1)) * 8;
  const bool two_tiles = rt0 + 1 < (B + 31) / 32;

  const int u_beg = blockIdx.z * a.units_per_block;
  const int u_end = u_beg + a.units_per_block < a.n_units ? u_beg + a.units_per_block : a.n_units;
  for (int u = u_beg; u < u_end; ++u) {
    const LstmX3Unit& U = a.unit[u];
    const int KS_in = U.ks_in;
    const int K2_in = (KS_in + 1) / 2, K2_rec = U.ks_rec / 2;
    // the unit's wide steps: the input's (if wide), then the recurrent ones (if wide); its pair steps likewise
    const int nw_in = U.in_pair ? 0 : K2_in, NW = nw_in + (U.rec_pair ? 0 : K2_rec);
    const int np_in = U.in_pair ? K2_in : 0, NP = np_in + (U.rec_pair ? K2_rec : 0);
    const WaveSteps ws(NW, NP, wave);
    const int n_ww = ws.n_wide, n_w = n_ww + ws.n_pair;
    f32x4 e_c[2], e_hp[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    const int e_len = a.seq_lengths ? a.seq_lengths[g_rowc] : F;
    {
      const size_t hc = (size_t)g_rowc * H + g_unit;
      e_c[0] = *reinterpret_cast<const f32x4*>(U.c + hc);
      e_c[1] = *reinterpret_cast<const f32x4*>(U.c + hc + 4);
      if (!skip_h) {
        e_hp[0] = *reinterpret_cast<const f32x4*>(U.h_prev + hc);
        e_hp[1] = *reinterpret_cast<const f32x4*>(U.h_prev + hc + 4);
      }
    }

    f32x4 acc[RT][CB];
#pragma unroll
    for (int r = 0; r < RT; ++r)
#pragma unroll
      for (int cb = 0; cb < CB; ++cb) acc[r][cb] = f32x4{0.f, 0.f, 0.f, 0.f};

    // ---- step i of the wave: wide for i < n_ww, then pair.  NPC pieces are fetched (3 also fetches a pair step: its third
    // slot exists and is not used).  Past the wave's last step: its last again (a wave without steps: the unit's first).
    u32x4_t fa[2][RT][3], fw[2][CB][3];
    const unsigned short* const p_in = U.a3_in; const unsigned short* const p_rec = U.a3_rec;
    const unsigned short* const p_wih = U.w3_ih; const unsigned short* const p_whh = U.w3_hh;
    // the half step of an odd (wide) input: k-step of 16 number KS_in does not exist.  Pair parts are H / 16 steps: even
    const int j_half = (KS_in & 1) && !U.in_pair ? K2_in - 1 : -1;
    auto load = [&, p_in, p_rec, p_wih, p_whh](auto npc, u32x4_t (&A)[RT][3], u32x4_t (&W)[CB][3], int i) {
      constexpr int NPC = decltype(npc)::value;
      i = i < n_w ? i : n_w - 1;
      const bool wide = n_w > 0 ? i < n_ww : NW > 0;
      const int j = n_w > 0 ? (wide ? ws.wide_step(i) : ws.pair_step(i - n_ww)) : 0;
      const int n_in = wide ? nw_in : np_in;
      const bool in = j < n_in;
      const int k2 = in ? j : j - n_in, ksn = in ? KS_in : KS_h;
      const int ks = 2 * k2 + ((2 * k2 + 1 < ksn) ? (lq >> 1) : 0);
      x3_gptr_t ab = (x3_gptr_t)(in ? p_in : p_rec) + (((size_t)rt0 * ksn + ks) * 3) * FRAG + lane_off;
      x3_gptr_t wb = (x3_gptr_t)(in ? p_wih : p_whh) + ((((size_t)k2 * JB4 + jb * CB)) * 3) * FRAG + lane * 8;
      const size_t rt_stride = two_tiles ? (size_t)ksn * 3 * FRAG : 0;
#pragma unroll
      for (int r = 0; r < RT; ++r)
#pragma unroll
        for (int pc = 0; pc < NPC; ++pc) A[r][pc] = *(x3_gvec_t)(ab + (r >> 1) * rt_stride + (r & 1) * 16 * 8 + pc * FRAG);
#pragma unroll
      for (int cb = 0; cb < CB; ++cb)
#pragma unroll
        for (int pc = 0; pc < NPC; ++pc) W[cb][pc] = *(x3_gvec_t)(wb + (cb * 3 + pc) * FRAG);
    };
    const std::integral_constant<int, 3> P3; const std::integral_constant<int, 2> P2;
    auto fix_half = [&](u32x4_t (&A)[RT][3], int i) {   // (wide steps only)
      if (ws.wide_step(i) == j_half) {
        const bool exists = (lq >> 1) == 0;
#pragma unroll
        for (int r = 0; r < RT; ++r)
#pragma unroll
          for (int pc = 0; pc < 3; ++pc) A[r][pc] = exists ? A[r][pc] : u32x4_t{0u, 0u, 0u, 0u};
      }
    };
    auto mma_wide = [&](const u32x4_t (&A)[RT][3], const u32x4_t (&W)[CB][3]) {
#pragma unroll
      for (int p = 0; p < 6; ++p)
#pragma unroll
        for (int r = 0; r < RT; ++r)
#pragma unroll
          for (int cb = 0; cb < CB; ++cb)
            acc[r][cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, A[r][X3_PA[p]]),
                                                                 __builtin_bit_cast(bf16x8_t, W[cb][X3_PB[p]]), acc[r][cb], 0, 0, 0);
    };
    auto mma_pair = [&](const u32x4_t (&A)[RT][3], const u32x4_t (&W)[CB][3]) {
#pragma unroll
      for (int p = 0; p < 3; ++p)
#pragma unroll
        for (int r = 0; r < RT; ++r)
#pragma unroll
          for (int cb = 0; cb < CB; ++cb)
            acc[r][cb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, A[r][pair16::PA[p]]),
                                                                __builtin_bit_cast(f16x8_t, W[cb][pair16::PB[p]]), acc[r][cb], 0, 0, 0);
    };
    // `n_mfma` MFMAs with the `n_load` fragment loads of the next step between them, `per` MFMAs to a load
    auto pattern = [&](auto n_mfma, auto n_load, auto per) {
#pragma unroll
      for (int q = 0; q < decltype(n_load)::value; ++q) { SGB(SG_MFMA, decltype(per)::value); SGB(SG_VMEM_RD, 1); }
      SGB(SG_MFMA, decltype(n_mfma)::value - decltype(n_load)::value * decltype(per)::value);
    };
    typedef std::integral_constant<int, 192> C192; typedef std::integral_constant<int, 96> C96;
    typedef std::integral_constant<int, 36> C36; typedef std::integral_constant<int, 24> C24;
    typedef std::integral_constant<int, 4> C4; typedef std::integral_constant<int, 3> C3;
    load(P3, fa[0], fw[0], 0);
    int i = 0;
    for (; i + 2 <= n_ww; i += 2) {
      fix_half(fa[0], i);
      load(P3, fa[1], fw[1], i + 1);
      mma_wide(fa[0], fw[0]);
      pattern(C192(), C36(), C4());
      fix_half(fa[1], i + 1);
      load(P3, fa[0], fw[0], i + 2);
      mma_wide(fa[1], fw[1]);
      pattern(C192(), C36(), C4());
    }
    if (i < n_ww) {   // an odd wide step left: it and the first pair step make one round of the two sets
      fix_half(fa[0], i);
      load(P2, fa[1], fw[1], i + 1);
      mma_wide(fa[0], fw[0]);
      pattern(C192(), C24(), C4());
      if (i + 1 < n_w) {
        load(P2, fa[0], fw[0], i + 2);
        mma_pair(fa[1], fw[1]);
        pattern(C96(), C24(), C3());
      }
      i += 2;
    }
    for (; i + 2 <= n_w; i += 2) {
      load(P2, fa[1], fw[1], i + 1);
      mma_pair(fa[0], fw[0]);
      pattern(C96(), C24(), C3());
      load(P2, fa[0], fw[0], i + 2);
      mma_pair(fa[1], fw[1]);
      pattern(C96(), C24(), C3());
    }
    if (i < n_w) mma_pair(fa[0], fw[0]);
    // (fetched here, where the fragment registers are free, their latency under the LDS stores and the barrier)
    float e_bias[4][8], e_inv[4][8];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const f32x4 b0 = *reinterpret_cast<const f32x4*>(U.bias + q * H + g_unit);
      const f32x4 b1 = *reinterpret_cast<const f32x4*>(U.bias + q * H + g_unit + 4);
      const f32x4 s0 = *reinterpret_cast<const f32x4*>(U.inv_scale + q * H + g_unit);
      const f32x4 s1 = *reinterpret_cast<const f32x4*>(U.inv_scale + q * H + g_unit + 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) { e_bias[q][e] = b0[e]; e_bias[q][4 + e] = b1[e]; e_inv[q][e] = s0[e]; e_inv[q][4 + e] = s1[e]; }
    }

    if (u > u_beg) __syncthreads();   // the previous unit's finish has read its sums
    {
      float* pw = part + (size_t)wave * WAVE_FLOATS + col_off(l15 >> 2, l15 & 3) + 4 * lq;
#pragma unroll
      for (int cb = 0; cb < CB; ++cb)
#pragma unroll
        for (int r = 0; r < RT; ++r) *reinterpret_cast<f32x4*>(pw + cb * 4 * PLD + r * 16) = acc[r][cb];
    }
    __syncthreads();

    finish_pair(a, U, part, tid, m0, j0, e_c, e_hp, e_bias, e_inv, e_len);
  }
}

hipError_t launch_lstm_chain16_x3(const LstmX3Args& a, hipStream_t stream) {
  if (a.n_units == 0) return hipSuccess;
  dim3 grid(a.H / lx16::BU, (a.B + lx16::BM - 1) / lx16::BM, (a.n_units + a.units_per_block - 1) / a.units_per_block);
  return launch_lds(lstm_chain16_x3_kernel, grid, dim3(lx16::NT), lx16::LDS_BYTES, stream, a);
}
hipError_t launch_lstm_chain16_pair(const LstmX3Args& a, hipStream_t stream) {
  if (a.n_units == 0) return hipSuccess;
  dim3 grid(a.H / lx16::BU, (a.B + lx16::BM - 1) / lx16::BM, (a.n_units + a.units_per_block - 1) / a.units_per_block);
  return launch_lds(lstm_chain16_pair_kernel, grid, dim3(lx16::NT), lx16::LDS_BYTES, stream, a);
}

}  // namespace empose
