// The fused update MLP (mlp_fused.hip: all layers of one or two nets in ONE launch, activations resident in LDS) with
// every fp32 product formed on the bf16 matrix path from THREE bf16 pieces per operand -- fp32-equivalent arithmetic at
// 6/16 of the fp32 MFMA's cost.
//
//   x = x_h + x_m + x_l,   x_h = bf16(x), x_m = bf16(x - x_h), x_l = bf16(x - x_h - x_m)      (round to nearest, 8 + 8 + 8
//   w = w_h + w_m + w_l                                                                        mantissa bits: all 24)
//   x w  ~=  x_h w_h + (x_h w_m + x_m w_h) + (x_h w_l + x_m w_m + x_l w_h)
// Each piece product is exact (8 x 8 bits), the accumulation is the matrix core's fp32; what is dropped -- x_m w_l,
// x_l w_m, x_l w_l -- is below 2^-23 of the product, i.e. below the rounding the fp32 instruction commits on its own
// products.  (Two pieces, 2^-16, would not do for the 1e-4 parity bar through 4 x 6 layers; this is NOT the opt-in
// "bf16x3" of the full-mesh kernel, which keeps two pieces.)
// v_mfma_f32_32x32x16_bf16 retires 16 k per 32 cycles and SIMD where v_mfma_f32_32x32x2_f32 retires 2 k per 64: six of
// them per 16 k = 192 cycles against 512.
//
// Structure = mlp_fused.hip: a workgroup owns 64 rows of one net, its activations [64][<= 512] stay in ONE fp32 LDS
// buffer (three bf16 planes of it, 196 KB, would not fit), four waves of 64 rows x 128 columns, two barriers per layer.
//   * A side: a lane reads its 8 consecutive fp32 of a k-step (two ds_read_b128) and splits them into the three pieces in
//     registers (v_cvt_pk_bf16_f32 + shift/mask + subtract: 11 VALU per pair, 88 per k-step for the two row tiles,
//     hidden under the 48 MFMAs of the step).  Every wave splits the same A block: redundant, but free in the MFMA shadow,
//     whereas split planes in LDS would cost 64 more KB.
//   * B side: the weights are split ONCE at model creation (api_model.hip pack_fragments_x3_raw) and stored in fragment order, per
//     (k-step, 32-column tile, piece) one 1 KB wave fragment: lane (n = lane & 31, half = lane >> 5) owns
//     W_piece[tile * 32 + n][ks * 16 + half * 8 .. + 7].  They stream from L2 straight into a register ring, three
//     k-steps deep; 12 KB per wave and k-step.
//   * one wave per SIMD (132 KB of LDS per workgroup), as everything in this tree that issues the bf16 32x32x16 MFMA
//     (scripts/dev/bf16_hazard_repro.md).
// The default form since option mlp_pair16 is p16_layer below: TWO f16 pieces per operand under power-of-two scales
// (f16pair.h), three products instead of six, the same workgroup.
#include <type_traits>

#include "bf16x3.h"
#include "f16pair.h"
#include "gemm_epilogue.h"
#include "gemm_kernels.h"
#include "launch.h"
#include "mlp_kernels.h"
#include "stage_block.h"

namespace empose {

namespace fx {
constexpr int BM = 64, NT = 256;
constexpr int LDA = FUSED_MAX_WIDTH + 4;
constexpr size_t LDS_BYTES = (size_t)BM * LDA * sizeof(float) + 64;
constexpr int RING = 4;                      // weight ring: three k-steps in flight + the one being multiplied
}  // namespace fx

typedef const __attribute__((address_space(1))) char* fx_gbyte_t;

// the pieces of a lane's 8 consecutive k
__device__ __forceinline__ Pieces fx_split8(const f32x4& lo, const f32x4& hi) {
  return split8(lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]);
}

// One layer for the workgroup's 64 rows.  `act`: fp32 [64][lda], columns [0, 16 * KS4) valid or zero.
// The wave computes WM x WN tiles of 32 x 32 starting at (row_tile0, col_tile0).
template <int WM, int WN>
__device__ __forceinline__ void x3_layer(const FusedNet& net, const FusedLayer& L, int M, int m0, float* act, int lda,
                                         int row_tile0, int col_tile0, bool last) {
  using namespace fx;
  const int lane = threadIdx.x & 63;
  const int l31 = lane & 31, lh = lane >> 5;
  const int K = L.K, N = L.N;
  const int NT32 = (N + 31) / 32;
  const int KS4 = ((K + 15) / 16 + 3) & ~3;   // k-steps of the packed weights (zero-padded to whole quads)
  if (col_tile0 >= NT32) {   // wave-uniform: nothing of this layer falls to this wave; keep the two barriers
    __syncthreads();
    __syncthreads();
    return;
  }
  unsigned b_voff[WN];
#pragma unroll
  for (int j = 0; j < WN; ++j)
    b_voff[j] = (unsigned)((col_tile0 + j < NT32 ? col_tile0 + j : NT32 - 1) * 3072 + lane * 16);
  fx_gbyte_t wb = (fx_gbyte_t)L.W;
  const float* a_rd = act + (row_tile0 * 32 + l31) * lda + lh * 8;

  float e_sc[WN], e_sh[WN];
  const float e_slope = L.act == 1 ? L.slope : 1.f;
  const bool slope_unit = e_slope >= 0.f && e_slope <= 1.f;
#pragma unroll
  for (int j = 0; j < WN; ++j) {
    const int n = (col_tile0 + j) * 32 + l31;
    const bool real = n < N;
    const int nc = real ? n : N - 1;
    e_sc[j] = real ? (L.scale ? L.scale[nc] : 1.f) : 0.f;
    e_sh[j] = real ? (L.shift ? L.shift[nc] : 0.f) : 0.f;
  }

  f32x16 acc[WM][WN];
  f32x4 ra[2][WM][2];              // raw fp32 A: k-steps s + 1 (being split) and s + 2 (in flight from LDS)
  Pieces ap[2][WM];                // the pieces of k-steps s (multiplied) and s + 1 (being made)
  u32x4_t fb[RING][WN][3];         // weight pieces: slot s & 3 holds k-step s, loaded three steps ahead

  auto aread = [&](int ks, f32x4 (&a)[WM][2]) {
    const int kc = ks < KS4 ? ks : KS4 - 1;   // (the look-ahead past the last step stays inside the padded row)
#pragma unroll
    for (int i = 0; i < WM; ++i) {
      a[i][0] = *reinterpret_cast<const f32x4*>(a_rd + i * 32 * lda + kc * 16);
      a[i][1] = *reinterpret_cast<const f32x4*>(a_rd + i * 32 * lda + kc * 16 + 4);
    }
  };
  auto bload = [&](u32x4_t (&b)[WN][3], int ks) {
    const int kc = ks < KS4 ? ks : KS4 - 1;   // (clamped: fetched, never used)
    fx_gbyte_t p = wb + (size_t)kc * NT32 * 3072;
#pragma unroll
    for (int j = 0; j < WN; ++j)
#pragma unroll
      for (int q = 0; q < 3; ++q) b[j][q] = *(x3_gvec_t)(p + b_voff[j] + q * 1024);
  };
  auto split = [&](const f32x4 (&a)[WM][2], Pieces (&q)[WM]) {
#pragma unroll
    for (int i = 0; i < WM; ++i) q[i] = fx_split8(a[i][0], a[i][1]);
  };
  // One k-step as NCH chunks, each fenced by a scheduling barrier: 48 / NCH of the step's MFMAs, the split of ONE pair of the
  // next step's A values (11 VALU) and 16 / NCH of the step's memory operations (the weight loads of step s + 3, the LDS
  // reads of step s + 2).  Left to itself over a whole step (or four), the scheduler emits the split as one dependent
  // chain behind the MFMAs and sinks the LDS reads down to their use, where the split then waits for the round trip.
  auto step = [&](int s, const Pieces (&ap_cur)[WM], Pieces (&ap_nxt)[WM], f32x4 (&ra_nxt)[WM][2], f32x4 (&ra_free)[WM][2],
                  const u32x4_t (&b_cur)[WN][3], u32x4_t (&b_free)[WN][3]) {
    constexpr int NM = WM * WN * 6, NP = WM * 4, NMEM = 3 * WN + 2 * WM;   // MFMAs, pairs to split, memory operations
    constexpr int NCH = NP;                                                // one pair per chunk
    const int kb = s + 3 < KS4 ? s + 3 : KS4 - 1, ka = s + 2 < KS4 ? s + 2 : KS4 - 1;
    fx_gbyte_t pb = wb + (size_t)kb * NT32 * 3072;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      // ---- memory operations of this chunk
#pragma unroll
      for (int o = c * NMEM / NCH; o < (c + 1) * NMEM / NCH; ++o) {
        if (o < 3 * WN) {
          b_free[o / 3][o % 3] = *(x3_gvec_t)(pb + b_voff[o / 3] + (o % 3) * 1024);
        } else {
          const int r = o - 3 * WN;
          ra_free[r / 2][r % 2] = *reinterpret_cast<const f32x4*>(a_rd + (r / 2) * 32 * lda + ka * 16 + (r % 2) * 4);
        }
      }
      // ---- the split of pair c of the next step: row tile c / 4, k pair c % 4
      {
        const int i = c / 4, q = c % 4;
        const f32x4& v = ra_nxt[i][q / 2];
        unsigned h, m, l;
        split_pair(v[(q % 2) * 2], v[(q % 2) * 2 + 1], h, m, l);
        ap_nxt[i].p[0][q] = h; ap_nxt[i].p[1][q] = m; ap_nxt[i].p[2][q] = l;
      }
      // ---- this chunk's share of the step's MFMAs, in (product, row tile, column tile) order
#pragma unroll
      for (int mm = c * NM / NCH; mm < (c + 1) * NM / NCH; ++mm) {
        const int t = mm / (WM * WN), i = (mm / WN) % WM, j = mm % WN;
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, ap_cur[i].p[X3_PA[t]]),
                                                            __builtin_bit_cast(bf16x8_t, b_cur[j][X3_PB[t]]), acc[i][j], 0, 0, 0);
      }
#pragma unroll
      for (int mm = 0; mm < (NM + NCH - 1) / NCH; ++mm) { SGB(SG_MFMA, 1); SGB(SG_VALU, 2); if (mm < 2) SGB(SG_VMEM_RD | SG_DS_RD, 1); }
      __builtin_amdgcn_sched_barrier(0);
    }
  };
  auto quad = [&](int g) {
    step(g, ap[0], ap[1], ra[1], ra[0], fb[0], fb[3]);
    step(g + 1, ap[1], ap[0], ra[0], ra[1], fb[1], fb[0]);
    step(g + 2, ap[0], ap[1], ra[1], ra[0], fb[2], fb[1]);
    step(g + 3, ap[1], ap[0], ra[0], ra[1], fb[3], fb[2]);
  };

#pragma unroll
  for (int i = 0; i < WM; ++i)
#pragma unroll
    for (int j = 0; j < WN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  bload(fb[0], 0);
  bload(fb[1], 1);
  bload(fb[2], 2);
  aread(0, ra[0]);
  aread(1, ra[1]);
  split(ra[0], ap[0]);
  // the first quad is peeled so that the loop header merges two states with the same outstanding loads (mlp_fused.hip)
  quad(0);
  for (int g = 4; g < KS4; g += 4) quad(g);

  __syncthreads();   // every wave has read its last A fragment: the buffer may be overwritten
  if (last) {
    GemmProb p;
    p.C = net.out; p.ldc = net.ld_out;
    p.M = M; p.N = N; p.K = K;
    p.scale = L.scale; p.shift = L.shift; p.resid = nullptr; p.ldr = 0;
    p.act = L.act; p.slope = L.slope;
    p.A = nullptr; p.W = nullptr; p.lda = 0; p.ldw = 0;
    epilogue<WM, WN>(p, acc, m0 + row_tile0 * 32, col_tile0 * 32, l31, lh);
  } else {
#pragma unroll
    for (int j = 0; j < WN; ++j) {
      const int n = (col_tile0 + j) * 32 + l31;
      if (col_tile0 + j >= NT32) continue;
      if (slope_unit) {
#pragma unroll
        for (int i = 0; i < WM; ++i)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int row = (row_tile0 + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
            const float y = acc[i][j][r] * e_sc[j] + e_sh[j];
            act[row * lda + n] = fmaxf(y, y * e_slope);
          }
      } else {
#pragma unroll
        for (int i = 0; i < WM; ++i)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int row = (row_tile0 + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
            const float y = acc[i][j][r] * e_sc[j] + e_sh[j];
            act[row * lda + n] = y >= 0.f ? y : y * e_slope;
          }
      }
    }
  }
  __syncthreads();
}

// ---------------------------------------------------------------------------------------------------------------------
// What the two layers on the 16x16x32 instructions share (x16_layer: three bf16 pieces, p16_layer: two f16 pieces; their
// schedules are described there).  Each takes the caller's tid / l15 / lq / wave: re-derived from threadIdx.x here, they
// are computed twice.
// What they do NOT share although it reads alike: the wave's plan (col_tile0 .. step_bytes), the peeled pair loop and the
// L.N ladder of the kernel body.  Written once, each of the three changes the K loops the compiler emits (the waits at
// the head of p16_layer's loop, a last step of its own in x16_layer) and cost 1 to 2 us per launch where the parent's
// runs lay within 2 (profiles/mlp_scaffold_ab_parent_vs_head.txt); with what is below, every block of the two kernels that
// holds MFMAs has the parent's size.  A change to the plan or to the loop is made in both layers.
namespace l16 {
constexpr int RT = 4, NCHUNK = 8;   // a wave's 64 rows are four row tiles; a step is eight chunks, one per column tile

// Output column n's epilogue constants; a column past N gives zeros.  Returns the column to read further constants of.
__device__ __forceinline__ int col_consts(const float* scale, const float* shift, int n, int N, float& sc, float& sh) {
  const bool real = n < N;
  const int nc = real ? n : N - 1;
  sc = real ? (scale ? scale[nc] : 1.f) : 0.f;
  sh = real ? (shift ? shift[nc] : 0.f) : 0.f;
  return nc;
}

// K-split layers: every wave's partial sums go to the (then free) activation buffer as [wave][64][NC] ...
template <int NCT>
__device__ __forceinline__ void ksplit_spill(float* act, const f32x4 (&acc)[RT][NCT], int wave, int l15, int lq) {
  constexpr int NC = NCT * 16;
  float* pw = act + ((size_t)wave * fx::BM + 4 * lq) * NC + l15;
#pragma unroll
  for (int j = 0; j < NCT; ++j)
#pragma unroll
    for (int r = 0; r < RT; ++r)
#pragma unroll
      for (int e = 0; e < 4; ++e) pw[(r * 16 + e) * NC + j * 16] = acc[r][j][e];
}
// ... and, a barrier later, are added in wave order: thread (c16 = tid & 15, r16 = tid >> 4) takes column c16 of every
// column tile and rows r16, r16 + 16, .. -- shifts and masks only (a division by NC here is loop-invariant, gets hoisted
// out of the layer loop and lives through every K loop); a row's columns lie in 16 adjacent lanes.
// `fin(j, rr, nc, sum, sc, sh)` is what the layer does with the sum of (column tile j, row r16 + 16 rr).
template <int NCT, typename Fin>
__device__ __forceinline__ void ksplit_sum(const float* act, int tid, int N, const float* scale, const float* shift, Fin fin) {
  constexpr int NC = NCT * 16;
  const int c16 = tid & 15, r16 = tid >> 4;
#pragma unroll
  for (int j = 0; j < NCT; ++j) {
    const int n = j * 16 + c16;
    float sc, sh;
    const int nc = col_consts(scale, shift, n, N, sc, sh);
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const float* ps = act + (r16 + 16 * rr) * NC + n;
      fin(j, rr, nc, ((ps[0] + ps[fx::BM * NC]) + ps[2 * fx::BM * NC]) + ps[3 * fx::BM * NC], sc, sh);
    }
  }
}

// The last layer's results, fp32 [64][lda] in LDS, go out to global memory by all threads, coalesced, after the layer's
// final barrier: no global store while any MFMA of the workgroup is in flight (bf16x3.h).
__device__ __forceinline__ void copy_out(const FusedNet& net, const float* act, int lda, int M, int m0, int N, int tid) {
  float* const out = net.out;
  const int ld_out = net.ld_out;
  const int rows = M - m0 < fx::BM ? M - m0 : fx::BM;
  for (int idx = tid; idx < rows * N; idx += fx::NT) {
    const int r = idx / N, n = idx - r * N;
    out[(size_t)(m0 + r) * ld_out + n] = act[r * lda + n];
  }
}
}  // namespace l16

// ---------------------------------------------------------------------------------------------------------------------
// The same layer on v_mfma_f32_16x16x32_bf16 (option mlp_fused16): same workgroup, same single fp32 activation buffer, same
// pieces of the same values, weights from L2 into registers, no barrier in the K loop.  Where the chip holds its clock down
// under matrix load it holds a higher one on this shape at equal cycles per FLOP; what the shape takes away is issue room --
// an MFMA gap is 16 cycles, 8 of them the MFMA's own -- so every filler has its place:
//   * a wave's 64 x 128 tile is 4 x 8 accumulator tiles of 16 x 16 (C layout: col = lane & 15, row = 4 (lane >> 4) + reg); a
//     k-step is 32 wide and lane (r = lane & 15, q = lane >> 4) owns k = 8 q .. 8 q + 7 of it, on both operands;
//   * weights in the order of api_model.hip pack_fragments_x3_16_raw: [k-step of 32][16-column tile][piece] -> 1 KB;
//   * a step is 8 chunks, one per column tile: the tile's 24 MFMAs (six products x four row tiles; the products of one
//     accumulator in the order of bf16x3.h) with, between them, the split of two of the next step's 16 k pairs (22 VALU),
//     one ds_read_b128 and the three weight fragments of the tile just finished, for the next step.  So ONE set of weight
//     registers (96) and ONE of raw fp32 A values (32) are each refilled 7/8 of a step (~2,700 cycles) before their use;
//     only the A pieces (2 x 48) are double.  With the 128 accumulators ~350 registers;
//   * the A read -- 16 rows at stride LDA = 516 floats, four k-quarters 8 floats apart -- is 2-way conflicted in each of the
//     ds_read_b128's groups of 16 lanes (rows 12, 13 of quarter q meet rows 4, 5 of quarter q + 1), and no pad repairs it:
//     a group holds two quarters of 8 rows each, and the quarters' offset of two 16-byte slots is even.  8 LDS cycles per
//     read instead of 4, 32 reads per step and workgroup: 256 of a step's 3,072 cycles of an otherwise idle LDS.  Left;
//   * layer 0's ragged K (296 = 9 steps and a quarter): the lanes whose k does not exist read ZEROS that the staging loop
//     wrote (it fills up to whole pairs of steps, kpad), and the packed weights are zero there too: 0 x 0, never 0 x garbage;
//   * layers of up to 128 columns (the output layers: 66 -> 5 tiles, 10 -> 1; hidden widths 64, 128) are split over the waves
//     by K instead of by columns (KSPLIT): every wave multiplies all 64 rows x NCT column tiles for the steps w, w + 4, ...,
//     the partial sums meet in the (then free) activation buffer and are added in wave order.  Split by rows, each wave
//     would stream all of the layer's weights: four times the L2 traffic for the same MFMAs;
//   * every layer leaves its results in the activation buffer; the last one's then go out to global memory by all threads,
//     coalesced, after the barrier: no global store while any MFMA of the workgroup is in flight (bf16x3.h).
template <int NCT, bool KSPLIT>
__device__ __forceinline__ void x16_layer(const FusedNet& net, const FusedLayer& L, int M, int m0, float* act, int lda,
                                          int wave, bool last) {
  using namespace l16;
  static_assert(NCT >= 1 && NCT <= 8, "a wave owns up to 128 columns");
  const int tid = threadIdx.x, lane = tid & 63;
  const int l15 = lane & 15, lq = lane >> 4;
  const int K = L.K, N = L.N;
  const int NT16 = (N + 15) / 16;
  const int KS2 = ((K + 31) / 32 + 1) & ~1;                 // k-steps of the packed weights (zero-padded to whole pairs)
  const int col_tile0 = KSPLIT ? 0 : wave * NCT;
  // the wave's steps: g0, g0 + gs, ... (n_w of them; a wave that owns no column of the layer has none)
  const int g0 = KSPLIT ? wave : 0, gs = KSPLIT ? 4 : 1;
  const int n_w = KSPLIT ? (KS2 - wave + 3) / 4 : (col_tile0 < NT16 ? KS2 : 0);
  auto gk = [&](int i) { const int g = g0 + i * gs; return g < KS2 ? g : KS2 - 1; };   // (look-ahead past the end: clamped)
  // a fragment's address: wave-uniform (step, column tile: scalar registers) + the lane's 16 bytes (one register for all)
  const unsigned b_lane = (unsigned)lane * 16u;
  auto tile_off = [&](int j) { return (size_t)(col_tile0 + j < NT16 ? col_tile0 + j : NT16 - 1) * 3072; };
  fx_gbyte_t wb = (fx_gbyte_t)L.W;
  const size_t step_bytes = (size_t)NT16 * 3072;
  const float* a_rd = act + l15 * lda + lq * 8;

  f32x4 acc[RT][NCT];
  f32x4 raw[RT][2];                // raw fp32 A, slot c = (row tile c / 2, half c % 2): split in chunk c, read again in chunk c + 1
  Pieces ap[2][RT];                // the pieces of the step being multiplied and of the next one, being made
  u32x4_t fb[NCT][3];              // weight pieces of column tile j: multiplied in chunk j, loaded again in chunk j + 1

  auto bload = [&](u32x4_t (&b)[3], fx_gbyte_t p, int j) {
#pragma unroll
    for (int q = 0; q < 3; ++q) b[q] = *(x3_gvec_t)(p + tile_off(j) + q * 1024 + b_lane);
  };
  auto aread = [&](f32x4& r, const float* p, int c) {
    r = *reinterpret_cast<const f32x4*>(p + (c / 2) * 16 * lda + (c % 2) * 4);
  };
  auto split_slot = [&](const f32x4& v, Pieces& q, int h) {   // the two k pairs of half h of a lane's 8 k
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      unsigned ph, pm, pl;
      split_pair(v[2 * e], v[2 * e + 1], ph, pm, pl);
      q.p[0][2 * h + e] = ph; q.p[1][2 * h + e] = pm; q.p[2][2 * h + e] = pl;
    }
  };
  // the wave's step number i: multiplies ap_cur by fb, makes ap_nxt
  auto step = [&](int i, const Pieces (&ap_cur)[RT], Pieces (&ap_nxt)[RT]) {
    const int g1 = gk(i + 1);
    fx_gbyte_t pb_cur = wb + (size_t)gk(i) * step_bytes, pb_nxt = wb + (size_t)g1 * step_bytes;
    const float* pa1 = a_rd + g1 * 32;
    const float* pa2 = a_rd + gk(i + 2) * 32;
#pragma unroll
    for (int c = 0; c < NCHUNK; ++c) {
      // ---- refills: what the previous chunk has finished with (chunk 0: the last slots, still for this / the next step)
      if (c == 0) {
        if constexpr (NCT == 8) bload(fb[NCT - 1], pb_cur, NCT - 1);
        aread(raw[RT - 1][1], pa1, NCHUNK - 1);
      } else {
        if (c - 1 < NCT) bload(fb[c - 1 < NCT ? c - 1 : 0], pb_nxt, c - 1 < NCT ? c - 1 : 0);
        aread(raw[(c - 1) / 2][(c - 1) % 2], pa2, c - 1);
      }
      // ---- the split of slot c of the next step
      split_slot(raw[c / 2][c % 2], ap_nxt[c / 2], c % 2);
      // ---- the 24 MFMAs of column tile c
      if (c < NCT) {
        const int j = c < NCT ? c : 0;
#pragma unroll
        for (int mm = 0; mm < 6 * RT; ++mm) {
          const int t = mm / RT, r = mm % RT;
          acc[r][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, ap_cur[r].p[X3_PA[t]]),
                                                              __builtin_bit_cast(bf16x8_t, fb[j][X3_PB[t]]), acc[r][j], 0, 0, 0);
        }
#pragma unroll
        for (int mm = 0; mm < 6 * RT; ++mm) { SGB(SG_MFMA, 1); SGB(SG_VALU, 1); if (mm < 4) SGB(SG_VMEM_RD | SG_DS_RD, 1); }
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  };

#pragma unroll
  for (int r = 0; r < RT; ++r)
#pragma unroll
    for (int j = 0; j < NCT; ++j) acc[r][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // ---- prologue: weights of the first step (all but the tile its chunk 0 loads), its pieces, the raw values of the second
  {
    fx_gbyte_t pb0 = wb + (size_t)gk(0) * step_bytes;
#pragma unroll
    for (int j = 0; j < (NCT == 8 ? NCT - 1 : NCT); ++j) bload(fb[j], pb0, j);
#pragma unroll
    for (int c = 0; c < NCHUNK; ++c) aread(raw[c / 2][c % 2], a_rd + gk(0) * 32, c);
#pragma unroll
    for (int c = 0; c < NCHUNK; ++c) split_slot(raw[c / 2][c % 2], ap[0][c / 2], c % 2);
#pragma unroll
    for (int c = 0; c < NCHUNK - 1; ++c) aread(raw[c / 2][c % 2], a_rd + gk(1) * 32, c);
  }
  // the first pair is peeled so that the loop header merges two states with the same outstanding loads (mlp_fused.hip):
  // entered from the prologue, the loop began with a wait for ALL of them
  int i = 0;
  if (n_w >= 2) {
    step(0, ap[0], ap[1]);
    step(1, ap[1], ap[0]);
    i = 2;
  }
  for (; i + 2 <= n_w; i += 2) {
    step(i, ap[0], ap[1]);
    step(i + 1, ap[1], ap[0]);
  }
  if (i < n_w) step(i, ap[0], ap[1]);

  const float e_slope = L.act == 1 ? L.slope : 1.f;         // slope 1: no activation (exact identity)
  const float* const scale = L.scale;
  const float* const shift = L.shift;
  if constexpr (!KSPLIT) {
    float e_sc[NCT], e_sh[NCT];
#pragma unroll
    for (int j = 0; j < NCT; ++j) col_consts(scale, shift, (col_tile0 + j) * 16 + l15, N, e_sc[j], e_sh[j]);
    __syncthreads();   // every wave has read its last A values: the buffer may be overwritten
#pragma unroll
    for (int j = 0; j < NCT; ++j) {
      if (col_tile0 + j >= NT16) continue;
      const int n = (col_tile0 + j) * 16 + l15;
#pragma unroll
      for (int r = 0; r < RT; ++r)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float y = acc[r][j][e] * e_sc[j] + e_sh[j];
          act[(r * 16 + 4 * lq + e) * lda + n] = y >= 0.f ? y : y * e_slope;
        }
    }
  } else {
    __syncthreads();   // every wave has read its last A values: the buffer is free for the partial sums
    ksplit_spill<NCT>(act, acc, wave, l15, lq);
    __syncthreads();
    const int c16 = tid & 15, r16 = tid >> 4;
    float y[NCT][4];
    ksplit_sum<NCT>(act, tid, N, scale, shift, [&](int j, int rr, int, float sum, float sc, float sh) {
      const float v = sum * sc + sh;
      y[j][rr] = v >= 0.f ? v : v * e_slope;
    });
    __syncthreads();   // the partial sums are read: the activations take their place
#pragma unroll
    for (int j = 0; j < NCT; ++j)
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) act[(r16 + 16 * rr) * lda + j * 16 + c16] = y[j][rr];
  }
  __syncthreads();
  if (last) copy_out(net, act, lda, M, m0, N, tid);   // (no MFMA of the workgroup is in flight: every accumulator was read)
}

// ---------------------------------------------------------------------------------------------------------------------
// The same layer with every fp32 product formed from TWO f16 pieces per operand (f16pair.h; option mlp_pair16): three
// v_mfma_f32_16x16x32_f16 per accumulator and k-step instead of six of the bf16 instruction -- same shape, rate and
// fragment layout as x16_layer's, half the executed matrix work.  x16_layer's skeleton (64 rows, four waves, column split
// for wide layers, K split up to 128 columns, weights from L2 into registers, no barrier in the K loop, results through
// LDS, the last layer out by the coalesced copy: namespace l16 above), and what differs:
//   * a (hi, lo) pair is 4 bytes, the size of the fp32 it replaces, so the activation buffer holds FINISHED pieces: two
//     f16 planes [64][PLD], a lane's A fragment of a piece is one ds_read_b128 and the K loop has no split, no VALU at
//     all.  PLD = 528 halves: a row is 66 16-byte slots, and 66 = 2 (mod 16) spreads each of the ds_read_b128's lane
//     groups (rows 0-3, 12-15 of one k quarter with rows 4-11 of the next) over all 16 slots of a bank row: conflict-free;
//   * the pieces of a row need the row's scale, the scale the row's largest magnitude: the epilogue keeps its results in
//     registers, reduces the maxima (in the lane; over the 16 lanes of a row, which are a DPP row: no LDS trip, and as a
//     reduce-scatter of the lane's 16 rows that leaves one row per lane; over the four waves by ONE LDS atomic of all lanes
//     on a 64-word array), and writes the pieces after ONE more barrier than x16_layer has.  Nothing in it compares: 128
//     select masks per wave did not fit the scalar registers (p16_activation, pair16::finite_key).  The K-split layers
//     need neither the atomic nor the barrier: their reduction already has a row's columns in 16 adjacent lanes.  Two
//     arrays of maxima alternate by layer: the scale a layer's input was packed with is undone in that layer's epilogue;
//   * two adjacent lanes exchange half of their values (DPP again), so that each writes (column, column + 1) of two rows
//     as one word: as many LDS writes as x16_layer's fp32 results took;
//   * weights in the order of api_model.hip pack_fragments_pair16_raw: [k-step of 32][16-column tile][piece] -> 1 KB, with
//     the columns' inverse scales beside them (FusedLayer::wexp).  A chunk is one column tile's 12 MFMAs with one A
//     fragment of the next step and the two weight fragments of the tile just finished, for the step AFTER the next: the
//     registers the third piece and the raw values gave back hold a second set of weights, so a fragment is asked for
//     1 7/8 steps (~2,900 cycles, as before) ahead of its use although a step is half as long;
//   * the last layer leaves fp32 results in the same memory at x16_layer's stride.
namespace fx {
constexpr int PLD = FUSED_MAX_WIDTH + 16;                       // halves per row of a piece plane
constexpr int PLANE_BYTES = BM * PLD * 2;
constexpr size_t LDS_BYTES_P = (size_t)2 * PLANE_BYTES + 2 * BM * sizeof(unsigned);   // + the two arrays of row maxima
static_assert((size_t)2 * PLANE_BYTES >= (size_t)BM * LDA * sizeof(float), "the last layer's fp32 results fit");
static_assert((size_t)2 * PLANE_BYTES >= (size_t)4 * BM * 128 * sizeof(float), "the K-split partial sums fit");
}  // namespace fx

typedef __attribute__((address_space(3))) char* p16_lds_t;
// a value of the lane next door (lane ^ 1)
__device__ __forceinline__ float p16_swap1(float v) {
  const int b = __builtin_bit_cast(int, v);                 // (`old` = the source: no register to set up, f16pair.h)
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(b, b, pair16::DPP_XOR1, 0xf, 0xf, false));
}
// A lane's four scaled values of one (row tile, column tile) -- rows e = 0 .. 3 of column c -- go out as pieces: the even
// lane takes rows 0, 1 and the odd lane rows 2, 3 of the columns (c & ~1, c | 1) of both; the two trade through DPP.
// `p_hi`, `p_lo`: where the lane's first piece pair goes in either plane (PLANE_BYTES apart is past a ds_write's 16-bit
// offset: one address register per plane, everything else an immediate `off`); `row2`: bytes to its second pair.
__device__ __forceinline__ void p16_put4(p16_lds_t p_hi, p16_lds_t p_lo, int off, int row2, bool odd, float v0, float v1,
                                         float v2, float v3) {
  const float r0 = p16_swap1(odd ? v0 : v2), r1 = p16_swap1(odd ? v1 : v3);
  unsigned h0, l0, h1, l1;
  pair16::split_pair(odd ? r0 : v0, odd ? v2 : r0, h0, l0);
  pair16::split_pair(odd ? r1 : v1, odd ? v3 : r1, h1, l1);
  typedef __attribute__((address_space(3))) unsigned* word_t;
  *(word_t)(p_hi + off) = h0;
  *(word_t)(p_lo + off) = l0;
  *(word_t)(p_hi + off + row2) = h1;
  *(word_t)(p_lo + off + row2) = l1;
}
// The address of a lane's first store in either plane, each in a register of its own (left to itself the compiler keeps
// one and adds the planes' distance, which no immediate holds, before every second store).
__device__ __forceinline__ void p16_planes(char* p, p16_lds_t& p_hi, p16_lds_t& p_lo) {
  unsigned a = (unsigned)(size_t)(p16_lds_t)p, b = a + (unsigned)fx::PLANE_BYTES;
  asm volatile("" : "+v"(a), "+v"(b));
  p_hi = (p16_lds_t)(size_t)a;
  p_lo = (p16_lds_t)(size_t)b;
}

// y >= 0 ? y : y slope.  For a slope in (0, 1] (UNIT) that is the larger of y and y slope, bit for bit: both zeros keep
// their sign (-0 slope = -0), +-inf and NaN come out as they do from the select.  One v_max_f32 and no compare mask: 128 of
// those per wave and layer did not fit the scalar registers.  Slope 0 is not UNIT: -inf x 0 is NaN, which a maximum drops.
// `ys`: y slope, the caller's (packed) multiply.
template <bool UNIT>
__device__ __forceinline__ float p16_activation(float y, float ys) {
  if constexpr (UNIT) return fmaxf(y, ys);
  else return y >= 0.f ? y : ys;
}

// Layer 0's input: row-major x[M][ldx], rows m0 .. m0 + 63, columns [0, K0) -> the piece planes, columns [K0, kpad) zero;
// rows past M - 1 repeat row M - 1 (never stored).  16 lanes share a row (256-byte runs), a thread holds its 4 rows x
// kpad / 64 chunks of 16 bytes in registers -- all loads in flight (stage_block.h) -- until the row maxima are known.
__device__ __forceinline__ void p16_stage(const float* x, int ldx, int m0, int M, int K0, int kpad, char* lds, unsigned* mx) {
  const int tid = threadIdx.x, l15 = tid & 15, rg = tid >> 4;
  const int k4 = K0 >> 2, nu = kpad >> 6;       // nu <= 8: kpad <= FUSED_MAX_WIDTH
  const int r_max = M - 1 - m0;
  const stage::gbyte_t xb = (stage::gbyte_t)(x + (size_t)m0 * ldx);
  const unsigned ldx4 = (unsigned)ldx * 4u;
  f32x4 v[4][8];
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    const int row = rg + 16 * rr, rc = row < r_max ? row : r_max;
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (u < nu) {                             // wave-uniform
        const int c = l15 + 16 * u, cc = c < k4 ? c : k4 - 1;
        v[rr][u] = *(stage::gvec_t)(xb + ((unsigned)rc * ldx4 + (unsigned)cc * 16u));
      }
  }
  p16_lds_t p_hi, p_lo;
  p16_planes(lds + (rg * fx::PLD + l15 * 4) * 2, p_hi, p_lo);
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    const int row = rg + 16 * rr;
    unsigned key = pair16::KEY_ZERO;
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (u < nu) {
        if (l15 + 16 * u >= k4) v[rr][u] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const unsigned b = pair16::finite_key(v[rr][u][e]);
          key = b > key ? b : key;
        }
      }
    const unsigned m = pair16::key_bits(pair16::max16(key));
    if (l15 == 0) mx[row] = m;
    const float s = pair16::pow2(pair16::scale_exp(m));
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (u < nu) {
        typedef unsigned u32x2_t __attribute__((ext_vector_type(2)));
        typedef __attribute__((address_space(3))) u32x2_t* pair_t;
        unsigned h0, l0, h1, l1;
        pair16::split_pair(v[rr][u][0] * s, v[rr][u][1] * s, h0, l0);
        pair16::split_pair(v[rr][u][2] * s, v[rr][u][3] * s, h1, l1);
        const int off = (16 * rr * fx::PLD + 16 * u * 4) * 2;
        *(pair_t)(p_hi + off) = u32x2_t{h0, h1};
        *(pair_t)(p_lo + off) = u32x2_t{l0, l1};
      }
  }
}

// `lds`: the two piece planes, columns [0, 32 KS2) of the layer's input valid or zero; `mx_in`: the row maxima that input
// was scaled by, `mx_out`: those of this layer's results (left for the next layer).
template <int NCT, bool KSPLIT>
__device__ __forceinline__ void p16_layer(const FusedNet& net, const FusedLayer& L, int M, int m0, char* lds,
                                          const unsigned* mx_in, unsigned* mx_out, int wave, bool last) {
  using namespace l16;
  static_assert(NCT >= 1 && NCT <= 8, "a wave owns up to 128 columns");
  const int tid = threadIdx.x, lane = tid & 63;
  const int l15 = lane & 15, lq = lane >> 4;
  const int K = L.K, N = L.N;
  const int NT16 = (N + 15) / 16;
  const int KS2 = ((K + 31) / 32 + 1) & ~1;                 // k-steps of the packed weights (zero-padded to whole pairs)
  const int col_tile0 = KSPLIT ? 0 : wave * NCT;
  const int g0 = KSPLIT ? wave : 0, gs = KSPLIT ? 4 : 1;
  const int n_w = KSPLIT ? (KS2 - wave + 3) / 4 : (col_tile0 < NT16 ? KS2 : 0);
  auto gk = [&](int i) { const int g = g0 + i * gs; return g < KS2 ? g : KS2 - 1; };   // (look-ahead past the end: clamped)
  const unsigned b_lane = (unsigned)lane * 16u;
  auto tile_off = [&](int j) { return (size_t)(col_tile0 + j < NT16 ? col_tile0 + j : NT16 - 1) * 2048; };
  fx_gbyte_t wb = (fx_gbyte_t)L.W;
  const size_t step_bytes = (size_t)NT16 * 2048;
  const char* a_rd = lds + (l15 * fx::PLD + lq * 8) * 2;
  float* const act = reinterpret_cast<float*>(lds);         // the same memory as fp32, once the K loop has read its last
  constexpr int lda = fx::LDA;

  if (tid < fx::BM) mx_out[tid] = 0u;                       // (last read before the previous layer's final barrier)

  f32x4 acc[RT][NCT];
  u32x4_t ap[2][RT][2];            // A pieces of the step being multiplied and of the next one, in flight from LDS
  u32x4_t fb[2][NCT][2];           // weight pieces of two steps: tile j multiplied in chunk j, asked for again in chunk j + 1

  auto bload = [&](u32x4_t (&b)[2], int g, int j) {
    fx_gbyte_t p = wb + (size_t)g * step_bytes + tile_off(j) + b_lane;
    b[0] = *(x3_gvec_t)p;
    b[1] = *(x3_gvec_t)(p + 1024);
  };
  auto aread = [&](u32x4_t (&a)[RT][2], int g, int c) {     // slot c = (row tile c / 2, piece c % 2) of step g
    a[c / 2][c % 2] = *reinterpret_cast<const u32x4_t*>(a_rd + (c / 2) * 16 * fx::PLD * 2 + (c % 2) * fx::PLANE_BYTES + g * 64);
  };
  // the wave's step number i: multiplies ap_cur by fb_cur, fetches ap_nxt; fb_oth holds the next step's weights
  auto step = [&](int i, const u32x4_t (&ap_cur)[RT][2], u32x4_t (&ap_nxt)[RT][2], u32x4_t (&fb_cur)[NCT][2],
                  u32x4_t (&fb_oth)[NCT][2]) {
    const int g1 = gk(i + 1), g2 = gk(i + 2);
#pragma unroll
    for (int c = 0; c < NCHUNK; ++c) {
      if (c == 0) {
        if constexpr (NCT == 8) bload(fb_oth[NCT - 1], g1, NCT - 1);   // (the previous step's last tile)
      } else if (c - 1 < NCT) {
        bload(fb_cur[c - 1 < NCT ? c - 1 : 0], g2, c - 1 < NCT ? c - 1 : 0);
      }
      aread(ap_nxt, g1, c);
      if (c < NCT) {
        const int j = c < NCT ? c : 0;
#pragma unroll
        for (int mm = 0; mm < 3 * RT; ++mm) {
          const int t = mm / RT, r = mm % RT;
          acc[r][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, ap_cur[r][pair16::PA[t]]),
                                                             __builtin_bit_cast(f16x8_t, fb_cur[j][pair16::PB[t]]), acc[r][j], 0, 0, 0);
        }
#pragma unroll
        for (int mm = 0; mm < 3 * RT; ++mm) { SGB(SG_MFMA, 1); if (mm < 3) SGB(SG_VMEM_RD | SG_DS_RD, 1); }
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  };

#pragma unroll
  for (int r = 0; r < RT; ++r)
#pragma unroll
    for (int j = 0; j < NCT; ++j) acc[r][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // ---- prologue: the weights of the first two steps (but the tile the first chunk asks for), the A pieces of the first
#pragma unroll
  for (int j = 0; j < NCT; ++j) bload(fb[0][j], gk(0), j);
#pragma unroll
  for (int j = 0; j < (NCT == 8 ? NCT - 1 : NCT); ++j) bload(fb[1][j], gk(1), j);
#pragma unroll
  for (int c = 0; c < NCHUNK; ++c) aread(ap[0], gk(0), c);
  // the first pair is peeled so that the loop header merges two states with the same outstanding loads (mlp_fused.hip)
  int i = 0;
  if (n_w >= 2) {
    step(0, ap[0], ap[1], fb[0], fb[1]);
    step(1, ap[1], ap[0], fb[1], fb[0]);
    i = 2;
  }
  for (; i + 2 <= n_w; i += 2) {
    step(i, ap[0], ap[1], fb[0], fb[1]);
    step(i + 1, ap[1], ap[0], fb[1], fb[0]);
  }
  if (i < n_w) step(i, ap[0], ap[1], fb[0], fb[1]);

  const float e_slope = L.act == 1 ? L.slope : 1.f;         // slope 1: no activation (exact identity)
  const bool slope_unit = e_slope > 0.f && e_slope <= 1.f;  // (wave-uniform) the activation is then a maximum, p16_activation
  const float* const scale = L.scale;
  const float* const shift = L.shift;
  const float* const wexp = L.wexp;
  if constexpr (!KSPLIT) {
    float e_ci[NCT], e_sc[NCT], e_sh[NCT];
#pragma unroll
    for (int j = 0; j < NCT; ++j) {
      const int nc = col_consts(scale, shift, (col_tile0 + j) * 16 + l15, N, e_sc[j], e_sh[j]);
      e_ci[j] = wexp[nc];
    }
    const bool mine = col_tile0 < NT16;                     // (wave-uniform; a tile past N gives zeros: e_sc, e_sh)
    unsigned key[RT * 4];                                   // pair16::finite_key maxima of the lane's rows (r, e)
    auto finish = [&](auto unit) {
      // (rows in pairs, spelled as vectors: the multiplies and the fused multiply-add are packed instructions, which the
      // compiler no longer finds by itself once the activation, which has no packed form, is a maximum)
#pragma unroll
      for (int r = 0; r < RT; ++r)
#pragma unroll
        for (int e = 0; e < 4; e += 2) {
          const f32x2_t ri = {pair16::pow2(-pair16::scale_exp(mx_in[r * 16 + 4 * lq + e])),
                              pair16::pow2(-pair16::scale_exp(mx_in[r * 16 + 4 * lq + e + 1]))};
          unsigned k0 = pair16::KEY_ZERO, k1 = pair16::KEY_ZERO;
#pragma unroll
          for (int j = 0; j < NCT; ++j) {
            const f32x2_t a = {acc[r][j][e], acc[r][j][e + 1]};
            const f32x2_t y = __builtin_elementwise_fma((a * e_ci[j]) * ri, f32x2_t{e_sc[j], e_sc[j]}, f32x2_t{e_sh[j], e_sh[j]});
            const f32x2_t z = y * e_slope;
            acc[r][j][e] = p16_activation<decltype(unit)::value>(y[0], z[0]);
            acc[r][j][e + 1] = p16_activation<decltype(unit)::value>(y[1], z[1]);
            const unsigned b0 = pair16::finite_key(acc[r][j][e]), b1 = pair16::finite_key(acc[r][j][e + 1]);
            k0 = b0 > k0 ? b0 : k0;
            k1 = b1 > k1 ? b1 : k1;
          }
          key[r * 4 + e] = k0;
          key[r * 4 + e + 1] = k1;
        }
    };
    if (slope_unit) finish(std::true_type{});
    else finish(std::false_type{});
    unsigned mr = 0u;                                       // lane l15 of a row group: the maximum of the group's row l15
    if (!last && mine) mr = pair16::key_bits(pair16::max16_scatter(key, l15));
    __syncthreads();   // every wave has read its last A pieces: the buffer may be overwritten
    if (last) {
      if (mine) {
#pragma unroll
        for (int j = 0; j < NCT; ++j) {
          if (col_tile0 + j >= NT16) continue;
          const int n = (col_tile0 + j) * 16 + l15;
#pragma unroll
          for (int r = 0; r < RT; ++r)
#pragma unroll
            for (int e = 0; e < 4; ++e) act[(r * 16 + 4 * lq + e) * lda + n] = acc[r][j][e];
        }
      }
    } else {
      // one ds_max_u32 of all 64 lanes: lane l15 = 4 r + e holds row (r, e) of its group's sixteen
      if (mine) atomicMax(&mx_out[(l15 >> 2) * 16 + 4 * lq + (l15 & 3)], mr);
      __syncthreads();   // the rows' maxima are complete
      if (mine) {
        const bool odd = l15 & 1;
        p16_lds_t p_hi, p_lo;
        p16_planes(lds + ((4 * lq + (odd ? 2 : 0)) * fx::PLD + col_tile0 * 16 + (l15 & ~1)) * 2, p_hi, p_lo);
#pragma unroll
        for (int r = 0; r < RT; ++r) {
          float s[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) s[e] = pair16::pow2(pair16::scale_exp(mx_out[r * 16 + 4 * lq + e]));
#pragma unroll
          for (int j = 0; j < NCT; ++j) {
            const f32x2_t v01 = f32x2_t{acc[r][j][0], acc[r][j][1]} * f32x2_t{s[0], s[1]};
            const f32x2_t v23 = f32x2_t{acc[r][j][2], acc[r][j][3]} * f32x2_t{s[2], s[3]};
            p16_put4(p_hi, p_lo, (r * 16 * fx::PLD + j * 16) * 2, fx::PLD * 2, odd, v01[0], v01[1], v23[0], v23[1]);
          }
        }
      }
    }
  } else {
    __syncthreads();   // every wave has read its last A pieces: the buffer is free for the partial sums
    ksplit_spill<NCT>(act, acc, wave, l15, lq);
    __syncthreads();
    const int c16 = tid & 15, r16 = tid >> 4;
    float y[NCT][4];
    unsigned key[4] = {pair16::KEY_ZERO, pair16::KEY_ZERO, pair16::KEY_ZERO, pair16::KEY_ZERO};
    float ri[4];
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) ri[rr] = pair16::pow2(-pair16::scale_exp(mx_in[r16 + 16 * rr]));
    ksplit_sum<NCT>(act, tid, N, scale, shift, [&](int j, int rr, int nc, float sum, float sc, float sh) {
      y[j][rr] = ((sum * wexp[nc]) * ri[rr]) * sc + sh;
    });
    auto finish = [&](auto unit) {
#pragma unroll
      for (int j = 0; j < NCT; ++j)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          y[j][rr] = p16_activation<decltype(unit)::value>(y[j][rr], y[j][rr] * e_slope);
          const unsigned b = pair16::finite_key(y[j][rr]);
          key[rr] = b > key[rr] ? b : key[rr];
        }
    };
    if (slope_unit) finish(std::true_type{});
    else finish(std::false_type{});
    __syncthreads();   // the partial sums are read: the results take their place
    if (last) {
#pragma unroll
      for (int j = 0; j < NCT; ++j)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) act[(r16 + 16 * rr) * lda + j * 16 + c16] = y[j][rr];
    } else {
      float s[4];
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const unsigned m = pair16::key_bits(pair16::max16(key[rr]));
        if (c16 == 0) mx_out[r16 + 16 * rr] = m;
        s[rr] = pair16::pow2(pair16::scale_exp(m));
      }
      // (lane pairs as in the wide layers, the four values of a lane now 16 rows apart)
      const bool odd = c16 & 1;
      p16_lds_t p_hi, p_lo;
      p16_planes(lds + ((r16 + (odd ? 32 : 0)) * fx::PLD + (c16 & ~1)) * 2, p_hi, p_lo);
#pragma unroll
      for (int j = 0; j < NCT; ++j)
        p16_put4(p_hi, p_lo, j * 16 * 2, 16 * fx::PLD * 2, odd, y[j][0] * s[0], y[j][1] * s[1], y[j][2] * s[2], y[j][3] * s[3]);
    }
  }
  __syncthreads();
  if (last) copy_out(net, act, lda, M, m0, N, tid);   // (no MFMA of the workgroup is in flight: every accumulator was read)
}

// SHAPE: the MFMA the products run on -- 32: v_mfma_f32_32x32x16_bf16 (x3_layer), 16: v_mfma_f32_16x16x32_bf16
// (x16_layer), PAIR16: v_mfma_f32_16x16x32_f16 on two f16 pieces (p16_layer); each with its own order of the packed
// weights.  One name for all, as the profile readers know it.
constexpr int PAIR16 = 2;
template <int SHAPE>
__global__ __launch_bounds__(fx::NT) void mlp_fused_x3_kernel(FusedMlpArgs args) {
  X3_EXCLUSIVE_SIMD();
  using namespace fx;
  static_assert(SHAPE == 32 || SHAPE == 16 || SHAPE == PAIR16, "the two shapes of the bf16 MFMA, or f16 pairs");
  extern __shared__ __attribute__((aligned(16))) float act[];
  const FusedNet& net = args.net[blockIdx.y];
  const int M = args.M, m0 = blockIdx.x * BM;
  const int tid = threadIdx.x;
  if constexpr (SHAPE == PAIR16) {
    char* const lds = reinterpret_cast<char*>(act);
    unsigned* const mx = reinterpret_cast<unsigned*>(lds + 2 * PLANE_BYTES);   // [2][64] row maxima, alternating by layer
    {
      const int K0 = net.layer[0].K;          // K0 % 4 == 0
      p16_stage(net.x, net.ldx, m0, M, K0, (K0 + 63) / 64 * 64, lds, mx);
    }
    __syncthreads();
    for (int l = 0; l < net.n_layers; ++l) {
      const FusedLayer& L = net.layer[l];
      const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
      const bool last = l == net.n_layers - 1;
      const unsigned* mx_in = mx + (l & 1) * BM;
      unsigned* mx_out = mx + ((l + 1) & 1) * BM;
      if (L.N <= 16) p16_layer<1, true>(net, L, M, m0, lds, mx_in, mx_out, wave, last);
      else if (L.N <= 64) p16_layer<4, true>(net, L, M, m0, lds, mx_in, mx_out, wave, last);
      else if (L.N <= 80) p16_layer<5, true>(net, L, M, m0, lds, mx_in, mx_out, wave, last);
      else if (L.N <= 128) p16_layer<8, true>(net, L, M, m0, lds, mx_in, mx_out, wave, last);
      else p16_layer<8, false>(net, L, M, m0, lds, mx_in, mx_out, wave, last);
    }
    return;
  }
  {
    const int K0 = net.layer[0].K;          // K0 % 4 == 0
    const int kpad = (K0 + 63) / 64 * 64;   // whole quads of k-steps of 16 = whole pairs of k-steps of 32
    stage::rows<BM, NT>(net.x, net.ldx, m0, M, K0, kpad, act, LDA);   // all of a thread's loads in flight (stage_block.h)
  }
  __syncthreads();
  for (int l = 0; l < net.n_layers; ++l) {
    const FusedLayer& L = net.layer[l];
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool last = l == net.n_layers - 1;
    if constexpr (SHAPE == 32) {
      if (L.N <= 32) x3_layer<1, 1>(net, L, M, m0, act, LDA, wave & 1, wave >> 1, last);
      else if (L.N <= 128) x3_layer<1, 2>(net, L, M, m0, act, LDA, wave & 1, (wave >> 1) * 2, last);
      else x3_layer<2, 4>(net, L, M, m0, act, LDA, 0, wave * 4, last);
    } else {
      if (L.N <= 16) x16_layer<1, true>(net, L, M, m0, act, LDA, wave, last);
      else if (L.N <= 64) x16_layer<4, true>(net, L, M, m0, act, LDA, wave, last);
      else if (L.N <= 80) x16_layer<5, true>(net, L, M, m0, act, LDA, wave, last);
      else if (L.N <= 128) x16_layer<8, true>(net, L, M, m0, act, LDA, wave, last);
      else x16_layer<8, false>(net, L, M, m0, act, LDA, wave, last);
    }
  }
}

hipError_t launch_mlp_fused_x3(const FusedMlpArgs& args, FusedForm form, hipStream_t stream) {
  dim3 grid((args.M + fx::BM - 1) / fx::BM, args.count);
  switch (form) {
    case FusedForm::pair16: return launch_lds(mlp_fused_x3_kernel<PAIR16>, grid, dim3(fx::NT), fx::LDS_BYTES_P, stream, args);
    case FusedForm::x3_16: return launch_lds(mlp_fused_x3_kernel<16>, grid, dim3(fx::NT), fx::LDS_BYTES, stream, args);
    case FusedForm::x3_32: return launch_lds(mlp_fused_x3_kernel<32>, grid, dim3(fx::NT), fx::LDS_BYTES, stream, args);
    case FusedForm::fp32: break;   // (mlp_fused.hip's launch)
  }
  return hipErrorInvalidValue;
}

}  // namespace empose
