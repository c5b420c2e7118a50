// The weight-gradient products of the training backward pass (BASELINE.json configs[4]; reference nn/models.py:634-688
// runs it through torch.autograd).
//
//   gemm_atb     C[N][K] = A[M][N]^T . B[M][K]  -- the weight gradient of a linear layer (dW = dY^T X) and of the LSTM
//                (dW_ih = dG^T X, dW_hh = dG^T H_prev), optionally with the column sums of A (the bias gradient).
//                Both operands are read as they lie in memory (row-major activations, the reduction index m is the row):
//                for v_mfma_f32_32x32x2_f32 the A operand wants A^T[n][m] per lane (n = lane & 31, m parity = lane >> 5)
//                and the B operand B[m][k] (k = lane & 31), i.e. two coalesced 128-byte rows per half-wave straight from
//                global memory into registers -- no LDS, no transposed copy.  The output has few tiles (512 x 512 = 16
//                tiles of 128 x 128) and a long reduction (M = frames), so M is split over blockIdx.y; partial tiles go
//                to a workspace and are summed in split order by a second kernel (deterministic).
#include <algorithm>

#include "options.h"
#include "train_kernels.h"

namespace empose {

typedef float f32x16t __attribute__((ext_vector_type(16)));

namespace atb {
constexpr int NT = 256;            // 4 waves: 2 x 2 wave tiles of 64 x 64
constexpr int BN = 128, BK = 128;
}  // namespace atb

__global__ __launch_bounds__(atb::NT) void gemm_atb_kernel(AtbArgs a) {
  using namespace atb;
  const int tiles_k = (a.K + BK - 1) / BK;
  const int tn = blockIdx.x / tiles_k, tk = blockIdx.x - tn * tiles_k;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l31 = lane & 31, lh = lane >> 5;
  const int n0 = tn * BN + (wave >> 1) * 64, k0 = tk * BK + (wave & 1) * 64;
  // rows of this split: chunks of 8 rows (four k-pairs of the 32x32x2 instruction per trip)
  const int chunk = (((a.M + a.S - 1) / a.S) + 7) & ~7;
  const int ms = blockIdx.y * chunk, me = min(a.M, ms + chunk);
  f32x16t acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  const bool nv[2] = {n0 + l31 < a.N, n0 + 32 + l31 < a.N};
  const bool kv[2] = {k0 + l31 < a.K, k0 + 32 + l31 < a.K};
  const float* pa = a.A + n0 + l31;
  const float* pb = a.B + k0 + l31;
  float bsum[2] = {0.f, 0.f};
  const bool do_bias = a.bias_partial != nullptr && tk == 0 && (wave & 1) == 0;
  for (int m = ms; m < me; m += 8) {
    float fa[4][2], fb[4][2];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int mm = m + 2 * q + lh;
      const bool ok = mm < me;
      const size_t ra = (size_t)mm * a.lda, rb = (size_t)mm * a.ldb;
      fa[q][0] = ok && nv[0] ? pa[ra] : 0.f;
      fa[q][1] = ok && nv[1] ? pa[ra + 32] : 0.f;
      fb[q][0] = ok && kv[0] ? pb[rb] : 0.f;
      fb[q][1] = ok && kv[1] ? pb[rb + 32] : 0.f;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[q][i], fb[q][j], acc[i][j], 0, 0, 0);
      if (do_bias) { bsum[0] += fa[q][0]; bsum[1] += fa[q][1]; }
    }
  }
  // C/D layout of the 32x32 instruction: col = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)
  float* out = a.S > 1 ? a.partial + (size_t)blockIdx.y * a.N * a.K : a.C;
  const int ldo = a.S > 1 ? a.K : a.ldc;
  const bool acc_c = a.S == 1 && a.accumulate;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int k = k0 + j * 32 + l31;
      if (k >= a.K) continue;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int n = n0 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        if (n < a.N) out[(size_t)n * ldo + k] = acc[i][j][r] + (acc_c ? out[(size_t)n * ldo + k] : 0.f);
      }
    }
  if (do_bias) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const float v = bsum[i] + __shfl_xor(bsum[i], 32, 64);   // the two row parities
      const int n = n0 + i * 32 + l31;
      if (lh == 0 && n < a.N) {
        float* bo = a.S > 1 ? a.bias_partial + (size_t)blockIdx.y * a.N : a.bias;
        bo[n] = v + (acc_c ? bo[n] : 0.f);
      }
    }
  }
}

// The same product with the operands staged through LDS: 16-byte coalesced global loads (a quarter of the load
// instructions and of the texture-addresser time of the register version, which issues one 4-byte load per lane and
// MFMA operand), each element fetched once per workgroup and read by the waves that need it from LDS in the layout it
// has in memory -- [row m][column]: lane (column = lane & 31, m parity = lane >> 5) is exactly the 32x32x2 operand
// order, consecutive lanes hit consecutive banks.  Chunks of 32 rows, double-buffered.  Needs 16-byte aligned rows
// (lda, ldb multiples of 4, aligned bases); the register kernel takes the rest.
// MC = rows per chunk: 32 with one workgroup per CU, 16 when the reduction is split far enough for two or more (long
// reductions: the second workgroup of a CU hides what a single wave per SIMD cannot -- load latency, the LDS writes;
// measured on 32768 x 512 x 512 with scripts/dev/atb_lab.hip: 176 us at 256 workgroups x 32 rows, 138 at 512 x 16).
namespace atbl {
constexpr int NT = 256, BN = 128, BK = 128;
}  // namespace atbl

template <int MC>
__global__ __launch_bounds__(atbl::NT) void gemm_atb_lds_kernel(AtbArgs a) {
  using namespace atbl;
  constexpr int LDS_FLOATS = 2 * MC * (BN + BK);
  constexpr int P = MC / 8;   // rows a thread stages per chunk and operand
  __shared__ __attribute__((aligned(16))) float lds[LDS_FLOATS];
  const int tiles_k = (a.K + BK - 1) / BK;
  const int tn = blockIdx.x / tiles_k, tk = blockIdx.x - tn * tiles_k;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, lh = lane >> 5;
  const int nw = (wave >> 1) * 64, kw = (wave & 1) * 64;      // this wave's 64 x 64 inside the tile
  const int n_base = tn * BN, k_base = tk * BK;
  const int chunk = (((a.M + a.S - 1) / a.S) + MC - 1) / MC * MC;
  const int ms = blockIdx.y * chunk, me = min(a.M, ms + chunk);
  f32x16t acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  // staging: thread (row r8 = tid / 32, 16-byte piece c4 = tid % 32) moves rows r8 + 8 p, p < P, of both operands
  const int r8 = tid >> 5, c4 = (tid & 31) * 4;
  typedef float f4 __attribute__((ext_vector_type(4)));
  f4 ga[P], gb[P];
  // column sums of A (the bias gradient): every row passes through the staging registers exactly once, so the threads
  // add what they write to LDS (per thread: rows r8 + 8 j of four columns); the eight row groups meet in LDS at the end
  const bool do_bias = a.bias_partial != nullptr && tk == 0;   // uniform over the workgroup
  f4 bs = {0.f, 0.f, 0.f, 0.f};
  const bool tile_full = n_base + BN <= a.N && k_base + BK <= a.K;   // uniform over the workgroup
  // row segments (the applications of one network): a chunk never straddles two (seg_rows is a multiple of 32), and
  // the segment is looked up again only when the walk leaves it
  const float* A0 = a.A; const float* B0 = a.B;
  // Operand transform of the fused train-mode layer (train_kernels.h AtbArgs): a thread stages the same four columns of every
  // row, so its coefficients are registers, re-read only when the walk enters another segment (= application).
  f4 cbs = {1.f, 1.f, 1.f, 1.f}, cbt = {0.f, 0.f, 0.f, 0.f};
  const float b_slope = a.b_mode ? a.b_slope[0] : 0.f;
  const int b_cols = min(4, max(0, a.K - (k_base + c4)));
  auto load_coefs = [&](int sg) {
    if (a.b_mode && b_cols > 0) {
      const float* c = a.Bs_seg[sg] + k_base + c4;
      for (int e = 0; e < b_cols; ++e) { cbs[e] = c[e]; cbt[e] = c[a.K + e]; }
    }
  };
  if (a.n_seg == 0) load_coefs(0);
  bool rv[P];
  int mrel = 0, seg_end = a.n_seg > 0 ? 0 : 0x7fffffff;
  auto gload = [&](int m0) {
    if (m0 >= seg_end) {
      const int sg = min(m0 / a.seg_rows, a.n_seg - 1);
      A0 = a.A_seg[sg]; B0 = a.B_seg[sg]; mrel = sg * a.seg_rows;
      load_coefs(sg);
      seg_end = sg + 1 < a.n_seg ? mrel + a.seg_rows : 0x7fffffff;
    }
    if (tile_full && m0 + MC <= me) {   // interior chunk (all but the edges): straight loads, no per-lane branches
      const float* pa = A0 + (size_t)(m0 - mrel + r8) * a.lda + n_base + c4;
      const float* pb = B0 + (size_t)(m0 - mrel + r8) * a.ldb + k_base + c4;
#pragma unroll
      for (int p = 0; p < P; ++p) {
        ga[p] = *reinterpret_cast<const f4*>(pa + (size_t)(8 * p) * a.lda);
        gb[p] = *reinterpret_cast<const f4*>(pb + (size_t)(8 * p) * a.ldb);
        rv[p] = true;
      }
      return;
    }
#pragma unroll
    for (int p = 0; p < P; ++p) {
      const int mm = m0 + r8 + 8 * p;
      const bool row_ok = mm < me;
      f4 va = {0.f, 0.f, 0.f, 0.f}, vb = {0.f, 0.f, 0.f, 0.f};
      if (row_ok) {
        const float* pa = A0 + (size_t)(mm - mrel) * a.lda + n_base + c4;
        const float* pb = B0 + (size_t)(mm - mrel) * a.ldb + k_base + c4;
        if (n_base + c4 + 4 <= a.N) va = *reinterpret_cast<const f4*>(pa);
        else
          for (int e = 0; e < 4; ++e) if (n_base + c4 + e < a.N) va[e] = pa[e];
        if (k_base + c4 + 4 <= a.K) vb = *reinterpret_cast<const f4*>(pb);
        else
          for (int e = 0; e < 4; ++e) if (k_base + c4 + e < a.K) vb[e] = pb[e];
      }
      ga[p] = va; gb[p] = vb; rv[p] = row_ok;
    }
  };
  auto lwrite = [&](float* st) {
#pragma unroll
    for (int p = 0; p < P; ++p) {
      if (a.b_mode && rv[p]) {   // a_{l-1} = PReLU(s y + t)
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (e < b_cols) {
            const float y = cbs[e] * gb[p][e] + cbt[e];
            gb[p][e] = y > 0.f ? y : b_slope * y;
          }
      }
      *reinterpret_cast<f4*>(st + (r8 + 8 * p) * BN + c4) = ga[p];
      *reinterpret_cast<f4*>(st + MC * BN + (r8 + 8 * p) * BK + c4) = gb[p];
      if (do_bias) bs += ga[p];   // here, not at the load: the loads have landed by now
    }
  };
  constexpr int STAGE = MC * (BN + BK);
  gload(ms);
  lwrite(lds);
  __syncthreads();
  int buf = 0;
  for (int m = ms; m < me; m += MC) {
    const bool more = m + MC < me;
    if (more) gload(m + MC);
    const float* sA = lds + buf * STAGE + nw + l31;
    const float* sB = lds + buf * STAGE + MC * BN + kw + l31;
    // One wave per SIMD: nothing else hides the LDS latency, so the operands of row pair q + 1 are read before the
    // four MFMAs of row pair q (order pinned: left alone the compiler reads each pair right before its use).
    float a0 = sA[lh * BN], a1 = sA[lh * BN + 32];
    float b0 = sB[lh * BK], b1 = sB[lh * BK + 32];
    __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
#pragma unroll
    for (int q = 0; q < MC / 2; ++q) {
      const int row = (q + 1 < MC / 2 ? 2 * (q + 1) : 0) + lh;
      const float na0 = sA[row * BN], na1 = sA[row * BN + 32];
      const float nb0 = sB[row * BK], nb1 = sB[row * BK + 32];
      acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
      __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);   // the two ds_read2 of the next row pair
      __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);   // this row pair's MFMAs
      a0 = na0; a1 = na1; b0 = nb0; b1 = nb1;
    }
    if (more) lwrite(lds + (buf ^ 1) * STAGE);
    __syncthreads();
    buf ^= 1;
  }
  const int n0 = n_base + nw, k0 = k_base + kw;
  float* out = a.S > 1 ? a.partial + (size_t)blockIdx.y * a.N * a.K : a.C;
  const int ldo = a.S > 1 ? a.K : a.ldc;
  const bool acc_c = a.S == 1 && a.accumulate;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int k = k0 + j * 32 + l31;
      if (k >= a.K) continue;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int n = n0 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        if (n < a.N) out[(size_t)n * ldo + k] = acc[i][j][r] + (acc_c ? out[(size_t)n * ldo + k] : 0.f);
      }
    }
  if (do_bias) {   // (the loop left through a barrier: the LDS stages are free)
    *reinterpret_cast<f4*>(lds + r8 * BN + c4) = bs;
    __syncthreads();
    if (tid < BN && n_base + tid < a.N) {
      float v = 0.f;
#pragma unroll
      for (int g = 0; g < 8; ++g) v += lds[g * BN + tid];
      float* bo = a.S > 1 ? a.bias_partial + (size_t)blockIdx.y * a.N : a.bias;
      bo[n_base + tid] = v + (acc_c ? bo[n_base + tid] : 0.f);
    }
  }
}

// The interior of the same product as its own kernel (round 4): whole 128 x 128 tiles, every workgroup the same number
// of whole MC-row chunks inside ONE row segment, plain operands (no transform).  That is what the hidden layers of the
// update networks give (32768 x 512 x 512 over four applications), and for it the general kernel above carries its edge
// handling, segment walk and transform switches through the loop as branches and scalar reloads: 165 us where a stripped
// copy of the loop measured 138 (scripts/dev/atb_lab.hip).  Same staging, same operand order, same split -- the same bits.
struct AtbFastArgs {
  const float* A; const float* B; int lda, ldb;      // (segment bases are resolved per workgroup on the host side of the loop)
  const float* A_seg[ATB_MAX_SEG]; const float* B_seg[ATB_MAX_SEG];
  int n_seg, seg_rows;
  float* out; int ldo;            // partial tiles [S][N][K] (ldo = K) or C itself (S == 1)
  float* bias_out;                // [S][N] partial column sums, the bias itself (S == 1), or nullptr
  int N, K, tiles_k, chunk_rows;  // rows per workgroup (a multiple of MC)
  int acc_c;                      // S == 1 and accumulate
};

template <int MC>
__global__ __launch_bounds__(atbl::NT) void gemm_atb_fast_kernel(AtbFastArgs a) {
  using namespace atbl;
  constexpr int LDS_FLOATS = 2 * MC * (BN + BK);
  constexpr int P = MC / 8;
  __shared__ __attribute__((aligned(16))) float lds[LDS_FLOATS];
  const int tn = blockIdx.x / a.tiles_k, tk = blockIdx.x - tn * a.tiles_k;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, lh = lane >> 5;
  const int nw = (wave >> 1) * 64, kw = (wave & 1) * 64;
  const int n_base = tn * BN, k_base = tk * BK;
  const int ms = blockIdx.y * a.chunk_rows;
  typedef float f4 __attribute__((ext_vector_type(4)));
  const int r8 = tid >> 5, c4 = (tid & 31) * 4;
  // this workgroup's rows lie in one segment: two row pointers, advanced by MC rows per chunk
  const float* pa; const float* pb;
  {
    const int sg = a.n_seg > 0 ? ms / a.seg_rows : 0;
    const int mrel = a.n_seg > 0 ? ms - sg * a.seg_rows : ms;
    const float* A0 = a.n_seg > 0 ? a.A_seg[sg] : a.A;
    const float* B0 = a.n_seg > 0 ? a.B_seg[sg] : a.B;
    pa = A0 + (size_t)(mrel + r8) * a.lda + n_base + c4;
    pb = B0 + (size_t)(mrel + r8) * a.ldb + k_base + c4;
  }
  const size_t step_a = (size_t)MC * a.lda, step_b = (size_t)MC * a.ldb;
  const size_t row8_a = (size_t)8 * a.lda, row8_b = (size_t)8 * a.ldb;
  f32x16t acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  f4 ga[P], gb[P];
  const bool do_bias = a.bias_out != nullptr && tk == 0;   // uniform over the workgroup
  f4 bs = {0.f, 0.f, 0.f, 0.f};
  auto gload = [&]() {
#pragma unroll
    for (int p = 0; p < P; ++p) {
      ga[p] = *reinterpret_cast<const f4*>(pa + p * row8_a);
      gb[p] = *reinterpret_cast<const f4*>(pb + p * row8_b);
    }
    pa += step_a; pb += step_b;
  };
  auto lwrite = [&](float* st) {
#pragma unroll
    for (int p = 0; p < P; ++p) {
      *reinterpret_cast<f4*>(st + (r8 + 8 * p) * BN + c4) = ga[p];
      *reinterpret_cast<f4*>(st + MC * BN + (r8 + 8 * p) * BK + c4) = gb[p];
      if (do_bias) bs += ga[p];
    }
  };
  constexpr int STAGE = MC * (BN + BK);
  gload();
  lwrite(lds);
  __syncthreads();
  int buf = 0;
  const int n_chunks = a.chunk_rows / MC;
  for (int ch = 0; ch < n_chunks; ++ch) {
    const bool more = ch + 1 < n_chunks;
    if (more) gload();
    const float* sA = lds + buf * STAGE + nw + l31;
    const float* sB = lds + buf * STAGE + MC * BN + kw + l31;
    float a0 = sA[lh * BN], a1 = sA[lh * BN + 32];
    float b0 = sB[lh * BK], b1 = sB[lh * BK + 32];
    __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
#pragma unroll
    for (int q = 0; q < MC / 2; ++q) {
      const int row = (q + 1 < MC / 2 ? 2 * (q + 1) : 0) + lh;
      const float na0 = sA[row * BN], na1 = sA[row * BN + 32];
      const float nb0 = sB[row * BK], nb1 = sB[row * BK + 32];
      acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
      __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
      a0 = na0; a1 = na1; b0 = nb0; b1 = nb1;
    }
    if (more) lwrite(lds + (buf ^ 1) * STAGE);
    __syncthreads();
    buf ^= 1;
  }
  const int n0 = n_base + nw, k0 = k_base + kw;
  float* out = a.out + (gridDim.y > 1 ? (size_t)blockIdx.y * a.N * a.K : 0);   // the split's partial tile, or C itself
  const int ldo = a.ldo;
  const bool acc_c = a.acc_c != 0;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int k = k0 + j * 32 + l31;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int n = n0 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        out[(size_t)n * ldo + k] = acc[i][j][r] + (acc_c ? out[(size_t)n * ldo + k] : 0.f);
      }
    }
  if (do_bias) {
    *reinterpret_cast<f4*>(lds + r8 * BN + c4) = bs;
    __syncthreads();
    if (tid < BN) {
      float v = 0.f;
#pragma unroll
      for (int g = 0; g < 8; ++g) v += lds[g * BN + tid];
      float* bo = a.bias_out + (gridDim.y > 1 ? (size_t)blockIdx.y * a.N : 0);
      bo[n_base + tid] = v + (acc_c ? bo[n_base + tid] : 0.f);
    }
  }
}

// C[i] = sum_s partial[s][i] in split order; the same for the bias partials
__global__ void atb_reduce_kernel(AtbArgs a) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t nk = (size_t)a.N * a.K;
  if (i < nk) {
    float v = 0.f;
    int s = 0;
    for (; s + 8 <= a.S; s += 8) {   // eight loads in flight, added in split order
      float t[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) t[j] = a.partial[(size_t)(s + j) * nk + i];
#pragma unroll
      for (int j = 0; j < 8; ++j) v += t[j];
    }
    for (; s < a.S; ++s) v += a.partial[(size_t)s * nk + i];
    const size_t n = i / a.K, k = i - n * a.K;
    a.C[n * a.ldc + k] = v + (a.accumulate ? a.C[n * a.ldc + k] : 0.f);
  }
  if (a.bias_partial && i < (size_t)a.N) {
    float v = 0.f;
    for (int s = 0; s < a.S; ++s) v += a.bias_partial[(size_t)s * a.N + i];
    a.bias[i] = v + (a.accumulate ? a.bias[i] : 0.f);
  }
}

// Long reductions (>= 768 rows per workgroup at twice the target) split twice as far and stage 16-row chunks, so that
// two workgroups share a CU (scripts/dev/bench_atb.py: 32768 x 512 x 512 216 -> 172 us, 32768 x 512 x 296 254 -> 195,
// 16384 x 512 x 512 and below unchanged); "atb_target" / "atb_chunk" (dev options) override both.
static bool atb_long(int M, int tiles) { return (long)M * tiles >= (long)512 * 768; }

// The plan: everything launch_gemm_atb and the sizing calls decide about a product, from its shape, the operand facts
// below and the floats the workspace holds.  The only reader of the options atb_target, atb_chunk and atb_fast.
enum class AtbKernel { general, lds, fast };   // gemm_atb_kernel, gemm_atb_lds_kernel<chunk_rows>, gemm_atb_fast_kernel<chunk_rows>
struct AtbOperands {
  bool aligned = true;                      // pointers (of every segment) and leading dimensions are 16-byte multiples
  int b_mode = 0, n_seg = 0, seg_rows = 0;  // as AtbArgs
};
struct AtbPlan {
  int tiles, splits, chunk_rows;            // 128 x 128 output tiles; workgroups per tile; staged rows per chunk, 16 or 32
  AtbKernel kernel;
};
constexpr size_t ATB_UNBOUNDED = ~(size_t)0;   // workspace capacity of the sizing calls

// `workspace_floats` is what the caller carved: the split count grows as the tile count shrinks, so a workspace sized
// for ONE product shape is not automatically large enough for a smaller one.  Callers size it over every
// product they launch (atb_workspace_floats_max); should one ever come up short, the split count is reduced to what
// fits instead of writing past the buffer.
static AtbPlan atb_plan(int M, int N, int K, const AtbOperands& op, size_t workspace_floats) {
  AtbPlan p;
  p.tiles = ((N + atb::BN - 1) / atb::BN) * ((K + atb::BK - 1) / atb::BK);
  const int target = options().atb_target > 0 ? options().atb_target : (atb_long(M, p.tiles) ? 512 : 256);
  int s = (target + p.tiles - 1) / p.tiles;
  s = std::min(s, std::max(1, M / 64));
  p.splits = std::max(1, std::min(s, 256));
  if (p.splits > 1) {
    const size_t per_split = (size_t)N * K + N;
    const size_t fit = workspace_floats / per_split;
    if (fit < (size_t)p.splits) p.splits = fit >= 2 ? (int)fit : 1;
  }
  p.chunk_rows = options().atb_chunk == 16 || options().atb_chunk == 32 ? options().atb_chunk : (atb_long(M, p.tiles) ? 16 : 32);
  // the interior kernel: whole tiles, equal whole-chunk row ranges that do not straddle a segment, plain operands
  const int S = p.splits, mc = p.chunk_rows;
  const int rows_per_wg = S > 0 ? M / S : 0;
  const bool fast = options().atb_fast && op.aligned && !op.b_mode && N % atbl::BN == 0 && K % atbl::BK == 0 &&
                    M % S == 0 && rows_per_wg % mc == 0 && rows_per_wg > 0 &&
                    (op.n_seg == 0 || op.seg_rows % rows_per_wg == 0) &&
                    ((((M + S - 1) / S) + mc - 1) / mc * mc) == rows_per_wg;   // = the split the general kernel would use
  p.kernel = fast ? AtbKernel::fast : (op.aligned ? AtbKernel::lds : AtbKernel::general);
  return p;
}

int atb_splits(int M, int N, int K) { return atb_plan(M, N, K, AtbOperands{}, ATB_UNBOUNDED).splits; }

size_t atb_workspace_floats(int M, int N, int K) {
  const int s = atb_splits(M, N, K);
  return s > 1 ? (size_t)s * ((size_t)N * K + N) : 0;
}

size_t atb_workspace_floats_max(int M, std::initializer_list<std::pair<int, int>> products) {
  size_t m = 0;
  for (const auto& nk : products)
    if (nk.first > 0 && nk.second > 0) m = std::max(m, atb_workspace_floats(M, nk.first, nk.second));
  return m;
}

// Launches what atb_plan says for the product in `a` and a workspace of `workspace_floats` floats (none: nullptr).
hipError_t launch_gemm_atb(AtbArgs a, float* workspace, size_t workspace_floats, hipStream_t stream) {
  bool aligned = a.lda % 4 == 0 && a.ldb % 4 == 0;
  if (a.n_seg > 0) {
    for (int s = 0; s < a.n_seg; ++s) aligned = aligned && ((uintptr_t)a.A_seg[s] & 15) == 0 && ((uintptr_t)a.B_seg[s] & 15) == 0;
    if (!aligned || a.seg_rows % 32 != 0 || a.n_seg > ATB_MAX_SEG) return hipErrorInvalidValue;   // callers check first
  } else {
    aligned = aligned && ((uintptr_t)a.A & 15) == 0 && ((uintptr_t)a.B & 15) == 0;
  }
  if (a.b_mode && !aligned) return hipErrorInvalidValue;   // callers keep these operands aligned
  const AtbPlan plan = atb_plan(a.M, a.N, a.K, AtbOperands{aligned, a.b_mode, a.n_seg, a.seg_rows},
                                workspace ? workspace_floats : 0);
  a.S = plan.splits;
  a.partial = nullptr;
  a.bias_partial = a.bias;   // S == 1: the kernel writes the bias directly (pointer doubles as the flag)
  if (a.S > 1) {
    a.partial = workspace;
    a.bias_partial = a.bias ? workspace + (size_t)a.S * a.N * a.K : nullptr;
  }
  const dim3 grid(plan.tiles, a.S);
  const bool mc16 = plan.chunk_rows == 16;
  if (plan.kernel == AtbKernel::fast) {
    AtbFastArgs f{};
    f.A = a.A; f.B = a.B; f.lda = a.lda; f.ldb = a.ldb; f.n_seg = a.n_seg; f.seg_rows = a.seg_rows;
    for (int s = 0; s < a.n_seg; ++s) { f.A_seg[s] = a.A_seg[s]; f.B_seg[s] = a.B_seg[s]; }
    f.out = a.S > 1 ? a.partial : a.C; f.ldo = a.S > 1 ? a.K : a.ldc;
    f.bias_out = a.bias_partial; f.N = a.N; f.K = a.K; f.tiles_k = a.K / atbl::BK; f.chunk_rows = a.M / a.S;
    f.acc_c = a.S == 1 && a.accumulate;
    if (mc16) hipLaunchKernelGGL(gemm_atb_fast_kernel<16>, grid, dim3(atbl::NT), 0, stream, f);
    else hipLaunchKernelGGL(gemm_atb_fast_kernel<32>, grid, dim3(atbl::NT), 0, stream, f);
  } else if (plan.kernel == AtbKernel::lds) {
    if (mc16) hipLaunchKernelGGL(gemm_atb_lds_kernel<16>, grid, dim3(atbl::NT), 0, stream, a);
    else hipLaunchKernelGGL(gemm_atb_lds_kernel<32>, grid, dim3(atbl::NT), 0, stream, a);
  } else {
    hipLaunchKernelGGL(gemm_atb_kernel, grid, dim3(atb::NT), 0, stream, a);
  }
  if (a.S > 1) {
    const size_t n = (size_t)a.N * a.K;
    hipLaunchKernelGGL(atb_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, a);
  }
  return hipGetLastError();
}

}  // namespace empose
