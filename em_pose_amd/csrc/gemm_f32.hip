// fp32 linear layers on the CDNA4 matrix cores (v_mfma_f32_32x32x2_f32: exact fp32, 64 FLOP/clk/SIMD).
//
// Every dense contraction of the LGD path goes through this kernel: the LSTM input projections, the init heads, the
// two 6-layer update MLPs (reference nn/layers.py:46-77, eval-mode BatchNorm folded into a per-column scale/shift and
// PReLU in the epilogue), and the blend-shape / joint-regression matrix of the SMPL sub-mesh (and its transpose for
// the reverse pass).  Operands are "A[M][K] row-major" x "W[N][K] row-major" (the nn.Linear weight layout), i.e.
// both K-contiguous, so both tiles are staged through LDS with the same 16-byte loads and read back as
// ds_read_b128; since a dot product does not care about the order of k, each half-wave takes 4 consecutive k of an
// 8-wide group, which maps the b128 read straight onto four 32x32x2 MFMAs.
//
// Tile: 256 threads = 2x2 waves, each wave WM x WN tiles of 32x32 -> block tile (64*WM) x (64*WN), BK = 32.
// LDS rows are padded to 36 floats: 16 lanes of a ds_read_b128 group then hit 16 distinct 16-byte slots.
//
// Besides the tile kernels: the split-K tile for small problems (and its strided form), the matrix-vector kernel for a
// handful of rows, and the dispatch between them (pick_gemm).  The recurrent products of back-propagation through time
// are in gemm_rec.hip, the three-piece bf16 training product in gemm_train_x3.hip.
#include <cstdint>

#include "device_common.h"
#include "gemm_kernels.h"
#include "launch.h"
#include "lstm_cell_bwd.h"
#include "options.h"
#include "train_epilogue.h"
#include "train_kernels.h"

namespace empose {

// Tile configuration: WR x WC waves per block, each wave WM x WN tiles of 32x32, K tile BK, DB = LDS double buffering
// (one barrier per K tile instead of two).
template <int WR_, int WC_, int WM_, int WN_, int BK_, bool DB_>
struct Cfg {
  static constexpr int WR = WR_, WC = WC_, WM = WM_, WN = WN_, BK = BK_;
  static constexpr bool DB = DB_;
  static constexpr int NT = 64 * WR * WC;
  static constexpr int BM = 32 * WM * WR, BN = 32 * WN * WC;
  static constexpr int LDT = BK + 4;  // padded LDS row (floats): ds_read_b128 lane groups hit 16 distinct 16-byte slots
  static constexpr int C4 = BK / 4;   // float4 per tile row
  static constexpr int NA = BM * C4 / NT, NB_ = BN * C4 / NT;
  static constexpr int STAGE = (BM + BN) * LDT;
  static constexpr int LDS_FLOATS = STAGE * (DB ? 2 : 1);
  static_assert(BM * C4 % NT == 0 && BN * C4 % NT == 0, "tile rows must divide evenly over the threads");
};

template <typename C, int N>
__device__ __forceinline__ void load_tile(const float* __restrict__ base, int ld, int row0, int nrows, int k0, int K,
                                          int tid, float4 (&regs)[N]) {
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const int slot = tid + i * C::NT;
    const int r = slot / C::C4, c4 = (slot % C::C4) * 4;
    const int gr = row0 + r, gk = k0 + c4;
    if (gr < nrows && gk < K) {
      regs[i] = *reinterpret_cast<const float4*>(base + (size_t)gr * ld + gk);
    } else {
      regs[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
}

template <typename C, int N>
__device__ __forceinline__ void store_tile(float* lds, int tid, const float4 (&regs)[N]) {
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const int slot = tid + i * C::NT;
    const int r = slot / C::C4, c4 = (slot % C::C4) * 4;
    *reinterpret_cast<float4*>(lds + r * C::LDT + c4) = regs[i];
  }
}

// Train-mode fusion (ROLE 2, train_fused.hip): the staged A tile becomes PReLU(s[k] A + t[k]); padding stays zero.
// The coefficients of a K tile are fetched together with the tile (coef_tile), not between the barrier and the LDS store.
template <typename C>
__device__ __forceinline__ void coef_tile(const float* __restrict__ a_s, const float* __restrict__ a_t, int k0, int K, int tid,
                                          float4& s, float4& t) {
  const int gk = k0 + (tid % C::C4) * 4;   // NT % C4 == 0: the same k columns for every slot of a thread
  if (gk < K) { s = *reinterpret_cast<const float4*>(a_s + gk); t = *reinterpret_cast<const float4*>(a_t + gk); }
}
template <typename C, int N>
__device__ __forceinline__ void transform_tile(const float4 s, const float4 t, float slope, int row0, int nrows, int k0, int K,
                                               int tid, float4 (&regs)[N]) {
  if (k0 + (tid % C::C4) * 4 >= K) return;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const int r = (tid + i * C::NT) / C::C4;
    if (row0 + r >= nrows) continue;
    float y;
    y = s.x * regs[i].x + t.x; regs[i].x = y > 0.f ? y : slope * y;
    y = s.y * regs[i].y + t.y; regs[i].y = y > 0.f ? y : slope * y;
    y = s.z * regs[i].z + t.z; regs[i].z = y > 0.f ? y : slope * y;
    y = s.w * regs[i].w + t.w; regs[i].w = y > 0.f ? y : slope * y;
  }
}

// ROLE only separates instantiations by name so that profilers report the update-net hidden layers (ROLE 1) apart
// from the other users of the same tile configuration; ROLE 2 / 3 add the train-mode fusion (forward: optional
// A-operand transform above + the statistics epilogue of train_epilogue.h; reverse: its dyh epilogue).
template <typename C, int ROLE>
__global__ __launch_bounds__(C::NT) void gemm_tn_f32_kernel(GemmBatch batch) {
  constexpr int BM = C::BM, BN = C::BN, BK = C::BK, LDT = C::LDT, WM = C::WM, WN = C::WN;
  extern __shared__ __attribute__((aligned(16))) float lds[];

  const GemmProb& p = batch.p[blockIdx.y];
  const int tiles_n = (p.N + BN - 1) / BN;
  const int tiles_m = (p.M + BM - 1) / BM;
  const int nt = tiles_n * tiles_m;
  if ((int)blockIdx.x >= nt) return;
  // XCD-aware tile order: workgroup b runs on XCD b % 8 (each XCD has its own L2), so hand every XCD a contiguous
  // run of tiles; the tiles_n column tiles that share one A row panel then hit the same L2.  Bijective for any nt.
  int tile = blockIdx.x;
  if (batch.xcd_swizzle) {
    const int q = nt / 8, r = nt % 8, xcd = tile % 8, k = tile / 8;
    tile = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + k;
  }
  const int m0 = (tile / tiles_n) * BM;
  const int n0 = (tile % tiles_n) * BN;

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wrow = wave / C::WC, wcol = wave % C::WC;
  const int l31 = lane & 31, lh = lane >> 5;

  f32x16 acc[WM][WN];
#pragma unroll
  for (int i = 0; i < WM; ++i)
#pragma unroll
    for (int j = 0; j < WN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  float4 ra[C::NA], rb[C::NB_];
  const int nk = (p.K + BK - 1) / BK;
  const bool a_tr = ROLE == 2 && p.a_s != nullptr;
  const float a_slope = a_tr ? p.a_slope[0] : 0.f;
  float4 cs = make_float4(0.f, 0.f, 0.f, 0.f), ct = cs;
  load_tile<C>(p.A, p.lda, m0, p.M, 0, p.K, tid, ra);
  load_tile<C>(p.W, p.ldw, n0, p.N, 0, p.K, tid, rb);
  if (ROLE == 2) {
    if (a_tr) {
      coef_tile<C>(p.a_s, p.a_t, 0, p.K, tid, cs, ct);
      transform_tile<C>(cs, ct, a_slope, m0, p.M, 0, p.K, tid, ra);
    }
  }
  store_tile<C>(lds, tid, ra);
  store_tile<C>(lds + BM * LDT, tid, rb);
  __syncthreads();

  for (int kt = 0; kt < nk; ++kt) {
    const float* As = lds + (C::DB ? (kt & 1) * C::STAGE : 0);
    const float* Bs = As + BM * LDT;
    if (kt + 1 < nk) {
      load_tile<C>(p.A, p.lda, m0, p.M, (kt + 1) * BK, p.K, tid, ra);
      load_tile<C>(p.W, p.ldw, n0, p.N, (kt + 1) * BK, p.K, tid, rb);
      if (ROLE == 2) { if (a_tr) coef_tile<C>(p.a_s, p.a_t, (kt + 1) * BK, p.K, tid, cs, ct); }
    }
#pragma unroll
    for (int kk = 0; kk < BK / 8; ++kk) {
      float4 a[WM], b[WN];
#pragma unroll
      for (int i = 0; i < WM; ++i)
        a[i] = *reinterpret_cast<const float4*>(As + (wrow * 32 * WM + i * 32 + l31) * LDT + kk * 8 + lh * 4);
#pragma unroll
      for (int j = 0; j < WN; ++j)
        b[j] = *reinterpret_cast<const float4*>(Bs + (wcol * 32 * WN + j * 32 + l31) * LDT + kk * 8 + lh * 4);
#pragma unroll
      for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int j = 0; j < WN; ++j) {
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i].x, b[j].x, acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i].y, b[j].y, acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i].z, b[j].z, acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i].w, b[j].w, acc[i][j], 0, 0, 0);
        }
    }
    if (ROLE == 2) { if (a_tr && kt + 1 < nk) transform_tile<C>(cs, ct, a_slope, m0, p.M, (kt + 1) * BK, p.K, tid, ra); }
    if (C::DB) {
      // The other stage was last read in iteration kt-1, and every wave has passed that iteration's barrier.
      if (kt + 1 < nk) {
        float* nx = lds + ((kt + 1) & 1) * C::STAGE;
        store_tile<C>(nx, tid, ra);
        store_tile<C>(nx + BM * LDT, tid, rb);
      }
      __syncthreads();
    } else {
      __syncthreads();
      if (kt + 1 < nk) {
        store_tile<C>(lds, tid, ra);
        store_tile<C>(lds + BM * LDT, tid, rb);
        __syncthreads();
      }
    }
  }

  if (ROLE >= 2) {   // 2, 4: forward statistics epilogue (2: + the optional A-operand transform above); 3: reverse
    train_epilogue<WM, WN, ROLE == 3>(p, acc, m0 + wrow * 32 * WM, n0 + wcol * 32 * WN, l31, lh);
  } else {
    epilogue<WM, WN>(p, acc, m0 + wrow * 32 * WM, n0 + wcol * 32 * WN, l31, lh);
  }
}

template <typename C, int ROLE = 0>
static hipError_t launch_cfg(const GemmBatch& batch, hipStream_t stream) {
  int blocks = 0;
  for (int i = 0; i < batch.count; ++i) {
    const GemmProb& p = batch.p[i];
    const int t = ((p.M + C::BM - 1) / C::BM) * ((p.N + C::BN - 1) / C::BN);
    blocks = t > blocks ? t : blocks;
  }
  if (blocks == 0) return hipSuccess;
  constexpr size_t lds = (size_t)C::LDS_FLOATS * sizeof(float);
  return launch_lds(gemm_tn_f32_kernel<C, ROLE>, dim3(blocks, batch.count), dim3(C::NT), lds, stream, batch);
}

// ---------------------------------------------------------------------------------------------------------------
// Wide tile for the large contractions (update-net layers at T >= 32k rows): block 256 x 256, FOUR waves, each wave a
// 128 x 128 tile = 4 x 4 MFMA tiles (256 accumulator registers, one wave per SIMD).  Compared with the 8-wave
// 256 x 128 tile above this halves the LDS bytes read per flop and takes a third off the global->LDS bytes, but with a
// single wave per SIMD nothing hides a stall any more, so the K loop is software-pipelined by hand:
//   k-group 0 : MFMAs of group 0 | fragment reads of group 1 | 16 global loads of the NEXT K tile -> registers
//   k-group 1 : MFMAs of group 1 | fragment reads of group 2
//   k-group 2 : MFMAs of group 2 | fragment reads of group 3 | 16 LDS writes of the next K tile -> other LDS stage
//   barrier
//   k-group 3 : MFMAs of group 3 | fragment reads of group 0 of the next K tile
// (LDS double-buffered: 2 x 73,728 B; one barrier per K tile.)  `sched_group_barrier` pins the interleaving: one memory
// instruction every two to four MFMAs (an MFMA occupies the matrix pipe for 64 cycles = 16 issue slots).
// ---------------------------------------------------------------------------------------------------------------
namespace wide {
constexpr int BM = 256, BN = 256, BK = 32, LDT = BK + 4, NT = 256;
constexpr int STAGE = (BM + BN) * LDT;
constexpr size_t LDS_BYTES = 2 * (size_t)STAGE * sizeof(float);
}  // namespace wide

#ifdef EMPOSE_GEMM_TRACE   // dev lab only: per-phase shader-clock stamps of two blocks
__device__ long long g_gemm_trace[2][64];
#define EMPOSE_STAMP(i)                                                                              \
  if (tid == 0 && blockIdx.x == 0) {                                                                 \
    g_gemm_trace[blockIdx.y][(i)] = clock64();                                                       \
    if ((i) == 0) g_gemm_trace[blockIdx.y][62] = wall_clock64();                                     \
    else g_gemm_trace[blockIdx.y][63] = wall_clock64();                                              \
  }
#else
#define EMPOSE_STAMP(i)
#endif

template <int ROLE>
__global__ __launch_bounds__(wide::NT) void gemm_wide_f32_kernel(GemmBatch batch) {
  using namespace wide;
  extern __shared__ __attribute__((aligned(16))) float lds[];

  const GemmProb& p = batch.p[blockIdx.y];
  const int tiles_n = (p.N + BN - 1) / BN;
  const int tiles_m = (p.M + BM - 1) / BM;
  const int nt = tiles_n * tiles_m;
  if ((int)blockIdx.x >= nt) return;
  int tile = blockIdx.x;
  if (batch.xcd_swizzle) {  // contiguous run of tiles per XCD, see gemm_tn_f32_kernel
    const int q = nt / 8, r = nt % 8, xcd = tile % 8, k = tile / 8;
    tile = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + k;
  }
  const int m0 = (tile / tiles_n) * BM;
  const int n0 = (tile % tiles_n) * BN;

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wrow = wave >> 1, wcol = wave & 1;
  const int l31 = lane & 31, lh = lane >> 5;

  // Global side: thread t moves 16 bytes of row (t / 8) + 32 i, columns 4 (t % 8) .. +3 of both operands, i = 0..7.
  // Rows past the end are clamped (their products land in accumulator rows / columns that are never stored).
  const int lr = tid >> 3, lc = (tid & 7) * 4;
  const float* pa[8];
  const float* pb[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int ra = m0 + lr + 32 * i, rb = n0 + lr + 32 * i;
    pa[i] = p.A + (size_t)(ra < p.M ? ra : p.M - 1) * p.lda + lc;
    pb[i] = p.W + (size_t)(rb < p.N ? rb : p.N - 1) * p.ldw + lc;
  }
  const int wofs = lr * LDT + lc;                                  // LDS write offset (floats) of the i = 0 piece
  const int a_rd = (wrow * 128 + l31) * LDT + lh * 4;              // fragment read offsets (floats), tile i adds 32 rows
  const int b_rd = BM * LDT + (wcol * 128 + l31) * LDT + lh * 4;

  f32x16 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  f32x4 g[16];         // global -> LDS staging of one K tile (8 pieces of A, 8 of W)
  f32x4 fa[2][4], fb[2][4];  // MFMA operand fragments, double-buffered over the k-groups

  auto gload = [&](int k0) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      g[i] = *reinterpret_cast<const f32x4*>(pa[i] + k0);
      g[8 + i] = *reinterpret_cast<const f32x4*>(pb[i] + k0);
    }
  };
  auto lwrite = [&](float* st) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      *reinterpret_cast<f32x4*>(st + wofs + i * 32 * LDT) = g[i];
      *reinterpret_cast<f32x4*>(st + BM * LDT + wofs + i * 32 * LDT) = g[8 + i];
    }
  };
  auto fread = [&](const float* st, int kk, f32x4 (&a)[4], f32x4 (&b)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) a[i] = *reinterpret_cast<const f32x4*>(st + a_rd + i * 32 * LDT + kk * 8);
#pragma unroll
    for (int j = 0; j < 4; ++j) b[j] = *reinterpret_cast<const f32x4*>(st + b_rd + j * 32 * LDT + kk * 8);
  };
  // 64 MFMAs of one k-group; consecutive instructions go to different accumulators.
  auto mma = [&](const f32x4 (&a)[4], const f32x4 (&b)[4]) {
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i][e], b[j][e], acc[i][j], 0, 0, 0);
  };

  const int nk = (p.K + BK - 1) / BK;
  // A ragged last K tile: this thread's 4 columns are either all inside K or all outside (K % 4 == 0); outside, they
  // are fetched from column 0 of the row (always valid) and zeroed before they reach the LDS.
  const bool col_ok = (nk - 1) * BK + lc < p.K;
  const bool ragged = (p.K % BK) != 0;

  EMPOSE_STAMP(0)
  gload(nk == 1 && !col_ok ? -lc : 0);
  if (nk == 1 && !col_ok) {
#pragma unroll
    for (int i = 0; i < 16; ++i) g[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  lwrite(lds);
  __syncthreads();
  fread(lds, 0, fa[0], fb[0]);
  EMPOSE_STAMP(1)
  // Every iteration runs the same body (one scheduling pattern): the last one re-fetches K tile 0 into the idle stage,
  // which nobody reads afterwards.
  for (int kt = 0; kt < nk; ++kt) {
    const float* cur = lds + (kt & 1) * STAGE;
    float* nxt = lds + ((kt + 1) & 1) * STAGE;
    const bool last_fetch = kt + 2 == nk;   // this iteration fetches the (possibly ragged) last K tile
    const int k_next = kt + 1 < nk ? (kt + 1) * BK : 0;
    const bool kill = ragged && last_fetch && !col_ok;
    // ---- k-group 0
    fread(cur, 1, fa[1], fb[1]);
    gload(kill ? -lc : k_next);
    mma(fa[0], fb[0]);
#pragma unroll
    for (int s = 0; s < 8; ++s) { SGB(SG_MFMA, 2); SGB(SG_DS_RD, 1); }
#pragma unroll
    for (int s = 0; s < 16; ++s) { SGB(SG_MFMA, 2); SGB(SG_VMEM_RD, 1); }
    SGB(SG_MFMA, 16);
    // ---- k-group 1
    fread(cur, 2, fa[0], fb[0]);
    mma(fa[1], fb[1]);
#pragma unroll
    for (int s = 0; s < 8; ++s) { SGB(SG_MFMA, 4); SGB(SG_DS_RD, 1); }
    SGB(SG_MFMA, 32);
    if (ragged && last_fetch) {   // uniform branch, taken once per block at most
#pragma unroll
      for (int i = 0; i < 16; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) g[i][e] = col_ok ? g[i][e] : 0.f;
    }
    // ---- k-group 2
    fread(cur, 3, fa[1], fb[1]);
    lwrite(nxt);
    mma(fa[0], fb[0]);
#pragma unroll
    for (int s = 0; s < 8; ++s) { SGB(SG_MFMA, 2); SGB(SG_DS_RD, 1); }
#pragma unroll
    for (int s = 0; s < 16; ++s) { SGB(SG_MFMA, 2); SGB(SG_DS_WR, 1); }
    SGB(SG_MFMA, 16);
    __syncthreads();
    // ---- k-group 3
    fread(nxt, 0, fa[0], fb[0]);
    mma(fa[1], fb[1]);
#pragma unroll
    for (int s = 0; s < 8; ++s) { SGB(SG_MFMA, 4); SGB(SG_DS_RD, 1); }
    SGB(SG_MFMA, 32);
    EMPOSE_STAMP(2 + kt)
  }

  epilogue<4, 4>(p, acc, m0 + wrow * 128, n0 + wcol * 128, l31, lh);
  EMPOSE_STAMP(2 + nk)
}

template <int ROLE>
static hipError_t launch_wide(const GemmBatch& batch, hipStream_t stream) {
  int blocks = 0;
  for (int i = 0; i < batch.count; ++i) {
    const GemmProb& p = batch.p[i];
    const int t = ((p.M + wide::BM - 1) / wide::BM) * ((p.N + wide::BN - 1) / wide::BN);
    blocks = t > blocks ? t : blocks;
  }
  if (blocks == 0) return hipSuccess;
  return launch_lds(gemm_wide_f32_kernel<ROLE>, dim3(blocks, batch.count), dim3(wide::NT), wide::LDS_BYTES, stream, batch);
}

using CfgS11 = Cfg<2, 2, 1, 1, 32, false>;   //  64 x  64
using CfgS12 = Cfg<2, 2, 1, 2, 32, false>;   //  64 x 128
using CfgS21 = Cfg<2, 2, 2, 1, 32, false>;   // 128 x  64
using CfgX = Cfg<4, 2, 2, 2, 32, false>;     // 256 x 128, 8 waves

// Measured on MI355X (M = 65536, N = K = 512, before the epilogue fix): 128x128 / 4 waves 94 TF, + LDS double buffer
// 96, BK = 64 95, 256x128 / 8 waves 105, 128x256 / 8 waves 106 TFLOP/s -> the 8-wave 256x128 tile is the large tile
// of this template; the hand-pipelined 256x256 tile above takes over when whole rounds of it fill the CUs.
template <int ROLE>
static hipError_t launch_large(const GemmBatch& batch, hipStream_t stream) {
  return launch_cfg<CfgX, ROLE>(batch, stream);
}

// The largest M / N / K and the smallest K of a batch's problems: what the dispatch and the small-problem launchers size by.
struct BatchExtent { int maxM = 0, maxN = 0, minK = 1 << 30, maxK = 0; };
static BatchExtent batch_extent(const GemmBatch& batch) {
  BatchExtent x;
  for (int i = 0; i < batch.count; ++i) {
    const GemmProb& p = batch.p[i];
    x.maxM = p.M > x.maxM ? p.M : x.maxM;
    x.maxN = p.N > x.maxN ? p.N : x.maxN;
    x.minK = p.K < x.minK ? p.K : x.minK;
    x.maxK = p.K > x.maxK ? p.K : x.maxK;
  }
  return x;
}

// ---------------------------------------------------------------------------------------------------------------
// Small problems (a few hundred rows: the streaming driver's 256-frame chunks, single windows): with the tiles above a
// layer is a few dozen workgroups that each walk the whole K behind LDS staging and barriers -- 19 us for
// 256 x 512 x 512.  Here a workgroup owns ONE 32 x 32 output tile and its four waves split K: every wave fetches its
// operand fragments straight from global memory (one 16-byte piece per lane and 8 k: the k-permutation of the fused
// MLP kernel, no LDS, no barrier), the four partial tiles meet in LDS and are added in wave order, each wave finishes a
// quarter of the tile.  Four times as many workgroups, a quarter of the MFMA chain per wave.
// ---------------------------------------------------------------------------------------------------------------
template <int NW>   // waves that split K: 4, or 8 for a long K on few tiles (256 x 512 x 2048: 24.5 -> see DESIGN)
__global__ __launch_bounds__(NW * 64) void gemm_splitk_f32_kernel(GemmBatch batch) {
  __shared__ float red[NW * 16 * 64];
  const GemmProb& p = batch.p[blockIdx.y];
  const int M = p.M, N = p.N, K = p.K;
  const int nt_n = (N + 31) / 32, nt_m = (M + 31) / 32;
  if ((int)blockIdx.x >= nt_n * nt_m) return;
  const int m0 = ((int)blockIdx.x / nt_n) * 32, n0 = ((int)blockIdx.x % nt_n) * 32;
  const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, lh = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int KG = (K + 7) / 8, gq = (KG + NW - 1) / NW;
  const int g_beg = wave * gq, g_end = min(g_beg + gq, KG);
  const float* __restrict__ arow = p.A + (size_t)min(m0 + l31, M - 1) * p.lda + lh * 4;
  const float* __restrict__ wrow = p.W + (size_t)min(n0 + l31, N - 1) * p.ldw + lh * 4;

  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  constexpr int CH = 16;  // k-groups per batch of loads: a wave's whole share of K = 512 in one round trip
  for (int g0 = g_beg; g0 < g_end; g0 += CH) {
    f32x4 fa[CH], fb[CH];
#pragma unroll
    for (int u = 0; u < CH; ++u) {
      const int k = (g0 + u) * 8 + lh * 4;
      const bool ok = g0 + u < g_end && k < K;       // K % 4 == 0: a piece is entirely inside or outside
      fa[u] = ok ? *reinterpret_cast<const f32x4*>(arow + (g0 + u) * 8) : f32x4{0.f, 0.f, 0.f, 0.f};
      fb[u] = ok ? *reinterpret_cast<const f32x4*>(wrow + (g0 + u) * 8) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int u = 0; u < CH; ++u)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[u][e], fb[u][e], acc, 0, 0, 0);
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) red[(wave * 16 + r) * 64 + lane] = acc[r];
  __syncthreads();

  const int n = n0 + l31;
  if (n >= N) return;
  const float sc = p.scale ? p.scale[n] : 1.f, sh = p.shift ? p.shift[n] : 0.f;
  const float slope = p.act == 1 ? p.slope : 1.f;
#pragma unroll
  for (int i = 0; i < 16 / NW; ++i) {
    const int r = wave * (16 / NW) + i;
    const int row = m0 + (r & 3) + 8 * (r >> 2) + 4 * lh;   // C/D layout of the 32x32 MFMA
    if (row >= M) continue;
    float v = red[(0 * 16 + r) * 64 + lane];
#pragma unroll
    for (int w2 = 1; w2 < NW; ++w2) v += red[(w2 * 16 + r) * 64 + lane];
    p.C[(size_t)row * p.ldc + n] = epilogue_elem(p, row, n, v, sc, sh, slope);
  }
}

static hipError_t launch_splitk(const GemmBatch& batch, hipStream_t stream) {
  int blocks = 0;
  for (int i = 0; i < batch.count; ++i) {
    const int t = ((batch.p[i].M + 31) / 32) * ((batch.p[i].N + 31) / 32);
    blocks = t > blocks ? t : blocks;
  }
  if (blocks == 0) return hipSuccess;
  // a long K on few tiles (the recurrent products of back-propagation through time at a few hundred rows): eight waves
  if (batch_extent(batch).minK >= 1024 && (long)blocks * batch.count <= 256)
    hipLaunchKernelGGL(gemm_splitk_f32_kernel<8>, dim3(blocks, batch.count), dim3(512), 0, stream, batch);
  else
    hipLaunchKernelGGL(gemm_splitk_f32_kernel<4>, dim3(blocks, batch.count), dim3(256), 0, stream, batch);
  return hipGetLastError();
}

constexpr long SPLITK_MAX_TILES = 512;   // 256 x 512 x 512: 8 us against 15; 2048 rows (1024 tiles): 25 against 15

// The same split-K tile for operands of any layout: element (row, k) of an operand lives at base[row * rs + k * ks].
// ks == 1 is the K-contiguous case above (16-byte pieces); otherwise a lane gathers its four k with the row index
// running across lanes, so the loads of a wave are still contiguous (ks is then the leading dimension of a transposed
// matrix).  This is what the backward pass of a small linear layer needs: dX = dY . W (W transposed) and
// dW = dY^T . X (both transposed) without materialising a transpose.
template <bool A_KC, bool W_KC>
__global__ __launch_bounds__(256) void gemm_strided_splitk_kernel(StridedGemm p) {
  __shared__ float red[4 * 16 * 64];
  const int M = p.M, N = p.N, K = p.K;
  const int nt_n = (N + 31) / 32;
  const int m0 = ((int)blockIdx.x / nt_n) * 32, n0 = ((int)blockIdx.x % nt_n) * 32;
  const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, lh = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int KG = (K + 7) / 8, gq = (KG + 3) / 4;
  const int g_beg = wave * gq, g_end = min(g_beg + gq, KG);
  const float* __restrict__ arow = p.A + (size_t)min(m0 + l31, M - 1) * p.a_rs;
  const float* __restrict__ wrow = p.W + (size_t)min(n0 + l31, N - 1) * p.w_rs;
  auto fetch = [&](const float* row, long ks, bool kc, int k) {
    f32x4 v{0.f, 0.f, 0.f, 0.f};
    if (kc) {
      if (k + 3 < K) return *reinterpret_cast<const f32x4*>(row + k);
#pragma unroll
      for (int e = 0; e < 4; ++e) if (k + e < K) v[e] = row[k + e];
      return v;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) if (k + e < K) v[e] = row[(size_t)(k + e) * ks];
    return v;
  };
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  constexpr int CH = 16;  // as above: the loads of a wave's share of K are all in flight together
  for (int g0 = g_beg; g0 < g_end; g0 += CH) {
    f32x4 fa[CH], fb[CH];
#pragma unroll
    for (int u = 0; u < CH; ++u) {
      const int k = (g0 + u) * 8 + lh * 4;
      const bool ok = g0 + u < g_end;
      fa[u] = ok ? fetch(arow, p.a_ks, A_KC, k) : f32x4{0.f, 0.f, 0.f, 0.f};
      fb[u] = ok ? fetch(wrow, p.w_ks, W_KC, k) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int u = 0; u < CH; ++u)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[u][e], fb[u][e], acc, 0, 0, 0);
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) red[(wave * 16 + r) * 64 + lane] = acc[r];
  __syncthreads();
  const int n = n0 + l31;
  if (n >= N) return;
  const float b = p.bias ? p.bias[n] : 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = wave * 4 + i;
    const int row = m0 + (r & 3) + 8 * (r >> 2) + 4 * lh;
    if (row >= M) continue;
    float v = red[(0 * 16 + r) * 64 + lane];
#pragma unroll
    for (int w2 = 1; w2 < 4; ++w2) v += red[(w2 * 16 + r) * 64 + lane];
    p.C[(size_t)row * p.ldc + n] = v + b;
  }
}

bool strided_gemm_applicable(int M, int N) {
  return (long)((M + 31) / 32) * ((N + 31) / 32) <= SPLITK_MAX_TILES;
}

hipError_t launch_strided_gemm(const StridedGemm& p, hipStream_t stream) {
  const int blocks = ((p.M + 31) / 32) * ((p.N + 31) / 32);
  // K-contiguous pieces need 16-byte aligned rows; anything else takes the gathering path
  auto kc = [](const float* base, long rs, long ks) { return ks == 1 && rs % 4 == 0 && ((uintptr_t)base & 15) == 0; };
  const bool a_kc = kc(p.A, p.a_rs, p.a_ks), w_kc = kc(p.W, p.w_rs, p.w_ks);
  if (a_kc && w_kc) hipLaunchKernelGGL((gemm_strided_splitk_kernel<true, true>), dim3(blocks), dim3(256), 0, stream, p);
  else if (a_kc) hipLaunchKernelGGL((gemm_strided_splitk_kernel<true, false>), dim3(blocks), dim3(256), 0, stream, p);
  else if (w_kc) hipLaunchKernelGGL((gemm_strided_splitk_kernel<false, true>), dim3(blocks), dim3(256), 0, stream, p);
  else hipLaunchKernelGGL((gemm_strided_splitk_kernel<false, false>), dim3(blocks), dim3(256), 0, stream, p);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------
// A handful of rows against a long K (back-propagation through time at the reference's training batch: dh = dG . W_hh
// is 12 x 2048 . 2048 x 512, sixty-four times per step): a matrix-vector problem bound by streaming W once.  The 32 x 32
// split-K tile leaves it on 16 workgroups that each walk 256 KB (19.9 us per call); here a wave owns ONE output column,
// its lanes split K in 16-byte pieces (coalesced 1 KB reads of the weight row, all in flight at once), the rows of A
// are staged in LDS once per workgroup, and the lane sums meet in a butterfly -- a fixed order: reproducible results.
// ---------------------------------------------------------------------------------------------------------------
constexpr size_t FEWROWS_MAX_LDS = 128 * 1024;   // the rows of A (M x K floats) are staged in LDS once per workgroup
template <int MB>   // rows computed (M rounded up to a multiple of 4; rows past M are staged as zeros, never stored)
__global__ __launch_bounds__(256) void gemm_fewrows_kernel(GemmBatch b, LstmCellBwdArgs cell, int with_cell) {
  extern __shared__ __attribute__((aligned(16))) float arow[];   // [MB][K]
  const GemmProb& p = b.p[blockIdx.y];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int n = blockIdx.x * 4 + wave;
  const int M = p.M, N = p.N, K = p.K;
  const int k4n = K >> 2;
  // this wave's weight row first: its 16-byte pieces are in flight while the rows of A are staged
  constexpr int WMAX = 8;   // K <= 64 lanes x 4 x 8 = 2048 per pass
  const float* __restrict__ wrow = p.W + (size_t)(n < N ? n : N - 1) * p.ldw;
  f32x4 w[WMAX];
#pragma unroll
  for (int j = 0; j < WMAX; ++j) {
    const int k4 = j * 256 + lane * 4;
    w[j] = k4 < K ? *reinterpret_cast<const f32x4*>(wrow + k4) : f32x4{0.f, 0.f, 0.f, 0.f};
  }
  {
    // (row, piece) of this thread's pieces tid, tid + 256, ... without a division per piece: k4n >= 256 (K >= 1024),
    // so a step of 256 pieces wraps to the next row at most once.  Rows M .. MB-1 are zeros.
    const float* __restrict__ A = p.A;
    constexpr int SB = 8;   // 16-byte pieces per thread in flight
    int m = (int)threadIdx.x / k4n, c = (int)threadIdx.x - m * k4n;
    for (int i0 = threadIdx.x; i0 < MB * k4n; i0 += 256 * SB) {
      f32x4 v[SB];
      int mu[SB], cu[SB];
#pragma unroll
      for (int u = 0; u < SB; ++u) {
        mu[u] = m; cu[u] = c;
        const int mr = m < M ? m : M - 1;   // (clamped address, value discarded below)
        v[u] = *reinterpret_cast<const f32x4*>(A + (size_t)mr * p.lda + (c < k4n ? c : 0) * 4);
        if (m >= M) v[u] = f32x4{0.f, 0.f, 0.f, 0.f};
        c += 256;
        if (c >= k4n) { c -= k4n; ++m; }
      }
#pragma unroll
      for (int u = 0; u < SB; ++u)
        if (mu[u] < MB) *reinterpret_cast<f32x4*>(arow + (size_t)mu[u] * K + cu[u] * 4) = v[u];
    }
  }
  __syncthreads();
  float acc[MB];
#pragma unroll
  for (int m = 0; m < MB; ++m) acc[m] = 0.f;
  for (int kb = 0; kb < K; kb += 256 * WMAX) {
    if (kb > 0) {
#pragma unroll
      for (int j = 0; j < WMAX; ++j) {
        const int k4 = kb + j * 256 + lane * 4;
        w[j] = k4 < K ? *reinterpret_cast<const f32x4*>(wrow + k4) : f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }
    // branch-free inner loops: pieces past K multiply zero weights (w) with whatever row 0.. holds at piece 0
#pragma unroll
    for (int j = 0; j < WMAX; ++j) {
      const int k4 = kb + j * 256 + lane * 4;
      const int kk = k4 < K ? k4 : 0;
#pragma unroll
      for (int m = 0; m < MB; ++m) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(arow + (size_t)m * K + kk);
        acc[m] = __builtin_fmaf(a[3], w[j][3], __builtin_fmaf(a[2], w[j][2], __builtin_fmaf(a[1], w[j][1], __builtin_fmaf(a[0], w[j][0], acc[m]))));
      }
    }
  }
  if (n >= N) return;
  float out = 0.f;   // lane m ends up with row m
#pragma unroll
  for (int m = 0; m < MB; ++m) {
    float v = acc[m];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    if (lane == m) out = v;
  }
  if (lane < M) {
    const float y = epilogue_elem(p, lane, n, out);
    // back-propagation through time: y is dh of (row, unit n) for the step below; run that step's cell right here
    if (with_cell) lstm_cell_bwd_elem(cell, lane * cell.H + n, y);
    else p.C[(size_t)lane * p.ldc + n] = y;
  }
}

template <int MB>
static hipError_t launch_fewrows_cfg(const GemmBatch& batch, int maxN, int maxK, hipStream_t stream,
                                     const LstmCellBwdArgs* cell = nullptr) {
  const size_t lds = (size_t)MB * maxK * sizeof(float);   // arow[MB][K of the widest problem]
  if (lds > FEWROWS_MAX_LDS) return hipErrorInvalidValue;
  dim3 grid((maxN + 3) / 4, batch.count);
  return launch_lds(gemm_fewrows_kernel<MB>, grid, dim3(256), lds, stream, batch, cell ? *cell : LstmCellBwdArgs{},
                    cell ? 1 : 0);
}

static hipError_t launch_fewrows(const GemmBatch& batch, hipStream_t stream, const LstmCellBwdArgs* cell = nullptr) {
  const BatchExtent x = batch_extent(batch);
  if (x.maxM <= 4) return launch_fewrows_cfg<4>(batch, x.maxN, x.maxK, stream, cell);
  if (x.maxM <= 8) return launch_fewrows_cfg<8>(batch, x.maxN, x.maxK, stream, cell);
  if (x.maxM <= 12) return launch_fewrows_cfg<12>(batch, x.maxN, x.maxK, stream, cell);
  return launch_fewrows_cfg<16>(batch, x.maxN, x.maxK, stream, cell);
}

// The matrix-vector shape: at most FEWROWS_MAX_M rows, every K long enough to split over a wave's lanes, and the rows of A
// (rounded up to a multiple of 4) of the longest K within the kernel's LDS.
static bool fewrows_shape(const BatchExtent& x) {
  return options().gemm_splitk != 0 && x.maxM <= FEWROWS_MAX_M && x.minK >= 1024 && x.maxN >= 64 &&
         (size_t)((x.maxM + 3) & ~3) * x.maxK * sizeof(float) <= FEWROWS_MAX_LDS;
}

// The matrix-vector kernel with the LSTM cell of the step below as its epilogue (back-propagation through time at the
// reference's training batch); false when the shape is not this kernel's.
bool gemm_fewrows_applicable(int M, int N, int K) {
  BatchExtent x;
  x.maxM = M; x.maxN = N; x.minK = x.maxK = K;
  return K % 4 == 0 && fewrows_shape(x);
}
hipError_t launch_gemm_fewrows_cell(const GemmProb& p, const LstmCellBwdArgs& cell, hipStream_t stream) {
  GemmBatch b;
  b.count = 1; b.p[0] = p;
  return launch_fewrows(b, stream, &cell);
}

enum GemmPick { PICK_S11, PICK_S12, PICK_S21, PICK_WIDE, PICK_LARGE, PICK_SPLITK, PICK_FEWROWS };

static GemmPick pick_gemm(const GemmBatch& batch) {
  const BatchExtent x = batch_extent(batch);
  // Narrow outputs (heads: 66 / 10 columns) and short batches take the smaller tiles; everything else the large ones,
  // unless that would leave most of the 256 CUs without a block.
  const bool narrow = x.maxN <= 64;
  const bool shortm = x.maxM <= 64;
  auto nblocks = [&](int bm, int bn) {
    long t = 0;
    for (int i = 0; i < batch.count; ++i)
      t += (long)((batch.p[i].M + bm - 1) / bm) * ((batch.p[i].N + bn - 1) / bn);
    return t;
  };
  if (fewrows_shape(x)) return PICK_FEWROWS;
  // few 32 x 32 tiles in total and a K worth splitting: one tile per workgroup, K over its four waves
  if (options().gemm_splitk != 0 && x.minK >= 64 && nblocks(32, 32) <= SPLITK_MAX_TILES) return PICK_SPLITK;
  if (shortm && narrow) return PICK_S11;
  if (shortm) return PICK_S12;
  if (narrow) return PICK_S21;
  // The 256 x 256 four-wave tile runs one block per CU, so it only pays when the tiles fill whole rounds of the 256
  // CUs and the 256-wide column tiles are not mostly padding (measured: 125 vs 114 TFLOP/s at M=2x32768, N=K=512;
  // 105 vs 96 at K=296; but 48 vs 76 at N=200).
  bool wide_ok = options().gemm_wide != 0;
  for (int i = 0; i < batch.count; ++i) wide_ok = wide_ok && batch.p[i].N % wide::BN == 0 && batch.p[i].K >= 2 * wide::BK;
  if (wide_ok) {
    const long t = nblocks(wide::BM, wide::BN);
    const long rounds = (t + 255) / 256;
    if (t >= 256 && t * 10 >= rounds * 256 * 8) return PICK_WIDE;
  }
  if (nblocks(128, 128) >= 512) return PICK_LARGE;
  if (nblocks(64, 128) >= 256) return PICK_S12;
  return PICK_S11;
}

// The train-mode fused layer GEMM (train_fused.hip) on the training step's 64 x 128 tile.
hipError_t launch_gemm_train(const TrainGemmArgs& t, int amode, int emode, hipStream_t stream) {
  if (amode > 1 || emode > 2) return hipErrorInvalidValue;
  GemmBatch b;
  b.count = 1; b.xcd_swizzle = 1; b.role = 2;
  GemmProb& g = b.p[0];
  g.A = t.A; g.lda = t.lda; g.W = t.W; g.ldw = t.ldw; g.C = t.C; g.ldc = t.ldc; g.M = t.M; g.N = t.N; g.K = t.K;
  g.scale = nullptr; g.shift = t.bias; g.resid = nullptr; g.ldr = 0; g.act = 0; g.slope = 0.f;
  if (amode == 1) { g.a_s = t.a_s; g.a_t = t.a_t; g.a_slope = t.a_slope; }
  if (emode >= 1) g.stat_part = t.part;
  if (emode == 2) {
    g.e_y = t.e_y; g.ld_ey = t.ld_ey; g.e_s = t.e_s; g.e_t = t.e_t; g.e_mean = t.e_mean; g.e_rstd = t.e_rstd;
    g.e_slope = t.e_slope;
  }
  if (emode == 2) return launch_cfg<CfgS12, 3>(b, stream);
  // without the operand transform: an instantiation that does not carry its code in the K loop (ROLE 2 ran 8 us slower
  // per 8192 x 512 x 512 launch than the plain tile even with the transform switched off at run time)
  if (amode == 0) return emode == 1 ? launch_cfg<CfgS12, 4>(b, stream) : launch_cfg<CfgS12, 0>(b, stream);
  return launch_cfg<CfgS12, 2>(b, stream);
}

// Name (as a profiler prints it) of the kernel `launch_gemm` runs for `count` problems of this shape.
const char* gemm_kernel_name(int M, int N, int K, int count, int role) {
  GemmBatch b;
  b.count = count; b.role = role;
  for (int i = 0; i < count && i < 2; ++i) { b.p[i] = GemmProb{}; b.p[i].M = M; b.p[i].N = N; b.p[i].K = K; }
  switch (pick_gemm(b)) {
    case PICK_SPLITK: return "gemm_splitk_f32_kernel";
    case PICK_FEWROWS: return "gemm_fewrows_kernel";
    case PICK_S11: return "gemm_tn_f32_kernel<Cfg<2,2,1,1,32,false>,0>";
    case PICK_S12: return "gemm_tn_f32_kernel<Cfg<2,2,1,2,32,false>,0>";
    case PICK_S21: return "gemm_tn_f32_kernel<Cfg<2,2,2,1,32,false>,0>";
    case PICK_WIDE: return role == 1 ? "gemm_wide_f32_kernel<1>" : "gemm_wide_f32_kernel<0>";
    default: return role == 1 ? "gemm_tn_f32_kernel<Cfg<4,2,2,2,32,false>,1>" : "gemm_tn_f32_kernel<Cfg<4,2,2,2,32,false>,0>";
  }
}

hipError_t launch_gemm(const GemmBatch& batch_in, hipStream_t stream) {
  GemmBatch batch = batch_in;
  batch.xcd_swizzle = 1;
  switch (pick_gemm(batch)) {
    case PICK_SPLITK: return launch_splitk(batch, stream);
    case PICK_FEWROWS: return launch_fewrows(batch, stream);
    case PICK_S11: return launch_cfg<CfgS11>(batch, stream);
    case PICK_S12: return launch_cfg<CfgS12>(batch, stream);
    case PICK_S21: return launch_cfg<CfgS21>(batch, stream);
    case PICK_WIDE: return batch.role == 1 ? launch_wide<1>(batch, stream) : launch_wide<0>(batch, stream);
    default: return batch.role == 1 ? launch_large<1>(batch, stream) : launch_large<0>(batch, stream);
  }
}

}  // namespace empose
