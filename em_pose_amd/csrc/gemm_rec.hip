// The recurrent products of back-propagation through time (BPTT) of the training LSTM: dh_{t-1} = dG_t . W_hh (+ the
// carry), formed and fed straight into the cell of the step below (lstm_cell_bwd.h) instead of being stored.  fp32 on the
// v_mfma_f32_32x32x2_f32 instruction or plain FMAs; every sum in a fixed order, so results are reproducible.
//
// Two kernels by row count, both on a RecBatch (gemm_kernels.h): up to two problems per launch, each a sum over up to two K
// segments with their own operands, each followed by its own cell.  The wavefront form of the reverse pass launches two
// problems per step; the layer-after-layer form launches the K-split pair with one problem of one segment (and takes
// gemm_fewrows_kernel of gemm_f32.hip for a handful of rows).
#include <cstdint>

#include "gemm_epilogue.h"
#include "gemm_kernels.h"
#include "launch.h"
#include "lstm_cell_bwd.h"
#include "lane_reduce.h"
#include "train_kernels.h"

namespace empose {

// ---------------------------------------------------------------------------------------------------------------
// A few hundred rows against a long K with a small output (back-propagation through time at 256 windows: dh = dG . W_hh
// is 256 x 2048 . 2048 x 512, sixty-two times per step): 32 x 32 tiles that each walk the whole K leave it at 22 us per
// call (128 workgroups, strided 16-byte operand reads).  Here K is split over the workgroups: a workgroup owns a
// 64 x 64 output tile for a K slice of 256, stages both operand slices in LDS with coalesced row reads in one round
// trip, runs 128 MFMAs per wave (four waves, a 32 x 32 quadrant each) without a barrier, and writes its partial tile;
// a small second kernel adds the partial tiles in slice order (fixed order: reproducible), adds the residual and runs the
// cell.  32 tiles x 8 slices = 256 workgroups.  A problem's slices are those of its segment 0, then those of segment 1; a
// segment's last slice may be partial (K % 4 == 0).
// ---------------------------------------------------------------------------------------------------------------
namespace ks {
constexpr int BT = 64, KS = 256, LDK = KS + 4;   // tile, K slice per workgroup, LDS row stride (floats)
constexpr size_t LDS_BYTES = (size_t)2 * BT * LDK * sizeof(float);
}
__global__ __launch_bounds__(256) void rec_ksplit_kernel(RecBatch b, float* partial, int tiles, int s_max) {
  using namespace ks;
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float* sA = sm;
  float* sW = sm + BT * LDK;
  const RecProb& p = b.p[blockIdx.z];
  const int M = p.M, N = p.N;
  const int nt_n = (N + BT - 1) / BT;
  const int tile = blockIdx.x, m0 = (tile / nt_n) * BT, n0 = (tile % nt_n) * BT;
  // slice -> (segment, k0): the slices of segment 0 first
  const int s0 = (p.seg[0].K + KS - 1) / KS;
  const int s_tot = s0 + (p.nseg > 1 ? (p.seg[1].K + KS - 1) / KS : 0);
  if ((int)blockIdx.y >= s_tot) return;
  const bool second = (int)blockIdx.y >= s0;
  const RecSeg& sg = p.seg[second ? 1 : 0];
  const int k0 = ((int)blockIdx.y - (second ? s0 : 0)) * KS, K = sg.K;
  const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, lh = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // staging: 64 rows x 256 floats of each operand = 2 x 4096 16-byte pieces over 256 threads, all in flight at once
  {
    f32x4 va[16], vw[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int i = tid + u * 256, r = i >> 6, c = (i & 63) * 4;
      const bool kin = k0 + c < K;   // K % 4 == 0
      va[u] = kin ? *reinterpret_cast<const f32x4*>(sg.A + (size_t)min(m0 + r, M - 1) * sg.lda + k0 + c) : f32x4{0.f, 0.f, 0.f, 0.f};
      vw[u] = kin ? *reinterpret_cast<const f32x4*>(sg.W + (size_t)min(n0 + r, N - 1) * sg.ldw + k0 + c) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int i = tid + u * 256, r = i >> 6, c = (i & 63) * 4;
      *reinterpret_cast<f32x4*>(sA + r * LDK + c) = va[u];
      *reinterpret_cast<f32x4*>(sW + r * LDK + c) = vw[u];
    }
  }
  __syncthreads();
  const int mq = (wave >> 1) * 32, nq = (wave & 1) * 32;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  const float* ar = sA + (mq + l31) * LDK + lh * 4;
  const float* wr = sW + (nq + l31) * LDK + lh * 4;
#pragma unroll 8
  for (int g = 0; g < KS / 8; ++g) {   // k-groups of 8: lane half lh holds k = 8 g + 4 lh .. + 3 of both operands
    const f32x4 fa = *reinterpret_cast<const f32x4*>(ar + g * 8);
    const f32x4 fb = *reinterpret_cast<const f32x4*>(wr + g * 8);
#pragma unroll
    for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[e], fb[e], acc, 0, 0, 0);
  }
  // partial tile of this slice: [problem][slice][tile][wave][reg][lane]; a second kernel adds the slices in order (a
  // last-arriver reduction inside this kernel was measured: the agent-scope fences it needs write back and invalidate the
  // whole L2 of every workgroup's XCD -- 60 us per call instead of 22)
  float* pt = partial + ((((size_t)blockIdx.z * s_max + blockIdx.y) * tiles + tile) * 4 + wave) * 1024;
#pragma unroll
  for (int r = 0; r < 16; ++r) pt[r * 64 + lane] = acc[r];
}

// dh = sum over the K slices, in slice order (+ resid), then the cell: one thread per output element, its S partial values
// requested together (one round trip) and added in slice order
constexpr int KSPLIT_MAX_S = 16;
__global__ __launch_bounds__(256) void rec_ksplit_reduce_kernel(RecBatch b, const float* partial, int tiles, int s_max,
                                                                LstmCellBwdArgs cell0, LstmCellBwdArgs cell1) {
  using namespace ks;
  const RecProb& p = b.p[blockIdx.y];
  const LstmCellBwdArgs& cell = blockIdx.y == 0 ? cell0 : cell1;
  const int M = p.M, N = p.N;
  const int nt_n = (N + BT - 1) / BT;
  const int S = (p.seg[0].K + KS - 1) / KS + (p.nseg > 1 ? (p.seg[1].K + KS - 1) / KS : 0);
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)tiles * 4096) return;
  const float* base = partial + (size_t)blockIdx.y * s_max * tiles * 4096 + idx;
  float ps[KSPLIT_MAX_S];
#pragma unroll
  for (int s2 = 0; s2 < KSPLIT_MAX_S; ++s2) ps[s2] = s2 < S ? base[(size_t)s2 * tiles * 4096] : 0.f;
  float v = 0.f;
#pragma unroll
  for (int s2 = 0; s2 < KSPLIT_MAX_S; ++s2) v += ps[s2];   // (slices past S add 0: the same bits as stopping at S)
  const int tile = (int)(idx >> 12), wave = (int)(idx >> 10) & 3, r = (int)(idx >> 6) & 15, lane = (int)idx & 63;
  const int m0 = (tile / nt_n) * BT, n0 = (tile % nt_n) * BT;
  const int mq = (wave >> 1) * 32, nq = (wave & 1) * 32, l31 = lane & 31, lh = lane >> 5;
  const int row = m0 + mq + (r & 3) + 8 * (r >> 2) + 4 * lh, n = n0 + nq + l31;
  if (row >= M || n >= N) return;
  float y = v;   // (the bits of v * 1 + 0, a scale / shift epilogue without either: v starts from 0.f and is never -0)
  if (p.resid) y += p.resid[(size_t)row * p.ldr + n];
  lstm_cell_bwd_elem(cell, row * cell.H + n, y);
}

// One segment of K (the layer-after-layer form decides by it; a wavefront step's second segment doubles the slices).
bool rec_ksplit_applicable(int M, int N, int K) {
  const long tiles = (long)((M + ks::BT - 1) / ks::BT) * ((N + ks::BT - 1) / ks::BT);
  const int S = (K + ks::KS - 1) / ks::KS;
  return K % 4 == 0 && M > FEWROWS_MAX_M && S >= 4 && S <= KSPLIT_MAX_S && tiles * S >= 32 && tiles * S <= 1024;
}
size_t rec_ksplit_workspace_floats(int M, int N, int K_total_max, int count) {
  const size_t tiles = (size_t)((M + ks::BT - 1) / ks::BT) * ((N + ks::BT - 1) / ks::BT);
  const size_t S = (K_total_max + ks::KS - 1) / ks::KS;
  return (size_t)count * tiles * S * 4096 + 64;
}

hipError_t launch_rec_ksplit(const RecBatch& b, const LstmCellBwdArgs* cells, float* workspace, hipStream_t stream) {
  int tiles = 0, s_max = 0;
  for (int i = 0; i < b.count; ++i) {
    const RecProb& p = b.p[i];
    int s = 0;
    for (int g = 0; g < p.nseg; ++g) {
      if (p.seg[g].K % 4 != 0) return hipErrorInvalidValue;
      s += (p.seg[g].K + ks::KS - 1) / ks::KS;   // (the kernels mask a partial last slice)
    }
    if (s > KSPLIT_MAX_S || p.nseg < 1 || p.nseg > 2) return hipErrorInvalidValue;
    s_max = s > s_max ? s : s_max;
    const int t = ((p.M + ks::BT - 1) / ks::BT) * ((p.N + ks::BT - 1) / ks::BT);
    if (i > 0 && t != tiles) return hipErrorInvalidValue;   // the problems of a wavefront step share M and N
    tiles = t;
  }
  if (hipError_t e = launch_lds(rec_ksplit_kernel, dim3(tiles, s_max, b.count), dim3(256), ks::LDS_BYTES, stream, b, workspace,
                                tiles, s_max))
    return e;
  hipLaunchKernelGGL(rec_ksplit_reduce_kernel, dim3(tiles * 16, b.count), dim3(256), 0, stream, b, (const float*)workspace,
                     tiles, s_max, cells[0], cells[b.count > 1 ? 1 : 0]);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------
// At most FEWROWS_MAX_M rows (the reference's training batch: 12 windows): a matrix-vector problem, with the K range split
// over the four waves and BOTH operands in registers.  (The form that staged the M rows of A in LDS, as gemm_fewrows_kernel
// does -- 98 KB per segment at 12 rows x 2048, every wave re-reading all of them for its one column -- left a 12-window
// BPTT step waiting for that staging and on LDS reads, 4 per 16 multiply-adds; it is gone, docs/history.md.)  Here
// wave w owns the quarter [w K / 4, (w + 1) K / 4) of every segment for all four columns of the workgroup: a lane loads
// its 16-byte pieces of the M rows and of the 4 weight rows once (all loads of a segment in flight together), 4 M
// accumulators per lane; the sums over the 64 lanes are a reduce-scatter (each step halves what a lane carries: 51 lane
// exchanges for 48 sums instead of 288), the four waves' sums meet in LDS and are added in wave order.  Needs K % 16 == 0.
// ---------------------------------------------------------------------------------------------------------------
template <int MB>
__global__ __launch_bounds__(256) void rec_fewrows_reg_kernel(RecBatch b, LstmCellBwdArgs cell0, LstmCellBwdArgs cell1) {
  __shared__ float wsum[4][4 * MB + 4];
  const RecProb& p = b.p[blockIdx.y];
  const LstmCellBwdArgs& cell = blockIdx.y == 0 ? cell0 : cell1;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n0 = blockIdx.x * 4;
  const int M = p.M, N = p.N;
  // thread (column c, row m) finishes element (m, n0 + c): what the cell's reverse reads besides dh is fetched now
  const int f_c = tid / MB, f_m = tid - f_c * MB;
  const bool fin = tid < 4 * MB && f_m < M && n0 + f_c < N;
  LstmCellBwdPre pre{};
  float res = 0.f;
  if (fin) {
    pre = lstm_cell_bwd_load(cell, f_m * cell.H + n0 + f_c);
    if (p.resid) res = p.resid[(size_t)f_m * p.ldr + n0 + f_c];
  }
  float v[64];
#pragma unroll
  for (int i = 0; i < 4 * MB; ++i) v[i] = 0.f;
  for (int g = 0; g < p.nseg; ++g) {
    const RecSeg& sg = p.seg[g];
    const int Kq = sg.K >> 2;                      // this wave's quarter: Kq <= 512 floats, a multiple of 4
    const int kbase = wave * Kq;
    f32x4 a[MB][2], w[4][2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int kl = j * 256 + lane * 4;
      const bool in = kl < Kq;
      const int k = kbase + (in ? kl : 0);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const f32x4 x = *reinterpret_cast<const f32x4*>(sg.W + (size_t)min(n0 + c, N - 1) * sg.ldw + k);
        w[c][j] = in ? x : f32x4{0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (int m = 0; m < MB; ++m) {
        const f32x4 x = *reinterpret_cast<const f32x4*>(sg.A + (size_t)min(m, M - 1) * sg.lda + k);
        a[m][j] = (in && m < M) ? x : f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int m = 0; m < MB; ++m) {
          float t = v[c * MB + m];
          t = __builtin_fmaf(a[m][j][0], w[c][j][0], t);
          t = __builtin_fmaf(a[m][j][1], w[c][j][1], t);
          t = __builtin_fmaf(a[m][j][2], w[c][j][2], t);
          t = __builtin_fmaf(a[m][j][3], w[c][j][3], t);
          v[c * MB + m] = t;
        }
  }
  int base = 0, count = 0;
  LaneReduceScatter<4 * MB, 32, 64>::run(v, lane, base, count);
#pragma unroll
  for (int i = 0; i < 4; ++i)          // (count <= 3 for the instantiated row counts; lanes that hold the same sums write the same)
    if (i < count) wsum[wave][base + i] = v[i];
  __syncthreads();
  if (fin) {
    const float out = ((wsum[0][tid] + wsum[1][tid]) + wsum[2][tid]) + wsum[3][tid];
    lstm_cell_bwd_finish(cell, f_m * cell.H + n0 + f_c, pre, out + res);
  }
}

template <int MB>
static hipError_t launch_rec_fewrows_cfg(const RecBatch& b, const LstmCellBwdArgs* cells, int maxN, hipStream_t stream) {
  hipLaunchKernelGGL(rec_fewrows_reg_kernel<MB>, dim3((maxN + 3) / 4, b.count), dim3(256), 0, stream, b, cells[0],
                     cells[b.count > 1 ? 1 : 0]);
  return hipGetLastError();
}

// Every segment's K must be a multiple of 16 in [1024, 2048] (a wave's quarter in 16-byte pieces, two per lane).  The one
// caller, the wavefront of the training LSTM's reverse pass, guarantees it: it runs only when 4 H is a multiple of 256,
// and every segment has K = 4 H (carve_train_lstm in api_lstm.hip).
hipError_t launch_rec_fewrows(const RecBatch& b, const LstmCellBwdArgs* cells, hipStream_t stream) {
  int maxN = 0, maxM = 0;
  for (int i = 0; i < b.count; ++i) {
    const RecProb& p = b.p[i];
    if (p.nseg < 1 || p.nseg > 2) return hipErrorInvalidValue;
    for (int g = 0; g < p.nseg; ++g)
      if (p.seg[g].K < 1024 || p.seg[g].K > 2048 || p.seg[g].K % 16 != 0) return hipErrorInvalidValue;
    maxN = p.N > maxN ? p.N : maxN;
    maxM = p.M > maxM ? p.M : maxM;
  }
  if (maxM > FEWROWS_MAX_M) return hipErrorInvalidValue;
  if (maxM <= 4) return launch_rec_fewrows_cfg<4>(b, cells, maxN, stream);
  if (maxM <= 8) return launch_rec_fewrows_cfg<8>(b, cells, maxN, stream);
  if (maxM <= 12) return launch_rec_fewrows_cfg<12>(b, cells, maxN, stream);
  return launch_rec_fewrows_cfg<16>(b, cells, maxN, stream);
}

}  // namespace empose
