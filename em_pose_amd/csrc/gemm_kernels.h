// Launch interfaces of the fp32 GEMM kernels (gemm_f32.hip, gemm_rec.hip; launch_gemm_rows: mlp_fused.hip).  Internal, not
// part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace empose {

// ---------------------------------------------------------------------------------------------------------------
// fp32 matrix-core linear layer:  C[m][n] = act( (sum_k A[m][k] * W[n][k]) * scale[n] + shift[n] ) (+ resid[m][n])
// ---------------------------------------------------------------------------------------------------------------
struct GemmProb {
  const float* A; int lda;
  const float* W; int ldw;
  float* C; int ldc;
  int M, N, K;              // K % 4 == 0, lda/ldw % 4 == 0, A/W 16-byte aligned
  const float* scale;       // [N] or nullptr (=1)
  const float* shift;       // [N] or nullptr (=0)
  const float* resid; int ldr;  // added after the activation (skip connections) or nullptr
  int act;                  // 0 none, 1 PReLU(slope) then + resid, 2 + resid then ReLU
  float slope;
  // Train-mode layer fusion (gemm_tn_f32_kernel<Cfg, 2> only; see TrainGemmArgs / train_fused.hip):
  const float* a_s = nullptr; const float* a_t = nullptr; const float* a_slope = nullptr;   // A' = PReLU(s[k] A + t[k])
  float* stat_part = nullptr;                                                               // column statistics of C
  const float* e_y = nullptr; int ld_ey = 0;                                                // product is dA: C = dyh, sums
  const float* e_s = nullptr; const float* e_t = nullptr; const float* e_mean = nullptr; const float* e_rstd = nullptr;
  const float* e_slope = nullptr;
};
struct GemmBatch { GemmProb p[2]; int count; int role = 0; int xcd_swizzle = 1; };  // role 1 = update-net hidden layer (profiling name only)

// At most FEWROWS_MAX_M rows against a long K: the matrix-vector kernel of gemm_f32.hip (launch_gemm picks it by itself).
// With `cell` (back-propagation through time, layer after layer): the product is dh of the step below (N = H, one value per
// (row, unit)), and the kernel runs that step's cell on it instead of storing C.
constexpr int FEWROWS_MAX_M = 16;
struct LstmCellBwdArgs;
bool gemm_fewrows_applicable(int M, int N, int K);
hipError_t launch_gemm_fewrows_cell(const GemmProb& p, const LstmCellBwdArgs& cell, hipStream_t stream);

// The recurrent products of back-propagation through time (gemm_rec.hip): one launch forms the incoming hidden-state
// cotangent of up to two (layer, step) units and runs their cells on it.  A unit's product may have two K segments with
// their own operands -- in the wavefront over two layers, dh0_t = dG0_{t+1} . W_hh0 + dG1_t . W_ih1 is one K = 8H product
// over the rows [dG0_{t+1} | dG1_t] that are never concatenated in memory.  C = sum_seg A_seg . W_seg^T (+ resid); the
// unit's cell consumes it, nothing is stored.  The layer-after-layer form launches one unit of one segment.
struct RecSeg { const float* A; int lda; const float* W; int ldw; int K; };   // A [M][lda], W [N][ldw], K % 4 == 0
struct RecProb { RecSeg seg[2]; int nseg; int M, N; const float* resid; int ldr; };
struct RecBatch { RecProb p[2]; int count; };
// K split over workgroups (more than FEWROWS_MAX_M rows, long K, small output; at most 16 slices of 256 per unit, a
// segment's last slice may be partial): whether one segment of K is this kernel pair's shape, and the floats of `workspace`
// for `count` units of K_total_max in all.  Deterministic: the partial tiles are added in slice order by a second kernel.
bool rec_ksplit_applicable(int M, int N, int K);
size_t rec_ksplit_workspace_floats(int M, int N, int K_total_max, int count);
// cells[i] is the cell of unit i.  launch_rec_fewrows: at most FEWROWS_MAX_M rows, every segment's K a multiple of 16 in
// [1024, 2048].
hipError_t launch_rec_ksplit(const RecBatch& b, const LstmCellBwdArgs* cells, float* workspace, hipStream_t stream);
hipError_t launch_rec_fewrows(const RecBatch& b, const LstmCellBwdArgs* cells, hipStream_t stream);

// C[M][N] = A . W^T (+ bias) with strided operands: A(m, k) = A[m * a_rs + k * a_ks], W(n, k) = W[n * w_rs + k * w_ks]
// (small problems only, split-K tile; `strided_gemm_applicable`).
struct StridedGemm {
  const float* A; long a_rs, a_ks;
  const float* W; long w_rs, w_ks;
  float* C; int ldc;
  const float* bias;
  int M, N, K;
};
bool strided_gemm_applicable(int M, int N);
hipError_t launch_strided_gemm(const StridedGemm& p, hipStream_t stream);

// Launches one grid covering all problems of the batch (blockIdx.y selects the problem).
hipError_t launch_gemm(const GemmBatch& batch, hipStream_t stream);
const char* gemm_kernel_name(int M, int N, int K, int count, int role);

// One linear layer C = A . W^T with A's row block resident in LDS and W (fragment order) streamed from L2.
bool gemm_rows_applicable(int M, int N, int K);
hipError_t launch_gemm_rows(const float* A, int lda, const float* Wp, float* C, int ldc, int M, int N, int K,
                            hipStream_t stream);

}  // namespace empose
