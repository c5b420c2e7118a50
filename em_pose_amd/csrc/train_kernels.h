// Launch interfaces of the training kernels (bn_prelu.hip, train_cols.hip, train_fused.hip, gemm_train_x3.hip,
// gemm_atb.hip, train_glue.hip, train_loss.hip, adam.hip).  Internal, not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include <initializer_list>
#include <utility>

namespace empose {

// Train-mode BatchNorm1d + PReLU, forward or backward (bn_prelu.hip).
struct BnPreluArgs {
  int M, C;
  const float* x; int ldx;
  const float* gamma; const float* beta; const float* slope;   // slope: one device float
  float eps, momentum;
  float* running_mean; float* running_var; long long* num_batches_tracked;   // forward only, may be null
  float* z; int ldz;                                                         // forward output
  float* save_mean; float* save_rstd;                                        // written by forward, read by backward
  const float* dz; int lddz; float* dx; int lddx;                            // backward
  float* dgamma; float* dbeta; float* dslope_partial;                        // [C], [C], [ceil(C / 32)] scratch
  float* dslope; int* counter;   // slope gradient (one float); arrival counter, zero before the first launch, self re-arming
  float* workspace = nullptr;    // bn_prelu_workspace_floats(M, C) floats: partial sums of the row-split path (large M)
  int accumulate = 0;            // backward: add to dgamma / dbeta / dslope instead of overwriting them
};
// One train-mode layer (product + BatchNorm + PReLU, forward or backward) of one or two MLPs as ONE launch at small
// batches (train_cols.hip): a workgroup per 16 columns x quarter of the rows, the column statistics exchanged between
// the row parts through a mailbox of tagged words.
struct ColsNet {
  const float* A; int lda;           // operand rows [M][K]: the layer input (forward) / the cotangent dZ_l (backward)
  const float* W; int ldw;           // [N][K]: W_l (forward) / W_l^T (backward: rows = columns of the layer below);
  int w_kmajor, Kw;                  // backward: W is W_l itself, [Kw][N] with Kw <= K rows -- no transposed copy needed
  const float* bias;                 // forward: [N]
  int N, K;                          // K % 4 == 0, lda % 4 == 0, ldw % 4 == 0
  const float* gamma; const float* beta; const float* slope;       // BatchNorm / PReLU of the N columns
  float* running_mean; float* running_var; long long* num_batches; // forward, may be null
  const float* z_in; float* z; int ldz;   // pre-BatchNorm rows: written by the forward, read (z_in) by the backward
  float* out; int ld_out;            // forward: the activations (mode 1: the plain product); backward: dZ of the N columns
  float* mean; float* rstd;          // [N]: written by the forward, read by the backward
  float* dgamma; float* dbeta; float* dslope;   // backward
};
struct ColsArgs {
  ColsNet net[2];
  int n_nets, M;
  float eps, momentum;
  int accumulate;
  unsigned tag;                      // unique among the launches that share the mailbox since it was zeroed; > 0
  unsigned long long* mailbox;       // cols_mailbox_words(widest N) words
  int R, tiles_per_part, s_max, slices_per_group, plain, spin_limit; unsigned* timeouts;   // set by launch_cols
};
constexpr int COLS_MAX_ROWS = 512;
size_t cols_mailbox_words(int n_max);
bool cols_launchable(int n_max, int n_nets);   // every workgroup of such a launch resident at once on this device
hipError_t launch_cols(ColsArgs a, int mode, hipStream_t stream);   // mode 0 forward, 1 forward without BatchNorm, 2 backward

constexpr int BN_SINGLE_PASS_ROWS = 1024;   // up to here one workgroup per 32 columns walks all rows
size_t bn_prelu_workspace_floats(int M, int C);
hipError_t launch_bn_prelu(const BnPreluArgs& a, bool backward, hipStream_t stream);

// ---------------------------------------------------------------------------------------------------------------
// Train-mode MLP layer with the BatchNorm / PReLU passes folded into the GEMMs (train_fused.hip)
// ---------------------------------------------------------------------------------------------------------------
struct TrainGemmArgs {       // C[M][N] = A'[M][K] . W[N][K]^T (+ bias), 64 x 128 tile
  const float* A; int lda;
  const float* W; int ldw;
  float* C; int ldc;
  int M, N, K;               // K % 4 == 0, lda / ldw / ld_ay % 4 == 0, 16-byte aligned operands
  const float* bias;         // [N] or nullptr
  // A operand as it is staged.  amode 1: A' = PReLU(s[k] A + t[k]) (a_slope: one device float)
  const float* a_s; const float* a_t; const float* a_slope;
  const float* a_y; int ld_ay; const float* a_c;   // (amode 2, dev: A' = c[k] A + c[K + k] Y[m][k] + c[2K + k])
  // epilogue.  emode 1: also per 32-row block and column the sum and centred sum of squares of C -> part [M/32][2][N];
  // emode 2: the product is dA: C = dyh = dA * PReLU'(e_s y + e_t) and part [M/32][3][N] = sums of dyh,
  // dyh * (y - mean) rstd, (yhat <= 0) dA yhat
  float* part;
  const float* e_y; int ld_ey; const float* e_s; const float* e_t; const float* e_mean; const float* e_rstd;
  const float* e_slope;
};
hipError_t launch_gemm_train(const TrainGemmArgs& p, int amode, int emode, hipStream_t stream);
// The same products (amode 0) on three bf16 pieces per operand for large batches (gemm_train_x3.hip, gemm_train_x3_kernel):
// `wfrag` = the weight matrix W [N][K] as pieces in fragment order, made by launch_pack_x3 once per optimiser step.
bool gemm_train_x3_applicable(int M, int N, int K);
hipError_t launch_gemm_train_x3(const TrainGemmArgs& p, const unsigned short* wfrag, int emode, hipStream_t stream);
size_t pack_x3_elems(int N, int K);
hipError_t launch_pack_x3(const float* W, int ldw, int N, int K, unsigned short* out, hipStream_t stream);
struct BnFusedFwdArgs {
  int M, C; const float* part;                        // [ceil(M / 32)][2][C]
  const float* gamma; const float* beta; float eps, momentum;
  float* running_mean; float* running_var; long long* num_batches_tracked;   // may be null
  float* mean; float* rstd; float* s; float* t;       // [C] each: statistics and the fused transform a = PReLU(s y + t)
};
hipError_t launch_bn_fused_combine_fwd(const BnFusedFwdArgs& a, hipStream_t stream);
struct BnFusedBwdArgs {
  int M, C; const float* part;                        // [ceil(M / 32)][3][C]
  const float* gamma; const float* mean; const float* rstd;
  float* dgamma; float* dbeta; float* dslope; float* dslope_partial;   // [C], [C], [1], [ceil(C / 64)] scratch
  float* coef;                                        // [3][C]: dY = coef0 dyh + coef1 y + coef2
  int accumulate;
};
hipError_t launch_bn_fused_combine_bwd(const BnFusedBwdArgs& a, hipStream_t stream);
size_t bn_fused_partial_floats(int M, int C);
// Round 4: combine + apply in one launch on materialised activations / cotangents (train_fused.hip, "finish" kernels).
struct BnFinishFwdArgs {
  int M, C; const float* part;                        // [ceil(M / 32)][2][C] from the GEMM's statistics epilogue
  const float* gamma; const float* beta; float eps, momentum;
  float* running_mean; float* running_var; long long* num_batches_tracked;   // may be null
  float* mean; float* rstd; float* s; float* t;       // [C] each (out)
  const float* y; int ldy;                            // the GEMM's output
  float* act; int ld_act;                             // a = PReLU(s y + t)
  const float* slope;
  int rows_per_block = 0;                             // (set by the launcher)
};
hipError_t launch_bn_finish_fwd(BnFinishFwdArgs a, hipStream_t stream);
struct BnFinishBwdArgs {
  int M, C; const float* part;                        // [ceil(M / 32)][3][C] from the dX GEMM's epilogue
  const float* gamma; const float* mean; const float* rstd;
  float* dgamma; float* dbeta; float* dslope;         // [C], [C], [1]
  float* dslope_partial; int* counter;                // [ceil(C / 32)] scratch; a zeroed int (re-arms itself)
  int accumulate;
  float* dyh; int ld;                                 // in: dA * PReLU'(yhat); out: dY (in place)
  const float* y; int ldy;
  int rows_per_block = 0;
};
hipError_t launch_bn_finish_bwd(BnFinishBwdArgs a, hipStream_t stream);
hipError_t launch_bn_fused_apply_bwd(float* dyh, const float* y, const float* coef, int M, int C, hipStream_t stream);

// ---------------------------------------------------------------------------------------------------------------
// Training backward (gemm_atb.hip, train_glue.hip, train_loss.hip, adam.hip)
// ---------------------------------------------------------------------------------------------------------------
constexpr int ATB_MAX_SEG = 8;
struct AtbArgs {             // C[N][ldc] = A[M][lda]^T . B[M][ldb]  (+ bias[n] = sum_m A[m][n])
  const float* A; int lda;
  const float* B; int ldb;
  float* C; int ldc;
  float* bias;               // [N] or nullptr
  int M, N, K;
  int accumulate;            // 1: C += A^T B, bias += column sums (gradient accumulation over the LGD iterations)
  // Row segments: with n_seg > 0 the M rows are n_seg blocks of seg_rows rows (a multiple of 32) that live at
  // A_seg[s] / B_seg[s] (same leading dimensions) -- the operands of one layer over the applications of the LGD loop.
  int n_seg = 0, seg_rows = 0;
  const float* A_seg[ATB_MAX_SEG] = {};
  const float* B_seg[ATB_MAX_SEG] = {};
  // Operand transform of the fused train-mode layer (train_fused.hip), per segment (index 0 without segments):
  //   b_mode 1: B' = PReLU(Bs[k] B + Bs[K + k])   (the layer input a_{l-1} re-formed from y_{l-1}; b_slope: device float)
  int b_mode = 0;
  const float* Bs_seg[ATB_MAX_SEG] = {};
  const float* b_slope = nullptr;
  // set by launch_gemm_atb
  int S; float* partial; float* bias_partial;
};
hipError_t launch_window_mean(const float* in, int ld_in, float* out, int ld_out, int T, int F, int C, hipStream_t stream);
hipError_t launch_axpby2d(int rows, int cols, float alpha, const float* x, int ldx, float beta, const float* y, int ldy,
                          float* out, int ldo, hipStream_t stream);
hipError_t launch_lgd_assemble(int T, int d_in, const float* x0, int ld0, const float* pose, const float* shape, float* X,
                               int ldx, hipStream_t stream);
hipError_t launch_lgd_update(int B, int F, float step, int shape_avg, const float* pose, const float* d_pose,
                             const float* shape, const float* d_shape, float* pose_next, float* shape_next,
                             hipStream_t stream);
hipError_t launch_lgd_cotangent(int B, int F, int first, const float* d_pose, const float* d_shape, const float* vp,
                                const float* vs, const float* g_theta, int ld_g, const float* g_beta, int ld_gb, float* Dp,
                                float* Ds, float step, int shape_avg, float* dpad, float* dspad, hipStream_t stream);
struct LossArgs {
  int B, F, N1, n_markers;
  int used_slot[12];                       // column slot of virtual sensor m in the network input, or -1
  const float* pose_hist; const float* shape_hist; const float* pos_hist; const float* ori_hist;   // [N1][T][66|10|36|108]
  const float* joints_final;               // [T][66]
  const float* pose_gt; const float* shape_gt; const float* joints_gt;   // [T][66], [B][10], [T][66] or nullptr
  const float* x_in; int ldx;              // measured sensors in the network input layout
  const int* seq_lengths; const float* masks;   // [B] or nullptr, [T][12] or nullptr
  float w_pose, w_shape, w_fk, w_rec;
  float* d_pose; float* d_shape; float* d_pos; float* d_ori; float* d_joints;
  float* partial;                          // [4][N1 * T]
  float* loss_vals;                        // [5]
};
hipError_t launch_lgd_losses(const LossArgs& a, hipStream_t stream);
constexpr int ADAM_CHUNK = 4096;
struct AdamArgs {
  void* const* params; void* const* grads; void* const* exp_avg; void* const* exp_avg_sq;   // device pointer tables
  const long long* sizes; const int* chunk_tensor; const long long* chunk_offset;
  float beta1, beta2, eps, step_size, inv_sqrt_bc2;
};
hipError_t launch_adam(const AdamArgs& a, int n_chunks, hipStream_t stream);
int atb_splits(int M, int N, int K);
size_t atb_workspace_floats(int M, int N, int K);
size_t atb_workspace_floats_max(int M, std::initializer_list<std::pair<int, int>> products);   // over (N, K) pairs
hipError_t launch_gemm_atb(AtbArgs a, float* workspace, size_t workspace_floats, hipStream_t stream);
hipError_t launch_transpose(const float* src, int ld_src, float* dst, int ld_dst, int rows, int cols, hipStream_t stream);
hipError_t launch_add2(const float* a, const float* b, float* out, int n, hipStream_t stream);
struct LstmCellBwdArgs {
  const float* gates;        // [B][F][4H] saved activations
  const float* c_all;        // [B][F][H]
  const float* c0;           // [B][H] or nullptr (zeros)
  const float* dy; int ld_dy;   // [B][F][ld_dy] cotangent of the layer's output sequence, or nullptr
  const float* dh_in;        // [B][H] from step t + 1, or nullptr (zeros)
  float* dc;                 // [B][H] in: from step t + 1, out: for step t - 1
  float* dgates;             // [B][F][4H] pre-activation gradients (this step's rows are written)
  float* dh_carry;           // [B][H] out: dh_in of rows that had ended at this step, else 0
  const int* seq_lengths;
  int B, F, H, t;
};
hipError_t launch_lstm_cell_bwd(const LstmCellBwdArgs& a, hipStream_t stream);

}  // namespace empose
