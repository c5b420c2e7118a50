// Internal launch interfaces of the HIP kernels (gfx950 only). Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <initializer_list>
#include <utility>
#include <vector>

namespace empose {

// Kernel-variant selection for A/B and bit-identity tests (empose_set_option in the C ABI).  Plain process-wide ints set
// by an explicit call -- the library never reads the environment.  X(name, default) per option: this one list makes the
// fields of Options and the names empose_set_option / empose_get_option take (api.hip); empose_reset_options restores
// the defaults.
#define EMPOSE_OPTIONS(X) \
  X(mlp_fused, 1)      /* one-launch LDS-resident update MLPs (0: layer by layer) */ \
  X(lstm_persist, 1)   /* whole-sequence small-batch LSTM kernel (0: step launches) */ \
  X(gemm_splitk, 1)    /* split-K tile for problems of few output tiles (0: generic tiles) */ \
  X(heads_rows, 1)     /* large batches: both init heads as one row-block product (0: two problems on the generic tile) */ \
  X(lstm_seq, 0)       /* large batches: the whole sequence in one cooperative launch (measured slower: 0 = a launch per wavefront step) */ \
  X(bptt_wave, 1)      /* training: the reverse recurrences of a 2-layer LSTM as a wavefront (0: layer after layer) */ \
  X(gemm_wide, 1)      /* 256 x 256 four-wave tile (0: generic tiles) */ \
  X(smpl_tile, 1)      /* frame-per-lane SMPL sub-mesh kernel: 0 never, 1 from 16384 frames on, 2 always */ \
  X(smpl_fuse, 1)      /* on that path: update + feature row / Rodrigues reverse inside the blend GEMMs (0: own kernels) */ \
  X(train_fused, 0)    /* train-mode BatchNorm / PReLU folded into the GEMMs: 0 never (default: measured no faster, \
                             DESIGN.md), 1 above 1024 rows, 2 always */ \
  X(atb_target, 0)     /* workgroups the A^T B weight-gradient GEMM aims for when it splits its reduction (0: by size) */ \
  X(atb_fast, 1)       /* A^T B: whole-tile / whole-chunk problems on the branch-free interior kernel (0: the general kernel) */ \
  X(atb_chunk, 0)      /* rows per staged chunk of that kernel, 16 or 32 (0: by size) */ \
  X(mesh_skin_mfma, 0) /* split-bf16 full-mesh variant: the bone blend as a second matrix-core contraction (mesh_rows_bf16s_kernel; \
                             measured 9 % SLOWER than vector skinning: 15.6 against 17.1 M frames/s, so off by default) */ \
  X(train_epi, 1)      /* train-mode MLP layer: BatchNorm statistics in the GEMM epilogues + ONE combine-and-apply launch per \
                             layer and direction (train_fused.hip, finish kernels): 0 never, 1 above BN_SINGLE_PASS_ROWS rows, 2 always */ \
  X(spin_limit, 0)     /* polls of the cooperative LSTM kernels give up after this many spins (0: their own limits) */ \
  X(rows_x3, 1)        /* the row-block products with fused prologue / epilogue (blend GEMMs of the frame-per-lane SMPL path, init \
                             heads) on the same three-piece bf16 arithmetic; 0: the fp32 MFMA instruction */ \
  X(lstm_x3, 1)        /* large-batch LSTM steps (inference, uni-directional): fp32 products as six bf16-MFMA products of three \
                             bf16 pieces per operand; 1: lstm_x3.hip (K-split waves); 2: lstm_rows_x3.hip (row-split waves, weights \
                             through LDS, cell update in registers -- round 6, measured 10 % SLOWER: 47.5 against 42.9 us per \
                             launch, profiles/r06_lstm_rows_lab.txt, so opt-in); 3: lstm_chain16_x3.hip, kernel 1 on \
                             v_mfma_f32_16x16x32_bf16 -- measured FASTER: 37.8 against 39.5 us per launch in the headline profile, \
                             38.8 against 40.7 stand-alone, 5.20 against 5.30 ms per step (profiles/r07_*; docs/history.md \
                             "LSTM"), equal to rounding only: what the default 1 takes while lstm_chain16 is on, 3 forces it; \
                             0: the fp32 MFMA instruction (lstm_chain_kernel) */ \
  X(train_cols, 1)     /* training at <= 512 rows: a layer's product + BatchNorm + PReLU as one launch, both update networks \
                             side by side (train_cols.hip); 0: a product and a BatchNorm launch per layer and network */ \
  X(cols_coop, 1)      /* those one-launch layers, eager: launched with hipLaunchCooperativeKernel (all workgroups resident by \
                             the runtime's guarantee); 0: the ordinary launch (residency argued from the occupancy query) */ \
  X(mesh_x3, 1)        /* full-mesh vertices: blend shapes as six bf16-MFMA products of three bf16 pieces per operand \
                             (mesh_x3.hip): 1 stores staggered into the next tile's products, 2 stores at the end of the tile, \
                             3 skinning software-pipelined under the next tile's products; 0: the fp32 MFMA instruction \
                             (mesh_rows_kernel) */ \
  X(train_x3, 1)       /* training at more than 1024 rows: the layer products y = a W^T and dA = dY W of the update networks on \
                             three bf16 pieces (gemm_train_x3_kernel) when the caller supplies the packed weights \
                             (empose_mlp_params::weight_x3 / weight_t_x3); 0: the fp32 MFMA tile */ \
  X(lstm_midseq, 0)    /* 1: medium batches (4 .. 64 rows, inference): the whole sequence in one cooperative launch with the \
                             weight pieces in registers (lstm_midseq_x3.hip) -- built, same bits, measured SLOWER than a launch \
                             per wavefront step (10.5 against 8.2 us per step at 32 rows: a hand-over between XCDs costs more \
                             than a kernel boundary; profiles/r06i_lstm_midseq_lab.txt), so opt-in */ \
  X(lstm_mid16, 1)     /* LSTM steps of 17 .. 64 rows: 64 rows x 4-unit tiles on all 256 CUs (lstm_mid16_x3.hip); 0: the 8-unit \
                             tiles of lstm_mid_x3.hip (128 workgroups) */ \
  X(lstm_mid_x3, 1)    /* LSTM steps of 17 .. 256 rows (inference, uni-directional) on three bf16 pieces, 64 x 8-unit tiles \
                             (lstm_mid_x3.hip); 0: lstm_mid_kernel (fp32 MFMA, operands through LDS) */ \
  X(lstm_fewrows, 1)   /* LSTM steps of 4 .. 16 rows: all threads of a workgroup split K, lane reduce-scatter (lstm_fewrows_kernel), \
                             instead of the whole-sequence kernel / lstm_small_kernel (0: those; they share their bits) */ \
  X(mlp_x3, 1)         /* fused update MLPs: fp32 products as six bf16-MFMA products of three bf16 pieces per operand \
                             (mlp_fused_x3.hip: fp32-equivalent accuracy, measured equal to the fp32 instruction's against \
                             float64); 0: the fp32 MFMA instruction (mlp_fused.hip); any other value is on.  Which \
                             instruction and how many pieces is mlp_fused16's and mlp_pair16's choice */ \
  X(last_pass_joints, 1) /* LGD forward, frame-per-lane path: an SMPL evaluation nobody asks sensor outputs of (the last pass \
                             without histories) multiplies only the rest-joint column tiles of the blend matrix and runs the \
                             chain alone (smpl_tile_kernel, CHAIN_ONLY); 0: the whole sub-mesh, as for every other pass */ \
  X(lstm_state_direct, 1) /* large-batch LSTM steps (lstm_x3.hip), new sequences: the piece planes of the zero initial state by \
                             one fill, h_n / c_n stored by the last step of each layer; 0: a split launch and a fill per layer, \
                             2 L trailing copies */ \
  X(lstm_skip_dead, 1) /* chain step kernels (lstm_x3 = 1 / 3): work whose result nobody reads is left out, same bits -- the \
                             recurrent k-steps of a unit whose h_{t-1} is the zero state of a new sequence, and without \
                             seq_lengths (lstm_state_direct path) the fp32 h_prev loads / h_next stores; 0: all of it runs */ \
  X(mlp_fused16, 1)    /* fused update MLPs with mlp_x3 != 0: the products on v_mfma_f32_16x16x32_bf16 (mlp_fused_x3_kernel<16>, \
                             weights in the [k-step of 32][16-column tile][piece] order); 0: v_mfma_f32_32x32x16_bf16 \
                             (mlp_fused_x3_kernel<32>).  Equal to rounding, not to the bit */ \
  X(mlp_pair16, 1)     /* fused update MLPs with mlp_x3 != 0 and mlp_fused16 != 0: every fp32 product from TWO f16 pieces per \
                             operand under per-row / per-column power-of-two scales, three v_mfma_f32_16x16x32_f16 instead of six \
                             of the bf16 instruction (mlp_fused_x3_kernel<PAIR16>, f16pair.h); 0: the three bf16 pieces of \
                             mlp_fused_x3_kernel<16>.  Equal to rounding, not to the bit */ \
  X(lstm_chain16, 1)   /* large-batch LSTM steps with lstm_x3 = 1: lstm_chain16_x3.hip (v_mfma_f32_16x16x32_bf16) where the model \
                             has the LSTM_MID16 weight order; 0: lstm_chain_x3_kernel (32x32x16) */ \
  X(lstm_pair16, 1)    /* large-batch LSTM steps on the 16x16x32 chain kernel (lstm_x3 = 3, or 1 with lstm_chain16 on): every \
                             operand the kernel itself produced -- h_{t-1} and the layer below's h_t, both in [-1, 1] -- as TWO \
                             f16 pieces under the fixed scale 2^14, weights under per-column power-of-two scales, three \
                             v_mfma_f32_16x16x32_f16 instead of six of the bf16 instruction (lstm_chain16_pair_kernel, \
                             f16pair.h); the raw input of layer 0 and a caller's h0 stay on three bf16 pieces and share the \
                             accumulator; 0: three bf16 pieces throughout (lstm_chain16_x3_kernel).  Equal to rounding, not to \
                             the bit */

struct Options {
#define EMPOSE_OPTION_FIELD(name, default_value) int name = default_value;
  EMPOSE_OPTIONS(EMPOSE_OPTION_FIELD)
#undef EMPOSE_OPTION_FIELD
};
Options& options();

// Dynamic LDS above the 64 KB a kernel may use by default: hipFuncAttributeMaxDynamicSharedMemorySize of `fn` on the
// CURRENT device, raised when `bytes` exceeds what was already allowed there (cached per (device, kernel): a process that
// drives several GPUs sets it on each).  More than a CU has (LDS_BYTES_PER_CU) is refused here instead of at the launch.
// The cooperative whole-sequence LSTM kernels poll exchange words written by other workgroups; a poll that exceeds its
// spin limit gives up, poisons the outputs with NaN (it does not hang) and counts itself in ONE host-mapped word that the
// entry points read without synchronising: the next empose_* call that runs a recurrence returns EMPOSE_ETIMEOUT, and
// empose_async_status() reports it to a caller that has synchronised.  Option "spin_limit" (0 = the kernels' own limits)
// forces a limit, for tests.
unsigned* poll_timeout_word();          // device-visible address of the counter
unsigned poll_timeouts_take();          // host: read and clear
unsigned poll_timeouts_peek();          // host: read
int poll_spin_limit(int kernel_default);   // option "spin_limit" where it is set, else the polling kernel's own limit
constexpr size_t LDS_BYTES_PER_CU = 160 * 1024;
hipError_t allow_dynamic_lds(const void* fn, size_t bytes);
// A launch of a kernel with a large dynamic-LDS request: raises the limit of `fn` (above), launches, returns the launch's
// error.  `args` convert to the kernel's parameter types here, as they would at a direct launch.
template <typename... Params, typename... Args>
inline hipError_t launch_lds(void (*fn)(Params...), dim3 grid, dim3 block, size_t lds_bytes, hipStream_t stream,
                             const Args&... args) {
  if (hipError_t e = allow_dynamic_lds(reinterpret_cast<const void*>(fn), lds_bytes)) return e;
  hipLaunchKernelGGL(fn, grid, block, lds_bytes, stream, static_cast<Params>(args)...);
  return hipGetLastError();
}
// Workgroups of `fn` (block size `threads`, `lds_bytes` of dynamic LDS) that can be resident at once on the CURRENT device:
// what a cooperative launch may ask for.  Cached per (device, kernel); the attribute above is set on the way.
hipError_t coresident_blocks(const void* fn, int threads, size_t lds_bytes, int* blocks);

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

// Launches one grid covering all problems of the batch (blockIdx.y selects the problem).
hipError_t launch_gemm(const GemmBatch& batch, hipStream_t stream);
const char* gemm_kernel_name(int M, int N, int K, int count, int role);

// One or two whole MLPs (all layers) in one launch: a workgroup keeps the activations of 64 rows in LDS from the first
// layer to the last (mlp_fused.hip).
constexpr int FUSED_MAX_LAYERS = 8;
constexpr int FUSED_MAX_WIDTH = 512;     // widest layer output the four 128-column waves cover
struct FusedLayer {
  const float* W; int K, N;              // weights in fragment order (api_model.hip pack_fragments), K % 4 == 0, N <= FUSED_MAX_WIDTH
  const float* scale; const float* shift;
  float slope; int act;                  // 0 none, 1 PReLU
  const float* wexp = nullptr;           // pair16 only: [N] the inverse of the power-of-two scale W's columns were packed with
};
struct FusedNet {
  const float* x; int ldx;
  float* out; int ld_out;
  int n_layers;                          // the last layer writes `out`, the others stay in LDS
  FusedLayer layer[FUSED_MAX_LAYERS];
};
struct FusedMlpArgs { FusedNet net[2]; int count; int M; };
hipError_t launch_mlp_fused(const FusedMlpArgs& args, hipStream_t stream);
// The form the products of that launch take, and with it the order FusedLayer::W is packed in (api_model.hip
// pack_fragments keeps one table per form):
//   fp32    the fp32 MFMA instruction (mlp_fused.hip, launch_mlp_fused);
//   x3_32   three bf16 pieces per operand on v_mfma_f32_32x32x16_bf16, six products (mlp_fused_x3_kernel<32>);
//   x3_16   the same pieces on v_mfma_f32_16x16x32_bf16 (mlp_fused_x3_kernel<16>);
//   pair16  two f16 pieces per operand under power-of-two scales on v_mfma_f32_16x16x32_f16, three products
//           (mlp_fused_x3_kernel<PAIR16>, f16pair.h), FusedLayer::wexp set.
enum class FusedForm { fp32, x3_32, x3_16, pair16 };
constexpr int FUSED_FORMS = 4;
// The same launch in one of the piece forms (mlp_fused_x3.hip; `form` is not fp32).  Hidden widths must be multiples of 64.
hipError_t launch_mlp_fused_x3(const FusedMlpArgs& args, FusedForm form, hipStream_t stream);
// One linear layer C = A . W^T with A's row block resident in LDS and W (fragment order) streamed from L2.
bool gemm_rows_applicable(int M, int N, int K);
hipError_t launch_gemm_rows(const float* A, int lda, const float* Wp, float* C, int ldc, int M, int N, int K,
                            hipStream_t stream);

// ---------------------------------------------------------------------------------------------------------------
// LSTM
// ---------------------------------------------------------------------------------------------------------------
struct LstmUnitArgs {        // one (layer, direction), selected by blockIdx.z
  const float* w_ih;   // [4H][in_k]
  const float* w_hh;   // [4H][H]
  const float* bias;   // [4H] = b_ih + b_hh
  int in_k;            // width of the unit's input
  const float* in_seq; int in_ld;  // stored input sequence [B][F][in_ld] (used when in_from < 0)
  int in_from;         // >= 0: the input is the hidden state of unit `in_from` after its step (stacked wavefront)
  int t_offset;        // the unit processes step k = s - t_offset
  int reverse;         // 1: at step k row b visits time len_b - 1 - k
  float* h[2];         // [B][H] ping-pong: step k reads h[k & 1], writes h[(k + 1) & 1]
  float* c;            // [B][H] updated in place
  float* y; int y_ld; int y_col;   // output sequence [B][F][y_ld], columns [y_col, y_col + H), or nullptr
  // Training forward (forward units only): what back-propagation through time needs, batch-major like y.
  float* sv_gates = nullptr;       // [B][F][4H] activated gates (i | f | g | o) of every step, or nullptr
  float* sv_c = nullptr;           // [B][F][H] cell state after the step (unchanged past a row's length)
  float* sv_hprev = nullptr;       // [B][F][H] hidden state BEFORE the step; the caller fills slot t = 0 (h_0)
};
struct LstmSeg {             // one operand segment (input part / recurrent part) of a unit's step; built on the host
  const float* a;            // A rows: a + row * lda (+ per-row time offset, below)
  const float* w;            // W rows: w + (gate * H + unit) * ldw
  int lda, ldw;
  int K;
  int tstride;               // != 0: reverse unit on a stored sequence; row b adds max(len_b - 1 - k, 0) * tstride
  int k;                     // the unit's step index
  int ntiles;                // ceil(K / 64)
  int unit;                  // index into LstmWaveArgs::unit
  int pad;
};
struct LstmWaveArgs {
  LstmUnitArgs unit[4];
  int n_units;
  const int* seq_lengths;    // [B] or nullptr (required for reverse units)
  int B, F, H;
  int s;                     // launch index
  // set by lstm_build_chain (lstm_wave.h): blockIdx.z walks through the segments [z_beg[z], z_beg[z] + z_cnt[z]) (two per active unit)
  LstmSeg seg[8];
  int z_beg[4], z_cnt[4];
};
// The fp32 step kernels, one launcher each; plan_lstm (api_lstm.hip) picks, the launchers take no decisions.  All expect the
// segment table built (lstm_build_chain, lstm_wave.h): one unit per slice, lstm_chain_kernel `units_per_block`.  A shape
// outside a kernel's ..._shape_ok is hipErrorInvalidValue.
hipError_t launch_lstm_chain(const LstmWaveArgs& a, int units_per_block, hipStream_t stream);   // lstm_chain.hip
hipError_t launch_lstm_mid(const LstmWaveArgs& a, hipStream_t stream);                          // lstm_mid.hip
bool lstm_small_shape_ok(int B);                                                                 // lstm_fewrows.hip
bool lstm_fewrows_shape_ok(int B, int H, int n_units, const int* in_k);
hipError_t launch_lstm_small(const LstmWaveArgs& a, hipStream_t stream);
hipError_t launch_lstm_fewrows(const LstmWaveArgs& a, hipStream_t stream);
// Whole sequence of a stacked uni-directional LSTM on a LARGE batch in one cooperative launch (lstm_seq.hip,
// lstm_seq_kernel): the units' hidden states rotate through three buffers (h[0], h[1] of the unit + a third one), the
// workgroups of a 64-row group synchronise through `counters` (lstm_seq_counter_uints(B) unsigned, zeroed by the launcher).
struct LstmSeqArgs {
  LstmUnitArgs unit[4];
  float* hs[4][3];
  int n_units;
  const int* seq_lengths;
  int B, F, H;
  unsigned* counters;
  int spin_limit;
  unsigned* timeouts;   // poll_timeout_word(): counts the polls that gave up (the outputs are NaN from there on)
};
// The wavefront step of large batches on the bf16 matrix path, three bf16 pieces per fp32 operand (lstm_x3.hip).  All
// operands arrive in fragment order: weights packed at model creation (api_lstm.hip pack_lstm_x3: [k-step][32-unit block][gate]
// [piece][512 bf16]), activations as A planes [32-row tile][k-step][piece][512 bf16] written by the producing step (hidden
// states) or by launch_lstm_split_rows (stored input, initial state).
struct LstmX3Unit {
  const unsigned short* w3_ih; const unsigned short* w3_hh;
  const float* bias;                 // [4H] = b_ih + b_hh
  const unsigned short* a3_in;       // the unit's input at this step: planes of x_t, or of the unit below's new hidden state
  int ks_in;                         // k-steps of 16 of that input
  // k-steps of 16 of the recurrent operand the chain kernels multiply: H / 16, or 0 where h_{t-1} is the zero state of a new
  // sequence (its products are all +-0: leaving them out changes no bit).  The other step kernels walk H / 16 regardless.
  int ks_rec;
  const unsigned short* a3_rec;      // planes of h_{t-1}
  unsigned short* a3_out;            // planes of h_t
  const float* h_prev; float* h_next; float* c;   // [B][H] fp32: state hand-over and rows past their length
  float* y; int y_ld, y_col;         // output sequence [B][F][y_ld] or nullptr
  int t;                             // the unit's time step in this launch
  // the layer's slices of h_n / c_n ([B][H]) on the launch of its last step, else nullptr: a second copy of what goes to
  // h_next / c (the chain kernels only; the other step kernels ignore them and the caller copies the state out)
  float* h_final = nullptr; float* c_final = nullptr;
  // lstm_chain16_pair_kernel only.  A part (input / recurrent) is walked in pair steps -- its planes hold two f16 pieces of
  // h 2^14, its weights (w3_ih / w3_hh) two f16 pieces of w s_n, both at the three-piece stride -- or in wide steps: three
  // bf16 pieces of the operand as it is, weights those of w s_n 2^14.  inv_scale: [4H] 2^-14 / s_n, applied to the gate sums
  int in_pair = 0, rec_pair = 0;
  const float* inv_scale = nullptr;
};
struct LstmX3Args {
  LstmX3Unit unit[4];
  int n_units, units_per_block;      // blockIdx.z walks units [z * units_per_block, ...)
  const int* seq_lengths;
  int B, F, H;
  // chain kernels: nobody reads the fp32 hidden-state buffers (no seq_lengths: every row live at every step; the last step
  // stores h_final) -- h_prev is not loaded, h_next not stored
  int skip_h_state = 0;
};
hipError_t launch_lstm_chain_x3(const LstmX3Args& a, hipStream_t stream);
// the same step on v_mfma_f32_16x16x32_bf16, weights in the LSTM_MID16 order (lstm_chain16_x3.hip; option lstm_x3 = 3)
hipError_t launch_lstm_chain16_x3(const LstmX3Args& a, hipStream_t stream);
// ... with the operands the kernel produced itself on two f16 pieces (LstmX3Unit::in_pair / rec_pair; option lstm_pair16)
hipError_t launch_lstm_chain16_pair(const LstmX3Args& a, hipStream_t stream);
// the same step with the waves splitting ROWS, the weight block of a k-step shared through LDS and the cell update in
// registers (lstm_rows_x3.hip; option lstm_x3 = 2): one unit per workgroup, `units_per_block` unused
hipError_t launch_lstm_rows_x3(const LstmX3Args& a, hipStream_t stream);
// the step of MEDIUM batches (17 .. 256 rows): 64 rows x 8 units per workgroup, weights in the 8-unit-block order
// (api_lstm.hip pack_lstm_x3 with mid = true), K split over the waves (lstm_mid_x3.hip; option lstm_mid_x3)
hipError_t launch_lstm_mid_x3(const LstmX3Args& a, hipStream_t stream);
// ... at most 64 rows: 4-unit tiles (16 columns, v_mfma_f32_16x16x32_bf16), weights in the order of api_lstm.hip
// pack_lstm_x3_mid16, twice the workgroups (lstm_mid16_x3.hip; option lstm_mid16)
bool lstm_mid16_shape_ok(int B, int H);
hipError_t launch_lstm_mid16_x3(const LstmX3Args& a, hipStream_t stream);
// The whole sequence of a medium batch (B <= 64) in one cooperative launch with the weight pieces in registers
// (lstm_midseq_x3.hip; option lstm_midseq): same tiles, products and bits as the step launches of lstm_mid_x3.hip.
struct LstmMidSeqUnit {
  const unsigned short* w3_ih; const unsigned short* w3_hh;   // the 8-unit-block order of lstm_mid_x3.hip
  const float* bias;                 // [4H] = b_ih + b_hh
  const unsigned short* in3; size_t in_t_stride;   // layer 0: planes of the stored input, bf16 elements per time step
  int ks_in;                         // k-steps of 16 of the unit's input
  unsigned short* xa;                // [F + 1] sets of planes of the unit's hidden state: slot 0 = initial, slot t + 1 = h_t
  const float* h0; float* h_last; float* c;   // [B][H] fp32: initial hidden state, final hidden state, cell state (in place)
  float* y; int y_ld, y_col;         // output sequence [B][F][y_ld] or nullptr
};
struct LstmMidSeqArgs {
  LstmMidSeqUnit unit[4];
  int n_units;
  const int* seq_lengths;
  int B, F, H;
  unsigned* flags;                   // [n_units][H / 8] progress counters (lstm_midseq_flag_uints), zeroed by the launcher
  int spin_limit;
  unsigned* timeouts;                // poll_timeout_word()
};
size_t lstm_midseq_flag_uints(int n_units, int H);
bool lstm_midseq_shape_ok(int B, int H, int n_units, const int* ks_in);
hipError_t launch_lstm_midseq_x3(const LstmMidSeqArgs& a, hipStream_t stream, bool* done);
hipError_t launch_lstm_split_rows(const float* src, long row_stride, long z_stride, int n_z, int B, int K, int KS,
                                  unsigned short* dst, long dst_z_stride, hipStream_t stream);
constexpr int LSTM_SEQ_MIN_B = 257;   // below: lstm_mid_kernel / the small-batch kernels
size_t lstm_seq_counter_uints(int B);
bool lstm_seq_shape_ok(int H, int n_units, const int* in_k);   // enough K tiles per unit (per-unit input widths in_k)
hipError_t launch_lstm_seq(const LstmWaveArgs& a, float* const* h_third, unsigned* counters, hipStream_t stream, bool* done);
// Whole sequence of a stacked uni-directional LSTM in one cooperative launch (lstm_persist.hip, B <= 16); *done = false:
// its workgroups cannot all be resident here.
constexpr int LSTM_PERSIST_B = 16;   // largest batch of the whole-sequence kernel
constexpr int LSTM_FEWROWS_MIN_B = 4;   // from here to 16 rows a step launch of lstm_fewrows_kernel beats it (option lstm_fewrows)
size_t lstm_persist_xch_floats(int n_units, int B, int H);   // its exchange buffer (8-byte aligned)
bool lstm_persist_shape_ok(int B, int H, int n_units, const int* in_k);   // H, in_k <= 512 in 16-byte pieces, rows within LDS
hipError_t launch_lstm_persist(const LstmWaveArgs& a, float* xch, hipStream_t stream, bool* done);

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

// ---------------------------------------------------------------------------------------------------------------
// SMPL sub-mesh kernels
// ---------------------------------------------------------------------------------------------------------------
constexpr int CHAIN_CHUNK = 8;  // pairs per partial-sum chunk of the per-bone (vertex, weight) lists
constexpr int NB = 22;           // body joints

// LDS record of one frame in chain_sensors_kernel (shared with the host, which packs LDS offsets into the tables).
struct ChainLds {  // per-frame float offsets
  int rot, out, g, at, v, dv, u, total;
  // inside u (time-shared): fn | fg | scr   then   part (later: pd, fp64 prefix sums) | m | x
  int fn, fg, scr, part, pd, m, x;
};

__host__ __device__ inline ChainLds chain_layout(int nv, int ncp, int max_deg, int n_chunks) {
  // Live ranges (phases of chain_sensors_kernel): rot P0-P2 | out P0-P5 | g, at P2-P7 | v P3-P4c | dv P4d-P5 |
  // fn P4a-P4b, fg P4c-P4d, scr P4b-P4d | part P5-P5c | m P5c-P6a | pd P6a-P6b | x P6b-P7.  Records that are never
  // live together share their space (rot with the scratch area, dv with v, x with m): 6.9 KB per frame instead of
  // 9.7 KB, i.e. one more workgroup per CU.
  ChainLds l;
  int o = 0;
  l.out = o; o += ncp;
  l.g = o; o += NB * 12;    // per joint: G^R (9, row-major) | G^t (3)
  l.at = o; o += NB * 3;    // A^t = G^t - G^R J
  l.v = o; o += nv * 3;
  l.dv = l.v;
  o = (o + 1) & ~1;         // 8-byte alignment for the fp64 prefix sums (below)
  l.u = o;
  l.rot = l.u;
  const int nf = 12 * max_deg;
  l.fn = l.u; l.fg = l.fn + nf * 3; l.scr = l.fg + nf * 6;
  const int sz1 = nf * 9 + 12 * 9;
  const int pd_floats = (NB + 1) * 12 * 2;             // [23][12] doubles, aliases the chunk partial sums
  const int part_size = n_chunks * 12 > pd_floats ? n_chunks * 12 : pd_floats;
  l.part = l.u; l.pd = l.u; l.m = l.part + part_size; l.x = l.m;
  const int sz2 = part_size + NB * 12;
  int sz = sz1 > sz2 ? sz1 : sz2;
  sz = sz > NB * 9 ? sz : NB * 9;
  o += sz;
  l.total = (o + 3) & ~3;
  return l;
}


// Word offsets into the packed table blob that chain_sensors_kernel stages into LDS (all entries are 32-bit).
struct ChainTabs {
  int path_mask, sub_mask, parents;       // [22] each: ancestors-or-self mask, subtree mask, parent index
  int dfs_pos, sub_size;                  // [22] each: position of a joint in depth-first pre-order, size of its subtree
  int skin_idx, skin_w;                   // [nv*kb]
  int chunk_bone, chunk_beg;              // [n_chunks]: CHAIN_CHUNK-pair slices of the per-bone (vertex, weight) lists
  int bone_chunk_ptr;                     // [23]
  int bone_vert, bone_w;                  // [nnz]
  int s_center, s_helper, s_deg, s_faces; // [12], [12], [12], [12*max_deg*3]
  int inc_ptr, inc_code;                  // [nv+1], [n_inc]: per vertex, what contributes to its cotangent
  int total;
};

struct SmplTables {  // device pointers
  int n_sensors, nv, j_off, ncp, kb, max_deg;
  int n_chunks;
  const uint32_t* blob;
  ChainTabs off;

  const float* wc; const float* wct;
  const int* parents;
  const int* skin_idx; const float* skin_w;
  const int* bone_ptr; const int* bone_vert; const float* bone_w;
  const int* s_center; const int* s_helper; const int* s_deg; const int* s_faces;
  const int* path_ptr; const int* path; const int* sub_ptr; const int* sub;
};

// Pack the network input columns and the per-frame loss weight.
struct PackArgs {
  const float* marker_pos; const float* marker_oris;  // [T][36], [T][108]
  const float* marker_masks;                           // [T][12] or nullptr
  const int* seq_lengths;                              // [B] or nullptr
  float* x; int ldx;                                   // cols [0, 12*n_markers)
  float* frame_scale;                                  // [T]
  int B, F, n_markers;
  int marker_idx[12];
  int rows_as_unpadded = 0;   // 1: a ragged row counts as an unpadded window of its own length
  int suppress_missing = 0;   // 1: readings of sensors whose mask is not 1 are replaced by mask_value (the
  float mask_value = 0.f;     //    arithmetic of reference data/data.py:284-302: x * valid + mask_value * !valid)
};
hipError_t launch_pack_inputs(const PackArgs& a, hipStream_t stream);

// theta/beta update (+ window mean of the shape), Rodrigues and the GEMM feature row.
struct FeatArgs {
  float* theta; int ld_theta;          // [T][>=66] updated in place
  float* beta; int ld_beta;            // [T][>=10] updated in place
  const float* d_theta;                // [T][66] or nullptr
  const float* d_beta;                 // [T][10] or nullptr
  float theta_step;                    // theta += theta_step * d_theta
  float beta_keep, beta_step;          // beta = beta_keep * beta + beta_step * (shape_avg ? mean_F(d_beta) : d_beta)
  int shape_avg;                       // 0 none, 1 mean over all F frames, 2 mean over the valid frames
  const int* seq_lengths = nullptr;    // [T/F], only read when shape_avg == 2
  float* rot;                          // [T][22][9]
  float* feat;                         // [T][200]
  float* out_theta; float* out_beta;   // optional dense copies [T][66], [T][10]
  float* out_theta2; float* out_beta2; // optional second copy (history)
  float* theta_t = nullptr;            // optional: the updated theta in tile layout [tiles][66][64] (smpl_tile.hip)
  int T, F;
  int rod_conv = 0;                    // EMPOSE_RODRIGUES_SMPLX (0) or EMPOSE_RODRIGUES_SO3 (1)
};
hipError_t launch_update_feat(const FeatArgs& a, hipStream_t stream);

struct ChainArgs {
  SmplTables tab;
  const float* rot;        // [T][22][9]
  const float* out;        // [T][ncp] = feat . wc^T
  const float* offset_r;   // [T/F][12][9]
  const float* offset_t;   // [T/F][12][3]
  const float* tgt; int ld_tgt;   // network-input layout; nullptr => forward only
  const float* frame_scale;       // [T]
  int n_markers; int used_slot[12];  // used_slot[m] = column slot of virtual sensor m in tgt, or -1
  float* pos; float* ori; float* joints;   // [T][36], [T][108], [T][66]
  float* pos2; float* ori2; float* joints2;  // optional second copies
  float* d_out;            // [T][ncp]
  float* d_rot;            // [T][22][9]
  int T, F;
  const float* cot_pos = nullptr;    // [T][36]  external cotangents (vector-Jacobian product for training);
  const float* cot_ori = nullptr;    // [T][108] when set they replace the residual of `tgt`
  const float* cot_joints = nullptr; // [T][66]  optional
};
size_t chain_lds_bytes(const SmplTables& tab, int frames_per_block);
hipError_t launch_chain_sensors(const ChainArgs& a, hipStream_t stream);


struct RodBwdArgs {
  const float* theta; int ld_theta;
  const float* d_rot;      // [T][22][9]
  const float* d_feat;     // [T][200]
  float* g_theta; int ld_g;
  float* g_beta; int ld_gb;
  float* trace_g_theta; float* trace_g_beta;  // optional dense copies
  int T;
  int rod_conv = 0;
};
hipError_t launch_rodrigues_bwd(const RodBwdArgs& a, hipStream_t stream);

// ---------------------------------------------------------------------------------------------------------------
// SMPL sub-mesh with one frame per lane (smpl_tile.hip): tables, arguments, launchers.
// "Tile layout" of a per-frame matrix X[T][C]: X_t[tile = t / 64][c][t % 64] -- a column of 64 frames is contiguous.
// ---------------------------------------------------------------------------------------------------------------
constexpr int TL_FR = 64;             // frames per tile = lanes of a wave
constexpr int ROD_BWD_LD = 77;        // row stride of rodrigues_bwd_tile's staging block [TL_FR][77] (66 g_theta | 10 g_beta | pad)
constexpr int TL_NR = 8;              // largest ring (= sensor vertex degree) the kernel takes
constexpr int TL_NLOC = TL_NR + 1;    // local vertices of a sensor patch: centre + ring
constexpr int TL_NBL = 8;              // distinct bones under one patch
struct TileSensor {
  int deg, helper, col, nb;           // ring size, ring index of the helper vertex, first column of the patch, bones
  int bone[TL_NBL];                   // the patch's bones (unused slots: bone 0 with zero weights)
  int bones, pad[3];                  // bit mask of the bones (host: scheduling)
  float w[TL_NLOC][TL_NBL];           // dense skin weights of local vertex i over the patch's bones
};
struct TileTables {                   // one per model, in device memory, read with scalar loads
  int ncp2, j_off2, nloc, nbl;        // columns of the tile (multiple of 32), first rest-joint column, most local
                                      // vertices / bones of a patch
  int n_rounds;
  TileSensor s[12];
  int parent[22];
};
bool build_tile_tables(int nv, int kb, int max_deg, int j_off, const float* wc, const int* parents, const int* skin_idx,
                       const float* skin_w, const int* s_center, const int* s_helper, const int* s_deg,
                       const int* s_faces, TileTables* out, std::vector<float>* wc2);
struct TileArgs {
  const TileTables* tab;
  const float* theta; int ld_theta;   // [T][ld] axis-angles (66 used)
  const float* theta_t = nullptr;     // the same in tile layout [tiles][66][64], or nullptr (strided loads: 64 cache
                                      // lines per load instruction)
  const float* tgt_t = nullptr;       // tgt in tile layout [tiles][12 * n_markers][64], or nullptr
  const float* out_t;                 // tile layout [tiles][ncp2][64]: v_posed of the patches | rest joints
  const float* offset_r;              // [T/F][12][9]
  const float* offset_t;              // [T/F][12][3]
  const float* tgt; int ld_tgt;       // network-input layout; nullptr with backward => external cotangents
  const float* frame_scale;           // [T]
  int n_markers; int used_slot[12];
  float* pos; float* ori; float* joints;       // [T][36], [T][108], [T][66] or nullptr (not wanted)
  float* pos2; float* ori2; float* joints2;    // optional second copies
  float* d_out_t;                     // tile layout [tiles][ncp2][64]
  float* d_rot_t;                     // tile layout [tiles][198][64]
  int T, F;
  int rod_conv;
  const float* cot_pos = nullptr;     // [T][36], [T][108]: external cotangents instead of the residual
  const float* cot_ori = nullptr;
};
// `chain_only` (forward, no sensor outputs asked for): Rodrigues + chain and the joint stores alone; reads only the
// rest-joint columns of out_t
hipError_t launch_smpl_tile(const TileArgs& a, bool backward, int nloc, int nbl, hipStream_t stream, bool chain_only = false);
struct RodBwdTArgs {
  const float* theta; int ld_theta;
  const float* theta_t = nullptr;     // optional: the same values in tile layout [tiles][66][64] (coalesced loads)
  const float* d_rot_t;               // tile layout [tiles][198][64]
  const float* d_feat_t; int ld_feat_t;   // tile layout [tiles][ld_feat_t][64] (columns 0..198 used)
  float* g_theta; int ld_g; float* g_beta; int ld_gb;
  float* trace_g_theta; float* trace_g_beta;
  int T; int rod_conv;
};
hipError_t launch_rodrigues_bwd_t(const RodBwdTArgs& a, hipStream_t stream);
hipError_t launch_rows_to_tile(const float* src, int ld, int cols, float* dst_t, int T, hipStream_t stream);
// C = A . Wp^T with tile-layout operands (mlp_fused.hip): A row-major [M][lda] or tile layout (a_tile), C in tile layout
// [tiles][ldc_t][64] (ldc_t == N rounded up to 32; the padding columns are written as zeros).
hipError_t launch_gemm_rows_t(const float* A, int lda, bool a_tile, const float* Wp, float* C_t, int ldc_t, int M, int N,
                              int K, hipStream_t stream);

// The same two products with the small kernels around them folded in (mlp_fused.hip): the pose / shape update +
// feature row as the prologue of the first (the [T][200] feature matrix never reaches HBM), the Rodrigues reverse as
// the epilogue of the second (neither do the feature cotangents).
// x3: Wp = three bf16 pieces per weight in bf16-MFMA fragment order (pack_fragments_x3_raw), product on the bf16 matrix path
// [col_lo, col_hi): compute and write only the 32-column tiles of C_t that cover these columns (same bits there as the
// full product); the default is every column
hipError_t launch_blend_feat_gemm(const FeatArgs& fa, const float* Wp, float* C_t, int ldc_t, int N, bool x3,
                                  hipStream_t stream, int col_lo = 0, int col_hi = 0);
hipError_t launch_blend_t_gemm_rod(const float* A_t, int lda_t, const float* Wp, int K, const RodBwdTArgs& ra, bool x3,
                                   hipStream_t stream);

// The two init heads on the LSTM output as one product over their stacked columns (mlp_fused.hip): Wp = the stacked weight
// [n_pose + n_shape][K] in fragment order, bias stacked likewise.
bool heads_rows_applicable(int M, int K);
hipError_t launch_heads_rows(const float* y, int ldy, const float* Wp, const float* bias, float* theta, int ld_theta,
                             float* shape, int ld_shape, int M, int K, int n_pose, int n_shape, bool x3, hipStream_t stream);

// Full-mesh: chain only (joints + relative transforms) and dense skinning.
constexpr int MESH_MAX_JOINTS = 52;   // SMPL-H: 22 body + 2 x 15 hand joints
struct MeshChainArgs {
  const float* rot; const float* out; int ncp; int j_off;   // out: rest joints [T][ncp], n_joints * 3 used from j_off
  const int* parents;      // [n_joints], topologically ordered
  const float* trans;      // [T][3] or nullptr
  float* xf;               // [T][22][3][4]: per body bone and row (G^R[r][0..2], A^t[r])
  float* joints;           // [T][n_joints][3]
  int T;
  int n_joints = NB;       // 22 (body) or up to MESH_MAX_JOINTS (hand joints ride on their parents, zero hand pose)
};
hipError_t launch_mesh_chain(const MeshChainArgs& a, hipStream_t stream);
struct MeshSkinArgs {
  const float* feat;           // [T][200]
  const float* wc;             // [V*3 (+66)][200]: row 3s+c = coefficients of coordinate c of vertex s
  const float* xf;             // [T][22][3][4]: row r of bone b = (G^R[r][0..2], A^t[r])
  const int* skin_idx; const float* skin_w; int kb;
  const float* trans;
  float* vertices;             // [T][V][3]
  int T, V;
  const float* wc_frag;        // [tiles][25][3][64][4]: wc in fragment order per 32-vertex tile (api_mesh.hip pack_mesh_tiles)
  const int* skin_idx4; const float* skin_w4;   // [tiles * 32][4]
  const void* wc_bf16 = nullptr;   // bf16 pieces of wc in fragment order per tile (api_mesh.hip pack_mesh_tiles_bf16), or nullptr
  const void* skin_bf16 = nullptr; // dense skin weights per 32-vertex tile as bf16 pieces in fragment order (pack_mesh_skin_bf16)
  const void* wc_x3 = nullptr;     // THREE bf16 pieces of wc in fragment order per tile (api_mesh.hip pack_mesh_tiles_x3)
  int stagger = 1;                 // mesh_rows_x3_kernel: a tile's stores ride in the next tile's K loop, at a per-wave k-step
};
hipError_t launch_mesh_rows(const MeshSkinArgs& a, hipStream_t stream);
// The same evaluation with the blend-shape contraction in split bf16 (mesh_bf16.hip); needs MeshSkinArgs::wc_bf16.
hipError_t launch_mesh_rows_bf16(const MeshSkinArgs& a, hipStream_t stream);
constexpr int MESH_BF16_TILE_BYTES = 14 * 3 * 2 * 1024;
// ... and with the bone blend as a second contraction on the matrix cores (needs MeshSkinArgs::skin_bf16 too).
hipError_t launch_mesh_rows_bf16s(const MeshSkinArgs& a, hipStream_t stream);
constexpr int MESH_SKIN_BF16_TILE_BYTES = 2 * 2 * 1024;
// The blend-shape contraction on three bf16 pieces per operand -- fp32-equivalent, the default arithmetic of the full-mesh
// evaluation since round 6 (mesh_x3.hip; option mesh_x3: 1 = products, skinning, stores one after the other with the stores
// staggered into the next tile's K loop, 2 = the same with the stores at the end of their tile, 3 = the skinning
// software-pipelined under the next tile's K loop (measured no faster), 0 = the fp32 MFMA kernel).  Four bones per vertex
// (kb <= 4); needs MeshSkinArgs::wc_x3.
hipError_t launch_mesh_rows_x3(const MeshSkinArgs& a, bool overlap, hipStream_t stream);
constexpr int MESH_X3_TILE_BYTES = 13 * 9 * 1024;

// Per-vertex error between two bodies (mesh_err.hip): both bodies of a frame are evaluated in the same lanes on the fp32
// MFMA instruction and only their distances are kept -- part [T][tiles][2] = the sums of |v_A - v_B| and of its square
// over the 32 vertices of a tile (vertices past V count as an exact 0), tiles = ceil(V / 32).  launch_mesh_err_sum adds a
// frame's partials in ascending tile order in double: out [T][2].  Fixed-order sums only; a frame's result depends on
// nothing but that frame.
struct MeshPairErrorArgs {
  const float *feat_a, *xf_a, *trans_a;   // body A: [T][200], [T][22][3][4], [T][3] or nullptr
  const float *feat_b, *xf_b, *trans_b;   // body B likewise
  const int* skin_idx; const float* skin_w; int kb;
  int T, V;
  const float* wc_frag;                   // as MeshSkinArgs
  const int* skin_idx4; const float* skin_w4;
  float* part;
};
hipError_t launch_mesh_pair_error(const MeshPairErrorArgs& a, hipStream_t stream);
hipError_t launch_mesh_err_sum(const float* part, int n_tiles, int T, double* out, hipStream_t stream);

// Full-mesh vector-Jacobian product (mesh_vjp.hip): the two vertex sweeps of the reverse for a cotangent dV [T][V][3].
//   feat sweep: d_feat[t][k] = sum_v,c dvp[t][v][c] wc[3v+c][k], dvp_v = sum_b w_vb (A_b^R)^T dV_v   -> out [T][200]
//   bone sweep: dA_b[t][r][c] = sum_v w_vb dV_v[r] [vp_v; 1][c]                                       -> out [T][22][12]
//   the feat sweep also sums dV over the vertices in double precision (the translation's cotangent)   -> dtrans
// Deterministic: fixed-order sums only.  With mesh_vjp_split(..) > 1 the vertex tiles are split over grid.y and the
// partials ([split][T][cols] in `part`) are summed in slot order by a second launch.
constexpr int MESH_VJP_BM = 32;            // frames per workgroup of both sweeps
constexpr int MESH_VJP_DA = NB * 12;       // bone-sweep output columns per frame
constexpr int MESH_VJP_WC_TILE_FLOATS = 16 * 6 * 64 * 4;   // wc_vjp per 32-vertex tile: [16 vertex pairs][6][64 lanes][4]
constexpr int MESH_VJP_SKIN_TILE_FLOATS = 4 * 64 * 4;      // skin_dense per tile: [4][64 lanes][4]
struct MeshVjpArgs {
  const float* feat;           // [T][200]
  const float* xf;             // [T][22][3][4] (mesh_chain_kernel)
  const float* dv;             // [T][V][3]
  const float* wc_frag;        // forward fragment order (MeshSkinArgs::wc_frag), bone sweep
  const float* wc_vjp;         // vertex rows of wc in the feat sweep's B-fragment order (api_mesh.hip pack_mesh_vjp)
  const float* skin_dense;     // dense bone weights per tile in the bone sweep's B-fragment order (ditto)
  const int* skin_idx4; const float* skin_w4;   // [tiles * 32][4]
  const int* skin_idx; const float* skin_w; int kb;
  float* out;                  // [T][200] (feat sweep) or [T][MESH_VJP_DA] (bone sweep)
  float* part;                 // [split][T][cols] scratch when the sweep is split over grid.y
  double* dtrans;              // feat sweep: [split][T][3], sum_v dV_v over the slice's vertices
  int T, V;
};
int mesh_vjp_feat_split(int T, int V);
int mesh_vjp_bone_split(int T, int V);
hipError_t launch_mesh_vjp_feat(const MeshVjpArgs& a, hipStream_t stream);
hipError_t launch_mesh_vjp_bone(const MeshVjpArgs& a, hipStream_t stream);
// Reverse kinematic chain (mesh_chain.hip, beside mesh_chain_kernel): one thread per frame recomputes the 22 global rotations
// and takes dA (bone sweep) and the joint cotangents back to d_rot, the rest-joint cotangents and d_trans.
struct MeshChainBwdArgs {
  const float* rot;            // [T][22][9]
  const float* jrest; int ld_j;    // rest joints [T][ld_j], n_joints * 3 used
  const int* parents;          // [n_joints]
  const float* dA;             // [T][MESH_VJP_DA] or nullptr
  const float* dJ;             // [T][n_joints][3] or nullptr
  const double* dtrans; int n_slices;   // [n_slices][T][3] (feat sweep) or nullptr
  float* d_rot;                // [T][22][9]
  float* d_jrest; int ld_dj;   // [T][ld_dj]; columns past n_joints * 3 are written as zeros
  float* g_trans;              // [T][3] or nullptr
  int T, n_joints;
};
hipError_t launch_mesh_chain_bwd(const MeshChainBwdArgs& a, hipStream_t stream);

struct VirtualSensorArgs {
  const float* vertices;   // [T][V][3]
  const int* center; const int* helper; const int* deg; const int* faces;  // [M], [M], [M], [M][max_deg][3] (mesh ids)
  float* pos; float* ori; float* normals;   // [T][M][3], [T][M][9], [T][M][3] (un-normalised) or nullptr
  int T, V, M, max_deg;
};
hipError_t launch_virtual_sensors(const VirtualSensorArgs& a, hipStream_t stream);
// Vector-Jacobian product of virtual_sensors_kernel (sensors_vjp.hip) for one slab of T frames: a sensor pass writes
// SENSOR_VJP_ROW floats per (frame, sensor) to `scratch` (dn / deg, the center's and the helper's cotangents), a vertex
// pass writes every element of d_vertices.  Reverse tables (api: empose_virtual_sensors_vjp): sub_faces [Fs][3],
// face_ptr [Fs + 1] / face_sensors (ascending), vf_ptr [V + 1] / vf_corner (f * 3 + k, ascending f), vs_ptr [V + 1] /
// vs_role (m * 2 + role, role 0 center, 1 helper, ascending), touched [n_touched].
constexpr int SENSOR_VJP_ROW = 9;
struct SensorVjpArgs {
  const float* vertices;   // [T][V][3]
  const int* center; const int* helper; const int* deg; const int* faces;   // the forward's tables
  const int* sub_faces; const int* face_ptr; const int* face_sensors;
  const int* vf_ptr; const int* vf_corner; const int* vs_ptr; const int* vs_role;
  const int* touched; int n_touched;   // the vertices with entries in vf / vs, ascending
  const float* d_pos; const float* d_ori; const float* d_normals;   // [T][M][3], [T][M][9], [T][M][3], each or nullptr
  float* scratch;          // [T][M][SENSOR_VJP_ROW]
  float* d_vertices;       // [T][V][3]
  int T, V, M, max_deg;
};
hipError_t launch_sensors_vjp(const SensorVjpArgs& a, hipStream_t stream);

// Synthetic sensor sampling (sensor_sample.hip): the frames of virtual_sensors_kernel plus the per-subject offsets,
// pos_synth = pos + ori . local, ori_synth = ori . r, in one launch; and the fold of the reverse, which turns the
// cotangents of the six outputs into those of (pos, ori) for launch_sensors_vjp.
constexpr int SAMPLE_LOCAL_NONE = 0;     // EMPOSE_SAMPLE_LOCAL_* (include/empose_hip.h)
constexpr int SAMPLE_LOCAL_WINDOW = 1;   // local [N][M][3]
constexpr int SAMPLE_LOCAL_FRAME = 2;    // local [N * F][M][3]
struct SampleSensorsArgs {
  const float* vertices;   // [T][V][3], T = N * F
  const int* center; const int* helper; const int* deg; const int* faces;   // as VirtualSensorArgs
  const float* local;      // by mode, or nullptr (SAMPLE_LOCAL_NONE)
  const float* r;          // [N][M][3][3] or nullptr (identity)
  float* pos; float* ori; float* normals;                   // [T][M][3], [T][M][9], [T][M][3], each or nullptr
  float* pos_synth; float* ori_synth; float* normal_synth;  // likewise
  int T, F, V, M, max_deg, mode;
};
hipError_t launch_sample_sensors(const SampleSensorsArgs& a, hipStream_t stream);
// One slab of T frames whose first frame is frame t0 of the batch (t0 selects the window of local and r); the pointers
// of the cotangents and of the outputs start at the slab.  d_pos_out is written when d_pos or d_pos_synth is given,
// d_ori_out when any of d_ori, d_ori_synth, d_normal_synth or (mode != NONE and d_pos_synth) is.
struct SampleFoldArgs {
  const float* d_pos; const float* d_ori;                                        // un-offset outputs, each or nullptr
  const float* d_pos_synth; const float* d_ori_synth; const float* d_normal_synth;   // each or nullptr
  const float* local; const float* r;   // whole batch, as SampleSensorsArgs
  float* d_pos_out; float* d_ori_out;   // [T][M][3], [T][M][9], each or nullptr
  int T, t0, F, M, mode;
};
hipError_t launch_sample_fold(const SampleFoldArgs& a, hipStream_t stream);

// Root normalisation and its vector-Jacobian product (root_frame.hip).  T frames in segments of seg_len rows; the root
// axis-angles are the first three columns of rows of ld_root floats.  `flags`: what happens to the translation.
constexpr int ROOT_FRAME_ROTATE = 1;     // trans_out = R_0^T trans
constexpr int ROOT_FRAME_SUBTRACT = 2;   // ... minus the first frame's (rotated) translation
constexpr int ROOT_FRAME_SUMS = 9;       // floats per wave of the reverse in `part`
struct RootFrameArgs {
  const float* root; int ld_root;
  const float* trans;                              // [T][3], read when flags != 0
  float* root_out; float* trans_out;               // forward: [T][3], [T][3] (flags != 0)
  const float* d_root_out; const float* d_trans_out;   // reverse: [T][3] each or nullptr
  float* g_root; float* g_trans;                   // reverse: [T][3]; g_trans is written when d_trans_out is given
  float* part;                                     // reverse: [root_frame_vjp_waves(T, seg_len)][ROOT_FRAME_SUMS]
  int T, seg_len, rod_conv, flags;
};
long root_frame_vjp_waves(int T, int seg_len);
hipError_t launch_root_frame_fwd(const RootFrameArgs& a, hipStream_t stream);
hipError_t launch_root_frame_vjp(const RootFrameArgs& a, hipStream_t stream);

// Resampling of a ragged batch of sequences to another frame rate (resample.hip).  One entry per sequence; the layout is
// that of empose_resample_seq (include/empose_hip.h).  Output rows are packed: out_row[s + 1] = out_row[s] + f_out[s].
struct ResampleSeq {
  int in_row, f_in, out_row, f_out;
  double fps_in, fps_out;
};
struct ResampleArgs {
  const ResampleSeq* seqs; int S;   // device table
  const float* in; int ld_in;       // rows of ld_in floats; the first 3 * n (rotations) or n (positions) columns are read
  float* out; int ld_out;
  int n;                            // joints per row (rotations) or channels (positions)
  long out_rows;                    // sum of f_out
  double* ws;                       // positions: [input rows][n] spline derivatives
};
hipError_t launch_resample_rotations(const ResampleArgs& a, hipStream_t stream);
hipError_t launch_resample_positions(const ResampleArgs& a, hipStream_t stream);

// Sensor-noise augmentation (sensor_noise.hip): one launch writes the noisy copies of [N][F][M * 3] positions and, when
// suppressing, [N][F][M * 9] orientations and [N][F][M * 3] normals, from a plan in device memory.
constexpr int SENSOR_NOISE_SPHERICAL = 0;   // EMPOSE_SENSOR_NOISE_* (include/empose_hip.h)
constexpr int SENSOR_NOISE_SUPPRESS = 1;
struct SensorNoiseArgs {
  const float* pos; const float* ori; const float* normal;   // ori, normal: suppression only
  float* pos_out; float* ori_out; float* normal_out;
  const int* start;                                // [N] first affected frame of a window
  const int* sensor;                               // suppression: [N][K], spherical: [K]
  const float* u_r; const float* theta; const float* phi;   // spherical: [N][window_len][K]
  int N, F, M, K, window_len, mode, thigh_a, thigh_b;
  float max_r, mask_value;
};
hipError_t launch_sensor_noise(const SensorNoiseArgs& a, hipStream_t stream);

// Per-subject sensor offsets from calibration recordings (offset_stats.hip): the inverse of launch_sample_sensors.  Per
// frame f and sensor m, with (pos, ori) the frame of sensor_frame.h on the ground-truth mesh and (p, R) the real reading,
//   o = ori^T (p - pos),   Q = ori^T R,
// and per (group, sensor) over the group's frames with mask == 1: the mean and the sample covariance of o, and the
// rotation closest to the mean of Q.  A group is a run of consecutive frames; the layout of a row is that of
// empose_offset_group (include/empose_hip.h).
constexpr int OFFSET_STATS_CHUNK = 256;   // frames per workgroup of the first pass, counted from the group's first frame
constexpr int OFFSET_STATS_SUMS = 19;     // count | sum o (3) | sum o o^T xx xy xz yy yz zz | sum Q (9)
struct OffsetGroup {
  int first_frame, n_frames;
};
struct OffsetStatsArgs {
  const float* vertices;   // [T][V][3]
  const int* center; const int* helper; const int* deg; const int* faces;   // as VirtualSensorArgs
  const float* p; const float* R;   // [T][M][3], [T][M][9]
  const float* masks;               // [T][M] or nullptr (every frame counts)
  const OffsetGroup* groups; int G; // device table
  double* sums;                     // [n_chunks][M][OFFSET_STATS_SUMS], a group's chunks after those of the groups before it
  float* local_f; float* q_f;       // [T][M][3], [T][M][9] or nullptr; written for the frames of the groups only
  float* means; float* covs; float* r; float* r_trace; int* counts;   // [G][M][3], [G][M][9], [G][M][9], [G][M], [G][M]
  int T, V, M, max_deg;
  int n_chunks;                     // sum over the groups of ceil(n_frames / OFFSET_STATS_CHUNK)
};
hipError_t launch_offset_stats(const OffsetStatsArgs& a, hipStream_t stream);

struct MetricsArgs {
  const float* joints_gt; const float* joints_hat;   // [T][22][3]
  const float* pose_gt; const float* pose_hat;       // [T][63] body axis-angles (no root) or nullptr
  double* rows;                                      // [T][65] = 22 distances | 22 aligned distances | 21 angles (deg)
  int parents[22];
  int T;
};
hipError_t launch_metrics_rows(const MetricsArgs& a, hipStream_t stream);

// Model-free sensor fitting (sensor_fit.hip): first-order descent on the sensor residual plus priors, per window w
//   J_w = sum_t s_t E_t + lambda_pose / 2 sum_{t live} |theta_t[3:66] - p_t[3:66]|^2 + lambda_shape / 2 |beta_w|^2
//         + lambda_smooth / 2 sum_{t >= 1, live} |theta_t - theta_{t-1}|^2        
// What the three kernels share: the window batch, the readings and the weights of the terms.
struct FitProblem {
  const float* tgt; int ld_tgt;     // [T][ld_tgt]: n_markers * 3 positions, then n_markers * 9 orientations
  const float* s;                   // [T] frame weight of the data term (0 or 1)
  const int* seq_lengths;           // [B] or nullptr (= F everywhere)
  const float* prior;               // [T][66] or nullptr (zeros)
  int B, F, n_markers;
  int used_slot[12];                // sensor -> slot in a target row, -1: not read by the model
  float lambda_pose, lambda_shape, lambda_smooth;
  int shape_per_window;             // 1: one shape per window (every row of a window holds it), 0: one per frame
};
struct FitPrepareArgs {
  FitProblem p;
  const float* marker_masks;        // [T][12] or nullptr
  const float* pose_init; const float* shape_init;   // [T][66], [T][10] or nullptr (zeros)
  float* theta; float* beta;        // [T][66], [T][10]: the iterate 0
  float* moments; size_t n_moments; // zeroed
  float* s;                         // [T] written
  float* best_J;                    // [B] = +inf
};
struct FitStepArgs {
  FitProblem p;
  const float* theta; const float* beta;       // iterate k
  const float* g_theta; const float* g_beta;   // [T][66], [T][10] gradient of sum_t s_t E_t at iterate k
  const float* pos; const float* ori;          // [T][36], [T][108] sensors of iterate k
  float* m_theta; float* v_theta;              // [T][66] Adam moments, updated in place (live frames)
  float* m_beta; float* v_beta;                // [T][10]; one shape per window: the window's first row only
  float* theta_next; float* beta_next;         // iterate k + 1 (never the buffers of iterate k)
  float* energy;                               // [T] s_t E_t or nullptr
  float* J;                                    // [B] J_w at iterate k
  float* best_J; float* best_theta; float* best_beta;   // keep-best ([B], [T][66], [T][10]) or nullptr
  float lr_k, c1, c2, beta1, beta2, eps;       // lr decay^k, 1 / (1 - beta1^(k+1)), 1 / (1 - beta2^(k+1)): rounded by the host
};
struct FitFinishArgs {
  FitProblem p;
  const float* theta; const float* beta;       // iterate K
  const float* pos; const float* ori;          // its sensors
  const float* best_J; const float* best_theta; const float* best_beta;   // or nullptr: the last iterate is returned
  float* pose; float* shape;                   // [T][66], [T][10] what is returned
  float* J_last; float* J_out;                 // [B] J_w of iterate K, and of what is returned
};
hipError_t launch_fit_prepare(const FitPrepareArgs& a, hipStream_t stream);
hipError_t launch_fit_step(const FitStepArgs& a, hipStream_t stream);
hipError_t launch_fit_finish(const FitFinishArgs& a, hipStream_t stream);
// energy[t] = s_t E_t of given sensors (the optional per-frame output of the fit)
hipError_t launch_fit_energy(const FitProblem& p, const float* pos, const float* ori, float* energy, hipStream_t stream);

}  // namespace empose
