/*
 * empose_hip.h -- C ABI of the MI355X (gfx950) implementation of EM-POSE's learned-gradient-descent fitting loop.
 *
 * The reference (facebookresearch/em-pose) has no FFI/operator layer for this path: it sits behind Python objects
 * (SURVEY.md 8b).  This header is the boundary the build introduces underneath those objects; every entry point
 * names the reference interface it replaces.  Conventions:
 *   - extern "C", plain C types only; every function returns 0 on success or a negative EMPOSE_E* code, and
 *     empose_last_error() returns a thread-local description.  No exception crosses the boundary.
 *   - All tensors are caller-owned DEVICE pointers, fp32, row-major contiguous unless a leading dimension is given;
 *     index data is int32.  Model descriptors (empose_*_desc) hold HOST pointers and are consumed at create time.
 *   - Every compute call takes a stream handle (a hipStream_t passed as void*; NULL = default stream), is
 *     asynchronous and stream-ordered, and never allocates: scratch comes from the caller via
 *     empose_lgd_workspace_bytes().  A model is immutable after creation, so concurrent calls on distinct streams
 *     with distinct workspaces are safe.
 */
#ifndef EMPOSE_HIP_H_
#define EMPOSE_HIP_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EMPOSE_OK 0
#define EMPOSE_EINVAL (-1)   /* bad argument / unsupported configuration */
#define EMPOSE_EHIP (-2)     /* a HIP runtime call failed */
#define EMPOSE_ENOMEM (-3)   /* workspace too small / allocation failed */
#define EMPOSE_ETIMEOUT (-4) /* a cooperative kernel gave up waiting for another workgroup: outputs poisoned with NaN */

#define EMPOSE_N_BODY 22      /* root + 21 body joints, reference configuration.py:104 */
#define EMPOSE_N_SENSORS 12   /* virtual sensors always evaluated, reference models.py:383,538 */
#define EMPOSE_K_FEAT 200     /* 189 pose-feature + 10 shape + 1 */
#define EMPOSE_MAX_DENSE 8
#define EMPOSE_N_JOINTS_SMPLH 52  /* joints of `body.Jtr`, reference bodymodels/smpl.py:121-122 */

/* How the axis-angle -> rotation map guards the angle at r = 0.  The body-model arithmetic lives in an un-vendored
 * dependency (human_body_prior fork, reference requirements.txt:9), so the convention is a property of the model
 * handle instead of being baked into the kernels:
 *   SMPLX  angle = ||r + 1e-8||                (smplx lbs.batch_rodrigues; default)
 *   SO3    angle = sqrt(clamp(||r||^2, 1e-4))  (reference helpers/so3.py:116-121, so3_exponential_map) */
#define EMPOSE_RODRIGUES_SMPLX 0
#define EMPOSE_RODRIGUES_SO3 1

typedef void* empose_stream_t;
typedef struct empose_model empose_model_t;
typedef struct empose_mesh empose_mesh_t;
typedef struct empose_rnn empose_rnn_t;

const char* empose_last_error(void);
/* Library/ABI version and the offload architecture it was compiled for ("gfx950"). */
int empose_version(void);
const char* empose_arch(void);

/* Kernel-variant selection for A/B measurements and bit-identity tests: several paths have two implementations (the
 * one-launch fused update MLPs vs layer-by-layer GEMMs, whole-sequence LSTM kernels vs step launches, ...) that must
 * give the same results.  Options are process-wide ints, default 1 = the faster variant; the library never reads the
 * environment.  Names: "mlp_fused", "lstm_persist", "gemm_splitk", "gemm_wide", "atb_target", "atb_chunk",
 * "smpl_tile" (frame-per-lane SMPL sub-mesh kernels: 0 never, 1 from 16384 frames on [default], 2 always),
 * "smpl_fuse" (on that path: pose / shape update and Rodrigues reverse inside the blend GEMMs; 0 = own kernels),
 * "heads_rows" (both init heads as one row-block product from 4096 frames on; 0 = two problems on the generic tile),
 * "lstm_seq" (batches above 256 rows: the LSTM's whole sequence in one cooperative launch; 0 [default] = one launch per
 * wavefront step, which measured faster), "bptt_wave" (training: reverse LSTM recurrences of two layers as a wavefront),
 * "train_fused" (train-mode MLP layer with BatchNorm / PReLU folded into the GEMMs: 0 never [default], 1 above 1024
 * rows, 2 always), "train_epi" (train-mode MLP layer with the BatchNorm statistics in the GEMM epilogues and ONE
 * combine-and-apply launch per layer and direction: 0 never, 1 above 1024 rows [default], 2 always), "atb_fast" (weight
 * gradients: whole-tile / whole-chunk products on a branch-free interior kernel, bit-identical; 0 = the general kernel),
 * "mlp_x3" (the fused update MLPs form every fp32 product from three bf16 pieces per operand -- six bf16 matrix-core
 * products with fp32 accumulation, fp32-equivalent and 2.7 times the fp32 instruction's rate -- when every hidden width
 * is a multiple of 64: 1 [default]; 0 = the fp32 MFMA instruction; any other value is on, like 1), "lstm_x3" (the same arithmetic for the LSTM steps of batches above 256 rows, inference,
 * uni-directional stacks with a hidden size of whole 32s: 1 [default]; 0 = the fp32 MFMA instruction; 2 = a row-split
 * variant, measured slower; 3 = force the kernel on the 16x16x32 form of the bf16 instruction), "lstm_chain16" (those
 * steps with lstm_x3 = 1 on the 16x16x32 form of the bf16 instruction -- equal to the 32x32x16 form to rounding, not to the
 * bit; measured 3 to 6 % faster per launch: 1 [default]; 0 = the 32x32x16 form), "mlp_fused16" (the same choice for the
 * fused update MLPs with mlp_x3 != 0; measured 4 to 8 % faster per launch: 1 [default]; 0 = the 32x32x16 form), "mlp_pair16"
 * (the fused update MLPs with mlp_x3 != 0 and mlp_fused16 != 0 form every fp32 product from TWO f16 pieces per operand
 * under a power-of-two scale per activation row and per weight column -- three f16 matrix-core products instead of six
 * bf16 ones, as accurate against float64, equal to rounding and not to the bit; measured 17 % faster per launch:
 * 1 [default]; 0 = the three bf16 pieces), "lstm_pair16" (the same choice for the LSTM steps on the 16x16x32 form: the
 * hidden states the kernel itself produced, which lie in [-1, 1], go as two f16 pieces under the fixed scale 2^14; the raw
 * input of layer 0 and a caller's h0 stay on three bf16 pieces: 1 [default]; 0 = three bf16 pieces throughout), "rows_x3" (the
 * same arithmetic for the row-block products with fused prologue / epilogue: the blend products of the frame-per-lane
 * SMPL path and the stacked init heads; 0 = the fp32 MFMA instruction), "train_cols" (training at up to 512 rows: a
 * layer's product + BatchNorm + PReLU as one launch, forward and backward, both update networks side by side -- see
 * empose_mlp_train_fwd_pair; 0 = a product and a BatchNorm launch per layer and network), "lstm_fewrows" (LSTM steps of 4 to
 * 16 rows -- the reference's training batch, chunks of recordings -- as launches whose workgroups own two hidden units and
 * split K over all their threads; 0 = the whole-sequence kernel / the small-batch step kernel, which share their bits),
 * "mesh_skin_mfma" (split-bf16 full-mesh variant only: the bone blend as a second matrix-core contraction; 0 [default,
 * measured faster] = vector skinning), "spin_limit" (see empose_async_status), "last_pass_joints" (LGD forward on the
 * frame-per-lane path: an SMPL evaluation that is asked for joints only -- the last pass when no marker histories are
 * kept -- multiplies just the rest-joint column tiles of the blend matrix and runs the kinematic chain without the
 * sensors, bit-identical; 0 = the whole sub-mesh as in every other pass), "lstm_state_direct" (LSTM steps of batches above
 * 256 rows, new sequences [h0 = c0 = NULL]: the zero initial hidden-state planes by one fill and h_n / c_n stored by the
 * last step of each layer, bit-identical; 0 = a split launch and a fill per layer and 2 x layers trailing copies),
 * "lstm_skip_dead" (those LSTM steps with lstm_x3 = 1 or 3: work whose result nobody reads is left out, bit-identical --
 * the recurrent half of the first step of a new sequence, whose hidden state is zero, and without seq_lengths the fp32
 * copy of the hidden state that only rows past their length need; 0 = all of it runs).
 * empose_get_option returns -1 for an unknown name.  New in this library (no counterpart in the reference). */
int empose_set_option(const char* name, int value);
int empose_get_option(const char* name);
int empose_reset_options(void);   /* every option back to its default */

/* Launches are asynchronous, so a failure INSIDE a kernel cannot be the return value of the call that launched it.  The
 * one such failure this library has: the whole-sequence LSTM kernels (small batches: lstm_persist; opt-in lstm_seq) are
 * cooperative -- workgroups poll exchange words written by other workgroups -- and a poll that exceeds its spin limit
 * gives up, writes NaN from there on (it never hangs the GPU) and counts itself in a host-visible word.
 *   - every later empose_lstm_fwd / empose_rnn_fwd / empose_lgd_forward[_phase] call of the process returns
 *     EMPOSE_ETIMEOUT instead of running (count in empose_last_error()) -- STICKY, whichever model, stream or thread it
 *     belongs to -- until
 *   - empose_async_status() has returned EMPOSE_ETIMEOUT once (it reports and clears; EMPOSE_OK otherwise): call it after
 *     synchronising the stream, before trusting / averaging outputs (em_pose_amd.eval.helpers, bench.py and
 *     scripts/train.py do), and re-create the state the failed call carried (it is NaN).
 * Option "spin_limit" (> 0) forces the limit of those polls (tests).  The reference's forward has no counterpart (a
 * single Python thread, reference nn/layers.py:133-157). */
int empose_async_status(void);

/* ---- model description (host pointers) ------------------------------------------------------------------------ */

/* Packed SMPL-H constants for the sensor sub-mesh; produced by em_pose_amd/bodymodels/tables.py.
 * Replaces what the reference keeps as BodyModel buffers + VirtualMarkerHelper index caches
 * (reference bodymodels/smpl.py:42-67, data/virtual_sensors.py:47-75). */
typedef struct {
  int n_sensors;          /* 12 */
  int nv;                 /* needed vertices */
  int j_off;              /* column of the first rest-joint coordinate in `wc` rows */
  int ncp;                /* padded row count of wc (multiple of 4) */
  int kb;                 /* skinning weights per vertex (after folding the hands into the wrists) */
  int max_deg;            /* faces per sensor vertex (padded) */
  const float* wc;        /* [ncp][200] */
  const float* wct;       /* [200][ncp] */
  const int* parents;     /* [22] */
  const int* skin_idx;    /* [nv][kb] */
  const float* skin_w;    /* [nv][kb] */
  const int* bone_ptr;    /* [23] CSR over bones */
  const int* bone_vert;   /* [bone_ptr[22]] */
  const float* bone_w;    /* [bone_ptr[22]] */
  const int* s_center;    /* [12] local vertex of the sensor */
  const int* s_helper;    /* [12] local helper vertex */
  const int* s_deg;       /* [12] */
  const int* s_faces;     /* [12][max_deg][3] local vertex ids */
  const int* path_ptr;    /* [23] root->joint paths */
  const int* path;
  const int* sub_ptr;     /* [23] subtree member lists */
  const int* sub;
  int rodrigues;          /* EMPOSE_RODRIGUES_*: honoured by the forward, the residual gradient and the training VJP */
} empose_smpl_desc;

/* One Linear (+ BatchNorm1d in eval mode) (+ PReLU): reference nn/layers.py:13-43,46-77. weight is [out][in]. */
typedef struct {
  int in_dim, out_dim;
  const float* weight;
  const float* bias;
  const float* bn_weight; /* NULL => no batch norm */
  const float* bn_bias;
  const float* bn_mean;
  const float* bn_var;
  float bn_eps;
  int has_prelu;
  float prelu;            /* single shared slope, nn.PReLU() */
} empose_dense_desc;

/* reference nn/layers.py:46-77: layers[0]=input_to_hidden, then 2*num_blocks hidden layers, then hidden_to_output. */
typedef struct {
  int n_layers;           /* 2 + 2*num_blocks, <= EMPOSE_MAX_DENSE; 0 => MLP absent */
  int skip;               /* m_skip_connections: residual around every 2-layer block */
  empose_dense_desc layers[EMPOSE_MAX_DENSE];
} empose_mlp_desc;

/* reference nn/layers.py:114 (nn.LSTM, unidirectional, gate order i,f,g,o). */
typedef struct {
  int num_layers;         /* <= 4; 0 => absent */
  int input_size, hidden_size;
  const float* w_ih[4];   /* [4H][in] */
  const float* w_hh[4];   /* [4H][H] */
  const float* b_ih[4];
  const float* b_hh[4];
} empose_lstm_desc;

/* reference nn/models.py:372-394,424-457 (IterativeErrorFeedback.__init__/create_model). */
typedef struct {
  empose_smpl_desc smpl;
  int n_markers;          /* 6 or 12: sensors fed to the networks */
  int marker_idx[12];     /* first n_markers entries: which of the 12 virtual sensors they are (S_CONFIG_6) */
  int n_iterations;       /* N */
  float step_size;
  int shape_avg;          /* 0 off; 1 mean over all F frames incl. padding (reference models.py:529-532);
                             2 ragged rows behave as unpadded windows of their own length: shape mean over the
                               valid frames and residual weight 1 instead of F/len (batched streaming evaluation) */
  int use_gradient;
  int rnn_init;
  empose_lstm_desc rnn;           /* rnn_init */
  empose_dense_desc pose_head;    /* rnn_init: Linear(H,66) */
  empose_dense_desc shape_head;   /* rnn_init: Linear(H,10) */
  empose_mlp_desc pose_init;      /* !rnn_init */
  empose_mlp_desc shape_init;
  empose_mlp_desc pose_iter;
  empose_mlp_desc shape_iter;
} empose_model_desc;

/* Replaces IterativeErrorFeedback construction + load_state_dict (reference models.py:23-33, eval/helpers.py:131-137):
 * copies and packs every constant to the current HIP device. */
int empose_model_create(const empose_model_desc* desc, empose_model_t** out);
void empose_model_destroy(empose_model_t* model);

/* ---- the whole N-step loop ------------------------------------------------------------------------------------ */

/* Inputs are what `batch.get_inputs()` yields (reference data/data.py:304-309,433-459). */
typedef struct {
  int B, F;                      /* windows x frames; T = B*F */
  const float* marker_pos;       /* [B][F][12*3] */
  const float* marker_oris;      /* [B][F][12*9] row-major 3x3 */
  const float* offset_t;         /* [B][12][3] */
  const float* offset_r;         /* [B][12][3][3] */
  const float* marker_masks;     /* [B][F][12] 1=present, or NULL */
  const int* seq_lengths;        /* [B] or NULL (= F everywhere) */
  const float* h0;               /* [L][B][H] carried LSTM state or NULL (zeros): reference layers.py:149-150 */
  const float* c0;
  float* h_n;                    /* [L][B][H] out, may be NULL */
  float* c_n;
  /* outputs (reference models.py:602-609,631): pose_hat holds root+body (66); callers slice [..., :3] / [..., 3:] */
  float* pose_hat;               /* [B][F][66] */
  float* shape_hat;              /* [B][F][10] */
  float* joints_hat;             /* [B][F][66] */
  /* optional histories, N+1 entries each (reference models.py:620-629); NULL to skip */
  float* hist_pose;              /* [N+1][T][66] */
  float* hist_shape;             /* [N+1][T][10] */
  float* hist_joints;            /* [N+1][T][66] */
  float* hist_markers;           /* [N+1][T][12*3] */
  float* hist_markers_ori;       /* [N+1][T][12*9] */
  /* optional trace of the gradient features fed to the update nets (reference models.py:578-582); NULL to skip */
  float* trace_g_pose;           /* [N][T][66] */
  float* trace_g_shape;          /* [N][T][10] */
  /* RealBatch.get_inputs replaces the readings of missing sensors by a constant before the model sees them
   * (reference data/data.py:284-302,304-309).  suppress_missing != 0: marker_pos / marker_oris are the RAW readings
   * and the packing kernel does that replacement (x * valid + mask_value * !valid with valid = mask == 1). */
  int suppress_missing;
  float mask_value;
} empose_lgd_io;

size_t empose_lgd_workspace_bytes(const empose_model_t* model, int B, int F);

/* Replaces IterativeErrorFeedback.forward for one window batch (reference models.py:485-632). */
int empose_lgd_forward(const empose_model_t* model, const empose_lgd_io* io, void* workspace, size_t workspace_bytes,
                       empose_stream_t stream);

/* The same forward in two parts that may be issued on different streams: EMPOSE_LGD_PHASE_INIT = input packing + the
 * initial estimate (LSTM with state carry + heads, or the init MLPs; reads io->h0/c0, writes io->h_n/c_n),
 * EMPOSE_LGD_PHASE_ITER = the N refinement iterations and the outputs.  The second part reads what the first left in
 * `workspace` (same io, same workspace; order them with an event).  A streaming caller runs chunk c + 1's INIT -- which
 * depends only on chunk c's final LSTM state -- beside chunk c's ITER, with two workspaces.  New in this library; the
 * reference runs the chunks of a recording strictly one after the other (scripts/evaluate_real.py:39-61). */
#define EMPOSE_LGD_PHASE_INIT 1
#define EMPOSE_LGD_PHASE_ITER 2
int empose_lgd_forward_phase(const empose_model_t* model, const empose_lgd_io* io, void* workspace,
                             size_t workspace_bytes, empose_stream_t stream, int phases);

/* ---- building blocks (also what the unit tests drive) --------------------------------------------------------- */

/* One SMPL-H evaluation restricted to the sensor sub-mesh and, optionally, the residual gradient.
 * Replaces get_estimated_real_markers + reconstruction_loss + autograd.backward
 * (reference models.py:471-483,560-579; loss.py:23-41; virtual_sensors.py:85-96).
 *   theta [T][ld_theta] (66 used), beta [T][ld_beta] (10 used)
 *   offset_r/offset_t per WINDOW ([T/F][12][3][3], [T/F][12][3]); F = frames per window
 *   targets: tgt [T][ld_tgt] holding n_markers*3 positions then n_markers*9 orientations (the network input
 *            layout of prepare_inputs, reference models.py:106-125); frame_scale [T] per-frame loss weight
 *   outputs pos [T][36], ori [T][108], joints [T][66]; g_theta [T][ld_g] (66), g_beta [T][ld_gb] (10) or NULL.
 * workspace: empose_smpl_workspace_bytes(model, T).
 * Launches of 16384 frames and more run the frame-per-lane kernels (csrc/smpl_tile.hip) when the model's sensor patches
 * allow it -- closed triangle fans of at most 8 faces over at most 8 bones, what a closed manifold body mesh gives;
 * empose_smpl_tile_supported says whether they do (option "smpl_tile": 0 never, 1 by size, 2 always). */
size_t empose_smpl_workspace_bytes(const empose_model_t* model, int T);
int empose_smpl_tile_supported(const empose_model_t* model);
int empose_smpl_sensors_fwd_bwd(const empose_model_t* model, int T, int F,
                                const float* theta, int ld_theta, const float* beta, int ld_beta,
                                const float* offset_r, const float* offset_t,
                                const float* tgt, int ld_tgt, const float* frame_scale,
                                float* pos, float* ori, float* joints,
                                float* g_theta, int ld_g, float* g_beta, int ld_gb,
                                void* workspace, size_t workspace_bytes, empose_stream_t stream);

/* Vector-Jacobian product of the same evaluation for training: given cotangents of the outputs
 * d_pos [T][36], d_ori [T][108], d_joints [T][66] (or NULL) returns g_theta [T][66], g_beta [T][10].
 * This is the backward of `get_estimated_real_markers` that the reference gets from autograd when
 * IterativeErrorFeedback.backward calls total_loss.backward() (reference models.py:634-688). */
size_t empose_smpl_vjp_workspace_bytes(const empose_model_t* model, int T);
int empose_smpl_sensors_vjp(const empose_model_t* model, int T, int F, const float* theta, int ld_theta,
                            const float* beta, int ld_beta, const float* offset_r, const float* offset_t,
                            const float* d_pos, const float* d_ori, const float* d_joints, float* g_theta,
                            float* g_beta, void* workspace, size_t workspace_bytes, empose_stream_t stream);

/* Both update networks on x [T][ldx]: d_pose [T][66], d_shape [T][10]
 * (replaces pose_net_iter / shape_net_iter, reference models.py:586-587; layers.py:46-77). */
size_t empose_update_workspace_bytes(const empose_model_t* model, int T);
int empose_update_nets_fwd(const empose_model_t* model, int T, const float* x, int ldx, float* d_pose, float* d_shape,
                           void* workspace, size_t workspace_bytes, empose_stream_t stream);

/* The init LSTM over ragged windows: x [B][F][ldx] (input_size used) -> y [B][F][H]
 * (replaces RNNLayer.forward, reference layers.py:133-157). */
size_t empose_lstm_workspace_bytes(const empose_model_t* model, int B, int F);
int empose_lstm_fwd(const empose_model_t* model, int B, int F, const float* x, int ldx, const int* seq_lengths,
                    const float* h0, const float* c0, float* y, float* h_n, float* c_n,
                    void* workspace, size_t workspace_bytes, empose_stream_t stream);

/* C[M][ldc] = act((A[M][lda] . W[N][ldw]^T) * scale[n] + shift[n]) on the fp32 matrix cores; scale/shift may be NULL.
 * Exposed for tests and for host code that needs a plain fp32 linear layer. */
int empose_linear_f32(const float* A, int lda, const float* W, int ldw, float* C, int ldc, int M, int N, int K,
                      const float* scale, const float* shift, int prelu, float slope, empose_stream_t stream);

/* As empose_linear_f32 with an optional residual operand resid [M][ldr]:
 *   act 0: y = acc*scale + shift (+ resid);  act 1: PReLU(slope) then + resid (MLP skip connection, layers.py:35-43);
 *   act 2: + resid, then ReLU (FeedForwardResidualBlock of the ResNet baseline, reference nn/layers.py:170-182). */
int empose_linear_f32_ex(const float* A, int lda, const float* W, int ldw, float* C, int ldc, int M, int N, int K,
                         const float* scale, const float* shift, const float* resid, int ldr, int act, float slope,
                         empose_stream_t stream);

/* Small GEMM with strided operands: C[M][ldc] = A . W^T (+ bias[n]) where A(m, k) = A[m * a_rs + k * a_ks] and
 * W(n, k) = W[n * w_rs + k * w_ks] -- any of the four transposition cases without a transposed copy.  This is what the
 * backward pass of the training path's linear layers needs (torch.nn.functional.linear's autograd, reference
 * nn/layers.py:46-77 in train mode): dX = dY . W and dW = dY^T . X.  Only problems of at most 512 output tiles of
 * 32 x 32 (empose_gemm_strided_applicable); larger ones belong to a library GEMM. */
int empose_gemm_strided_applicable(int M, int N);
int empose_gemm_strided_f32(int M, int N, int K, const float* A, long a_rs, long a_ks, const float* W, long w_rs,
                            long w_ks, float* C, int ldc, const float* bias, empose_stream_t stream);

/* Train-mode BatchNorm1d + PReLU (one shared slope) of an MLP hidden layer, forward and backward as one kernel each
 * (reference nn/layers.py:13-77 in training mode; torch.nn.BatchNorm1d semantics: batch statistics, biased variance for
 * the normalisation, running statistics updated with `momentum` and the unbiased variance, num_batches_tracked + 1).
 * x, z, dz, dx are [M][ld] row-major; gamma, beta, save_mean, save_rstd, dgamma, dbeta are [C]; slope is one device float;
 * dslope receives the slope gradient; dslope_partial (ceil(C / 32) floats) and counter (one int, zero before the first
 * call, left at zero by every call) are scratch. running_mean / running_var / num_batches_tracked may be NULL.
 * Batches of more than 1024 rows split the rows over workgroups and need empose_bn_prelu_workspace_bytes(M, C) bytes of
 * workspace for the partial sums (0 for smaller batches, workspace may then be NULL). */
size_t empose_bn_prelu_workspace_bytes(int M, int C);
int empose_bn_prelu_train_fwd(int M, int C, const float* x, int ldx, const float* gamma, const float* beta,
                              const float* slope, float eps, float momentum, float* running_mean, float* running_var,
                              long long* num_batches_tracked, float* z, int ldz, float* save_mean, float* save_rstd,
                              void* workspace, size_t workspace_bytes, empose_stream_t stream);
int empose_bn_prelu_train_bwd(int M, int C, const float* x, int ldx, const float* dz, int lddz, const float* gamma,
                              const float* beta, const float* slope, const float* save_mean, const float* save_rstd,
                              float* dx, int lddx, float* dgamma, float* dbeta, float* dslope, float* dslope_partial,
                              int* counter, void* workspace, size_t workspace_bytes, empose_stream_t stream);

/* ---- training backward: building blocks (BASELINE.json configs[4]) ------------------------------------------------ */
/* The reference trains through torch.autograd (reference nn/models.py:634-688, scripts/train.py:133-152); these are the
 * hand-written pieces the Python autograd Functions of em_pose_amd/nn call instead of library kernels.  All pointers are
 * DEVICE pointers (the parameters live in torch tensors and change every optimiser step: nothing is packed or cached). */

/* C[N][ldc] = A[M][lda]^T . B[M][ldb], optionally bias[n] = sum_m A[m][n]: the weight and bias gradient of a linear
 * layer y = x W^T + b (dW = dY^T X, db = column sums of dY; torch.nn.functional.linear's backward).  The reduction over
 * M is split over workgroups and summed in a fixed order (deterministic).  workspace: empose_gemm_atb_workspace_bytes. */
size_t empose_gemm_atb_workspace_bytes(int M, int N, int K);
int empose_gemm_atb_f32(int M, int N, int K, const float* A, int lda, const float* B, int ldb, float* C, int ldc,
                        float* bias, void* workspace, size_t workspace_bytes, empose_stream_t stream);
/* dst[c][r] = src[r][c] (rows x cols): W^T copies so that dX = dY . W runs on the forward GEMM (empose_linear_f32). */
int empose_transpose_f32(int rows, int cols, const float* src, int ld_src, float* dst, int ld_dst,
                         empose_stream_t stream);

/* One MLP of the LGD model (reference nn/layers.py:46-77) in TRAINING mode: Linear -> BatchNorm1d (batch statistics) ->
 * PReLU for every layer but the last, which is a plain Linear.  Device pointers to the parameters as torch holds them. */
typedef struct {
  int n_layers;                 /* 2 + 2 * blocks, <= EMPOSE_MAX_DENSE; no skip connections */
  int in_dim, hidden, out_dim;  /* in_dim and hidden multiples of 4 */
  const float* weight[EMPOSE_MAX_DENSE];   /* [out_l][in_l] */
  const float* bias[EMPOSE_MAX_DENSE];
  const float* bn_weight[EMPOSE_MAX_DENSE];   /* layers 0 .. n_layers-2 */
  const float* bn_bias[EMPOSE_MAX_DENSE];
  float* bn_running_mean[EMPOSE_MAX_DENSE];   /* updated in place like torch.nn.BatchNorm1d, may be NULL */
  float* bn_running_var[EMPOSE_MAX_DENSE];
  long long* bn_num_batches[EMPOSE_MAX_DENSE];
  const float* prelu[EMPOSE_MAX_DENSE];       /* one device float per layer */
  float bn_eps, bn_momentum;
  /* Optional, backward only: the weights of layers 1 .. n_layers-1 transposed, [in_l][out_l] with the leading dimension
   * of the last layer padded to a multiple of 4 and its padding columns ZERO (empose_transpose_f32 into a zeroed buffer).
   * With NULL entries the backward transposes the weights itself on every call; a caller that applies the network
   * several times per step (the LGD loop) transposes once per step instead.  empose_mlp_train_uses_weight_t() says
   * whether the backward of M rows reads them at all (the one-launch layers of up to 512 rows read W itself). */
  const float* weight_t[EMPOSE_MAX_DENSE];
  /* How `save` is laid out: 0 = whatever the options "train_fused" / "train_epi" select AT THE TIME OF EACH CALL (every
   * call of a step must then see the same options); 1 / 2 / 3 = the layout empose_mlp_train_save_layout() reported when
   * the forward ran -- the backward and weight-gradient calls of that step then read the buffer the way it was written
   * even if an option changed in between (an A/B script, another thread). */
  int save_layout;
  /* Optional (round 6), large batches only: the weights of layers 0 .. n_layers-2 (weight_x3: W_l itself, [hidden][in_l])
   * and of layers 1 .. n_layers-1 (weight_t_x3: the transposed copy `weight_t[l]`, [in_l][ld]) as three bf16 pieces per
   * weight in matrix-core fragment order, made by empose_pack_weight_x3 once per optimiser step.  When present (and option
   * "train_x3" != 0, M >= 1024, hidden % 64 == 0) the forward products y_l = a_{l-1} W_l^T and the reverse products
   * dA_{l-1} = dY_l W_l form every fp32 product from three bf16 pieces per operand (fp32-equivalent; bf16x3.h) instead of
   * running on the fp32 MFMA instruction.  NULL entries: the fp32 instruction. */
  const unsigned short* weight_x3[EMPOSE_MAX_DENSE];
  const unsigned short* weight_t_x3[EMPOSE_MAX_DENSE];
} empose_mlp_params;
/* A weight matrix W [N][ldw] (K columns used, K % 4 == 0) as three bf16 pieces per weight in fragment order; `out`:
 * empose_pack_weight_x3_bytes(N, K) bytes of device memory, 16-byte aligned. */
size_t empose_pack_weight_x3_bytes(int N, int K);
int empose_pack_weight_x3(const float* W, int ldw, int N, int K, void* out, empose_stream_t stream);
typedef struct {                /* gradient outputs, shapes of the parameters */
  float* weight[EMPOSE_MAX_DENSE];
  float* bias[EMPOSE_MAX_DENSE];
  float* bn_weight[EMPOSE_MAX_DENSE];
  float* bn_bias[EMPOSE_MAX_DENSE];
  float* prelu[EMPOSE_MAX_DENSE];
} empose_mlp_grads;
/* `save`: per hidden layer the pre-BatchNorm and the activated outputs [M][hidden] and the batch mean / rstd. */
/* 1 (BatchNorm kernels) / 2 (BatchNorm folded into the GEMMs) / 3 (statistics in the GEMM epilogues): the layout the
 * current options select for M rows; store it in empose_mlp_params::save_layout for the calls of the step. */
int empose_mlp_train_save_layout(const empose_mlp_params* p, int M);
/* 1: the backward of M rows reads `weight_t` (or transposes on every call when it is NULL); 0: it does not. */
int empose_mlp_train_uses_weight_t(const empose_mlp_params* p, int M);
size_t empose_mlp_train_save_floats(const empose_mlp_params* p, int M);
size_t empose_mlp_train_workspace_bytes(const empose_mlp_params* p, int M);
/* x [M][ldx] -> out [M][ld_out] (out_dim columns written). */
int empose_mlp_train_fwd(const empose_mlp_params* p, int M, const float* x, int ldx, float* out, int ld_out,
                         float* save, void* workspace, size_t workspace_bytes, empose_stream_t stream);
/* d_out [M][ld_dout]: ld_dout a multiple of 4 and >= out_dim, columns past out_dim ZERO.  Parameter gradients are
 * overwritten (accumulate = 0) or added to (1: the same network applied N times in the LGD loop).  The input x is not
 * differentiated: the LGD loop feeds the update networks detached values (reference models.py:549-551). */
int empose_mlp_train_bwd(const empose_mlp_params* p, int M, const float* x, int ldx, const float* d_out, int ld_dout,
                         const float* save, const empose_mlp_grads* grads, int accumulate, void* workspace,
                         size_t workspace_bytes, empose_stream_t stream);

/* Deferred weight gradients (the same network applied n_app times, as the N iterations of the LGD loop): the backward
 * of each application keeps its layer cotangents in `dz_stash` (empose_mlp_train_stash_floats floats) instead of forming
 * dW / db, and ONE call of empose_mlp_train_wgrad forms them over the rows of all applications -- one A^T B product of
 * n_app * M rows per layer instead of n_app products and reductions.  BatchNorm / PReLU parameter gradients are produced
 * by the deferred backward exactly as by empose_mlp_train_bwd.  x / save / dz_stash of wgrad: host arrays of n_app
 * device pointers (n_app <= 8), the arguments the applications were run with.  Same sums in a different order:
 * results agree with the per-application path to rounding, not bitwise.
 * The stash keeps d_out at dz_stash + M * (n_layers - 1) * hidden, row stride (out_dim + 3) & ~3: a caller that
 * produces d_out there (d_out = that address, ld_dout = that stride) saves the copy. */
size_t empose_mlp_train_stash_floats(const empose_mlp_params* p, int M);
int empose_mlp_train_bwd_deferred(const empose_mlp_params* p, int M, const float* x, int ldx, const float* d_out,
                                  int ld_dout, const float* save, const empose_mlp_grads* grads, int accumulate,
                                  float* dz_stash, void* workspace, size_t workspace_bytes, empose_stream_t stream);
/* Both update networks of one LGD iteration (they read the same rows x; reference nn/models.py:584-587 applies
 * `pose_net` and `shape_net` to the same detached input) in one call.  Up to 512 rows -- the reference's training batch of
 * 12 windows x 32 frames (scripts/train.py:125-152) -- every layer of BOTH networks is ONE launch, forward (product +
 * bias + train-mode BatchNorm + PReLU) and backward (dA = dZ W + the BatchNorm / PReLU reverse of the layer below):
 * a workgroup per 16 columns x quarter of the rows, whose column statistics meet through a mailbox of tagged words inside
 * the workspace (csrc/train_cols.hip; option "train_cols", 0 = a product and a BatchNorm launch per layer and network).
 * Networks the paired launches do not cover (different depth / hidden width / BatchNorm constants, more rows) run one
 * after the other through the single-network entry points: same results either way.
 * Reads and writes save layout 1, like empose_mlp_train_fwd / _bwd at these sizes (which use the same launches for one
 * network).  A poll of the mailbox that gives up is reported like the cooperative LSTM kernels' (empose_async_status).
 * Like those kernels the paired launches need every workgroup of a launch resident at once -- the device to themselves:
 * processes that SHARE one GPU must set "train_cols" to 0 (em_pose_amd/helpers/distributed.py does when ranks wrap around
 * the devices), or their launches starve each other until the polls give up; the same holds beside collective kernels that
 * wait for other ranks on another stream (the helper's gradient buckets switch it off for the overlapped sweep).
 * workspace: empose_mlp_train_pair_workspace_bytes. */
size_t empose_mlp_train_pair_workspace_bytes(const empose_mlp_params* p0, const empose_mlp_params* p1, int M);
int empose_mlp_train_fwd_pair(const empose_mlp_params* p0, const empose_mlp_params* p1, int M, const float* x, int ldx,
                              float* out0, int ld_out0, float* out1, int ld_out1, float* save0, float* save1,
                              void* workspace, size_t workspace_bytes, empose_stream_t stream);
int empose_mlp_train_bwd_deferred_pair(const empose_mlp_params* p0, const empose_mlp_params* p1, int M, const float* x,
                                       int ldx, const float* d_out0, int ld_dout0, const float* d_out1, int ld_dout1,
                                       const float* save0, const float* save1, const empose_mlp_grads* grads0,
                                       const empose_mlp_grads* grads1, int accumulate, float* dz_stash0, float* dz_stash1,
                                       void* workspace, size_t workspace_bytes, empose_stream_t stream);
size_t empose_mlp_train_wgrad_workspace_bytes(const empose_mlp_params* p, int n_app, int M);
int empose_mlp_train_wgrad(const empose_mlp_params* p, int n_app, int M, const float* const* x, int ldx,
                           const float* const* save, const float* const* dz_stash, const empose_mlp_grads* grads,
                           int accumulate, void* workspace, size_t workspace_bytes, empose_stream_t stream);

/* Network input rows and the per-frame residual weight as one launch.
 * Replaces `BaseModel.prepare_inputs` (reference models.py:106-125: reshape, 6-sensor subset S_CONFIG_6, concat
 * positions | row-major orientations) and the frame weighting of `reconstruction_loss` as the loop applies it
 * (reference loss.py:31-39 with the B * F rescale of models.py:578-579): weight[t] = [f < len_b] * F / len_b *
 * [all 12 sensors present].
 *   marker_pos [B*F][36], marker_oris [B*F][108]; marker_idx: the n_markers (<= 12) sensors taken, in order;
 *   marker_masks [B*F][12] or NULL; seq_lengths [B] (int32) or NULL (= F everywhere);
 *   x [B*F][ldx]: columns [0, 12 * n_markers) are written; frame_weight [B*F] or NULL (not wanted). */
int empose_pack_inputs(int B, int F, int n_markers, const int* marker_idx, const float* marker_pos,
                       const float* marker_oris, const float* marker_masks, const int* seq_lengths, float* x, int ldx,
                       float* frame_weight, empose_stream_t stream);

/* out[t][c] = mean of in[.][c] over the window of frame t (F consecutive rows); the operator is its own adjoint, so
 * the same call back-propagates (`_to_single_shape`, reference models.py:529-535,588-589). */
int empose_window_mean(int T, int F, int C, const float* in, int ld_in, float* out, int ld_out, empose_stream_t stream);
/* out = alpha x + beta y over a [rows][cols] block with row strides; x or y may be NULL (treated as 0), out may alias. */
int empose_axpby2d(int rows, int cols, float alpha, const float* x, int ldx, float beta, const float* y, int ldy,
                   float* out, int ldo, empose_stream_t stream);

/* Bookkeeping of the LGD loop around the update networks as single launches (each replaces 3-9 axpby / mean launches; at
 * the reference's training batch a step is launch-bound):
 *   assemble_inputs   X[t] = [x0[t] (d_in) | pose[t] (66) | shape[t] (10)]; the gradient columns d_in+76.. are written by
 *                     empose_smpl_sensors_fwd_bwd (reference models.py:584)
 *   additive_update   pose_next = pose + step d_pose, shape_next = shape + step (mean over the window of) d_shape
 *                     (reference models.py:588-600)
 *   cotangent_step    reverse sweep at history entry i: Dp = [Dp +] d_pose + vp [+ g_theta / (B F)], Ds likewise (loss
 *                     terms, body-model VJP, the in-forward E_i.backward() deposit of models.py:576), and with dpad / dspad
 *                     the zero-padded cotangents [T][68] / [T][12] of the update networks' outputs:
 *                     step * Dp, step * (window mean of) Ds.  `first`: Dp / Ds are overwritten, not accumulated. */
int empose_lgd_assemble_inputs(int T, int d_in, const float* x0, int ld_x0, const float* pose, const float* shape,
                               float* X, int ldx, empose_stream_t stream);
int empose_lgd_additive_update(int B, int F, float step, int shape_avg, const float* pose, const float* d_pose,
                               const float* shape, const float* d_shape, float* pose_next, float* shape_next,
                               empose_stream_t stream);
int empose_lgd_cotangent_step(int B, int F, int first, const float* d_pose, const float* d_shape, const float* vp,
                              const float* vs, const float* g_theta, int ld_g, const float* g_beta, int ld_gb, float* Dp,
                              float* Ds, float step, int shape_avg, float* dpad, float* dspad, empose_stream_t stream);

/* The loss of IterativeErrorFeedback.backward (reference models.py:634-688, loss.py:13-41) and the cotangents of the
 * total loss with respect to every history entry, in one pass. */
typedef struct {
  int B, F, n_hist, n_markers;  /* n_hist = N + 1 */
  int marker_idx[12];           /* first n_markers entries: which virtual sensors feed the network */
  const float* pose_hist;       /* [n_hist][T][66] */
  const float* shape_hist;      /* [n_hist][T][10] */
  const float* markers_hist;    /* [n_hist][T][36] */
  const float* markers_ori_hist;/* [n_hist][T][108] */
  const float* joints_final;    /* [T][66] */
  const float* pose_gt;         /* [T][66] */
  const float* shape_gt;        /* [B][10] */
  const float* joints_gt;       /* [T][66] or NULL (no FK loss) */
  const float* inputs; int ld_inputs;   /* network input rows: n_markers*3 positions then n_markers*9 orientations;
                                         * ld_inputs >= 12 * n_markers */
  const int* seq_lengths;       /* [B] or NULL */
  const float* marker_masks;    /* [T][12] or NULL */
  float w_pose, w_shape, w_fk, w_rec;
  float* d_pose; float* d_shape; float* d_markers; float* d_markers_ori;   /* like the histories */
  float* d_joints;              /* [T][66] */
  float* loss_vals;             /* [5] device floats: pose, shape, reconstruction, fk, total_loss */
} empose_loss_io;
size_t empose_lgd_losses_workspace_bytes(int B, int F, int n_hist);
int empose_lgd_losses(const empose_loss_io* io, void* workspace, size_t workspace_bytes, empose_stream_t stream);

/* torch.optim.Adam (amsgrad off, no weight decay) over n tensors in one launch.  The pointer tables are DEVICE arrays:
 * params/grads/exp_avg/exp_avg_sq [n] (void*), sizes [n] (int64), and the chunk tables chunk_tensor [n_chunks] (int32),
 * chunk_offset [n_chunks] (int64): chunk c covers elements [offset, offset + 4096) of tensor chunk_tensor[c].
 * step is the 1-based step count (bias correction). */
int empose_adam_step(int n_chunks, const void* params, const void* grads, const void* exp_avg, const void* exp_avg_sq,
                     const void* sizes, const void* chunk_tensor, const void* chunk_offset, float lr, float beta1,
                     float beta2, float eps, int step, empose_stream_t stream);

/* Stacked uni-directional LSTM with autograd support (reference nn/layers.py:133-157 in training mode: nn.LSTM over
 * packed ragged sequences, its backward through cuDNN/MIOpen).  Parameters as torch.nn.LSTM holds them. */
typedef struct {
  int num_layers, input_size, hidden_size;   /* num_layers <= 4 */
  const float* w_ih[4];   /* [4H][in]  (in = input_size for layer 0, H above) */
  const float* w_hh[4];   /* [4H][H] */
  const float* b_ih[4];   /* [4H] */
  const float* b_hh[4];
} empose_lstm_params;
typedef struct {          /* gradient outputs, same shapes; every weight / bias pointer required */
  float* w_ih[4];
  float* w_hh[4];
  float* b_ih[4];
  float* b_hh[4];
  /* optional (NULL: not wanted): the cotangents of the initial state, [B][H] per layer -- what a learned initial state
   * (reference nn/layers.py:121-131, `learn_init_state`) is trained with */
  float* d_h0[4];
  float* d_c0[4];
} empose_lstm_grads;
/* floats of the `save` buffer the forward fills for the backward: per layer gates [B][F][4H], cell states [B][F][H],
 * incoming hidden states [B][F][H], output sequence [B][F][H] */
size_t empose_lstm_train_save_floats(int num_layers, int B, int F, int hidden_size);
size_t empose_lstm_train_workspace_bytes(const empose_lstm_params* p, int B, int F);
/* x [B][F][ldx], seq_lengths [B] or NULL, h0/c0 [L][B][H] or NULL -> y [B][F][H], h_n/c_n [L][B][H] (may be NULL). */
int empose_lstm_train_fwd(const empose_lstm_params* p, int B, int F, const float* x, int ldx, const int* seq_lengths,
                          const float* h0, const float* c0, float* y, float* h_n, float* c_n, float* save,
                          void* workspace, size_t workspace_bytes, empose_stream_t stream);
/* dy [B][F][H] -> parameter gradients (overwritten), if dx != NULL dx [B][F][input_size], and where grads->d_h0 / d_c0 are
 * given the cotangents of the initial state.  The final state is not differentiated (it only seeds the next chunk,
 * detached, reference models.py:489-492). */
int empose_lstm_train_bwd(const empose_lstm_params* p, int B, int F, const float* x, int ldx, const int* seq_lengths,
                          const float* c0, const float* save, const float* dy, float* dx,
                          const empose_lstm_grads* grads, void* workspace, size_t workspace_bytes,
                          empose_stream_t stream);

/* ---- stand-alone (Bi)LSTM: the RNNLayer of the BiRNN baseline --------------------------------- */
/* reference nn/layers.py:80-157 (nn.LSTM, optionally bidirectional, packed ragged sequences). Parameter index
 * u = layer * dirs + direction (direction 1 = reverse), as PyTorch orders `*_l{k}` / `*_l{k}_reverse`; layer k > 0 of
 * a bidirectional stack takes 2*hidden inputs. State tensors are [num_layers*dirs][B][H]; y is [B][F][dirs*H]. */
typedef struct {
  int num_layers, input_size, hidden_size, bidirectional;
  const float* w_ih[8];
  const float* w_hh[8];
  const float* b_ih[8];
  const float* b_hh[8];
} empose_rnn_desc;
int empose_rnn_create(const empose_rnn_desc* desc, empose_rnn_t** out);
void empose_rnn_destroy(empose_rnn_t* rnn);
size_t empose_rnn_workspace_bytes(const empose_rnn_t* rnn, int B, int F);
int empose_rnn_fwd(const empose_rnn_t* rnn, int B, int F, const float* x, int ldx, const int* seq_lengths,
                   const float* h0, const float* c0, float* y, float* h_n, float* c_n, void* workspace,
                   size_t workspace_bytes, empose_stream_t stream);

/* Virtual sensor positions and local frames from full-mesh vertices [T][V][3]
 * (replaces VirtualMarkerHelper.get_virtual_pos_and_rot, reference data/virtual_sensors.py:85-96, and
 * compute_vertex_and_face_normals restricted to the sensor vertices, helpers/utils.py:126-146).
 * Index tables are DEVICE int32 arrays in mesh numbering: center/helper/deg [M], faces [M][max_deg][3].
 * Outputs pos [T][M][3], ori [T][M][3][3] (columns tangent, bitangent, normal), normals [T][M][3] un-normalised or NULL. */
int empose_virtual_sensors_fwd(int T, int V, const float* vertices, int M, int max_deg, const int* center,
                               const int* helper, const int* deg, const int* faces, float* pos, float* ori,
                               float* normals, empose_stream_t stream);

/* Vector-Jacobian product of empose_virtual_sensors_fwd (what autograd of the reference's VirtualMarkerHelper and
 * vertex normals computes): for the cotangents d_pos [T][M][3], d_ori [T][M][3][3] and d_normals [T][M][3] (any may be
 * NULL, not all three) it writes d_vertices [T][V][3], every element: vertices no sensor touches get 0.  It recomputes
 * the forward from `vertices`; nothing is saved from the forward.  fp32 throughout (csrc/sensors_vjp.hip: one pass per
 * (frame, sensor), one per (frame, mesh vertex)); deterministic: every destination sums its terms in the fixed order of
 * the tables below, no atomics, so repeated calls give the same bits.  No limit on max_deg.
 * Tables: the forward's center/helper/deg [M] and faces [M][max_deg][3], and the reverse's, all DEVICE int32:
 *   sub_faces     [n_sub_faces][3]   the distinct faces incident to the sensor vertices, mesh vertex ids, corners in
 *                                    the mesh's order (every face of `faces` is one of them)
 *   face_ptr      [n_sub_faces + 1]  CSR over sub-faces: face_sensors[face_ptr[f] .. face_ptr[f + 1]) are the sensors m
 *   face_sensors                     whose `faces` rows hold sub-face f, ascending m
 *   vf_ptr        [V + 1]            CSR over mesh vertices: vf_corner[vf_ptr[u] .. vf_ptr[u + 1]) = f * 3 + k for every
 *   vf_corner                        sub-face f whose corner k is u, ascending f
 *   vs_ptr        [V + 1]            CSR over mesh vertices: vs_role[vs_ptr[u] .. vs_ptr[u + 1]) = m * 2 + role for every
 *   vs_role                          sensor m with center[m] == u (role 0) or helper[m] == u (role 1), ascending
 *   touched       [n_touched]        the vertices u with entries in either CSR, ascending.  When they are at most a
 *                                    quarter of the mesh, d_vertices is cleared and only their rows are computed
 *                                    (a few sensors on the full mesh).  On a sensor sub-mesh (SMPLLayer.sub_mesh)
 *                                    every vertex is touched: there the dense form is the common case
 * Workspace: empose_virtual_sensors_vjp_workspace_bytes(T, M) -- 36 bytes per (frame, sensor) for a slab of frames
 * capped at 16384 and at 128 MB (0 for T or M <= 0).  Returns EMPOSE_EINVAL for a NULL vertex, table or d_vertices
 * pointer, T, V, M, max_deg, n_sub_faces or n_touched <= 0, all three cotangents NULL or a workspace that is too
 * small, before any GPU work.  Indices are not checked: the tables must be consistent with V and M. */
size_t empose_virtual_sensors_vjp_workspace_bytes(int T, int M);
int empose_virtual_sensors_vjp(int T, int V, const float* vertices, int M, int max_deg, const int* center,
                               const int* helper, const int* deg, const int* faces, int n_sub_faces,
                               const int* sub_faces, const int* face_ptr, const int* face_sensors, const int* vf_ptr,
                               const int* vf_corner, const int* vs_ptr, const int* vs_role, int n_touched,
                               const int* touched, const float* d_pos, const float* d_ori, const float* d_normals,
                               float* d_vertices, void* workspace, size_t workspace_bytes, empose_stream_t stream);

/* ---- synthetic sensor sampling (reference data/transforms.py:132-226, SampleMarkersWithOffsets) ------------------- */
/* Forward, one launch (csrc/sensor_sample.hip), one lane per (frame, sensor): the virtual sensors of
 * empose_virtual_sensors_fwd -- same tables, same arithmetic in the same order (csrc/sensor_frame.h) -- of N windows of
 * F frames, vertices [N * F][V][3], and on top of them the per-subject offsets:
 *   pos_synth    [N * F][M][3]     = pos + ori . local
 *   ori_synth    [N * F][M][3][3]  = ori . r[i][m] for window i; r [N][M][3][3], or NULL for the identity
 *   normal_synth [N * F][M][3]     = the third column of ori_synth
 * `mode` says what `local` is: EMPOSE_SAMPLE_LOCAL_WINDOW one offset per window [N][M][3], EMPOSE_SAMPLE_LOCAL_FRAME
 * one per frame [N * F][M][3], EMPOSE_SAMPLE_LOCAL_NONE none (`local` is ignored, pos_synth = pos).  pos, ori and normals
 * are the three outputs of empose_virtual_sensors_fwd.  Any of the six outputs may be NULL, not all.  fp32; repeated
 * calls give the same bits.  Returns EMPOSE_EINVAL, before any GPU work, for a NULL vertex or table pointer, N, F, V, M or
 * max_deg <= 0 (or N * F * M above 2^31 - 1), an unknown mode, `local` NULL in a mode that reads it, or six NULL outputs.
 * Indices are not checked: the tables must be consistent with V and M. */
#define EMPOSE_SAMPLE_LOCAL_NONE 0
#define EMPOSE_SAMPLE_LOCAL_WINDOW 1
#define EMPOSE_SAMPLE_LOCAL_FRAME 2
int empose_sample_sensors_fwd(int N, int F, int V, const float* vertices, int M, int max_deg, const int* center,
                              const int* helper, const int* deg, const int* faces, int mode, const float* local,
                              const float* r, float* pos, float* ori, float* normals, float* pos_synth,
                              float* ori_synth, float* normal_synth, empose_stream_t stream);

/* Vector-Jacobian product of empose_sample_sensors_fwd with respect to the vertices (`local` and `r` are constants and
 * get no cotangent): for the cotangents of the six outputs (any may be NULL, not all) it writes d_vertices
 * [N * F][V][3], every element.  One launch folds the synth cotangents into those of (pos, ori),
 *   d_pos = d_pos_synth,   d_ori = d_pos_synth (x) local + (d_ori_synth + d_normal_synth in column 2) . r^T,
 * and adds d_pos and d_ori; the sensor and vertex passes of empose_virtual_sensors_vjp, with its tables and its choice
 * between the dense and the touched-vertices form, do the rest.  Deterministic, no atomics.
 * Workspace: empose_sample_sensors_vjp_workspace_bytes(N * F, M) -- 84 bytes per (frame, sensor) for a slab of frames
 * with the caps of empose_virtual_sensors_vjp_workspace_bytes (0 for T or M <= 0).  Returns EMPOSE_EINVAL, before any GPU
 * work, for what the forward refuses, a NULL reverse table or d_vertices, n_sub_faces or n_touched <= 0, six NULL
 * cotangents or a workspace that is too small. */
size_t empose_sample_sensors_vjp_workspace_bytes(int T, int M);
int empose_sample_sensors_vjp(int N, int F, int V, const float* vertices, int M, int max_deg, const int* center,
                              const int* helper, const int* deg, const int* faces, int n_sub_faces,
                              const int* sub_faces, const int* face_ptr, const int* face_sensors, const int* vf_ptr,
                              const int* vf_corner, const int* vs_ptr, const int* vs_role, int n_touched,
                              const int* touched, int mode, const float* local, const float* r, const float* d_pos,
                              const float* d_ori, const float* d_normals, const float* d_pos_synth,
                              const float* d_ori_synth, const float* d_normal_synth, float* d_vertices,
                              void* workspace, size_t workspace_bytes, empose_stream_t stream);

/* ---- per-subject sensor offsets from calibration recordings (the inverse of empose_sample_sensors_fwd) -------------- */
/* The offset sets empose_sample_sensors_fwd consumes, estimated from recordings with ground-truth meshes and real
 * readings (csrc/offset_stats.hip).  The definition is this library's own: the reference ships the resulting files, not
 * their estimator.  Per frame f and sensor m, with (pos, ori) the virtual sensor of empose_virtual_sensors_fwd on
 * vertices [T][V][3] -- same tables, same arithmetic (csrc/sensor_frame.h) -- and (p [T][M][3], R [T][M][3][3]) the real
 * reading in the same frame:
 *   o = ori^T (p - pos)        Q = ori^T R
 * A frame counts for a sensor iff masks [T][M] reads 1 there (masks NULL: every frame counts).  A group is a run of
 * consecutive frames, one subject's pooled recordings; per (group, sensor), over its n counting frames:
 *   means   [G][M][3]     sum o / n
 *   covs    [G][M][3][3]  sum (o - means)(o - means)^T / (n - 1); zeros when n < 2
 *   r       [G][M][3][3]  the rotation closest to A = sum Q / n: with A = U S V^T, singular values descending,
 *                         U diag(1, 1, det(U V^T)) V^T
 *   r_trace [G][M]        s1 + s2 + det(U V^T) s3 = the mean of trace(r^T Q), in [-1, 3]; 3: every Q equals r
 *   counts  [G][M]        n (int32)
 * and for n = 0: means = 0, covs = 0, r = I, r_trace = 3.  local_f [T][M][3] and q_f [T][M][3][3], each optional (NULL),
 * receive o and Q of the frames of the groups, zeros where the frame does not count; frames outside every group are
 * not written.  o and Q are fp32; the sums are float64, added in a fixed order without atomics, a group in chunks of 256
 * frames counted from its own first frame: repeated calls give the same bits, and a group gives the same bits alone as
 * among others.  The outputs are fp32.
 * The group table is given twice, like the sequence table of empose_resample_rotations: groups_host is checked here,
 * groups_dev (the same G rows in device memory) is what the kernels read.
 * Workspace: empose_offset_stats_workspace_bytes(T, G, M) -- 19 doubles per sensor and chunk for ceil(T / 256) + G
 * chunks, a bound on what non-overlapping groups can own (0 for T, G or M <= 0).
 * Returns EMPOSE_EINVAL, before any GPU work, for a NULL vertex, table, reading, group-table or statistics pointer, T, V,
 * M, max_deg or G <= 0 (or T * M or G * M above 2^31 - 1), a group with n_frames < 0, with frames outside [0, T) or
 * starting before the end of the group before it (groups ascend and do not overlap; n_frames = 0 is allowed), or a
 * workspace that is too small.  Indices are not checked: the tables must be consistent with V and M. */
typedef struct {
  int first_frame, n_frames;
} empose_offset_group;
size_t empose_offset_stats_workspace_bytes(int T, int G, int M);
int empose_offset_stats(int T, int V, const float* vertices, int M, int max_deg, const int* center, const int* helper,
                        const int* deg, const int* faces, const float* p, const float* R, const float* masks, int G,
                        const empose_offset_group* groups_host, const empose_offset_group* groups_dev, float* means,
                        float* covs, float* r, float* r_trace, int* counts, float* local_f, float* q_f,
                        void* workspace, size_t workspace_bytes, empose_stream_t stream);

/* ---- sensor placement search (the step before empose_offset_stats) -------------------------------------------------- */
/* Which vertex does each sensor sit over?  The same recordings as empose_offset_stats, searched over the whole mesh
 * (csrc/placement.hip).  The definition is this library's own; the reference has no such tool.  Per sensor m and candidate
 * vertex c, over the n frames of a group in which the sensor was read, with p [T][M][3] the real reading and
 * vertices [T][V][3] the ground-truth mesh in the same frame:
 *   score[m][c] = sum_f |p_f(m) - x_f(c)|^2 / n   (m^2)        site[m] = argmin_c score[m][c], the lowest c on an exact tie
 * which is what the offsets pay for a site: |means|^2 + (n - 1) / n trace(covs) of empose_offset_stats there.
 *
 * empose_placement_accumulate adds one slab of T frames of one group to the running sums [M][C] (float64, device) and
 * counts [M] (int32, device), which the caller zeroes before a group's first slab; groups and slabs are the caller's loop.
 * A frame counts for a sensor iff masks [T][M] reads 1 there (masks NULL: every frame counts); what p holds where it does not
 * count is never used.  Candidates: cand NULL and C == V (candidate c is vertex c), or C strictly ascending vertex ids,
 * given twice like the group table of empose_offset_stats: cand_host is checked here, cand_dev (the same C ids in device
 * memory) is what the kernels read.  The difference and the square are fp32, every sum over frames float64, added in a
 * fixed order without atomics: the slab in chunks of 64 frames counted from its first frame, the chunks in ascending
 * order onto the running sum.  The same inputs in slabs of the same size give the same bits; other slab sizes agree to
 * float64 rounding.
 * Workspace: empose_placement_workspace_bytes(T, M, C) -- one double per sensor, candidate and chunk (0 for T, M or
 * C <= 0).
 * Returns EMPOSE_EINVAL, before any GPU work, for a NULL vertices, p, sums or counts, T, V, M or C <= 0, T * M or M * C above
 * 2^31 - 1, T above 64 * 65535 (use slabs), only one of cand_host and cand_dev, C != V without a list, a list that is not
 * strictly ascending within [0, V), or a workspace that is too small.
 *
 * empose_placement_finish turns the sums into score [M][C] (fp32; +inf where counts[m] == 0), best [M] (int32: the vertex
 * id of the winning candidate, cand_dev[c] or c; -1 where counts[m] == 0) and best_score [M].  The argmin runs over the
 * fp32 scores it writes, in a fixed order, and takes the lower id on equal scores.  cand_dev: the device list of the
 * accumulation, or NULL.  Returns EMPOSE_EINVAL for a NULL sums, counts or output pointer, M or C <= 0, or M * C above
 * 2^31 - 1. */
size_t empose_placement_workspace_bytes(int T, int M, int C);
int empose_placement_accumulate(int T, int V, const float* vertices, int M, const float* p, const float* masks, int C,
                                const int* cand_host, const int* cand_dev, double* sums, int* counts, void* workspace,
                                size_t workspace_bytes, empose_stream_t stream);
int empose_placement_finish(int M, int C, const double* sums, const int* counts, const int* cand_dev, float* score,
                            int* best, float* best_score, empose_stream_t stream);

/* ---- optional per-launch timing ------------------------------------------------------------------------------- */
/* While enabled, every kernel launch issued by the entry points above is bracketed by HIP events on the launch stream
 * and attributed to one of empose_profile_ntags() categories (GEMMs by role, LSTM step, chain kernel, ...).
 * empose_profile_read() waits for the recorded events, returns per-category total milliseconds and launch counts, and
 * clears the log. New in this library (the reference only has wall-clock prints, scripts/train.py:136-173). */
int empose_profile_enable(int on);
/* Single-kernel mode: only the launches of category `tag_name` are bracketed (start event, end event right after the
 * launch), the rest of the step runs unperturbed; every empose_lgd_forward additionally records one empty event pair,
 * reported as category "event_pair": what two event packets cost by themselves, to be subtracted from the bracketed
 * duration. This is how bench.py times the dominant kernel inside the step. */
int empose_profile_enable_only(const char* tag_name);
int empose_profile_ntags(void);
const char* empose_profile_tag_name(int tag);
int empose_profile_read(double* total_ms, long long* count);
/* Name, as rocprofv3 prints it, of the kernel a linear layer of `count` (1 or 2) problems of shape M x N x K is
 * dispatched to (role 1 = update-net hidden layer); lets bench.py label its roofline entry with the kernel that ran. */
const char* empose_profile_gemm_kernel_name(int M, int N, int K, int count, int role);

/* ---- full-mesh evaluation (final vertices; ground-truth preprocessing) ---------------------------------------- */

typedef struct {
  int n_vertices, j_off, ncp, kb;
  const float* wc;        /* [ncp][200] rows: V*3 vertex coordinates then n_joints*3 rest-joint coordinates */
  const int* skin_idx;    /* [V][kb], bone ids < 22 (hand weights folded into the wrists) */
  const float* skin_w;    /* [V][kb] */
  const int* parents;     /* [n_joints], topologically ordered, parents[0] < 0 */
  int n_joints;           /* posed joints returned: 22 (body) ... 52 (all of SMPL-H, as `body.Jtr`); 0 means 22 */
  int rodrigues;          /* EMPOSE_RODRIGUES_* */
  int with_bf16x3;        /* also pack the TWO-piece split-bf16 tables of empose_mesh_vertices_fwd_bf16x3 (+18 MB); the
                           * three-piece tables of the default path (25 MB) are always packed when kb <= 4 */
} empose_mesh_desc;

int empose_mesh_create(const empose_mesh_desc* desc, empose_mesh_t** out);
void empose_mesh_destroy(empose_mesh_t* mesh);
size_t empose_mesh_workspace_bytes(const empose_mesh_t* mesh, int T);
int empose_mesh_n_joints(const empose_mesh_t* mesh);
/* Replaces SMPLLayer.forward/fk (reference bodymodels/smpl.py:81-147): poses [T][66] (root first), betas [T][10],
 * trans [T][3] or NULL -> vertices [T][V][3], joints [T][n_joints][3] (n_joints = 52 reproduces `body.Jtr`; the 30 hand
 * joints have zero pose, reference smpl.py:99, so they ride rigidly on the wrists' frames).
 * Arithmetic (round 6): fp32 operands and fp32 accumulation; for body models with at most four bones per vertex the
 * blend-shape contraction forms every fp32 product from three bf16 pieces per operand on the bf16 matrix cores
 * (csrc/mesh_x3.hip: fp32-equivalent, measured against float64 in tests/test_hip_round6.py); option "mesh_x3" = 0 selects
 * the kernel on the fp32 MFMA instruction, which models with more bones per vertex always take. */
int empose_mesh_vertices_fwd(const empose_mesh_t* mesh, int T, const float* poses, const float* betas,
                             const float* trans, float* vertices, float* joints,
                             void* workspace, size_t workspace_bytes, empose_stream_t stream);

/* The same evaluation with the blend-shape contraction in split bf16 on the bf16 matrix cores, fp32 accumulate (pose
 * blend-shapes: 2 pieces / 3 products; template + shape: 3 pieces / 6 products; kinematic chain and skinning unchanged,
 * fp32).  NOT the arithmetic of the reference or of the headline benchmark: an explicitly selected variant whose vertices
 * stay within 1e-4 of the fp32 path (tests/test_hip_boundary.py); joints are identical (the chain does not use it). */
int empose_mesh_vertices_fwd_bf16x3(const empose_mesh_t* mesh, int T, const float* poses, const float* betas,
                                    const float* trans, float* vertices, float* joints, void* workspace,
                                    size_t workspace_bytes, empose_stream_t stream);

/* Joints only (forward kinematics without the mesh): what MetricsEngine needs from `smpl_model.fk`
 * (reference eval/metrics.py:223-228 keeps `kp3d[:, :22]` and discards the vertices). joints [T][n_joints][3]; same
 * workspace as above. */
int empose_mesh_joints_fwd(const empose_mesh_t* mesh, int T, const float* poses, const float* betas,
                           const float* trans, float* joints, void* workspace, size_t workspace_bytes,
                           empose_stream_t stream);

/* Vector-Jacobian product of empose_mesh_vertices_fwd (what autograd of the reference's SMPLLayer computes): for the
 * cotangents d_vertices [T][V][3] and/or d_joints [T][n_joints][3] (either may be NULL, not both) it writes
 * g_poses [T][66] and g_betas [T][10], and g_trans [T][3] unless NULL (the gradient with respect to trans, which the
 * forward adds to every vertex and joint).  It recomputes the forward's rotations, features, rest joints and transforms
 * from poses and betas; nothing is saved from the forward.  The gradient is that of the exact function, fp32 throughout
 * (csrc/mesh_vjp.hip: the two vertex sweeps on the fp32 MFMA instruction; mesh_chain.hip: the reverse kinematic chain), whatever
 * arithmetic the forward of the handle uses.  Deterministic: repeated calls give the same bits.
 * Workspace: empose_mesh_vjp_workspace_bytes(mesh, T) -- about 8.2 KB per frame of a slab of min(T, 16384) frames for
 * SMPL-H (the forward's scratch, the sweeps' outputs and the reverse's cotangents); below 8192 frames the vertex sweeps
 * split the mesh over more workgroups and add per-slice partial sums (at most about 4.5 MB more).
 * Every handle carries the reverse's tables (packed by empose_mesh_create): per 32-vertex tile 96 KB of coefficients in
 * the feat sweep's fragment order and 4 KB of dense skin weights, plus the rest-joint rows transposed, 200 x (ncp - j_off)
 * floats: 22 MB for SMPL-H (V = 6890).  Returns EMPOSE_EINVAL for a NULL handle, poses, betas, g_poses or g_betas, T <= 0,
 * both cotangents NULL or a workspace that is too small, before any GPU work. */
size_t empose_mesh_vjp_workspace_bytes(const empose_mesh_t* mesh, int T);
int empose_mesh_vjp(const empose_mesh_t* mesh, int T, const float* poses, const float* betas, const float* d_vertices,
                    const float* d_joints, float* g_poses, float* g_betas, float* g_trans, void* workspace,
                    size_t workspace_bytes, empose_stream_t stream);

/* Per-vertex error between two bodies on the same mesh handle (PVE / MPVPE; this project's addition, the reference has no
 * such metric): body A (poses_a, betas_a, trans_a: the ground truth) and body B (the estimate) with the layouts of
 * empose_mesh_vertices_fwd, trans_a / trans_b each [T][3] or NULL.  sums [T][2] (double) receives per frame the sum over
 * the handle's V vertices of |v_A - v_B| and of |v_A - v_B|^2, in metres and square metres; the mean per-vertex error of a
 * frame is sums[t][0] / V.  No mesh is written: both bodies of a frame are evaluated in the same lanes (csrc/mesh_err.hip,
 * fp32 operands on the fp32 MFMA instruction whatever arithmetic the handle's forward uses) and only per-tile partial
 * sums, 8 bytes per frame and 32 vertices, go through the workspace.  Deterministic, and a frame's two numbers depend on
 * that frame alone: not on T, on the frame's position in the call or on the other frames.
 * Workspace: empose_mesh_vertex_error_workspace_bytes(mesh, T), for a slab of min(T, 16384) frames twice the forward's
 * scratch, the posed joints and the partials (about 8.9 KB per frame for SMPL-H); 0 for a NULL handle or T <= 0.
 * Before any GPU work: EMPOSE_EINVAL for a NULL mesh, poses_a, betas_a, poses_b, betas_b, sums or workspace and for
 * T <= 0, EMPOSE_ENOMEM for a workspace that is too small; empose_last_error() names the argument. */
size_t empose_mesh_vertex_error_workspace_bytes(const empose_mesh_t* mesh, int T);
int empose_mesh_vertex_error(const empose_mesh_t* mesh, int T, const float* poses_a, const float* betas_a,
                             const float* trans_a, const float* poses_b, const float* betas_b, const float* trans_b,
                             double* sums, void* workspace, size_t workspace_bytes, empose_stream_t stream);

/* The same with the Procrustes-aligned error beside it (PA-PVE / PA-MPVPE; this project's addition like PVE): sums [T][4]
 * (double) receives per frame the two sums of empose_mesh_vertex_error, bit for bit, and then the sums of d_pa and d_pa^2
 * over the V vertices, d_pa = |v_A - (s R v_B + t)| with the similarity transform (optimal rotation, scale and
 * translation, a reflection turned into a rotation by flipping the last singular vector and value) that best maps the
 * vertices of B onto those of A -- the convention of the PA-MPJPE rows of empose_metrics_rows, over the vertices instead
 * of the joints.  No mesh is written: the bodies are evaluated twice in registers (csrc/mesh_err.hip), once for the 17
 * moments of the alignment, taken about each body's posed root joint, and once for the aligned distances; a 3 x 3 SVD per
 * frame in float64 lies between; the bone transforms of the second sweep are recomputed in float64 (Rodrigues, rest
 * joints, chain) and rounded once.  Deterministic, a frame's four numbers depend on that frame alone.  The transform itself
 * is not returned.
 * Workspace: empose_mesh_vertex_error_pa_workspace_bytes(mesh, T), for a slab of min(T, 16384) frames the scratch of
 * empose_mesh_vertex_error, a second set of posed joints, 68 bytes per frame and 32 vertices for the moments, 64 bytes
 * per frame for the transform and 2.1 KB per frame for the float64 rotations and rest joints (about 26 KB per frame for
 * SMPL-H); 0 for a NULL handle or T <= 0.  Asynchronous on
 * `stream`; allocates, copies and synchronises nothing.
 * Before any GPU work: EMPOSE_EINVAL for a NULL mesh, poses_a, betas_a, poses_b, betas_b, sums or workspace and for
 * T <= 0, EMPOSE_ENOMEM for a workspace that is too small; empose_last_error() names the argument. */
size_t empose_mesh_vertex_error_pa_workspace_bytes(const empose_mesh_t* mesh, int T);
int empose_mesh_vertex_error_pa(const empose_mesh_t* mesh, int T, const float* poses_a, const float* betas_a,
                                const float* trans_a, const float* poses_b, const float* betas_b, const float* trans_b,
                                double* sums, void* workspace, size_t workspace_bytes, empose_stream_t stream);

/* ---- root normalisation (reference bodymodels/smpl.py:112-119, data/transforms.py:247-254) ----------------------- */
/* T frames in segments of seg_len consecutive rows (T % seg_len == 0): a sequence is re-expressed in the frame of the
 * first root orientation of its segment, R_0 = exp(root[first]):
 *   root_out[t]  = log(R_0^T exp(root[t]))                                   [T][3]
 *   trans_out[t] = R_0^T trans[t] - R_0^T trans[first]                       [T][3], by `flags`
 * `root` points at rows of ld_root >= 3 floats whose first three columns are the root axis-angle (poses [T][66] in
 * place: ld_root = 66); `rodrigues` is the EMPOSE_RODRIGUES_* convention of the exponential map.  flags = 0 leaves the
 * translation alone (trans and trans_out may be NULL); EMPOSE_ROOT_FRAME_ROTATE rotates it, EMPOSE_ROOT_FRAME_SUBTRACT
 * subtracts the segment's first (rotated, if also ROTATE) translation; the reference's layer does both.  The first
 * frame of every segment gets exact zeros for the orientation and, with SUBTRACT, for the translation.  The logarithm is
 * accurate over the whole range [0, pi] (csrc/root_frame.hip); outputs must not alias inputs.  No workspace.
 *
 * empose_root_frame_vjp: for cotangents d_root_out and/or d_trans_out [T][3] (either may be NULL, not both; d_trans_out
 * needs flags != 0) it writes g_root [T][3] and, when d_trans_out is given, g_trans [T][3].  The first frame's rows
 * collect what every frame of the segment sends back through R_0 and trans[first], summed in one fixed order: repeated
 * calls give the same bits.  The derivative is that of the exact maps (left and right Jacobians of SO(3), series at small
 * angles), finite everywhere including Rn = I -- not that of the reference's acos-based logarithm, which is 0 * inf at
 * the first frame of every sequence.  Workspace: empose_root_frame_vjp_workspace_bytes(T, seg_len), 36 bytes per 64
 * frames of a segment (0 for bad sizes).
 * Both return EMPOSE_EINVAL, before any GPU work, for a NULL required pointer, T <= 0, seg_len <= 0, T % seg_len != 0,
 * ld_root < 3, an unknown `rodrigues` or unknown flag bits; the reverse also for both cotangents NULL, d_trans_out with
 * flags == 0 and a workspace that is too small. */
#define EMPOSE_ROOT_FRAME_ROTATE 1
#define EMPOSE_ROOT_FRAME_SUBTRACT 2
int empose_root_frame_fwd(int T, int seg_len, int rodrigues, const float* root, int ld_root, const float* trans,
                          float* root_out, float* trans_out, int flags, empose_stream_t stream);
size_t empose_root_frame_vjp_workspace_bytes(int T, int seg_len);
int empose_root_frame_vjp(int T, int seg_len, int rodrigues, const float* root, int ld_root, const float* trans,
                          const float* d_root_out, const float* d_trans_out, float* g_root, float* g_trans, int flags,
                          void* workspace, size_t workspace_bytes, empose_stream_t stream);

/* ---- resampling to another frame rate (reference scripts/preprocess_amass_3dpw.py:63-123) ----------------------- */
/* One launch resamples a ragged batch of S sequences.  Sequence s reads f_in input rows from row in_row (knots at
 * k / fps_in) and writes f_out output rows from row out_row (times k / fps_out).  f_out is the caller's: the reference's
 * len(np.arange(0, f_in / fps_in, 1 / fps_out)), which the kernels trust.  Output rows are packed in table order
 * (out_row[0] = 0, out_row[s + 1] = out_row[s] + f_out[s]); input rows may lie anywhere inside [0, in_rows). */
typedef struct {
  int in_row, f_in, out_row, f_out;
  double fps_in, fps_out;
} empose_resample_seq;

/* The table is passed twice: `seqs_host` is validated (no GPU work), `seqs_dev` is the same S entries in device memory,
 * which the kernels read.  `in` points at in_rows rows of ld_in floats, `out` at out_rows rows of ld_out floats (float32,
 * device); arithmetic inside a thread is double precision.  Outputs must not alias inputs.
 *
 * empose_resample_rotations replaces resample_rotations / interpolate_rotations: the first 3 * J columns of a row are J
 * rotation vectors.  Shoemake's SQUAD on uniform knots over a hemisphere-consistent four-knot stencil, constant-velocity
 * phantom knots at both ends (so the end control points are the end knots, and f_in = 2 is plain slerp), the last
 * segment's formula past the last knot; the result is the rotation vector with |r| <= pi (csrc/resample.hip).  The
 * reference takes SQUAD from the numpy-quaternion package: interior segments follow the same published formula, its
 * treatment of the first and last segment and of times past the last knot is not verified against this one.
 *
 * empose_resample_positions replaces resample_positions / interpolate_positions: the first C columns of a row are C
 * channels; the not-a-knot cubic spline scipy.interpolate.CubicSpline computes by default (f_in = 2: the line, f_in = 3:
 * the parabola), extrapolated with the last polynomial.  The tridiagonal first-derivative system is solved in double by
 * one serial sweep per (sequence, channel), in one fixed order, in a workspace of
 * empose_resample_positions_workspace_bytes(in_rows, C) = one double per input row and channel (0 for bad sizes).
 *
 * Both are deterministic, and a sequence's result does not depend on the rest of the batch.  Both return EMPOSE_EINVAL,
 * before any GPU work, for a NULL pointer, S, J or C <= 0, a leading dimension smaller than the columns read or written,
 * f_in < 2 (one frame cannot be resampled), f_out < 1, a rate that is not positive and finite, input rows outside
 * [0, in_rows), output rows that are not packed or do not sum to out_rows; the positions also for a workspace that is too
 * small. */
int empose_resample_rotations(int S, const empose_resample_seq* seqs_host, const empose_resample_seq* seqs_dev, int J,
                              const float* in, int ld_in, int in_rows, float* out, int ld_out, int out_rows,
                              empose_stream_t stream);
size_t empose_resample_positions_workspace_bytes(int in_rows, int C);
int empose_resample_positions(int S, const empose_resample_seq* seqs_host, const empose_resample_seq* seqs_dev, int C,
                              const float* in, int ld_in, int in_rows, float* out, int ld_out, int out_rows,
                              void* workspace, size_t workspace_bytes, empose_stream_t stream);

/* ---- sensor-noise augmentation (reference empose/data/noise_functions.py) -------------------------------------- */
/* One launch writes the noisy copies of the synthetic sensor readings of N windows of F frames and M sensors: positions
 * [N][F][M * 3], orientations [N][F][M * 9], normals [N][F][M * 3], float32, device.  The random draws are the caller's
 * (the reference's seeded host generators); `window_len` consecutive frames of window i are affected, from frame
 * start[i].  The plan's integers are passed twice: `start_host` / `sensor_host` are validated (no GPU work),
 * `start_dev` / `sensor_dev` are the same values in device memory, which the kernel reads.
 *
 * EMPOSE_SENSOR_NOISE_SUPPRESS: sensors sensor[i][0..K) of window i (ids into the batch's own M sensors; [N][K]) read
 *   `mask_value` in all 3 + 9 + 3 floats over the affected frames; every other float is a bit copy.  u_r, theta, phi,
 *   max_r and the thigh indices are ignored.
 * EMPOSE_SENSOR_NOISE_SPHERICAL: the K sensors sensor[0..K) ([K], shared by all windows) are displaced by
 *   (r cos(theta) sin(phi), r sin(theta) cos(phi), r cos(phi)) -- the reference's formula as written -- with
 *   r = u_r * max_r * thigh / 2 and thigh = |pos[0][F / 2][thigh_a] - pos[0][0][thigh_b]| read on the device; u_r, theta
 *   and phi are [N][window_len][K] (may be NULL when window_len = 0).  Only positions are written: ori, normal, ori_out,
 *   normal_out and mask_value are ignored.  Every product and sum is rounded on its own (no contraction).
 *
 * A sensor id named twice in a plan is harmless (spherical: its last entry counts), window_len = 0 copies, repeated calls
 * give the same bits, and a window's result does not depend on the rest of the batch.  Returns EMPOSE_EINVAL, before any
 * GPU work, for a NULL required pointer, N, F or M <= 0 (or N * F * M * 15 above 2^39: one launch), K < 1 or K > M,
 * window_len < 0 or > F, an unknown mode, a thigh index outside [0, M) (spherical), an output pointer equal to its input,
 * suppression without the orientation and normal buffers, a start outside [0, F - window_len] or a sensor id outside
 * [0, M). */
#define EMPOSE_SENSOR_NOISE_SPHERICAL 0
#define EMPOSE_SENSOR_NOISE_SUPPRESS 1
int empose_sensor_noise(int mode, int N, int F, int M, int K, int window_len, const int* start_host,
                        const int* sensor_host, const int* start_dev, const int* sensor_dev, const float* u_r,
                        const float* theta, const float* phi, float max_r, int thigh_a, int thigh_b, float mask_value,
                        const float* pos, const float* ori, const float* normal, float* pos_out, float* ori_out,
                        float* normal_out, empose_stream_t stream);

/* ---- evaluation metrics ------------------------------------------------------------------------ */
/* Per frame: 22 Euclidean joint distances, 22 distances after similarity-Procrustes alignment of the prediction onto
 * the ground truth, and 21 geodesic angles (degrees) between global joint orientations with the root fixed to the
 * identity. Replaces MetricsEngine._compute_eucl_dist / _procrustes / _compute_angular_dist + local_to_global
 * (reference eval/metrics.py:18-66,110-162; helpers/utils.py:165-199). joints_* [T][22][3], pose_* [T][63] (body
 * axis-angles, no root) or NULL (angles reported as 0), parents: HOST int[22]; rows: device double [T][65]. */
int empose_metrics_rows(int T, const float* joints_gt, const float* joints_hat, const float* pose_gt,
                        const float* pose_hat, const int* parents_host, double* rows, empose_stream_t stream);

/* ---- temporal metrics (new in this library) ---------------------------------------------------- */
/* Acceleration error and jitter of two point trajectories over a ragged batch of sequences (csrc/temporal.hip).  The
 * definitions are this library's own; the reference has no temporal metric.  x_gt, x_hat [N][F][P][3] (fp32, metres,
 * contiguous), valid [N][F] (non-zero where the frame counts), fps frames per second.  Backward stencils, per row:
 *   acc[t]  = (x[t] - 2 x[t-1] + x[t-2]) fps^2               defined where frames t-2 .. t all count
 *   jerk[t] = (x[t] - 3 x[t-1] + 3 x[t-2] - x[t-3]) fps^3    defined where frames t-3 .. t all count
 * A stencil never reaches across a frame that does not count and never across two rows; what the inputs hold at a frame
 * that does not count is never used.  defined [N][F]: bit 0 (EMPOSE_TEMPORAL_ACC) acc is defined at the frame, bit 1
 * (EMPOSE_TEMPORAL_JERK) jerk is.
 *   reduce = 0: rows [N * F][3 P] float64 -- |acc_gt - acc_hat| per point (m/s^2), then |jerk_hat| per point, then
 *               |jerk_gt| per point (m/s^3)
 *   reduce = 1: rows [N * F][6] float64 -- for each of the three quantities the sum over the P points and the sum of
 *               squares, added in an order fixed by P alone, without atomics
 * Undefined entries are written as 0; every element of rows and defined is written by every call.  Every difference,
 * product and norm is float64 on the fp32 inputs, without fused multiply-adds.  A frame's row depends only on its own four
 * frames: two calls, or a call on a slab that holds those frames, give the same bits.  The time axis is walked in segments
 * of EMPOSE_TEMPORAL_SEGMENT frames, each after three frames of lead-in.  F < 3 is legal and yields nothing defined.
 * Returns EMPOSE_EINVAL, before any GPU work, for N, F or P <= 0, a NULL pointer, fps <= 0 or not finite, reduce other
 * than 0 or 1, or N * F (or the launch's workgroups) above 2^31 - 1. */
#define EMPOSE_TEMPORAL_SEGMENT 32
#define EMPOSE_TEMPORAL_ACC 1
#define EMPOSE_TEMPORAL_JERK 2
int empose_temporal_rows(int N, int F, int P, const float* x_gt, const float* x_hat, const unsigned char* valid, double fps,
                         int reduce, double* rows, unsigned char* defined, empose_stream_t stream);

/* ---- smoothing of pose sequences (new in this library) ----------------------------------------- */
/* Two filters for estimated pose sequences (csrc/smooth.hip); the reference has none, and the definitions below are this
 * library's own.  A row of `in` [N * F][ld_in] (fp32, device) is [3 J rotation-vector columns | C linear columns |
 * padding]; `out` [N * F][ld_out] likewise, and its columns at or beyond 3 J + C are never written.  valid [N][F]: non-zero
 * where the frame counts; NULL: every frame counts.  A run is a maximal stretch of consecutive counting frames of one
 * row.  Neither filter reaches across a frame that does not count or across two rows; such a frame gets its input columns
 * copied bit for bit, and what it holds (NaN included) never reaches another frame.  Rotations are filtered on SO(3)
 * through unit quaternions q(.), not as rotation-vector components; every rotation written has |r| <= pi.  Arithmetic
 * inside a thread is float64 on the fp32 inputs without fused multiply-adds; there are no atomics; a row's result does not
 * depend on the rest of the batch, and repeated calls give the same bits.
 *
 * empose_smooth_window: a zero-phase FIR filter.  taps_host: R + 1 host doubles w[0 .. R], one side of a symmetric
 * kernel, 0 <= R <= EMPOSE_SMOOTH_MAX_RADIUS.  For a counting frame t of the run [a, b] the half-width shrinks
 * symmetrically, r = min(R, t - a, b - t): the window never leaves the run and stays symmetric, so constant-velocity
 * motion is reproduced, and the end frames of a run pass through.
 *   channel:   acc = w0 x[t], then for k = 1 .. r ascending acc += w_k (x[t-k] + x[t+k]); wsum = w0, wsum += 2 w_k;
 *              out = acc / wsum
 *   rotation:  c = q(r[t]); acc = w0 c; acc += w_k (s- q(r[t-k]) + s+ q(r[t+k])) with s = -1 where the dot product with
 *              c is negative, else +1; out = the rotation vector of acc / |acc| with w >= 0.  |acc| >= w0 > 0.
 * This sign-aligned chordal mean is this library's definition of the windowed mean of rotations (not the Karcher mean).
 * The time axis is cut into segments of EMPOSE_SMOOTH_SEGMENT frames, which does not change the result.
 *
 * empose_smooth_one_euro: the causal One-Euro filter (Casiez, Roussel, Vogel 2012), alpha(fc) = 1 / (1 + fps / (2 pi fc)).
 * At the first counting frame of a run x^ = x, s^ = 0.  Afterwards
 *   channel:   d = (x - x^) fps; s^ += alpha(d_cutoff) (d - s^); fc = min_cutoff + beta |s^|; x^ += alpha(fc) (x - x^)
 *   rotation:  q = q(r) in the hemisphere of x^; delta = log(x^-1 q); theta = 2 |delta| in [0, pi]; d = theta fps; s^ and
 *              fc as above; x^ <- x^ exp(alpha(fc) delta), renormalised; out = its rotation vector.
 * A frame that does not count ends the run and clears the state.  state_in / state_out: [N][J + C][EMPOSE_SMOOTH_STATE]
 * device doubles (x^ as 4 -- a channel uses the first --, s^, live flag), each may be NULL; state_in NULL: every row starts
 * fresh; state_out receives the state after frame F - 1.  Feeding a sequence in chunks through the state gives the bits
 * of feeding it whole.
 *
 * Both return EMPOSE_EINVAL, before any GPU work, for N or F <= 0, J or C < 0 or J + C = 0, a leading dimension below
 * 3 J + C, NULL in, out or taps_host, out == in, R outside [0, 32], a tap that is negative or not finite or w0 <= 0, fps,
 * min_cutoff or d_cutoff not positive and finite, beta negative or not finite, or N * F above 2^31 - 1. */
#define EMPOSE_SMOOTH_SEGMENT 64
#define EMPOSE_SMOOTH_MAX_RADIUS 32
#define EMPOSE_SMOOTH_STATE 6
int empose_smooth_window(int N, int F, int J, int C, const float* in, int ld_in, const unsigned char* valid, int R,
                         const double* taps_host, float* out, int ld_out, empose_stream_t stream);
int empose_smooth_one_euro(int N, int F, int J, int C, const float* in, int ld_in, const unsigned char* valid, double fps,
                           double min_cutoff, double beta, double d_cutoff, const double* state_in, double* state_out,
                           float* out, int ld_out, empose_stream_t stream);

/* ---- model-free sensor fitting (new in this library) ------------------------------------------- */
/* A pose per frame and a shape per window (or per frame) from sensor readings alone: K steps of Adam on, per window w
 * of F frames with live_t = [t < seq_length],
 *   J_w = sum_t s_t E_t + lambda_pose / 2 sum_{t live} |theta_t[3:66] - p_t[3:66]|^2 + lambda_shape / 2 |beta_w|^2
 *         + lambda_smooth / 2 sum_{t >= 1, live} |theta_t - theta_{t-1}|^2.
 * E_t is the reconstruction energy of empose_smpl_sensors_fwd_bwd (sum over the model's sensors of |pos - target| and
 * |ori - target|_F, reference loss.py:23-41) and s_t = live_t * [every sensor the model reads has mask 1 in the frame]:
 * the weight of a frame is 1, not F / len.  The root orientation theta[0:3] is not regularised towards the prior.  With
 * one shape per frame the shape term is summed over the live frames.  The reference has no such optimiser; its learned
 * loop (models.py:547-600) is this one with the step replaced by two networks.
 *   tgt [B*F][ld_tgt]       the rows empose_pack_inputs writes for the model's sensors (12 * n_markers columns read)
 *   seq_lengths [B] int32 or NULL (= F), marker_masks [B*F][12] or NULL, offset_r [B][12][3][3], offset_t [B][12][3]
 *   pose_init [B*F][66], shape_init [B*F][10] or NULL (zeros; one shape per window: the row of the window's first
 *   frame); pose_prior p [B*F][66] or NULL (zeros)
 *   iterate k + 1 = iterate k - lr lr_decay^k c1 m / (sqrt(c2 v) + eps), m and v the Adam moments with beta1, beta2 and
 *   c1 = 1 / (1 - beta1^(k+1)), c2 = 1 / (1 - beta2^(k+1)); the three k-dependent factors are computed in double on the
 *   host and rounded to float once.  Padded frames keep their init.  One shape per window: the gradient is the sum over
 *   the window's live frames and every row of `shape` holds the window's shape.
 *   keep_best: what is returned is, per window, the iterate of 0 .. K with the smallest J_w (the earliest of equal
 *   ones); otherwise iterate K.
 *   outputs: pose [B*F][66], shape [B*F][10], and joints [B*F][66], pos [B*F][36], ori [B*F][108] of what is returned
 *   (the bits of empose_smpl_sensors_fwd_bwd on it at T = B*F); objective [K + 2][B] or NULL: J_w of the iterates
 *   0 .. K, then of what is returned; energy [B*F] or NULL: s_t E_t of what is returned.
 * K + 2 SMPL evaluations (K with the reverse pass) through the path of empose_smpl_sensors_fwd_bwd at T = B*F, one
 * launch of csrc/sensor_fit.hip after each.  No host synchronisation, no allocation, no copy from the host: the call is
 * asynchronous on `stream` and may be captured in a HIP graph.  Every sum runs in a fixed order and nothing is
 * accumulated atomically: the same inputs give the same bits.  K = 0 returns the init with its outputs and J.
 * Returns, before any GPU work, EMPOSE_EINVAL for a NULL model, io, workspace, tgt, offset_r, offset_t, pose, shape,
 * joints, pos or ori, B or F <= 0 (or B * F above 2^24), K < 0, ld_tgt < 12 * n_markers, lr or lr_decay not finite or
 * not positive, beta1 or beta2 outside [0, 1), eps not finite or negative, or a negative or non-finite lambda;
 * EMPOSE_ENOMEM for a workspace below empose_sensor_fit_workspace_bytes (0 for a NULL model or B, F <= 0);
 * empose_last_error() names the field. */
typedef struct {
  int B, F, K;
  const float* tgt; int ld_tgt;
  const int* seq_lengths; const float* marker_masks;
  const float* offset_r; const float* offset_t;
  const float* pose_init; const float* shape_init; const float* pose_prior;
  float lr, lr_decay, beta1, beta2, eps, lambda_pose, lambda_shape, lambda_smooth;
  int shape_per_window, keep_best;
  float* pose; float* shape; float* joints; float* pos; float* ori;
  float* objective; float* energy;
} empose_fit_io;
size_t empose_sensor_fit_workspace_bytes(const empose_model_t* model, int B, int F);
int empose_sensor_fit(const empose_model_t* model, const empose_fit_io* io, void* workspace, size_t workspace_bytes,
                      empose_stream_t stream);
/* What one iteration does after its SMPL evaluation, as exactly one launch on the caller's buffers (the unit tests drive
 * it; empose_sensor_fit is K of these between evaluations).  From `io`: B, F, tgt, ld_tgt, seq_lengths, pose_prior, the
 * step sizes, betas, eps, lambdas and shape_per_window; everything else of it is ignored.  k >= 0 is the iteration.
 *   theta, beta: iterate k; g_theta [B*F][66], g_beta [B*F][10], pos, ori: what empose_smpl_sensors_fwd_bwd gave for it
 *   with frame_scale = s; s [B*F] the frame weights
 *   m_theta, v_theta [B*F][66], m_beta, v_beta [B*F][10]: Adam moments, updated in place on live frames (one shape per
 *   window: the window's first row only)
 *   theta_next, beta_next: iterate k + 1, buffers other than theta and beta
 *   energy [B*F] (s_t E_t at iterate k) or NULL, J [B] (J_w at iterate k)
 *   best_J [B], best_theta, best_beta: where J_w is below best_J, iterate k and J_w are copied there; all three or none. */
int empose_sensor_fit_step(const empose_model_t* model, const empose_fit_io* io, int k, const float* theta,
                           const float* beta, const float* g_theta, const float* g_beta, const float* pos,
                           const float* ori, const float* s, float* m_theta, float* v_theta, float* m_beta,
                           float* v_beta, float* theta_next, float* beta_next, float* energy, float* J, float* best_J,
                           float* best_theta, float* best_beta, empose_stream_t stream);

/* ---- headless mesh rendering (new in this library) -------------------------------------------- */
/* A z-buffer rasteriser for posed meshes: T frames of V vertices and one table of n_faces triangles to T images of
 * H x W pixels, in three launches per slab of frames (csrc/raster.hip).  The definition is this library's own:
 *   camera    p_c = R p + t with a row-major 3 x 3 R and a 3-vector t, one for all frames or, camera_per_frame != 0, one
 *             per frame ([T][3][3], [T][3]); the camera looks along +z; x = fx X / Z + cx, y = fy Y / Z + cy, image y
 *             points down, and the pixel of row i, column j has its centre at (j + 0.5, i + 0.5).
 *   coverage  a face with a vertex at Z <= near is dropped whole (no clipping against the near plane), a face whose
 *             bounding box holds no pixel centre or whose screen area is exactly 0 is skipped, and there is no back-face
 *             culling.  A pixel centre is covered where the three edge functions, oriented by the sign of the area, are
 *             all >= 0: edges are inclusive.
 *   depth     perspective-correct, Z = 1 / sum_k lambda_k / Z_k.  The nearest face wins; on an exact tie of the depth the
 *             lower face id does.  The z-buffer is a 64-bit integer key per pixel, (bits of Z) << 32 | face id, updated
 *             with integer atomicMin: no floating-point atomics, the result does not depend on the order of arrival.
 *   shading   intensity = ambient + (1 - ambient) |n . l| / (|n| |l|), two-sided; `light` is a direction in camera
 *             space (normalised here); n is interpolated from `normals` ([T][V][3], un-normalised, world space, rotated
 *             by R) or, normals == NULL, the face normal (flat shading).  The base colour is `colors`: [3] for
 *             EMPOSE_RENDER_COLOR_UNIFORM, [V][3] for _VERTEX, [T][V][3] for _FRAME, the latter two interpolated like
 *             the normals; a byte is floor(255 c + 0.5) clamped to 0 .. 255.
 *   outputs   rgb uint8 [T][H][W][3]; face_id int32 [T][H][W] (or NULL); depth float32 [T][H][W] (or NULL).  Pixels no
 *             face covers: face_id -1, depth +inf, `background`.
 * Every pixel depends on its own frame alone and nothing is summed: a second call gives the same bits, and a frame gives
 * the same bits alone, inside a batch and on either side of a slab edge.  H and W are at most EMPOSE_RENDER_MAX_IMAGE,
 * which bounds the pixels one face can cover; a face whose bounding box holds more than 256 pixel centres is walked by its
 * whole wave, not by one lane.  Frames are rendered in slabs (slab_frames of them, 0: what fits 64 MB of workspace, at
 * least one; a larger value than that is lowered to it), so empose_render_workspace_bytes(T, V, H, W) -- the projected
 * vertices and the keys of one slab; 0 for sizes the call refuses -- is bounded whatever T is.
 * Face indices: `faces_host`, when given, is a host copy of the device table `faces` and is checked against [0, V) on
 * every call; the kernels clamp an index into [0, V) in any case, so a table that was not checked reads inside `vertices`.
 * All other pointers are device memory.  The call is asynchronous on `stream`: it never synchronises, allocates or copies.
 * Returns EMPOSE_EINVAL, before any GPU work, for a NULL descriptor, vertices, faces, colors, cam_R, cam_t, rgb or
 * workspace, T, V, n_faces, H or W <= 0 (V above 2^24, n_faces above 2^26), H or W above the cap, an unknown color_mode,
 * near <= 0 or not finite, fx, fy, cx, cy not finite or fx, fy zero, ambient outside [0, 1], a zero or non-finite light,
 * a non-finite background, slab_frames < 0, a face index of faces_host outside [0, V) and a workspace that is too small. */
#define EMPOSE_RENDER_MAX_IMAGE 2048
#define EMPOSE_RENDER_COLOR_UNIFORM 0
#define EMPOSE_RENDER_COLOR_VERTEX 1
#define EMPOSE_RENDER_COLOR_FRAME 2
typedef struct {
  int T, V, n_faces, H, W;
  const float* vertices; const int* faces; const int* faces_host;
  const float* normals; const float* colors; int color_mode;
  const float* cam_R; const float* cam_t; int camera_per_frame;
  float fx, fy, cx, cy, near;
  float light[3]; float ambient; float background[3];
  int slab_frames;
  unsigned char* rgb; int* face_id; float* depth;
} empose_render_desc;
size_t empose_render_workspace_bytes(int T, int V, int H, int W);
int empose_render_meshes(const empose_render_desc* desc, void* workspace, size_t workspace_bytes, empose_stream_t stream);

/* ---- overlay primitives in rendered frames (new in this library) -------------------------------- */
/* A per-pixel analytic ray caster that draws thin solid primitives -- a skeleton, sensor tripods, residuals -- into the
 * frames empose_render_meshes produced, depth-tested against the mesh (csrc/overlay.hip: two launches per slab of frames,
 * no atomics).  The definition is this library's own:
 *   primitive one type, the CAPSULE: all points within `radius` of the segment a - b, world coordinates.  a == b in all
 *             three components is a sphere.  A frame has P of them: seg_a, seg_b [T][P][3], radius [P] or, radius_per_frame
 *             != 0, [T][P], colors [P][3] in [0, 1].  A primitive is SKIPPED in a frame when its radius there is not > 0 or
 *             a component of a, b or the radius is not finite (how a missing sensor is left out: radius 0).
 *   camera    that of empose_render_meshes: p_c = R p + t, one camera or one per frame; the ray of the pixel of row i,
 *             column j is s d with d = ((j + 0.5 - cx) / fx, (i + 0.5 - cy) / fy, 1), so the ray parameter s IS camera-space
 *             Z, the quantity empose_render_meshes writes to `depth`.
 *   hit       of one primitive at one pixel: where the ray enters the union of the sphere about a_c, the sphere about b_c
 *             and the open side surface of the cylinder between them -- the smaller root of each quadratic where its
 *             discriminant is >= 0; the side root only where the leading coefficient is > 0 and the axial coordinate of
 *             the hit lies strictly inside (0, |b - a|^2); s is the smallest of those that exist (a sphere has the one).
 *             s <= near: the primitive does not cover the pixel (no clipping, no view from inside).  The quadratics are
 *             formed about the point of the ray at the depth of the segment's midpoint, not about the eye.
 *   pixel     (s*, id*) is the lexicographic minimum of (s, primitive index) over the frame's primitives: the nearest wins,
 *             the lower index an exact tie.  prim_id = id* or -1, prim_depth = s* or +inf (both optional, both independent
 *             of the mesh).  Without a hit rgb keeps its bytes.  Else n = (hit point - nearest point of the segment) /
 *             radius in camera space and c = colour (ambient + (1 - ambient) |n . l|), `light` as for the mesh.  The hit
 *             is VISIBLE when mesh_depth is NULL or s* < mesh_depth there, strictly (a tie goes to the mesh; +inf never
 *             hides): rgb = clamp(floor(255 c + 0.5)).  Hidden: rgb = clamp(floor((1 - alpha) rgb + alpha 255 c + 0.5))
 *             with alpha = hidden_alpha; 0 leaves the bytes as they are (the plain depth test), 1 gives what no
 *             mesh_depth gives (x-ray).  Only the nearest primitive is considered: there are no layers.
 * Every pixel depends on its own frame alone, nothing is summed: a second call gives the same bits, and a frame gives the
 * same bits alone, inside a batch and on either side of a slab edge.  P is at most EMPOSE_OVERLAY_MAX_PRIMS, H and W at
 * most EMPOSE_RENDER_MAX_IMAGE.  Frames go in slabs (slab_frames of them, 0: what fits 16 MB of workspace, at most 4096; a
 * larger value is lowered to that), so empose_render_overlay_workspace_bytes(T, P, H, W) -- the camera-space primitives
 * and their screen boxes of one slab; 0 for sizes the call refuses -- is bounded whatever T is.  The screen boxes only
 * bound the work (they are conservative) and are no part of the definition.
 * All pointers are device memory.  The call is asynchronous on `stream`: it never synchronises, allocates or copies.
 * Returns EMPOSE_EINVAL, before any GPU work, for a NULL descriptor, seg_a, seg_b, radius, colors, cam_R, cam_t, rgb or
 * workspace, T, P, H or W <= 0, P or the image above its cap, hidden_alpha or ambient outside [0, 1], fx, fy, cx, cy not
 * finite or fx, fy zero, near <= 0 or not finite, a zero or non-finite light, slab_frames < 0 and a workspace that is too
 * small. */
#define EMPOSE_OVERLAY_MAX_PRIMS 4096
typedef struct {
  int T, P, H, W;
  const float* seg_a; const float* seg_b; const float* radius; int radius_per_frame; const float* colors;
  const float* cam_R; const float* cam_t; int camera_per_frame;
  float fx, fy, cx, cy, near;
  float light[3]; float ambient; float hidden_alpha;
  const float* mesh_depth;
  int slab_frames;
  unsigned char* rgb; int* prim_id; float* prim_depth;
} empose_overlay_desc;
size_t empose_render_overlay_workspace_bytes(int T, int P, int H, int W);
int empose_render_overlay(const empose_overlay_desc* desc, void* workspace, size_t workspace_bytes, empose_stream_t stream);

/* ---- point-to-mesh queries (new in this library) ------------------------------------------------ */
/* For Q query points in each of T frames, the closest point of the frame's triangle mesh (V vertices per frame, one table
 * of F faces) and, want_inside != 0, whether the point lies inside the mesh (csrc/surface_query.hip: one launch, a
 * workgroup per frame and block of 12 queries, the frame's vertices in LDS).  Both definitions are this library's own:
 *   closest   c(p, f), the closest point of the closed triangle f to p, in fp32 by Voronoi regions (Ericson, Real-Time
 *             Collision Detection 5.1.5) tried in the order vertex 0, vertex 1, edge 01, vertex 2, edge 02, edge 12,
 *             interior; every comparison includes its boundary, so a face without area ends in an edge or a vertex; a
 *             quotient whose denominator is not positive counts as 0: no NaN from finite input.  d2(p, f) = |p - c|^2.
 *   result    the face with the lowest fp32 d2, the lowest face id on an exact tie -- an integer min over the 64-bit keys
 *             (bits of d2) << 32 | face id, no floating-point atomics.  dist = sqrt(d2); bary: the weights of c on the
 *             face's corners in the face's own order, each >= 0; closest = c.
 *   inside    the parity of the faces the ray from p along +z crosses.  A face counts when (a) the projection of p on the
 *             xy plane lies in the projected triangle under a half-open rule and (b) the ray meets the face's plane
 *             above p.  All of it in float64 on the fp32 coordinates (the values round; no exact sign is claimed).  The
 *             edge function of an edge is formed from its
 *             endpoint with the lower vertex id to the one with the higher, e = (hi.x - lo.x) (p.y - lo.y) - (hi.y - lo.y)
 *             (p.x - lo.x), and negated for the face that runs it the other way; a face whose projected area (the edge
 *             function of edge 01 at corner 2) is 0 never counts; otherwise the three values w are oriented by the sign
 *             of the area, and p is covered where every w > 0, or w == 0 on an edge the face owns: one that runs down in
 *             y, or level and towards +x, in the oriented direction (the side the point displaced by (+eps, +eps^2) falls
 *             on).  (b): (w0 (z2 - p.z) + w1 (z0 - p.z)) + w2 (z1 - p.z) > 0, w_k the value of the edge opposite corner
 *             k + 2.  A ray through a shared edge or vertex of a closed mesh is so counted once per crossing.  On a mesh
 *             that is not closed, or that intersects itself, the flag follows the same rule and means nothing.
 *   masked    mask [T][Q] (or NULL: none): a query whose mask is 0 gives dist +inf, face -1, bary = closest = 0,
 *             inside 0, and its coordinates -- anything, NaN included -- are never read into arithmetic.
 * A (query, face) pair is evaluated by one function whatever lane or workgroup holds it, and min and xor are exact in any
 * order: a second call gives the same bits, and a query gives the same bits whatever T is and whatever other queries
 * the frame holds.  face, bary, closest and inside are optional (NULL), inside is required with want_inside.  T is at most
 * EMPOSE_SURFACE_MAX_FRAMES per call (a workgroup per frame in one grid dimension), V at most
 * EMPOSE_SURFACE_MAX_VERTICES, F at most EMPOSE_SURFACE_MAX_FACES, Q at most EMPOSE_SURFACE_MAX_QUERIES; a frame of up to
 * 12 288 vertices is staged in LDS, a larger one is gathered from L2 by the same code.  faces_host is a host copy of the
 * device table faces_dev and is checked against [0, V) on every call (the kernel clamps an index in any case).  All
 * other pointers are device memory.  empose_surface_query_workspace_bytes is 0 for every shape (a frame's partial results
 * are combined inside its workgroup) and workspace may then be NULL.  The call is asynchronous on `stream`: it never
 * synchronises, allocates or copies.  Returns EMPOSE_EINVAL, before any GPU work, for a NULL descriptor, vertices, points,
 * faces_host, faces_dev or dist, T, V, F or Q <= 0 or above its cap, want_inside without inside, and a face index outside
 * [0, V). */
#define EMPOSE_SURFACE_MAX_FRAMES (1 << 22)
#define EMPOSE_SURFACE_MAX_VERTICES (1 << 24)
#define EMPOSE_SURFACE_MAX_FACES (1 << 26)
#define EMPOSE_SURFACE_MAX_QUERIES 4096
typedef struct {
  int T, V, F, Q;
  const float* vertices; const int* faces_host; const int* faces_dev;
  const float* points; const float* mask; int want_inside;
  float* dist; int* face; float* bary; float* closest; unsigned char* inside;
} empose_surface_desc;
size_t empose_surface_query_workspace_bytes(int T, int V, int F, int Q);
int empose_surface_query(const empose_surface_desc* desc, void* workspace, size_t workspace_bytes, empose_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* EMPOSE_HIP_H_ */
