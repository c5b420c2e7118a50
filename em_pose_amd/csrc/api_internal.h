// What the pieces of the C ABI (api.hip, api_model.hip, api_lstm.hip, api_train.hip, api_mesh.hip, api_fit.hip, ...) share: the error
// state, the profiler, workspace carving and upload, the packed model, and the LSTM dispatcher.  Host code only.
#pragma once
#include "../../include/empose_hip.h"
#include "gemm_kernels.h"
#include "mlp_kernels.h"
#include "smpl_kernels.h"

#include <cstring>
#include <vector>

namespace empose {
namespace api __attribute__((visibility("hidden"))) {

// ---- errors ---------------------------------------------------------------------------------------------------
int fail(int code, const char* fmt, ...);   // sets the message empose_last_error() returns; returns `code`

#define HIP_TRY(expr)                                                                            \
  do {                                                                                           \
    hipError_t e_ = (expr);                                                                      \
    if (e_ != hipSuccess) return fail(EMPOSE_EHIP, "%s: %s", #expr, hipGetErrorString(e_));       \
  } while (0)

#define HIP_CHECK(expr, msg)                                                                     \
  do {                                                                                           \
    hipError_t e_ = (expr);                                                                      \
    if (e_ != hipSuccess) return fail(EMPOSE_EHIP, msg ": %s", hipGetErrorString(e_));           \
  } while (0)

#define TRY(expr)            \
  do {                       \
    int rc_ = (expr);        \
    if (rc_ != EMPOSE_OK) return rc_; \
  } while (0)

// A poll of a cooperative kernel launched by an EARLIER call gave up (that call's outputs are NaN): reported by every entry
// point that launches or consumes such kernels -- the recurrences and, round 6, the training layers (empose_mlp_train_*,
// empose_lstm_train_*) -- without synchronising (the counter is a host-mapped word), and STICKY until
// empose_async_status() has reported and cleared it.
int earlier_poll_timeouts();

// ---- optional per-launch timing (HIP events on the launch stream), used by bench.py for the roofline numbers ---------
enum ProfTag { P_PACK = 0, P_LSTM_STEP, P_HEADS, P_UPDATE_FEAT, P_BLEND_GEMM, P_CHAIN, P_BLEND_T_GEMM,
               P_ROD_BWD, P_MLP_IN, P_MLP_HIDDEN, P_MLP_OUT, P_MLP_FUSED, P_INIT_MLP, P_COPY, P_EVENT_PAIR, P_END, P_NTAGS };
void prof_mark(int tag, hipStream_t stream);
void prof_end_forward(hipStream_t stream);   // P_END, and in single-kernel mode the empty calibration pair

// ---- workspace carving and upload -----------------------------------------------------------------------------
inline size_t align_up(size_t x, size_t a = 256) { return (x + a - 1) / a * a; }

struct Carver {
  char* base;
  size_t off = 0;
  explicit Carver(void* p) : base(static_cast<char*>(p)) {}
  float* f(size_t count) {
    float* r = base ? reinterpret_cast<float*>(base + off) : nullptr;
    off += align_up(count * sizeof(float));
    return r;
  }
  // The bytes a layout takes: `carve` run on a null base (the workspace-size queries).
  template <typename Carve>
  static size_t measure(Carve carve) {
    Carver c(nullptr);
    carve(c);
    return c.off;
  }
};

template <typename T>
int upload(std::vector<void*>& allocs, const T* host, size_t count, T** dev) {
  *dev = nullptr;
  if (count == 0) return EMPOSE_OK;
  if (!host) return fail(EMPOSE_EINVAL, "null host pointer in model descriptor");
  void* p = nullptr;
  HIP_TRY(hipMalloc(&p, count * sizeof(T)));
  allocs.push_back(p);
  HIP_TRY(hipMemcpy(p, host, count * sizeof(T), hipMemcpyHostToDevice));
  *dev = static_cast<T*>(p);
  return EMPOSE_OK;
}

// ---- three bf16 pieces per weight (bf16x3.h) ------------------------------------------------------------------------
// Round to nearest even; Inf and NaN pass through as they are.
inline unsigned short bf16_round(float x) {
  unsigned u;
  std::memcpy(&u, &x, 4);
  if ((u & 0x7f800000u) == 0x7f800000u) return (unsigned short)(u >> 16);   // inf / nan: as they are
  u += 0x7fffu + ((u >> 16) & 1u);
  return (unsigned short)(u >> 16);
}
inline float bf16_value(unsigned short h) {
  const unsigned u = (unsigned)h << 16;
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}
// w = p[0] + p[1] + p[2], every piece the round-to-nearest bf16 of what the previous ones leave: 8 + 8 + 8 mantissa bits,
// all of an fp32's 24.
inline void split3(float w, unsigned short p[3]) {
  p[0] = bf16_round(w);
  const float r = w - bf16_value(p[0]);
  p[1] = bf16_round(r);
  p[2] = bf16_round(r - bf16_value(p[1]));
}
// B operands of the three-piece kernels on the host: `n_frag` fragments of 3 x 512 bf16 -- piece 0, 1, 2 of the same 64 lanes x
// 8 consecutive k, 1 KB each -- in the order the caller's layout gives them.  `src(frag, lane, &row, &k0)` names what a lane
// of a fragment owns: row[k0 .. k0 + 7] (k0 = k-step * 16 + (lane >> 5) * 8 for the 32x32x16 instruction,
// k-step * 32 + (lane >> 4) * 8 for the 16x16x32 one); it returns false for a lane that owns nothing.  What is not
// written -- those lanes and k >= K -- is zero.
template <typename Src>
std::vector<unsigned short> pack_fragments_x3(size_t n_frag, int K, Src src) {
  std::vector<unsigned short> buf(n_frag * 3 * 512, 0);
  for (size_t f = 0; f < n_frag; ++f)
    for (int lane = 0; lane < 64; ++lane) {
      const float* row = nullptr;
      int k0 = 0;
      if (!src(f, lane, &row, &k0)) continue;
      for (int e = 0; e < 8 && k0 + e < K; ++e) {
        unsigned short p[3];
        split3(row[k0 + e], p);
        const size_t at = f * 3 * 512 + (size_t)lane * 8 + e;
        buf[at] = p[0]; buf[at + 512] = p[1]; buf[at + 1024] = p[2];
      }
    }
  return buf;
}
// A table of bf16 pieces goes to the device as it is; `out` is typed as the kernels that read it take it.
template <typename T>
int upload_bf16(std::vector<void*>& allocs, const std::vector<unsigned short>& buf, T** out) {
  unsigned short* dev = nullptr;
  TRY(upload(allocs, buf.data(), buf.size(), &dev));
  *out = reinterpret_cast<T*>(dev);
  return EMPOSE_OK;
}

// ---- the packed model -----------------------------------------------------------------------------------------
// A packed Linear(+BN)(+PReLU): device weight and the per-column epilogue (scale, shift).
struct Dense {
  int in_dim = 0, out_dim = 0;
  float* w = nullptr;      // [out][in]
  float* frag[FUSED_FORMS] = {};   // the same weights in the fragment order of each FusedForm (mlp_kernels.h), only for MLP layers
  float* wexp = nullptr;   // [out] the inverse of the power-of-two scale each output column's pair16 pieces carry
  float* scale = nullptr;  // nullptr => 1
  float* shift = nullptr;  // bias (and folded BN)
  int act = 0;
  float slope = 0.f;
};

struct Mlp {
  int n_layers = 0, skip = 0;
  Dense layers[EMPOSE_MAX_DENSE];
};

// ---- operand set-ups the host drivers share ---------------------------------------------------------------------
// One product with no epilogue: C[M][N] = A . W^T.
inline GemmProb plain_prob(const float* A, int lda, const float* W, int ldw, float* C, int ldc, int M, int N, int K) {
  GemmProb p;
  p.A = A; p.lda = lda; p.W = W; p.ldw = ldw; p.C = C; p.ldc = ldc;
  p.M = M; p.N = N; p.K = K;
  p.scale = nullptr; p.shift = nullptr; p.resid = nullptr; p.ldr = 0; p.act = 0; p.slope = 0.f;
  return p;
}
// A packed layer on M rows: the product with the layer's epilogue.
inline GemmProb linear_prob(const float* A, int lda, const Dense& d, float* C, int ldc, int M) {
  GemmProb p = plain_prob(A, lda, d.w, d.in_dim, C, ldc, M, d.out_dim, d.in_dim);
  p.scale = d.scale; p.shift = d.shift; p.act = d.act; p.slope = d.slope;
  return p;
}
// Plain evaluation: the caller's rows are read in place (no update: the kernel does not write them back), no copies.
// Where rot / feat / theta_t go, T, F and the Rodrigues convention are the evaluation's to fill in.
inline FeatArgs plain_feat_args(const float* theta, int ld_theta, const float* beta, int ld_beta) {
  FeatArgs fa;
  fa.theta = const_cast<float*>(theta); fa.ld_theta = ld_theta; fa.beta = const_cast<float*>(beta); fa.ld_beta = ld_beta;
  fa.d_theta = nullptr; fa.d_beta = nullptr; fa.theta_step = 0.f; fa.beta_keep = 1.f; fa.beta_step = 0.f;
  fa.shape_avg = 0;
  fa.out_theta = fa.out_beta = fa.out_theta2 = fa.out_beta2 = nullptr;
  return fa;
}

// The three-piece bf16 weights of a stack, per unit, in the fragment order of one family of step kernels (api_lstm.hip
// LSTM_LAYOUTS): chain -- lstm_x3.hip, lstm_rows_x3.hip; mid -- lstm_mid_x3.hip, lstm_midseq_x3.hip; mid16 -- lstm_mid16_x3.hip,
// lstm_chain16_x3.hip
enum LstmLayout { LSTM_CHAIN = 0, LSTM_MID, LSTM_MID16, LSTM_N_LAYOUTS };
struct LstmW3 { unsigned short* ih[8] = {}; unsigned short* hh[8] = {}; };
struct Lstm {   // unit u = layer * dirs + direction
  int num_layers = 0, input_size = 0, H = 0, dirs = 1;
  float* w_ih[8] = {};
  float* w_hh[8] = {};
  float* bias[8] = {};   // b_ih + b_hh
  LstmW3 w3[LSTM_N_LAYOUTS];   // uni-directional stacks with H % 32 == 0 only, else null
  // lstm_chain16_pair_kernel (LSTM_MID16 order, three-piece stride; same stacks): per gate column n one power-of-two scale
  // s_n from the column of [W_ih | W_hh].  pair: two f16 pieces of w s_n -- W_hh, and W_ih of layers >= 1; wide: three
  // bf16 pieces of w s_n 2^14 -- W_ih of layer 0, and every W_hh for the step that consumes a caller's h0
  LstmW3 w_pair, w_wide;
  float* inv_scale[8] = {};    // [4H] 2^-14 / s_n
};

// Uploads an LSTM stack (api_lstm.hip): fp32 weights, summed biases and, for uni-directional stacks with H % 32 == 0, the
// three-piece bf16 weights in every layout of the table above and the scaled pieces of lstm_chain16_pair_kernel.
int pack_lstm(std::vector<void*>& allocs, const empose_lstm_desc& r, int dirs, const float* const* w_ih,
              const float* const* w_hh, const float* const* b_ih, const float* const* b_hh, Lstm* out);

// ---- the LSTM dispatcher (api_lstm.hip) ------------------------------------------------------------------------
// What one call does, decided in ONE place (plan_lstm, over plan_lstm_f32 for the fp32 kernels) from the stack, the shape
// and the options of the moment: which whole-sequence kernels get buffers (persist and seq by shape alone, midseq by shape
// and options); the cooperative launches to try, in order -- listed only where the kernel covers the shape and would
// really be tried; each may still report done = false at run time (its workgroups cannot all be resident) -- and the step
// kernel that runs when none finished, with its weight layout and how it treats the state of new sequences.
// wave: fp32, the kernel LstmPlan::wave names; chain16_pair: two f16 pieces where the operand is the kernel's own; else
// three bf16 pieces
enum class LstmStep { wave, chain_x3, rows_x3, mid_x3, mid16_x3, chain16_x3, chain16_pair };
// the fp32 step kernels: lstm_small_kernel, lstm_fewrows_kernel (lstm_fewrows.hip), lstm_mid_kernel, lstm_chain_kernel
enum class LstmWave { small, fewrows, mid, chain };
enum class LstmCoop { persist, seq, midseq };   // lstm_persist_kernel (small), lstm_seq_kernel (large), lstm_midseq_x3.hip
// What the fp32 kernels are chosen by: the units of one launch (a stacked wavefront's layers, or the two directions of a
// bidirectional layer) and the width of each one's input
struct LstmShape { int B, F, H, n_units; int in_k[4]; bool stacked; };
struct LstmPlan {
  bool persist = false;   // exchange words of lstm_persist_kernel
  bool seq = false;       // third hidden buffers + counters of lstm_seq_kernel
  bool midseq = false;    // hidden-state plane sets + progress counters of lstm_midseq_x3.hip
  bool x3 = false;        // the bf16 piece planes of the inputs and hidden states (a three-piece step kernel or midseq)
  int n_coop = 0; LstmCoop coop[3];
  LstmStep step = LstmStep::wave; LstmLayout layout = LSTM_CHAIN;   // (the layout of the three-piece step kernel)
  LstmWave wave = LstmWave::chain;   // the fp32 step kernel (step == wave)
  // lstm_chain_kernel and the three-piece chain kernels: a workgroup walks all active units (the tiles alone fill the CUs:
  // equal work per workgroup) instead of one
  bool chain_all_units = false;
  // three-piece steps on new sequences (option lstm_state_direct): the zero hidden-state planes by one fill, and on the
  // chain kernels h_n / c_n stored by the last step of each layer
  bool zero_planes = false, state_direct = false;
  bool skip_dead = false;   // chain kernels, option lstm_skip_dead: zero-state k-steps and unread fp32 state traffic left out
};

struct LstmWs {
  float* h[8][2];
  float* c[8];
  float* yb[2];   // [B][F][2H] ping-pong between the layers of a bidirectional stack
  float* xch;     // exchange words of the whole-sequence small-batch kernel (lstm_persist_kernel), or nullptr
  float* h3[8];   // third hidden-state buffer per unit + counters of the whole-sequence large-batch kernel, or nullptr
  unsigned* seq_cnt;
  // lstm_x3.hip: the stored input of every time step and the hidden states (ping-pong) as bf16 piece planes, or nullptr
  unsigned short* x3; size_t x3_t_stride;
  unsigned short* a3[8][2];
  // lstm_midseq_x3.hip: [F + 1] sets of hidden-state planes per layer and the progress counters, or nullptr
  unsigned short* xa[8];
  unsigned* midseq_flags;
};
LstmWs carve_lstm_of(Carver& c, const Lstm& r, int B, int F);
// State layout of h0/c0/h_n/c_n: [num_layers * dirs][B][H], unit u = layer * dirs + direction (PyTorch's order).
int run_lstm(const Lstm& r, int B, int F, const float* x, int ldx, const int* seq_lengths, const float* h0,
             const float* c0, float* y, float* h_n, float* c_n, const LstmWs& ws, hipStream_t stream);

// What empose_smpl_sensors_fwd_bwd runs once its arguments are checked (api_model.hip): plan_smpl for this T and request, then
// run_smpl_eval.  The sensor fit (api_fit.hip) evaluates through it, so its residual gradient has the bits of the public
// call at the same T.  tgt == nullptr: forward only.  workspace: empose_smpl_workspace_bytes(m, T).
int smpl_sensors_eval(const empose_model* m, int T, int F, const float* theta, int ld_theta, const float* beta, int ld_beta,
                      const float* offset_r, const float* offset_t, const float* tgt, int ld_tgt, const float* frame_scale,
                      float* pos, float* ori, float* joints, float* g_theta, int ld_g, float* g_beta, int ld_gb,
                      void* workspace, hipStream_t stream);

// Frames per pass of the virtual-sensor reverse (api_mesh.hip), shared by empose_sample_sensors_vjp (api_sample.hip).
int sensors_vjp_slab(int T, int M);

}  // namespace api
}  // namespace empose

struct empose_model {
  std::vector<void*> allocs;
  empose::SmplTables tab;
  float* wc_frag = nullptr;    // tab.wc / tab.wct in MFMA fragment order (row-block GEMM)
  float* wct_frag = nullptr;
  int n_markers = 12;
  int marker_idx[12];
  int used_slot[12];
  int N = 4;
  float step = 0.1f;
  int shape_avg = 1, use_gradient = 1, rnn_init = 1;
  int d_in = 144, d_x = 296;
  empose::api::Lstm rnn;
  empose::api::Dense pose_head, shape_head;
  float* heads_frag = nullptr;   // both heads stacked ([66 + 10][H]) in fragment order, and their stacked bias
  float* heads_frag3 = nullptr;  // ... as three bf16 pieces per weight (x3_rows_layer)
  float* heads_bias = nullptr;
  empose::api::Mlp pose_init, shape_init, pose_iter, shape_iter;
  int hidden_max = 0;
  int any_skip = 0;
  int smpl_only = 0;
  int rod_conv = 0;            // EMPOSE_RODRIGUES_*
  // frame-per-lane path (smpl_tile.hip): tables, the blend matrix with per-patch vertex copies in fragment order
  int tile_ok = 0, ncp2 = 0, tile_nloc = 0, tile_nbl = 0, tile_j_off2 = 0;   // (host copies of TileTables fields)
  empose::TileTables* tile_tab = nullptr;
  float* wc2_frag = nullptr;   // [ncp2][200]
  float* wc2t_frag = nullptr;  // [200][ncp2]
  float* wc2_frag3 = nullptr;  // the same two as three bf16 pieces per weight (x3_rows_layer)
  float* wc2t_frag3 = nullptr;
};

struct empose_rnn {
  std::vector<void*> allocs;
  empose::api::Lstm rnn;
};
