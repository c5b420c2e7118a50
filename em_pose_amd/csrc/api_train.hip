// C ABI (include/empose_hip.h), training building blocks: plain products, BatchNorm + PReLU, A^T B, transpose,
// input packing, the LGD update / cotangent / loss kernels, Adam; one MLP (or both update networks) in training mode.
#include "api_internal.h"
#include "gemm_kernels.h"
#include "options.h"
#include "smpl_kernels.h"
#include "train_kernels.h"

#include <cmath>

using namespace empose;
using namespace empose::api;

// ---- one MLP in training mode -------------------------------------------------------------------------------------
namespace {
int check_mlp_params(const empose_mlp_params* p) {
  if (!p) return fail(EMPOSE_EINVAL, "null argument");
  if (p->n_layers < 2 || p->n_layers > EMPOSE_MAX_DENSE || p->in_dim <= 0 || p->hidden <= 0 || p->out_dim <= 0 ||
      p->in_dim % 4 != 0 || p->hidden % 4 != 0)
    return fail(EMPOSE_EINVAL, "unsupported MLP configuration");
  for (int l = 0; l < p->n_layers; ++l) {
    if (!p->weight[l] || !p->bias[l]) return fail(EMPOSE_EINVAL, "null MLP parameter");
    if (l < p->n_layers - 1 && (!p->bn_weight[l] || !p->bn_bias[l] || !p->prelu[l]))
      return fail(EMPOSE_EINVAL, "the training MLP needs BatchNorm + PReLU on every hidden layer");
  }
  return EMPOSE_OK;
}
// HIP_CHECK with a message chosen at run time
#define HIP_CHECK_AS(expr, what)                                                                 \
  do {                                                                                           \
    hipError_t e_ = (expr);                                                                      \
    if (e_ != hipSuccess) return fail(EMPOSE_EHIP, "%s: %s", what, hipGetErrorString(e_));       \
  } while (0)

struct MlpTrainWs {
  float* d[2];       // [M][hidden] cotangent ping-pong
  float* wt;         // transposed weight [hidden][max(hidden, out_pad)]
  float* atb; size_t atb_floats; float* bn; float* slope_partial; int* counter;
  float* part; float* coef;   // fused path: per-row-block partial sums, BatchNorm-reverse coefficients [3][H]
  // one-launch layers (train_cols.hip): mailbox words, zeroed once per call
  unsigned long long* mbox; size_t mbox_bytes;
};
size_t cols_zero_bytes(const empose_mlp_params* p) {
  return cols_mailbox_words(p->hidden > p->out_dim ? p->hidden : p->out_dim) * sizeof(unsigned long long);
}
// every A^T B product of one MLP over M rows: (H, in_dim), (H, H), (out_dim, H)
size_t mlp_atb_floats(const empose_mlp_params* p, int M) {
  return atb_workspace_floats_max(M, {{p->hidden, p->in_dim}, {p->hidden, p->hidden}, {p->out_dim, p->hidden}});
}
MlpTrainWs carve_mlp_train(Carver& c, const empose_mlp_params* p, int M) {
  MlpTrainWs w;
  const int H = p->hidden, op = (p->out_dim + 3) & ~3;
  w.d[0] = c.f((size_t)M * H); w.d[1] = c.f((size_t)M * H);
  w.wt = c.f((size_t)H * (H > op ? H : op));
  w.atb_floats = mlp_atb_floats(p, M);
  w.atb = c.f(w.atb_floats + 64);
  w.bn = c.f(bn_prelu_workspace_floats(M, H) + 64);
  w.slope_partial = c.f((size_t)(H + 31) / 32 + 8);
  w.counter = reinterpret_cast<int*>(c.f(64));
  w.part = c.f(bn_fused_partial_floats(M, H) + 64);
  w.coef = c.f((size_t)3 * H + 64);
  w.mbox_bytes = cols_zero_bytes(p);
  w.mbox = reinterpret_cast<unsigned long long*>(c.f(w.mbox_bytes / sizeof(float)));
  return w;
}

// Layer l as the product out [M][N] = in [M][K] . W [N][K]^T: `lda` the leading dimension of its input (the network
// input's for layer 0), `out_pad` that of its output cotangent in the stash (the last layer's padded to a multiple of 4).
struct LayerDims { bool last; int N, K, lda, ldw, out_pad; };
LayerDims layer_dims(const empose_mlp_params* p, int l, int ldx) {
  LayerDims d;
  d.last = l == p->n_layers - 1;
  d.N = d.last ? p->out_dim : p->hidden;
  d.K = l == 0 ? p->in_dim : p->hidden;
  d.lda = l == 0 ? ldx : p->hidden;
  d.ldw = d.K;
  d.out_pad = d.last ? (p->out_dim + 3) & ~3 : p->hidden;
  return d;
}

// How one MLP trains on M rows, decided once per entry point: which family of launches runs and, the one place that
// knows it, where everything sits in the save buffer and the stash.  One record per hidden layer:
//   layout 1, passes  z [M][H] | a [M][H] | mean [H] | rstd [H]        GEMM + BatchNorm / PReLU launches (round 2), and
//                                                                      the one-launch layers of train_cols.hip (round 5)
//   layout 2, fused   y [M][H] | mean | rstd | s | t                   the passes folded into the GEMMs (train_fused.hip):
//                     the activations are not stored, consumers re-form a = PReLU(s y + t) while they stage the operand
//   layout 3, epi     y [M][H] | a [M][H] | mean | rstd | s | t        statistics from the GEMM epilogues, ONE
//                     combine-and-apply launch per layer and direction (bn_finish_*): GEMM + 1 launch instead of GEMM + 3
// Options: "train_fused" 0 never (default; gradient parity is tested, but at 256 windows the step is no faster: 701-711 k
// against 705-720 k frames/s), "train_epi" 1 (default); both: 1 above BN_SINGLE_PASS_ROWS rows, 2 always (tests);
// "train_fused" takes precedence.  empose_mlp_params::save_layout != 0: the layout chosen when the step's forward ran wins
// over the options of the moment.
// Stash of one application: dZ of the hidden layers [M][H] each, then a copy of d_out [M][out_pad].
struct MlpPlan {
  const empose_mlp_params* p;
  int M, H, L, op;
  int layout;
  // At the reference's training batch a layer is one launch: product, BatchNorm and PReLU of both update networks in
  // train_cols.hip (option "train_cols": 0 never, 1 up to COLS_MAX_ROWS rows).  Reads and writes layout 1; not pinned by
  // save_layout.  (Asks the device: only the entry points that launch, and empose_mlp_train_uses_weight_t, read it.)
  bool cols() const {
    if (options().train_cols == 0 || M > COLS_MAX_ROWS || layout != 1) return false;
    return cols_launchable(H > p->out_dim ? H : p->out_dim, 2);
  }
  size_t planes() const { return layout == 2 ? 1 : 2; }
  size_t layer_floats() const { return planes() * M * H + (size_t)(layout == 1 ? 2 : 4) * H; }
  size_t save_floats() const { return (size_t)(L - 1) * layer_floats(); }
  template <typename F> F* pre(F* save, int l) const { return save + (size_t)l * layer_floats(); }   // z / y
  template <typename F> F* act(F* save, int l) const { return pre(save, l) + (size_t)M * H; }        // (not in layout 2)
  template <typename F> F* mean(F* save, int l) const { return pre(save, l) + planes() * M * H; }
  template <typename F> F* rstd(F* save, int l) const { return mean(save, l) + H; }
  template <typename F> F* s(F* save, int l) const { return mean(save, l) + 2 * H; }                 // (layouts 2, 3)
  template <typename F> F* t(F* save, int l) const { return mean(save, l) + 3 * H; }
  size_t stash_floats() const { return (size_t)M * ((size_t)(L - 1) * H + op); }
  template <typename F> F* stash_slot(F* stash, int l) const { return stash + (size_t)M * l * H; }   // l = L - 1: d_out
};
MlpPlan mlp_plan(const empose_mlp_params* p, int M) {
  MlpPlan pl;
  pl.p = p; pl.M = M; pl.H = p->hidden; pl.L = p->n_layers; pl.op = (p->out_dim + 3) & ~3;
  auto on = [&](int opt) {
    return opt != 0 && (opt == 2 || M > BN_SINGLE_PASS_ROWS) && p->hidden % 4 == 0 && p->in_dim % 4 == 0;
  };
  if (p->save_layout) pl.layout = p->save_layout == 2 ? 2 : (p->save_layout == 3 ? 3 : 1);
  else pl.layout = on(options().train_fused) ? 2 : (on(options().train_epi) ? 3 : 1);
  return pl;
}
bool mlp_cols_pairable(const MlpPlan& a, const MlpPlan& b) {
  return a.L == b.L && a.H == b.H && a.p->bn_eps == b.p->bn_eps && a.p->bn_momentum == b.p->bn_momentum && a.cols() &&
         b.cols() && b.p->out_dim <= (a.H > a.p->out_dim ? a.H : a.p->out_dim);
}

// ---- what the sweeps share ----------------------------------------------------------------------------------------
hipError_t gemm_one(const float* A, int lda, const float* W, int ldw, float* C, int ldc, int M, int N, int K,
                    const float* scale, const float* shift, const float* resid, int ldr, int act, float slope,
                    hipStream_t stream) {
  GemmBatch b;
  b.count = 1;
  GemmProb& g = b.p[0];
  g.A = A; g.lda = lda; g.W = W; g.ldw = ldw; g.C = C; g.ldc = ldc; g.M = M; g.N = N; g.K = K;
  g.scale = scale; g.shift = shift; g.resid = resid; g.ldr = ldr; g.act = act; g.slope = slope;
  return launch_gemm(b, stream);
}
// Weight gradients deferred: keep d_out for empose_mlp_train_wgrad (no copy when the caller produced it in its stash slot
// already, include/empose_hip.h)
int stash_d_out(const MlpPlan& pl, const float* d_out, int ld_dout, float* stash, hipStream_t stream) {
  float* slot = pl.stash_slot(stash, pl.L - 1);
  if (d_out != slot || ld_dout != pl.op) {
    HIP_CHECK(launch_axpby2d(pl.M, pl.op, 1.f, d_out, ld_dout, 0.f, nullptr, 0, slot, pl.op, stream), "stash");
  }
  return EMPOSE_OK;
}
// W_l^T [H][out_pad] for dA_{l-1} = dY_l W_l on the K-contiguous GEMM: the caller's copy (made once per step), else
// transposed into the workspace (the last layer's padding columns zero)
int weight_t_of(const MlpPlan& pl, int l, const MlpTrainWs& w, hipStream_t stream, const float** wt) {
  const empose_mlp_params* p = pl.p;
  *wt = p->weight_t[l];
  if (*wt) return EMPOSE_OK;
  const LayerDims d = layer_dims(p, l, 0);
  const int H = pl.H, op = pl.op;
  if (d.last) HIP_TRY(hipMemsetAsync(w.wt, 0, (size_t)H * op * sizeof(float), stream));
  HIP_CHECK(launch_transpose(p->weight[l], H, w.wt, d.out_pad, d.N, H, stream), "transpose");
  *wt = w.wt;
  return EMPOSE_OK;
}
// dW_l, db_l over n applications of the network: dy[s]^T in[s], with dy[s] the cotangent of layer l's product (leading
// dimension ld_dy) and in[s] the layer's input, x[s] or a_{l-1} in save[s].  Layout 2 stores y_{l-1} only: the product
// re-forms a_{l-1} from it and its (s, t) while it stages its B operand.  `segmented`: one product over the n row
// segments (M % 32 == 0, aligned operands); else one per application, added up.
int layer_wgrad(const MlpPlan& pl, int l, int n, bool segmented, const float* const* dy, int ld_dy, const float* const* x,
                int ldx, const float* const* save, const empose_mlp_grads* gr, int accumulate, float* ws, size_t ws_floats,
                const char* what, hipStream_t stream) {
  const LayerDims d = layer_dims(pl.p, l, ldx);
  const bool reform = pl.layout == 2 && l > 0;
  AtbArgs ab{};
  ab.lda = ld_dy; ab.ldb = d.lda; ab.C = gr->weight[l]; ab.ldc = d.K; ab.bias = gr->bias[l]; ab.N = d.N; ab.K = d.K;
  if (reform) { ab.b_mode = 1; ab.b_slope = pl.p->prelu[l - 1]; }
  auto fill = [&](int slot, int s) {
    ab.A_seg[slot] = dy[s];
    ab.B_seg[slot] = l == 0 ? x[s] : (reform ? pl.pre(save[s], l - 1) : pl.act(save[s], l - 1));
    ab.Bs_seg[slot] = reform ? pl.s(save[s], l - 1) : nullptr;
  };
  if (segmented) {
    for (int s = 0; s < n; ++s) fill(s, s);
    ab.n_seg = n; ab.seg_rows = pl.M;
  }
  for (int s = 0; s < (segmented ? 1 : n); ++s) {
    if (!segmented) fill(0, s);
    ab.A = ab.A_seg[0]; ab.B = ab.B_seg[0]; ab.M = segmented ? n * pl.M : pl.M; ab.accumulate = s > 0 ? 1 : accumulate;
    HIP_CHECK_AS(launch_gemm_atb(ab, ws, ws_floats, stream), what);
  }
  return EMPOSE_OK;
}

// ---- the forward sweeps ---------------------------------------------------------------------------------------------
// GEMM, then BatchNorm + PReLU as launches of their own (layout 1)
int fwd_passes(const MlpPlan& pl, const float* x, int ldx, float* out, int ld_out, float* save, const MlpTrainWs& w,
               hipStream_t stream) {
  const empose_mlp_params* p = pl.p;
  const int M = pl.M, H = pl.H;
  for (int l = 0; l < pl.L; ++l) {
    const LayerDims d = layer_dims(p, l, ldx);
    float* z = d.last ? out : pl.pre(save, l);
    HIP_CHECK(gemm_one(l == 0 ? x : pl.act(save, l - 1), d.lda, p->weight[l], d.ldw, z, d.last ? ld_out : H, M, d.N, d.K,
                       nullptr, p->bias[l], nullptr, 0, 0, 0.f, stream), "mlp forward gemm");
    if (d.last) break;
    BnPreluArgs a{};
    a.M = M; a.C = H; a.x = z; a.ldx = H; a.gamma = p->bn_weight[l]; a.beta = p->bn_bias[l]; a.slope = p->prelu[l];
    a.eps = p->bn_eps; a.momentum = p->bn_momentum; a.running_mean = p->bn_running_mean[l];
    a.running_var = p->bn_running_var[l]; a.num_batches_tracked = p->bn_num_batches[l];
    a.z = pl.act(save, l); a.ldz = H; a.save_mean = pl.mean(save, l); a.save_rstd = pl.rstd(save, l);
    a.workspace = w.bn;
    HIP_CHECK(launch_bn_prelu(a, false, stream), "bn_prelu forward");
  }
  return EMPOSE_OK;
}
// y_l = a_{l-1} W_l^T + b_l, the epilogue leaving the column statistics of y_l per row block (layouts 2 and 3).
// fused: a_{l-1} = PReLU(s y_{l-1} + t) is formed while the GEMM stages its A operand, and a small kernel turns the
// statistics into (mean, rstd, s, t);  epi: the GEMM reads the materialised a_{l-1}, and ONE launch turns the statistics
// into (mean, rstd, s, t), updates the running statistics and writes a_l = PReLU(s y_l + t).
int fwd_stats(const MlpPlan& pl, const float* x, int ldx, float* out, int ld_out, float* save, const MlpTrainWs& w,
              hipStream_t stream) {
  const empose_mlp_params* p = pl.p;
  const int M = pl.M, H = pl.H;
  const bool epi = pl.layout == 3;
  for (int l = 0; l < pl.L; ++l) {
    const LayerDims d = layer_dims(p, l, ldx);
    const bool transform = !epi && l > 0;
    TrainGemmArgs g{};
    g.A = l == 0 ? x : (epi ? pl.act(save, l - 1) : pl.pre(save, l - 1)); g.lda = d.lda; g.W = p->weight[l]; g.ldw = d.ldw;
    g.C = d.last ? out : pl.pre(save, l); g.ldc = d.last ? ld_out : H;
    g.M = M; g.N = d.N; g.K = d.K; g.bias = p->bias[l];
    if (transform) { g.a_s = pl.s(save, l - 1); g.a_t = pl.t(save, l - 1); g.a_slope = p->prelu[l - 1]; }
    g.part = w.part;
    const bool x3 = epi && !d.last && options().train_x3 != 0 && p->weight_x3[l] && gemm_train_x3_applicable(g.M, g.N, g.K);
    HIP_CHECK_AS(x3 ? launch_gemm_train_x3(g, p->weight_x3[l], 1, stream)
                    : launch_gemm_train(g, transform ? 1 : 0, d.last ? 0 : 1, stream),
                 epi ? "mlp forward gemm (statistics epilogue)" : "fused mlp forward gemm");
    if (d.last) break;
    auto statistics = [&](auto& c) {
      c.M = M; c.C = H; c.part = w.part; c.gamma = p->bn_weight[l]; c.beta = p->bn_bias[l];
      c.eps = p->bn_eps; c.momentum = p->bn_momentum; c.running_mean = p->bn_running_mean[l];
      c.running_var = p->bn_running_var[l]; c.num_batches_tracked = p->bn_num_batches[l];
      c.mean = pl.mean(save, l); c.rstd = pl.rstd(save, l); c.s = pl.s(save, l); c.t = pl.t(save, l);
    };
    if (epi) {
      BnFinishFwdArgs c{};
      statistics(c);
      c.y = pl.pre(save, l); c.ldy = H; c.act = pl.act(save, l); c.ld_act = H; c.slope = p->prelu[l];
      HIP_CHECK(launch_bn_finish_fwd(c, stream), "bn finish forward");
    } else {
      BnFusedFwdArgs c{};
      statistics(c);
      HIP_CHECK(launch_bn_fused_combine_fwd(c, stream), "fused bn combine");
    }
  }
  return EMPOSE_OK;
}
// One launch per layer for one network or a pair (train_cols.hip)
int mlp_fwd_cols(const MlpPlan* pls, int n, const float* x, int ldx, float* const* outs, const int* ld_outs,
                 float* const* saves, const MlpTrainWs& w, hipStream_t stream) {
  const int L = pls[0].L, M = pls[0].M;
  HIP_TRY(hipMemsetAsync(w.mbox, 0, w.mbox_bytes, stream));
  for (int l = 0; l < L; ++l) {
    const bool last = l == L - 1;
    ColsArgs a{};
    a.n_nets = n; a.M = M; a.eps = pls[0].p->bn_eps; a.momentum = pls[0].p->bn_momentum; a.tag = (unsigned)l + 1;
    a.mailbox = w.mbox;
    for (int i = 0; i < n; ++i) {
      const MlpPlan& pl = pls[i];
      const empose_mlp_params* p = pl.p;
      const LayerDims d = layer_dims(p, l, ldx);
      ColsNet& c = a.net[i];
      c.A = l == 0 ? x : pl.act(saves[i], l - 1); c.lda = d.lda;
      c.W = p->weight[l]; c.ldw = d.ldw; c.bias = p->bias[l];
      c.N = d.N; c.K = d.K;
      if (last) { c.out = outs[i]; c.ld_out = ld_outs[i]; continue; }
      c.gamma = p->bn_weight[l]; c.beta = p->bn_bias[l]; c.slope = p->prelu[l];
      c.running_mean = p->bn_running_mean[l]; c.running_var = p->bn_running_var[l]; c.num_batches = p->bn_num_batches[l];
      c.z = pl.pre(saves[i], l); c.ldz = pl.H; c.out = pl.act(saves[i], l); c.ld_out = pl.H;
      c.mean = pl.mean(saves[i], l); c.rstd = pl.rstd(saves[i], l);
    }
    HIP_CHECK(launch_cols(a, last ? 1 : 0, stream), "one-launch layer forward");
  }
  return EMPOSE_OK;
}

// ---- the reverse sweeps ---------------------------------------------------------------------------------------------
// With a stash the weight gradients are deferred (empose_mlp_train_wgrad) and dZ_l of every layer stays in it; without,
// they are formed here, layer by layer, and the dZ_l ping-pong in the workspace.
struct MlpBwdIo {
  const float* x; int ldx;
  const float* d_out; int ld_dout;
  const float* save;
  const empose_mlp_grads* gr; int accumulate;
  float* stash;   // or nullptr
};
int sweep_wgrad(const MlpPlan& pl, const MlpBwdIo& io, int l, const float* dy, int ld_dy, const MlpTrainWs& w,
                const char* what, hipStream_t stream) {
  return layer_wgrad(pl, l, 1, false, &dy, ld_dy, &io.x, io.ldx, &io.save, io.gr, io.accumulate, w.atb, w.atb_floats, what,
                     stream);
}
// dA_{l-1} = dY_l W_l as a plain GEMM, then the BatchNorm / PReLU reverse of layer l - 1 as a launch of its own (layout 1)
int bwd_passes(const MlpPlan& pl, const MlpBwdIo& io, const MlpTrainWs& w, hipStream_t stream) {
  const empose_mlp_params* p = pl.p;
  const int M = pl.M, H = pl.H;
  if (io.stash) TRY(stash_d_out(pl, io.d_out, io.ld_dout, io.stash, stream));
  // w.d[0]: cotangent of the current layer's activation (the one of the layer below overwrites the consumed one);
  // w.d[1]: dZ_l when it is not stashed
  const float* dy = io.d_out;
  int ld_dy = io.ld_dout;
  for (int l = pl.L - 1; l >= 0; --l) {
    const LayerDims d = layer_dims(p, l, io.ldx);
    if (!d.last) {
      BnPreluArgs a{};
      a.M = M; a.C = H; a.x = pl.pre(io.save, l); a.ldx = H; a.gamma = p->bn_weight[l]; a.beta = p->bn_bias[l];
      a.slope = p->prelu[l];
      a.save_mean = const_cast<float*>(pl.mean(io.save, l)); a.save_rstd = const_cast<float*>(pl.rstd(io.save, l));
      float* dz = io.stash ? pl.stash_slot(io.stash, l) : w.d[1];
      a.dz = w.d[0]; a.lddz = H; a.dx = dz; a.lddx = H;
      a.dgamma = io.gr->bn_weight[l]; a.dbeta = io.gr->bn_bias[l]; a.dslope = io.gr->prelu[l];
      a.dslope_partial = w.slope_partial; a.counter = w.counter; a.workspace = w.bn; a.accumulate = io.accumulate;
      HIP_CHECK(launch_bn_prelu(a, true, stream), "bn_prelu backward");
      dy = dz; ld_dy = H;
    }
    if (!io.stash) TRY(sweep_wgrad(pl, io, l, dy, ld_dy, w, "dW", stream));
    if (l == 0) break;
    const float* wt = nullptr;
    TRY(weight_t_of(pl, l, w, stream, &wt));
    HIP_CHECK(gemm_one(dy, ld_dy, wt, d.out_pad, w.d[0], H, M, H, d.out_pad, nullptr, nullptr, nullptr, 0, 0, 0.f, stream),
              "dX gemm");
  }
  return EMPOSE_OK;
}
// Layouts 2 and 3: dA_{l-1} = dY_l W_l on the forward tile against W_l^T, its epilogue already in terms of layer l - 1: it
// writes dyh = dA * PReLU'(yhat) and the column sums BatchNorm's reverse needs.  fused: a small kernel turns the sums into
// dgamma / dbeta / dslope and three per-column coefficients, one pass forms dY = c1 dyh + c3 y + c0 in place;  epi: both
// in ONE launch (bn_finish_bwd).
int bwd_stats(const MlpPlan& pl, const MlpBwdIo& io, const MlpTrainWs& w, hipStream_t stream) {
  const empose_mlp_params* p = pl.p;
  const int M = pl.M, H = pl.H;
  const bool epi = pl.layout == 3;
  auto dz_of = [&](int l) -> float* { return io.stash ? pl.stash_slot(io.stash, l) : w.d[l & 1]; };
  if (io.stash) TRY(stash_d_out(pl, io.d_out, io.ld_dout, io.stash, stream));
  for (int l = pl.L - 1; l >= 0; --l) {
    const LayerDims d = layer_dims(p, l, io.ldx);
    const float* dy = d.last ? io.d_out : dz_of(l);
    const int ld_dy = d.last ? io.ld_dout : H;
    if (!io.stash) TRY(sweep_wgrad(pl, io, l, dy, ld_dy, w, "fused dW", stream));
    if (l == 0) break;
    const float* wt = nullptr;
    TRY(weight_t_of(pl, l, w, stream, &wt));
    TrainGemmArgs g{};
    g.A = dy; g.lda = ld_dy; g.W = wt; g.ldw = d.out_pad;
    g.C = dz_of(l - 1); g.ldc = H; g.M = M; g.N = H; g.K = d.out_pad; g.bias = nullptr;
    g.part = w.part; g.e_y = pl.pre(io.save, l - 1); g.ld_ey = H;
    g.e_mean = pl.mean(io.save, l - 1); g.e_rstd = pl.rstd(io.save, l - 1); g.e_s = pl.s(io.save, l - 1);
    g.e_t = pl.t(io.save, l - 1); g.e_slope = p->prelu[l - 1];
    const bool x3 = options().train_x3 != 0 && p->weight_t[l] && p->weight_t_x3[l] && gemm_train_x3_applicable(g.M, g.N, g.K);
    HIP_CHECK(x3 ? launch_gemm_train_x3(g, p->weight_t_x3[l], 2, stream) : launch_gemm_train(g, 0, 2, stream), "fused dX gemm");
    auto sums = [&](auto& c) {
      c.M = M; c.C = H; c.part = w.part; c.gamma = p->bn_weight[l - 1];
      c.mean = pl.mean(io.save, l - 1); c.rstd = pl.rstd(io.save, l - 1);
      c.dgamma = io.gr->bn_weight[l - 1]; c.dbeta = io.gr->bn_bias[l - 1]; c.dslope = io.gr->prelu[l - 1];
      c.dslope_partial = w.slope_partial; c.accumulate = io.accumulate;
    };
    if (epi) {
      BnFinishBwdArgs f{};
      sums(f);
      f.counter = w.counter; f.dyh = dz_of(l - 1); f.ld = H; f.y = pl.pre(io.save, l - 1); f.ldy = H;
      HIP_CHECK(launch_bn_finish_bwd(f, stream), "bn finish backward");
    } else {
      BnFusedBwdArgs c{};
      sums(c);
      c.coef = w.coef;
      HIP_CHECK(launch_bn_fused_combine_bwd(c, stream), "fused bn reverse combine");
      HIP_CHECK(launch_bn_fused_apply_bwd(dz_of(l - 1), pl.pre(io.save, l - 1), w.coef, M, H, stream), "fused bn reverse apply");
    }
  }
  return EMPOSE_OK;
}
// One or two MLPs on the one-launch layers: layer l's launch forms dA_{l-1} = dZ_l W_l and, in its epilogue, the
// BatchNorm / PReLU reverse of layer l - 1 (whose column sums the row parts exchange) -> dZ_{l-1}.  A pair runs deferred.
int mlp_bwd_cols(const MlpPlan* pls, int n, const MlpBwdIo* ios, const MlpTrainWs& w, hipStream_t stream) {
  const int L = pls[0].L, M = pls[0].M;
  const bool deferred = ios[0].stash != nullptr;
  if (!deferred && n != 1) return fail(EMPOSE_EINVAL, "a pair of networks runs its reverse sweep with deferred weight gradients");
  HIP_TRY(hipMemsetAsync(w.mbox, 0, w.mbox_bytes, stream));
  auto dz_of = [&](int i, int l) -> float* { return deferred ? pls[i].stash_slot(ios[i].stash, l) : w.d[l & 1]; };
  for (int i = 0; i < n && deferred; ++i) TRY(stash_d_out(pls[i], ios[i].d_out, ios[i].ld_dout, ios[i].stash, stream));
  for (int l = L - 1; l >= 0; --l) {
    const bool last = l == L - 1;
    if (!deferred) TRY(sweep_wgrad(pls[0], ios[0], l, last ? ios[0].d_out : dz_of(0, l), last ? ios[0].ld_dout : pls[0].H, w, "dW", stream));
    if (l == 0) break;
    ColsArgs a{};
    a.n_nets = n; a.M = M; a.eps = pls[0].p->bn_eps; a.momentum = pls[0].p->bn_momentum; a.accumulate = ios[0].accumulate;
    a.tag = (unsigned)l; a.mailbox = w.mbox;
    for (int i = 0; i < n; ++i) {
      const MlpPlan& pl = pls[i];
      const MlpBwdIo& io = ios[i];
      const empose_mlp_params* p = pl.p;
      const LayerDims d = layer_dims(p, l, io.ldx);
      const int H = pl.H;
      ColsNet& c = a.net[i];
      c.A = last ? io.d_out : dz_of(i, l); c.lda = last ? io.ld_dout : H;
      c.N = H; c.K = d.out_pad;
      if (p->weight_t[l]) { c.W = p->weight_t[l]; c.ldw = d.out_pad; }
      else { c.W = p->weight[l]; c.ldw = H; c.w_kmajor = 1; c.Kw = d.N; }   // the layer's own W, read by rows
      c.gamma = p->bn_weight[l - 1]; c.beta = p->bn_bias[l - 1]; c.slope = p->prelu[l - 1];
      c.z_in = pl.pre(io.save, l - 1); c.ldz = H;
      c.mean = const_cast<float*>(pl.mean(io.save, l - 1)); c.rstd = const_cast<float*>(pl.rstd(io.save, l - 1));
      c.out = dz_of(i, l - 1); c.ld_out = H;
      c.dgamma = io.gr->bn_weight[l - 1]; c.dbeta = io.gr->bn_bias[l - 1]; c.dslope = io.gr->prelu[l - 1];
    }
    HIP_CHECK(launch_cols(a, 2, stream), "one-launch layer backward");
  }
  return EMPOSE_OK;
}

// ---- in front of the reverse sweeps, immediate or deferred: the argument checks, once (the forward: empose_mlp_train_fwd)
int mlp_train_bwd(const empose_mlp_params* p, int M, const MlpBwdIo& io, void* workspace, size_t workspace_bytes,
                  empose_stream_t stream_) {
  TRY(check_mlp_params(p));
  TRY(earlier_poll_timeouts());
  if (!io.x || !io.d_out || !io.save || !io.gr || !workspace) return fail(EMPOSE_EINVAL, "null argument");
  const int L = p->n_layers, op = (p->out_dim + 3) & ~3;
  if (M <= 0 || io.ldx < p->in_dim || io.ld_dout < op || io.ld_dout % 4 != 0) return fail(EMPOSE_EINVAL, "bad sizes");
  if (workspace_bytes < empose_mlp_train_workspace_bytes(p, M)) return fail(EMPOSE_ENOMEM, "workspace too small");
  for (int l = 0; l < L; ++l) {
    if (!io.gr->weight[l] || !io.gr->bias[l]) return fail(EMPOSE_EINVAL, "null gradient output");
    if (l < L - 1 && (!io.gr->bn_weight[l] || !io.gr->bn_bias[l] || !io.gr->prelu[l])) return fail(EMPOSE_EINVAL, "null gradient output");
  }
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  Carver c(workspace);
  const MlpTrainWs w = carve_mlp_train(c, p, M);
  const MlpPlan pl = mlp_plan(p, M);
  if (pl.cols()) return mlp_bwd_cols(&pl, 1, &io, w, stream);
  // the last-arriver counter of the single-pass BatchNorm reverse kernel (it re-arms itself; the workspace may be fresh)
  if (M <= BN_SINGLE_PASS_ROWS || pl.layout == 3) HIP_TRY(hipMemsetAsync(w.counter, 0, sizeof(int), stream));
  return pl.layout == 1 ? bwd_passes(pl, io, w, stream) : bwd_stats(pl, io, w, stream);
}
}  // namespace

extern "C" {

int empose_linear_f32_ex(const float* A, int lda, const float* W, int ldw, float* C, int ldc, int M, int N, int K,
                         const float* scale, const float* shift, const float* resid, int ldr, int act, float slope,
                         empose_stream_t stream_) {
  if (!A || !W || !C) return fail(EMPOSE_EINVAL, "null argument");
  if (K % 4 != 0 || lda % 4 != 0 || ldw % 4 != 0) return fail(EMPOSE_EINVAL, "K, lda, ldw must be multiples of 4");
  if (((uintptr_t)A & 15) || ((uintptr_t)W & 15)) return fail(EMPOSE_EINVAL, "A and W must be 16-byte aligned");
  if (act < 0 || act > 2) return fail(EMPOSE_EINVAL, "act must be 0 (none), 1 (PReLU, residual added after) or 2 (residual, then ReLU)");
  HIP_CHECK(gemm_one(A, lda, W, ldw, C, ldc, M, N, K, scale, shift, resid, ldr, act, slope, static_cast<hipStream_t>(stream_)),
            "gemm launch");
  return EMPOSE_OK;
}

int empose_gemm_strided_f32(int M, int N, int K, const float* A, long a_rs, long a_ks, const float* W, long w_rs,
                            long w_ks, float* C, int ldc, const float* bias, empose_stream_t stream_) {
  if (!A || !W || !C) return fail(EMPOSE_EINVAL, "null argument");
  if (M <= 0 || N <= 0 || K <= 0 || ldc < N) return fail(EMPOSE_EINVAL, "bad sizes");
  if (!strided_gemm_applicable(M, N))
    return fail(EMPOSE_EINVAL, "problem too large for the small-problem GEMM (%d x %d outputs)", M, N);
  StridedGemm p;
  p.A = A; p.a_rs = a_rs; p.a_ks = a_ks; p.W = W; p.w_rs = w_rs; p.w_ks = w_ks; p.C = C; p.ldc = ldc; p.bias = bias;
  p.M = M; p.N = N; p.K = K;
  HIP_CHECK(launch_strided_gemm(p, static_cast<hipStream_t>(stream_)), "strided gemm launch");
  return EMPOSE_OK;
}

int empose_gemm_strided_applicable(int M, int N) { return strided_gemm_applicable(M, N) ? 1 : 0; }

size_t empose_bn_prelu_workspace_bytes(int M, int C) {
  return (M > 0 && C > 0) ? bn_prelu_workspace_floats(M, C) * sizeof(float) : 0;
}

int empose_bn_prelu_train_fwd(int M, int C, const float* x, int ldx, const float* gamma, const float* beta,
                              const float* slope, float eps, float momentum, float* running_mean, float* running_var,
                              long long* num_batches_tracked, float* z, int ldz, float* save_mean, float* save_rstd,
                              void* workspace, size_t workspace_bytes, empose_stream_t stream_) {
  if (!x || !gamma || !beta || !slope || !z || !save_mean || !save_rstd) return fail(EMPOSE_EINVAL, "null argument");
  if (M <= 0 || C <= 0 || ldx < C || ldz < C) return fail(EMPOSE_EINVAL, "bad sizes");
  if (bn_prelu_workspace_floats(M, C) * sizeof(float) > (workspace ? workspace_bytes : 0))
    return fail(EMPOSE_ENOMEM, "workspace too small (empose_bn_prelu_workspace_bytes)");
  if ((running_mean == nullptr) != (running_var == nullptr)) return fail(EMPOSE_EINVAL, "running_mean and running_var go together");
  BnPreluArgs a{};
  a.M = M; a.C = C; a.x = x; a.ldx = ldx; a.gamma = gamma; a.beta = beta; a.slope = slope; a.eps = eps;
  a.momentum = momentum; a.running_mean = running_mean; a.running_var = running_var;
  a.num_batches_tracked = num_batches_tracked; a.z = z; a.ldz = ldz; a.save_mean = save_mean; a.save_rstd = save_rstd;
  a.workspace = static_cast<float*>(workspace);
  HIP_CHECK(launch_bn_prelu(a, false, static_cast<hipStream_t>(stream_)), "bn_prelu forward");
  return EMPOSE_OK;
}

int empose_bn_prelu_train_bwd(int M, int C, const float* x, int ldx, const float* dz, int lddz, const float* gamma,
                              const float* beta, const float* slope, const float* save_mean, const float* save_rstd,
                              float* dx, int lddx, float* dgamma, float* dbeta, float* dslope, float* dslope_partial,
                              int* counter, void* workspace, size_t workspace_bytes, empose_stream_t stream_) {
  if (!x || !dz || !gamma || !beta || !slope || !save_mean || !save_rstd || !dx || !dgamma || !dbeta || !dslope ||
      !dslope_partial || !counter)
    return fail(EMPOSE_EINVAL, "null argument");
  if (M <= 0 || C <= 0 || ldx < C || lddz < C || lddx < C) return fail(EMPOSE_EINVAL, "bad sizes");
  if (bn_prelu_workspace_floats(M, C) * sizeof(float) > (workspace ? workspace_bytes : 0))
    return fail(EMPOSE_ENOMEM, "workspace too small (empose_bn_prelu_workspace_bytes)");
  BnPreluArgs a{};
  a.workspace = static_cast<float*>(workspace);
  a.M = M; a.C = C; a.x = x; a.ldx = ldx; a.gamma = gamma; a.beta = beta; a.slope = slope;
  a.save_mean = const_cast<float*>(save_mean); a.save_rstd = const_cast<float*>(save_rstd);
  a.dz = dz; a.lddz = lddz; a.dx = dx; a.lddx = lddx; a.dgamma = dgamma; a.dbeta = dbeta; a.dslope_partial = dslope_partial; a.dslope = dslope; a.counter = counter;
  HIP_CHECK(launch_bn_prelu(a, true, static_cast<hipStream_t>(stream_)), "bn_prelu backward");
  return EMPOSE_OK;
}

// ---- training backward building blocks ------------------------------------------------------------------------
size_t empose_gemm_atb_workspace_bytes(int M, int N, int K) {
  if (M <= 0 || N <= 0 || K <= 0) return 0;
  return atb_workspace_floats(M, N, K) * sizeof(float) + 256;
}

int empose_gemm_atb_f32(int M, int N, int K, const float* A, int lda, const float* B, int ldb, float* C, int ldc,
                        float* bias, void* workspace, size_t workspace_bytes, empose_stream_t stream_) {
  if (!A || !B || !C) return fail(EMPOSE_EINVAL, "null argument");
  if (M <= 0 || N <= 0 || K <= 0 || lda < N || ldb < K || ldc < K) return fail(EMPOSE_EINVAL, "bad sizes");
  const size_t need = atb_workspace_floats(M, N, K) * sizeof(float);
  if (need > 0 && (!workspace || workspace_bytes < need)) return fail(EMPOSE_ENOMEM, "workspace too small");
  AtbArgs a{};
  a.A = A; a.lda = lda; a.B = B; a.ldb = ldb; a.C = C; a.ldc = ldc; a.bias = bias; a.M = M; a.N = N; a.K = K;
  a.accumulate = 0;
  HIP_CHECK(launch_gemm_atb(a, static_cast<float*>(workspace), workspace_bytes / sizeof(float),
                            static_cast<hipStream_t>(stream_)), "A^T B gemm");
  return EMPOSE_OK;
}

int empose_transpose_f32(int rows, int cols, const float* src, int ld_src, float* dst, int ld_dst,
                         empose_stream_t stream_) {
  if (!src || !dst) return fail(EMPOSE_EINVAL, "null argument");
  if (rows <= 0 || cols <= 0 || ld_src < cols || ld_dst < rows) return fail(EMPOSE_EINVAL, "bad sizes");
  HIP_CHECK(launch_transpose(src, ld_src, dst, ld_dst, rows, cols, static_cast<hipStream_t>(stream_)), "transpose");
  return EMPOSE_OK;
}

int empose_pack_inputs(int B, int F, int n_markers, const int* marker_idx, const float* marker_pos,
                       const float* marker_oris, const float* marker_masks, const int* seq_lengths, float* x, int ldx,
                       float* frame_weight, empose_stream_t stream_) {
  if (!marker_idx || !marker_pos || !marker_oris || !x) return fail(EMPOSE_EINVAL, "null argument");
  if (B <= 0 || F <= 0 || n_markers < 1 || n_markers > 12 || ldx < 12 * n_markers) return fail(EMPOSE_EINVAL, "bad sizes");
  PackArgs pa;
  pa.marker_pos = marker_pos; pa.marker_oris = marker_oris; pa.marker_masks = marker_masks; pa.seq_lengths = seq_lengths;
  pa.x = x; pa.ldx = ldx; pa.frame_scale = frame_weight; pa.B = B; pa.F = F; pa.n_markers = n_markers;
  for (int i = 0; i < 12; ++i) {
    pa.marker_idx[i] = i < n_markers ? marker_idx[i] : 0;
    if (pa.marker_idx[i] < 0 || pa.marker_idx[i] > 11) return fail(EMPOSE_EINVAL, "sensor index out of range");
  }
  HIP_CHECK(launch_pack_inputs(pa, static_cast<hipStream_t>(stream_)), "pack kernel");
  return EMPOSE_OK;
}

int empose_window_mean(int T, int F, int C, const float* in, int ld_in, float* out, int ld_out, empose_stream_t stream_) {
  if (!in || !out) return fail(EMPOSE_EINVAL, "null argument");
  if (T <= 0 || F <= 0 || C <= 0 || T % F != 0 || ld_in < C || ld_out < C) return fail(EMPOSE_EINVAL, "bad sizes");
  HIP_CHECK(launch_window_mean(in, ld_in, out, ld_out, T, F, C, static_cast<hipStream_t>(stream_)), "window mean");
  return EMPOSE_OK;
}

int empose_axpby2d(int rows, int cols, float alpha, const float* x, int ldx, float beta, const float* y, int ldy,
                   float* out, int ldo, empose_stream_t stream_) {
  if (!out) return fail(EMPOSE_EINVAL, "null argument");
  if (rows <= 0 || cols <= 0 || ldo < cols || (x && ldx < cols) || (y && ldy < cols)) return fail(EMPOSE_EINVAL, "bad sizes");
  HIP_CHECK(launch_axpby2d(rows, cols, alpha, x, ldx, beta, y, ldy, out, ldo, static_cast<hipStream_t>(stream_)), "axpby");
  return EMPOSE_OK;
}

int empose_lgd_assemble_inputs(int T, int d_in, const float* x0, int ld_x0, const float* pose, const float* shape,
                               float* X, int ldx, empose_stream_t stream_) {
  if (!x0 || !pose || !shape || !X) return fail(EMPOSE_EINVAL, "null argument");
  if (T <= 0 || d_in <= 0 || ld_x0 < d_in || ldx < d_in + 76) return fail(EMPOSE_EINVAL, "bad sizes");
  HIP_CHECK(launch_lgd_assemble(T, d_in, x0, ld_x0, pose, shape, X, ldx, static_cast<hipStream_t>(stream_)), "assemble");
  return EMPOSE_OK;
}

int empose_lgd_additive_update(int B, int F, float step, int shape_avg, const float* pose, const float* d_pose,
                               const float* shape, const float* d_shape, float* pose_next, float* shape_next,
                               empose_stream_t stream_) {
  if (!pose || !d_pose || !shape || !d_shape || !pose_next || !shape_next) return fail(EMPOSE_EINVAL, "null argument");
  if (B <= 0 || F <= 0) return fail(EMPOSE_EINVAL, "bad sizes");
  HIP_CHECK(launch_lgd_update(B, F, step, shape_avg, pose, d_pose, shape, d_shape, pose_next, shape_next,
                              static_cast<hipStream_t>(stream_)), "update");
  return EMPOSE_OK;
}

int empose_lgd_cotangent_step(int B, int F, int first, const float* d_pose, const float* d_shape, const float* vp,
                              const float* vs, const float* g_theta, int ld_g, const float* g_beta, int ld_gb, float* Dp,
                              float* Ds, float step, int shape_avg, float* dpad, float* dspad, empose_stream_t stream_) {
  if (!d_pose || !d_shape || !vp || !vs || !Dp || !Ds) return fail(EMPOSE_EINVAL, "null argument");
  if (B <= 0 || F <= 0 || (size_t)F * 10 * sizeof(float) > 48 * 1024) return fail(EMPOSE_EINVAL, "bad sizes");
  if ((g_theta && ld_g < 66) || (g_beta && ld_gb < 10) || ((dpad == nullptr) != (dspad == nullptr)))
    return fail(EMPOSE_EINVAL, "bad arguments");
  HIP_CHECK(launch_lgd_cotangent(B, F, first, d_pose, d_shape, vp, vs, g_theta, ld_g, g_beta, ld_gb, Dp, Ds, step,
                                 shape_avg, dpad, dspad, static_cast<hipStream_t>(stream_)), "cotangent step");
  return EMPOSE_OK;
}

size_t empose_lgd_losses_workspace_bytes(int B, int F, int n_hist) {
  if (B <= 0 || F <= 0 || n_hist <= 0) return 0;
  return (size_t)4 * n_hist * B * F * sizeof(float) + 256;
}

int empose_lgd_losses(const empose_loss_io* io, void* workspace, size_t workspace_bytes, empose_stream_t stream_) {
  if (!io || !workspace) return fail(EMPOSE_EINVAL, "null argument");
  if (io->B <= 0 || io->F <= 0 || io->n_hist <= 0 || (io->n_markers != 6 && io->n_markers != 12))
    return fail(EMPOSE_EINVAL, "bad sizes");
  if (!io->pose_hist || !io->shape_hist || !io->markers_hist || !io->markers_ori_hist || !io->joints_final ||
      !io->pose_gt || !io->shape_gt || !io->inputs || !io->d_pose || !io->d_shape || !io->d_markers ||
      !io->d_markers_ori || !io->d_joints || !io->loss_vals)
    return fail(EMPOSE_EINVAL, "null tensor");
  if (io->ld_inputs < 12 * io->n_markers) return fail(EMPOSE_EINVAL, "ld_inputs below 12 * n_markers");
  if (workspace_bytes < empose_lgd_losses_workspace_bytes(io->B, io->F, io->n_hist)) return fail(EMPOSE_ENOMEM, "workspace too small");
  LossArgs a;
  a.B = io->B; a.F = io->F; a.N1 = io->n_hist; a.n_markers = io->n_markers;
  for (int m = 0; m < 12; ++m) a.used_slot[m] = -1;
  for (int i = 0; i < io->n_markers; ++i) {
    if (io->marker_idx[i] < 0 || io->marker_idx[i] >= 12) return fail(EMPOSE_EINVAL, "marker_idx out of range");
    a.used_slot[io->marker_idx[i]] = i;
  }
  a.pose_hist = io->pose_hist; a.shape_hist = io->shape_hist; a.pos_hist = io->markers_hist; a.ori_hist = io->markers_ori_hist;
  a.joints_final = io->joints_final; a.pose_gt = io->pose_gt; a.shape_gt = io->shape_gt; a.joints_gt = io->joints_gt;
  a.x_in = io->inputs; a.ldx = io->ld_inputs; a.seq_lengths = io->seq_lengths; a.masks = io->marker_masks;
  a.w_pose = io->w_pose; a.w_shape = io->w_shape; a.w_fk = io->w_fk; a.w_rec = io->w_rec;
  a.d_pose = io->d_pose; a.d_shape = io->d_shape; a.d_pos = io->d_markers; a.d_ori = io->d_markers_ori;
  a.d_joints = io->d_joints; a.partial = static_cast<float*>(workspace); a.loss_vals = io->loss_vals;
  HIP_CHECK(launch_lgd_losses(a, static_cast<hipStream_t>(stream_)), "loss kernels");
  return EMPOSE_OK;
}

int empose_adam_step(int n_chunks, const void* params, const void* grads, const void* exp_avg, const void* exp_avg_sq,
                     const void* sizes, const void* chunk_tensor, const void* chunk_offset, float lr, float beta1,
                     float beta2, float eps, int step, empose_stream_t stream_) {
  if (!params || !grads || !exp_avg || !exp_avg_sq || !sizes || !chunk_tensor || !chunk_offset)
    return fail(EMPOSE_EINVAL, "null argument");
  if (n_chunks <= 0 || step < 1) return fail(EMPOSE_EINVAL, "bad sizes");
  AdamArgs a;
  a.params = static_cast<void* const*>(params); a.grads = static_cast<void* const*>(grads);
  a.exp_avg = static_cast<void* const*>(exp_avg); a.exp_avg_sq = static_cast<void* const*>(exp_avg_sq);
  a.sizes = static_cast<const long long*>(sizes); a.chunk_tensor = static_cast<const int*>(chunk_tensor);
  a.chunk_offset = static_cast<const long long*>(chunk_offset);
  a.beta1 = beta1; a.beta2 = beta2; a.eps = eps;
  const double bc1 = 1.0 - std::pow((double)beta1, (double)step), bc2 = 1.0 - std::pow((double)beta2, (double)step);
  a.step_size = (float)((double)lr / bc1);
  a.inv_sqrt_bc2 = (float)(1.0 / std::sqrt(bc2));
  HIP_CHECK(launch_adam(a, n_chunks, static_cast<hipStream_t>(stream_)), "adam");
  return EMPOSE_OK;
}

int empose_mlp_train_uses_weight_t(const empose_mlp_params* p, int M) {
  if (!p || M <= 0) return fail(EMPOSE_EINVAL, "null parameters / no rows");
  return mlp_plan(p, M).cols() ? 0 : 1;
}

int empose_mlp_train_save_layout(const empose_mlp_params* p, int M) {
  if (!p || M <= 0) return fail(EMPOSE_EINVAL, "null parameters / no rows");
  if (p->save_layout < 0 || p->save_layout > 3) return fail(EMPOSE_EINVAL, "save_layout must be 0 .. 3");
  return mlp_plan(p, M).layout;
}

size_t empose_mlp_train_save_floats(const empose_mlp_params* p, int M) {
  if (!p || M <= 0) return 0;
  return mlp_plan(p, M).save_floats();
}

size_t empose_mlp_train_workspace_bytes(const empose_mlp_params* p, int M) {
  if (!p || M <= 0) return 0;
  Carver c(nullptr);
  carve_mlp_train(c, p, M);
  return c.off;
}

int empose_mlp_train_fwd(const empose_mlp_params* p, int M, const float* x, int ldx, float* out, int ld_out,
                         float* save, void* workspace, size_t workspace_bytes, empose_stream_t stream_) {
  TRY(check_mlp_params(p));
  TRY(earlier_poll_timeouts());
  if (!x || !out || !save || !workspace) return fail(EMPOSE_EINVAL, "null argument");
  if (M <= 0 || ldx < p->in_dim || ldx % 4 != 0 || ld_out < p->out_dim) return fail(EMPOSE_EINVAL, "bad sizes");
  if (workspace_bytes < empose_mlp_train_workspace_bytes(p, M)) return fail(EMPOSE_ENOMEM, "workspace too small");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  Carver c(workspace);
  const MlpTrainWs w = carve_mlp_train(c, p, M);
  const MlpPlan pl = mlp_plan(p, M);
  if (pl.cols()) return mlp_fwd_cols(&pl, 1, x, ldx, &out, &ld_out, &save, w, stream);
  return pl.layout == 1 ? fwd_passes(pl, x, ldx, out, ld_out, save, w, stream)
                        : fwd_stats(pl, x, ldx, out, ld_out, save, w, stream);
}

int empose_mlp_train_bwd(const empose_mlp_params* p, int M, const float* x, int ldx, const float* d_out, int ld_dout,
                         const float* save, const empose_mlp_grads* gr, int accumulate, void* workspace,
                         size_t workspace_bytes, empose_stream_t stream) {
  return mlp_train_bwd(p, M, {x, ldx, d_out, ld_dout, save, gr, accumulate, nullptr}, workspace, workspace_bytes, stream);
}

size_t empose_mlp_train_stash_floats(const empose_mlp_params* p, int M) {
  if (!p || M <= 0 || check_mlp_params(p) != EMPOSE_OK) return 0;
  return mlp_plan(p, M).stash_floats();
}

int empose_mlp_train_bwd_deferred(const empose_mlp_params* p, int M, const float* x, int ldx, const float* d_out,
                                  int ld_dout, const float* save, const empose_mlp_grads* gr, int accumulate,
                                  float* dz_stash, void* workspace, size_t workspace_bytes, empose_stream_t stream) {
  if (!dz_stash) return fail(EMPOSE_EINVAL, "null stash");
  return mlp_train_bwd(p, M, {x, ldx, d_out, ld_dout, save, gr, accumulate, dz_stash}, workspace, workspace_bytes, stream);
}

// ---- both update networks of an iteration in one call: paired launches on the one-launch layers, else one after the other
size_t empose_mlp_train_pair_workspace_bytes(const empose_mlp_params* p0, const empose_mlp_params* p1, int M) {
  const size_t a = empose_mlp_train_workspace_bytes(p0, M), b = empose_mlp_train_workspace_bytes(p1, M);
  return a > b ? a : b;
}

int empose_mlp_train_fwd_pair(const empose_mlp_params* p0, const empose_mlp_params* p1, int M, const float* x, int ldx,
                              float* out0, int ld_out0, float* out1, int ld_out1, float* save0, float* save1,
                              void* workspace, size_t workspace_bytes, empose_stream_t stream_) {
  TRY(check_mlp_params(p0));
  TRY(check_mlp_params(p1));
  TRY(earlier_poll_timeouts());
  if (workspace_bytes < empose_mlp_train_pair_workspace_bytes(p0, p1, M)) return fail(EMPOSE_ENOMEM, "workspace too small");
  const MlpPlan pls[2] = {mlp_plan(p0, M), mlp_plan(p1, M)};
  if (M > 0 && x && out0 && out1 && save0 && save1 && workspace && ldx % 4 == 0 && ldx >= p0->in_dim && ldx >= p1->in_dim &&
      ld_out0 >= p0->out_dim && ld_out1 >= p1->out_dim && mlp_cols_pairable(pls[0], pls[1])) {
    Carver c(workspace);
    const MlpTrainWs w = carve_mlp_train(c, p0, M);
    float* outs[2] = {out0, out1};
    const int lds[2] = {ld_out0, ld_out1};
    float* saves[2] = {save0, save1};
    return mlp_fwd_cols(pls, 2, x, ldx, outs, lds, saves, w, static_cast<hipStream_t>(stream_));
  }
  TRY(empose_mlp_train_fwd(p0, M, x, ldx, out0, ld_out0, save0, workspace, workspace_bytes, stream_));
  return empose_mlp_train_fwd(p1, M, x, ldx, out1, ld_out1, save1, workspace, workspace_bytes, stream_);
}

int empose_mlp_train_bwd_deferred_pair(const empose_mlp_params* p0, const empose_mlp_params* p1, int M, const float* x,
                                       int ldx, const float* d_out0, int ld_dout0, const float* d_out1, int ld_dout1,
                                       const float* save0, const float* save1, const empose_mlp_grads* gr0,
                                       const empose_mlp_grads* gr1, int accumulate, float* dz_stash0, float* dz_stash1,
                                       void* workspace, size_t workspace_bytes, empose_stream_t stream_) {
  TRY(check_mlp_params(p0));
  TRY(check_mlp_params(p1));
  TRY(earlier_poll_timeouts());
  if (!dz_stash0 || !dz_stash1) return fail(EMPOSE_EINVAL, "null stash");
  if (workspace_bytes < empose_mlp_train_pair_workspace_bytes(p0, p1, M)) return fail(EMPOSE_ENOMEM, "workspace too small");
  const MlpPlan pls[2] = {mlp_plan(p0, M), mlp_plan(p1, M)};
  const MlpBwdIo ios[2] = {{x, ldx, d_out0, ld_dout0, save0, gr0, accumulate, dz_stash0},
                           {x, ldx, d_out1, ld_dout1, save1, gr1, accumulate, dz_stash1}};
  bool pair = M > 0 && x && d_out0 && d_out1 && save0 && save1 && gr0 && gr1 && workspace && mlp_cols_pairable(pls[0], pls[1]) &&
              ld_dout0 % 4 == 0 && ld_dout1 % 4 == 0 && ld_dout0 >= pls[0].op && ld_dout1 >= pls[1].op;
  for (int l = 0; l < p0->n_layers - 1 && pair; ++l)
    if (!gr0->bn_weight[l] || !gr0->bn_bias[l] || !gr0->prelu[l] || !gr1->bn_weight[l] || !gr1->bn_bias[l] || !gr1->prelu[l])
      pair = false;
  if (pair) {
    Carver c(workspace);
    const MlpTrainWs w = carve_mlp_train(c, p0, M);
    return mlp_bwd_cols(pls, 2, ios, w, static_cast<hipStream_t>(stream_));
  }
  TRY(mlp_train_bwd(p0, M, ios[0], workspace, workspace_bytes, stream_));
  return mlp_train_bwd(p1, M, ios[1], workspace, workspace_bytes, stream_);
}

size_t empose_mlp_train_wgrad_workspace_bytes(const empose_mlp_params* p, int n_app, int M) {
  if (!p || M <= 0 || n_app <= 0 || check_mlp_params(p) != EMPOSE_OK) return 0;
  // batched: one product over n_app * M rows; row counts off the 32-row grid run per application (M rows each)
  const size_t a = mlp_atb_floats(p, n_app * M), b = mlp_atb_floats(p, M);
  return ((a > b ? a : b) + 64) * sizeof(float);
}

int empose_mlp_train_wgrad(const empose_mlp_params* p, int n_app, int M, const float* const* x, int ldx,
                           const float* const* save, const float* const* dz_stash, const empose_mlp_grads* gr,
                           int accumulate, void* workspace, size_t workspace_bytes, empose_stream_t stream_) {
  TRY(check_mlp_params(p));
  TRY(earlier_poll_timeouts());
  if (!x || !save || !dz_stash || !gr || !workspace) return fail(EMPOSE_EINVAL, "null argument");
  if (n_app < 1 || n_app > ATB_MAX_SEG || M <= 0 || ldx < p->in_dim) return fail(EMPOSE_EINVAL, "bad sizes");
  if (workspace_bytes < empose_mlp_train_wgrad_workspace_bytes(p, n_app, M)) return fail(EMPOSE_ENOMEM, "workspace too small");
  // one product over all applications when their rows can be addressed as 32-row aligned segments, else one per application
  bool batched = M % 32 == 0 && ldx % 4 == 0;
  for (int s = 0; s < n_app && batched; ++s)
    batched = x[s] && save[s] && dz_stash[s] && ((uintptr_t)x[s] & 15) == 0 && ((uintptr_t)save[s] & 15) == 0 &&
              ((uintptr_t)dz_stash[s] & 15) == 0;
  for (int s = 0; s < n_app; ++s)
    if (!x[s] || !save[s] || !dz_stash[s]) return fail(EMPOSE_EINVAL, "null argument");
  const MlpPlan pl = mlp_plan(p, M);
  for (int l = 0; l < pl.L; ++l) {
    if (!gr->weight[l] || !gr->bias[l]) return fail(EMPOSE_EINVAL, "null gradient output");
    // operands as the reverse sweeps left them: dY_l (stash) and the layer's input (x, save)
    const float* dy[ATB_MAX_SEG];
    for (int s = 0; s < n_app; ++s) dy[s] = pl.stash_slot(dz_stash[s], l);
    TRY(layer_wgrad(pl, l, n_app, batched, dy, layer_dims(p, l, ldx).out_pad, x, ldx, save, gr, accumulate,
                    static_cast<float*>(workspace), workspace_bytes / sizeof(float), pl.layout == 2 ? "fused dW" : "dW",
                    static_cast<hipStream_t>(stream_)));
  }
  return EMPOSE_OK;
}

int empose_linear_f32(const float* A, int lda, const float* W, int ldw, float* C, int ldc, int M, int N, int K,
                      const float* scale, const float* shift, int prelu, float slope, empose_stream_t stream) {
  return empose_linear_f32_ex(A, lda, W, ldw, C, ldc, M, N, K, scale, shift, nullptr, 0, prelu ? 1 : 0, slope, stream);
}

}  // extern "C"
