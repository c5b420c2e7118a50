// C ABI (include/empose_hip.h), training building blocks: plain products, BatchNorm + PReLU, A^T B, transpose,
// input packing, the LGD update / cotangent / loss kernels, Adam; one MLP (or both update networks) in training mode.
#include "api_internal.h"

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
// The BatchNorm / PReLU passes folded into the GEMMs (train_fused.hip).  Opt-in: gradient parity with the reference is
// tested, but at 256 windows the step is no faster (the operand transform and the statistics epilogue cost the GEMMs
// about what the removed passes cost: 701-711 k against 705-720 k frames/s).  Option "train_fused": 0 never (default),
// 1 from BN_SINGLE_PASS_ROWS rows on, 2 always (tests).
// (empose_mlp_params::save_layout != 0: the layout chosen when the step's forward ran wins over the options of the moment)
bool mlp_train_fused(const empose_mlp_params* p, int M) {
  if (p->save_layout) return p->save_layout == 2;
  const int opt = options().train_fused;
  return opt != 0 && (opt == 2 || M > BN_SINGLE_PASS_ROWS) && p->hidden % 4 == 0 && p->in_dim % 4 == 0;
}
// Round 4, the default above BN_SINGLE_PASS_ROWS rows: the statistics still come out of the GEMM epilogues, but the
// activations / cotangents are materialised by ONE combine-and-apply launch per layer and direction (train_fused.hip,
// bn_finish_*): GEMM + 1 launch instead of GEMM + 3, and every consumer reads a ready operand.  Option "train_epi":
// 0 never, 1 above BN_SINGLE_PASS_ROWS rows (default), 2 always (tests).  "train_fused" takes precedence when both apply.
bool mlp_train_epi(const empose_mlp_params* p, int M) {
  if (p->save_layout) return p->save_layout == 3;
  const int opt = options().train_epi;
  return !mlp_train_fused(p, M) && opt != 0 && (opt == 2 || M > BN_SINGLE_PASS_ROWS) && p->hidden % 4 == 0 &&
         p->in_dim % 4 == 0;
}
// per hidden layer: passes  z [M][H] | a [M][H] | mean [H] | rstd [H];  fused  y [M][H] | mean | rstd | s | t;
//                   epi     y [M][H] | a [M][H] | mean | rstd | s | t
size_t mlp_layer_save(const empose_mlp_params* p, int M) {
  if (mlp_train_fused(p, M)) return (size_t)M * p->hidden + 4 * (size_t)p->hidden;
  if (mlp_train_epi(p, M)) return (size_t)2 * M * p->hidden + 4 * (size_t)p->hidden;
  return (size_t)2 * M * p->hidden + 2 * (size_t)p->hidden;
}
// At the reference's training batch a layer is one launch: product, BatchNorm and PReLU of both update networks in
// train_cols.hip (option "train_cols": 0 never, 1 up to COLS_MAX_ROWS rows).  Reads and writes save layout 1 (passes).
bool mlp_train_cols(const empose_mlp_params* p, int M) {
  if (options().train_cols == 0 || M > COLS_MAX_ROWS) return false;
  if (mlp_train_fused(p, M) || mlp_train_epi(p, M)) return false;
  return cols_launchable(p->hidden > p->out_dim ? p->hidden : p->out_dim, 2);
}
bool mlp_cols_pairable(const empose_mlp_params* a, const empose_mlp_params* b, int M) {
  return a->n_layers == b->n_layers && a->hidden == b->hidden && a->bn_eps == b->bn_eps &&
         a->bn_momentum == b->bn_momentum && mlp_train_cols(a, M) && mlp_train_cols(b, M) &&
         b->out_dim <= (a->hidden > a->out_dim ? a->hidden : a->out_dim);
}

int mlp_fwd_cols(const empose_mlp_params* const* ps, int n, int M, const float* x, int ldx, float* const* outs,
                 const int* ld_outs, float* const* saves, const MlpTrainWs& w, hipStream_t stream) {
  const int L = ps[0]->n_layers;
  HIP_TRY(hipMemsetAsync(w.mbox, 0, w.mbox_bytes, stream));
  for (int l = 0; l < L; ++l) {
    const bool last = l == L - 1;
    ColsArgs a{};
    a.n_nets = n; a.M = M; a.eps = ps[0]->bn_eps; a.momentum = ps[0]->bn_momentum; a.tag = (unsigned)l + 1;
    a.mailbox = w.mbox;
    for (int i = 0; i < n; ++i) {
      const empose_mlp_params* p = ps[i];
      const int H = p->hidden;
      const size_t lsz = (size_t)2 * M * H + 2 * (size_t)H;
      float* sv = saves[i] + (size_t)l * lsz;                                   // z | a | mean | rstd
      ColsNet& c = a.net[i];
      c.A = l == 0 ? x : saves[i] + (size_t)(l - 1) * lsz + (size_t)M * H; c.lda = l == 0 ? ldx : H;
      c.W = p->weight[l]; c.ldw = l == 0 ? p->in_dim : H; c.bias = p->bias[l];
      c.N = last ? p->out_dim : H; c.K = l == 0 ? p->in_dim : H;
      if (last) { c.out = outs[i]; c.ld_out = ld_outs[i]; continue; }
      c.gamma = p->bn_weight[l]; c.beta = p->bn_bias[l]; c.slope = p->prelu[l];
      c.running_mean = p->bn_running_mean[l]; c.running_var = p->bn_running_var[l]; c.num_batches = p->bn_num_batches[l];
      c.z = sv; c.ldz = H; c.out = sv + (size_t)M * H; c.ld_out = H;
      c.mean = sv + (size_t)2 * M * H; c.rstd = c.mean + H;
    }
    HIP_CHECK(launch_cols(a, last ? 1 : 0, stream), "one-launch layer forward");
  }
  return EMPOSE_OK;
}

// stash of one application: dZ of the hidden layers [M][hidden] each, then a copy of d_out [M][out_pad]
size_t mlp_stash_floats(const empose_mlp_params* p, int M) {
  return (size_t)M * ((size_t)(p->n_layers - 1) * p->hidden + ((p->out_dim + 3) & ~3));
}
// The reverse sweep of one or two MLPs on the one-launch layers: layer l's launch forms dA_{l-1} = dZ_l W_l and, in its
// epilogue, the BatchNorm / PReLU reverse of layer l - 1 (whose column sums the row parts exchange) -> dZ_{l-1}.  With
// stashes the weight gradients are deferred (empose_mlp_train_wgrad); without (one network only) they are formed here.
int mlp_bwd_cols(const empose_mlp_params* const* ps, int n, int M, const float* x, int ldx, const float* const* d_outs,
                 const int* ld_douts, const float* const* saves, const empose_mlp_grads* const* grs, int accumulate,
                 float* const* stashes, const MlpTrainWs& w, hipStream_t stream) {
  const int L = ps[0]->n_layers;
  const bool deferred = stashes && stashes[0];
  if (!deferred && n != 1) return fail(EMPOSE_EINVAL, "a pair of networks runs its reverse sweep with deferred weight gradients");
  HIP_TRY(hipMemsetAsync(w.mbox, 0, w.mbox_bytes, stream));
  auto layer_save = [&](int i, int l) { return saves[i] + (size_t)l * ((size_t)2 * M * ps[i]->hidden + 2 * (size_t)ps[i]->hidden); };
  auto dz_of = [&](int i, int l) -> float* { return deferred ? stashes[i] + (size_t)M * l * ps[i]->hidden : w.d[l & 1]; };
  auto atb = [&](int l) -> int {   // dW_l, db_l of the single network (not deferred)
    const empose_mlp_params* p = ps[0];
    const int H = p->hidden;
    const bool last = l == L - 1;
    AtbArgs ab{};
    ab.A = last ? d_outs[0] : dz_of(0, l); ab.lda = last ? ld_douts[0] : H;
    ab.B = l == 0 ? x : layer_save(0, l - 1) + (size_t)M * H; ab.ldb = l == 0 ? ldx : H;
    ab.C = grs[0]->weight[l]; ab.ldc = l == 0 ? p->in_dim : H; ab.bias = grs[0]->bias[l];
    ab.M = M; ab.N = last ? p->out_dim : H; ab.K = l == 0 ? p->in_dim : H; ab.accumulate = accumulate;
    HIP_CHECK(launch_gemm_atb(ab, w.atb, w.atb_floats, stream), "dW");
    return EMPOSE_OK;
  };
  for (int i = 0; i < n && deferred; ++i) {   // keep d_out for empose_mlp_train_wgrad (no copy when it was produced in its slot)
    const int op = (ps[i]->out_dim + 3) & ~3;
    float* slot = stashes[i] + (size_t)M * (L - 1) * ps[i]->hidden;
    if (d_outs[i] != slot || ld_douts[i] != op) {
      HIP_CHECK(launch_axpby2d(M, op, 1.f, d_outs[i], ld_douts[i], 0.f, nullptr, 0, slot, op, stream), "stash");
    }
  }
  for (int l = L - 1; l >= 1; --l) {
    const bool last = l == L - 1;
    if (!deferred) TRY(atb(l));
    ColsArgs a{};
    a.n_nets = n; a.M = M; a.eps = ps[0]->bn_eps; a.momentum = ps[0]->bn_momentum; a.accumulate = accumulate;
    a.tag = (unsigned)l; a.mailbox = w.mbox;
    for (int i = 0; i < n; ++i) {
      const empose_mlp_params* p = ps[i];
      const int H = p->hidden, op = (p->out_dim + 3) & ~3, kdim = last ? op : H;
      const float* sv = layer_save(i, l - 1);
      ColsNet& c = a.net[i];
      c.A = last ? d_outs[i] : dz_of(i, l); c.lda = last ? ld_douts[i] : H;
      c.N = H; c.K = kdim;
      if (p->weight_t[l]) { c.W = p->weight_t[l]; c.ldw = kdim; }
      else { c.W = p->weight[l]; c.ldw = H; c.w_kmajor = 1; c.Kw = last ? p->out_dim : H; }   // the layer's own W, read by rows
      c.gamma = p->bn_weight[l - 1]; c.beta = p->bn_bias[l - 1]; c.slope = p->prelu[l - 1];
      c.z_in = sv; c.ldz = H; c.mean = const_cast<float*>(sv + (size_t)2 * M * H); c.rstd = c.mean + H;
      c.out = dz_of(i, l - 1); c.ld_out = H;
      c.dgamma = grs[i]->bn_weight[l - 1]; c.dbeta = grs[i]->bn_bias[l - 1]; c.dslope = grs[i]->prelu[l - 1];
    }
    HIP_CHECK(launch_cols(a, 2, stream), "one-launch layer backward");
  }
  if (!deferred) TRY(atb(0));
  return EMPOSE_OK;
}

int mlp_train_bwd_impl(const empose_mlp_params* p, int M, const float* x, int ldx, const float* d_out, int ld_dout,
                       const float* save, const empose_mlp_grads* gr, int accumulate, float* stash, void* workspace,
                       size_t workspace_bytes, empose_stream_t stream_) {
  TRY(check_mlp_params(p));
  TRY(earlier_poll_timeouts());
  if (!x || !d_out || !save || !gr || !workspace) return fail(EMPOSE_EINVAL, "null argument");
  const int H = p->hidden, L = p->n_layers, op = (p->out_dim + 3) & ~3;
  if (M <= 0 || ldx < p->in_dim || ld_dout < op || ld_dout % 4 != 0) return fail(EMPOSE_EINVAL, "bad sizes");
  if (workspace_bytes < empose_mlp_train_workspace_bytes(p, M)) return fail(EMPOSE_ENOMEM, "workspace too small");
  for (int l = 0; l < L; ++l) {
    if (!gr->weight[l] || !gr->bias[l]) return fail(EMPOSE_EINVAL, "null gradient output");
    if (l < L - 1 && (!gr->bn_weight[l] || !gr->bn_bias[l] || !gr->prelu[l])) return fail(EMPOSE_EINVAL, "null gradient output");
  }
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  Carver c(workspace);
  MlpTrainWs w = carve_mlp_train(c, p, M);
  if (mlp_train_cols(p, M))
    return mlp_bwd_cols(&p, 1, M, x, ldx, &d_out, &ld_dout, &save, &gr, accumulate, &stash, w, stream);
  // the last-arriver counter of the single-pass BatchNorm reverse kernel (it re-arms itself; the workspace may be fresh)
  const bool epi = mlp_train_epi(p, M);
  if (M <= BN_SINGLE_PASS_ROWS || epi) HIP_TRY(hipMemsetAsync(w.counter, 0, sizeof(int), stream));
  auto gemm = [&](const float* A, int lda, const float* W, int ldw, float* C, int ldc, int N, int K) -> hipError_t {
    GemmBatch b;
    b.count = 1;
    GemmProb& g = b.p[0];
    g.A = A; g.lda = lda; g.W = W; g.ldw = ldw; g.C = C; g.ldc = ldc; g.M = M; g.N = N; g.K = K;
    g.scale = nullptr; g.shift = nullptr; g.resid = nullptr; g.ldr = 0; g.act = 0; g.slope = 0.f;
    return launch_gemm(b, stream);
  };
  auto layer_save = [&](int l) { return save + (size_t)l * mlp_layer_save(p, M); };
  if (mlp_train_fused(p, M) || epi) {
    // The dX GEMM's epilogue writes dyh_l = dA_l * PReLU'(yhat_l) and the column sums BatchNorm's reverse needs; a
    // small kernel turns the sums into dgamma / dbeta / dslope and three per-column coefficients, one pass forms
    // dY_l = c1 dyh_l + c3 y_l + c0 in place (`epi`: both in ONE launch, bn_finish_bwd).  Fused: the layer inputs a_{l-1}
    // are not stored, the A^T B product re-forms them from y_{l-1} while it stages its B operand; `epi`: they are.
    auto stats_of = [&](int l) { return layer_save(l) + (size_t)(epi ? 2 : 1) * M * H; };   // mean | rstd | s | t
    auto dz_of = [&](int l) -> float* { return stash ? stash + (size_t)M * l * H : w.d[l & 1]; };
    auto atb = [&](int l) -> int {   // dW_l, db_l (not deferred)
      const bool last = l == L - 1;
      AtbArgs ab{};
      ab.A = last ? d_out : dz_of(l); ab.lda = last ? ld_dout : H;
      ab.B = l == 0 ? x : layer_save(l - 1) + (epi ? (size_t)M * H : 0); ab.ldb = l == 0 ? ldx : H;
      ab.C = gr->weight[l]; ab.ldc = l == 0 ? p->in_dim : H; ab.bias = gr->bias[l];
      ab.M = M; ab.N = last ? p->out_dim : H; ab.K = l == 0 ? p->in_dim : H; ab.accumulate = accumulate;
      if (l > 0 && !epi) { ab.b_mode = 1; ab.Bs_seg[0] = stats_of(l - 1) + 2 * H; ab.b_slope = p->prelu[l - 1]; }
      HIP_CHECK(launch_gemm_atb(ab, w.atb, w.atb_floats, stream), "fused dW");
      return EMPOSE_OK;
    };
    for (int l = L - 1; l >= 0; --l) {
      const bool last = l == L - 1;
      if (last && stash) {   // keep d_out for empose_mlp_train_wgrad (no copy when the caller produced it in its slot)
        float* slot = stash + (size_t)M * (L - 1) * H;
        if (d_out != slot || ld_dout != op) {
          HIP_CHECK(launch_axpby2d(M, op, 1.f, d_out, ld_dout, 0.f, nullptr, 0, slot, op, stream), "stash");
        }
      }
      if (!stash) TRY(atb(l));
      if (l == 0) break;
      // dA_{l-1} = dY_l W_l on the forward tile against W_l^T, its epilogue already in terms of layer l - 1
      const float* wt = p->weight_t[l];
      const int kdim = last ? op : H;
      if (!wt) {
        if (last) HIP_TRY(hipMemsetAsync(w.wt, 0, (size_t)H * op * sizeof(float), stream));
        HIP_CHECK(launch_transpose(p->weight[l], H, w.wt, kdim, last ? p->out_dim : H, H, stream), "transpose");
        wt = w.wt;
      }
      TrainGemmArgs g{};
      g.A = last ? d_out : dz_of(l); g.lda = last ? ld_dout : H; g.W = wt; g.ldw = kdim;
      g.C = dz_of(l - 1); g.ldc = H; g.M = M; g.N = H; g.K = kdim; g.bias = nullptr;
      g.part = w.part; g.e_y = layer_save(l - 1); g.ld_ey = H;
      g.e_mean = stats_of(l - 1); g.e_rstd = g.e_mean + H; g.e_s = g.e_rstd + H; g.e_t = g.e_s + H; g.e_slope = p->prelu[l - 1];
      const bool x3 = options().train_x3 != 0 && p->weight_t[l] && p->weight_t_x3[l] && gemm_train_x3_applicable(g.M, g.N, g.K);
      HIP_CHECK(x3 ? launch_gemm_train_x3(g, p->weight_t_x3[l], 2, stream) : launch_gemm_train(g, 0, 2, stream), "fused dX gemm");
      if (epi) {
        BnFinishBwdArgs f{};
        f.M = M; f.C = H; f.part = w.part; f.gamma = p->bn_weight[l - 1]; f.mean = stats_of(l - 1); f.rstd = f.mean + H;
        f.dgamma = gr->bn_weight[l - 1]; f.dbeta = gr->bn_bias[l - 1]; f.dslope = gr->prelu[l - 1];
        f.dslope_partial = w.slope_partial; f.counter = w.counter; f.accumulate = accumulate;
        f.dyh = dz_of(l - 1); f.ld = H; f.y = layer_save(l - 1); f.ldy = H;
        HIP_CHECK(launch_bn_finish_bwd(f, stream), "bn finish backward");
        continue;
      }
      BnFusedBwdArgs c{};
      c.M = M; c.C = H; c.part = w.part; c.gamma = p->bn_weight[l - 1]; c.mean = stats_of(l - 1); c.rstd = stats_of(l - 1) + H;
      c.dgamma = gr->bn_weight[l - 1]; c.dbeta = gr->bn_bias[l - 1]; c.dslope = gr->prelu[l - 1];
      c.dslope_partial = w.slope_partial; c.coef = w.coef; c.accumulate = accumulate;
      HIP_CHECK(launch_bn_fused_combine_bwd(c, stream), "fused bn reverse combine");
      HIP_CHECK(launch_bn_fused_apply_bwd(dz_of(l - 1), layer_save(l - 1), w.coef, M, H, stream), "fused bn reverse apply");
    }
    return EMPOSE_OK;
  }
  // output layer: dW = d_out^T a_{L-2}, db, dA = d_out . W
  {
    const int l = L - 1;
    if (stash) {   // weight gradients deferred: keep d_out for empose_mlp_train_wgrad (no copy when the caller
                   // produced it in its stash slot already, include/empose_hip.h)
      float* slot = stash + (size_t)M * (L - 1) * H;
      if (d_out != slot || ld_dout != op) {
        HIP_CHECK(launch_axpby2d(M, op, 1.f, d_out, ld_dout, 0.f, nullptr, 0, slot, op, stream), "stash");
      }
    } else {
      AtbArgs ab{};
      ab.A = d_out; ab.lda = ld_dout; ab.B = layer_save(l - 1) + (size_t)M * H; ab.ldb = H; ab.C = gr->weight[l]; ab.ldc = H;
      ab.bias = gr->bias[l]; ab.M = M; ab.N = p->out_dim; ab.K = H; ab.accumulate = accumulate;
      HIP_CHECK(launch_gemm_atb(ab, w.atb, w.atb_floats, stream), "dW");
    }
    const float* wt = p->weight_t[l];
    if (!wt) {
      HIP_TRY(hipMemsetAsync(w.wt, 0, (size_t)H * op * sizeof(float), stream));
      HIP_CHECK(launch_transpose(p->weight[l], H, w.wt, op, p->out_dim, H, stream), "transpose");
      wt = w.wt;
    }
    HIP_CHECK(gemm(d_out, ld_dout, wt, op, w.d[0], H, H, op), "dX gemm");
  }
  const int cur = 0;   // w.d[0]: cotangent of the current layer's activation; w.d[1]: dZ when it is not stashed
  for (int l = L - 2; l >= 0; --l) {
    const float* sv = layer_save(l);
    BnPreluArgs a{};
    a.M = M; a.C = H; a.x = sv; a.ldx = H; a.gamma = p->bn_weight[l]; a.beta = p->bn_bias[l]; a.slope = p->prelu[l];
    a.save_mean = const_cast<float*>(sv + (size_t)2 * M * H); a.save_rstd = a.save_mean + H;
    float* dz = stash ? stash + (size_t)M * l * H : w.d[cur ^ 1];   // dZ_l: into the stash when the dW are deferred
    a.dz = w.d[cur]; a.lddz = H; a.dx = dz; a.lddx = H;
    a.dgamma = gr->bn_weight[l]; a.dbeta = gr->bn_bias[l]; a.dslope = gr->prelu[l];
    a.dslope_partial = w.slope_partial; a.counter = w.counter; a.workspace = w.bn; a.accumulate = accumulate;
    HIP_CHECK(launch_bn_prelu(a, true, stream), "bn_prelu backward");
    const float* in = l == 0 ? x : layer_save(l - 1) + (size_t)M * H;
    const int ld_in = l == 0 ? ldx : H, k_in = l == 0 ? p->in_dim : H;
    if (!stash) {
      AtbArgs ab{};
      ab.A = dz; ab.lda = H; ab.B = in; ab.ldb = ld_in; ab.C = gr->weight[l]; ab.ldc = k_in;
      ab.bias = gr->bias[l]; ab.M = M; ab.N = H; ab.K = k_in; ab.accumulate = accumulate;
      HIP_CHECK(launch_gemm_atb(ab, w.atb, w.atb_floats, stream), "dW");
    }
    if (l == 0) break;
    const float* wt = p->weight_t[l];
    if (!wt) {
      HIP_CHECK(launch_transpose(p->weight[l], H, w.wt, H, H, H, stream), "transpose");
      wt = w.wt;
    }
    HIP_CHECK(gemm(dz, H, wt, H, w.d[cur], H, H, H), "dX gemm");   // the cotangent of the layer below overwrites the consumed one
  }
  return EMPOSE_OK;
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
  GemmBatch b;
  b.count = 1;
  GemmProb& p = b.p[0];
  p.A = A; p.lda = lda; p.W = W; p.ldw = ldw; p.C = C; p.ldc = ldc; p.M = M; p.N = N; p.K = K;
  p.scale = scale; p.shift = shift; p.resid = resid; p.ldr = ldr; p.act = act; p.slope = slope;
  HIP_CHECK(launch_gemm(b, static_cast<hipStream_t>(stream_)), "gemm launch");
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
  return mlp_train_cols(p, M) ? 0 : 1;
}

int empose_mlp_train_save_layout(const empose_mlp_params* p, int M) {
  if (!p || M <= 0) return fail(EMPOSE_EINVAL, "null parameters / no rows");
  if (p->save_layout < 0 || p->save_layout > 3) return fail(EMPOSE_EINVAL, "save_layout must be 0 .. 3");
  return mlp_train_fused(p, M) ? 2 : (mlp_train_epi(p, M) ? 3 : 1);
}

size_t empose_mlp_train_save_floats(const empose_mlp_params* p, int M) {
  if (!p || M <= 0) return 0;
  return (size_t)(p->n_layers - 1) * mlp_layer_save(p, M);
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
  MlpTrainWs w = carve_mlp_train(c, p, M);
  const int H = p->hidden, L = p->n_layers;
  if (mlp_train_cols(p, M)) return mlp_fwd_cols(&p, 1, M, x, ldx, &out, &ld_out, &save, w, stream);
  if (mlp_train_epi(p, M)) {
    // y_l = a_{l-1} W_l^T + b_l on the materialised a_{l-1}; the epilogue leaves the column statistics of y_l per row
    // block; ONE launch turns them into (mean, rstd, s, t), updates the running statistics and writes a_l = PReLU(s y_l + t)
    const size_t lsz = mlp_layer_save(p, M);
    for (int l = 0; l < L; ++l) {
      const bool last = l == L - 1;
      float* sv = save + (size_t)l * lsz;                      // this layer's y | a | mean | rstd | s | t
      const float* pa = l > 0 ? save + (size_t)(l - 1) * lsz + (size_t)M * H : nullptr;
      TrainGemmArgs g{};
      g.A = l == 0 ? x : pa; g.lda = l == 0 ? ldx : H; g.W = p->weight[l]; g.ldw = l == 0 ? p->in_dim : H;
      g.C = last ? out : sv; g.ldc = last ? ld_out : H;
      g.M = M; g.N = last ? p->out_dim : H; g.K = l == 0 ? p->in_dim : H; g.bias = p->bias[l];
      g.part = w.part;
      const bool x3 = !last && options().train_x3 != 0 && p->weight_x3[l] && gemm_train_x3_applicable(g.M, g.N, g.K);
      HIP_CHECK(x3 ? launch_gemm_train_x3(g, p->weight_x3[l], 1, stream) : launch_gemm_train(g, 0, last ? 0 : 1, stream), "mlp forward gemm (statistics epilogue)");
      if (last) break;
      BnFinishFwdArgs c{};
      c.M = M; c.C = H; c.part = w.part; c.gamma = p->bn_weight[l]; c.beta = p->bn_bias[l];
      c.eps = p->bn_eps; c.momentum = p->bn_momentum; c.running_mean = p->bn_running_mean[l];
      c.running_var = p->bn_running_var[l]; c.num_batches_tracked = p->bn_num_batches[l];
      c.mean = sv + (size_t)2 * M * H; c.rstd = c.mean + H; c.s = c.rstd + H; c.t = c.s + H;
      c.y = sv; c.ldy = H; c.act = sv + (size_t)M * H; c.ld_act = H; c.slope = p->prelu[l];
      HIP_CHECK(launch_bn_finish_fwd(c, stream), "bn finish forward");
    }
    return EMPOSE_OK;
  }
  if (mlp_train_fused(p, M)) {
    // y_l = a_{l-1} W_l^T + b_l with a_{l-1} = PReLU(s y_{l-1} + t) formed while the GEMM stages its A operand; the
    // epilogue leaves the column statistics of y_l per row block, a small kernel turns them into (mean, rstd, s, t)
    const size_t lsz = mlp_layer_save(p, M);
    for (int l = 0; l < L; ++l) {
      const bool last = l == L - 1;
      float* sv = save + (size_t)l * lsz;                      // this layer's y | mean | rstd | s | t
      const float* pv = l > 0 ? save + (size_t)(l - 1) * lsz : nullptr;
      TrainGemmArgs g{};
      g.A = l == 0 ? x : pv; g.lda = l == 0 ? ldx : H; g.W = p->weight[l]; g.ldw = l == 0 ? p->in_dim : H;
      g.C = last ? out : sv; g.ldc = last ? ld_out : H;
      g.M = M; g.N = last ? p->out_dim : H; g.K = l == 0 ? p->in_dim : H; g.bias = p->bias[l];
      if (l > 0) { g.a_s = pv + (size_t)M * H + 2 * H; g.a_t = g.a_s + H; g.a_slope = p->prelu[l - 1]; }
      g.part = w.part;
      HIP_CHECK(launch_gemm_train(g, l > 0 ? 1 : 0, last ? 0 : 1, stream), "fused mlp forward gemm");
      if (last) break;
      BnFusedFwdArgs c{};
      c.M = M; c.C = H; c.part = w.part; c.gamma = p->bn_weight[l]; c.beta = p->bn_bias[l];
      c.eps = p->bn_eps; c.momentum = p->bn_momentum; c.running_mean = p->bn_running_mean[l];
      c.running_var = p->bn_running_var[l]; c.num_batches_tracked = p->bn_num_batches[l];
      c.mean = sv + (size_t)M * H; c.rstd = c.mean + H; c.s = c.rstd + H; c.t = c.s + H;
      HIP_CHECK(launch_bn_fused_combine_fwd(c, stream), "fused bn combine");
    }
    return EMPOSE_OK;
  }
  const float* in = x;
  int ld_in = ldx, k_in = p->in_dim;
  for (int l = 0; l < L; ++l) {
    const bool last = l == L - 1;
    float* sv = save + (size_t)l * mlp_layer_save(p, M);
    float* z = last ? out : sv;
    GemmBatch b;
    b.count = 1;
    GemmProb& g = b.p[0];
    g.A = in; g.lda = ld_in; g.W = p->weight[l]; g.ldw = k_in; g.C = z; g.ldc = last ? ld_out : H;
    g.M = M; g.N = last ? p->out_dim : H; g.K = k_in;
    g.scale = nullptr; g.shift = p->bias[l]; g.resid = nullptr; g.ldr = 0; g.act = 0; g.slope = 0.f;
    HIP_CHECK(launch_gemm(b, stream), "mlp forward gemm");
    if (last) break;
    float* act = sv + (size_t)M * H;
    BnPreluArgs a{};
    a.M = M; a.C = H; a.x = z; a.ldx = H; a.gamma = p->bn_weight[l]; a.beta = p->bn_bias[l]; a.slope = p->prelu[l];
    a.eps = p->bn_eps; a.momentum = p->bn_momentum; a.running_mean = p->bn_running_mean[l];
    a.running_var = p->bn_running_var[l]; a.num_batches_tracked = p->bn_num_batches[l];
    a.z = act; a.ldz = H; a.save_mean = sv + (size_t)2 * M * H; a.save_rstd = a.save_mean + H;
    a.workspace = w.bn;
    HIP_CHECK(launch_bn_prelu(a, false, stream), "bn_prelu forward");
    in = act; ld_in = H; k_in = H;
  }
  return EMPOSE_OK;
}

int empose_mlp_train_bwd(const empose_mlp_params* p, int M, const float* x, int ldx, const float* d_out, int ld_dout,
                         const float* save, const empose_mlp_grads* gr, int accumulate, void* workspace,
                         size_t workspace_bytes, empose_stream_t stream) {
  return mlp_train_bwd_impl(p, M, x, ldx, d_out, ld_dout, save, gr, accumulate, nullptr, workspace, workspace_bytes, stream);
}

size_t empose_mlp_train_stash_floats(const empose_mlp_params* p, int M) {
  if (!p || M <= 0 || check_mlp_params(p) != EMPOSE_OK) return 0;
  return mlp_stash_floats(p, M);
}

int empose_mlp_train_bwd_deferred(const empose_mlp_params* p, int M, const float* x, int ldx, const float* d_out,
                                  int ld_dout, const float* save, const empose_mlp_grads* gr, int accumulate,
                                  float* dz_stash, void* workspace, size_t workspace_bytes, empose_stream_t stream) {
  if (!dz_stash) return fail(EMPOSE_EINVAL, "null stash");
  return mlp_train_bwd_impl(p, M, x, ldx, d_out, ld_dout, save, gr, accumulate, dz_stash, workspace, workspace_bytes, stream);
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
  if (M > 0 && x && out0 && out1 && save0 && save1 && workspace && ldx % 4 == 0 && ldx >= p0->in_dim && ldx >= p1->in_dim &&
      ld_out0 >= p0->out_dim && ld_out1 >= p1->out_dim && mlp_cols_pairable(p0, p1, M)) {
    Carver c(workspace);
    MlpTrainWs w = carve_mlp_train(c, p0, M);
    const empose_mlp_params* ps[2] = {p0, p1};
    float* outs[2] = {out0, out1};
    const int lds[2] = {ld_out0, ld_out1};
    float* saves[2] = {save0, save1};
    return mlp_fwd_cols(ps, 2, M, x, ldx, outs, lds, saves, w, static_cast<hipStream_t>(stream_));
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
  bool pair = M > 0 && x && d_out0 && d_out1 && save0 && save1 && gr0 && gr1 && workspace && mlp_cols_pairable(p0, p1, M) &&
              ld_dout0 % 4 == 0 && ld_dout1 % 4 == 0 && ld_dout0 >= ((p0->out_dim + 3) & ~3) && ld_dout1 >= ((p1->out_dim + 3) & ~3);
  for (int l = 0; l < p0->n_layers - 1 && pair; ++l)
    if (!gr0->bn_weight[l] || !gr0->bn_bias[l] || !gr0->prelu[l] || !gr1->bn_weight[l] || !gr1->bn_bias[l] || !gr1->prelu[l])
      pair = false;
  if (pair) {
    Carver c(workspace);
    MlpTrainWs w = carve_mlp_train(c, p0, M);
    const empose_mlp_params* ps[2] = {p0, p1};
    const float* d_outs[2] = {d_out0, d_out1};
    const int lds[2] = {ld_dout0, ld_dout1};
    const float* saves[2] = {save0, save1};
    const empose_mlp_grads* grs[2] = {gr0, gr1};
    float* stashes[2] = {dz_stash0, dz_stash1};
    return mlp_bwd_cols(ps, 2, M, x, ldx, d_outs, lds, saves, grs, accumulate, stashes, w, static_cast<hipStream_t>(stream_));
  }
  TRY(empose_mlp_train_bwd_deferred(p0, M, x, ldx, d_out0, ld_dout0, save0, gr0, accumulate, dz_stash0, workspace,
                                    workspace_bytes, stream_));
  return empose_mlp_train_bwd_deferred(p1, M, x, ldx, d_out1, ld_dout1, save1, gr1, accumulate, dz_stash1, workspace,
                                       workspace_bytes, stream_);
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
  const int H = p->hidden, L = p->n_layers, op = (p->out_dim + 3) & ~3;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  float* ws = static_cast<float*>(workspace);
  const size_t ws_floats = workspace_bytes / sizeof(float);
  // one product over all applications when their rows can be addressed as 32-row aligned segments, else one per application
  bool batched = M % 32 == 0 && ldx % 4 == 0;
  for (int s = 0; s < n_app && batched; ++s)
    batched = x[s] && save[s] && dz_stash[s] && ((uintptr_t)x[s] & 15) == 0 && ((uintptr_t)save[s] & 15) == 0 &&
              ((uintptr_t)dz_stash[s] & 15) == 0;
  for (int s = 0; s < n_app; ++s)
    if (!x[s] || !save[s] || !dz_stash[s]) return fail(EMPOSE_EINVAL, "null argument");
  const bool fused = mlp_train_fused(p, M);
  for (int l = 0; l < L; ++l) {
    if (!gr->weight[l] || !gr->bias[l]) return fail(EMPOSE_EINVAL, "null gradient output");
    const bool last = l == L - 1;
    const int ld_a = last ? op : H, n_out = last ? p->out_dim : H;
    const int ld_b = l == 0 ? ldx : H, k_in = l == 0 ? p->in_dim : H;
    if (fused) {
      // operands as the fused sweeps left them: dY_l (stash), y_{l-1} and its (s, t) (save)
      const size_t lsz = mlp_layer_save(p, M);
      AtbArgs ab{};
      ab.lda = ld_a; ab.ldb = ld_b; ab.C = gr->weight[l]; ab.ldc = k_in; ab.bias = gr->bias[l]; ab.N = n_out; ab.K = k_in;
      ab.b_mode = l > 0 ? 1 : 0; ab.b_slope = l > 0 ? p->prelu[l - 1] : nullptr;
      auto fill = [&](int slot, int s) {
        ab.A_seg[slot] = dz_stash[s] + (size_t)M * l * H;
        ab.B_seg[slot] = l == 0 ? x[s] : save[s] + (size_t)(l - 1) * lsz;
        ab.Bs_seg[slot] = l > 0 ? save[s] + (size_t)(l - 1) * lsz + (size_t)M * H + 2 * H : nullptr;
      };
      if (batched) {
        for (int s = 0; s < n_app; ++s) fill(s, s);
        ab.A = ab.A_seg[0]; ab.B = ab.B_seg[0]; ab.M = n_app * M; ab.accumulate = accumulate;
        ab.n_seg = n_app; ab.seg_rows = M;
        HIP_CHECK(launch_gemm_atb(ab, ws, ws_floats, stream), "fused dW");
      } else {
        for (int s = 0; s < n_app; ++s) {
          fill(0, s);
          ab.A = ab.A_seg[0]; ab.B = ab.B_seg[0]; ab.M = M; ab.accumulate = accumulate || s > 0;
          HIP_CHECK(launch_gemm_atb(ab, ws, ws_floats, stream), "fused dW");
        }
      }
      continue;
    }
    auto a_of = [&](int s) { return dz_stash[s] + (size_t)M * l * H; };
    auto b_of = [&](int s) { return l == 0 ? x[s] : save[s] + (size_t)(l - 1) * mlp_layer_save(p, M) + (size_t)M * H; };
    AtbArgs ab{};
    ab.lda = ld_a; ab.ldb = ld_b; ab.C = gr->weight[l]; ab.ldc = k_in; ab.bias = gr->bias[l]; ab.N = n_out; ab.K = k_in;
    if (batched) {
      ab.A = a_of(0); ab.B = b_of(0); ab.M = n_app * M; ab.accumulate = accumulate;
      ab.n_seg = n_app; ab.seg_rows = M;
      for (int s = 0; s < n_app; ++s) { ab.A_seg[s] = a_of(s); ab.B_seg[s] = b_of(s); }
      HIP_CHECK(launch_gemm_atb(ab, ws, ws_floats, stream), "dW");
    } else {
      for (int s = 0; s < n_app; ++s) {
        ab.A = a_of(s); ab.B = b_of(s); ab.M = M; ab.accumulate = accumulate || s > 0;
        HIP_CHECK(launch_gemm_atb(ab, ws, ws_floats, stream), "dW");
      }
    }
  }
  return EMPOSE_OK;
}

int empose_linear_f32(const float* A, int lda, const float* W, int ldw, float* C, int ldc, int M, int N, int K,
                      const float* scale, const float* shift, int prelu, float slope, empose_stream_t stream_) {
  if (!A || !W || !C) return fail(EMPOSE_EINVAL, "null argument");
  if (K % 4 != 0 || lda % 4 != 0 || ldw % 4 != 0) return fail(EMPOSE_EINVAL, "K, lda, ldw must be multiples of 4");
  if (((uintptr_t)A & 15) || ((uintptr_t)W & 15)) return fail(EMPOSE_EINVAL, "A and W must be 16-byte aligned");
  GemmBatch b;
  b.count = 1;
  GemmProb& p = b.p[0];
  p.A = A; p.lda = lda; p.W = W; p.ldw = ldw; p.C = C; p.ldc = ldc; p.M = M; p.N = N; p.K = K;
  p.scale = scale; p.shift = shift; p.resid = nullptr; p.ldr = 0; p.act = prelu ? 1 : 0; p.slope = slope;
  HIP_CHECK(launch_gemm(b, static_cast<hipStream_t>(stream_)), "gemm launch");
  return EMPOSE_OK;
}

}  // extern "C"
