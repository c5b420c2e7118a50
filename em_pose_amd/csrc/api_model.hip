// C ABI (include/empose_hip.h), the LGD model: weight packing, empose_model_create, the SMPL / update-net / LGD
// workspaces and the launch sequence of the LGD loop; the stand-alone SMPL and update-net entry points.
#include "api_internal.h"
#include "f16pair.h"
#include "gemm_kernels.h"
#include "mlp_kernels.h"
#include "options.h"
#include "smpl_kernels.h"

#include <cmath>

using namespace empose;
using namespace empose::api;

namespace {

// Packs every index/weight table the chain kernel needs into one array of 32-bit words (staged into LDS per block).
int build_chain_blob(const empose_smpl_desc& s, std::vector<uint32_t>& blob, ChainTabs& off, int* n_chunks) {
  auto put_i = [&](const std::vector<int>& v) { int o = (int)blob.size(); for (int x : v) blob.push_back((uint32_t)x); return o; };
  auto put_f = [&](const float* p, size_t n) {
    int o = (int)blob.size();
    for (size_t i = 0; i < n; ++i) { uint32_t u; std::memcpy(&u, p + i, 4); blob.push_back(u); }
    return o;
  };
  std::vector<int> path_mask(22, 0), sub_mask(22, 0), parents(s.parents, s.parents + 22);
  for (int j = 0; j < 22; ++j) {
    for (int q = s.path_ptr[j]; q < s.path_ptr[j + 1]; ++q) path_mask[j] |= 1 << s.path[q];
    for (int q = s.sub_ptr[j]; q < s.sub_ptr[j + 1]; ++q) sub_mask[j] |= 1 << s.sub[q];
  }
  off.path_mask = put_i(path_mask);
  off.sub_mask = put_i(sub_mask);
  off.parents = put_i(parents);
  {
    // depth-first pre-order: every subtree is a contiguous range, so a subtree sum is a difference of prefix sums
    std::vector<int> pos(22, 0), size(22, 0), stack, order;
    stack.push_back(0);
    while (!stack.empty()) {
      const int j = stack.back();
      stack.pop_back();
      pos[j] = (int)order.size();
      order.push_back(j);
      for (int c = 21; c >= 1; --c)
        if (parents[c] == j) stack.push_back(c);
    }
    for (int j = 0; j < 22; ++j) size[j] = __builtin_popcount((unsigned)sub_mask[j]);
    off.dfs_pos = put_i(pos);
    off.sub_size = put_i(size);
  }
  off.skin_idx = put_i(std::vector<int>(s.skin_idx, s.skin_idx + (size_t)s.nv * s.kb));
  off.skin_w = put_f(s.skin_w, (size_t)s.nv * s.kb);
  // per-bone (vertex, weight) lists cut into chunks of CHAIN_CHUNK pairs, each chunk padded with (vertex 0, weight 0)
  std::vector<int> cb, cbeg, bcp(23, 0), pv;
  std::vector<float> pw;
  for (int b = 0; b < 22; ++b) {
    bcp[b] = (int)cb.size();
    for (int q = s.bone_ptr[b]; q < s.bone_ptr[b + 1]; q += CHAIN_CHUNK) {
      cb.push_back(b);
      cbeg.push_back((int)pv.size());
      for (int k = 0; k < CHAIN_CHUNK; ++k) {
        const bool in = q + k < s.bone_ptr[b + 1];
        pv.push_back(in ? s.bone_vert[q + k] : 0);
        pw.push_back(in ? s.bone_w[q + k] : 0.f);
      }
    }
  }
  bcp[22] = (int)cb.size();
  *n_chunks = (int)cb.size();
  off.chunk_bone = put_i(cb); off.chunk_beg = put_i(cbeg);
  off.bone_chunk_ptr = put_i(bcp);
  off.bone_vert = put_i(pv);
  off.bone_w = put_f(pw.data(), pw.size());
  off.s_center = put_i(std::vector<int>(s.s_center, s.s_center + 12));
  off.s_helper = put_i(std::vector<int>(s.s_helper, s.s_helper + 12));
  off.s_deg = put_i(std::vector<int>(s.s_deg, s.s_deg + 12));
  {
    std::vector<int> faces(s.s_faces, s.s_faces + (size_t)12 * s.max_deg * 3);
    for (int m = 0; m < 12; ++m)
      for (int k = s.s_deg[m]; k < s.max_deg; ++k)
        for (int c = 0; c < 3; ++c) faces[((size_t)m * s.max_deg + k) * 3 + c] = s.s_center[m];
    off.s_faces = put_i(faces);
  }
  // Incidence lists of P4d as packed words (see the kernel): offsets are relative to the frame's LDS record.
  const ChainLds lay = chain_layout(s.nv, s.ncp, s.max_deg, *n_chunks);
  if (lay.total >= (1 << 13)) return fail(EMPOSE_EINVAL, "sensor sub-mesh too large for the packed incidence words");
  if (s.max_deg > 64) return fail(EMPOSE_EINVAL, "more than 64 faces around a sensor vertex");
  auto pack = [](int a, int b, int use_b, int neg) {
    return (int)((uint32_t)a | ((uint32_t)b << 13) | ((uint32_t)use_b << 26) | ((uint32_t)neg << 27));
  };
  std::vector<int> inc_ptr(s.nv + 1, 0), inc_code;
  for (int v = 0; v < s.nv; ++v) {
    inc_ptr[v] = (int)inc_code.size();
    for (int m = 0; m < 12; ++m) {
      if (s.s_center[m] == v) { const int o = lay.scr + m * 9 + 3; inc_code.push_back(pack(o, o, 0, 0)); }
      if (s.s_helper[m] == v) { const int o = lay.scr + m * 9 + 6; inc_code.push_back(pack(o, o, 0, 0)); }
      for (int k = 0; k < s.s_deg[m]; ++k)
        for (int c = 0; c < 3; ++c)
          if (s.s_faces[((size_t)m * s.max_deg + k) * 3 + c] == v) {
            const int fg = lay.fg + (m * s.max_deg + k) * 6;
            if (c == 0) inc_code.push_back(pack(fg, fg + 3, 1, 1));       // v0: -(d e1 + d e2)
            else if (c == 1) inc_code.push_back(pack(fg, fg, 0, 0));      // v1: + d e1
            else inc_code.push_back(pack(fg + 3, fg + 3, 0, 0));          // v2: + d e2
          }
    }
    while ((inc_code.size() - (size_t)inc_ptr[v]) % 4 != 0) inc_code.push_back((int)(1u << 28));   // null
  }
  inc_ptr[s.nv] = (int)inc_code.size();
  off.inc_ptr = put_i(inc_ptr);
  off.inc_code = put_i(inc_code);
  while (blob.size() % 4 != 0) blob.push_back(0u);   // staged into LDS in 16-byte pieces
  off.total = (int)blob.size();
  return EMPOSE_OK;
}

int pack_dense(std::vector<void*>& allocs, const empose_dense_desc& d, Dense* out) {
  if (d.in_dim <= 0 || d.out_dim <= 0 || !d.weight) return fail(EMPOSE_EINVAL, "dense layer: bad dims / null weight");
  if (d.in_dim % 4 != 0) return fail(EMPOSE_EINVAL, "dense layer: in_dim %d must be a multiple of 4", d.in_dim);
  out->in_dim = d.in_dim;
  out->out_dim = d.out_dim;
  TRY(upload(allocs, d.weight, (size_t)d.in_dim * d.out_dim, &out->w));
  std::vector<float> shift(d.out_dim, 0.f), scale;
  if (d.bn_weight) {
    if (!d.bn_bias || !d.bn_mean || !d.bn_var) return fail(EMPOSE_EINVAL, "dense layer: incomplete batch norm");
    scale.resize(d.out_dim);
    for (int n = 0; n < d.out_dim; ++n) {
      const double s = (double)d.bn_weight[n] / std::sqrt((double)d.bn_var[n] + (double)d.bn_eps);
      const double b = d.bias ? (double)d.bias[n] : 0.0;
      scale[n] = (float)s;
      shift[n] = (float)((b - (double)d.bn_mean[n]) * s + (double)d.bn_bias[n]);
    }
    TRY(upload(allocs, scale.data(), scale.size(), &out->scale));
  } else if (d.bias) {
    for (int n = 0; n < d.out_dim; ++n) shift[n] = d.bias[n];
  }
  TRY(upload(allocs, shift.data(), shift.size(), &out->shift));
  out->act = d.has_prelu ? 1 : 0;
  out->slope = d.prelu;
  return EMPOSE_OK;
}

// Weights in the order the matrix cores consume them (mlp_fused.hip): for every k-group of 8 and every 32-column tile,
// lane (n = lane & 31, half = lane >> 5) owns W[tile * 32 + n][kg * 8 + half * 4 .. + 3]; columns / k past the matrix
// are zero, so a wave's fragment is one coalesced 1 KB read and ragged K needs no masking on this operand.
int pack_fragments_raw(std::vector<void*>& allocs, const float* weight, int N, int K, float** out) {
  const int KG = (K + 7) / 8, NT = (N + 31) / 32;
  const int KG4 = (KG + 3) & ~3;   // the kernels walk four k-groups per iteration
  std::vector<float> buf((size_t)KG4 * NT * 256, 0.f);
  for (int kg = 0; kg < KG; ++kg)
    for (int nt = 0; nt < NT; ++nt)
      for (int lane = 0; lane < 64; ++lane) {
        const int n = nt * 32 + (lane & 31);
        if (n >= N) continue;
        for (int e = 0; e < 4; ++e) {
          const int k = kg * 8 + (lane >> 5) * 4 + e;
          if (k < K) buf[(((size_t)kg * NT + nt) * 64 + lane) * 4 + e] = weight[(size_t)n * K + k];
        }
      }
  return upload(allocs, buf.data(), buf.size(), out);
}

// The order the piece kernels of mlp_fused_x3.hip consume their weights in: fragment f = ks * NT + tile of
// [k-steps of S][tiles of C columns], and in it lane owns row[tile * C + (lane mod C)], k0 = ks * S + (lane / C) * 8 .. + 7.
// C, S = 32, 16 for v_mfma_f32_32x32x16_bf16 and 16, 32 for the 16x16x32 instructions.  The k-steps are padded with zeros
// to a multiple of PAD (the steps the kernel's loop walks at a time: the padding starts past K, so nothing is written
// there); columns past N and k past K are zero too, so a wave's fragment is one coalesced 1 KB read per piece and ragged
// K needs no masking on this operand.
struct FragOrder {
  int C, S, N, K, NT, KSP;
  FragOrder(int C_, int S_, int PAD, int N_, int K_)
      : C(C_), S(S_), N(N_), K(K_), NT((N_ + C_ - 1) / C_), KSP(((K_ + S_ - 1) / S_ + PAD - 1) & ~(PAD - 1)) {}
  size_t n_frag() const { return (size_t)KSP * NT; }
  bool owns(size_t f, int lane, int* n, int* k0) const {
    *n = (int)(f % NT) * C + lane % C;
    *k0 = (int)(f / NT) * S + lane / C * 8;
    return *n < N;
  }
};
// The weights as three bf16 pieces each (split3) in that order: [fragment][piece] -> 1 KB, 6 bytes per weight.
int pack_x3_order(std::vector<void*>& allocs, const float* weight, const FragOrder& o, float** out) {
  return upload_bf16(allocs, pack_fragments_x3(o.n_frag(), o.K, [&](size_t f, int lane, const float** row, int* k0) {
    int n;
    if (!o.owns(f, lane, &n, k0)) return false;
    *row = weight + (size_t)n * o.K;
    return true;
  }), out);
}
// ... for v_mfma_f32_32x32x16_bf16 (mlp_fused_x3_kernel<32>, whose loop walks quads of k-steps; also x3_rows_layer's)
int pack_fragments_x3_raw(std::vector<void*>& allocs, const float* weight, int N, int K, float** out) {
  return pack_x3_order(allocs, weight, FragOrder(32, 16, 4, N, K), out);
}
// ... and for v_mfma_f32_16x16x32_bf16 (mlp_fused_x3_kernel<16>, whose loop walks pairs)
int pack_fragments_x3_16_raw(std::vector<void*>& allocs, const float* weight, int N, int K, float** out) {
  return pack_x3_order(allocs, weight, FragOrder(16, 32, 2, N, K), out);
}

// The weights as TWO f16 pieces each (f16pair.h) in the order of the 16x16x32 instruction: [fragment][piece] -> 1 KB.
// Output column n's pieces are those of W[n][:] 2^e(n), e(n) from the column's largest magnitude; inv[n] = 2^-e(n) is
// what the kernel's epilogue multiplies the accumulator by.
int pack_fragments_pair16_raw(std::vector<void*>& allocs, const float* weight, int N, int K, float** out, float** inv_out) {
  const FragOrder o(16, 32, 2, N, K);
  std::vector<unsigned short> buf(o.n_frag() * 2 * FRAG, 0);
  std::vector<float> inv(N, 1.f), sc(N, 1.f);
  for (int n = 0; n < N; ++n) {
    unsigned m = 0u;
    for (int k = 0; k < K; ++k) {
      const unsigned b = pair16::finite_abs_bits(weight[(size_t)n * K + k]);
      m = b > m ? b : m;
    }
    const int e = pair16::scale_exp(m);
    sc[n] = pair16::pow2(e);
    inv[n] = pair16::pow2(-e);
  }
  for (size_t f = 0; f < o.n_frag(); ++f)
    for (int lane = 0; lane < 64; ++lane) {
      int n, k0;
      if (!o.owns(f, lane, &n, &k0)) continue;
      for (int e = 0; e < 8 && k0 + e < K; ++e) {
        const float x = weight[(size_t)n * K + k0 + e] * sc[n];
        const _Float16 hi = (_Float16)x;                       // round to nearest even
        const _Float16 lo = (_Float16)(x - (float)hi);
        const size_t at = f * 2 * FRAG + (size_t)lane * 8 + e;
        buf[at] = __builtin_bit_cast(unsigned short, hi);
        buf[at + FRAG] = __builtin_bit_cast(unsigned short, lo);
      }
    }
  TRY(upload_bf16(allocs, buf, out));
  return upload(allocs, inv.data(), inv.size(), inv_out);
}

// Every form's order is packed here, at creation: the options choose between them at run time, and the library does
// not allocate after creation (16 bytes per weight together).
int pack_fragments(std::vector<void*>& allocs, const empose_dense_desc& d, Dense* out) {
  auto frag = [&](FusedForm f) { return &out->frag[(int)f]; };
  TRY(pack_fragments_x3_raw(allocs, d.weight, d.out_dim, d.in_dim, frag(FusedForm::x3_32)));
  TRY(pack_fragments_x3_16_raw(allocs, d.weight, d.out_dim, d.in_dim, frag(FusedForm::x3_16)));
  TRY(pack_fragments_pair16_raw(allocs, d.weight, d.out_dim, d.in_dim, frag(FusedForm::pair16), &out->wexp));
  return pack_fragments_raw(allocs, d.weight, d.out_dim, d.in_dim, frag(FusedForm::fp32));
}

int pack_mlp(std::vector<void*>& allocs, const empose_mlp_desc& d, Mlp* out, int* hidden_max, int* any_skip) {
  out->n_layers = d.n_layers;
  out->skip = d.skip;
  if (d.n_layers == 0) return EMPOSE_OK;
  if (d.skip) *any_skip = 1;
  if (d.n_layers < 2 || d.n_layers > EMPOSE_MAX_DENSE || (d.n_layers % 2) != 0)
    return fail(EMPOSE_EINVAL, "mlp: n_layers=%d unsupported", d.n_layers);
  for (int i = 0; i < d.n_layers; ++i) {
    TRY(pack_dense(allocs, d.layers[i], &out->layers[i]));
    TRY(pack_fragments(allocs, d.layers[i], &out->layers[i]));
    if (i > 0 && d.layers[i].in_dim != d.layers[i - 1].out_dim) return fail(EMPOSE_EINVAL, "mlp: layer dims do not chain");
    if (i + 1 < d.n_layers && d.layers[i].out_dim > *hidden_max) *hidden_max = d.layers[i].out_dim;
  }
  return EMPOSE_OK;
}

// ---- workspace layouts ------------------------------------------------------------------------------------------
struct SmplWs {
  float *rot, *feat, *out, *d_out, *d_feat, *d_rot;
  float* theta_t;   // theta in tile layout for the frame-per-lane kernel
  float* tgt_t;     // targets in tile layout (stand-alone entry points; the LGD loop has its own copy)
};
constexpr int D_FEAT_T_COLS = 224;   // the 200 feature cotangents in tile layout, whole 32-column tiles
SmplWs carve_smpl(Carver& c, const empose_model* m, int T) {
  // Either path fits: row-major [T][cols] for chain_sensors_kernel, tile layout [ceil(T / 64)][cols][64] for
  // smpl_tile_kernel (which does not use `rot`: it evaluates Rodrigues itself).
  SmplWs w;
  const size_t Tp = (size_t)(T + TL_FR - 1) / TL_FR * TL_FR;
  const size_t ncp = m->tab.ncp > m->ncp2 ? m->tab.ncp : m->ncp2;
  w.rot = c.f((size_t)T * 198);
  w.feat = c.f((size_t)T * 200);
  w.out = c.f(Tp * ncp);
  w.d_out = c.f(Tp * ncp);
  w.d_feat = c.f(Tp * D_FEAT_T_COLS);
  w.d_rot = c.f(Tp * 198);
  w.theta_t = c.f(Tp * 66);
  w.tgt_t = c.f(Tp * 144);
  return w;
}

struct UpdWs { float* buf[3]; };  // [2 nets][T][hidden_max] each; buf[2] only when a net uses skip connections
UpdWs carve_upd(Carver& c, const empose_model* m, int T) {
  const size_t n = (size_t)2 * T * m->hidden_max;
  return {{c.f(n), c.f(n), m->any_skip ? c.f(n) : nullptr}};
}

// One or two MLPs that share the input x (the update nets / the init nets), both nets per launch.
struct MlpRun {
  const Mlp* nets[2]; int n_nets;
  float* outs[2]; int out_ld[2];
  const float* x; int ldx; int T;
  bool init_net;   // (profiler tag only)
};

// Large batches: every layer of both nets in ONE launch (mlp_fused.hip); a workgroup keeps 128 rows through all the
// layers. Needs enough row panels to fill the chip and layers no wider than the four 128-column waves.
// form (FusedForm, mlp_kernels.h): each piece form rests on the one before it --
//   x3_32 (option mlp_x3): fp32 products from three bf16 pieces per operand on the bf16 matrix path (mlp_fused_x3.hip;
//          fp32-equivalent, 2.7 times the fp32 instruction's rate): needs every hidden width to be whole quads of k-steps
//          of the next layer;
//   x3_16 (option mlp_fused16): that kernel on the 16x16x32 form of the instruction;
//   pair16 (option mlp_pair16): its place taken by the kernel on two f16 pieces per operand.
struct MlpPlan { bool one_launch; FusedForm form; };
MlpPlan plan_mlps(const MlpRun& r) {
  const int L = r.nets[0]->n_layers;
  bool one_launch = options().mlp_fused != 0 && L <= FUSED_MAX_LAYERS && (long)((r.T + 63) / 64) * r.n_nets >= 256;
  bool x3 = options().mlp_x3 != 0, shape16 = options().mlp_fused16 != 0, pair16 = options().mlp_pair16 != 0;
  for (int i = 0; i < r.n_nets; ++i) {
    const Mlp& net = *r.nets[i];
    if (net.skip || net.layers[0].in_dim > FUSED_MAX_WIDTH) one_launch = false;   // no room for a block input
    for (int l = 0; l < L; ++l) {
      const Dense& d = net.layers[l];
      if (d.out_dim > FUSED_MAX_WIDTH || d.act > 1) one_launch = false;
      if (l + 1 < L && (d.out_dim % 64 != 0 || !d.frag[(int)FusedForm::x3_32])) x3 = false;
      if (!d.frag[(int)FusedForm::x3_16]) shape16 = false;
      if (!d.frag[(int)FusedForm::pair16] || !d.wexp) pair16 = false;
    }
  }
  return {one_launch, !x3 ? FusedForm::fp32 : !shape16 ? FusedForm::x3_32 : !pair16 ? FusedForm::x3_16 : FusedForm::pair16};
}

int run_mlps_one_launch(const MlpRun& r, FusedForm form, hipStream_t stream) {
  FusedMlpArgs fa;
  fa.count = r.n_nets; fa.M = r.T;
  for (int i = 0; i < r.n_nets; ++i) {
    FusedNet& fn = fa.net[i];
    fn.x = r.x; fn.ldx = r.ldx; fn.out = r.outs[i]; fn.ld_out = r.out_ld[i];
    fn.n_layers = r.nets[i]->n_layers;   // the activations stay in LDS: no scratch
    for (int l = 0; l < fn.n_layers; ++l) {
      const Dense& d = r.nets[i]->layers[l];
      FusedLayer& fl = fn.layer[l];
      fl.W = d.frag[(int)form];
      fl.wexp = form == FusedForm::pair16 ? d.wexp : nullptr;
      fl.K = d.in_dim; fl.N = d.out_dim; fl.scale = d.scale; fl.shift = d.shift;
      fl.slope = d.slope; fl.act = d.act;
    }
  }
  prof_mark(r.init_net ? P_INIT_MLP : P_MLP_FUSED, stream);
  HIP_CHECK(form == FusedForm::fp32 ? launch_mlp_fused(fa, stream) : launch_mlp_fused_x3(fa, form, stream), "fused mlp launch");
  prof_mark(P_END, stream);   // close the dominant kernel's interval at its completion, not at the next launch
  return EMPOSE_OK;
}

// Layer by layer.  Hidden blocks are layer pairs (1,2), (3,4), ...; with skip connections the block input is added to
// the block output (reference layers.py:35-43), which needs the block input kept alive in a third buffer.
int run_mlps_layers(const MlpRun& r, const UpdWs& ws, int hidden_max, hipStream_t stream) {
  const int L = r.nets[0]->n_layers, T = r.T;
  int cur[2] = {-1, -1}, block_in[2] = {-1, -1};
  for (int l = 0; l < L; ++l) {
    GemmBatch b;
    b.count = r.n_nets;
    int nxt[2] = {-1, -1};
    for (int i = 0; i < r.n_nets; ++i) {
      const Mlp& net = *r.nets[i];
      const Dense& d = net.layers[l];
      auto buf = [&](int k) { return ws.buf[k] + (size_t)i * T * hidden_max; };
      const float* in = (l == 0) ? r.x : buf(cur[i]);
      const int ld_in = (l == 0) ? r.ldx : net.layers[l - 1].out_dim;
      const bool block_first = (l >= 1) && (l % 2 == 1) && (l < L - 1);
      const bool block_last = (l >= 2) && (l % 2 == 0) && (l < L - 1);
      if (block_first) block_in[i] = cur[i];
      float* out = r.outs[i];
      int ld_out = r.out_ld[i];
      if (l < L - 1) {
        int k = 0;
        while (k == cur[i] || (net.skip && k == block_in[i])) ++k;
        if (k > 2 || !ws.buf[k]) return fail(EMPOSE_EINVAL, "internal: MLP scratch buffers exhausted");
        nxt[i] = k;
        out = buf(k);
        ld_out = d.out_dim;
      }
      b.p[i] = linear_prob(in, ld_in, d, out, ld_out, T);
      if (block_last && net.skip) {
        b.p[i].resid = buf(block_in[i]);
        b.p[i].ldr = d.out_dim;
      }
    }
    b.role = (!r.init_net && l > 0 && l < L - 1) ? 1 : 0;
    prof_mark(r.init_net ? P_INIT_MLP : (l == 0 ? P_MLP_IN : (l == L - 1 ? P_MLP_OUT : P_MLP_HIDDEN)), stream);
    HIP_CHECK(launch_gemm(b, stream), "gemm launch");
    for (int i = 0; i < r.n_nets; ++i) cur[i] = nxt[i];
  }
  return EMPOSE_OK;
}

int run_mlps(const MlpRun& r, const UpdWs& ws, int hidden_max, hipStream_t stream) {
  for (int i = 1; i < r.n_nets; ++i)
    if (r.nets[i]->n_layers != r.nets[0]->n_layers) return fail(EMPOSE_EINVAL, "paired MLPs must have the same depth");
  const MlpPlan p = plan_mlps(r);
  return p.one_launch ? run_mlps_one_launch(r, p.form, stream) : run_mlps_layers(r, ws, hidden_max, stream);
}

// Where the residual gradient of one SMPL evaluation goes.
struct GradOut {
  float* g_theta; int ld_g; float* g_beta; int ld_gb;
  float* trace_g_theta; float* trace_g_beta;
};
// One SMPL evaluation, as its caller asks for it.  What is not filled in is not wanted.
struct SmplEval {
  FeatArgs update;   // the pose / shape update and where its copies go (rot / feat / theta_t, T, F: filled in by run_smpl_eval)
  const float* offset_r = nullptr; const float* offset_t = nullptr;
  float* pos = nullptr; float* ori = nullptr; float* joints = nullptr;      // sensor outputs
  float* pos2 = nullptr; float* ori2 = nullptr; float* joints2 = nullptr;   // ... second copies
  // the reverse: none, or the residual against a target (tgt_t: its tile-layout copy, on the frame-per-lane path), or
  // external cotangents -- either needs `grad`
  const float* tgt = nullptr; int ld_tgt = 0; const float* frame_scale = nullptr; const float* tgt_t = nullptr;
  const float* cot_pos = nullptr; const float* cot_ori = nullptr; const float* cot_joints = nullptr;
  const GradOut* grad = nullptr;
};

// How an entry point evaluates SMPL: the one place that reads the options "smpl_tile", "smpl_fuse", "rows_x3" and
// "last_pass_joints" for this path.  The callers take from it whether scratch outputs and tile-layout targets are
// needed, the evaluation which launches to make.
//   tile  the frame-per-lane path.  It pays once its 64-frame workgroups fill the 256 CUs (one per CU, 152 KB of LDS
//         each): from 16384 frames on.  Measured at 8192 frames (the training step at 256 windows): 2 % slower than the
//         general kernel.  Option "smpl_tile": 0 never, 1 by size, 2 always (tests).  Joint cotangents: general path.
//   fuse, rx3  on that path the update + feature row and the Rodrigues reverse ride on the GEMMs ("smpl_fuse"), which
//         multiply three bf16 pieces per operand ("rows_x3")
//   bwd, joints_only  of the request: it wants a gradient; or ("last_pass_joints"; the last pass of an LGD forward
//         without histories) no gradient and no sensor output, so of the blend product only the 66 rest-joint columns are
//         read -- the GEMM multiplies just their column tiles (same fragments, same order: same bits) and the tile kernel
//         stops after the chain
struct SmplPlan {
  bool tile = false, fuse = false, rx3 = false, bwd = false, joints_only = false;
  bool joints_opt = false;   // "last_pass_joints" as read with the others
  // The same path for another request of the same call (the passes of the LGD loop); reads no option.
  SmplPlan with(const SmplEval& rq) const {
    SmplPlan p = *this;
    p.bwd = rq.tgt || rq.cot_pos;
    p.joints_only = fuse && joints_opt && !p.bwd && !rq.pos && !rq.ori && !rq.pos2 && !rq.ori2 && (rq.joints || rq.joints2);
    return p;
  }
};
SmplPlan plan_smpl(const empose_model* m, int T, const SmplEval& rq) {
  const Options& o = options();
  SmplPlan p;
  p.tile = m->tile_ok && o.smpl_tile != 0 && !rq.cot_joints && (o.smpl_tile == 2 || T >= 16384);
  p.fuse = p.tile && o.smpl_fuse != 0;
  p.rx3 = p.tile && o.rows_x3 != 0 && m->wc2_frag3 && m->wc2t_frag3;
  p.joints_opt = o.last_pass_joints != 0;
  return p.with(rq);
}

// What ChainArgs and TileArgs share: the sensor side of a request.
template <typename Args>
void set_sensor_io(Args& a, const empose_model* m, int T, int F, const SmplEval& rq) {
  a.offset_r = rq.offset_r; a.offset_t = rq.offset_t; a.tgt = rq.tgt; a.ld_tgt = rq.ld_tgt; a.frame_scale = rq.frame_scale;
  a.n_markers = m->n_markers;
  for (int i = 0; i < 12; ++i) a.used_slot[i] = m->used_slot[i];
  a.pos = rq.pos; a.ori = rq.ori; a.joints = rq.joints; a.pos2 = rq.pos2; a.ori2 = rq.ori2; a.joints2 = rq.joints2;
  a.T = T; a.F = F;
  a.cot_pos = rq.cot_pos; a.cot_ori = rq.cot_ori;
}
// What RodBwdArgs and RodBwdTArgs share.
template <typename Args>
void set_rod_bwd(Args& ra, const empose_model* m, int T, const SmplEval& rq) {
  ra.theta = rq.update.theta; ra.ld_theta = rq.update.ld_theta;
  ra.g_theta = rq.grad->g_theta; ra.ld_g = rq.grad->ld_g; ra.g_beta = rq.grad->g_beta; ra.ld_gb = rq.grad->ld_gb;
  ra.trace_g_theta = rq.grad->trace_g_theta; ra.trace_g_beta = rq.grad->trace_g_beta;
  ra.T = T; ra.rod_conv = m->rod_conv;
}

// Frame-per-lane path: blend GEMM -> tile layout -> smpl_tile_kernel -> tile layout -> transposed GEMM.
int smpl_eval_tile(const empose_model* m, int T, int F, const SmplWs& ws, const SmplPlan& plan, const SmplEval& rq,
                   hipStream_t stream) {
  const FeatArgs& fa = rq.update;
  const int lo = plan.joints_only ? m->tile_j_off2 : 0, hi = plan.joints_only ? m->tile_j_off2 + 66 : 0;
  prof_mark(P_BLEND_GEMM, stream);
  HIP_CHECK(plan.fuse ? launch_blend_feat_gemm(fa, plan.rx3 ? m->wc2_frag3 : m->wc2_frag, ws.out, m->ncp2, m->ncp2, plan.rx3, stream, lo, hi)
                      : launch_gemm_rows_t(ws.feat, 200, false, m->wc2_frag, ws.out, m->ncp2, T, m->ncp2, 200, stream),
            "blend gemm (tile)");
  TileArgs a;
  set_sensor_io(a, m, T, F, rq);
  a.tab = m->tile_tab; a.theta = fa.theta; a.ld_theta = fa.ld_theta; a.out_t = ws.out;
  a.theta_t = ws.theta_t; a.tgt_t = rq.tgt ? rq.tgt_t : nullptr;
  a.d_out_t = ws.d_out; a.d_rot_t = ws.d_rot; a.rod_conv = m->rod_conv;
  prof_mark(P_CHAIN, stream);
  HIP_CHECK(launch_smpl_tile(a, plan.bwd, m->tile_nloc, m->tile_nbl, stream, plan.joints_only), "smpl tile kernel");
  if (!plan.bwd) return EMPOSE_OK;
  RodBwdTArgs ra;
  set_rod_bwd(ra, m, T, rq);
  ra.theta_t = ws.theta_t; ra.d_rot_t = ws.d_rot; ra.d_feat_t = ws.d_feat; ra.ld_feat_t = D_FEAT_T_COLS;
  prof_mark(P_BLEND_T_GEMM, stream);
  if (plan.fuse) {
    HIP_CHECK(launch_blend_t_gemm_rod(ws.d_out, m->ncp2, plan.rx3 ? m->wc2t_frag3 : m->wc2t_frag, m->ncp2, ra, plan.rx3, stream), "blend^T gemm + rodrigues_bwd (tile)");
    return EMPOSE_OK;
  }
  HIP_CHECK(launch_gemm_rows_t(ws.d_out, m->ncp2, true, m->wc2t_frag, ws.d_feat, D_FEAT_T_COLS, T, 200, m->ncp2, stream), "blend^T gemm (tile)");
  prof_mark(P_ROD_BWD, stream);
  HIP_CHECK(launch_rodrigues_bwd_t(ra, stream), "rodrigues_bwd (tile) kernel");
  return EMPOSE_OK;
}

// General path: blend GEMM, chain + skinning + sensors (+ reverse), transposed GEMM, Rodrigues reverse.
int smpl_eval_rows(const empose_model* m, int T, int F, const SmplWs& ws, const SmplPlan& plan, const SmplEval& rq,
                   hipStream_t stream) {
  const int ncp = m->tab.ncp;
  GemmBatch b;
  b.count = 1;
  b.p[0] = plain_prob(ws.feat, 200, m->tab.wc, 200, ws.out, ncp, T, ncp, 200);
  prof_mark(P_BLEND_GEMM, stream);
  HIP_CHECK((m->wc_frag && gemm_rows_applicable(T, ncp, 200))
                ? launch_gemm_rows(ws.feat, 200, m->wc_frag, ws.out, ncp, T, ncp, 200, stream)
                : launch_gemm(b, stream), "blend gemm");
  ChainArgs c;
  set_sensor_io(c, m, T, F, rq);
  c.tab = m->tab;
  c.rot = ws.rot; c.out = ws.out; c.d_out = ws.d_out; c.d_rot = ws.d_rot; c.cot_joints = rq.cot_joints;
  prof_mark(P_CHAIN, stream);
  HIP_CHECK(launch_chain_sensors(c, stream), "chain kernel");
  if (!plan.bwd) return EMPOSE_OK;
  b.p[0] = plain_prob(ws.d_out, ncp, m->tab.wct, ncp, ws.d_feat, 200, T, 200, ncp);
  prof_mark(P_BLEND_T_GEMM, stream);
  HIP_CHECK((m->wct_frag && gemm_rows_applicable(T, 200, ncp))
                ? launch_gemm_rows(ws.d_out, ncp, m->wct_frag, ws.d_feat, 200, T, 200, ncp, stream)
                : launch_gemm(b, stream), "blend^T gemm");
  RodBwdArgs ra;
  set_rod_bwd(ra, m, T, rq);
  ra.d_rot = ws.d_rot; ra.d_feat = ws.d_feat;
  prof_mark(P_ROD_BWD, stream);
  HIP_CHECK(launch_rodrigues_bwd(ra, stream), "rodrigues_bwd kernel");
  return EMPOSE_OK;
}

// One SMPL evaluation by `plan` (made for this request): pose / shape update + feature row -- on the fused
// frame-per-lane path it rides on the blend GEMM -- then the path's own launches.
int run_smpl_eval(const empose_model* m, int T, int F, const SmplWs& ws, const SmplPlan& plan, SmplEval rq,
                  hipStream_t stream) {
  if (plan.bwd && !rq.grad) return fail(EMPOSE_EINVAL, "gradient outputs missing");
  FeatArgs& fa = rq.update;
  fa.rot = plan.tile ? nullptr : ws.rot; fa.feat = ws.feat; fa.theta_t = plan.tile ? ws.theta_t : nullptr;
  fa.T = T; fa.F = F; fa.rod_conv = m->rod_conv;
  if (!plan.fuse) {
    prof_mark(P_UPDATE_FEAT, stream);
    HIP_CHECK(launch_update_feat(fa, stream), "update_feat kernel");
  }
  return plan.tile ? smpl_eval_tile(m, T, F, ws, plan, rq, stream) : smpl_eval_rows(m, T, F, ws, plan, rq, stream);
}

struct LgdWs {
  float *x, *scale, *d_pose, *d_shape, *pos, *ori, *joints;
  float* x_t;   // the sensor columns of x in tile layout (targets of the frame-per-lane kernel)
  SmplWs smpl;
  UpdWs upd;
  LstmWs lstm;
  float* y;
};
LgdWs carve_lgd(Carver& c, const empose_model* m, int B, int F) {
  LgdWs w;
  const size_t T = (size_t)B * F;
  w.x = c.f(T * m->d_x);
  w.scale = c.f(T);
  w.d_pose = c.f(T * 66);
  w.d_shape = c.f(T * 10);
  w.pos = c.f(T * 36);
  w.ori = c.f(T * 108);
  w.joints = c.f(T * 66);
  w.x_t = c.f((T + TL_FR - 1) / TL_FR * TL_FR * m->d_in);
  w.smpl = carve_smpl(c, m, (int)T);
  w.upd = carve_upd(c, m, (int)T);
  if (m->rnn_init) {
    w.lstm = carve_lstm_of(c, m->rnn, B, F);
    w.y = c.f(T * m->rnn.H);
  } else {
    w.y = nullptr;
  }
  return w;
}


// One LGD forward: the model, the caller's tensors, the carved workspace and how this call evaluates SMPL.
struct LgdRun {
  const empose_model* m; const empose_lgd_io* io; int B, F, T;
  LgdWs w; SmplPlan path; hipStream_t stream;
  float* x_col(int c) const { return w.x + m->d_in + c; }   // the columns of the network input x after the sensors:
  float* x_theta() const { return x_col(0); }               // theta | beta | g_theta | g_beta
  float* x_beta() const { return x_col(66); }
};

// EMPOSE_LGD_PHASE_INIT: the network input and the initial estimate (reference models.py:511-526).
int lgd_init(const LgdRun& r) {
  const empose_model* m = r.m; const empose_lgd_io* io = r.io; const LgdWs& w = r.w;
  const int dx = m->d_x, T = r.T;
  PackArgs pa;
  pa.marker_pos = io->marker_pos; pa.marker_oris = io->marker_oris; pa.marker_masks = io->marker_masks;
  pa.seq_lengths = io->seq_lengths; pa.x = w.x; pa.ldx = dx; pa.frame_scale = w.scale;
  pa.B = r.B; pa.F = r.F; pa.n_markers = m->n_markers;
  pa.rows_as_unpadded = (m->shape_avg == 2) ? 1 : 0;
  pa.suppress_missing = io->suppress_missing; pa.mask_value = io->mask_value;
  for (int i = 0; i < 12; ++i) pa.marker_idx[i] = m->marker_idx[i];
  prof_mark(P_PACK, r.stream);
  HIP_CHECK(launch_pack_inputs(pa, r.stream), "pack kernel");
  if (m->use_gradient && m->N > 0 && r.path.tile)   // the targets of the frame-per-lane kernel, once per forward
    HIP_CHECK(launch_rows_to_tile(w.x, dx, m->d_in, w.x_t, T, r.stream), "tile transpose");
  if (!m->rnn_init) {
    const MlpRun init{{&m->pose_init, &m->shape_init}, 2, {r.x_theta(), w.d_shape}, {dx, 10}, w.x, dx, T, true};
    return run_mlps(init, w.upd, m->hidden_max, r.stream);
  }
  const int H = m->rnn.H;
  TRY(run_lstm(m->rnn, r.B, r.F, w.x, dx, io->seq_lengths, io->h0, io->c0, w.y, io->h_n, io->c_n, w.lstm, r.stream));
  GemmBatch b;
  b.count = 2;
  b.p[0] = linear_prob(w.y, H, m->pose_head, r.x_theta(), dx, T);
  b.p[1] = linear_prob(w.y, H, m->shape_head, w.d_shape, 10, T);
  prof_mark(P_HEADS, r.stream);
  const bool rows = m->heads_frag && options().heads_rows != 0 && heads_rows_applicable(T, H);
  const bool rx3 = options().rows_x3 != 0 && m->heads_frag3;
  HIP_CHECK(rows ? launch_heads_rows(w.y, H, rx3 ? m->heads_frag3 : m->heads_frag, m->heads_bias, r.x_theta(), dx,
                                     w.d_shape, 10, T, H, 66, 10, rx3, r.stream)
                 : launch_gemm(b, r.stream), "head gemm");
  return EMPOSE_OK;
}

// EMPOSE_LGD_PHASE_ITER: N + 1 SMPL evaluations with the update nets between them.
int lgd_iterate(const LgdRun& r) {
  const empose_model* m = r.m; const empose_lgd_io* io = r.io; const LgdWs& w = r.w;
  const int dx = m->d_x, T = r.T, N = m->N;
  const bool tile = r.path.tile;
  auto hist = [&](float* base, int i, size_t width) -> float* { return base ? base + (size_t)i * T * width : nullptr; };
  for (int i = 0; i <= N; ++i) {
    SmplEval rq;
    FeatArgs& fa = rq.update;
    fa.theta = r.x_theta(); fa.ld_theta = dx; fa.beta = r.x_beta(); fa.ld_beta = dx;
    fa.shape_avg = m->shape_avg; fa.seq_lengths = io->seq_lengths;
    fa.d_theta = i ? w.d_pose : nullptr; fa.theta_step = i ? m->step : 0.f;   // pass 0 takes the initial estimate as it is
    fa.d_beta = w.d_shape; fa.beta_keep = i ? 1.f : 0.f; fa.beta_step = i ? m->step : 1.f;
    fa.out_theta = hist(io->hist_pose, i, 66); fa.out_beta = hist(io->hist_shape, i, 10);
    fa.out_theta2 = (i == N) ? io->pose_hat : nullptr; fa.out_beta2 = (i == N) ? io->shape_hat : nullptr;
    float* hm = hist(io->hist_markers, i, 36);
    float* ho = hist(io->hist_markers_ori, i, 108);
    float* hj = hist(io->hist_joints, i, 66);
    if ((hm == nullptr) != (ho == nullptr)) return fail(EMPOSE_EINVAL, "hist_markers and hist_markers_ori go together");
    // (the frame-per-lane kernel skips outputs nobody asked for; the general kernel always writes its scratch copies)
    rq.offset_r = io->offset_r; rq.offset_t = io->offset_t;
    rq.pos = hm ? hm : (tile ? nullptr : w.pos); rq.ori = ho ? ho : (tile ? nullptr : w.ori);
    rq.joints = (i == N) ? io->joints_hat : (hj ? hj : (tile ? nullptr : w.joints));
    rq.joints2 = (i == N) ? hj : nullptr;
    rq.ld_tgt = dx; rq.frame_scale = w.scale; rq.tgt_t = w.x_t;
    const GradOut go{r.x_col(76), dx, r.x_col(142), dx, hist(io->trace_g_pose, i, 66), hist(io->trace_g_shape, i, 10)};
    if (i < N && m->use_gradient) { rq.tgt = w.x; rq.grad = &go; }
    TRY(run_smpl_eval(m, T, r.F, w.smpl, r.path.with(rq), rq, r.stream));
    if (i == N) break;
    const MlpRun upd{{&m->pose_iter, &m->shape_iter}, 2, {w.d_pose, w.d_shape}, {66, 10}, w.x, dx, T, false};
    TRY(run_mlps(upd, w.upd, m->hidden_max, r.stream));
  }
  prof_end_forward(r.stream);
  return EMPOSE_OK;
}

// empose_smpl_sensors_vjp: the SMPL workspace, then the scratch sensor outputs of the general kernel.
size_t smpl_vjp_bytes(const empose_model* m, int T) {
  return empose_smpl_workspace_bytes(m, T) + (size_t)T * (36 + 108 + 66) * sizeof(float) + 1024;
}

}  // namespace

namespace empose {
namespace api {

int smpl_sensors_eval(const empose_model* m, int T, int F, const float* theta, int ld_theta, const float* beta, int ld_beta,
                      const float* offset_r, const float* offset_t, const float* tgt, int ld_tgt, const float* frame_scale,
                      float* pos, float* ori, float* joints, float* g_theta, int ld_g, float* g_beta, int ld_gb,
                      void* workspace, hipStream_t stream) {
  Carver c(workspace);
  const SmplWs ws = carve_smpl(c, m, T);
  const GradOut go{g_theta, ld_g, g_beta, ld_gb, nullptr, nullptr};
  SmplEval rq;
  rq.update = plain_feat_args(theta, ld_theta, beta, ld_beta);
  rq.offset_r = offset_r; rq.offset_t = offset_t;
  rq.pos = pos; rq.ori = ori; rq.joints = joints;
  rq.tgt = tgt; rq.ld_tgt = ld_tgt; rq.frame_scale = frame_scale;
  if (tgt) rq.grad = &go;
  const SmplPlan plan = plan_smpl(m, T, rq);
  if (tgt && plan.tile) {
    HIP_CHECK(launch_rows_to_tile(tgt, ld_tgt, 12 * m->n_markers, ws.tgt_t, T, stream), "tile transpose");
    rq.tgt_t = ws.tgt_t;
  }
  return run_smpl_eval(m, T, F, ws, plan, rq, stream);
}

}  // namespace api
}  // namespace empose

extern "C" {

void empose_model_destroy(empose_model_t* model) {
  if (!model) return;
  for (void* p : model->allocs) (void)hipFree(p);
  delete model;
}

int empose_model_create(const empose_model_desc* d, empose_model_t** out) {
  if (!d || !out) return fail(EMPOSE_EINVAL, "null argument");
  *out = nullptr;
  const empose_smpl_desc& s = d->smpl;
  if (s.n_sensors != EMPOSE_N_SENSORS) return fail(EMPOSE_EINVAL, "n_sensors must be 12");
  if (s.nv <= 0 || s.ncp % 4 != 0 || s.j_off < s.nv * 3 || s.j_off + 66 > s.ncp || s.kb <= 0 || s.max_deg <= 0)
    return fail(EMPOSE_EINVAL, "inconsistent SMPL table sizes");
  if (d->n_markers != 6 && d->n_markers != 12) return fail(EMPOSE_EINVAL, "n_markers must be 6 or 12");
  if (d->n_iterations < 0) return fail(EMPOSE_EINVAL, "n_iterations < 0");
  if (s.rodrigues != EMPOSE_RODRIGUES_SMPLX && s.rodrigues != EMPOSE_RODRIGUES_SO3)
    return fail(EMPOSE_EINVAL, "unknown Rodrigues convention %d", s.rodrigues);
  empose_model* m = new empose_model();
  m->rod_conv = s.rodrigues;
  auto bail = [&](int rc) { empose_model_destroy(m); return rc; };
#define MTRY(expr) do { int rc_ = (expr); if (rc_ != EMPOSE_OK) return bail(rc_); } while (0)
  SmplTables& t = m->tab;
  t.n_sensors = s.n_sensors; t.nv = s.nv; t.j_off = s.j_off; t.ncp = s.ncp; t.kb = s.kb; t.max_deg = s.max_deg;
  float* fp; int* ip;
  MTRY(upload(m->allocs, s.wc, (size_t)s.ncp * 200, &fp)); t.wc = fp;
  MTRY(upload(m->allocs, s.wct, (size_t)s.ncp * 200, &fp)); t.wct = fp;
  MTRY(pack_fragments_raw(m->allocs, s.wc, s.ncp, 200, &m->wc_frag));     // the same two matrices in MFMA fragment order
  MTRY(pack_fragments_raw(m->allocs, s.wct, 200, s.ncp, &m->wct_frag));
  MTRY(upload(m->allocs, s.parents, 22, &ip)); t.parents = ip;
  MTRY(upload(m->allocs, s.skin_idx, (size_t)s.nv * s.kb, &ip)); t.skin_idx = ip;
  MTRY(upload(m->allocs, s.skin_w, (size_t)s.nv * s.kb, &fp)); t.skin_w = fp;
  if (!s.bone_ptr || !s.path_ptr || !s.sub_ptr) return bail(fail(EMPOSE_EINVAL, "null CSR pointer"));
  MTRY(upload(m->allocs, s.bone_ptr, 23, &ip)); t.bone_ptr = ip;
  MTRY(upload(m->allocs, s.bone_vert, (size_t)s.bone_ptr[22], &ip)); t.bone_vert = ip;
  MTRY(upload(m->allocs, s.bone_w, (size_t)s.bone_ptr[22], &fp)); t.bone_w = fp;
  MTRY(upload(m->allocs, s.s_center, 12, &ip)); t.s_center = ip;
  MTRY(upload(m->allocs, s.s_helper, 12, &ip)); t.s_helper = ip;
  MTRY(upload(m->allocs, s.s_deg, 12, &ip)); t.s_deg = ip;
  MTRY(upload(m->allocs, s.s_faces, (size_t)12 * s.max_deg * 3, &ip)); t.s_faces = ip;
  MTRY(upload(m->allocs, s.path_ptr, 23, &ip)); t.path_ptr = ip;
  MTRY(upload(m->allocs, s.path, (size_t)s.path_ptr[22], &ip)); t.path = ip;
  MTRY(upload(m->allocs, s.sub_ptr, 23, &ip)); t.sub_ptr = ip;
  MTRY(upload(m->allocs, s.sub, (size_t)s.sub_ptr[22], &ip)); t.sub = ip;
  {
    for (int i = 0; i < 12; ++i)
      if (s.s_deg[i] < 1 || s.s_deg[i] > s.max_deg) return bail(fail(EMPOSE_EINVAL, "sensor degree out of range"));
    std::vector<uint32_t> blob;
    MTRY(build_chain_blob(s, blob, t.off, &t.n_chunks));
    uint32_t* bp;
    MTRY(upload(m->allocs, blob.data(), blob.size(), &bp));
    t.blob = bp;
  }
  {
    // frame-per-lane path: only for patches that are closed fans of at most TL_NR faces over at most TL_NBL bones
    // (closed manifold meshes; anything else keeps chain_sensors_kernel)
    TileTables tt;
    std::vector<float> wc2;
    if (s.n_sensors == 12 && build_tile_tables(s.nv, s.kb, s.max_deg, s.j_off, s.wc, s.parents, s.skin_idx, s.skin_w,
                                               s.s_center, s.s_helper, s.s_deg, s.s_faces, &tt, &wc2)) {
      std::vector<float> wc2t((size_t)200 * tt.ncp2);
      for (int r = 0; r < tt.ncp2; ++r)
        for (int k = 0; k < 200; ++k) wc2t[(size_t)k * tt.ncp2 + r] = wc2[(size_t)r * 200 + k];
      MTRY(upload(m->allocs, &tt, 1, &m->tile_tab));
      MTRY(pack_fragments_raw(m->allocs, wc2.data(), tt.ncp2, 200, &m->wc2_frag));
      MTRY(pack_fragments_raw(m->allocs, wc2t.data(), 200, tt.ncp2, &m->wc2t_frag));
      MTRY(pack_fragments_x3_raw(m->allocs, wc2.data(), tt.ncp2, 200, &m->wc2_frag3));
      MTRY(pack_fragments_x3_raw(m->allocs, wc2t.data(), 200, tt.ncp2, &m->wc2t_frag3));
      m->ncp2 = tt.ncp2; m->tile_nloc = tt.nloc; m->tile_nbl = tt.nbl; m->tile_j_off2 = tt.j_off2;
      m->tile_ok = tt.ncp2 <= 320;   // the widest tile gemm_rows_t_kernel covers
    }
  }

  m->n_markers = d->n_markers;
  for (int i = 0; i < 12; ++i) { m->marker_idx[i] = 0; m->used_slot[i] = -1; }
  for (int i = 0; i < d->n_markers; ++i) {
    const int v = d->marker_idx[i];
    if (v < 0 || v >= 12) return bail(fail(EMPOSE_EINVAL, "marker_idx out of range"));
    m->marker_idx[i] = v;
    m->used_slot[v] = i;
  }
  m->N = d->n_iterations; m->step = d->step_size; m->shape_avg = d->shape_avg; m->use_gradient = d->use_gradient;
  m->rnn_init = d->rnn_init;
  m->d_in = d->n_markers * 12;
  m->d_x = m->d_in + 76 + (d->use_gradient ? 76 : 0);

  if (d->rnn_init) {
    const empose_lstm_desc& r = d->rnn;
    if (r.num_layers > 4 || r.input_size != m->d_in) return bail(fail(EMPOSE_EINVAL, "unsupported LSTM configuration"));
    MTRY(pack_lstm(m->allocs, r, 1, r.w_ih, r.w_hh, r.b_ih, r.b_hh, &m->rnn));
    MTRY(pack_dense(m->allocs, d->pose_head, &m->pose_head));
    MTRY(pack_dense(m->allocs, d->shape_head, &m->shape_head));
    if (d->pose_head.out_dim == 66 && d->shape_head.out_dim == 10 && d->pose_head.in_dim == d->shape_head.in_dim &&
        !d->pose_head.bn_weight && !d->shape_head.bn_weight && !d->pose_head.has_prelu && !d->shape_head.has_prelu) {
      const int K = d->pose_head.in_dim;
      std::vector<float> wst((size_t)76 * K), bst(76, 0.f);
      std::memcpy(wst.data(), d->pose_head.weight, (size_t)66 * K * sizeof(float));
      std::memcpy(wst.data() + (size_t)66 * K, d->shape_head.weight, (size_t)10 * K * sizeof(float));
      for (int n = 0; n < 66; ++n) bst[n] = d->pose_head.bias ? d->pose_head.bias[n] : 0.f;
      for (int n = 0; n < 10; ++n) bst[66 + n] = d->shape_head.bias ? d->shape_head.bias[n] : 0.f;
      MTRY(pack_fragments_raw(m->allocs, wst.data(), 76, K, &m->heads_frag));
      MTRY(pack_fragments_x3_raw(m->allocs, wst.data(), 76, K, &m->heads_frag3));
      MTRY(upload(m->allocs, bst.data(), bst.size(), &m->heads_bias));
    }
    if (m->pose_head.out_dim != 66 || m->shape_head.out_dim != 10 || m->pose_head.in_dim != r.hidden_size)
      return bail(fail(EMPOSE_EINVAL, "init head dims"));
  } else if (d->pose_init.n_layers == 0 && d->n_iterations == 0) {
    // body-model-only handle: serves empose_smpl_sensors_fwd_bwd / _vjp (training path), not empose_lgd_forward
    m->smpl_only = 1;
  } else {
    MTRY(pack_mlp(m->allocs, d->pose_init, &m->pose_init, &m->hidden_max, &m->any_skip));
    MTRY(pack_mlp(m->allocs, d->shape_init, &m->shape_init, &m->hidden_max, &m->any_skip));
    if (m->pose_init.n_layers == 0 || m->pose_init.layers[0].in_dim != m->d_in)
      return bail(fail(EMPOSE_EINVAL, "init MLP dims"));
  }
  if (m->N > 0) {
    MTRY(pack_mlp(m->allocs, d->pose_iter, &m->pose_iter, &m->hidden_max, &m->any_skip));
    MTRY(pack_mlp(m->allocs, d->shape_iter, &m->shape_iter, &m->hidden_max, &m->any_skip));
    if (m->pose_iter.n_layers == 0 || m->pose_iter.layers[0].in_dim != m->d_x ||
        m->pose_iter.layers[m->pose_iter.n_layers - 1].out_dim != 66 ||
        m->shape_iter.layers[m->shape_iter.n_layers - 1].out_dim != 10)
      return bail(fail(EMPOSE_EINVAL, "update MLP dims (expected input %d)", m->d_x));
  }
  if (m->hidden_max == 0) m->hidden_max = 4;
#undef MTRY
  *out = m;
  return EMPOSE_OK;
}

int empose_smpl_tile_supported(const empose_model_t* m) { return m && m->tile_ok ? 1 : 0; }

size_t empose_smpl_workspace_bytes(const empose_model_t* m, int T) {
  return m && T > 0 ? Carver::measure([&](Carver& c) { carve_smpl(c, m, T); }) : 0;
}

size_t empose_update_workspace_bytes(const empose_model_t* m, int T) {
  return m && T > 0 ? Carver::measure([&](Carver& c) { carve_upd(c, m, T); }) : 0;
}

size_t empose_lgd_workspace_bytes(const empose_model_t* m, int B, int F) {
  return m && B > 0 && F > 0 ? Carver::measure([&](Carver& c) { carve_lgd(c, m, B, F); }) : 0;
}

int empose_lgd_forward(const empose_model_t* m, const empose_lgd_io* io, void* workspace, size_t workspace_bytes,
                       empose_stream_t stream_) {
  return empose_lgd_forward_phase(m, io, workspace, workspace_bytes, stream_, EMPOSE_LGD_PHASE_INIT | EMPOSE_LGD_PHASE_ITER);
}

int empose_lgd_forward_phase(const empose_model_t* m, const empose_lgd_io* io, void* workspace, size_t workspace_bytes,
                             empose_stream_t stream_, int phases) {
  if (!m || !io || !workspace) return fail(EMPOSE_EINVAL, "null argument");
  if (phases < 1 || phases > 3) return fail(EMPOSE_EINVAL, "phases: EMPOSE_LGD_PHASE_INIT, _ITER or both");
  if (m->smpl_only) return fail(EMPOSE_EINVAL, "this handle holds the body model only (no networks)");
  const int B = io->B, F = io->F;
  if (B <= 0 || F <= 0) return fail(EMPOSE_EINVAL, "B and F must be positive");
  if (!io->marker_pos || !io->marker_oris || !io->offset_t || !io->offset_r || !io->pose_hat || !io->shape_hat ||
      !io->joints_hat)
    return fail(EMPOSE_EINVAL, "null input/output tensor");
  if (workspace_bytes < empose_lgd_workspace_bytes(m, B, F)) return fail(EMPOSE_ENOMEM, "workspace too small");
  Carver c(workspace);
  const LgdRun r{m, io, B, F, B * F, carve_lgd(c, m, B, F), plan_smpl(m, B * F, SmplEval()), static_cast<hipStream_t>(stream_)};
  if (phases & EMPOSE_LGD_PHASE_INIT) TRY(lgd_init(r));
  if (phases & EMPOSE_LGD_PHASE_ITER) TRY(lgd_iterate(r));
  return EMPOSE_OK;
}

int empose_smpl_sensors_fwd_bwd(const empose_model_t* m, int T, int F, const float* theta, int ld_theta,
                                const float* beta, int ld_beta, const float* offset_r, const float* offset_t,
                                const float* tgt, int ld_tgt, const float* frame_scale, float* pos, float* ori,
                                float* joints, float* g_theta, int ld_g, float* g_beta, int ld_gb, void* workspace,
                                size_t workspace_bytes, empose_stream_t stream_) {
  if (!m || !theta || !beta || !offset_r || !offset_t || !pos || !ori || !joints || !workspace)
    return fail(EMPOSE_EINVAL, "null argument");
  if (T <= 0 || F <= 0 || T % F != 0) return fail(EMPOSE_EINVAL, "T must be a positive multiple of F");
  if (tgt && (!frame_scale || !g_theta || !g_beta)) return fail(EMPOSE_EINVAL, "gradient outputs missing");
  if (workspace_bytes < empose_smpl_workspace_bytes(m, T)) return fail(EMPOSE_ENOMEM, "workspace too small");
  return smpl_sensors_eval(m, T, F, theta, ld_theta, beta, ld_beta, offset_r, offset_t, tgt, ld_tgt, frame_scale, pos, ori,
                           joints, g_theta, ld_g, g_beta, ld_gb, workspace, static_cast<hipStream_t>(stream_));
}

int empose_smpl_sensors_vjp(const empose_model_t* m, int T, int F, const float* theta, int ld_theta, const float* beta,
                            int ld_beta, const float* offset_r, const float* offset_t, const float* d_pos,
                            const float* d_ori, const float* d_joints, float* g_theta, float* g_beta, void* workspace,
                            size_t workspace_bytes, empose_stream_t stream_) {
  if (!m || !theta || !beta || !offset_r || !offset_t || !d_pos || !d_ori || !g_theta || !g_beta || !workspace)
    return fail(EMPOSE_EINVAL, "null argument");
  if (T <= 0 || F <= 0 || T % F != 0) return fail(EMPOSE_EINVAL, "T must be a positive multiple of F");
  if (workspace_bytes < smpl_vjp_bytes(m, T))
    return fail(EMPOSE_ENOMEM, "workspace too small (need empose_smpl_vjp_workspace_bytes)");
  Carver c(workspace);
  const SmplWs ws = carve_smpl(c, m, T);
  float* pos = c.f((size_t)T * 36);
  float* ori = c.f((size_t)T * 108);
  float* joints = c.f((size_t)T * 66);
  const GradOut go{g_theta, 66, g_beta, 10, nullptr, nullptr};
  SmplEval rq;
  rq.update = plain_feat_args(theta, ld_theta, beta, ld_beta);
  rq.offset_r = offset_r; rq.offset_t = offset_t;
  rq.cot_pos = d_pos; rq.cot_ori = d_ori; rq.cot_joints = d_joints;
  rq.grad = &go;
  const SmplPlan plan = plan_smpl(m, T, rq);
  if (!plan.tile) { rq.pos = pos; rq.ori = ori; rq.joints = joints; }   // the general kernel always writes them: to scratch
  return run_smpl_eval(m, T, F, ws, plan, rq, static_cast<hipStream_t>(stream_));
}

size_t empose_smpl_vjp_workspace_bytes(const empose_model_t* m, int T) { return smpl_vjp_bytes(m, T); }

int empose_update_nets_fwd(const empose_model_t* m, int T, const float* x, int ldx, float* d_pose, float* d_shape,
                           void* workspace, size_t workspace_bytes, empose_stream_t stream_) {
  if (!m || !x || !d_pose || !d_shape || !workspace) return fail(EMPOSE_EINVAL, "null argument");
  if (T <= 0) return fail(EMPOSE_EINVAL, "T must be positive");
  if (m->pose_iter.n_layers == 0) return fail(EMPOSE_EINVAL, "model has no update nets");
  if (ldx < m->d_x || ldx % 4 != 0) return fail(EMPOSE_EINVAL, "ldx must be >= %d and a multiple of 4", m->d_x);
  if (workspace_bytes < empose_update_workspace_bytes(m, T)) return fail(EMPOSE_ENOMEM, "workspace too small");
  Carver c(workspace);
  const UpdWs ws = carve_upd(c, m, T);
  const MlpRun upd{{&m->pose_iter, &m->shape_iter}, 2, {d_pose, d_shape}, {66, 10}, x, ldx, T, false};
  return run_mlps(upd, ws, m->hidden_max, static_cast<hipStream_t>(stream_));
}

}  // extern "C"
