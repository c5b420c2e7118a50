// C ABI (include/empose_hip.h), LSTM: the inference dispatcher (plan_lstm, carve_lstm_of, run_lstm), packing,
// empose_rnn_*, empose_lstm_fwd, and the training forward and backward of a uni-directional stack.
#include "api_internal.h"

using namespace empose;
using namespace empose::api;

namespace {

// bf16 elements of one set of A planes: [32-row tiles][k-steps][3 pieces][512]
size_t lstm_x3_plane_elems(int B, int K) { return (size_t)((B + 31) / 32) * ((K + 15) / 16) * 3 * 512; }
bool lstm_x3_covers(const Lstm& r, int B) {
  if (options().lstm_x3 == 0 || r.dirs != 1 || r.num_layers > 4 || B < LSTM_SEQ_MIN_B) return false;
  if (r.H % 32 != 0 || r.input_size % 4 != 0) return false;
  for (int l = 0; l < r.num_layers; ++l)
    if (!r.w3_ih[l] || !r.w3_hh[l]) return false;
  return true;
}
constexpr int LSTM_MID16_MIN_B = 9;
// ... up to 64 rows with half the tile, on all 256 CUs (lstm_mid16_x3.hip)
bool lstm_mid16_tiles(const Lstm& r, int B) {
  return options().lstm_mid16 != 0 && lstm_mid16_shape_ok(B, r.H) && r.w3q_ih[0] && r.w3q_hh[0];
}
// medium batches (the batched evaluation driver's chunks): lstm_mid_x3.hip / lstm_mid16_x3.hip
bool lstm_x3_mid_covers(const Lstm& r, int B) {
  if (options().lstm_x3 == 0 || options().lstm_mid_x3 == 0 || r.dirs != 1 || r.num_layers > 4) return false;
  // from 9 rows with the 4-unit tiles of lstm_mid16_x3.hip (7.0 us per step against 7.8 - 10.7 of lstm_fewrows_kernel at 9 - 16
  // rows), from 17 with the 8-unit tiles
  const bool tiles16 = lstm_mid16_tiles(r, B);
  if (B < (tiles16 ? LSTM_MID16_MIN_B : LSTM_PERSIST_B + 1) || B >= LSTM_SEQ_MIN_B) return false;
  if (r.H % 32 != 0 || r.input_size % 4 != 0) return false;
  for (int l = 0; l < r.num_layers; ++l)
    if (!r.w3m_ih[l] || !r.w3m_hh[l]) return false;
  return true;
}
// medium batches, whole sequence in one launch: lstm_midseq_x3.hip (needs the 8-unit-block weight order too)
constexpr int LSTM_MIDSEQ_MIN_B = 4, LSTM_MIDSEQ_MAX_B = 64;   // (up to 3 rows: lstm_persist_kernel)
bool lstm_x3_midseq_covers(const Lstm& r, int B) {
  if (options().lstm_x3 == 0 || options().lstm_mid_x3 == 0 || options().lstm_midseq == 0 || r.dirs != 1) return false;
  if (B < LSTM_MIDSEQ_MIN_B || B > LSTM_MIDSEQ_MAX_B || r.num_layers > 4 || r.input_size % 4 != 0) return false;
  int ks_in[4];
  for (int l = 0; l < r.num_layers; ++l) {
    if (!r.w3m_ih[l] || !r.w3m_hh[l]) return false;
    ks_in[l] = l == 0 ? (r.input_size + 15) / 16 : r.H / 16;
  }
  return lstm_midseq_shape_ok(B, r.H, r.num_layers, ks_in);
}

LstmPlan plan_lstm(const Lstm& r, int B) {
  LstmPlan p;
  // the whole-sequence kernels get their buffers by shape alone (their launches check the options)
  p.persist = r.dirs == 1 && B <= LSTM_PERSIST_B;
  p.seq = r.dirs == 1 && B >= LSTM_SEQ_MIN_B && r.num_layers <= 4;
  p.midseq = lstm_x3_midseq_covers(r, B);
  // the steps: large batches on lstm_x3.hip (or lstm_rows_x3.hip), medium ones on lstm_mid16_x3.hip / lstm_mid_x3.hip
  if (lstm_x3_covers(r, B)) p.step = options().lstm_x3 == 2 ? LstmStep::rows_x3 : LstmStep::chain_x3;
  else if (lstm_x3_mid_covers(r, B)) p.step = lstm_mid16_tiles(r, B) ? LstmStep::mid16_x3 : LstmStep::mid_x3;
  p.x3 = p.step != LstmStep::wave || p.midseq;
  return p;
}

void fill_unit(LstmUnitArgs& ua, const Lstm& r, const LstmWs& ws, int u) {
  ua.w_ih = r.w_ih[u]; ua.w_hh = r.w_hh[u]; ua.bias = r.bias[u];
  ua.h[0] = ws.h[u][0]; ua.h[1] = ws.h[u][1]; ua.c = ws.c[u];
  ua.in_seq = nullptr; ua.in_ld = 0; ua.in_from = -1; ua.t_offset = 0; ua.reverse = 0;
  ua.y = nullptr; ua.y_ld = 0; ua.y_col = 0;
}

// An LSTM weight matrix [4H][K] (gate-major rows) as three bf16 pieces per weight in the fragment order of lstm_x3.hip:
// [k-step of 16][32-unit block][gate][piece] -> one wave fragment of 512 bf16, lane (n = lane & 31, half = lane >> 5) owns
// W[gate * H + block * 32 + n][ks * 16 + half * 8 .. + 7]; k past K is zero.
// `mid`: the order of lstm_mid_x3.hip instead -- [k-step of 16][8-unit block][piece] -> one fragment whose column
// n = lane & 31 is gate n >> 3 of unit block * 8 + (n & 7).
int pack_lstm_x3(std::vector<void*>& allocs, const float* w, int H, int K, unsigned short** out, bool mid = false) {
  const int KS = (K + 15) / 16, JB = mid ? H / 8 : H / 32, NQ = mid ? 1 : 4;
  return upload_bf16(allocs, pack_fragments_x3((size_t)KS * JB * NQ, K, [&](size_t f, int lane, const float** row, int* k0) {
    const int q = (int)(f % NQ), jb = (int)(f / NQ % JB), ks = (int)(f / NQ / JB), n = lane & 31;
    *row = mid ? w + (size_t)((n >> 3) * H + jb * 8 + (n & 7)) * K : w + (size_t)(q * H + jb * 32 + n) * K;
    *k0 = ks * 16 + (lane >> 5) * 8;
    return true;
  }), out);
}

// ... and in the order of lstm_mid16_x3.hip: [k-step of 32][4-unit block][piece] -> one fragment of the 16x16x32 instruction,
// lane (n = lane & 15, q = lane >> 4) owns W[gate (n >> 2) * H + block * 4 + (n & 3)][ks * 32 + q * 8 .. + 7]; k past K is zero.
int pack_lstm_x3_mid16(std::vector<void*>& allocs, const float* w, int H, int K, unsigned short** out) {
  const int K2 = (K + 31) / 32, JB = H / 4;
  return upload_bf16(allocs, pack_fragments_x3((size_t)K2 * JB, K, [&](size_t f, int lane, const float** row, int* k0) {
    const int jb = (int)(f % JB), ks = (int)(f / JB), n = lane & 15;
    *row = w + (size_t)((n >> 2) * H + jb * 4 + (n & 3)) * K;
    *k0 = ks * 32 + (lane >> 4) * 8;
    return true;
  }), out);
}

struct TrainLstmWs {
  LstmWs st;               // h[l][2], c[l]
  float* bias[4];          // b_ih + b_hh
  float* dgates;           // [B*F][4H]
  float* dyl;              // [B*F][H] cotangent of the layer below's output
  float* dh[2]; float* carry; float* dc;   // [B][H]
  float* wt;               // transposed weights, max(H, in) x 4H
  float* atb;              // A^T B partials
  size_t atb_floats;
  float* ksplit;           // partial tiles of the K-split recurrent product, or nullptr
  size_t ksplit_floats;
  // the reverse recurrences of two layers as a wavefront (bptt_wave): the upper layer's pre-activation gradients, cell
  // state cotangent and carry next to the lower layer's, three transposed weight matrices at once
  int wave = 0;            // 0 no, 1 matrix-vector kernel, 2 K-split tiles
  float* dgates_up; float* carry_up; float* dc_up;
  float* wt_hh_up; float* wt_ih_up;
  float* rec;              // partial tiles of both problems of a wavefront step (K-split form)
};
int check_lstm_params(const empose_lstm_params* p) {
  if (!p) return fail(EMPOSE_EINVAL, "null argument");
  if (p->num_layers < 1 || p->num_layers > 4 || p->hidden_size % 4 != 0 || p->input_size % 4 != 0 ||
      p->hidden_size <= 0 || p->input_size <= 0)
    return fail(EMPOSE_EINVAL, "unsupported LSTM configuration");
  for (int l = 0; l < p->num_layers; ++l)
    if (!p->w_ih[l] || !p->w_hh[l] || !p->b_ih[l] || !p->b_hh[l]) return fail(EMPOSE_EINVAL, "null LSTM parameter");
  return EMPOSE_OK;
}
Lstm lstm_view(const empose_lstm_params* p) {   // device pointers as they are: nothing is uploaded
  Lstm r;
  r.num_layers = p->num_layers; r.input_size = p->input_size; r.H = p->hidden_size; r.dirs = 1;
  return r;
}
TrainLstmWs carve_train_lstm(Carver& c, const empose_lstm_params* p, int B, int F) {
  TrainLstmWs w;
  const int H = p->hidden_size, L = p->num_layers;
  const int in_max = p->input_size > H ? p->input_size : H;
  Lstm r = lstm_view(p);
  w.st = carve_lstm_of(c, r, B, F);   // B > LSTM_PERSIST_B or not, the exchange buffer is unused here
  for (int l = 0; l < 4; ++l) w.bias[l] = l < L ? c.f((size_t)4 * H) : nullptr;
  w.dgates = c.f((size_t)B * F * 4 * H);
  w.dyl = c.f((size_t)B * F * H);
  w.dh[0] = c.f((size_t)B * H); w.dh[1] = c.f((size_t)B * H); w.carry = c.f((size_t)B * H); w.dc = c.f((size_t)B * H);
  w.wt = c.f((size_t)in_max * 4 * H);
  w.atb_floats = atb_workspace_floats_max(B * F, {{4 * H, p->input_size}, {4 * H, H}});   // dW_ih (layer 0 / above), dW_hh
  w.atb = c.f(w.atb_floats + 64);
  w.ksplit_floats = gemm_ksplit_applicable(B, H, 4 * H) ? gemm_ksplit_workspace_floats(B, H, 4 * H) : 0;
  w.ksplit = w.ksplit_floats ? c.f(w.ksplit_floats) : nullptr;
  w.wave = 0;
  w.dgates_up = w.carry_up = w.dc_up = w.wt_hh_up = w.wt_ih_up = w.rec = nullptr;
  if (L == 2 && options().bptt_wave != 0 && (4 * H) % 256 == 0) {
    if (gemm_fewrows_applicable(B, H, 4 * H) && 4 * H <= 2048) w.wave = 1;
    else if (w.ksplit_floats && 8 * H / 256 <= 16) w.wave = 2;   // (not the pointer: null while sizes are counted)
  }
  if (w.wave) {
    w.dgates_up = c.f((size_t)B * F * 4 * H);
    w.carry_up = c.f((size_t)B * H); w.dc_up = c.f((size_t)B * H);
    w.wt_hh_up = c.f((size_t)H * 4 * H); w.wt_ih_up = c.f((size_t)H * 4 * H);
    if (w.wave == 2) w.rec = c.f(rec_ksplit_workspace_floats(B, H, 8 * H, 2));
  }
  return w;
}
}  // namespace

namespace empose {
namespace api {

LstmWs carve_lstm_of(Carver& c, const Lstm& r, int B, int F) {
  LstmWs w;
  const LstmPlan& p = w.plan = plan_lstm(r, B);
  const int H = r.H, U = r.num_layers * r.dirs;
  for (int u = 0; u < 8; ++u) {
    const bool used = u < U;
    w.h[u][0] = used ? c.f((size_t)B * H) : nullptr;
    w.h[u][1] = used ? c.f((size_t)B * H) : nullptr;
    w.c[u] = used ? c.f((size_t)B * H) : nullptr;
  }
  const bool need_y = r.dirs == 2 && r.num_layers > 1;
  w.yb[0] = need_y ? c.f((size_t)B * F * 2 * H) : nullptr;
  w.yb[1] = (need_y && r.num_layers > 2) ? c.f((size_t)B * F * 2 * H) : nullptr;
  w.xch = p.persist ? c.f(lstm_persist_xch_floats(r.num_layers, B, H)) : nullptr;
  for (int u = 0; u < 8; ++u) w.h3[u] = (p.seq && u < U) ? c.f((size_t)B * H) : nullptr;
  w.seq_cnt = p.seq ? reinterpret_cast<unsigned*>(c.f(lstm_seq_counter_uints(B))) : nullptr;
  w.x3_t_stride = lstm_x3_plane_elems(B, r.input_size);
  w.x3 = p.x3 ? reinterpret_cast<unsigned short*>(c.f((w.x3_t_stride * F + 1) / 2)) : nullptr;
  for (int u = 0; u < 8; ++u)
    for (int k = 0; k < 2; ++k)
      w.a3[u][k] = (p.x3 && u < U) ? reinterpret_cast<unsigned short*>(c.f((lstm_x3_plane_elems(B, H) + 1) / 2)) : nullptr;
  for (int u = 0; u < 8; ++u)
    w.xa[u] = (p.midseq && u < U) ? reinterpret_cast<unsigned short*>(c.f((lstm_x3_plane_elems(B, H) * (size_t)(F + 1) + 1) / 2))
                                : nullptr;
  w.midseq_flags = p.midseq ? reinterpret_cast<unsigned*>(c.f(lstm_midseq_flag_uints(U, H))) : nullptr;
  return w;
}

// State layout of h0/c0/h_n/c_n: [num_layers * dirs][B][H], unit u = layer * dirs + direction (PyTorch's order).
int run_lstm(const Lstm& r, int B, int F, const float* x, int ldx, const int* seq_lengths, const float* h0,
             const float* c0, float* y, float* h_n, float* c_n, const LstmWs& ws, hipStream_t stream) {
  const int H = r.H, L = r.num_layers, D = r.dirs, U = L * D;
  const size_t bh = (size_t)B * H;
  // a poll of a cooperative kernel of an EARLIER call gave up: everything that call (and what was fed from it) produced
  // is NaN.  Reported once, here, without synchronising (the counter is a host-mapped word).
  // STICKY: the count is only looked at here; it stays set -- and every recurrence of the process keeps failing, whichever
  // model, stream or thread it belongs to -- until empose_async_status() has reported and cleared it.  (Clearing it here
  // let the one call that happened to come next swallow the report while the call that produced the NaNs returned OK.)
  TRY(earlier_poll_timeouts());
  // the wavefront kernel addresses its operands with 32-bit byte offsets from a per-segment base
  if ((size_t)B * F * (size_t)(ldx > 2 * H ? ldx : 2 * H) * sizeof(float) >= ((size_t)1 << 32))
    return fail(EMPOSE_EINVAL, "LSTM batch of %d x %d frames is too large for one call; split the batch", B, F);
  prof_mark(P_COPY, stream);
  if (!h0 && !c0) {
    // new sequences: the state buffers of all units are carved back to back (carve_lstm_of) -- one fill instead of 2 U
    const char* lo = reinterpret_cast<const char*>(ws.h[0][0]);
    const char* hi = reinterpret_cast<const char*>(ws.c[U - 1] + bh);
    HIP_TRY(hipMemsetAsync(ws.h[0][0], 0, (size_t)(hi - lo), stream));
  } else {
    for (int u = 0; u < U; ++u) {
      if (h0) HIP_TRY(hipMemcpyAsync(ws.h[u][0], h0 + u * bh, bh * sizeof(float), hipMemcpyDeviceToDevice, stream));
      else HIP_TRY(hipMemsetAsync(ws.h[u][0], 0, bh * sizeof(float), stream));
      if (c0) HIP_TRY(hipMemcpyAsync(ws.c[u], c0 + u * bh, bh * sizeof(float), hipMemcpyDeviceToDevice, stream));
      else HIP_TRY(hipMemsetAsync(ws.c[u], 0, bh * sizeof(float), stream));
    }
  }
  LstmWaveArgs a;
  a.seq_lengths = seq_lengths; a.B = B; a.F = F; a.H = H;
  bool seq_done = false;
  bool state_direct = false;   // the step kernel has stored h_n / c_n itself
  if (D == 1) {
    // Stacked uni-directional layers: wavefront over (layer, time), launch s advances layer l by its step s - l.
    if (L > 4) return fail(EMPOSE_EINVAL, "at most 4 stacked layers per wavefront");
    a.n_units = L;
    for (int l = 0; l < L; ++l) {
      LstmUnitArgs& ua = a.unit[l];
      fill_unit(ua, r, ws, l);
      ua.in_k = (l == 0) ? r.input_size : H;
      if (l == 0) { ua.in_seq = x; ua.in_ld = ldx; }
      else ua.in_from = l - 1;
      ua.t_offset = l;
      if (l == L - 1) { ua.y = y; ua.y_ld = H; }
    }
    // The plan (plan_lstm) names the kernels this batch may use; the cooperative launches below report done = false when
    // their workgroups cannot all be resident, and the step launches take over.
    const LstmPlan& p = ws.plan;
    // Small batches: the whole sequence in one cooperative launch (weights in registers, grid barrier per step).
    bool done = false;
    if (p.persist && F >= 4 && options().lstm_persist != 0) {
      prof_mark(P_LSTM_STEP, stream);
      a.s = 0;
      HIP_CHECK(launch_lstm_persist(a, ws.xch, stream, &done), "lstm sequence kernel");
    }
    // Large batches: the whole sequence in one cooperative launch too (lstm_seq_kernel; the workgroups of a row group
    // synchronise through counters); falls back to the step launches when its workgroups cannot all be resident.
    if (!done && p.seq && F >= 4 && options().lstm_seq != 0) {
      prof_mark(P_LSTM_STEP, stream);
      a.s = 0;
      HIP_CHECK(launch_lstm_seq(a, ws.h3, ws.seq_cnt, stream, &done), "lstm sequence kernel (large batch)");
      seq_done = done;
    }
    // Medium batches, inference: the whole sequence in one cooperative launch on three bf16 pieces per operand, weights in
    // registers (lstm_midseq_x3.hip); falls back to the step launches below when it cannot be launched here.
    if (!done && p.midseq && F >= 4) {
      prof_mark(P_COPY, stream);
      const int KS_in = (r.input_size + 15) / 16, KS_h = H / 16;
      hipError_t e = launch_lstm_split_rows(x, (long)F * ldx, ldx, F, B, r.input_size, KS_in, ws.x3, (long)ws.x3_t_stride, stream);
      for (int l = 0; l < L && e == hipSuccess; ++l)
        e = launch_lstm_split_rows(ws.h[l][0], H, 0, 1, B, H, KS_h, ws.xa[l], 0, stream);
      if (e != hipSuccess) return fail(EMPOSE_EHIP, "lstm operand split: %s", hipGetErrorString(e));
      LstmMidSeqArgs qa;
      qa.n_units = L; qa.seq_lengths = seq_lengths; qa.B = B; qa.F = F; qa.H = H; qa.flags = ws.midseq_flags;
      for (int l = 0; l < 4; ++l) {
        const int ll = l < L ? l : 0;
        LstmMidSeqUnit& qu = qa.unit[l];
        qu.w3_ih = r.w3m_ih[ll]; qu.w3_hh = r.w3m_hh[ll]; qu.bias = r.bias[ll];
        qu.in3 = ws.x3; qu.in_t_stride = ws.x3_t_stride; qu.ks_in = ll == 0 ? KS_in : KS_h;
        qu.xa = ws.xa[ll]; qu.h0 = ws.h[ll][0]; qu.h_last = ws.h[ll][F & 1]; qu.c = ws.c[ll];
        qu.y = ll == L - 1 ? y : nullptr; qu.y_ld = H; qu.y_col = 0;
      }
      prof_mark(P_LSTM_STEP, stream);
      HIP_CHECK(launch_lstm_midseq_x3(qa, stream, &done), "lstm sequence kernel (medium batch)");
    }
    // Inference: the steps on the bf16 matrix path with three bf16 pieces per operand -- large batches on lstm_x3.hip
    // (or lstm_rows_x3.hip), medium ones on lstm_mid16_x3.hip (4-unit tiles) or lstm_mid_x3.hip (8-unit tiles)
    if (!done && p.step != LstmStep::wave) {
      const bool mid16 = p.step == LstmStep::mid16_x3, mid8 = p.step == LstmStep::mid_x3;
      prof_mark(P_COPY, stream);
      const int KS_in = (r.input_size + 15) / 16, KS_h = H / 16;
      hipError_t e = launch_lstm_split_rows(x, (long)F * ldx, ldx, F, B, r.input_size, KS_in, ws.x3, (long)ws.x3_t_stride, stream);
      // New sequences (option lstm_state_direct): the pieces of a zero state are zero planes, and the 2 L hidden-state
      // planes are carved back to back (carve_lstm_of) -- one fill instead of a split launch and a fill per layer.  On
      // the chain kernel the last step of each layer then stores h_n / c_n itself (rows past their length included: it
      // rewrites their frozen state at every step), so the 2 L trailing copies go too.
      const bool direct = options().lstm_state_direct != 0 && !h0 && !c0;
      state_direct = direct && p.step == LstmStep::chain_x3;
      const size_t plane_bytes = lstm_x3_plane_elems(B, H) * sizeof(unsigned short);
      if (direct) {
        // (checked, not assumed: the fill below covers [a3[0][0], a3[L-1][1] + plane) and must hit these planes only)
        const char* lo = reinterpret_cast<const char*>(ws.a3[0][0]);
        const size_t stride = align_up((lstm_x3_plane_elems(B, H) + 1) / 2 * sizeof(float));
        for (int l = 0; l < L; ++l)
          for (int k = 0; k < 2; ++k)
            if (reinterpret_cast<const char*>(ws.a3[l][k]) != lo + (size_t)(2 * l + k) * stride)
              return fail(EMPOSE_EINVAL, "internal: the LSTM hidden-state planes are not carved back to back");
        const size_t span = (size_t)(2 * L - 1) * stride + plane_bytes;
        if (e == hipSuccess) e = hipMemsetAsync(ws.a3[0][0], 0, span, stream);
      } else {
        for (int l = 0; l < L && e == hipSuccess; ++l) {
          e = launch_lstm_split_rows(ws.h[l][0], H, 0, 1, B, H, KS_h, ws.a3[l][0], 0, stream);
          if (e == hipSuccess) e = hipMemsetAsync(ws.a3[l][1], 0, plane_bytes, stream);
        }
      }
      if (e != hipSuccess) return fail(EMPOSE_EHIP, "lstm operand split: %s", hipGetErrorString(e));
      const int tiles = (H / 32) * ((B + 63) / 64);
      for (int s = 0; s < F + L - 1; ++s) {
        LstmX3Args xa;
        xa.n_units = 0; xa.seq_lengths = seq_lengths; xa.B = B; xa.F = F; xa.H = H;
        for (int l = 0; l < L; ++l) {
          const int t = s - l;
          if (t < 0 || t >= F) continue;
          LstmX3Unit& xu = xa.unit[xa.n_units++];
          xu.w3_ih = mid16 ? r.w3q_ih[l] : mid8 ? r.w3m_ih[l] : r.w3_ih[l];
          xu.w3_hh = mid16 ? r.w3q_hh[l] : mid8 ? r.w3m_hh[l] : r.w3_hh[l]; xu.bias = r.bias[l];
          xu.a3_in = l == 0 ? ws.x3 + (size_t)t * ws.x3_t_stride : ws.a3[l - 1][(t + 1) & 1];
          xu.ks_in = l == 0 ? KS_in : KS_h;
          xu.a3_rec = ws.a3[l][t & 1]; xu.a3_out = ws.a3[l][(t + 1) & 1];
          xu.h_prev = ws.h[l][t & 1]; xu.h_next = ws.h[l][(t + 1) & 1]; xu.c = ws.c[l];
          xu.y = l == L - 1 ? y : nullptr; xu.y_ld = H; xu.y_col = 0; xu.t = t;
          const bool last_step = state_direct && t == F - 1;
          xu.h_final = last_step && h_n ? h_n + l * bh : nullptr;
          xu.c_final = last_step && c_n ? c_n + l * bh : nullptr;
        }
        xa.units_per_block = tiles >= 192 ? xa.n_units : 1;
        prof_mark(P_LSTM_STEP, stream);
        HIP_CHECK(mid16 ? launch_lstm_mid16_x3(xa, stream) : mid8 ? launch_lstm_mid_x3(xa, stream)
                  : p.step == LstmStep::rows_x3 ? launch_lstm_rows_x3(xa, stream) : launch_lstm_chain_x3(xa, stream),
                  "lstm step (bf16 pieces)");
      }
      done = true;
    }
    for (int s = 0; !done && s < F + L - 1; ++s) {
      a.s = s;
      prof_mark(P_LSTM_STEP, stream);
      HIP_CHECK(launch_lstm_wave(a, stream), "lstm step");
    }
  } else {
    // Bidirectional: a layer needs the whole output sequence of the layer below, so layers run one after the other;
    // the two directions of a layer share each launch.
    if (!seq_lengths) return fail(EMPOSE_EINVAL, "bidirectional LSTM needs seq_lengths");
    a.n_units = 2;
    for (int l = 0; l < L; ++l) {
      const float* in = (l == 0) ? x : ws.yb[(l - 1) & 1];
      const int in_ld = (l == 0) ? ldx : 2 * H;
      float* out = (l == L - 1) ? y : ws.yb[l & 1];
      for (int d = 0; d < 2; ++d) {
        LstmUnitArgs& ua = a.unit[d];
        fill_unit(ua, r, ws, l * 2 + d);
        ua.in_k = (l == 0) ? r.input_size : 2 * H;
        ua.in_seq = in; ua.in_ld = in_ld; ua.reverse = d;
        ua.y = out; ua.y_ld = 2 * H; ua.y_col = d * H;
      }
      for (int s = 0; s < F; ++s) {
        a.s = s;
        prof_mark(P_LSTM_STEP, stream);
        HIP_CHECK(launch_lstm_wave(a, stream), "lstm step");
      }
    }
  }
  if (state_direct) return EMPOSE_OK;
  prof_mark(P_COPY, stream);
  for (int u = 0; u < U; ++u) {
    // the final hidden state: buffer F & 1 after step launches, F % 3 of (h[0], h[1], h3) after the large-batch sequence kernel
    const float* h_last = seq_done ? (F % 3 == 2 ? ws.h3[u] : ws.h[u][F % 3]) : ws.h[u][F & 1];
    if (h_n) HIP_TRY(hipMemcpyAsync(h_n + u * bh, h_last, bh * sizeof(float), hipMemcpyDeviceToDevice, stream));
    if (c_n) HIP_TRY(hipMemcpyAsync(c_n + u * bh, ws.c[u], bh * sizeof(float), hipMemcpyDeviceToDevice, stream));
  }
  return EMPOSE_OK;
}

int pack_lstm(std::vector<void*>& allocs, const empose_lstm_desc& r, int dirs, const float* const* w_ih,
              const float* const* w_hh, const float* const* b_ih, const float* const* b_hh, Lstm* out) {
  if (r.num_layers < 1 || r.num_layers * dirs > 8 || r.hidden_size % 4 != 0 || r.input_size % 4 != 0)
    return fail(EMPOSE_EINVAL, "unsupported LSTM configuration");
  out->num_layers = r.num_layers; out->input_size = r.input_size; out->H = r.hidden_size; out->dirs = dirs;
  for (int l = 0; l < r.num_layers; ++l)
    for (int d = 0; d < dirs; ++d) {
      const int u = l * dirs + d;
      const int k_in = l == 0 ? r.input_size : r.hidden_size * dirs;
      if (!w_ih[u] || !w_hh[u] || !b_ih[u] || !b_hh[u]) return fail(EMPOSE_EINVAL, "null LSTM parameter");
      TRY(upload(allocs, w_ih[u], (size_t)4 * r.hidden_size * k_in, &out->w_ih[u]));
      TRY(upload(allocs, w_hh[u], (size_t)4 * r.hidden_size * r.hidden_size, &out->w_hh[u]));
      std::vector<float> bias(4 * r.hidden_size);
      for (int i = 0; i < 4 * r.hidden_size; ++i) bias[i] = b_ih[u][i] + b_hh[u][i];
      TRY(upload(allocs, bias.data(), bias.size(), &out->bias[u]));
      if (dirs == 1 && r.hidden_size % 32 == 0) {
        TRY(pack_lstm_x3(allocs, w_ih[u], r.hidden_size, k_in, &out->w3_ih[u]));
        TRY(pack_lstm_x3(allocs, w_hh[u], r.hidden_size, r.hidden_size, &out->w3_hh[u]));
        TRY(pack_lstm_x3(allocs, w_ih[u], r.hidden_size, k_in, &out->w3m_ih[u], true));
        TRY(pack_lstm_x3(allocs, w_hh[u], r.hidden_size, r.hidden_size, &out->w3m_hh[u], true));
        TRY(pack_lstm_x3_mid16(allocs, w_ih[u], r.hidden_size, k_in, &out->w3q_ih[u]));
        TRY(pack_lstm_x3_mid16(allocs, w_hh[u], r.hidden_size, r.hidden_size, &out->w3q_hh[u]));
      }
    }
  return EMPOSE_OK;
}

}  // namespace api
}  // namespace empose

extern "C" {

size_t empose_lstm_workspace_bytes(const empose_model_t* m, int B, int F) {
  Carver c(nullptr);
  carve_lstm_of(c, m->rnn, B, F);
  return c.off;
}

int empose_lstm_fwd(const empose_model_t* m, int B, int F, const float* x, int ldx, const int* seq_lengths,
                    const float* h0, const float* c0, float* y, float* h_n, float* c_n, void* workspace,
                    size_t workspace_bytes, empose_stream_t stream_) {
  if (!m || !x || !y || !workspace) return fail(EMPOSE_EINVAL, "null argument");
  if (!m->rnn_init) return fail(EMPOSE_EINVAL, "model has no LSTM");
  if (ldx % 4 != 0) return fail(EMPOSE_EINVAL, "ldx must be a multiple of 4");
  if (workspace_bytes < empose_lstm_workspace_bytes(m, B, F)) return fail(EMPOSE_ENOMEM, "workspace too small");
  Carver c(workspace);
  LstmWs ws = carve_lstm_of(c, m->rnn, B, F);
  return run_lstm(m->rnn, B, F, x, ldx, seq_lengths, h0, c0, y, h_n, c_n, ws, static_cast<hipStream_t>(stream_));
}

void empose_rnn_destroy(empose_rnn_t* rnn) {
  if (!rnn) return;
  for (void* p : rnn->allocs) (void)hipFree(p);
  delete rnn;
}

int empose_rnn_create(const empose_rnn_desc* d, empose_rnn_t** out) {
  if (!d || !out) return fail(EMPOSE_EINVAL, "null argument");
  *out = nullptr;
  empose_rnn* r = new empose_rnn();
  empose_lstm_desc base;
  base.num_layers = d->num_layers; base.input_size = d->input_size; base.hidden_size = d->hidden_size;
  const int rc = pack_lstm(r->allocs, base, d->bidirectional ? 2 : 1, d->w_ih, d->w_hh, d->b_ih, d->b_hh, &r->rnn);
  if (rc != EMPOSE_OK) { empose_rnn_destroy(r); return rc; }
  if (!d->bidirectional && d->num_layers > 4) { empose_rnn_destroy(r); return fail(EMPOSE_EINVAL, "at most 4 stacked layers"); }
  *out = r;
  return EMPOSE_OK;
}

size_t empose_rnn_workspace_bytes(const empose_rnn_t* rnn, int B, int F) {
  if (!rnn || B <= 0 || F <= 0) return 0;
  Carver c(nullptr);
  carve_lstm_of(c, rnn->rnn, B, F);
  return c.off;
}

int empose_rnn_fwd(const empose_rnn_t* rnn, int B, int F, const float* x, int ldx, const int* seq_lengths,
                   const float* h0, const float* c0, float* y, float* h_n, float* c_n, void* workspace,
                   size_t workspace_bytes, empose_stream_t stream_) {
  if (!rnn || !x || !y || !workspace) return fail(EMPOSE_EINVAL, "null argument");
  if (B <= 0 || F <= 0) return fail(EMPOSE_EINVAL, "B and F must be positive");
  if (ldx % 4 != 0 || ldx < rnn->rnn.input_size) return fail(EMPOSE_EINVAL, "ldx must be a multiple of 4 and >= input_size");
  if (workspace_bytes < empose_rnn_workspace_bytes(rnn, B, F)) return fail(EMPOSE_ENOMEM, "workspace too small");
  Carver c(workspace);
  LstmWs ws = carve_lstm_of(c, rnn->rnn, B, F);
  return run_lstm(rnn->rnn, B, F, x, ldx, seq_lengths, h0, c0, y, h_n, c_n, ws, static_cast<hipStream_t>(stream_));
}

size_t empose_lstm_train_save_floats(int L, int B, int F, int H) {
  return (size_t)L * B * F * 7 * H;
}

size_t empose_lstm_train_workspace_bytes(const empose_lstm_params* p, int B, int F) {
  if (!p || B <= 0 || F <= 0) return 0;
  Carver c(nullptr);
  carve_train_lstm(c, p, B, F);
  return c.off;
}

int empose_lstm_train_fwd(const empose_lstm_params* p, int B, int F, const float* x, int ldx, const int* seq_lengths,
                          const float* h0, const float* c0, float* y, float* h_n, float* c_n, float* save,
                          void* workspace, size_t workspace_bytes, empose_stream_t stream_) {
  TRY(check_lstm_params(p));
  TRY(earlier_poll_timeouts());
  if (!x || !y || !save || !workspace) return fail(EMPOSE_EINVAL, "null argument");
  if (B <= 0 || F <= 0 || ldx < p->input_size || ldx % 4 != 0) return fail(EMPOSE_EINVAL, "bad sizes");
  if (workspace_bytes < empose_lstm_train_workspace_bytes(p, B, F)) return fail(EMPOSE_ENOMEM, "workspace too small");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const int H = p->hidden_size, L = p->num_layers;
  const size_t bh = (size_t)B * H, bfh = (size_t)B * F * H;
  if ((size_t)B * F * (size_t)(ldx > 4 * H ? ldx : 4 * H) * sizeof(float) >= ((size_t)1 << 32))
    return fail(EMPOSE_EINVAL, "LSTM batch of %d x %d frames is too large for one call; split the batch", B, F);
  Carver c(workspace);
  TrainLstmWs w = carve_train_lstm(c, p, B, F);
  LstmWaveArgs a;
  a.seq_lengths = seq_lengths; a.B = B; a.F = F; a.H = H; a.n_units = L;
  for (int l = 0; l < L; ++l) {
    HIP_CHECK(launch_add2(p->b_ih[l], p->b_hh[l], w.bias[l], 4 * H, stream), "bias sum");
    float* sv = save + (size_t)l * 7 * bfh;
    LstmUnitArgs& ua = a.unit[l];
    ua.w_ih = p->w_ih[l]; ua.w_hh = p->w_hh[l]; ua.bias = w.bias[l];
    ua.h[0] = w.st.h[l][0]; ua.h[1] = w.st.h[l][1]; ua.c = w.st.c[l];
    ua.in_k = l == 0 ? p->input_size : H;
    ua.in_seq = l == 0 ? x : nullptr; ua.in_ld = l == 0 ? ldx : 0; ua.in_from = l == 0 ? -1 : l - 1;
    ua.t_offset = l; ua.reverse = 0;
    ua.y = l == L - 1 ? y : sv + 6 * bfh; ua.y_ld = H; ua.y_col = 0;
    ua.sv_gates = sv; ua.sv_c = sv + 4 * bfh; ua.sv_hprev = sv + 5 * bfh;
    if (h0) {
      HIP_TRY(hipMemcpyAsync(ua.h[0], h0 + l * bh, bh * sizeof(float), hipMemcpyDeviceToDevice, stream));
      HIP_TRY(hipMemcpy2DAsync(ua.sv_hprev, (size_t)F * H * sizeof(float), h0 + l * bh, (size_t)H * sizeof(float),
                               (size_t)H * sizeof(float), B, hipMemcpyDeviceToDevice, stream));
    } else {
      HIP_TRY(hipMemsetAsync(ua.h[0], 0, bh * sizeof(float), stream));
      HIP_TRY(hipMemset2DAsync(ua.sv_hprev, (size_t)F * H * sizeof(float), 0, (size_t)H * sizeof(float), B, stream));
    }
    if (c0) HIP_TRY(hipMemcpyAsync(ua.c, c0 + l * bh, bh * sizeof(float), hipMemcpyDeviceToDevice, stream));
    else HIP_TRY(hipMemsetAsync(ua.c, 0, bh * sizeof(float), stream));
  }
  // Small batches (the reference's training batch of 12 windows): the whole sequence in one cooperative launch with the
  // weights in registers, as in inference -- the step-by-step kernel streams 13.8 MB of weights per wavefront step.
  bool done = false;
  if (w.st.xch && F >= 4 && options().lstm_persist != 0) {
    a.s = 0;
    HIP_CHECK(launch_lstm_persist(a, w.st.xch, stream, &done), "lstm sequence kernel");
  }
  for (int s = 0; !done && s < F + L - 1; ++s) {
    a.s = s;
    HIP_CHECK(launch_lstm_wave(a, stream), "lstm step");
  }
  for (int l = 0; l < L; ++l) {
    if (h_n) HIP_TRY(hipMemcpyAsync(h_n + l * bh, w.st.h[l][F & 1], bh * sizeof(float), hipMemcpyDeviceToDevice, stream));
    if (c_n) HIP_TRY(hipMemcpyAsync(c_n + l * bh, w.st.c[l], bh * sizeof(float), hipMemcpyDeviceToDevice, stream));
  }
  return EMPOSE_OK;
}

int empose_lstm_train_bwd(const empose_lstm_params* p, int B, int F, const float* x, int ldx, const int* seq_lengths,
                          const float* c0, const float* save, const float* dy, float* dx,
                          const empose_lstm_grads* grads, void* workspace, size_t workspace_bytes,
                          empose_stream_t stream_) {
  TRY(check_lstm_params(p));
  TRY(earlier_poll_timeouts());
  if (!x || !save || !dy || !grads || !workspace) return fail(EMPOSE_EINVAL, "null argument");
  if (B <= 0 || F <= 0 || ldx < p->input_size || ldx % 4 != 0) return fail(EMPOSE_EINVAL, "bad sizes");
  if (workspace_bytes < empose_lstm_train_workspace_bytes(p, B, F)) return fail(EMPOSE_ENOMEM, "workspace too small");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const int H = p->hidden_size, L = p->num_layers;
  const size_t bh = (size_t)B * H, bfh = (size_t)B * F * H;
  for (int l = 0; l < L; ++l)
    if (!grads->w_ih[l] || !grads->w_hh[l] || !grads->b_ih[l] || !grads->b_hh[l])
      return fail(EMPOSE_EINVAL, "null gradient output");
  Carver c(workspace);
  TrainLstmWs w = carve_train_lstm(c, p, B, F);
  auto gemm = [&](const float* A, int lda, const float* W, int ldw, float* C, int ldc, int M, int N, int K,
                  const float* resid, int ldr) -> hipError_t {
    GemmBatch b;
    b.count = 1;
    GemmProb& g = b.p[0];
    g.A = A; g.lda = lda; g.W = W; g.ldw = ldw; g.C = C; g.ldc = ldc; g.M = M; g.N = N; g.K = K;
    g.scale = nullptr; g.shift = nullptr; g.resid = resid; g.ldr = ldr; g.act = 0; g.slope = 0.f;
    return launch_gemm(b, stream);
  };
  if (w.wave) {
    // ---- two layers as a wavefront: stage s runs the cell of (layer 1, step s) and of (layer 0, step s + 1).  Both
    // need only what stage s + 1 left: dh1_s = dG1_{s+1} . W_hh1, and dh0_{s+1} = dG0_{s+2} . W_hh0 + dG1_{s+1} . W_ih1
    // -- the cotangent of layer 0's output, which the layer-after-layer form gets from one batched product over all
    // steps afterwards, is the second K segment of layer 0's recurrent product here.  F + 1 stages of one launch (or
    // one launch pair) instead of 2 F; the batched dX product of layer 1 disappears.
    hipError_t e = launch_transpose(p->w_hh[1], H, w.wt_hh_up, 4 * H, 4 * H, H, stream);
    if (e == hipSuccess) e = launch_transpose(p->w_ih[1], H, w.wt_ih_up, 4 * H, 4 * H, H, stream);
    if (e == hipSuccess) e = launch_transpose(p->w_hh[0], H, w.wt, 4 * H, 4 * H, H, stream);
    if (e != hipSuccess) return fail(EMPOSE_EHIP, "transpose: %s", hipGetErrorString(e));
    HIP_TRY(hipMemsetAsync(w.dc, 0, bh * sizeof(float), stream));
    HIP_TRY(hipMemsetAsync(w.dc_up, 0, bh * sizeof(float), stream));
    auto cell_of = [&](int l, int t) {
      const float* sv = save + (size_t)l * 7 * bfh;
      LstmCellBwdArgs ca;
      ca.gates = sv; ca.c_all = sv + 4 * bfh; ca.c0 = c0 ? c0 + l * bh : nullptr;
      ca.dy = l == 1 ? dy : nullptr; ca.ld_dy = H; ca.dh_in = nullptr;
      ca.dc = l == 1 ? w.dc_up : w.dc; ca.dgates = l == 1 ? w.dgates_up : w.dgates;
      ca.dh_carry = l == 1 ? w.carry_up : w.carry;
      ca.seq_lengths = seq_lengths; ca.B = B; ca.F = F; ca.H = H; ca.t = t;
      return ca;
    };
    // stage F - 1: nothing flows into the last step of the top layer
    HIP_CHECK(launch_lstm_cell_bwd(cell_of(1, F - 1), stream), "lstm cell backward");
    for (int s = F - 2; s >= -1; --s) {
      RecBatch rb;
      LstmCellBwdArgs cells[2];
      rb.count = 0;
      if (s >= 0) {   // (layer 1, step s)
        RecProb& q = rb.p[rb.count];
        q.nseg = 1; q.seg[0] = RecSeg{w.dgates_up + (size_t)(s + 1) * 4 * H, F * 4 * H, w.wt_hh_up, 4 * H, 4 * H};
        q.M = B; q.N = H; q.resid = w.carry_up; q.ldr = H;
        cells[rb.count++] = cell_of(1, s);
      }
      {               // (layer 0, step s + 1)
        const int t0 = s + 1;
        RecProb& q = rb.p[rb.count];
        q.nseg = 0;
        if (t0 + 1 <= F - 1) q.seg[q.nseg++] = RecSeg{w.dgates + (size_t)(t0 + 1) * 4 * H, F * 4 * H, w.wt, 4 * H, 4 * H};
        q.seg[q.nseg++] = RecSeg{w.dgates_up + (size_t)t0 * 4 * H, F * 4 * H, w.wt_ih_up, 4 * H, 4 * H};
        q.M = B; q.N = H; q.resid = t0 + 1 <= F - 1 ? w.carry : nullptr; q.ldr = H;
        cells[rb.count++] = cell_of(0, t0);
      }
      HIP_CHECK(w.wave == 2 ? launch_rec_ksplit(rb, cells, w.rec, stream) : launch_rec_fewrows(rb, cells, stream), "recurrent backward (wavefront)");
    }
    // ---- the cotangents of the initial state, where asked for: dh_{-1} = dG_0 . W_hh + carry, dc_{-1} = what the cell of
    // step 0 left in the running cell cotangent
    for (int l = 0; l < 2; ++l) {
      if (grads->d_h0[l]) {
        HIP_CHECK(gemm(l == 1 ? w.dgates_up : w.dgates, F * 4 * H, l == 1 ? w.wt_hh_up : w.wt, 4 * H, grads->d_h0[l], H, B,
                       H, 4 * H, l == 1 ? w.carry_up : w.carry, H), "initial-state cotangent");
      }
      if (grads->d_c0[l])
        HIP_TRY(hipMemcpyAsync(grads->d_c0[l], l == 1 ? w.dc_up : w.dc, bh * sizeof(float), hipMemcpyDeviceToDevice, stream));
    }
    // ---- the batched products: weight gradients of both layers, the input cotangent of layer 0
    for (int l = 1; l >= 0; --l) {
      const float* sv = save + (size_t)l * 7 * bfh;
      const int in_l = l == 0 ? p->input_size : H;
      const float* x_l = l == 0 ? x : save + 6 * bfh;
      const int ldx_l = l == 0 ? ldx : H;
      float* dg = l == 1 ? w.dgates_up : w.dgates;
      AtbArgs ab{};
      ab.A = dg; ab.lda = 4 * H; ab.B = x_l; ab.ldb = ldx_l; ab.C = grads->w_ih[l]; ab.ldc = in_l;
      ab.bias = grads->b_ih[l]; ab.M = B * F; ab.N = 4 * H; ab.K = in_l;
      HIP_CHECK(launch_gemm_atb(ab, w.atb, w.atb_floats, stream), "dW_ih");
      HIP_TRY(hipMemcpyAsync(grads->b_hh[l], grads->b_ih[l], (size_t)4 * H * sizeof(float), hipMemcpyDeviceToDevice, stream));
      ab.B = sv + 5 * bfh; ab.ldb = H; ab.C = grads->w_hh[l]; ab.ldc = H; ab.bias = nullptr; ab.K = H;
      HIP_CHECK(launch_gemm_atb(ab, w.atb, w.atb_floats, stream), "dW_hh");
    }
    if (dx) {
      HIP_CHECK(launch_transpose(p->w_ih[0], p->input_size, w.wt, 4 * H, 4 * H, p->input_size, stream), "transpose");
      HIP_CHECK(gemm(w.dgates, 4 * H, w.wt, 4 * H, dx, p->input_size, B * F, p->input_size, 4 * H, nullptr, 0), "dX gemm");
    }
    return EMPOSE_OK;
  }
  for (int l = L - 1; l >= 0; --l) {
    const float* sv = save + (size_t)l * 7 * bfh;
    const int in_l = l == 0 ? p->input_size : H;
    const float* x_l = l == 0 ? x : save + (size_t)(l - 1) * 7 * bfh + 6 * bfh;
    const int ldx_l = l == 0 ? ldx : H;
    const float* dy_l = l == L - 1 ? dy : w.dyl;
    // W_hh^T for the recurrent product dh_{t-1} = dG_t . W_hh on the forward GEMM kernel
    HIP_CHECK(launch_transpose(p->w_hh[l], H, w.wt, 4 * H, 4 * H, H, stream), "transpose");
    HIP_TRY(hipMemsetAsync(w.dc, 0, bh * sizeof(float), stream));
    const float* dh_in = nullptr;
    auto cell_args = [&](int t, const float* dh) {
      LstmCellBwdArgs ca;
      ca.gates = sv; ca.c_all = sv + 4 * bfh; ca.c0 = c0 ? c0 + l * bh : nullptr;
      ca.dy = dy_l; ca.ld_dy = H; ca.dh_in = dh; ca.dc = w.dc; ca.dgates = w.dgates; ca.dh_carry = w.carry;
      ca.seq_lengths = seq_lengths; ca.B = B; ca.F = F; ca.H = H; ca.t = t;
      return ca;
    };
    bool cell_done = false;   // the cell of step t already ran inside the previous step's reduce kernel
    for (int t = F - 1; t >= 0; --t) {
      if (!cell_done) {
        LstmCellBwdArgs ca = cell_args(t, dh_in);
        HIP_CHECK(launch_lstm_cell_bwd(ca, stream), "lstm cell backward");
      }
      cell_done = false;
      if (t == 0) break;
      float* out = w.dh[t & 1];
      hipError_t e;
      if (w.ksplit) {   // a few hundred rows: K split over the workgroups (gemm_ksplit_kernel); its reduce kernel
        GemmProb g;     // feeds dh straight into the cell of step t - 1 (the carry of step t is the residual)
        g.A = w.dgates + (size_t)t * 4 * H; g.lda = F * 4 * H; g.W = w.wt; g.ldw = 4 * H; g.C = out; g.ldc = H;
        g.M = B; g.N = H; g.K = 4 * H; g.scale = nullptr; g.shift = nullptr; g.resid = w.carry; g.ldr = H; g.act = 0;
        g.slope = 0.f;
        LstmCellBwdArgs cn = cell_args(t - 1, nullptr);
        e = launch_gemm_ksplit(g, w.ksplit, stream, &cn);
        cell_done = true;
      } else if (gemm_fewrows_applicable(B, H, 4 * H)) {   // the reference's batch: matrix-vector kernel, same fusion
        GemmProb g;
        g.A = w.dgates + (size_t)t * 4 * H; g.lda = F * 4 * H; g.W = w.wt; g.ldw = 4 * H; g.C = out; g.ldc = H;
        g.M = B; g.N = H; g.K = 4 * H; g.scale = nullptr; g.shift = nullptr; g.resid = w.carry; g.ldr = H; g.act = 0;
        g.slope = 0.f;
        e = launch_gemm_fewrows_cell(g, cell_args(t - 1, nullptr), stream);
        cell_done = true;
      } else {
        e = gemm(w.dgates + (size_t)t * 4 * H, F * 4 * H, w.wt, 4 * H, out, H, B, H, 4 * H, w.carry, H);
      }
      if (e != hipSuccess) return fail(EMPOSE_EHIP, "recurrent backward gemm: %s", hipGetErrorString(e));
      dh_in = out;
    }
    // the cotangents of this layer's initial state, where asked for (w.wt still holds W_hh^T, w.carry / w.dc what the cell
    // of step 0 left)
    if (grads->d_h0[l]) {
      HIP_CHECK(gemm(w.dgates, F * 4 * H, w.wt, 4 * H, grads->d_h0[l], H, B, H, 4 * H, w.carry, H), "initial-state cotangent");
    }
    if (grads->d_c0[l])
      HIP_TRY(hipMemcpyAsync(grads->d_c0[l], w.dc, bh * sizeof(float), hipMemcpyDeviceToDevice, stream));
    AtbArgs ab{};
    ab.A = w.dgates; ab.lda = 4 * H; ab.B = x_l; ab.ldb = ldx_l; ab.C = grads->w_ih[l]; ab.ldc = in_l;
    ab.bias = grads->b_ih[l]; ab.M = B * F; ab.N = 4 * H; ab.K = in_l;
    HIP_CHECK(launch_gemm_atb(ab, w.atb, w.atb_floats, stream), "dW_ih");
    HIP_TRY(hipMemcpyAsync(grads->b_hh[l], grads->b_ih[l], (size_t)4 * H * sizeof(float), hipMemcpyDeviceToDevice, stream));
    ab.B = sv + 5 * bfh; ab.ldb = H; ab.C = grads->w_hh[l]; ab.ldc = H; ab.bias = nullptr; ab.K = H;
    HIP_CHECK(launch_gemm_atb(ab, w.atb, w.atb_floats, stream), "dW_hh");
    float* dx_l = l > 0 ? w.dyl : dx;
    if (dx_l) {
      HIP_CHECK(launch_transpose(p->w_ih[l], in_l, w.wt, 4 * H, 4 * H, in_l, stream), "transpose");
      HIP_CHECK(gemm(w.dgates, 4 * H, w.wt, 4 * H, dx_l, in_l, B * F, in_l, 4 * H, nullptr, 0), "dX gemm");
    }
  }
  return EMPOSE_OK;
}

}  // extern "C"
