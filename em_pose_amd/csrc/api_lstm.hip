// C ABI (include/empose_hip.h), LSTM, host code only.  Inference: plan_lstm decides what a call does (api_internal.h
// LstmPlan), carve_lstm_of hands out the buffers the plan names, LstmRun walks it, one function per path.  Packing: the
// three-piece bf16 weights in every layout of LSTM_LAYOUTS and the scaled pieces of lstm_chain16_pair_kernel.  Training (empose_lstm_train_*): the forward saves what LstmSave
// lays out; back-propagation through time (Bptt) is two recurrences over one cell builder and one batched tail.
#include "api_internal.h"
#include "f16pair.h"
#include "gemm_kernels.h"
#include "lstm_kernels.h"
#include "lstm_wave.h"
#include "options.h"
#include "train_kernels.h"

#include <algorithm>

using namespace empose;
using namespace empose::api;

namespace {

// ---- the plan ---------------------------------------------------------------------------------------------------------
// bf16 elements of one set of A planes: [32-row tiles][k-steps][3 pieces][512]
size_t lstm_x3_plane_elems(int B, int K) { return (size_t)((B + 31) / 32) * ((K + 15) / 16) * 3 * 512; }
bool has_layout(const Lstm& r, LstmLayout y) {
  for (int l = 0; l < r.num_layers; ++l)
    if (!r.w3[y].ih[l] || !r.w3[y].hh[l]) return false;
  return true;
}
// The three-piece step kernels by LstmStep (wave: fp32, none of this).  A new one is an entry here, one in the enum, a line in plan_lstm.
struct X3Step { hipError_t (*launch)(const LstmX3Args&, hipStream_t); LstmLayout layout; };
const X3Step X3_STEPS[] = {{nullptr, LSTM_CHAIN}, {launch_lstm_chain_x3, LSTM_CHAIN}, {launch_lstm_rows_x3, LSTM_CHAIN},
                           {launch_lstm_mid_x3, LSTM_MID}, {launch_lstm_mid16_x3, LSTM_MID16},
                           {launch_lstm_chain16_x3, LSTM_MID16}, {launch_lstm_chain16_pair, LSTM_MID16}};
// the scaled pieces of lstm_chain16_pair_kernel (pack_lstm_pair16)
bool has_pair16(const Lstm& r) {
  for (int l = 0; l < r.num_layers; ++l)
    if (!r.w_pair.hh[l] || !r.w_wide.hh[l] || !r.inv_scale[l] || !(l == 0 ? r.w_wide.ih[l] : r.w_pair.ih[l])) return false;
  return true;
}
// medium batches step on lstm_mid_x3.hip from 17 rows (below: lstm_persist_kernel / lstm_fewrows_kernel), and from 9 with the
// 4-unit tiles of lstm_mid16_x3.hip (7.0 us per step against 7.8 - 10.7 of lstm_fewrows_kernel at 9 - 16 rows)
constexpr int LSTM_MID16_MIN_B = 9;
constexpr int LSTM_MIDSEQ_MIN_B = 4, LSTM_MIDSEQ_MAX_B = 64;   // (up to 3 rows: lstm_persist_kernel)

// fp32 steps: up to LSTM_SMALL_B rows the weight-streaming kernels of lstm_fewrows.hip, up to LSTM_MID_B lstm_mid_kernel, above
// lstm_chain_kernel -- lstm_mid_kernel against lstm_chain_kernel, us per wavefront step of the 2 x 512 stack
// (scripts/dev/bench_lstm_mid.py): B = 17..128: 17 vs 36, B = 256: 22 vs 37, B = 512: 44 vs 37.
constexpr int LSTM_SMALL_B = 16, LSTM_MID_B = 256;
static_assert(LSTM_MID_B + 1 == LSTM_SEQ_MIN_B, "lstm_seq_kernel takes over where lstm_chain_kernel does");

// The fp32 part of a plan, from the shape alone (inference, the layers of a bidirectional stack and the training forward
// alike): the step kernel, the buffers of the whole-sequence kernels and whether they are tried.  With plan_lstm below
// the only reader of the LSTM dispatch options.
LstmPlan plan_lstm_f32(const LstmShape& s) {
  const Options& o = options();
  LstmPlan p;
  const int B = s.B, n_k = s.n_units < 4 ? s.n_units : 4;   // (in_k has four entries; deeper stacks are refused at run time)
  if (B > LSTM_MID_B) p.wave = LstmWave::chain;
  else if (B > LSTM_SMALL_B) p.wave = LstmWave::mid;
  // from 4 rows all threads of a workgroup split K (reduce-scatter), below a wave per hidden unit
  else if (o.lstm_fewrows != 0 && B >= LSTM_FEWROWS_MIN_B && lstm_fewrows_shape_ok(B, s.H, n_k, s.in_k)) p.wave = LstmWave::fewrows;
  else p.wave = LstmWave::small;
  // Chain all units in one block (equal work per block) once the tiles alone fill the CUs; spread them otherwise.
  p.chain_all_units = ((s.H + lc::BU - 1) / lc::BU) * ((B + lc::BM - 1) / lc::BM) >= 192;
  if (!s.stacked) return p;   // bidirectional: layer after layer, step launches only
  // the whole-sequence kernels get their buffers by shape alone (the options gate their launches below)
  p.persist = B <= LSTM_PERSIST_B;
  p.seq = B >= LSTM_SEQ_MIN_B && s.n_units <= 4;
  // the whole sequence in one cooperative launch, from 4 steps; tried in this order
  if (s.F >= 4 && s.n_units <= 4) {
    // (from 4 rows on a step launch of lstm_fewrows_kernel is faster than polling B x H exchange words per layer and step)
    if (p.persist && o.lstm_persist != 0 && (o.lstm_fewrows == 0 || B < LSTM_FEWROWS_MIN_B) &&
        lstm_persist_shape_ok(B, s.H, s.n_units, s.in_k))
      p.coop[p.n_coop++] = LstmCoop::persist;
    if (p.seq && o.lstm_seq != 0 && lstm_seq_shape_ok(s.H, s.n_units, s.in_k)) p.coop[p.n_coop++] = LstmCoop::seq;
  }
  return p;
}
LstmShape stacked_shape(int L, int input_size, int H, int B, int F) {
  LstmShape s{B, F, H, L, {}, true};
  for (int l = 0; l < L && l < 4; ++l) s.in_k[l] = l == 0 ? input_size : H;
  return s;
}

// With plan_lstm_f32 the only reader of the LSTM options and shapes; `fresh_state`: new sequences (no h0, no c0).
LstmPlan plan_lstm(const Lstm& r, int B, int F, bool fresh_state) {
  const Options& o = options();
  if (r.dirs != 1) return LstmPlan();   // bidirectional: no buffers; LstmRun::bidirectional plans each layer's steps
  LstmPlan p = plan_lstm_f32(stacked_shape(r.num_layers, r.input_size, r.H, B, F));
  const bool x3 = o.lstm_x3 != 0 && r.num_layers <= 4 && r.H % 32 == 0 && r.input_size % 4 == 0;
  const bool mid = x3 && o.lstm_mid_x3 != 0 && has_layout(r, LSTM_MID);
  // ... up to 64 rows with half the tile, on all 256 CUs (lstm_mid16_x3.hip)
  const bool tiles16 = mid && o.lstm_mid16 != 0 && lstm_mid16_shape_ok(B, r.H) && has_layout(r, LSTM_MID16);
  // lstm_midseq_x3.hip gets its buffers by shape and options (it needs the 8-unit-block weight order too)
  if (mid && o.lstm_midseq != 0 && B >= LSTM_MIDSEQ_MIN_B && B <= LSTM_MIDSEQ_MAX_B) {
    int ks_in[4];
    for (int l = 0; l < r.num_layers; ++l) ks_in[l] = l == 0 ? (r.input_size + 15) / 16 : r.H / 16;
    p.midseq = lstm_midseq_shape_ok(B, r.H, r.num_layers, ks_in);
  }
  // the steps: large batches on lstm_x3.hip (or lstm_rows_x3.hip / lstm_chain16_x3.hip), medium ones on lstm_mid16_x3.hip /
  // lstm_mid_x3.hip
  if (x3 && B >= LSTM_SEQ_MIN_B && has_layout(r, LSTM_CHAIN)) {
    p.step = o.lstm_x3 == 2 ? LstmStep::rows_x3 : LstmStep::chain_x3;
    // the same step on the 16x16x32 instruction: what the default takes (lstm_chain16), and what lstm_x3 = 3 forces
    const bool want16 = o.lstm_x3 == 3 || (o.lstm_x3 == 1 && o.lstm_chain16 != 0);
    if (want16 && has_layout(r, LSTM_MID16)) p.step = LstmStep::chain16_x3;
    // ... and within that kernel, how many pieces (lstm_pair16, as mlp_pair16 within mlp_fused16)
    if (p.step == LstmStep::chain16_x3 && o.lstm_pair16 != 0 && has_pair16(r)) p.step = LstmStep::chain16_pair;
  }
  else if (mid && B >= (tiles16 ? LSTM_MID16_MIN_B : LSTM_PERSIST_B + 1) && B < LSTM_SEQ_MIN_B)
    p.step = tiles16 ? LstmStep::mid16_x3 : LstmStep::mid_x3;
  p.layout = X3_STEPS[(int)p.step].layout;
  p.x3 = p.step != LstmStep::wave || p.midseq;
  // the whole sequence in one cooperative launch, from 4 steps; tried after those of plan_lstm_f32
  if (F >= 4 && p.midseq) p.coop[p.n_coop++] = LstmCoop::midseq;
  p.zero_planes = p.step != LstmStep::wave && fresh_state && o.lstm_state_direct != 0;
  const bool chain = p.step == LstmStep::chain_x3 || p.step == LstmStep::chain16_x3 || p.step == LstmStep::chain16_pair;
  p.state_direct = p.zero_planes && chain;
  p.skip_dead = chain && o.lstm_skip_dead != 0;
  return p;
}

// the wavefront kernels address their operands with 32-bit byte offsets from a per-segment base; `width`: the widest row
int check_offsets_fit(int B, int F, int ldx, int width) {
  if ((size_t)B * F * (size_t)(ldx > width ? ldx : width) * sizeof(float) >= ((size_t)1 << 32))
    return fail(EMPOSE_EINVAL, "LSTM batch of %d x %d frames is too large for one call; split the batch", B, F);
  return EMPOSE_OK;
}
// one [B][H] state buffer of a unit: the caller's initial state, zero without one
hipError_t init_state(float* dst, const float* src, size_t bh, hipStream_t stream) {
  return src ? hipMemcpyAsync(dst, src, bh * sizeof(float), hipMemcpyDeviceToDevice, stream)
             : hipMemsetAsync(dst, 0, bh * sizeof(float), stream);
}
void fill_unit(LstmUnitArgs& ua, const float* w_ih, const float* w_hh, const float* bias, const LstmWs& ws, int u) {
  ua.w_ih = w_ih; ua.w_hh = w_hh; ua.bias = bias;
  ua.h[0] = ws.h[u][0]; ua.h[1] = ws.h[u][1]; ua.c = ws.c[u];
  ua.in_seq = nullptr; ua.in_ld = 0; ua.in_from = -1; ua.t_offset = 0; ua.reverse = 0;
  ua.y = nullptr; ua.y_ld = 0; ua.y_col = 0;
}
// Stacked uni-directional layers: wavefront over (layer, time), launch s advances layer l by its step s - l.
LstmWaveArgs stacked_wave_args(int L, int input_size, int H, const float* const* w_ih, const float* const* w_hh,
                               const float* const* bias, const LstmWs& ws, int B, int F, const float* x, int ldx,
                               const int* seq_lengths, float* y) {
  LstmWaveArgs a;
  a.seq_lengths = seq_lengths; a.B = B; a.F = F; a.H = H; a.n_units = L; a.s = 0;
  for (int l = 0; l < L; ++l) {
    LstmUnitArgs& ua = a.unit[l];
    fill_unit(ua, w_ih[l], w_hh[l], bias[l], ws, l);
    ua.in_k = l == 0 ? input_size : H;
    if (l == 0) { ua.in_seq = x; ua.in_ld = ldx; }
    else ua.in_from = l - 1;
    ua.t_offset = l;
    if (l == L - 1) { ua.y = y; ua.y_ld = H; }
  }
  return a;
}
// the fp32 steps on the kernel the plan names, one launch per wavefront step
int wave_steps(LstmWaveArgs& a, const LstmPlan& p, int n_steps, bool mark, hipStream_t stream) {
  const int units_per_block = p.wave == LstmWave::chain && p.chain_all_units ? a.n_units : 1;
  for (int s = 0; s < n_steps; ++s) {
    a.s = s;
    lstm_build_chain(a, units_per_block);
    if (mark) prof_mark(P_LSTM_STEP, stream);
    HIP_CHECK(p.wave == LstmWave::chain ? launch_lstm_chain(a, units_per_block, stream)
              : p.wave == LstmWave::mid ? launch_lstm_mid(a, stream)
              : p.wave == LstmWave::fewrows ? launch_lstm_fewrows(a, stream) : launch_lstm_small(a, stream), "lstm step");
  }
  return EMPOSE_OK;
}

// ---- run_lstm: the arguments of a call, its plan, and one function per path ------------------------------------------
struct LstmRun {
  const Lstm& r; int B, F; const float* x; int ldx; const int* seq_lengths; const float* h0; const float* c0;
  float* y; float* h_n; float* c_n; const LstmWs& ws; hipStream_t stream; LstmPlan p;
  size_t bh() const { return (size_t)B * r.H; }
  int units() const { return r.num_layers * r.dirs; }
  int set_initial_state() const {
    prof_mark(P_COPY, stream);
    if (!h0 && !c0) {
      // new sequences: the state buffers of all units are carved back to back (carve_lstm_of) -- one fill instead of 2 U
      const char* lo = reinterpret_cast<const char*>(ws.h[0][0]);
      const char* hi = reinterpret_cast<const char*>(ws.c[units() - 1] + bh());
      HIP_TRY(hipMemsetAsync(ws.h[0][0], 0, (size_t)(hi - lo), stream));
      return EMPOSE_OK;
    }
    for (int u = 0; u < units(); ++u) {
      HIP_TRY(init_state(ws.h[u][0], h0 ? h0 + u * bh() : nullptr, bh(), stream));
      HIP_TRY(init_state(ws.c[u], c0 ? c0 + u * bh() : nullptr, bh(), stream));
    }
    return EMPOSE_OK;
  }
  // The operands of the three-piece kernels, for the one-launch medium-batch path and the step path alike: k-steps of 16 of a
  // layer's input (recurrent operand: ks_in(1)), the stored input and a layer's initial hidden state as bf16 piece planes.
  int ks_in(int l) const { return l == 0 ? (r.input_size + 15) / 16 : r.H / 16; }
  hipError_t split_input() const {
    prof_mark(P_COPY, stream);
    return launch_lstm_split_rows(x, (long)F * ldx, ldx, F, B, r.input_size, ks_in(0), ws.x3, (long)ws.x3_t_stride, stream);
  }
  hipError_t split_state(int l, unsigned short* planes) const {
    return launch_lstm_split_rows(ws.h[l][0], r.H, 0, 1, B, r.H, ks_in(1), planes, 0, stream);
  }
  // Medium batches, inference: the whole sequence in one cooperative launch on three bf16 pieces per operand, weights in
  // registers (lstm_midseq_x3.hip).
  int midseq(bool* done) const {
    const int L = r.num_layers;
    hipError_t e = split_input();
    for (int l = 0; l < L && e == hipSuccess; ++l) e = split_state(l, ws.xa[l]);
    if (e != hipSuccess) return fail(EMPOSE_EHIP, "lstm operand split: %s", hipGetErrorString(e));
    LstmMidSeqArgs qa;
    qa.n_units = L; qa.seq_lengths = seq_lengths; qa.B = B; qa.F = F; qa.H = r.H; qa.flags = ws.midseq_flags;
    for (int l = 0; l < 4; ++l) {
      const int ll = l < L ? l : 0;
      LstmMidSeqUnit& qu = qa.unit[l];
      qu.w3_ih = r.w3[LSTM_MID].ih[ll]; qu.w3_hh = r.w3[LSTM_MID].hh[ll]; qu.bias = r.bias[ll];
      qu.in3 = ws.x3; qu.in_t_stride = ws.x3_t_stride; qu.ks_in = ks_in(ll);
      qu.xa = ws.xa[ll]; qu.h0 = ws.h[ll][0]; qu.h_last = ws.h[ll][F & 1]; qu.c = ws.c[ll];
      qu.y = ll == L - 1 ? y : nullptr; qu.y_ld = r.H; qu.y_col = 0;
    }
    prof_mark(P_LSTM_STEP, stream);
    HIP_CHECK(launch_lstm_midseq_x3(qa, stream, done), "lstm sequence kernel (medium batch)");
    return EMPOSE_OK;
  }
  // One cooperative attempt at the whole sequence; *done = false: its workgroups cannot all be resident here.  Small
  // batches: weights in registers, grid barrier per step; large ones: the workgroups of a row group synchronise by counters.
  int coop(LstmCoop which, const LstmWaveArgs& a, bool* done) const {
    if (which == LstmCoop::midseq) return midseq(done);
    prof_mark(P_LSTM_STEP, stream);
    if (which == LstmCoop::persist) HIP_CHECK(launch_lstm_persist(a, ws.xch, stream, done), "lstm sequence kernel");
    else HIP_CHECK(launch_lstm_seq(a, ws.h3, ws.seq_cnt, stream, done), "lstm sequence kernel (large batch)");
    return EMPOSE_OK;
  }
  // Inference: the steps on the bf16 matrix path with three bf16 pieces per operand, kernel and weight layout by the plan.
  int x3_steps() const {
    const int H = r.H, L = r.num_layers;
    const LstmW3& w3 = r.w3[p.layout];
    hipError_t e = split_input();
    const size_t plane_bytes = lstm_x3_plane_elems(B, H) * sizeof(unsigned short);
    if (p.zero_planes) {
      // New sequences: the pieces of a zero state are zero planes, and the 2 L hidden-state planes are carved back to back
      // (carve_lstm_of) -- one fill instead of a split launch and a fill per layer.  On the chain kernel (p.state_direct)
      // the last step of each layer then stores h_n / c_n itself (rows past their length included: it rewrites their
      // frozen state at every step), so the 2 L trailing copies go too.
      // (checked, not assumed: the fill below covers [a3[0][0], a3[L-1][1] + plane) and must hit these planes only)
      const char* lo = reinterpret_cast<const char*>(ws.a3[0][0]);
      const size_t stride = align_up((lstm_x3_plane_elems(B, H) + 1) / 2 * sizeof(float));
      for (int l = 0; l < L; ++l)
        for (int i = 0; i < 2; ++i)
          if (reinterpret_cast<const char*>(ws.a3[l][i]) != lo + (size_t)(2 * l + i) * stride)
            return fail(EMPOSE_EINVAL, "internal: the LSTM hidden-state planes are not carved back to back");
      const size_t span = (size_t)(2 * L - 1) * stride + plane_bytes;
      if (e == hipSuccess) e = hipMemsetAsync(ws.a3[0][0], 0, span, stream);
    } else {
      for (int l = 0; l < L && e == hipSuccess; ++l) {
        e = split_state(l, ws.a3[l][0]);
        if (e == hipSuccess) e = hipMemsetAsync(ws.a3[l][1], 0, plane_bytes, stream);
      }
    }
    if (e != hipSuccess) return fail(EMPOSE_EHIP, "lstm operand split: %s", hipGetErrorString(e));
    for (int s = 0; s < F + L - 1; ++s) {
      LstmX3Args xa;
      xa.n_units = 0; xa.seq_lengths = seq_lengths; xa.B = B; xa.F = F; xa.H = H;
      // (without lengths every row is live at every step: h_prev is never used, and on the direct path h_next is only the
      // next step's h_prev)
      xa.skip_h_state = p.skip_dead && p.state_direct && !seq_lengths;
      for (int l = 0; l < L; ++l) {
        const int t = s - l;
        if (t < 0 || t >= F) continue;
        LstmX3Unit& xu = xa.unit[xa.n_units++];
        xu.w3_ih = w3.ih[l]; xu.w3_hh = w3.hh[l]; xu.bias = r.bias[l];
        xu.a3_in = l == 0 ? ws.x3 + (size_t)t * ws.x3_t_stride : ws.a3[l - 1][(t + 1) & 1];
        xu.ks_in = ks_in(l);
        // (a new sequence's first step: h_{-1} is the zero plane -- its k-steps only add +-0)
        xu.ks_rec = p.skip_dead && p.zero_planes && t == 0 ? 0 : ks_in(1);
        xu.a3_rec = ws.a3[l][t & 1]; xu.a3_out = ws.a3[l][(t + 1) & 1];
        xu.h_prev = ws.h[l][t & 1]; xu.h_next = ws.h[l][(t + 1) & 1]; xu.c = ws.c[l];
        xu.y = l == L - 1 ? y : nullptr; xu.y_ld = H; xu.y_col = 0; xu.t = t;
        const bool last_step = p.state_direct && t == F - 1;
        xu.h_final = last_step && h_n ? h_n + l * bh() : nullptr;
        xu.c_final = last_step && c_n ? c_n + l * bh() : nullptr;
        if (p.step == LstmStep::chain16_pair) {
          // Pair steps for what the kernel wrote itself: the layer below's h_t, and h_{t-1} from the second step on (a
          // new sequence's zero planes are zero in either format).  Wide steps for the stored input and for a caller's
          // h0, which split_state left as three bf16 pieces: neither is bounded by 1.
          xu.in_pair = l > 0;
          xu.rec_pair = !(h0 && t == 0);
          xu.w3_ih = xu.in_pair ? r.w_pair.ih[l] : r.w_wide.ih[l];
          xu.w3_hh = xu.rec_pair ? r.w_pair.hh[l] : r.w_wide.hh[l];
          xu.inv_scale = r.inv_scale[l];
        }
      }
      xa.units_per_block = p.chain_all_units ? xa.n_units : 1;
      prof_mark(P_LSTM_STEP, stream);
      HIP_CHECK(X3_STEPS[(int)p.step].launch(xa, stream), "lstm step (bf16 pieces)");
    }
    return EMPOSE_OK;
  }
  // Bidirectional: a layer needs the whole output sequence of the layer below, so layers run one after the other; the two
  // directions of a layer share each launch.
  int bidirectional() const {
    const int H = r.H, L = r.num_layers;
    LstmWaveArgs a;
    a.seq_lengths = seq_lengths; a.B = B; a.F = F; a.H = H; a.n_units = 2;
    for (int l = 0; l < L; ++l) {
      const int in_k = l == 0 ? r.input_size : 2 * H;
      for (int d = 0; d < 2; ++d) {
        LstmUnitArgs& ua = a.unit[d];
        fill_unit(ua, r.w_ih[l * 2 + d], r.w_hh[l * 2 + d], r.bias[l * 2 + d], ws, l * 2 + d);
        ua.in_k = in_k;
        ua.in_seq = l == 0 ? x : ws.yb[(l - 1) & 1]; ua.in_ld = l == 0 ? ldx : 2 * H; ua.reverse = d;
        ua.y = l == L - 1 ? y : ws.yb[l & 1]; ua.y_ld = 2 * H; ua.y_col = d * H;
      }
      TRY(wave_steps(a, plan_lstm_f32(LstmShape{B, F, H, 2, {in_k, in_k}, false}), F, true, stream));
    }
    return EMPOSE_OK;
  }
  // the final hidden state: buffer F & 1 after step launches, F % 3 of (h[0], h[1], h3) after the large-batch sequence kernel
  int store_final_state(bool seq_done) const {
    prof_mark(P_COPY, stream);
    for (int u = 0; u < units(); ++u) {
      const float* h_last = seq_done ? (F % 3 == 2 ? ws.h3[u] : ws.h[u][F % 3]) : ws.h[u][F & 1];
      if (h_n) HIP_TRY(hipMemcpyAsync(h_n + u * bh(), h_last, bh() * sizeof(float), hipMemcpyDeviceToDevice, stream));
      if (c_n) HIP_TRY(hipMemcpyAsync(c_n + u * bh(), ws.c[u], bh() * sizeof(float), hipMemcpyDeviceToDevice, stream));
    }
    return EMPOSE_OK;
  }

  int run() const {
    TRY(set_initial_state());
    bool done = false, seq_done = false;
    if (r.dirs == 1) {
      if (r.num_layers > 4) return fail(EMPOSE_EINVAL, "at most 4 stacked layers per wavefront");
      LstmWaveArgs a = stacked_wave_args(r.num_layers, r.input_size, r.H, r.w_ih, r.w_hh, r.bias, ws, B, F, x, ldx, seq_lengths, y);
      for (int i = 0; i < p.n_coop && !done; ++i) {
        TRY(coop(p.coop[i], a, &done));
        seq_done = done && p.coop[i] == LstmCoop::seq;
      }
      if (!done && p.step == LstmStep::wave) TRY(wave_steps(a, p, F + r.num_layers - 1, true, stream));
      if (!done && p.step != LstmStep::wave) {
        TRY(x3_steps());
        if (p.state_direct) return EMPOSE_OK;   // the last step of each layer has stored h_n / c_n itself
      }
    } else {
      if (!seq_lengths) return fail(EMPOSE_EINVAL, "bidirectional LSTM needs seq_lengths");
      TRY(bidirectional());
    }
    return store_final_state(seq_done);
  }
};

// ---- packing ----------------------------------------------------------------------------------------------------------
// An LSTM weight matrix [4H][K] (gate-major rows) as three bf16 pieces per weight, in wave fragments of 512 bf16 ordered
// [k-step][unit block][fragment of the block].  A fragment is 512 / k_width columns by k_width k: lane (n = lane % columns,
// q = lane / columns) owns W[row of column n][k-step * k_width + q * 8 .. + 7]; k past K is zero.  Column n of fragment f
// is gate f * (4 / frags) + n / units of hidden unit block * units + n % units:
//   chain  {16, 32, 4}  a fragment per gate of a 32-unit block (32x32x16 instruction: n = lane & 31, half = lane >> 5)
//   mid    {16, 8, 1}   the four gates of 8 units in one 32-column fragment: gate n >> 3 of unit block * 8 + (n & 7)
//   mid16  {32, 4, 1}   16x16x32 instruction (n = lane & 15, q = lane >> 4): gate n >> 2 of unit block * 4 + (n & 3)
struct LstmLayoutDesc { int k_width, units, frags; };
constexpr LstmLayoutDesc LSTM_LAYOUTS[LSTM_N_LAYOUTS] = {{16, 32, 4}, {16, 8, 1}, {32, 4, 1}};
int pack_lstm_x3(std::vector<void*>& allocs, LstmLayout layout, const float* w, int H, int K, unsigned short** out) {
  const LstmLayoutDesc d = LSTM_LAYOUTS[layout];
  const int KS = (K + d.k_width - 1) / d.k_width, JB = H / d.units, NQ = d.frags, cols = 512 / d.k_width;
  return upload_bf16(allocs, pack_fragments_x3((size_t)KS * JB * NQ, K, [&](size_t f, int lane, const float** row, int* k0) {
    const int q = (int)(f % NQ), jb = (int)(f / NQ % JB), ks = (int)(f / NQ / JB), n = lane % cols;
    *row = w + (size_t)((q * (4 / NQ) + n / d.units) * H + jb * d.units + n % d.units) * K;
    *k0 = ks * d.k_width + lane / cols * 8;
    return true;
  }), out);
}

// The weights of lstm_chain16_pair_kernel for one layer, in the mid16 order at the three-piece stride.  Gate column n has
// one scale s_n = 2^e(n), e from the largest finite magnitude of row n of [W_ih | W_hh] (pair16::scale_exp; at most 2^100,
// so that 2^-14 / s_n stays a normal number).  pair: hi, lo = the two f16 pieces of w s_n, third slot zero; wide: the three
// bf16 pieces of w s_n 2^14 -- scaling by a power of two before the split is exact.  inv: [4H] 2^-14 / s_n.
int pack_lstm_pair16(std::vector<void*>& allocs, int l, const float* w_ih, const float* w_hh, int H, int K_in, Lstm* out) {
  const int N = 4 * H;
  std::vector<float> sc(N), inv(N);
  for (int n = 0; n < N; ++n) {
    unsigned m = 0u;
    for (int k = 0; k < K_in; ++k) m = std::max(m, pair16::finite_abs_bits(w_ih[(size_t)n * K_in + k]));
    for (int k = 0; k < H; ++k) m = std::max(m, pair16::finite_abs_bits(w_hh[(size_t)n * H + k]));
    const int e = std::min(pair16::scale_exp(m), 100);
    sc[n] = pair16::pow2(e);
    inv[n] = pair16::pow2(-e - pair16::EXP_TOP);
  }
  auto wide = [&](const float* w, int K, unsigned short** dst) {
    std::vector<float> ws((size_t)N * K);
    for (int n = 0; n < N; ++n)
      for (int k = 0; k < K; ++k) ws[(size_t)n * K + k] = w[(size_t)n * K + k] * sc[n] * pair16::pow2(pair16::EXP_TOP);
    return pack_lstm_x3(allocs, LSTM_MID16, ws.data(), H, K, dst);
  };
  auto pair = [&](const float* w, int K, unsigned short** dst) {
    const LstmLayoutDesc d = LSTM_LAYOUTS[LSTM_MID16];
    const int KS = (K + d.k_width - 1) / d.k_width, JB = H / d.units, cols = 512 / d.k_width;
    std::vector<unsigned short> buf((size_t)KS * JB * 3 * FRAG, 0);
    for (int ks = 0; ks < KS; ++ks)
      for (int jb = 0; jb < JB; ++jb)
        for (int lane = 0; lane < 64; ++lane) {
          const int c = lane % cols, n = (c / d.units) * H + jb * d.units + c % d.units, k0 = ks * d.k_width + lane / cols * 8;
          for (int e = 0; e < 8 && k0 + e < K; ++e) {
            const float x = w[(size_t)n * K + k0 + e] * sc[n];
            const _Float16 hi = (_Float16)x;                       // round to nearest even
            const _Float16 lo = (_Float16)(x - (float)hi);
            const size_t at = ((size_t)ks * JB + jb) * 3 * FRAG + (size_t)lane * 8 + e;
            buf[at] = __builtin_bit_cast(unsigned short, hi);
            buf[at + FRAG] = __builtin_bit_cast(unsigned short, lo);
          }
        }
    return upload_bf16(allocs, buf, dst);
  };
  TRY(l == 0 ? wide(w_ih, K_in, &out->w_wide.ih[l]) : pair(w_ih, K_in, &out->w_pair.ih[l]));
  TRY(pair(w_hh, H, &out->w_pair.hh[l]));
  TRY(wide(w_hh, H, &out->w_wide.hh[l]));
  return upload(allocs, inv.data(), inv.size(), &out->inv_scale[l]);
}

// ---- training ---------------------------------------------------------------------------------------------------------
// The save buffer of empose_lstm_train_*: per layer PLANES planes of [B][F][H], batch-major like y -- the activated gates
// (i | f | g | o: [B][F][4H]), the cell state after every step, the hidden state BEFORE every step, and the layer's output
// sequence (the input of the layer above; the top layer's goes to the caller's y instead).
struct LstmSave {
  static constexpr int GATE_PLANES = 4, PLANES = GATE_PLANES + 3;
  size_t bfh;
  LstmSave(int B, int F, int H) : bfh((size_t)B * F * H) {}
  size_t floats(int L) const { return (size_t)L * PLANES * bfh; }
  template <typename T> T* gates(T* save, int l) const { return save + (size_t)l * PLANES * bfh; }
  template <typename T> T* c(T* save, int l) const { return gates(save, l) + GATE_PLANES * bfh; }
  template <typename T> T* hprev(T* save, int l) const { return c(save, l) + bfh; }
  template <typename T> T* y(T* save, int l) const { return hprev(save, l) + bfh; }
};

// what a layer's reverse recurrence runs on: pre-activation gradients [B*F][4H], running cell cotangent and carry [B][H],
// W_hh^T (the lower layer's: max(H, in) x 4H, W_ih^T for the dX product afterwards)
struct BpttLayer { float* dgates; float* dc; float* carry; float* wt; };
struct TrainLstmWs {
  LstmWs st;               // h[l][2], c[l]
  float* bias[4];          // b_ih + b_hh
  BpttLayer lo;            // (layer after layer: every layer in its turn)
  float* dyl;              // [B*F][H] cotangent of the layer below's output
  float* dh[2];            // [B][H]
  float* atb;              // A^T B partials
  size_t atb_floats;
  float* ksplit;           // partial tiles of the K-split recurrent product, or nullptr
  // the reverse recurrences of two layers as a wavefront (bptt_wave): the upper layer's buffers next to the lower layer's,
  // three transposed weight matrices at once
  int wave = 0;            // 0 no, 1 matrix-vector kernel, 2 K-split tiles
  BpttLayer up{}; float* wt_ih_up = nullptr;
  float* rec = nullptr;    // partial tiles of both problems of a wavefront step (K-split form)
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
  w.st = carve_lstm_of(c, lstm_view(p), B, F);   // B > LSTM_PERSIST_B or not, the exchange buffer is unused here
  for (int l = 0; l < 4; ++l) w.bias[l] = l < L ? c.f((size_t)4 * H) : nullptr;
  w.lo.dgates = c.f((size_t)B * F * 4 * H);
  w.dyl = c.f((size_t)B * F * H);
  w.dh[0] = c.f((size_t)B * H); w.dh[1] = c.f((size_t)B * H); w.lo.carry = c.f((size_t)B * H); w.lo.dc = c.f((size_t)B * H);
  w.lo.wt = c.f((size_t)in_max * 4 * H);
  w.atb_floats = atb_workspace_floats_max(B * F, {{4 * H, p->input_size}, {4 * H, H}});   // dW_ih (layer 0 / above), dW_hh
  w.atb = c.f(w.atb_floats + 64);
  const size_t ksplit_floats = rec_ksplit_applicable(B, H, 4 * H) ? rec_ksplit_workspace_floats(B, H, 4 * H, 1) : 0;
  w.ksplit = ksplit_floats ? c.f(ksplit_floats) : nullptr;
  if (L == 2 && options().bptt_wave != 0 && (4 * H) % 256 == 0) {
    if (gemm_fewrows_applicable(B, H, 4 * H) && 4 * H <= 2048) w.wave = 1;
    else if (ksplit_floats && 8 * H / 256 <= 16) w.wave = 2;   // (not the pointer: null while sizes are counted)
  }
  if (w.wave) {
    w.up.dgates = c.f((size_t)B * F * 4 * H);
    w.up.carry = c.f((size_t)B * H); w.up.dc = c.f((size_t)B * H);
    w.up.wt = c.f((size_t)H * 4 * H); w.wt_ih_up = c.f((size_t)H * 4 * H);
    if (w.wave == 2) w.rec = c.f(rec_ksplit_workspace_floats(B, H, 8 * H, 2));
  }
  return w;
}

GemmProb gemm_prob(const float* A, int lda, const float* W, int ldw, float* C, int ldc, int M, int N, int K,
                   const float* resid, int ldr) {
  GemmProb g;
  g.A = A; g.lda = lda; g.W = W; g.ldw = ldw; g.C = C; g.ldc = ldc; g.M = M; g.N = N; g.K = K;
  g.scale = nullptr; g.shift = nullptr; g.resid = resid; g.ldr = ldr; g.act = 0; g.slope = 0.f;
  return g;
}
hipError_t gemm(const GemmProb& g, hipStream_t stream) {
  GemmBatch b;
  b.count = 1; b.p[0] = g;
  return launch_gemm(b, stream);
}
// a plain product + residual whose result feeds a cell: one unit of one K segment (C is not written)
RecBatch rec_batch_of(const GemmProb& g) {
  RecBatch rb;
  rb.count = 1;
  RecProb& q = rb.p[0];
  q.nseg = 1; q.seg[0] = RecSeg{g.A, g.lda, g.W, g.ldw, g.K};
  q.M = g.M; q.N = g.N; q.resid = g.resid; q.ldr = g.ldr;
  return rb;
}

// Back-propagation through time: the arguments of empose_lstm_train_bwd, the pieces both forms share, the two recurrences.
struct Bptt {
  const empose_lstm_params* p; int B, F, H; const float* x; int ldx; const int* seq_lengths; const float* c0;
  const float* save; LstmSave sv; const float* dy; float* dx; const empose_lstm_grads* grads; TrainLstmWs w;
  hipStream_t stream;
  size_t bh() const { return (size_t)B * H; }
  int in_k(int l) const { return l == 0 ? p->input_size : H; }
  // the cell of (layer l, step t): `dy_l` the cotangent of the layer's output sequence, `dh_in` that of step t + 1's product
  LstmCellBwdArgs cell_bwd_args(int l, int t, const BpttLayer& b, const float* dy_l, const float* dh_in) const {
    LstmCellBwdArgs ca;
    ca.gates = sv.gates(save, l); ca.c_all = sv.c(save, l); ca.c0 = c0 ? c0 + l * bh() : nullptr;
    ca.dy = dy_l; ca.ld_dy = H; ca.dh_in = dh_in; ca.dc = b.dc; ca.dgates = b.dgates; ca.dh_carry = b.carry;
    ca.seq_lengths = seq_lengths; ca.B = B; ca.F = F; ca.H = H; ca.t = t;
    return ca;
  }
  // the recurrent product dh_{t-1} = dG_t . W_hh + carry (the carry of step t is the residual)
  GemmProb rec_prob(const BpttLayer& b, int t, float* out) const {
    return gemm_prob(b.dgates + (size_t)t * 4 * H, F * 4 * H, b.wt, 4 * H, out, H, B, H, 4 * H, b.carry, H);
  }
  // the cotangents of a layer's initial state, where asked for: dh_{-1} = dG_0 . W_hh + carry, dc_{-1} = what the cell of
  // step 0 left in the running cell cotangent (b.wt still holds W_hh^T)
  int state_cotangents(int l, const BpttLayer& b) const {
    if (grads->d_h0[l]) HIP_CHECK(gemm(rec_prob(b, 0, grads->d_h0[l]), stream), "initial-state cotangent");
    if (grads->d_c0[l]) HIP_TRY(hipMemcpyAsync(grads->d_c0[l], b.dc, bh() * sizeof(float), hipMemcpyDeviceToDevice, stream));
    return EMPOSE_OK;
  }
  // the batched products of a layer over all steps: dW_ih + bias gradient, the b_hh copy, dW_hh
  int weight_grads(int l, const float* dgates) const {
    AtbArgs ab{};
    ab.A = dgates; ab.lda = 4 * H; ab.B = l == 0 ? x : sv.y(save, l - 1); ab.ldb = l == 0 ? ldx : H;
    ab.C = grads->w_ih[l]; ab.ldc = in_k(l); ab.bias = grads->b_ih[l]; ab.M = B * F; ab.N = 4 * H; ab.K = in_k(l);
    HIP_CHECK(launch_gemm_atb(ab, w.atb, w.atb_floats, stream), "dW_ih");
    HIP_TRY(hipMemcpyAsync(grads->b_hh[l], grads->b_ih[l], (size_t)4 * H * sizeof(float), hipMemcpyDeviceToDevice, stream));
    ab.B = sv.hprev(save, l); ab.ldb = H; ab.C = grads->w_hh[l]; ab.ldc = H; ab.bias = nullptr; ab.K = H;
    HIP_CHECK(launch_gemm_atb(ab, w.atb, w.atb_floats, stream), "dW_hh");
    return EMPOSE_OK;
  }
  // the cotangent of a layer's input sequence: dX = dG . W_ih (through w.lo.wt)
  int input_cotangent(int l, const float* dgates, float* dx_l) const {
    HIP_CHECK(launch_transpose(p->w_ih[l], in_k(l), w.lo.wt, 4 * H, 4 * H, in_k(l), stream), "transpose");
    HIP_CHECK(gemm(gemm_prob(dgates, 4 * H, w.lo.wt, 4 * H, dx_l, in_k(l), B * F, in_k(l), 4 * H, nullptr, 0), stream), "dX gemm");
    return EMPOSE_OK;
  }
  // Two layers as a wavefront: stage s runs the cell of (layer 1, step s) and of (layer 0, step s + 1).  Both need only
  // what stage s + 1 left: dh1_s = dG1_{s+1} . W_hh1, and dh0_{s+1} = dG0_{s+2} . W_hh0 + dG1_{s+1} . W_ih1 -- the
  // cotangent of layer 0's output, which the layer-after-layer form gets from one batched product over all steps
  // afterwards, is the second K segment of layer 0's recurrent product here.  F + 1 stages of one launch (or one launch
  // pair) instead of 2 F; the batched dX product of layer 1 disappears.
  int wavefront() const {
    const BpttLayer &lo = w.lo, &up = w.up;
    hipError_t e = launch_transpose(p->w_hh[1], H, up.wt, 4 * H, 4 * H, H, stream);
    if (e == hipSuccess) e = launch_transpose(p->w_ih[1], H, w.wt_ih_up, 4 * H, 4 * H, H, stream);
    if (e == hipSuccess) e = launch_transpose(p->w_hh[0], H, lo.wt, 4 * H, 4 * H, H, stream);
    if (e != hipSuccess) return fail(EMPOSE_EHIP, "transpose: %s", hipGetErrorString(e));
    HIP_TRY(hipMemsetAsync(lo.dc, 0, bh() * sizeof(float), stream));
    HIP_TRY(hipMemsetAsync(up.dc, 0, bh() * sizeof(float), stream));
    // stage F - 1: nothing flows into the last step of the top layer
    HIP_CHECK(launch_lstm_cell_bwd(cell_bwd_args(1, F - 1, up, dy, nullptr), stream), "lstm cell backward");
    for (int s = F - 2; s >= -1; --s) {
      RecBatch rb;
      LstmCellBwdArgs cells[2];
      rb.count = 0;
      if (s >= 0) {   // (layer 1, step s)
        RecProb& q = rb.p[rb.count];
        q.nseg = 1; q.seg[0] = RecSeg{up.dgates + (size_t)(s + 1) * 4 * H, F * 4 * H, up.wt, 4 * H, 4 * H};
        q.M = B; q.N = H; q.resid = up.carry; q.ldr = H;
        cells[rb.count++] = cell_bwd_args(1, s, up, dy, nullptr);
      }
      {               // (layer 0, step s + 1)
        const int t0 = s + 1;
        RecProb& q = rb.p[rb.count];
        q.nseg = 0;
        if (t0 + 1 <= F - 1) q.seg[q.nseg++] = RecSeg{lo.dgates + (size_t)(t0 + 1) * 4 * H, F * 4 * H, lo.wt, 4 * H, 4 * H};
        q.seg[q.nseg++] = RecSeg{up.dgates + (size_t)t0 * 4 * H, F * 4 * H, w.wt_ih_up, 4 * H, 4 * H};
        q.M = B; q.N = H; q.resid = t0 + 1 <= F - 1 ? lo.carry : nullptr; q.ldr = H;
        cells[rb.count++] = cell_bwd_args(0, t0, lo, nullptr, nullptr);
      }
      HIP_CHECK(w.wave == 2 ? launch_rec_ksplit(rb, cells, w.rec, stream) : launch_rec_fewrows(rb, cells, stream),
                "recurrent backward (wavefront)");
    }
    TRY(state_cotangents(0, lo));
    TRY(state_cotangents(1, up));
    TRY(weight_grads(1, up.dgates));
    TRY(weight_grads(0, lo.dgates));
    if (dx) TRY(input_cotangent(0, lo.dgates, dx));
    return EMPOSE_OK;
  }
  // Layer after layer, top down: a cell and a recurrent product per step, then the layer's batched products; the
  // cotangent of the layer below's output (w.dyl) is the layer's dX.
  int layer_after_layer() const {
    const BpttLayer& b = w.lo;
    const bool fewrows = !w.ksplit && gemm_fewrows_applicable(B, H, 4 * H);
    for (int l = p->num_layers - 1; l >= 0; --l) {
      const float* dy_l = l == p->num_layers - 1 ? dy : w.dyl;
      // W_hh^T for the recurrent product dh_{t-1} = dG_t . W_hh on the forward GEMM kernel
      HIP_CHECK(launch_transpose(p->w_hh[l], H, b.wt, 4 * H, 4 * H, H, stream), "transpose");
      HIP_TRY(hipMemsetAsync(b.dc, 0, bh() * sizeof(float), stream));
      const float* dh_in = nullptr;
      bool cell_done = false;   // the cell of step t already ran inside the previous step's reduce kernel
      for (int t = F - 1; t >= 0; --t) {
        if (!cell_done) HIP_CHECK(launch_lstm_cell_bwd(cell_bwd_args(l, t, b, dy_l, dh_in), stream), "lstm cell backward");
        if (t == 0) break;
        float* out = w.dh[t & 1];
        const GemmProb g = rec_prob(b, t, out);
        // a few hundred rows: K split over the workgroups (rec_ksplit_kernel), whose reduce kernel feeds dh straight into
        // the cell of step t - 1; the reference's batch: matrix-vector kernel, same fusion; else the GEMM and the cell
        cell_done = w.ksplit || fewrows;
        const LstmCellBwdArgs next = cell_bwd_args(l, t - 1, b, dy_l, nullptr);
        const hipError_t e = w.ksplit ? launch_rec_ksplit(rec_batch_of(g), &next, w.ksplit, stream)
                             : fewrows ? launch_gemm_fewrows_cell(g, next, stream) : gemm(g, stream);
        if (e != hipSuccess) return fail(EMPOSE_EHIP, "recurrent backward gemm: %s", hipGetErrorString(e));
        dh_in = out;
      }
      TRY(state_cotangents(l, b));
      TRY(weight_grads(l, b.dgates));
      float* dx_l = l > 0 ? w.dyl : dx;
      if (dx_l) TRY(input_cotangent(l, b.dgates, dx_l));
    }
    return EMPOSE_OK;
  }
};
}  // namespace

namespace empose {
namespace api {

LstmWs carve_lstm_of(Carver& c, const Lstm& r, int B, int F) {
  LstmWs w;
  const LstmPlan p = plan_lstm(r, B, F, false);   // (the buffers do not depend on the state)
  const int H = r.H, U = r.num_layers * r.dirs;
  // the state buffers of all units back to back: set_initial_state fills them at once
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
  // the hidden-state planes back to back too (run_x3_steps checks it before its one fill)
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
  // (api_internal.h; the count is only looked at here: clearing it here let the one call that happened to come next
  // swallow the report while the call that produced the NaNs returned OK)
  TRY(earlier_poll_timeouts());
  TRY(check_offsets_fit(B, F, ldx, 2 * r.H));
  return LstmRun{r, B, F, x, ldx, seq_lengths, h0, c0, y, h_n, c_n, ws, stream, plan_lstm(r, B, F, !h0 && !c0)}.run();
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
      if (dirs != 1 || r.hidden_size % 32 != 0) continue;
      for (int y = 0; y < LSTM_N_LAYOUTS; ++y) {
        TRY(pack_lstm_x3(allocs, (LstmLayout)y, w_ih[u], r.hidden_size, k_in, &out->w3[y].ih[u]));
        TRY(pack_lstm_x3(allocs, (LstmLayout)y, w_hh[u], r.hidden_size, r.hidden_size, &out->w3[y].hh[u]));
      }
      TRY(pack_lstm_pair16(allocs, l, w_ih[u], w_hh[u], r.hidden_size, k_in, out));
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

size_t empose_lstm_train_save_floats(int L, int B, int F, int H) { return LstmSave(B, F, H).floats(L); }

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
  const size_t bh = (size_t)B * H;
  const LstmSave sv(B, F, H);
  TRY(check_offsets_fit(B, F, ldx, 4 * H));
  Carver c(workspace);
  TrainLstmWs w = carve_train_lstm(c, p, B, F);
  LstmWaveArgs a = stacked_wave_args(L, p->input_size, H, p->w_ih, p->w_hh, w.bias, w.st, B, F, x, ldx, seq_lengths, y);
  for (int l = 0; l < L; ++l) {
    LstmUnitArgs& ua = a.unit[l];
    if (l < L - 1) { ua.y = sv.y(save, l); ua.y_ld = H; }
    ua.sv_gates = sv.gates(save, l); ua.sv_c = sv.c(save, l); ua.sv_hprev = sv.hprev(save, l);
    HIP_CHECK(launch_add2(p->b_ih[l], p->b_hh[l], w.bias[l], 4 * H, stream), "bias sum");
    // the initial state, and its hidden part as slot t = 0 of the saved incoming hidden states
    HIP_TRY(init_state(ua.h[0], h0 ? h0 + l * bh : nullptr, bh, stream));
    if (h0)
      HIP_TRY(hipMemcpy2DAsync(ua.sv_hprev, (size_t)F * H * sizeof(float), h0 + l * bh, (size_t)H * sizeof(float),
                               (size_t)H * sizeof(float), B, hipMemcpyDeviceToDevice, stream));
    else HIP_TRY(hipMemset2DAsync(ua.sv_hprev, (size_t)F * H * sizeof(float), 0, (size_t)H * sizeof(float), B, stream));
    HIP_TRY(init_state(ua.c, c0 ? c0 + l * bh : nullptr, bh, stream));
  }
  // Small batches (the reference's training batch of 12 windows): the whole sequence in one cooperative launch with the
  // weights in registers, as in inference -- the step-by-step kernel streams 13.8 MB of weights per wavefront step.
  // (the plan of the fp32 kernels, as in inference; lstm_seq_kernel saves nothing for the reverse pass)
  const LstmPlan plan = plan_lstm_f32(stacked_shape(L, p->input_size, H, B, F));
  bool done = false;
  if (plan.n_coop > 0 && plan.coop[0] == LstmCoop::persist)
    HIP_CHECK(launch_lstm_persist(a, w.st.xch, stream, &done), "lstm sequence kernel");
  if (!done) TRY(wave_steps(a, plan, F + L - 1, false, stream));
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
  for (int l = 0; l < p->num_layers; ++l)
    if (!grads->w_ih[l] || !grads->w_hh[l] || !grads->b_ih[l] || !grads->b_hh[l])
      return fail(EMPOSE_EINVAL, "null gradient output");
  Carver c(workspace);
  const Bptt bptt{p, B, F, p->hidden_size, x, ldx, seq_lengths, c0, save, LstmSave(B, F, p->hidden_size), dy, dx, grads,
                  carve_train_lstm(c, p, B, F), static_cast<hipStream_t>(stream_)};
  return bptt.w.wave ? bptt.wavefront() : bptt.layer_after_layer();
}

}  // extern "C"
