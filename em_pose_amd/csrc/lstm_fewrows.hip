// fp32 LSTM steps of up to 16 rows: lstm_small_kernel (a wave per hidden unit), lstm_fewrows_kernel (a workgroup per one or
// two hidden units, all threads split K) and their launchers (lstm_wave.h: the wavefront, units and segments).
#include "lstm_kernels.h"
#include "lstm_wave.h"

namespace empose {

// ---------------------------------------------------------------------------------------------------------------
// Small batches (the one-recording-at-a-time driver: B = 1, F = 256): a step is a matrix-VECTOR product, bound by
// streaming the weights (13.8 MB per wavefront step for 2 x 512), not by arithmetic; the matrix-core kernel above would
// spend a 64-row tile on one row.  Here a wave owns one hidden unit of one layer: its lanes split K, read the four gate
// rows of the unit as coalesced 16-byte pieces, and reduce with DPP shuffles; 4 units per block, so 2 x 128 blocks
// keep every CU streaming.  Same operands (host-built segment table), same state handling as lstm_chain_kernel.
// ---------------------------------------------------------------------------------------------------------------
template <int MB>   // rows handled, B <= MB
__global__ __launch_bounds__(256) void lstm_small_kernel(LstmWaveArgs a) {
  const int n_seg = a.z_cnt[blockIdx.y];
  if (n_seg == 0) return;
  const int seg_beg = a.z_beg[blockIdx.y];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int H = a.H, B = a.B, F = a.F;
  const int unit = blockIdx.x * 4 + wave;
  if (unit >= H) return;   // no barrier below: whole waves may leave
  const LstmUnitArgs& L = a.unit[a.seg[seg_beg].unit];
  const int t = a.seg[seg_beg].k;
  const int* __restrict__ lens = a.seq_lengths;

  float acc[4][MB];
#pragma unroll
  for (int g = 0; g < 4; ++g)
#pragma unroll
    for (int b = 0; b < MB; ++b) acc[g][b] = 0.f;

  for (int s = 0; s < 2; ++s) {
    const LstmSeg sg = a.seg[seg_beg + s];
    const float* __restrict__ wbase = sg.w + (size_t)unit * sg.ldw;
    for (int k4 = lane * 4; k4 < sg.K; k4 += 256) {
      f32x4 w[4];
#pragma unroll
      for (int g = 0; g < 4; ++g) w[g] = *reinterpret_cast<const f32x4*>(wbase + (size_t)g * H * sg.ldw + k4);
#pragma unroll
      for (int b = 0; b < MB; ++b) {
        if (b < B) {   // uniform; a predicate, not a `break`: the loop then unrolls completely and acc[][] stays in registers
          const int tr = (lens ? lens[b] : F) - 1 - sg.k;
          const float* row = sg.a + (size_t)b * sg.lda + (size_t)(tr > 0 ? tr : 0) * sg.tstride;
          const f32x4 v = *reinterpret_cast<const f32x4*>(row + k4);
#pragma unroll
          for (int g = 0; g < 4; ++g) acc[g][b] = dot4_acc(acc[g][b], w[g], v);
        }
      }
    }
  }
  // wave-wide sums (every lane ends up with all of them)
#pragma unroll
  for (int g = 0; g < 4; ++g)
#pragma unroll
    for (int b = 0; b < MB; ++b) {
      if (b < B) {
        float v = acc[g][b];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
        acc[g][b] = v;
      }
    }
  // lane b finishes row b
  float gi = 0.f, gf = 0.f, gg = 0.f, go = 0.f;
#pragma unroll
  for (int b = 0; b < MB; ++b)
    if (lane == b) { gi = acc[0][b]; gf = acc[1][b]; gg = acc[2][b]; go = acc[3][b]; }
  if (lane < B) {
    const int row = lane;
    const bool rev = L.reverse != 0;
    const float* __restrict__ bias = L.bias;
    const float* __restrict__ h_prev = L.h[t & 1];
    float* __restrict__ h_next = L.h[(t + 1) & 1];
    float* __restrict__ cst = L.c;
    const size_t hc = (size_t)row * H + unit;
    const int len = lens ? lens[row] : F;
    const bool live = t < len;
    const int t_out = (rev && live) ? len - 1 - t : t;   // a finished reverse row zero-fills the padded slot t
    float h_new = 0.f, c_old = 0.f, c_keep = 0.f, h_carry;
    if (live) {   // (these expressions are kept as they are: lstm_persist_kernel must give the same bits)
      c_old = cst[hc];
      const float c_new = fast_sigmoid(gf + bias[H + unit]) * c_old + fast_sigmoid(gi + bias[unit]) * fast_tanh(gg + bias[2 * H + unit]);
      h_new = fast_sigmoid(go + bias[3 * H + unit]) * fast_tanh(c_new);
      cst[hc] = c_new;
      h_next[hc] = h_carry = h_new;
      c_keep = c_new;
    } else {
      h_next[hc] = h_carry = h_prev[hc];
      if (L.sv_gates) c_keep = cst[hc];
    }
    if (L.y) L.y[((size_t)row * F + t_out) * L.y_ld + L.y_col + unit] = h_new;
    if (L.sv_gates) {   // training forward: what back-propagation through time reads
      const size_t rt = (size_t)row * F + t;
      float* sg = L.sv_gates + rt * 4 * H + unit;
      sg[0] = fast_sigmoid(gi + bias[unit]); sg[H] = fast_sigmoid(gf + bias[H + unit]);
      sg[2 * H] = fast_tanh(gg + bias[2 * H + unit]); sg[3 * H] = fast_sigmoid(go + bias[3 * H + unit]);
      L.sv_c[rt * H + unit] = c_keep;
      if (t + 1 < F) L.sv_hprev[(rt + 1) * H + unit] = h_carry;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------
// A few rows (4 .. 16: the reference's training batch of 12 windows, the batched evaluation driver's chunk of recordings),
// round 5.  lstm_small_kernel above costs 2.2 us per row and step (34 us per step at 12 rows: a row's 16-byte pieces are
// loaded inside the k loop, 6 lane exchanges per gate sum); the whole-sequence kernel below polls B x H exchange words per
// layer and step in every workgroup (16 us per step at 12 rows).  Here a step is one launch in which a workgroup owns TWO
// hidden units (8 gate columns) and ALL its 256 threads split the unit's K = [input | recurrent] (1024 floats at 2 x 512:
// one 16-byte piece per thread): a thread loads its piece of the B rows and of the 8 weight rows once, 8 B accumulators;
// the sums over a wave's lanes are a reduce-scatter (lane_reduce.h), the four waves' sums meet in LDS and are added in
// wave order; thread (unit, row) applies the cell.  Same state handling and saves as lstm_small_kernel; another summation
// order (option "lstm_fewrows" = 0 selects the kernels above, whose bits the whole-sequence kernel shares).
// ---------------------------------------------------------------------------------------------------------------
template <int MB, int NU>   // rows handled (B <= MB), hidden units per workgroup
__global__ __launch_bounds__(256) void lstm_fewrows_kernel(LstmWaveArgs a) {
  constexpr int C = 4 * NU, NV = C * MB;
  __shared__ float wsum[4][NV + 4];
  const int n_seg = a.z_cnt[blockIdx.y];
  if (n_seg == 0) return;
  const int seg_beg = a.z_beg[blockIdx.y];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int H = a.H, B = a.B, F = a.F;
  const int u0 = blockIdx.x * NU;
  const LstmUnitArgs& L = a.unit[a.seg[seg_beg].unit];
  const int t = a.seg[seg_beg].k;
  const int* __restrict__ lens = a.seq_lengths;
  // thread (unit f_u, row f_m) finishes a cell: its state and bias are fetched now, under the product
  const int f_u = tid / MB, f_m = tid - f_u * MB;
  const bool fin = tid < NU * MB && f_m < B && u0 + f_u < H;
  const int unit = u0 + (f_u < NU ? f_u : 0);
  float e_bias[4] = {0.f, 0.f, 0.f, 0.f}, e_c = 0.f, e_hp = 0.f;
  int e_len = F;
  if (fin) {
    const size_t hc = (size_t)f_m * H + unit;
#pragma unroll
    for (int q = 0; q < 4; ++q) e_bias[q] = L.bias[q * H + unit];
    e_c = L.c[hc];
    e_hp = L.h[t & 1][hc];
    e_len = lens ? lens[f_m] : F;
  }

  float v[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) v[i] = 0.f;
  {
    const LstmSeg s0 = a.seg[seg_beg], s1 = a.seg[seg_beg + 1];
    const int n0 = s0.K >> 2, n1 = n_seg > 1 ? s1.K >> 2 : 0;       // 16-byte pieces of the two operand segments
    for (int p = tid; p < n0 + n1; p += 256) {
      const bool first = p < n0;
      const int k4 = (first ? p : p - n0) * 4;
      const float* __restrict__ wb = (first ? s0.w : s1.w) + k4;
      const float* __restrict__ ab = (first ? s0.a : s1.a) + k4;
      const int ldw = first ? s0.ldw : s1.ldw, lda = first ? s0.lda : s1.lda;
      const int tstride = first ? s0.tstride : s1.tstride, sk = first ? s0.k : s1.k;
      f32x4 w[C], x[MB];
#pragma unroll
      for (int ul = 0; ul < NU; ++ul)
#pragma unroll
        for (int q = 0; q < 4; ++q)
          w[ul * 4 + q] = *reinterpret_cast<const f32x4*>(wb + (size_t)(q * H + min(u0 + ul, H - 1)) * ldw);
#pragma unroll
      for (int m = 0; m < MB; ++m) {
        const int mr = m < B ? m : B - 1;
        const int tr = (lens ? lens[mr] : F) - 1 - sk;
        x[m] = *reinterpret_cast<const f32x4*>(ab + (size_t)mr * lda + (size_t)(tr > 0 ? tr : 0) * tstride);
      }
#pragma unroll
      for (int c = 0; c < C; ++c)
#pragma unroll
        for (int m = 0; m < MB; ++m) v[c * MB + m] = dot4_acc(v[c * MB + m], w[c], x[m]);
    }
  }
  int base = 0, count = 0;
  LaneReduceScatter<NV, 32, NV>::run(v, lane, base, count);
#pragma unroll
  for (int i = 0; i < 4; ++i)      // (count <= 3 for the instantiated sizes; lanes that hold the same sums write the same)
    if (i < count) wsum[wave][base + i] = v[i];
  __syncthreads();
  if (!fin) return;
  float gs[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int o = (f_u * 4 + q) * MB + f_m;
    gs[q] = ((wsum[0][o] + wsum[1][o]) + wsum[2][o]) + wsum[3][o];
  }
  const int row = f_m;
  const bool rev = L.reverse != 0;
  const size_t hc = (size_t)row * H + unit;
  const bool live = t < e_len;
  const int t_out = (rev && live) ? e_len - 1 - t : t;   // a finished reverse row zero-fills the padded slot t
  const float g_i = fast_sigmoid(gs[0] + e_bias[0]), g_f = fast_sigmoid(gs[1] + e_bias[1]);
  const float g_g = fast_tanh(gs[2] + e_bias[2]), g_o = fast_sigmoid(gs[3] + e_bias[3]);
  const float c_new = g_f * e_c + g_i * g_g;
  const float h_new = g_o * fast_tanh(c_new);
  if (live) L.c[hc] = c_new;
  L.h[(t + 1) & 1][hc] = live ? h_new : e_hp;
  if (L.y) L.y[((size_t)row * F + t_out) * L.y_ld + L.y_col + unit] = live ? h_new : 0.f;
  if (L.sv_gates) {   // training forward: what back-propagation through time reads
    const size_t rt = (size_t)row * F + t;
    float* sg = L.sv_gates + rt * 4 * H + unit;
    sg[0] = g_i; sg[H] = g_f; sg[2 * H] = g_g; sg[3 * H] = g_o;
    L.sv_c[rt * H + unit] = live ? c_new : e_c;
    if (t + 1 < F) L.sv_hprev[(rt + 1) * H + unit] = live ? h_new : e_hp;
  }
}

constexpr int LSTM_SMALL_ROWS = 16;   // the largest MB either kernel is built for

bool lstm_small_shape_ok(int B) { return B <= LSTM_SMALL_ROWS; }
// 16-byte pieces of every segment, two units per workgroup
bool lstm_fewrows_shape_ok(int B, int H, int n_units, const int* in_k) {
  bool ok = B <= LSTM_SMALL_ROWS && H % 4 == 0;
  for (int u = 0; u < n_units; ++u) ok = ok && in_k[u] % 4 == 0;
  return ok;
}

// One step launch each; the caller has built the segment table with one unit per y slice (lstm_build_chain(a, 1)).
hipError_t launch_lstm_small(const LstmWaveArgs& a, hipStream_t stream) {
  if (!lstm_small_shape_ok(a.B)) return hipErrorInvalidValue;
  dim3 grid((a.H + 3) / 4, a.n_units);
  if (a.B <= 4) hipLaunchKernelGGL(lstm_small_kernel<4>, grid, dim3(256), 0, stream, a);
  else hipLaunchKernelGGL(lstm_small_kernel<LSTM_SMALL_ROWS>, grid, dim3(256), 0, stream, a);
  return hipGetLastError();
}
hipError_t launch_lstm_fewrows(const LstmWaveArgs& a, hipStream_t stream) {
  int in_k[4];
  for (int u = 0; u < a.n_units; ++u) in_k[u] = a.unit[u].in_k;
  if (!lstm_fewrows_shape_ok(a.B, a.H, a.n_units, in_k)) return hipErrorInvalidValue;
  if (a.B <= 4) hipLaunchKernelGGL((lstm_fewrows_kernel<4, 2>), dim3(a.H / 2, a.n_units), dim3(256), 0, stream, a);
  else if (a.B <= 8) hipLaunchKernelGGL((lstm_fewrows_kernel<8, 2>), dim3(a.H / 2, a.n_units), dim3(256), 0, stream, a);
  else if (a.B <= 12) hipLaunchKernelGGL((lstm_fewrows_kernel<12, 2>), dim3(a.H / 2, a.n_units), dim3(256), 0, stream, a);
  else hipLaunchKernelGGL((lstm_fewrows_kernel<16, 1>), dim3(a.H, a.n_units), dim3(256), 0, stream, a);
  return hipGetLastError();
}

}  // namespace empose
