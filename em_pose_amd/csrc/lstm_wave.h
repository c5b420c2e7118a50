// LSTM time steps on the fp32 matrix cores (reference nn/layers.py:133-157: nn.LSTM, gate order i,f,g,o, stacked
// layers, optionally bidirectional, pack_padded_sequence semantics).  What the fp32 kernel files share -- one file per
// kernel family: lstm_chain.hip, lstm_seq.hip, lstm_mid.hip, lstm_fewrows.hip, lstm_persist.hip; which of them a call takes
// is decided by plan_lstm (api_lstm.hip), never by a launcher.
//
// One launch advances the whole layer stack by one "wavefront" step s: layer l processes time step t = s - l, so
// all layers run concurrently (layer l at step t only needs layer l-1 at step t, produced by the previous launch,
// and its own state after step t-1).  For every (layer, step) the gate pre-activations are
//     gates = in_t . W_ih^T + h_{t-1} . W_hh^T + (b_ih + b_hh)
// i.e. one GEMM whose K dimension is the concatenation of two operand "segments"; the cell non-linearities are the
// epilogue.  Nothing but h, c and the last layer's output ever touches memory (no gate buffer, no separate input
// projection).
//
// A "unit" is one (layer, direction). Units either read a stored input sequence (layer 0, and the layers of a
// bidirectional stack, whose input is the concatenated output sequence of the previous layer) or the hidden state
// another unit produced in the previous launch (uni-directional stacks: the wavefront above).  A reverse unit visits, at
// its step k, time len_b-1-k of every row b (packed-sequence semantics for ragged batches).
//
// Tiling: v_mfma_f32_16x16x4_f32.  A wave owns 32 batch rows x 16 hidden units and keeps 2 x 4 accumulators
// (row half x gate), so i/f/g/o of one (row, unit) sit in the same lane; a block is 2x2 waves = 64 rows x 32 units.
// Since a dot product does not care about the order of k, each 16-lane group takes 4 consecutive k of a 16-wide chunk
// so that one ds_read_b128 feeds four MFMAs.
#pragma once
#include <type_traits>

#include "device_common.h"
#include "lane_reduce.h"
#include "lstm_kernels.h"

namespace empose {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(1))) f32x4* gvec_t;
typedef const __attribute__((address_space(1))) char* gbyte_t;

// tiles of lstm_chain_kernel / lstm_seq_kernel: 64 rows x 32 units, 64-wide K tiles, two stages in LDS
namespace lc {
constexpr int BM = 64, BU = 32, BK = 64;
constexpr int ROWS = BM + 4 * BU;
constexpr int STAGE = ROWS * BK;
constexpr size_t LDS_BYTES = 2 * (size_t)STAGE * sizeof(float);
}  // namespace lc

// tiles of lstm_mid_kernel: 32 rows x 16 units
namespace lm {
constexpr int BM = 32, BU = 16, BK = 64;
constexpr int ROWS = BM + 4 * BU;          // 96 staged rows per K tile
constexpr int STAGE = ROWS * BK;
constexpr size_t LDS_BYTES = 2 * (size_t)STAGE * sizeof(float);   // 48 KB; the reduction reuses it (4 x 32 x 64 floats)
}  // namespace lm

#ifdef EMPOSE_LSTM_TRACE   // dev lab only (one translation unit): per-phase shader-clock stamps of block (0,0,0)
__device__ long long g_lstm_trace[128];
#define LSTM_STAMP(i) \
  if (threadIdx.x == 0 && blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0) g_lstm_trace[(i)] = clock64();
#else
#define LSTM_STAMP(i)
#endif

// acc + w . v over a lane's four k, in one fixed order (explicit FMAs: lstm_small_kernel, lstm_fewrows_kernel and
// lstm_persist_kernel share it, the first and the last give the same bits)
__device__ __forceinline__ float dot4_acc(float acc, const f32x4& w, const f32x4& v) {
  return __builtin_fmaf(w[3], v[3], __builtin_fmaf(w[2], v[2], __builtin_fmaf(w[1], v[1], __builtin_fmaf(w[0], v[0], acc))));
}

// Segment table of one step launch: two segments per active unit, grouped by blockIdx.z (blockIdx.y of the few-row
// kernels).  Host side: the step loop of api_lstm.hip builds it with the plan's units per workgroup before every launch.
inline void lstm_build_chain(LstmWaveArgs& a, int units_per_block) {
  int n = 0, z = 0;
  for (int u0 = 0; u0 < a.n_units; u0 += units_per_block, ++z) {
    a.z_beg[z] = n;
    for (int u = u0; u < u0 + units_per_block && u < a.n_units; ++u) {
      const LstmUnitArgs& L = a.unit[u];
      const int t = a.s - L.t_offset;
      if (t < 0 || t >= a.F) continue;   // idle while the wavefront ramps up or down
      for (int s = 0; s < 2; ++s) {
        LstmSeg d;
        d.k = t; d.tstride = 0; d.unit = u; d.pad = 0;
        if (s == 0) {
          if (L.in_from < 0) {
            d.lda = a.F * L.in_ld;
            if (L.reverse) { d.a = L.in_seq; d.tstride = L.in_ld; }
            else d.a = L.in_seq + (size_t)t * L.in_ld;
          } else {
            d.a = a.unit[L.in_from].h[(t + 1) & 1]; d.lda = a.H;
          }
          d.w = L.w_ih; d.ldw = L.in_k; d.K = L.in_k;
        } else {
          d.a = L.h[t & 1]; d.lda = a.H; d.w = L.w_hh; d.ldw = a.H; d.K = a.H;
        }
        d.ntiles = (d.K + lc::BK - 1) / lc::BK;
        a.seg[n++] = d;
      }
    }
    a.z_cnt[z] = n - a.z_beg[z];
  }
  for (; z < 4; ++z) { a.z_beg[z] = 0; a.z_cnt[z] = 0; }
}

// The whole-sequence kernels cover the stacked uni-directional wavefront only: unit u is layer u, fed by layer u - 1.
inline bool lstm_is_stacked_wavefront(const LstmWaveArgs& w) {
  for (int u = 0; u < w.n_units; ++u) {
    const LstmUnitArgs& U = w.unit[u];
    if (U.reverse || U.t_offset != u || (u == 0 ? U.in_from >= 0 : U.in_from != u - 1)) return false;
  }
  return true;
}

}  // namespace empose
