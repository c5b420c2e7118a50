// fp32 LSTM step of large batches: lstm_chain_kernel and its launcher (lstm_wave.h: the wavefront, units and segments).
#include "launch.h"
#include "lstm_kernels.h"
#include "lstm_wave.h"

namespace empose {

// ---------------------------------------------------------------------------------------------------------------
// The wavefront kernel.
//
// A block owns one (64 batch rows) x (32 hidden units x 4 gates) tile and walks through a CHAIN of units one after the
// other -- for the stacked wavefront: layer 0 (K = input + H) then layer 1 (K = 2H) -- so every block does the same
// amount of work whatever the layers' K, and the 256 blocks of B = 1024, H = 512 are one block per CU.  The K tiles of
// the whole chain form one flat stream through a double-buffered LDS (2 x 48 KB, 64-wide K tiles, unpadded rows with
// the 16-byte chunks XOR-swizzled by row so that the ds_read_b128 lane groups of the 16x16x4 operand layout are
// conflict-free), one barrier per K tile, global loads two tiles ahead, and the instruction interleaving pinned with
// sched_group_barrier: with a single wave per SIMD nothing else hides a stall.
//   chunk 0 (k 0..15) : 32 MFMAs | fragment reads of chunk 1 | LDS writes of tile j+1 (fetched during tile j-1)
//   chunk 1           : 32 MFMAs | fragment reads of chunk 2 | global loads of tile j+2
//   chunk 2           : 32 MFMAs | fragment reads of chunk 3
//   barrier
//   chunk 3           : 32 MFMAs | fragment reads of chunk 0 of tile j+1
// The cell non-linearities run when the stream leaves a unit.
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void lstm_chain_kernel(LstmWaveArgs a) {
  using namespace lc;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  LSTM_STAMP(0)
  const int H = a.H, B = a.B, F = a.F;
  const int j0 = blockIdx.x * BU, m0 = blockIdx.y * BM;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wrow = wave >> 1, wcol = wave & 1;
  const int l15 = lane & 15, lq = lane >> 4;
  const int seg_beg = a.z_beg[blockIdx.z], n_seg = a.z_cnt[blockIdx.z];
  if (n_seg == 0) return;

  // ---- per-thread constants
  const int lr = tid >> 4, c16 = tid & 15;                 // global side: row lr + 16 i, 16-byte chunk c16 of the K tile
  int a_row[4], a_len[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = m0 + lr + 16 * i;
    a_row[i] = r < B ? r : B - 1;
    a_len[i] = a.seq_lengths ? a.seq_lengths[a_row[i]] : F;
  }
  int w_row[8];                                            // gate * H + unit of the thread's 8 weight rows
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int wr = lr + 16 * i, un = j0 + (wr & 31);
    w_row[i] = (wr >> 5) * H + (un < H ? un : H - 1);
  }
  const int wr_ofs = lr * BK + ((c16 ^ (lr & 15)) << 2);   // LDS write offset of piece 0 (floats); piece i: + 16 i rows
  const int a_rd = (wrow * 32 + l15) * BK;                 // fragment rows (floats); row tile i: + 16 rows
  const int b_rd = (BM + wcol * 16 + l15) * BK;            // gate g: + 32 rows
  int sw[4];                                               // swizzled chunk offset of k-chunk ch for this lane
#pragma unroll
  for (int ch = 0; ch < 4; ++ch) sw[ch] = ((((ch << 2) ^ (l15 & 12)) | (lq ^ (l15 & 3))) << 2);

  f32x4 g[12];
  bool g_ok = true;
  f32x4 fa[2][2], fb[2][4];
  f32x4 acc[2][4];

  // ---- the load side of the tile stream: current segment (scalar registers), the thread's byte offsets into its two
  // operands (recomputed when the stream enters a segment) and the k tile within the segment
  LstmSeg ld = a.seg[seg_beg];
  int ld_seg = 0, ld_kt = 0;
  unsigned a_off[4], w_off[8];
  auto seg_offsets = [&]() {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int tr = a_len[i] - 1 - ld.k;
      a_off[i] = (unsigned)(((long)a_row[i] * ld.lda + (long)(tr > 0 ? tr : 0) * ld.tstride + c16 * 4) * 4);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) w_off[i] = (unsigned)(((long)w_row[i] * ld.ldw + c16 * 4) * 4);
  };
  seg_offsets();
  auto gload = [&]() -> bool {   // fetch the tile under the load cursor; returns whether it is ragged
    g_ok = ld_kt * BK + c16 * 4 < ld.K;
    const unsigned back = g_ok ? 0u : (unsigned)(c16 * 16);   // lanes past K re-read chunk 0 of the tile; zeroed later
    gbyte_t pa = (gbyte_t)(ld.a + ld_kt * BK);
    gbyte_t pw = (gbyte_t)(ld.w + ld_kt * BK);
#pragma unroll
    for (int i = 0; i < 4; ++i) g[i] = *(gvec_t)(pa + (a_off[i] - back));
#pragma unroll
    for (int i = 0; i < 8; ++i) g[4 + i] = *(gvec_t)(pw + (w_off[i] - back));
    return (ld_kt + 1) * BK > ld.K;
  };
  auto ld_advance = [&]() {      // uniform; past the end of the stream it parks on a valid tile that is never used
    if (++ld_kt == ld.ntiles) {
      ld_kt = 0;
      if (ld_seg + 1 < n_seg) { ++ld_seg; ld = a.seg[seg_beg + ld_seg]; seg_offsets(); }
    }
  };
  auto gzero = [&]() {
#pragma unroll
    for (int i = 0; i < 12; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) g[i][e] = g_ok ? g[i][e] : 0.f;
  };
  auto lwrite = [&](float* st) {
#pragma unroll
    for (int i = 0; i < 4; ++i) *reinterpret_cast<f32x4*>(st + wr_ofs + i * 16 * BK) = g[i];
#pragma unroll
    for (int i = 0; i < 8; ++i) *reinterpret_cast<f32x4*>(st + BM * BK + wr_ofs + i * 16 * BK) = g[4 + i];
  };
  auto fread = [&](const float* st, int ch, f32x4 (&fa_)[2], f32x4 (&fb_)[4]) {
#pragma unroll
    for (int i = 0; i < 2; ++i) fa_[i] = *reinterpret_cast<const f32x4*>(st + a_rd + i * 16 * BK + sw[ch]);
#pragma unroll
    for (int q = 0; q < 4; ++q) fb_[q] = *reinterpret_cast<const f32x4*>(st + b_rd + q * 32 * BK + sw[ch]);
  };
  auto mma = [&](const f32x4 (&fa_)[2], const f32x4 (&fb_)[4]) {
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q)
          acc[i][q] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa_[i][e], fb_[q][e], acc[i][q], 0, 0, 0);
  };
  // Cell non-linearities of a finished unit; C/D layout: col = lane & 15, row = 4 * (lane >> 4) + r.  What they read
  // besides the accumulators (bias, old cell state, lengths, old hidden state of rows past their length) is fetched
  // when the stream ENTERS the unit, so the finish itself is arithmetic and stores only.  Nobody else touches these
  // (row, unit) elements during the launch.
  const int e_unit = j0 + wcol * 16 + l15;
  const int e_unit_c = e_unit < H ? e_unit : H - 1;
  float e_bias[4], e_c[8], e_hp[8];
  int e_len[8];
  auto enter_unit = [&](int u) {
    const LstmUnitArgs& L = a.unit[u];
    const int t = a.s - L.t_offset;
    const float* __restrict__ bias = L.bias;
    const float* __restrict__ h_prev = L.h[t & 1];
    const float* __restrict__ cst = L.c;
    const int* __restrict__ lens = a.seq_lengths;
#pragma unroll
    for (int q = 0; q < 4; ++q) e_bias[q] = bias[q * H + e_unit_c];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int row = m0 + wrow * 32 + (e >> 2) * 16 + lq * 4 + (e & 3);
      const int rc = row < B ? row : B - 1;
      const size_t hc = (size_t)rc * H + e_unit_c;
      e_c[e] = cst[hc];
      e_len[e] = lens ? lens[rc] : F;
      e_hp[e] = lens ? h_prev[hc] : 0.f;   // only rows past their length carry the old state over
    }
  };
  auto finish_unit = [&](int u) {
    const LstmUnitArgs& L = a.unit[u];
    const int t = a.s - L.t_offset;
    const bool rev = L.reverse != 0;
    if (e_unit >= H) return;
    float* __restrict__ h_next = L.h[(t + 1) & 1];
    float* __restrict__ cst = L.c;
    float* __restrict__ yout = L.y;
    const long y_ld = L.y_ld, y_col = L.y_col;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int i = e >> 2, r = e & 3;
      const int row = m0 + wrow * 32 + i * 16 + lq * 4 + r;
      if (row >= B) continue;
      const size_t hc = (size_t)row * H + e_unit;
      const bool live = t < e_len[e];
      const int t_out = (rev && live) ? e_len[e] - 1 - t : t;   // a finished reverse row zero-fills the padded slot t
      const float g_i = fast_sigmoid(acc[i][0][r] + e_bias[0]), g_f = fast_sigmoid(acc[i][1][r] + e_bias[1]);
      const float g_g = fast_tanh(acc[i][2][r] + e_bias[2]), g_o = fast_sigmoid(acc[i][3][r] + e_bias[3]);
      const float c_new = g_f * e_c[e] + g_i * g_g;
      const float h_new = g_o * fast_tanh(c_new);
      if (live) cst[hc] = c_new;
      h_next[hc] = live ? h_new : e_hp[e];
      if (yout) yout[((size_t)row * F + t_out) * y_ld + y_col + e_unit] = live ? h_new : 0.f;
      if (L.sv_gates) {   // training forward: what back-propagation through time reads
        const size_t rt = (size_t)row * F + t;
        float* sg = L.sv_gates + rt * 4 * H + e_unit;
        sg[0] = g_i; sg[H] = g_f; sg[2 * H] = g_g; sg[3 * H] = g_o;
        L.sv_c[rt * H + e_unit] = live ? c_new : e_c[e];
        if (t + 1 < F) L.sv_hprev[(rt + 1) * H + e_unit] = live ? h_new : e_hp[e];
      }
    }
  };

  LSTM_STAMP(1)
  // ---- prologue: tile 0 -> stage 0, tile 1 in flight
  bool ragged = gload();
  if (ragged) gzero();
  lwrite(lds);
  ld_advance();
  ragged = gload();
  ld_advance();
  __syncthreads();
  fread(lds, 0, fa[0], fb[0]);
  LSTM_STAMP(2)
  int stamp = 3;
  (void)stamp;

  int parity = 0;
  for (int us = 0; us < n_seg; us += 2) {   // one unit = two consecutive segments
    const int unit_tiles = a.seg[seg_beg + us].ntiles + a.seg[seg_beg + us + 1].ntiles;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[i][q] = f32x4{0.f, 0.f, 0.f, 0.f};
    enter_unit(a.seg[seg_beg + us].unit);
    for (int j = 0; j < unit_tiles; ++j) {
      const float* cur = lds + parity * STAGE;
      float* nxt = lds + (parity ^ 1) * STAGE;
      parity ^= 1;
      if (ragged) gzero();     // uniform branch; the registers hold the next tile of the stream
      // ---- chunk 0
      fread(cur, 1, fa[1], fb[1]);
      lwrite(nxt);
      mma(fa[0], fb[0]);
#pragma unroll
      for (int q = 0; q < 6; ++q) { SGB(SG_MFMA, 1); SGB(SG_DS_RD, 1); }
#pragma unroll
      for (int q = 0; q < 12; ++q) { SGB(SG_MFMA, 2); SGB(SG_DS_WR, 1); }
      SGB(SG_MFMA, 2);
      // ---- chunk 1
      fread(cur, 2, fa[0], fb[0]);
      ragged = gload();
      mma(fa[1], fb[1]);
#pragma unroll
      for (int q = 0; q < 6; ++q) { SGB(SG_MFMA, 1); SGB(SG_DS_RD, 1); }
#pragma unroll
      for (int q = 0; q < 12; ++q) { SGB(SG_MFMA, 2); SGB(SG_VMEM_RD, 1); }
      SGB(SG_MFMA, 2);
      // ---- chunk 2
      fread(cur, 3, fa[1], fb[1]);
      mma(fa[0], fb[0]);
#pragma unroll
      for (int q = 0; q < 6; ++q) { SGB(SG_MFMA, 2); SGB(SG_DS_RD, 1); }
      SGB(SG_MFMA, 20);
      __syncthreads();
      // ---- chunk 3
      fread(nxt, 0, fa[0], fb[0]);
      mma(fa[1], fb[1]);
#pragma unroll
      for (int q = 0; q < 6; ++q) { SGB(SG_MFMA, 2); SGB(SG_DS_RD, 1); }
      SGB(SG_MFMA, 20);
      ld_advance();
      LSTM_STAMP(stamp++)
    }
    finish_unit(a.seg[seg_beg + us].unit);
    LSTM_STAMP(stamp++)
  }
}

// One step launch; the caller has built the segment table with the same `units_per_block` (lstm_build_chain).
hipError_t launch_lstm_chain(const LstmWaveArgs& a, int units_per_block, hipStream_t stream) {
  dim3 grid((a.H + lc::BU - 1) / lc::BU, (a.B + lc::BM - 1) / lc::BM,
            (a.n_units + units_per_block - 1) / units_per_block);
  return launch_lds(lstm_chain_kernel, grid, dim3(256), lc::LDS_BYTES, stream, a);
}

}  // namespace empose
