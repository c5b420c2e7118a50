// Launch interfaces of the LSTM forward kernels (lstm_*.hip).  Internal, not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace empose {

// ---------------------------------------------------------------------------------------------------------------
// LSTM
// ---------------------------------------------------------------------------------------------------------------
struct LstmUnitArgs {        // one (layer, direction), selected by blockIdx.z
  const float* w_ih;   // [4H][in_k]
  const float* w_hh;   // [4H][H]
  const float* bias;   // [4H] = b_ih + b_hh
  int in_k;            // width of the unit's input
  const float* in_seq; int in_ld;  // stored input sequence [B][F][in_ld] (used when in_from < 0)
  int in_from;         // >= 0: the input is the hidden state of unit `in_from` after its step (stacked wavefront)
  int t_offset;        // the unit processes step k = s - t_offset
  int reverse;         // 1: at step k row b visits time len_b - 1 - k
  float* h[2];         // [B][H] ping-pong: step k reads h[k & 1], writes h[(k + 1) & 1]
  float* c;            // [B][H] updated in place
  float* y; int y_ld; int y_col;   // output sequence [B][F][y_ld], columns [y_col, y_col + H), or nullptr
  // Training forward (forward units only): what back-propagation through time needs, batch-major like y.
  float* sv_gates = nullptr;       // [B][F][4H] activated gates (i | f | g | o) of every step, or nullptr
  float* sv_c = nullptr;           // [B][F][H] cell state after the step (unchanged past a row's length)
  float* sv_hprev = nullptr;       // [B][F][H] hidden state BEFORE the step; the caller fills slot t = 0 (h_0)
};
struct LstmSeg {             // one operand segment (input part / recurrent part) of a unit's step; built on the host
  const float* a;            // A rows: a + row * lda (+ per-row time offset, below)
  const float* w;            // W rows: w + (gate * H + unit) * ldw
  int lda, ldw;
  int K;
  int tstride;               // != 0: reverse unit on a stored sequence; row b adds max(len_b - 1 - k, 0) * tstride
  int k;                     // the unit's step index
  int ntiles;                // ceil(K / 64)
  int unit;                  // index into LstmWaveArgs::unit
  int pad;
};
struct LstmWaveArgs {
  LstmUnitArgs unit[4];
  int n_units;
  const int* seq_lengths;    // [B] or nullptr (required for reverse units)
  int B, F, H;
  int s;                     // launch index
  // set by lstm_build_chain (lstm_wave.h): blockIdx.z walks through the segments [z_beg[z], z_beg[z] + z_cnt[z]) (two per active unit)
  LstmSeg seg[8];
  int z_beg[4], z_cnt[4];
};
// The fp32 step kernels, one launcher each; plan_lstm (api_lstm.hip) picks, the launchers take no decisions.  All expect the
// segment table built (lstm_build_chain, lstm_wave.h): one unit per slice, lstm_chain_kernel `units_per_block`.  A shape
// outside a kernel's ..._shape_ok is hipErrorInvalidValue.
hipError_t launch_lstm_chain(const LstmWaveArgs& a, int units_per_block, hipStream_t stream);   // lstm_chain.hip
hipError_t launch_lstm_mid(const LstmWaveArgs& a, hipStream_t stream);                          // lstm_mid.hip
bool lstm_small_shape_ok(int B);                                                                 // lstm_fewrows.hip
bool lstm_fewrows_shape_ok(int B, int H, int n_units, const int* in_k);
hipError_t launch_lstm_small(const LstmWaveArgs& a, hipStream_t stream);
hipError_t launch_lstm_fewrows(const LstmWaveArgs& a, hipStream_t stream);
// Whole sequence of a stacked uni-directional LSTM on a LARGE batch in one cooperative launch (lstm_seq.hip,
// lstm_seq_kernel): the units' hidden states rotate through three buffers (h[0], h[1] of the unit + a third one), the
// workgroups of a 64-row group synchronise through `counters` (lstm_seq_counter_uints(B) unsigned, zeroed by the launcher).
struct LstmSeqArgs {
  LstmUnitArgs unit[4];
  float* hs[4][3];
  int n_units;
  const int* seq_lengths;
  int B, F, H;
  unsigned* counters;
  int spin_limit;
  unsigned* timeouts;   // poll_timeout_word(): counts the polls that gave up (the outputs are NaN from there on)
};
// The wavefront step of large batches on the bf16 matrix path, three bf16 pieces per fp32 operand (lstm_x3.hip).  All
// operands arrive in fragment order: weights packed at model creation (api_lstm.hip pack_lstm_x3: [k-step][32-unit block][gate]
// [piece][512 bf16]), activations as A planes [32-row tile][k-step][piece][512 bf16] written by the producing step (hidden
// states) or by launch_lstm_split_rows (stored input, initial state).
struct LstmX3Unit {
  const unsigned short* w3_ih; const unsigned short* w3_hh;
  const float* bias;                 // [4H] = b_ih + b_hh
  const unsigned short* a3_in;       // the unit's input at this step: planes of x_t, or of the unit below's new hidden state
  int ks_in;                         // k-steps of 16 of that input
  // k-steps of 16 of the recurrent operand the chain kernels multiply: H / 16, or 0 where h_{t-1} is the zero state of a new
  // sequence (its products are all +-0: leaving them out changes no bit).  The other step kernels walk H / 16 regardless.
  int ks_rec;
  const unsigned short* a3_rec;      // planes of h_{t-1}
  unsigned short* a3_out;            // planes of h_t
  const float* h_prev; float* h_next; float* c;   // [B][H] fp32: state hand-over and rows past their length
  float* y; int y_ld, y_col;         // output sequence [B][F][y_ld] or nullptr
  int t;                             // the unit's time step in this launch
  // the layer's slices of h_n / c_n ([B][H]) on the launch of its last step, else nullptr: a second copy of what goes to
  // h_next / c (the chain kernels only; the other step kernels ignore them and the caller copies the state out)
  float* h_final = nullptr; float* c_final = nullptr;
  // lstm_chain16_pair_kernel only.  A part (input / recurrent) is walked in pair steps -- its planes hold two f16 pieces of
  // h 2^14, its weights (w3_ih / w3_hh) two f16 pieces of w s_n, both at the three-piece stride -- or in wide steps: three
  // bf16 pieces of the operand as it is, weights those of w s_n 2^14.  inv_scale: [4H] 2^-14 / s_n, applied to the gate sums
  int in_pair = 0, rec_pair = 0;
  const float* inv_scale = nullptr;
};
struct LstmX3Args {
  LstmX3Unit unit[4];
  int n_units, units_per_block;      // blockIdx.z walks units [z * units_per_block, ...)
  const int* seq_lengths;
  int B, F, H;
  // chain kernels: nobody reads the fp32 hidden-state buffers (no seq_lengths: every row live at every step; the last step
  // stores h_final) -- h_prev is not loaded, h_next not stored
  int skip_h_state = 0;
};
hipError_t launch_lstm_chain_x3(const LstmX3Args& a, hipStream_t stream);
// the same step on v_mfma_f32_16x16x32_bf16, weights in the LSTM_MID16 order (lstm_chain16_x3.hip; option lstm_x3 = 3)
hipError_t launch_lstm_chain16_x3(const LstmX3Args& a, hipStream_t stream);
// ... with the operands the kernel produced itself on two f16 pieces (LstmX3Unit::in_pair / rec_pair; option lstm_pair16)
hipError_t launch_lstm_chain16_pair(const LstmX3Args& a, hipStream_t stream);
// the same step with the waves splitting ROWS, the weight block of a k-step shared through LDS and the cell update in
// registers (lstm_rows_x3.hip; option lstm_x3 = 2): one unit per workgroup, `units_per_block` unused
hipError_t launch_lstm_rows_x3(const LstmX3Args& a, hipStream_t stream);
// the step of MEDIUM batches (17 .. 256 rows): 64 rows x 8 units per workgroup, weights in the 8-unit-block order
// (api_lstm.hip pack_lstm_x3 with mid = true), K split over the waves (lstm_mid_x3.hip; option lstm_mid_x3)
hipError_t launch_lstm_mid_x3(const LstmX3Args& a, hipStream_t stream);
// ... at most 64 rows: 4-unit tiles (16 columns, v_mfma_f32_16x16x32_bf16), weights in the order of api_lstm.hip
// pack_lstm_x3_mid16, twice the workgroups (lstm_mid16_x3.hip; option lstm_mid16)
bool lstm_mid16_shape_ok(int B, int H);
hipError_t launch_lstm_mid16_x3(const LstmX3Args& a, hipStream_t stream);
// The whole sequence of a medium batch (B <= 64) in one cooperative launch with the weight pieces in registers
// (lstm_midseq_x3.hip; option lstm_midseq): same tiles, products and bits as the step launches of lstm_mid_x3.hip.
struct LstmMidSeqUnit {
  const unsigned short* w3_ih; const unsigned short* w3_hh;   // the 8-unit-block order of lstm_mid_x3.hip
  const float* bias;                 // [4H] = b_ih + b_hh
  const unsigned short* in3; size_t in_t_stride;   // layer 0: planes of the stored input, bf16 elements per time step
  int ks_in;                         // k-steps of 16 of the unit's input
  unsigned short* xa;                // [F + 1] sets of planes of the unit's hidden state: slot 0 = initial, slot t + 1 = h_t
  const float* h0; float* h_last; float* c;   // [B][H] fp32: initial hidden state, final hidden state, cell state (in place)
  float* y; int y_ld, y_col;         // output sequence [B][F][y_ld] or nullptr
};
struct LstmMidSeqArgs {
  LstmMidSeqUnit unit[4];
  int n_units;
  const int* seq_lengths;
  int B, F, H;
  unsigned* flags;                   // [n_units][H / 8] progress counters (lstm_midseq_flag_uints), zeroed by the launcher
  int spin_limit;
  unsigned* timeouts;                // poll_timeout_word()
};
size_t lstm_midseq_flag_uints(int n_units, int H);
bool lstm_midseq_shape_ok(int B, int H, int n_units, const int* ks_in);
hipError_t launch_lstm_midseq_x3(const LstmMidSeqArgs& a, hipStream_t stream, bool* done);
hipError_t launch_lstm_split_rows(const float* src, long row_stride, long z_stride, int n_z, int B, int K, int KS,
                                  unsigned short* dst, long dst_z_stride, hipStream_t stream);
constexpr int LSTM_SEQ_MIN_B = 257;   // below: lstm_mid_kernel / the small-batch kernels
size_t lstm_seq_counter_uints(int B);
bool lstm_seq_shape_ok(int H, int n_units, const int* in_k);   // enough K tiles per unit (per-unit input widths in_k)
hipError_t launch_lstm_seq(const LstmWaveArgs& a, float* const* h_third, unsigned* counters, hipStream_t stream, bool* done);
// Whole sequence of a stacked uni-directional LSTM in one cooperative launch (lstm_persist.hip, B <= 16); *done = false:
// its workgroups cannot all be resident here.
constexpr int LSTM_PERSIST_B = 16;   // largest batch of the whole-sequence kernel
constexpr int LSTM_FEWROWS_MIN_B = 4;   // from here to 16 rows a step launch of lstm_fewrows_kernel beats it (option lstm_fewrows)
size_t lstm_persist_xch_floats(int n_units, int B, int H);   // its exchange buffer (8-byte aligned)
bool lstm_persist_shape_ok(int B, int H, int n_units, const int* in_k);   // H, in_k <= 512 in 16-byte pieces, rows within LDS
hipError_t launch_lstm_persist(const LstmWaveArgs& a, float* xch, hipStream_t stream, bool* done);

}  // namespace empose
