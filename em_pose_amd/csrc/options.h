// The kernel-variant options: one table, the struct made from it and its process-wide instance (api.hip reads and sets
// it by name).  Internal, not part of the C ABI; the other interface headers are launch.h and *_kernels.h.
#pragma once

namespace empose {

// Kernel-variant selection for A/B and bit-identity tests (empose_set_option in the C ABI).  Plain process-wide ints set
// by an explicit call -- the library never reads the environment.  X(name, default) per option: this one list makes the
// fields of Options and the names empose_set_option / empose_get_option take (api.hip); empose_reset_options restores
// the defaults.
#define EMPOSE_OPTIONS(X) \
  X(mlp_fused, 1)      /* one-launch LDS-resident update MLPs (0: layer by layer) */ \
  X(lstm_persist, 1)   /* whole-sequence small-batch LSTM kernel (0: step launches) */ \
  X(gemm_splitk, 1)    /* split-K tile for problems of few output tiles (0: generic tiles) */ \
  X(heads_rows, 1)     /* large batches: both init heads as one row-block product (0: two problems on the generic tile) */ \
  X(lstm_seq, 0)       /* large batches: the whole sequence in one cooperative launch (measured slower: 0 = a launch per wavefront step) */ \
  X(bptt_wave, 1)      /* training: the reverse recurrences of a 2-layer LSTM as a wavefront (0: layer after layer) */ \
  X(gemm_wide, 1)      /* 256 x 256 four-wave tile (0: generic tiles) */ \
  X(smpl_tile, 1)      /* frame-per-lane SMPL sub-mesh kernel: 0 never, 1 from 16384 frames on, 2 always */ \
  X(smpl_fuse, 1)      /* on that path: update + feature row / Rodrigues reverse inside the blend GEMMs (0: own kernels) */ \
  X(train_fused, 0)    /* train-mode BatchNorm / PReLU folded into the GEMMs: 0 never (default: measured no faster, \
                             DESIGN.md), 1 above 1024 rows, 2 always */ \
  X(atb_target, 0)     /* workgroups the A^T B weight-gradient GEMM aims for when it splits its reduction (0: by size) */ \
  X(atb_fast, 1)       /* A^T B: whole-tile / whole-chunk problems on the branch-free interior kernel (0: the general kernel) */ \
  X(atb_chunk, 0)      /* rows per staged chunk of that kernel, 16 or 32 (0: by size) */ \
  X(mesh_skin_mfma, 0) /* split-bf16 full-mesh variant: the bone blend as a second matrix-core contraction (mesh_rows_bf16s_kernel; \
                             measured 9 % SLOWER than vector skinning: 15.6 against 17.1 M frames/s, so off by default) */ \
  X(train_epi, 1)      /* train-mode MLP layer: BatchNorm statistics in the GEMM epilogues + ONE combine-and-apply launch per \
                             layer and direction (train_fused.hip, finish kernels): 0 never, 1 above BN_SINGLE_PASS_ROWS rows, 2 always */ \
  X(spin_limit, 0)     /* polls of the cooperative LSTM kernels give up after this many spins (0: their own limits) */ \
  X(rows_x3, 1)        /* the row-block products with fused prologue / epilogue (blend GEMMs of the frame-per-lane SMPL path, init \
                             heads) on the same three-piece bf16 arithmetic; 0: the fp32 MFMA instruction */ \
  X(lstm_x3, 1)        /* large-batch LSTM steps (inference, uni-directional): fp32 products as six bf16-MFMA products of three \
                             bf16 pieces per operand; 1: lstm_x3.hip (K-split waves); 2: lstm_rows_x3.hip (row-split waves, weights \
                             through LDS, cell update in registers -- round 6, measured 10 % SLOWER: 47.5 against 42.9 us per \
                             launch, profiles/r06_lstm_rows_lab.txt, so opt-in); 3: lstm_chain16_x3.hip, kernel 1 on \
                             v_mfma_f32_16x16x32_bf16 -- measured FASTER: 37.8 against 39.5 us per launch in the headline profile, \
                             38.8 against 40.7 stand-alone, 5.20 against 5.30 ms per step (profiles/r07_*; docs/history.md \
                             "LSTM"), equal to rounding only: what the default 1 takes while lstm_chain16 is on, 3 forces it; \
                             0: the fp32 MFMA instruction (lstm_chain_kernel) */ \
  X(train_cols, 1)     /* training at <= 512 rows: a layer's product + BatchNorm + PReLU as one launch, both update networks \
                             side by side (train_cols.hip); 0: a product and a BatchNorm launch per layer and network */ \
  X(cols_coop, 1)      /* those one-launch layers, eager: launched with hipLaunchCooperativeKernel (all workgroups resident by \
                             the runtime's guarantee); 0: the ordinary launch (residency argued from the occupancy query) */ \
  X(mesh_x3, 1)        /* full-mesh vertices: blend shapes as six bf16-MFMA products of three bf16 pieces per operand \
                             (mesh_x3.hip): 1 stores staggered into the next tile's products, 2 stores at the end of the tile, \
                             3 skinning software-pipelined under the next tile's products; 0: the fp32 MFMA instruction \
                             (mesh_rows_kernel) */ \
  X(train_x3, 1)       /* training at more than 1024 rows: the layer products y = a W^T and dA = dY W of the update networks on \
                             three bf16 pieces (gemm_train_x3_kernel) when the caller supplies the packed weights \
                             (empose_mlp_params::weight_x3 / weight_t_x3); 0: the fp32 MFMA tile */ \
  X(lstm_midseq, 0)    /* 1: medium batches (4 .. 64 rows, inference): the whole sequence in one cooperative launch with the \
                             weight pieces in registers (lstm_midseq_x3.hip) -- built, same bits, measured SLOWER than a launch \
                             per wavefront step (10.5 against 8.2 us per step at 32 rows: a hand-over between XCDs costs more \
                             than a kernel boundary; profiles/r06i_lstm_midseq_lab.txt), so opt-in */ \
  X(lstm_mid16, 1)     /* LSTM steps of 17 .. 64 rows: 64 rows x 4-unit tiles on all 256 CUs (lstm_mid16_x3.hip); 0: the 8-unit \
                             tiles of lstm_mid_x3.hip (128 workgroups) */ \
  X(lstm_mid_x3, 1)    /* LSTM steps of 17 .. 256 rows (inference, uni-directional) on three bf16 pieces, 64 x 8-unit tiles \
                             (lstm_mid_x3.hip); 0: lstm_mid_kernel (fp32 MFMA, operands through LDS) */ \
  X(lstm_fewrows, 1)   /* LSTM steps of 4 .. 16 rows: all threads of a workgroup split K, lane reduce-scatter (lstm_fewrows_kernel), \
                             instead of the whole-sequence kernel / lstm_small_kernel (0: those; they share their bits) */ \
  X(mlp_x3, 1)         /* fused update MLPs: fp32 products as six bf16-MFMA products of three bf16 pieces per operand \
                             (mlp_fused_x3.hip: fp32-equivalent accuracy, measured equal to the fp32 instruction's against \
                             float64); 0: the fp32 MFMA instruction (mlp_fused.hip); any other value is on.  Which \
                             instruction and how many pieces is mlp_fused16's and mlp_pair16's choice */ \
  X(last_pass_joints, 1) /* LGD forward, frame-per-lane path: an SMPL evaluation nobody asks sensor outputs of (the last pass \
                             without histories) multiplies only the rest-joint column tiles of the blend matrix and runs the \
                             chain alone (smpl_tile_kernel, CHAIN_ONLY); 0: the whole sub-mesh, as for every other pass */ \
  X(lstm_state_direct, 1) /* large-batch LSTM steps (lstm_x3.hip), new sequences: the piece planes of the zero initial state by \
                             one fill, h_n / c_n stored by the last step of each layer; 0: a split launch and a fill per layer, \
                             2 L trailing copies */ \
  X(lstm_skip_dead, 1) /* chain step kernels (lstm_x3 = 1 / 3): work whose result nobody reads is left out, same bits -- the \
                             recurrent k-steps of a unit whose h_{t-1} is the zero state of a new sequence, and without \
                             seq_lengths (lstm_state_direct path) the fp32 h_prev loads / h_next stores; 0: all of it runs */ \
  X(mlp_fused16, 1)    /* fused update MLPs with mlp_x3 != 0: the products on v_mfma_f32_16x16x32_bf16 (mlp_fused_x3_kernel<16>, \
                             weights in the [k-step of 32][16-column tile][piece] order); 0: v_mfma_f32_32x32x16_bf16 \
                             (mlp_fused_x3_kernel<32>).  Equal to rounding, not to the bit */ \
  X(mlp_pair16, 1)     /* fused update MLPs with mlp_x3 != 0 and mlp_fused16 != 0: every fp32 product from TWO f16 pieces per \
                             operand under per-row / per-column power-of-two scales, three v_mfma_f32_16x16x32_f16 instead of six \
                             of the bf16 instruction (mlp_fused_x3_kernel<PAIR16>, f16pair.h); 0: the three bf16 pieces of \
                             mlp_fused_x3_kernel<16>.  Equal to rounding, not to the bit */ \
  X(lstm_chain16, 1)   /* large-batch LSTM steps with lstm_x3 = 1: lstm_chain16_x3.hip (v_mfma_f32_16x16x32_bf16) where the model \
                             has the LSTM_MID16 weight order; 0: lstm_chain_x3_kernel (32x32x16) */ \
  X(lstm_pair16, 1)    /* large-batch LSTM steps on the 16x16x32 chain kernel (lstm_x3 = 3, or 1 with lstm_chain16 on): every \
                             operand the kernel itself produced -- h_{t-1} and the layer below's h_t, both in [-1, 1] -- as TWO \
                             f16 pieces under the fixed scale 2^14, weights under per-column power-of-two scales, three \
                             v_mfma_f32_16x16x32_f16 instead of six of the bf16 instruction (lstm_chain16_pair_kernel, \
                             f16pair.h); the raw input of layer 0 and a caller's h0 stay on three bf16 pieces and share the \
                             accumulator; 0: three bf16 pieces throughout (lstm_chain16_x3_kernel).  Equal to rounding, not to \
                             the bit */

struct Options {
#define EMPOSE_OPTION_FIELD(name, default_value) int name = default_value;
  EMPOSE_OPTIONS(EMPOSE_OPTION_FIELD)
#undef EMPOSE_OPTION_FIELD
};
Options& options();

}  // namespace empose
