// Launch interfaces of the SMPL sub-mesh kernels (smpl_chain.hip, smpl_rows.hip, smpl_tile.hip) and of the row-block
// products around them (mlp_fused.hip).  Internal, not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

namespace empose {

// ---------------------------------------------------------------------------------------------------------------
// SMPL sub-mesh kernels
// ---------------------------------------------------------------------------------------------------------------
constexpr int CHAIN_CHUNK = 8;  // pairs per partial-sum chunk of the per-bone (vertex, weight) lists
constexpr int NB = 22;           // body joints

// LDS record of one frame in chain_sensors_kernel (shared with the host, which packs LDS offsets into the tables).
struct ChainLds {  // per-frame float offsets
  int rot, out, g, at, v, dv, u, total;
  // inside u (time-shared): fn | fg | scr   then   part (later: pd, fp64 prefix sums) | m | x
  int fn, fg, scr, part, pd, m, x;
};

__host__ __device__ inline ChainLds chain_layout(int nv, int ncp, int max_deg, int n_chunks) {
  // Live ranges (phases of chain_sensors_kernel): rot P0-P2 | out P0-P5 | g, at P2-P7 | v P3-P4c | dv P4d-P5 |
  // fn P4a-P4b, fg P4c-P4d, scr P4b-P4d | part P5-P5c | m P5c-P6a | pd P6a-P6b | x P6b-P7.  Records that are never
  // live together share their space (rot with the scratch area, dv with v, x with m): 6.9 KB per frame instead of
  // 9.7 KB, i.e. one more workgroup per CU.
  ChainLds l;
  int o = 0;
  l.out = o; o += ncp;
  l.g = o; o += NB * 12;    // per joint: G^R (9, row-major) | G^t (3)
  l.at = o; o += NB * 3;    // A^t = G^t - G^R J
  l.v = o; o += nv * 3;
  l.dv = l.v;
  o = (o + 1) & ~1;         // 8-byte alignment for the fp64 prefix sums (below)
  l.u = o;
  l.rot = l.u;
  const int nf = 12 * max_deg;
  l.fn = l.u; l.fg = l.fn + nf * 3; l.scr = l.fg + nf * 6;
  const int sz1 = nf * 9 + 12 * 9;
  const int pd_floats = (NB + 1) * 12 * 2;             // [23][12] doubles, aliases the chunk partial sums
  const int part_size = n_chunks * 12 > pd_floats ? n_chunks * 12 : pd_floats;
  l.part = l.u; l.pd = l.u; l.m = l.part + part_size; l.x = l.m;
  const int sz2 = part_size + NB * 12;
  int sz = sz1 > sz2 ? sz1 : sz2;
  sz = sz > NB * 9 ? sz : NB * 9;
  o += sz;
  l.total = (o + 3) & ~3;
  return l;
}


// Word offsets into the packed table blob that chain_sensors_kernel stages into LDS (all entries are 32-bit).
struct ChainTabs {
  int path_mask, sub_mask, parents;       // [22] each: ancestors-or-self mask, subtree mask, parent index
  int dfs_pos, sub_size;                  // [22] each: position of a joint in depth-first pre-order, size of its subtree
  int skin_idx, skin_w;                   // [nv*kb]
  int chunk_bone, chunk_beg;              // [n_chunks]: CHAIN_CHUNK-pair slices of the per-bone (vertex, weight) lists
  int bone_chunk_ptr;                     // [23]
  int bone_vert, bone_w;                  // [nnz]
  int s_center, s_helper, s_deg, s_faces; // [12], [12], [12], [12*max_deg*3]
  int inc_ptr, inc_code;                  // [nv+1], [n_inc]: per vertex, what contributes to its cotangent
  int total;
};

struct SmplTables {  // device pointers
  int n_sensors, nv, j_off, ncp, kb, max_deg;
  int n_chunks;
  const uint32_t* blob;
  ChainTabs off;

  const float* wc; const float* wct;
  const int* parents;
  const int* skin_idx; const float* skin_w;
  const int* bone_ptr; const int* bone_vert; const float* bone_w;
  const int* s_center; const int* s_helper; const int* s_deg; const int* s_faces;
  const int* path_ptr; const int* path; const int* sub_ptr; const int* sub;
};

// Pack the network input columns and the per-frame loss weight.
struct PackArgs {
  const float* marker_pos; const float* marker_oris;  // [T][36], [T][108]
  const float* marker_masks;                           // [T][12] or nullptr
  const int* seq_lengths;                              // [B] or nullptr
  float* x; int ldx;                                   // cols [0, 12*n_markers)
  float* frame_scale;                                  // [T]
  int B, F, n_markers;
  int marker_idx[12];
  int rows_as_unpadded = 0;   // 1: a ragged row counts as an unpadded window of its own length
  int suppress_missing = 0;   // 1: readings of sensors whose mask is not 1 are replaced by mask_value (the
  float mask_value = 0.f;     //    arithmetic of reference data/data.py:284-302: x * valid + mask_value * !valid)
};
hipError_t launch_pack_inputs(const PackArgs& a, hipStream_t stream);

// theta/beta update (+ window mean of the shape), Rodrigues and the GEMM feature row.
struct FeatArgs {
  float* theta; int ld_theta;          // [T][>=66] updated in place
  float* beta; int ld_beta;            // [T][>=10] updated in place
  const float* d_theta;                // [T][66] or nullptr
  const float* d_beta;                 // [T][10] or nullptr
  float theta_step;                    // theta += theta_step * d_theta
  float beta_keep, beta_step;          // beta = beta_keep * beta + beta_step * (shape_avg ? mean_F(d_beta) : d_beta)
  int shape_avg;                       // 0 none, 1 mean over all F frames, 2 mean over the valid frames
  const int* seq_lengths = nullptr;    // [T/F], only read when shape_avg == 2
  float* rot;                          // [T][22][9]
  float* feat;                         // [T][200]
  float* out_theta; float* out_beta;   // optional dense copies [T][66], [T][10]
  float* out_theta2; float* out_beta2; // optional second copy (history)
  float* theta_t = nullptr;            // optional: the updated theta in tile layout [tiles][66][64] (smpl_tile.hip)
  int T, F;
  int rod_conv = 0;                    // EMPOSE_RODRIGUES_SMPLX (0) or EMPOSE_RODRIGUES_SO3 (1)
};
hipError_t launch_update_feat(const FeatArgs& a, hipStream_t stream);

struct ChainArgs {
  SmplTables tab;
  const float* rot;        // [T][22][9]
  const float* out;        // [T][ncp] = feat . wc^T
  const float* offset_r;   // [T/F][12][9]
  const float* offset_t;   // [T/F][12][3]
  const float* tgt; int ld_tgt;   // network-input layout; nullptr => forward only
  const float* frame_scale;       // [T]
  int n_markers; int used_slot[12];  // used_slot[m] = column slot of virtual sensor m in tgt, or -1
  float* pos; float* ori; float* joints;   // [T][36], [T][108], [T][66]
  float* pos2; float* ori2; float* joints2;  // optional second copies
  float* d_out;            // [T][ncp]
  float* d_rot;            // [T][22][9]
  int T, F;
  const float* cot_pos = nullptr;    // [T][36]  external cotangents (vector-Jacobian product for training);
  const float* cot_ori = nullptr;    // [T][108] when set they replace the residual of `tgt`
  const float* cot_joints = nullptr; // [T][66]  optional
};
size_t chain_lds_bytes(const SmplTables& tab, int frames_per_block);
hipError_t launch_chain_sensors(const ChainArgs& a, hipStream_t stream);


struct RodBwdArgs {
  const float* theta; int ld_theta;
  const float* d_rot;      // [T][22][9]
  const float* d_feat;     // [T][200]
  float* g_theta; int ld_g;
  float* g_beta; int ld_gb;
  float* trace_g_theta; float* trace_g_beta;  // optional dense copies
  int T;
  int rod_conv = 0;
};
hipError_t launch_rodrigues_bwd(const RodBwdArgs& a, hipStream_t stream);

// ---------------------------------------------------------------------------------------------------------------
// SMPL sub-mesh with one frame per lane (smpl_tile.hip): tables, arguments, launchers.
// "Tile layout" of a per-frame matrix X[T][C]: X_t[tile = t / 64][c][t % 64] -- a column of 64 frames is contiguous.
// ---------------------------------------------------------------------------------------------------------------
constexpr int TL_FR = 64;             // frames per tile = lanes of a wave
constexpr int ROD_BWD_LD = 77;        // row stride of rodrigues_bwd_tile's staging block [TL_FR][77] (66 g_theta | 10 g_beta | pad)
constexpr int TL_NR = 8;              // largest ring (= sensor vertex degree) the kernel takes
constexpr int TL_NLOC = TL_NR + 1;    // local vertices of a sensor patch: centre + ring
constexpr int TL_NBL = 8;              // distinct bones under one patch
struct TileSensor {
  int deg, helper, col, nb;           // ring size, ring index of the helper vertex, first column of the patch, bones
  int bone[TL_NBL];                   // the patch's bones (unused slots: bone 0 with zero weights)
  int bones, pad[3];                  // bit mask of the bones (host: scheduling)
  float w[TL_NLOC][TL_NBL];           // dense skin weights of local vertex i over the patch's bones
};
struct TileTables {                   // one per model, in device memory, read with scalar loads
  int ncp2, j_off2, nloc, nbl;        // columns of the tile (multiple of 32), first rest-joint column, most local
                                      // vertices / bones of a patch
  int n_rounds;
  TileSensor s[12];
  int parent[22];
};
bool build_tile_tables(int nv, int kb, int max_deg, int j_off, const float* wc, const int* parents, const int* skin_idx,
                       const float* skin_w, const int* s_center, const int* s_helper, const int* s_deg,
                       const int* s_faces, TileTables* out, std::vector<float>* wc2);
struct TileArgs {
  const TileTables* tab;
  const float* theta; int ld_theta;   // [T][ld] axis-angles (66 used)
  const float* theta_t = nullptr;     // the same in tile layout [tiles][66][64], or nullptr (strided loads: 64 cache
                                      // lines per load instruction)
  const float* tgt_t = nullptr;       // tgt in tile layout [tiles][12 * n_markers][64], or nullptr
  const float* out_t;                 // tile layout [tiles][ncp2][64]: v_posed of the patches | rest joints
  const float* offset_r;              // [T/F][12][9]
  const float* offset_t;              // [T/F][12][3]
  const float* tgt; int ld_tgt;       // network-input layout; nullptr with backward => external cotangents
  const float* frame_scale;           // [T]
  int n_markers; int used_slot[12];
  float* pos; float* ori; float* joints;       // [T][36], [T][108], [T][66] or nullptr (not wanted)
  float* pos2; float* ori2; float* joints2;    // optional second copies
  float* d_out_t;                     // tile layout [tiles][ncp2][64]
  float* d_rot_t;                     // tile layout [tiles][198][64]
  int T, F;
  int rod_conv;
  const float* cot_pos = nullptr;     // [T][36], [T][108]: external cotangents instead of the residual
  const float* cot_ori = nullptr;
};
// `chain_only` (forward, no sensor outputs asked for): Rodrigues + chain and the joint stores alone; reads only the
// rest-joint columns of out_t
hipError_t launch_smpl_tile(const TileArgs& a, bool backward, int nloc, int nbl, hipStream_t stream, bool chain_only = false);
struct RodBwdTArgs {
  const float* theta; int ld_theta;
  const float* theta_t = nullptr;     // optional: the same values in tile layout [tiles][66][64] (coalesced loads)
  const float* d_rot_t;               // tile layout [tiles][198][64]
  const float* d_feat_t; int ld_feat_t;   // tile layout [tiles][ld_feat_t][64] (columns 0..198 used)
  float* g_theta; int ld_g; float* g_beta; int ld_gb;
  float* trace_g_theta; float* trace_g_beta;
  int T; int rod_conv;
};
hipError_t launch_rodrigues_bwd_t(const RodBwdTArgs& a, hipStream_t stream);
hipError_t launch_rows_to_tile(const float* src, int ld, int cols, float* dst_t, int T, hipStream_t stream);
// C = A . Wp^T with tile-layout operands (mlp_fused.hip): A row-major [M][lda] or tile layout (a_tile), C in tile layout
// [tiles][ldc_t][64] (ldc_t == N rounded up to 32; the padding columns are written as zeros).
hipError_t launch_gemm_rows_t(const float* A, int lda, bool a_tile, const float* Wp, float* C_t, int ldc_t, int M, int N,
                              int K, hipStream_t stream);

// The same two products with the small kernels around them folded in (mlp_fused.hip): the pose / shape update +
// feature row as the prologue of the first (the [T][200] feature matrix never reaches HBM), the Rodrigues reverse as
// the epilogue of the second (neither do the feature cotangents).
// x3: Wp = three bf16 pieces per weight in bf16-MFMA fragment order (pack_fragments_x3_raw), product on the bf16 matrix path
// [col_lo, col_hi): compute and write only the 32-column tiles of C_t that cover these columns (same bits there as the
// full product); the default is every column
hipError_t launch_blend_feat_gemm(const FeatArgs& fa, const float* Wp, float* C_t, int ldc_t, int N, bool x3,
                                  hipStream_t stream, int col_lo = 0, int col_hi = 0);
hipError_t launch_blend_t_gemm_rod(const float* A_t, int lda_t, const float* Wp, int K, const RodBwdTArgs& ra, bool x3,
                                   hipStream_t stream);

// The two init heads on the LSTM output as one product over their stacked columns (mlp_fused.hip): Wp = the stacked weight
// [n_pose + n_shape][K] in fragment order, bias stacked likewise.
bool heads_rows_applicable(int M, int K);
hipError_t launch_heads_rows(const float* y, int ldy, const float* Wp, const float* bias, float* theta, int ld_theta,
                             float* shape, int ld_shape, int M, int K, int n_pose, int n_shape, bool x3, hipStream_t stream);

}  // namespace empose
