// Launch interfaces of the full-mesh kernels (mesh_*.hip, virtual_sensors.hip, sensors_vjp.hip).  Internal, not part of
// the C ABI.
#pragma once
#include <hip/hip_runtime.h>

#include "smpl_kernels.h"   // NB

namespace empose {

// Full-mesh: chain only (joints + relative transforms) and dense skinning.
constexpr int MESH_MAX_JOINTS = 52;   // SMPL-H: 22 body + 2 x 15 hand joints
struct MeshChainArgs {
  const float* rot; const float* out; int ncp; int j_off;   // out: rest joints [T][ncp], n_joints * 3 used from j_off
  const int* parents;      // [n_joints], topologically ordered
  const float* trans;      // [T][3] or nullptr
  float* xf;               // [T][22][3][4]: per body bone and row (G^R[r][0..2], A^t[r])
  float* joints;           // [T][n_joints][3]
  int T;
  int n_joints = NB;       // 22 (body) or up to MESH_MAX_JOINTS (hand joints ride on their parents, zero hand pose)
};
hipError_t launch_mesh_chain(const MeshChainArgs& a, hipStream_t stream);
// The 22 skinning transforms once more with everything ahead of them in float64 -- Rodrigues, the rest joints (the joint
// rows of wc times the feature row) and the chain -- and one rounding to float32 at the end: the transforms of the aligned
// sweep of the Procrustes-aligned vertex error (mesh_err.hip), whose error is otherwise that of the float32 rotations and
// rest joints.  Three small launches through the scratch rot [T][22][9] and jrest [T][66] (doubles).
struct MeshChainF64Args {
  const float* poses; const float* betas;   // [T][66] (root first), [T][10]
  const float* wj;                          // the rest-joint rows of wc, [>= 66][200]
  const int* parents;                       // the first NB entries are used
  double* rot; double* jrest;
  float* xf;                                // [T][22][3][4], as MeshChainArgs::xf
  int T, rod_conv;
};
hipError_t launch_mesh_chain_f64(const MeshChainF64Args& a, hipStream_t stream);
struct MeshSkinArgs {
  const float* feat;           // [T][200]
  const float* wc;             // [V*3 (+66)][200]: row 3s+c = coefficients of coordinate c of vertex s
  const float* xf;             // [T][22][3][4]: row r of bone b = (G^R[r][0..2], A^t[r])
  const int* skin_idx; const float* skin_w; int kb;
  const float* trans;
  float* vertices;             // [T][V][3]
  int T, V;
  const float* wc_frag;        // [tiles][25][3][64][4]: wc in fragment order per 32-vertex tile (api_mesh.hip pack_mesh_tiles)
  const int* skin_idx4; const float* skin_w4;   // [tiles * 32][4]
  const void* wc_bf16 = nullptr;   // bf16 pieces of wc in fragment order per tile (api_mesh.hip pack_mesh_tiles_bf16), or nullptr
  const void* skin_bf16 = nullptr; // dense skin weights per 32-vertex tile as bf16 pieces in fragment order (pack_mesh_skin_bf16)
  const void* wc_x3 = nullptr;     // THREE bf16 pieces of wc in fragment order per tile (api_mesh.hip pack_mesh_tiles_x3)
  int stagger = 1;                 // mesh_rows_x3_kernel: a tile's stores ride in the next tile's K loop, at a per-wave k-step
};
hipError_t launch_mesh_rows(const MeshSkinArgs& a, hipStream_t stream);
// The same evaluation with the blend-shape contraction in split bf16 (mesh_bf16.hip); needs MeshSkinArgs::wc_bf16.
hipError_t launch_mesh_rows_bf16(const MeshSkinArgs& a, hipStream_t stream);
constexpr int MESH_BF16_TILE_BYTES = 14 * 3 * 2 * 1024;
// ... and with the bone blend as a second contraction on the matrix cores (needs MeshSkinArgs::skin_bf16 too).
hipError_t launch_mesh_rows_bf16s(const MeshSkinArgs& a, hipStream_t stream);
constexpr int MESH_SKIN_BF16_TILE_BYTES = 2 * 2 * 1024;
// The blend-shape contraction on three bf16 pieces per operand -- fp32-equivalent, the default arithmetic of the full-mesh
// evaluation since round 6 (mesh_x3.hip; option mesh_x3: 1 = products, skinning, stores one after the other with the stores
// staggered into the next tile's K loop, 2 = the same with the stores at the end of their tile, 3 = the skinning
// software-pipelined under the next tile's K loop (measured no faster), 0 = the fp32 MFMA kernel).  Four bones per vertex
// (kb <= 4); needs MeshSkinArgs::wc_x3.
hipError_t launch_mesh_rows_x3(const MeshSkinArgs& a, bool overlap, hipStream_t stream);
constexpr int MESH_X3_TILE_BYTES = 13 * 9 * 1024;

// Per-vertex error between two bodies (mesh_err.hip): both bodies of a frame are evaluated in the same lanes on the fp32
// MFMA instruction and only their distances are kept -- part [T][tiles][2] = the sums of |v_A - v_B| and of its square
// over the 32 vertices of a tile (vertices past V count as an exact 0), tiles = ceil(V / 32).  launch_mesh_err_sum adds a
// frame's partials in ascending tile order in double: out [T][2].  Fixed-order sums only; a frame's result depends on
// nothing but that frame.
struct MeshPairErrorArgs {
  const float *feat_a, *xf_a, *trans_a;   // body A: [T][200], [T][22][3][4], [T][3] or nullptr
  const float *feat_b, *xf_b, *trans_b;   // body B likewise
  const int* skin_idx; const float* skin_w; int kb;
  int T, V;
  const float* wc_frag;                   // as MeshSkinArgs
  const int* skin_idx4; const float* skin_w4;
  float* part;
  // The Procrustes-aligned error (PA-PVE) takes two sweeps of the same kernel around mesh_pa_solve_kernel:
  //   MESH_PAIR_MOMENTS  part as the plain form, bit for bit, and part_m [T][tiles][MESH_PA_MOMENTS]: with a = v_A - pivot_a
  //                      and b = v_B - pivot_b the tile's sums of a (3), b (3), a b^T (9, row-major), |a|^2 and |b|^2;
  //   MESH_PAIR_ALIGNED  part holds the sums of d = |(v_A - c_A) - sR (v_B - c_B)| and d^2, sR and the centroids from
  //                      align [T][MESH_PA_ALIGN]: M (9, the aligned b is b M), c_A (3), c_B (3), one unused.
  int mode = 0;
  const float *pivot_a = nullptr, *pivot_b = nullptr; int ld_pivot = 0;   // MOMENTS: [T][ld_pivot], three used
  float* part_m = nullptr;
  const float* align = nullptr;
};
constexpr int MESH_PAIR_PLAIN = 0, MESH_PAIR_MOMENTS = 1, MESH_PAIR_ALIGNED = 2;
constexpr int MESH_PA_MOMENTS = 17, MESH_PA_ALIGN = 16;
hipError_t launch_mesh_pair_error(const MeshPairErrorArgs& a, hipStream_t stream);
// out[t * ld_out + 0 .. 1]
hipError_t launch_mesh_err_sum(const float* part, int n_tiles, int T, double* out, hipStream_t stream, int ld_out = 2);
// One lane per frame, float64: the tile partials of a MOMENTS sweep in ascending tile order, centred, normalised, the
// 3 x 3 SVD and the conventions of the joints' alignment (svd3.h procrustes_rotation).  Writes align [T][MESH_PA_ALIGN]
// for the ALIGNED sweep and the frame's plain sums to sums[t * 4 + 0 .. 1].  A NaN moment gives NaNs.
struct MeshPaSolveArgs {
  const float *part, *part_m;
  const float *pivot_a, *pivot_b; int ld_pivot;
  float* align;
  double* sums;
  int T, V;
};
hipError_t launch_mesh_pa_solve(const MeshPaSolveArgs& a, hipStream_t stream);

// Full-mesh vector-Jacobian product (mesh_vjp.hip): the two vertex sweeps of the reverse for a cotangent dV [T][V][3].
//   feat sweep: d_feat[t][k] = sum_v,c dvp[t][v][c] wc[3v+c][k], dvp_v = sum_b w_vb (A_b^R)^T dV_v   -> out [T][200]
//   bone sweep: dA_b[t][r][c] = sum_v w_vb dV_v[r] [vp_v; 1][c]                                       -> out [T][22][12]
//   the feat sweep also sums dV over the vertices in double precision (the translation's cotangent)   -> dtrans
// Deterministic: fixed-order sums only.  With mesh_vjp_split(..) > 1 the vertex tiles are split over grid.y and the
// partials ([split][T][cols] in `part`) are summed in slot order by a second launch.
constexpr int MESH_VJP_BM = 32;            // frames per workgroup of both sweeps
constexpr int MESH_VJP_DA = NB * 12;       // bone-sweep output columns per frame
constexpr int MESH_VJP_WC_TILE_FLOATS = 16 * 6 * 64 * 4;   // wc_vjp per 32-vertex tile: [16 vertex pairs][6][64 lanes][4]
constexpr int MESH_VJP_SKIN_TILE_FLOATS = 4 * 64 * 4;      // skin_dense per tile: [4][64 lanes][4]
struct MeshVjpArgs {
  const float* feat;           // [T][200]
  const float* xf;             // [T][22][3][4] (mesh_chain_kernel)
  const float* dv;             // [T][V][3]
  const float* wc_frag;        // forward fragment order (MeshSkinArgs::wc_frag), bone sweep
  const float* wc_vjp;         // vertex rows of wc in the feat sweep's B-fragment order (api_mesh.hip pack_mesh_vjp)
  const float* skin_dense;     // dense bone weights per tile in the bone sweep's B-fragment order (ditto)
  const int* skin_idx4; const float* skin_w4;   // [tiles * 32][4]
  const int* skin_idx; const float* skin_w; int kb;
  float* out;                  // [T][200] (feat sweep) or [T][MESH_VJP_DA] (bone sweep)
  float* part;                 // [split][T][cols] scratch when the sweep is split over grid.y
  double* dtrans;              // feat sweep: [split][T][3], sum_v dV_v over the slice's vertices
  int T, V;
};
int mesh_vjp_feat_split(int T, int V);
int mesh_vjp_bone_split(int T, int V);
hipError_t launch_mesh_vjp_feat(const MeshVjpArgs& a, hipStream_t stream);
hipError_t launch_mesh_vjp_bone(const MeshVjpArgs& a, hipStream_t stream);
// Reverse kinematic chain (mesh_chain.hip, beside mesh_chain_kernel): one thread per frame recomputes the 22 global rotations
// and takes dA (bone sweep) and the joint cotangents back to d_rot, the rest-joint cotangents and d_trans.
struct MeshChainBwdArgs {
  const float* rot;            // [T][22][9]
  const float* jrest; int ld_j;    // rest joints [T][ld_j], n_joints * 3 used
  const int* parents;          // [n_joints]
  const float* dA;             // [T][MESH_VJP_DA] or nullptr
  const float* dJ;             // [T][n_joints][3] or nullptr
  const double* dtrans; int n_slices;   // [n_slices][T][3] (feat sweep) or nullptr
  float* d_rot;                // [T][22][9]
  float* d_jrest; int ld_dj;   // [T][ld_dj]; columns past n_joints * 3 are written as zeros
  float* g_trans;              // [T][3] or nullptr
  int T, n_joints;
};
hipError_t launch_mesh_chain_bwd(const MeshChainBwdArgs& a, hipStream_t stream);

struct VirtualSensorArgs {
  const float* vertices;   // [T][V][3]
  const int* center; const int* helper; const int* deg; const int* faces;  // [M], [M], [M], [M][max_deg][3] (mesh ids)
  float* pos; float* ori; float* normals;   // [T][M][3], [T][M][9], [T][M][3] (un-normalised) or nullptr
  int T, V, M, max_deg;
};
hipError_t launch_virtual_sensors(const VirtualSensorArgs& a, hipStream_t stream);
// Vector-Jacobian product of virtual_sensors_kernel (sensors_vjp.hip) for one slab of T frames: a sensor pass writes
// SENSOR_VJP_ROW floats per (frame, sensor) to `scratch` (dn / deg, the center's and the helper's cotangents), a vertex
// pass writes every element of d_vertices.  Reverse tables (api: empose_virtual_sensors_vjp): sub_faces [Fs][3],
// face_ptr [Fs + 1] / face_sensors (ascending), vf_ptr [V + 1] / vf_corner (f * 3 + k, ascending f), vs_ptr [V + 1] /
// vs_role (m * 2 + role, role 0 center, 1 helper, ascending), touched [n_touched].
constexpr int SENSOR_VJP_ROW = 9;
struct SensorVjpArgs {
  const float* vertices;   // [T][V][3]
  const int* center; const int* helper; const int* deg; const int* faces;   // the forward's tables
  const int* sub_faces; const int* face_ptr; const int* face_sensors;
  const int* vf_ptr; const int* vf_corner; const int* vs_ptr; const int* vs_role;
  const int* touched; int n_touched;   // the vertices with entries in vf / vs, ascending
  const float* d_pos; const float* d_ori; const float* d_normals;   // [T][M][3], [T][M][9], [T][M][3], each or nullptr
  float* scratch;          // [T][M][SENSOR_VJP_ROW]
  float* d_vertices;       // [T][V][3]
  int T, V, M, max_deg;
};
hipError_t launch_sensors_vjp(const SensorVjpArgs& a, hipStream_t stream);

}  // namespace empose
