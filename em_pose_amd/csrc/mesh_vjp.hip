// Full-mesh vector-Jacobian product: the two vertex sweeps of the reverse of mesh_rows_kernel (mesh_rows.hip), gfx950 only.
//
// Forward, per frame: vp = wc[0:3V] . feat (v_posed), v = sum_b w_vb A_b [vp; 1] + trans.  For a cotangent dV:
//   feat sweep  d_feat = sum_v,c dvp[v][c] wc[3v+c][:] with dvp_v = sum_b w_vb (A_b^R)^T dV_v
//   bone sweep  dA_b = sum_v w_vb dV_v [vp_v; 1]^T
// and, in the feat sweep, sum_v dV_v (the translation's share) in double precision: a float sum of 6890 cotangents in a
// few long chains lost ten times more than float autograd's pairwise sum
// Both keep the forward's design rule: neither v_posed nor dvp exists in memory.  A workgroup owns 32 frames, its waves
// walk the 32-vertex tiles, and every contraction runs on the fp32 matrix cores (v_mfma_f32_32x32x2_f32, exact fp32
// products).  A wave first copies its tile's cotangents, 32 frames x 96 floats, into a private LDS block with coalesced
// loads; the products then read them with frames on `lane & 31`, which is where both contractions want the frames.
//
// feat sweep: C[frame][feature] over k = the tile's 96 (vertex, coordinate) rows.  The A operand is dvp itself: the lane
// of frame f and half h gathers the blended rotation of vertex 16h + p (four bones from LDS, as the forward's skinning)
// and forms dvp for the three coordinates in registers; B is wc in fragment order (api_mesh.hip pack_mesh_vjp).  Seven
// 32-column accumulators cover the 200 features.  Eight waves, 140 KB of LDS: one workgroup per CU, two waves per SIMD.
// bone sweep: vp is recomputed with the forward's contraction laid out as C[vertex][frame] (wc_frag as the A operand,
// the staged features as B), so a lane ends up with the frame `lane & 31` of 16 vertices -- exactly the A operand of
// C[frame][bone] = sum_v X[frame][v] W[v][bone] for the twelve X = dV[r] * [vp; 1][c]: no transpose.  B is a dense
// [32 vertices][32 bone slots] weight table per tile.  12 x 16 accumulator registers: four waves, one per SIMD.
// The waves' partial sums are added in wave order through LDS; a sweep split over grid.y adds its slices in slot order.
#include <hip/hip_runtime.h>

#include "gemm_epilogue.h"
#include "launch.h"
#include "mesh_kernels.h"
#include "smpl_kernels.h"

namespace empose {

namespace mv {
constexpr int BM = MESH_VJP_BM;
constexpr int DLD = 97;                      // staged cotangents: floats per frame (odd: lanes of consecutive frames
                                             // read different banks)
constexpr int DV_FLOATS = BM * DLD;          // one wave's block
constexpr int XLD = NB * 12 + 4;             // transforms: floats per frame (268: 16-byte reads of 8 consecutive frames
                                             // fall on disjoint banks)
constexpr int FNW = 8;                       // feat sweep: waves per workgroup
constexpr int FRLD = 228;                    // feat sweep reduction block: floats per frame
constexpr size_t F_LDS_BYTES = (size_t)(BM * XLD + FNW * DV_FLOATS) * sizeof(float);
constexpr int BNW = 4;                       // bone sweep
constexpr int K = 200, KG = K / 8, LDA = K + 4;
constexpr int BRLD = MESH_VJP_DA + 1;
constexpr size_t B_LDS_BYTES = (size_t)(BM * LDA + BNW * DV_FLOATS) * sizeof(float);
static_assert(BM * FRLD + BM * 2 * FNW * 3 * 2 <= FNW * DV_FLOATS, "feat reduction blocks alias the staging blocks");
static_assert(BM * FRLD % 2 == 0, "double block alignment");
static_assert(BM * BRLD <= BNW * DV_FLOATS, "bone reduction block aliases the staging blocks");
}  // namespace mv

// Wave-private LDS hand-off between lanes: a wave's LDS operations execute in order; this keeps the compiler from
// moving its reads above its writes.
__device__ __forceinline__ void mv_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The cotangents of tile vt for the block's 32 frames into the wave's block Dw[frame][vertex * 3 + c] (coalesced: 64
// consecutive floats per load).  Frames past T and vertices past V are zero.
__device__ __forceinline__ void mv_stage_dv(float* Dw, const float* __restrict__ dv, int f0, int vt, int T, int V,
                                           int lane) {
  const int n_valid = min(96, (V - vt * 32) * 3);
#pragma unroll 8
  for (int it = 0; it < mv::BM * 96 / 64; ++it) {
    const int idx = it * 64 + lane;
    const int f = idx / 96, k = idx - f * 96;
    float x = 0.f;
    if (f0 + f < T && k < n_valid) x = dv[((size_t)(f0 + f) * V + (size_t)vt * 32) * 3 + k];
    Dw[f * mv::DLD + k] = x;
  }
}

// The slice of tiles this workgroup's waves walk.
__device__ __forceinline__ void mv_tile_range(int V, int* first, int* end) {
  const int n_tiles = (V + 31) / 32;
  const int per_block = (n_tiles + gridDim.y - 1) / gridDim.y;
  *first = blockIdx.y * per_block;
  *end = min(*first + per_block, n_tiles);
}

template <bool EXTRA>   // EXTRA: more than four bones per vertex
__global__ __launch_bounds__(mv::FNW * 64) void mesh_vjp_feat_kernel(MeshVjpArgs a) {
  using namespace mv;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* XFs = lds;
  float* Dvs = lds + BM * XLD;
  const int T = a.T, V = a.V;
  const int f0 = blockIdx.x * BM;
  const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, lh = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

  for (int i = tid; i < BM * NB * 3; i += FNW * 64) {   // transforms (rows past T repeat row T-1; their dV is zero)
    const int r = i / (NB * 3), c = i % (NB * 3);
    const int row = f0 + r < T ? f0 + r : T - 1;
    *reinterpret_cast<f32x4*>(XFs + r * XLD + c * 4) = *reinterpret_cast<const f32x4*>(a.xf + ((size_t)row * NB * 3 + c) * 4);
  }
  __syncthreads();

  int first, end;
  mv_tile_range(V, &first, &end);
  f32x16 acc[7];
#pragma unroll
  for (int ct = 0; ct < 7; ++ct)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[ct][r] = 0.f;

  double ts[3] = {0.0, 0.0, 0.0};   // sum of this lane's cotangents (frame l31, vertices 16 lh .. + 15 of each tile)
  float* Dw = Dvs + wave * DV_FLOATS;
  const float* xf_lane = XFs + l31 * XLD;
  const float* dv_lane = Dw + l31 * DLD + lh * 48;
  const int kb = a.kb;
  for (int vt = first + wave; vt < end; vt += FNW) {
    mv_stage_dv(Dw, a.dv, f0, vt, T, V, lane);
    mv_wave_sync();
    const f32x4* wt = reinterpret_cast<const f32x4*>(a.wc_vjp + (size_t)vt * MESH_VJP_WC_TILE_FLOATS) + lane;
    f32x4 b[6];
#pragma unroll
    for (int q = 0; q < 6; ++q) b[q] = wt[q * 64];
#pragma unroll 2
    for (int p = 0; p < 16; ++p) {
      // this lane's vertex (16 lh + p) and frame (l31): dvp = (sum_k w_k G_k^R)^T dV
      const int s = vt * 32 + lh * 16 + p;
      const int4 bone4 = *reinterpret_cast<const int4*>(a.skin_idx4 + (size_t)s * 4);
      const f32x4 w4 = *reinterpret_cast<const f32x4*>(a.skin_w4 + (size_t)s * 4);
      const int bk[4] = {bone4.x, bone4.y, bone4.z, bone4.w};
      float M[3][3];
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        f32x4 g = *reinterpret_cast<const f32x4*>(xf_lane + bk[0] * 12 + r * 4);
        M[r][0] = w4[0] * g[0]; M[r][1] = w4[0] * g[1]; M[r][2] = w4[0] * g[2];
#pragma unroll
        for (int k = 1; k < 4; ++k) {
          g = *reinterpret_cast<const f32x4*>(xf_lane + bk[k] * 12 + r * 4);
          M[r][0] = __builtin_fmaf(w4[k], g[0], M[r][0]);
          M[r][1] = __builtin_fmaf(w4[k], g[1], M[r][1]);
          M[r][2] = __builtin_fmaf(w4[k], g[2], M[r][2]);
        }
      }
      if (EXTRA && s < V)
        for (int k = 4; k < kb; ++k) {
          const int bb = a.skin_idx[(size_t)s * kb + k];
          const float wk = a.skin_w[(size_t)s * kb + k];
#pragma unroll
          for (int r = 0; r < 3; ++r) {
            const f32x4 g = *reinterpret_cast<const f32x4*>(xf_lane + bb * 12 + r * 4);
            M[r][0] = __builtin_fmaf(wk, g[0], M[r][0]);
            M[r][1] = __builtin_fmaf(wk, g[1], M[r][1]);
            M[r][2] = __builtin_fmaf(wk, g[2], M[r][2]);
          }
        }
      const float d0 = dv_lane[p * 3], d1 = dv_lane[p * 3 + 1], d2 = dv_lane[p * 3 + 2];
      ts[0] += d0; ts[1] += d1; ts[2] += d2;
      float dvp[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) dvp[c] = __builtin_fmaf(M[0][c], d0, __builtin_fmaf(M[1][c], d1, M[2][c] * d2));
      // B fragments of the next vertex pair (the last one re-reads this tile's first: never consumed)
      f32x4 bn[6];
      const int pn = p + 1 < 16 ? p + 1 : 0;
#pragma unroll
      for (int q = 0; q < 6; ++q) bn[q] = wt[(pn * 6 + q) * 64];
#pragma unroll
      for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int ct = 0; ct < 7; ++ct)
          acc[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(dvp[c], b[(c * 8 + ct) >> 2][(c * 8 + ct) & 3], acc[ct], 0, 0, 0);
#pragma unroll
      for (int q = 0; q < 6; ++q) b[q] = bn[q];
    }
    mv_wave_sync();   // the next tile's staging overwrites the block
  }

  // partial sums of the waves, added in wave order (the block aliases the staging blocks: every wave is past its tiles)
  float* Red = Dvs;
  for (int w = 0; w < FNW; ++w) {
    __syncthreads();
    if (wave == w) {
#pragma unroll
      for (int ct = 0; ct < 7; ++ct)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          float* o = Red + ((r & 3) + 8 * (r >> 2) + 4 * lh) * FRLD + ct * 32 + l31;
          *o = w == 0 ? acc[ct][r] : *o + acc[ct][r];
        }
    }
  }
  double* Red2 = reinterpret_cast<double*>(Red + BM * FRLD);   // [frame][16 = wave x half][3]
#pragma unroll
  for (int c = 0; c < 3; ++c) Red2[(l31 * 16 + wave * 2 + lh) * 3 + c] = ts[c];
  __syncthreads();
  float* out = gridDim.y > 1 ? a.part + (size_t)blockIdx.y * T * K : a.out;
  for (int i = tid; i < BM * K; i += FNW * 64) {
    const int f = i / K, k = i - f * K;
    if (f0 + f < T) out[(size_t)(f0 + f) * K + k] = Red[f * FRLD + k];
  }
  if (tid < BM * 3 && f0 + tid / 3 < T) {
    const int f = tid / 3, c = tid - f * 3;
    double s = 0.0;
    for (int q = 0; q < 2 * FNW; ++q) s += Red2[(f * 16 + q) * 3 + c];
    a.dtrans[((size_t)blockIdx.y * T + f0 + f) * 3 + c] = s;
  }
}

__global__ __launch_bounds__(mv::BNW * 64) void mesh_vjp_bone_kernel(MeshVjpArgs a) {
  using namespace mv;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* As = lds;
  float* Dvs = lds + BM * LDA;
  const int T = a.T, V = a.V;
  const int f0 = blockIdx.x * BM;
  const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, lh = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

  for (int i = tid; i < BM * (K / 4); i += BNW * 64) {   // features (rows past T repeat row T-1; their dV is zero)
    const int r = i / (K / 4), c = (i % (K / 4)) * 4;
    const int row = f0 + r < T ? f0 + r : T - 1;
    *reinterpret_cast<f32x4*>(As + r * LDA + c) = *reinterpret_cast<const f32x4*>(a.feat + (size_t)row * K + c);
  }
  __syncthreads();

  int first, end;
  mv_tile_range(V, &first, &end);
  f32x16 dA[12];
#pragma unroll
  for (int q = 0; q < 12; ++q)
#pragma unroll
    for (int r = 0; r < 16; ++r) dA[q][r] = 0.f;
  // The translation columns (q = 3, 7, 11: sum_v w_vb dV_v) are summed in two levels, a tile's MFMA chain, then the
  // running total per tile: shorter rounding chains than one chain over all of a wave's tiles.
  f32x16 dAt[3];
#pragma unroll
  for (int q = 0; q < 3; ++q)
#pragma unroll
    for (int r = 0; r < 16; ++r) dAt[q][r] = 0.f;

  float* Dw = Dvs + wave * DV_FLOATS;
  const float* a_lane = As + l31 * LDA + lh * 4;
  const float* dv_lane = Dw + l31 * DLD;
  for (int vt = first + wave; vt < end; vt += BNW) {
    mv_stage_dv(Dw, a.dv, f0, vt, T, V, lane);
    // vp^T = wc_frag . feat^T: C[vertex][frame], a lane holds frame l31 of vertices (r & 3) + 8 (r >> 2) + 4 lh
    const f32x4* wf = reinterpret_cast<const f32x4*>(a.wc_frag + (size_t)vt * (KG * 3 * 256)) + lane;
    f32x16 vp[3];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int r = 0; r < 16; ++r) vp[c][r] = 0.f;
#pragma unroll 5
    for (int g = 0; g < KG; ++g) {
      const f32x4 fb = *reinterpret_cast<const f32x4*>(a_lane + g * 8);
      f32x4 w[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) w[c] = wf[(g * 3 + c) * 64];
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int c = 0; c < 3; ++c) vp[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[c][e], fb[e], vp[c], 0, 0, 0);
    }
    mv_wave_sync();
    const f32x4* st = reinterpret_cast<const f32x4*>(a.skin_dense + (size_t)vt * MESH_VJP_SKIN_TILE_FLOATS) + lane;
    f32x4 wd[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) wd[q] = st[q * 64];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int vr = (r & 3) + 8 * (r >> 2) + 4 * lh;
      const float d[3] = {dv_lane[vr * 3], dv_lane[vr * 3 + 1], dv_lane[vr * 3 + 2]};
      const float wv = wd[r >> 2][r & 3];
#pragma unroll
      for (int rr = 0; rr < 3; ++rr)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const float x = c < 3 ? d[rr] * vp[c][r] : d[rr];
          dA[rr * 4 + c] = __builtin_amdgcn_mfma_f32_32x32x2f32(x, wv, dA[rr * 4 + c], 0, 0, 0);
        }
    }
#pragma unroll
    for (int rr = 0; rr < 3; ++rr) {
      dAt[rr] += dA[rr * 4 + 3];
#pragma unroll
      for (int r = 0; r < 16; ++r) dA[rr * 4 + 3][r] = 0.f;
    }
    mv_wave_sync();
  }
#pragma unroll
  for (int rr = 0; rr < 3; ++rr) dA[rr * 4 + 3] = dAt[rr];

  float* Red = Dvs;
  for (int w = 0; w < BNW; ++w) {
    __syncthreads();
    if (wave == w && l31 < NB) {   // bone slots 0..21
#pragma unroll
      for (int q = 0; q < 12; ++q)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          float* o = Red + ((r & 3) + 8 * (r >> 2) + 4 * lh) * BRLD + l31 * 12 + q;
          *o = w == 0 ? dA[q][r] : *o + dA[q][r];
        }
    }
  }
  __syncthreads();
  float* out = gridDim.y > 1 ? a.part + (size_t)blockIdx.y * T * MESH_VJP_DA : a.out;
  for (int i = tid; i < BM * MESH_VJP_DA; i += BNW * 64) {
    const int f = i / MESH_VJP_DA, k = i - f * MESH_VJP_DA;
    if (f0 + f < T) out[(size_t)(f0 + f) * MESH_VJP_DA + k] = Red[f * BRLD + k];
  }
}

// out[t][k] = sum over the slices s (in order) of part[s][t][k]
__global__ void mesh_vjp_sum_kernel(const float* __restrict__ part, float* __restrict__ out, int n_slices, long count) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  float s = part[i];
  for (int k = 1; k < n_slices; ++k) s += part[(size_t)k * count + i];
  out[i] = s;
}

namespace {
// Fewer than one workgroup per CU: split the tiles over grid.y (at least one tile per wave), as launch_mesh_rows does.
int vjp_split(int T, int V, int nw) {
  const int bx = (T + mv::BM - 1) / mv::BM;
  int by = bx >= 256 ? 1 : (256 + bx - 1) / bx;
  const int max_by = ((V + 31) / 32 + nw - 1) / nw;
  return by > max_by ? max_by : by;
}

hipError_t sum_slices(const MeshVjpArgs& a, int by, int cols, hipStream_t stream) {
  const long count = (long)a.T * cols;
  hipLaunchKernelGGL(mesh_vjp_sum_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, stream, a.part, a.out, by,
                     count);
  return hipGetLastError();
}
}  // namespace

int mesh_vjp_feat_split(int T, int V) { return vjp_split(T, V, mv::FNW); }
int mesh_vjp_bone_split(int T, int V) { return vjp_split(T, V, mv::BNW); }

hipError_t launch_mesh_vjp_feat(const MeshVjpArgs& a, hipStream_t stream) {
  const int bx = (a.T + mv::BM - 1) / mv::BM, by = mesh_vjp_feat_split(a.T, a.V);
  if (by > 1 && !a.part) return hipErrorInvalidValue;
  if (hipError_t e = a.kb <= 4
          ? launch_lds(mesh_vjp_feat_kernel<false>, dim3(bx, by), dim3(mv::FNW * 64), mv::F_LDS_BYTES, stream, a)
          : launch_lds(mesh_vjp_feat_kernel<true>, dim3(bx, by), dim3(mv::FNW * 64), mv::F_LDS_BYTES, stream, a))
    return e;
  return by > 1 ? sum_slices(a, by, 200, stream) : hipSuccess;
}

hipError_t launch_mesh_vjp_bone(const MeshVjpArgs& a, hipStream_t stream) {
  const int bx = (a.T + mv::BM - 1) / mv::BM, by = mesh_vjp_bone_split(a.T, a.V);
  if (by > 1 && !a.part) return hipErrorInvalidValue;
  if (hipError_t e = launch_lds(mesh_vjp_bone_kernel, dim3(bx, by), dim3(mv::BNW * 64), mv::B_LDS_BYTES, stream, a)) return e;
  return by > 1 ? sum_slices(a, by, MESH_VJP_DA, stream) : hipSuccess;
}

}  // namespace empose
