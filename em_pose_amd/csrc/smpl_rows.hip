// SMPL-H on the sensor sub-mesh, general path: the per-frame kernels around the blend products.
//
//   pack_inputs    the network input columns of the sensors the model reads, and the per-frame loss weight
//   update_feat    theta/beta update of the LGD step (reference models.py:588-592), Rodrigues per joint
//                  (angle guard switchable: smplx ||r + 1e-8|| or the so3 clamp), GEMM feature row [vec(R_j - I) | beta | 1]
//   rodrigues_bwd  d R -> d theta, and the gradient features written into the network input row
//
// The chain between the two products is smpl_chain.hip; the frame-per-lane path has these bodies inside its blend GEMMs
// (feat_rows.h, mlp_fused.hip).
#include <cstdint>

#include "feat_rows.h"
#include "smpl_kernels.h"
#include "smpl_math.h"

namespace empose {

// ---------------------------------------------------------------------------------------------------------------
__global__ void pack_inputs_kernel(PackArgs a) {
  const int T = a.B * a.F;
  const int d_in = a.n_markers * 12;
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= T * (d_in + 1)) return;
  const int t = idx / (d_in + 1), c = idx % (d_in + 1);
  if (c == d_in) {
    if (!a.frame_scale) return;
    const int b = t / a.F, f = t % a.F;
    const int len = a.seq_lengths ? a.seq_lengths[b] : a.F;
    // reference: loss / n_frames, then grad * B * F  ->  F / len per valid frame (models.py:578-579, loss.py:36-39);
    // unpadded mode: every row is treated as a window of its own length (F == len), i.e. weight 1
    float s = (f < len) ? (a.rows_as_unpadded ? 1.f : (float)a.F / (float)len) : 0.f;
    if (a.marker_masks) {
      bool all = true;
      for (int m = 0; m < 12; ++m) all = all && (a.marker_masks[(size_t)t * 12 + m] != 0.f);
      if (!all) s = 0.f;
    }
    a.frame_scale[t] = s;
    return;
  }
  float v;
  int marker;
  if (c < a.n_markers * 3) {
    const int mi = c / 3, k = c % 3;
    marker = a.marker_idx[mi];
    v = a.marker_pos[(size_t)t * 36 + marker * 3 + k];
  } else {
    const int cc = c - a.n_markers * 3;
    const int mi = cc / 9, k = cc % 9;
    marker = a.marker_idx[mi];
    v = a.marker_oris[(size_t)t * 108 + marker * 9 + k];
  }
  if (a.suppress_missing && a.marker_masks) {   // the reference's arithmetic, so that a NaN reading stays a NaN
    const bool valid = a.marker_masks[(size_t)t * 12 + marker] == 1.f;
    v = v * (valid ? 1.f : 0.f) + (0.f + a.mask_value) * (valid ? 0.f : 1.f);
  }
  a.x[(size_t)t * a.ldx + c] = v;
}

// All twelve sensors in their own order and nothing to replace (the headline configuration): the input columns of a frame
// are its 36 position and 108 orientation values as they lie -- 36 pieces of 16 bytes per frame, no index arithmetic per
// element; thread 36 of a frame's group writes the frame weight.  (25.6 -> 13 us at 32768 frames.)
__global__ __launch_bounds__(256) void pack_inputs_all_kernel(PackArgs a) {
  const int T = a.B * a.F;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  const int t = (int)(idx / 37), q = (int)(idx - (long)t * 37);
  if (t >= T) return;
  if (q == 36) {
    if (!a.frame_scale) return;
    const int b = t / a.F, f = t - b * a.F;
    const int len = a.seq_lengths ? a.seq_lengths[b] : a.F;
    float s = (f < len) ? (a.rows_as_unpadded ? 1.f : (float)a.F / (float)len) : 0.f;
    if (a.marker_masks) {
      bool all = true;
      for (int m = 0; m < 12; ++m) all = all && (a.marker_masks[(size_t)t * 12 + m] != 0.f);
      if (!all) s = 0.f;
    }
    a.frame_scale[t] = s;
    return;
  }
  typedef float f4 __attribute__((ext_vector_type(4)));
  const f4 v = q < 9 ? reinterpret_cast<const f4*>(a.marker_pos + (size_t)t * 36)[q]
                     : reinterpret_cast<const f4*>(a.marker_oris + (size_t)t * 108)[q - 9];
  reinterpret_cast<f4*>(a.x + (size_t)t * a.ldx)[q] = v;
}

hipError_t launch_pack_inputs(const PackArgs& a, hipStream_t stream) {
  bool plain = a.n_markers == 12 && !(a.suppress_missing && a.marker_masks) && a.ldx % 4 == 0 &&
               (((uintptr_t)a.marker_pos | (uintptr_t)a.marker_oris | (uintptr_t)a.x) & 15) == 0;
  for (int i = 0; i < 12; ++i) plain = plain && a.marker_idx[i] == i;
  if (plain) {
    const long n37 = (long)a.B * a.F * 37;
    hipLaunchKernelGGL(pack_inputs_all_kernel, dim3((unsigned)((n37 + 255) / 256)), dim3(256), 0, stream, a);
    return hipGetLastError();
  }
  const long n = (long)a.B * a.F * (a.n_markers * 12 + 1);
  hipLaunchKernelGGL(pack_inputs_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, a);
  return hipGetLastError();
}

// One thread per (frame, slot): slots 0..21 are joints, 22..31 the ten shape coefficients.  The two wide outputs (rot:
// 198 floats per frame, feat: 200) are assembled in LDS and written out by the whole block as contiguous 8 / 16-byte
// pieces; a lane writing its nine floats at a 36-byte stride reached 2.9 TB/s.
constexpr int UF_FRAMES = 8;   // frames per 256-thread block
__global__ __launch_bounds__(256) void update_feat_kernel(FeatArgs a) {
  __shared__ __attribute__((aligned(16))) float s_rot[UF_FRAMES * NB * 9];
  __shared__ __attribute__((aligned(16))) float s_feat[UF_FRAMES * 200];
  const int t0 = blockIdx.x * UF_FRAMES;
  const int fl = threadIdx.x >> 5, slot = threadIdx.x & 31;
  feat_frame(a, t0 + fl, slot, s_feat + fl * 200, s_rot + fl * NB * 9);   // feat_rows.h
  __syncthreads();
  // the block's frames are contiguous in both outputs
  const int nf = min(UF_FRAMES, a.T - t0);
  if (a.rot) {   // (the frame-per-lane kernel evaluates the rotations itself)
    const float2* src = reinterpret_cast<const float2*>(s_rot);
    float2* dst = reinterpret_cast<float2*>(a.rot + (size_t)t0 * NB * 9);   // 198 floats per frame: 8-byte pieces
    for (int i = threadIdx.x; i < nf * (NB * 9 / 2); i += 256) dst[i] = src[i];
  }
  {
    const float4* src = reinterpret_cast<const float4*>(s_feat);
    float4* dst = reinterpret_cast<float4*>(a.feat + (size_t)t0 * 200);
    for (int i = threadIdx.x; i < nf * 50; i += 256) dst[i] = src[i];
  }
}

hipError_t launch_update_feat(const FeatArgs& a, hipStream_t stream) {
  hipLaunchKernelGGL(update_feat_kernel, dim3((unsigned)((a.T + UF_FRAMES - 1) / UF_FRAMES)), dim3(256), 0, stream, a);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------
__global__ void rodrigues_bwd_kernel(RodBwdArgs a) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  const int t = idx >> 5, slot = idx & 31;
  if (t >= a.T) return;
  if (slot < NB) {
    const float* th = a.theta + (size_t)t * a.ld_theta + slot * 3;
    Rod q; float R[9];
    rodrigues(th[0], th[1], th[2], a.rod_conv, q, R);
    float dR[9];
    const float* dr = a.d_rot + ((size_t)t * NB + slot) * 9;
#pragma unroll
    for (int e = 0; e < 9; ++e) dR[e] = dr[e];
    if (slot >= 1) {
      const float* df = a.d_feat + (size_t)t * 200 + (slot - 1) * 9;
#pragma unroll
      for (int e = 0; e < 9; ++e) dR[e] += df[e];
    }
    // K and K^2
    const float K[9] = {0.f, -q.dz, q.dy, q.dz, 0.f, -q.dx, -q.dy, q.dx, 0.f};
    const float KK[9] = {-q.dz * q.dz - q.dy * q.dy, q.dx * q.dy, q.dx * q.dz,
                         q.dx * q.dy, -q.dz * q.dz - q.dx * q.dx, q.dy * q.dz,
                         q.dx * q.dz, q.dy * q.dz, -q.dy * q.dy - q.dx * q.dx};
    float ds = 0.f, dc1 = 0.f;
#pragma unroll
    for (int e = 0; e < 9; ++e) { ds += dR[e] * K[e]; dc1 += dR[e] * KK[e]; }
    const float oc = 1.f - q.c;
    // dK = s dR + (1-c) (dR K^T + K^T dR)
    float dK[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        float m = 0.f;
#pragma unroll
        for (int k = 0; k < 3; ++k) m += dR[r * 3 + k] * K[c * 3 + k] + K[k * 3 + r] * dR[k * 3 + c];
        dK[r * 3 + c] = q.s * dR[r * 3 + c] + oc * m;
      }
    const float ddx = dK[7] - dK[5], ddy = dK[2] - dK[6], ddz = dK[3] - dK[1];
    float da = ds * q.c + dc1 * q.s;
    da -= (ddx * q.dx + ddy * q.dy + ddz * q.dz) / q.ang;
    const float g0 = ddx / q.ang + da * q.ux / q.ang;
    const float g1 = ddy / q.ang + da * q.uy / q.ang;
    const float g2 = ddz / q.ang + da * q.uz / q.ang;
    float* g = a.g_theta + (size_t)t * a.ld_g + slot * 3;
    g[0] = g0; g[1] = g1; g[2] = g2;
    if (a.trace_g_theta) { float* o = a.trace_g_theta + (size_t)t * 66 + slot * 3; o[0] = g0; o[1] = g1; o[2] = g2; }
  } else {
    const int k = slot - NB;
    const float v = a.d_feat[(size_t)t * 200 + 189 + k];
    a.g_beta[(size_t)t * a.ld_gb + k] = v;
    if (a.trace_g_beta) a.trace_g_beta[(size_t)t * 10 + k] = v;
  }
}

hipError_t launch_rodrigues_bwd(const RodBwdArgs& a, hipStream_t stream) {
  const long n = (long)a.T * 32;
  hipLaunchKernelGGL(rodrigues_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, a);
  return hipGetLastError();
}

}  // namespace empose
