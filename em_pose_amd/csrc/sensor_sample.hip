// Synthetic sensor sampling (data/transforms.py SampleMarkersWithOffsets, reference transforms.py:132-226), gfx950 only.
//
// Forward, one launch, one lane per (frame t, sensor m): the frame of virtual_sensors_kernel (sensor_frame.h: pos = the
// sensor vertex, ori = [tangent | bitangent | normal], n the un-normalised normal) and, with i = t / F the window,
//   pos_synth = pos + ori . local     local = local[i][m], local[t][m] or 0 by mode
//   ori_synth = ori . r[i][m]         (r NULL: ori)
//   normal_synth = the third column of ori_synth
// Every output is optional.  A lane reads its sensor's fan (about 7 vertices) and writes at most 36 floats: the launch is
// bound by its latency, not by bandwidth, at every batch size training uses.
//
// Reverse: local and r are constants, so the cotangents of the three synth outputs fold into those of (pos, ori),
//   d_pos = d_pos_synth,   d_ori = d_pos_synth (x) local + (d_ori_synth + d_normal_synth in column 2) . r^T,
// one lane per (frame, sensor), added to the cotangents of the un-offset outputs where given; the sensor and vertex
// passes of sensors_vjp.hip take it from there (api_sample.hip).  No atomics: repeated calls give the same bits.
#include <hip/hip_runtime.h>

#include "data_kernels.h"
#include "sensor_frame.h"

namespace empose {

namespace {

constexpr int SS_THREADS = 128;

// The offset of (frame t of the batch, sensor m), or nullptr.
__device__ __forceinline__ const float* local_of(const float* local, int mode, int t, int F, int M, int m) {
  if (mode == SAMPLE_LOCAL_WINDOW) return local + ((size_t)(t / F) * M + m) * 3;
  if (mode == SAMPLE_LOCAL_FRAME) return local + ((size_t)t * M + m) * 3;
  return nullptr;
}

__global__ void __launch_bounds__(SS_THREADS) sample_sensors_kernel(SampleSensorsArgs a) {
  const long idx = (long)blockIdx.x * SS_THREADS + threadIdx.x;
  if (idx >= (long)a.T * a.M) return;
  const int t = (int)(idx / a.M), m = (int)(idx - (long)t * a.M);
  const float* V = a.vertices + (size_t)t * a.V * 3;
  const int center = a.center[m];
  float n[3], ori[9];
  sensor_frame(V, a.faces + (size_t)m * a.max_deg * 3, a.deg[m], center, a.helper[m], n, ori);
  const float* vc = V + (size_t)center * 3;
  const size_t row = (size_t)idx;
  if (a.pos)
    for (int r = 0; r < 3; ++r) a.pos[row * 3 + r] = vc[r];
  if (a.ori)
    for (int e = 0; e < 9; ++e) a.ori[row * 9 + e] = ori[e];
  if (a.normals)
    for (int r = 0; r < 3; ++r) a.normals[row * 3 + r] = n[r];
  if (a.pos_synth) {
    const float* l = local_of(a.local, a.mode, t, a.F, a.M, m);
    for (int r = 0; r < 3; ++r)
      a.pos_synth[row * 3 + r] = l ? vc[r] + (ori[r * 3 + 0] * l[0] + ori[r * 3 + 1] * l[1] + ori[r * 3 + 2] * l[2]) : vc[r];
  }
  if (a.ori_synth || a.normal_synth) {
    float os[9];
    if (a.r) {
      const float* R = a.r + ((size_t)(t / a.F) * a.M + m) * 9;
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c)
          os[r * 3 + c] = ori[r * 3 + 0] * R[c] + ori[r * 3 + 1] * R[3 + c] + ori[r * 3 + 2] * R[6 + c];
    } else {
      for (int e = 0; e < 9; ++e) os[e] = ori[e];
    }
    if (a.ori_synth)
      for (int e = 0; e < 9; ++e) a.ori_synth[row * 9 + e] = os[e];
    if (a.normal_synth)
      for (int r = 0; r < 3; ++r) a.normal_synth[row * 3 + r] = os[r * 3 + 2];
  }
}

__global__ void __launch_bounds__(SS_THREADS) sample_fold_kernel(SampleFoldArgs a) {
  const long idx = (long)blockIdx.x * SS_THREADS + threadIdx.x;
  if (idx >= (long)a.T * a.M) return;
  const int ts = (int)(idx / a.M), m = (int)(idx - (long)ts * a.M);
  const int t = a.t0 + ts;   // the frame of the batch
  const size_t row = (size_t)idx;
  if (a.d_pos_out)
    for (int r = 0; r < 3; ++r) {
      float s = a.d_pos_synth ? a.d_pos_synth[row * 3 + r] : 0.f;
      if (a.d_pos) s += a.d_pos[row * 3 + r];
      a.d_pos_out[row * 3 + r] = s;
    }
  if (!a.d_ori_out) return;
  // G = d_ori_synth + d_normal_synth in column 2
  float G[9];
  for (int e = 0; e < 9; ++e) G[e] = a.d_ori_synth ? a.d_ori_synth[row * 9 + e] : 0.f;
  if (a.d_normal_synth)
    for (int r = 0; r < 3; ++r) G[r * 3 + 2] += a.d_normal_synth[row * 3 + r];
  float d[9];
  if (a.r && (a.d_ori_synth || a.d_normal_synth)) {
    const float* R = a.r + ((size_t)(t / a.F) * a.M + m) * 9;
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c)   // (G . R^T)[r][c] = sum_k G[r][k] R[c][k]
        d[r * 3 + c] = G[r * 3 + 0] * R[c * 3 + 0] + G[r * 3 + 1] * R[c * 3 + 1] + G[r * 3 + 2] * R[c * 3 + 2];
  } else {
    for (int e = 0; e < 9; ++e) d[e] = G[e];
  }
  const float* l = a.d_pos_synth ? local_of(a.local, a.mode, t, a.F, a.M, m) : nullptr;
  if (l)
    for (int r = 0; r < 3; ++r) {
      const float g = a.d_pos_synth[row * 3 + r];
      for (int c = 0; c < 3; ++c) d[r * 3 + c] += g * l[c];
    }
  if (a.d_ori)
    for (int e = 0; e < 9; ++e) d[e] += a.d_ori[row * 9 + e];
  for (int e = 0; e < 9; ++e) a.d_ori_out[row * 9 + e] = d[e];
}

inline unsigned blocks_of(long lanes) { return (unsigned)((lanes + SS_THREADS - 1) / SS_THREADS); }

}  // namespace

hipError_t launch_sample_sensors(const SampleSensorsArgs& a, hipStream_t stream) {
  hipLaunchKernelGGL(sample_sensors_kernel, dim3(blocks_of((long)a.T * a.M)), dim3(SS_THREADS), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_sample_fold(const SampleFoldArgs& a, hipStream_t stream) {
  hipLaunchKernelGGL(sample_fold_kernel, dim3(blocks_of((long)a.T * a.M)), dim3(SS_THREADS), 0, stream, a);
  return hipGetLastError();
}

}  // namespace empose
