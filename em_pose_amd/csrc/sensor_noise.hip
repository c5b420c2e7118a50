// Sensor-noise augmentation of the training data path (reference data/noise_functions.py:40-164), gfx950 only, fp32.
// The draws are the host's (the reference's seeded generators); this is the write over N windows x F frames x M sensors.
//
// Gather form, one launch: every output float looks its (window, frame, sensor) up in the plan, decides whether it is
// affected, and is written exactly once -- no scatter, no atomics, so a sensor id named twice in the plan is harmless and
// a result depends neither on the rest of the batch nor on the launch geometry.  Threads run over the output buffers in
// memory order (position rows, then orientation rows, then normal rows): consecutive lanes, consecutive floats.
//
//   suppression  window i, frames start[i] <= f < start[i] + window_len, sensors sensor[i][0..K): the 3 + 9 + 3 floats
//                become mask_value; everything else is a bit copy.
//   spherical    the same frames, the K sensors sensor[0..K) shared by all windows: the position gets
//                (r cos(theta) sin(phi), r sin(theta) cos(phi), r cos(phi)) added -- the reference's formula as written,
//                cos(phi) in y included --, r = u_r * max_r * thigh / 2, thigh = |pos[0][F / 2][a] - pos[0][0][b]| read
//                here from the input (the two different frames are the reference's).  u_r, theta, phi: [N][window_len][K].
//                Products and sums are rounded one by one, as the reference's tensor operations round them.  Where the
//                plan names a sensor twice, the last entry counts.  Orientation and normal are not touched.
#include <hip/hip_runtime.h>

#include "data_kernels.h"

namespace empose {

namespace {

constexpr int SN_THREADS = 256;

// The plan entry of `sensor` among ids[0..K), the last one that names it, or -1.
__device__ __forceinline__ int plan_entry(const int* ids, int K, int sensor) {
  int at = -1;
  for (int k = 0; k < K; ++k) at = ids[k] == sensor ? k : at;
  return at;
}

__device__ __forceinline__ float thigh_length(const SensorNoiseArgs& a) {
#pragma clang fp contract(off)
  const float* p = a.pos + ((long)(a.F / 2) * a.M + a.thigh_a) * 3;
  const float* q = a.pos + (long)a.thigh_b * 3;
  const float dx = p[0] - q[0], dy = p[1] - q[1], dz = p[2] - q[2];
  return sqrtf(dx * dx + dy * dy + dz * dz);
}

// One float of a buffer of rows of M sensors x C floats: which window, which frame of it, which sensor, which float.
struct Where { int n, f, sensor, c; };
__device__ __forceinline__ Where where_of(long e, int F, int M, int C) {
  const long row = e / ((long)M * C);
  const int col = (int)(e - row * ((long)M * C));
  return {(int)(row / F), (int)(row % F), col / C, col % C};
}

__global__ void __launch_bounds__(SN_THREADS) sensor_noise_kernel(SensorNoiseArgs a) {
  const long rows = (long)a.N * a.F;
  const long n_pos = rows * a.M * 3, n_ori = a.mode == SENSOR_NOISE_SUPPRESS ? rows * a.M * 9 : 0;
  const long total = n_pos + n_ori + (a.mode == SENSOR_NOISE_SUPPRESS ? n_pos : 0);
  const long e = (long)blockIdx.x * SN_THREADS + threadIdx.x;
  if (e >= total) return;
  if (a.mode == SENSOR_NOISE_SUPPRESS) {
    const float* in = a.pos; float* out = a.pos_out; long at = e; int C = 3;
    if (e >= n_pos + n_ori) { in = a.normal; out = a.normal_out; at = e - n_pos - n_ori; }
    else if (e >= n_pos) { in = a.ori; out = a.ori_out; at = e - n_pos; C = 9; }
    const Where w = where_of(at, a.F, a.M, C);
    const int s = a.start[w.n];
    const bool hit = w.f >= s && w.f < s + a.window_len && plan_entry(a.sensor + (long)w.n * a.K, a.K, w.sensor) >= 0;
    out[at] = hit ? a.mask_value : in[at];
    return;
  }
  const Where w = where_of(e, a.F, a.M, 3);
  const int s = a.start[w.n];
  float v = a.pos[e];
  if (w.f >= s && w.f < s + a.window_len) {
    const int k = plan_entry(a.sensor, a.K, w.sensor);
    if (k >= 0) {
#pragma clang fp contract(off)
      const long d = ((long)w.n * a.window_len + (w.f - s)) * a.K + k;
      const float r = a.u_r[d] * a.max_r * thigh_length(a) * 0.5f;
      const float th = a.theta[d], ph = a.phi[d];
      const float add = w.c == 0 ? r * cosf(th) * sinf(ph) : (w.c == 1 ? r * sinf(th) * cosf(ph) : r * cosf(ph));
      v = v + add;
    }
  }
  a.pos_out[e] = v;
}

}  // namespace

hipError_t launch_sensor_noise(const SensorNoiseArgs& a, hipStream_t stream) {
  const long per_row = a.mode == SENSOR_NOISE_SUPPRESS ? 15 : 3;
  const long total = (long)a.N * a.F * a.M * per_row;
  const long grid = (total + SN_THREADS - 1) / SN_THREADS;   // (the entry point keeps this below 2^31)
  hipLaunchKernelGGL(sensor_noise_kernel, dim3((unsigned)grid), dim3(SN_THREADS), 0, stream, a);
  return hipGetLastError();
}

}  // namespace empose
