// Per-subject sensor offsets from calibration recordings (data/offsets.py), gfx950 only: the inverse of synthetic sensor
// sampling (sensor_sample.hip).  The definition is this project's own; per frame f and sensor m, with
// (pos, ori) the frame of sensor_frame.h on the ground-truth mesh and (p, R) the real reading in the same body frame,
//   o = ori^T (p - pos),   Q = ori^T R,
// and per (group, sensor) over the n frames of the group whose mask is 1
//   means = sum o / n,   covs = sum (o - means)(o - means)^T / (n - 1),   r = the rotation closest to sum Q / n.
//
// Pass 1, one workgroup of 256 lanes per (group, chunk of 256 consecutive frames counted from the group's first frame), a
// lane per frame, a loop over the sensors: o and Q in fp32 (also the optional per-frame outputs; a frame that does not
// count writes zeros), then the 19 sums of data_kernels.h in double -- over the wave by the butterfly v += shfl_xor(v, off),
// off = 32 .. 1, then over the four waves through LDS in wave order; lane 0 writes them.  Lanes past the group's end add
// exact zeros.  Pass 2, one lane per (group, sensor): the group's chunks in ascending order, the moments, the SVD.
// No atomics, and a group's partition into chunks does not depend on the rest of the batch: repeated launches give the same
// bits, and a group gives the same bits alone as in a batch.
#include <hip/hip_runtime.h>

#include "data_kernels.h"
#include "sensor_frame.h"
#include "svd3.h"

namespace empose {

namespace {

constexpr int OS_THREADS = OFFSET_STATS_CHUNK;
constexpr int OS_WAVES = OS_THREADS / 64;
constexpr int OS_FINISH_THREADS = 64;
constexpr int NS = OFFSET_STATS_SUMS;

// (in long: n_frames may be within a chunk of 2^31)
__device__ __forceinline__ int chunks_of(int n_frames) {
  return (int)(((long)n_frames + OFFSET_STATS_CHUNK - 1) / OFFSET_STATS_CHUNK);
}

__global__ void __launch_bounds__(OS_THREADS) offset_accumulate_kernel(OffsetStatsArgs a) {
  __shared__ double part[2][OS_WAVES][NS];   // two sets: sensor m + 1 is written while lane 0 still reads sensor m
  // the block's group and its chunk of that group (the same for every lane)
  int g = 0, chunk = (int)blockIdx.x;
  for (; g < a.G; ++g) {
    const int c = chunks_of(a.groups[g].n_frames);
    if (chunk < c) break;
    chunk -= c;
  }
  if (g == a.G) return;
  const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const long in_group = (long)chunk * OFFSET_STATS_CHUNK + tid;
  const bool in_range = in_group < (long)a.groups[g].n_frames;
  const long t = (long)a.groups[g].first_frame + in_group;   // read only when in_range
  const float* V = a.vertices + (size_t)t * a.V * 3;
  double* out = a.sums + (size_t)blockIdx.x * a.M * NS;

  for (int m = 0; m < a.M; ++m) {
    const size_t row = (size_t)t * a.M + m;
    const bool valid = in_range && (!a.masks || a.masks[row] == 1.f);
    float o[3] = {0.f, 0.f, 0.f}, Q[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (valid) {
      const int center = a.center[m];
      float n[3], ori[9];
      sensor_frame(V, a.faces + (size_t)m * a.max_deg * 3, a.deg[m], center, a.helper[m], n, ori);
      const float* vc = V + (size_t)center * 3;
      const float* p = a.p + row * 3;
      const float* R = a.R + row * 9;
      const float d[3] = {p[0] - vc[0], p[1] - vc[1], p[2] - vc[2]};
      for (int c = 0; c < 3; ++c) {   // ori^T: column c of ori against d and against the columns of R
        o[c] = ori[0 * 3 + c] * d[0] + ori[1 * 3 + c] * d[1] + ori[2 * 3 + c] * d[2];
        for (int k = 0; k < 3; ++k)
          Q[c * 3 + k] = ori[0 * 3 + c] * R[0 * 3 + k] + ori[1 * 3 + c] * R[1 * 3 + k] + ori[2 * 3 + c] * R[2 * 3 + k];
      }
    }
    if (in_range) {
      if (a.local_f)
        for (int c = 0; c < 3; ++c) a.local_f[row * 3 + c] = o[c];
      if (a.q_f)
        for (int e = 0; e < 9; ++e) a.q_f[row * 9 + e] = Q[e];
    }
    double v[NS];
    const double od[3] = {(double)o[0], (double)o[1], (double)o[2]};
    v[0] = valid ? 1.0 : 0.0;
    v[1] = od[0]; v[2] = od[1]; v[3] = od[2];
    v[4] = od[0] * od[0]; v[5] = od[0] * od[1]; v[6] = od[0] * od[2];
    v[7] = od[1] * od[1]; v[8] = od[1] * od[2]; v[9] = od[2] * od[2];
    for (int e = 0; e < 9; ++e) v[10 + e] = (double)Q[e];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
      for (int i = 0; i < NS; ++i) v[i] += __shfl_xor(v[i], off, 64);
    if (lane == 0)
      for (int i = 0; i < NS; ++i) part[m & 1][wave][i] = v[i];
    __syncthreads();
    if (tid == 0)
      for (int i = 0; i < NS; ++i) {
        double s = part[m & 1][0][i];
        for (int w = 1; w < OS_WAVES; ++w) s += part[m & 1][w][i];
        out[(size_t)m * NS + i] = s;
      }
  }
}

__global__ void __launch_bounds__(OS_FINISH_THREADS) offset_finish_kernel(OffsetStatsArgs a) {
  const long idx = (long)blockIdx.x * OS_FINISH_THREADS + threadIdx.x;
  if (idx >= (long)a.G * a.M) return;
  const int g = (int)(idx / a.M), m = (int)(idx - (long)g * a.M);
  size_t first_chunk = 0;
  for (int k = 0; k < g; ++k) first_chunk += (size_t)chunks_of(a.groups[k].n_frames);
  const int n_chunks = chunks_of(a.groups[g].n_frames);
  double s[NS];
  for (int i = 0; i < NS; ++i) s[i] = 0.0;
  for (int c = 0; c < n_chunks; ++c) {
    const double* in = a.sums + ((first_chunk + c) * a.M + m) * NS;
    for (int i = 0; i < NS; ++i) s[i] += in[i];
  }
  const double n = s[0];
  a.counts[idx] = (int)n;
  float* means = a.means + (size_t)idx * 3;
  float* covs = a.covs + (size_t)idx * 9;
  float* r = a.r + (size_t)idx * 9;
  if (!(n >= 1.0)) {   // no frame counts: zero offset, identity
    for (int c = 0; c < 3; ++c) means[c] = 0.f;
    for (int e = 0; e < 9; ++e) { covs[e] = 0.f; r[e] = (e % 4 == 0) ? 1.f : 0.f; }
    a.r_trace[idx] = 3.f;
    return;
  }
  const double mu[3] = {s[1] / n, s[2] / n, s[3] / n};
  for (int c = 0; c < 3; ++c) means[c] = (float)mu[c];
  // The covariance from the raw moments, (sum o o^T - n mu mu^T) / (n - 1).  Double moments are enough here: offsets are
  // centimetres and their spread millimetres, so the subtraction loses about (1e-2 / 1e-3)^2 = 1e2 of the 1e16 a double
  // resolves, and the rounding of n <= 1e6 additions another 1e6 at the very worst.
  const int pair[3][3] = {{4, 5, 6}, {5, 7, 8}, {6, 8, 9}};
  for (int i = 0; i < 3; ++i)
    for (int k = 0; k < 3; ++k)
      covs[i * 3 + k] = n >= 2.0 ? (float)((s[pair[i][k]] - n * mu[i] * mu[k]) / (n - 1.0)) : 0.f;

  // r: with sum Q / n = U S V^T, singular values descending, r = U diag(1, 1, det(U V^T)) V^T.  The decomposition is the
  // metrics kernel's: one-sided Jacobi, then U built right-handed (u3 = u1 x u2, s3 = u3 . A v3 signed), so that it holds
  // whatever s3 is; with that U, det(U V^T) = det(V) and s3 carries its sign: r = U diag(1, 1, det V) V^T and
  // r_trace = s1 + s2 + det(V) s3.
  double W[9], Vm[9], nrm[3];
  for (int e = 0; e < 9; ++e) W[e] = s[10 + e] / n;
  svd3_one_sided(W, Vm);
  for (int c = 0; c < 3; ++c) nrm[c] = sqrt(W[c] * W[c] + W[3 + c] * W[3 + c] + W[6 + c] * W[6 + c]);
  int ord[3] = {0, 1, 2};
  for (int i = 0; i < 2; ++i)
    for (int k = i + 1; k < 3; ++k)
      if (nrm[ord[k]] > nrm[ord[i]]) { const int tmp = ord[i]; ord[i] = ord[k]; ord[k] = tmp; }
  double Vs[9], U[9], S[3];
  for (int c = 0; c < 3; ++c) {
    S[c] = nrm[ord[c]];
    for (int k = 0; k < 3; ++k) Vs[k * 3 + c] = Vm[k * 3 + ord[c]];
  }
  double u1[3], u2[3];
  for (int k = 0; k < 3; ++k) u1[k] = S[0] > 0 ? W[k * 3 + ord[0]] / S[0] : (k == 0 ? 1.0 : 0.0);
  if (S[1] > 0) {
    for (int k = 0; k < 3; ++k) u2[k] = W[k * 3 + ord[1]] / S[1];
  } else {
    int j = 0;  // e_j with the smallest |u1_j|, minus its u1 part
    for (int k = 1; k < 3; ++k)
      if (fabs(u1[k]) < fabs(u1[j])) j = k;
    double len = 0;
    for (int k = 0; k < 3; ++k) {
      u2[k] = (k == j ? 1.0 : 0.0) - u1[j] * u1[k];
      len += u2[k] * u2[k];
    }
    len = sqrt(len);
    for (int k = 0; k < 3; ++k) u2[k] /= len;
  }
  const double u3[3] = {u1[1] * u2[2] - u1[2] * u2[1], u1[2] * u2[0] - u1[0] * u2[2], u1[0] * u2[1] - u1[1] * u2[0]};
  S[2] = u3[0] * W[ord[2]] + u3[1] * W[3 + ord[2]] + u3[2] * W[6 + ord[2]];
  for (int k = 0; k < 3; ++k) { U[k * 3] = u1[k]; U[k * 3 + 1] = u2[k]; U[k * 3 + 2] = u3[k]; }
  const double dv = det3(Vs) < 0 ? -1.0 : 1.0;
  for (int i = 0; i < 3; ++i)
    for (int k = 0; k < 3; ++k)
      r[i * 3 + k] = (float)(U[i * 3] * Vs[k * 3] + U[i * 3 + 1] * Vs[k * 3 + 1] + dv * U[i * 3 + 2] * Vs[k * 3 + 2]);
  a.r_trace[idx] = (float)(S[0] + S[1] + dv * S[2]);
}

}  // namespace

hipError_t launch_offset_stats(const OffsetStatsArgs& a, hipStream_t stream) {
  if (a.n_chunks > 0) {
    hipLaunchKernelGGL(offset_accumulate_kernel, dim3((unsigned)a.n_chunks), dim3(OS_THREADS), 0, stream, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  const long lanes = (long)a.G * a.M;
  hipLaunchKernelGGL(offset_finish_kernel, dim3((unsigned)((lanes + OS_FINISH_THREADS - 1) / OS_FINISH_THREADS)),
                     dim3(OS_FINISH_THREADS), 0, stream, a);
  return hipGetLastError();
}

}  // namespace empose
