// Sensor placement search (data/placement.py), gfx950 only: which vertex of the mesh does each sensor sit over?  The
// definition is this project's own; per sensor m and candidate vertex c, over the n frames of a group
// whose mask is 1, with p the real reading and x the ground-truth vertex in the same body frame,
//   score[m][c] = sum_f |p_f(m) - x_f(c)|^2 / n,   best[m] = argmin_c score[m][c], the lowest id on an exact tie.
//
// Accumulation, one slab of T frames.  A workgroup of 256 lanes owns 64 consecutive candidates, one chunk of 64 consecutive
// frames counted from the slab's first, and up to 12 sensors: T = 1024 on the 6890 vertices is 108 x 16 workgroups.  The
// chunk's readings go to LDS once (x, y, z and whether the frame counts); every lane then reads them at one address, a
// broadcast.  Lane l of every wave owns candidate 64 * tile + l, so neighbouring lanes read neighbouring vertices; wave w
// walks the frames w, w + 4, ... of the chunk in ascending order.  The difference and the square are fp32, every sum is
// double: a lane's 12 running sums, then the four waves through LDS as ((w0 + w1) + w2) + w3, written to the chunk's row of
// `part`.  A second launch adds the chunks to the running sums in ascending order, a lane per (sensor, candidate), and
// counts the frames, a workgroup per sensor (integers: exact in any order).
// Finish: a workgroup per sensor writes the fp32 scores and reduces (score, candidate) to the smallest pair.
// No atomics; every sum's order follows from the slab's frame range alone, so the same inputs and slab size give the same
// bits, and a group gives the same bits whatever was searched before it.
#include <hip/hip_runtime.h>

#include <climits>

#include "data_kernels.h"

namespace empose {

namespace {

constexpr int PL_THREADS = 256;
constexpr int PL_WAVES = PL_THREADS / 64;
constexpr int PL_TILE = 64;   // candidates per workgroup: a lane each
constexpr int PL_MB = PLACEMENT_SENSORS;

__global__ void __launch_bounds__(PL_THREADS) placement_accumulate_kernel(PlacementArgs a) {
  __shared__ float4 reading[PLACEMENT_CHUNK][PL_MB];   // (p, 1 if the frame counts for the sensor else 0)
  __shared__ double other[PL_WAVES - 1][PL_MB][PL_TILE];
  const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int chunk = (int)blockIdx.y;
  const int t0 = chunk * PLACEMENT_CHUNK;
  const int nf = min(PLACEMENT_CHUNK, a.T - t0);
  const int m0 = (int)blockIdx.z * PL_MB;
  const int nm = min(PL_MB, a.M - m0);

  for (int i = tid; i < nf * PL_MB; i += PL_THREADS) {
    const int f = i / PL_MB, k = i - f * PL_MB;
    float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
    if (k < nm) {
      const size_t row = (size_t)(t0 + f) * a.M + (m0 + k);
      if (!a.masks || a.masks[row] == 1.f) q = make_float4(a.p[row * 3], a.p[row * 3 + 1], a.p[row * 3 + 2], 1.f);
    }
    reading[f][k] = q;
  }
  __syncthreads();

  const int c = (int)blockIdx.x * PL_TILE + lane;
  const bool live = c < a.C;
  const int cc = live ? c : a.C - 1;   // lanes past the end read the last candidate and write nothing
  const int vid = a.cand ? a.cand[cc] : cc;
  const float* x = a.vertices + ((size_t)t0 * a.V + vid) * 3;
  double acc[PL_MB];
#pragma unroll
  for (int k = 0; k < PL_MB; ++k) acc[k] = 0.0;
#pragma unroll 2
  for (int f = wave; f < nf; f += PL_WAVES) {
    const float* xf = x + (size_t)f * a.V * 3;
    const float x0 = xf[0], x1 = xf[1], x2 = xf[2];
#pragma unroll
    for (int k = 0; k < PL_MB; ++k) {
      if (k < nm) {   // the same for every lane
        const float4 q = reading[f][k];
        const float dx = q.x - x0, dy = q.y - x1, dz = q.z - x2;
        const float d2 = dx * dx + dy * dy + dz * dz;
        acc[k] += q.w != 0.f ? (double)d2 : 0.0;   // a select: a frame that does not count may hold anything
      }
    }
  }
  if (wave > 0) {
#pragma unroll
    for (int k = 0; k < PL_MB; ++k) other[wave - 1][k][lane] = acc[k];
  }
  __syncthreads();
  if (wave == 0 && live) {
    const size_t mc = (size_t)a.M * a.C;
#pragma unroll
    for (int k = 0; k < PL_MB; ++k) {
      if (k < nm) {
        double s = acc[k];
        for (int w = 0; w < PL_WAVES - 1; ++w) s += other[w][k][lane];
        a.part[(size_t)chunk * mc + (size_t)(m0 + k) * a.C + c] = s;
      }
    }
  }
}

// Blocks [0, n_sum): sums[m][c] += the chunks in ascending order.  Blocks [n_sum, n_sum + M): counts[m] += the frames.
__global__ void __launch_bounds__(PL_THREADS) placement_combine_kernel(PlacementArgs a, int n_sum, int n_chunks) {
  __shared__ int wave_n[PL_WAVES];
  const int tid = (int)threadIdx.x;
  const size_t mc = (size_t)a.M * a.C;
  if ((int)blockIdx.x < n_sum) {
    const size_t idx = (size_t)blockIdx.x * PL_THREADS + tid;
    if (idx >= mc) return;
    double s = a.sums[idx];
    for (int k = 0; k < n_chunks; ++k) s += a.part[(size_t)k * mc + idx];
    a.sums[idx] = s;
    return;
  }
  const int m = (int)blockIdx.x - n_sum;
  int n = 0;
  if (a.masks) {
    for (int t = tid; t < a.T; t += PL_THREADS) n += a.masks[(size_t)t * a.M + m] == 1.f ? 1 : 0;
  } else {
    for (int t = tid; t < a.T; t += PL_THREADS) n += 1;
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) n += __shfl_xor(n, off, 64);
  if ((tid & 63) == 0) wave_n[tid >> 6] = n;
  __syncthreads();
  if (tid == 0) {
    int total = a.counts[m];
    for (int w = 0; w < PL_WAVES; ++w) total += wave_n[w];
    a.counts[m] = total;
  }
}

// The smaller of two (score, candidate) pairs: the lower score, and on equal scores the lower candidate.
__device__ __forceinline__ void take_smaller(float& s, int& i, float os, int oi) {
  if (os < s || (os == s && oi < i)) { s = os; i = oi; }
}

__global__ void __launch_bounds__(PL_THREADS) placement_finish_kernel(PlacementArgs a) {
  __shared__ float wave_s[PL_WAVES];
  __shared__ int wave_i[PL_WAVES];
  const int tid = (int)threadIdx.x, m = (int)blockIdx.x;
  const int n = a.counts[m];
  const double* sums = a.sums + (size_t)m * a.C;
  float* score = a.score + (size_t)m * a.C;
  float bs = __builtin_inff();
  int bi = INT_MAX;   // no candidate yet: loses every tie
  for (int c = tid; c < a.C; c += PL_THREADS) {
    const float s = n > 0 ? (float)(sums[c] / (double)n) : __builtin_inff();
    score[c] = s;
    if (s < bs) { bs = s; bi = c; }   // ascending c: the first of equal scores stays
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const float os = __shfl_xor(bs, off, 64);
    const int oi = __shfl_xor(bi, off, 64);
    take_smaller(bs, bi, os, oi);
  }
  if ((tid & 63) == 0) { wave_s[tid >> 6] = bs; wave_i[tid >> 6] = bi; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < PL_WAVES; ++w) take_smaller(bs, bi, wave_s[w], wave_i[w]);
    a.best[m] = bi == INT_MAX ? -1 : (a.cand ? a.cand[bi] : bi);
    a.best_score[m] = bs;
  }
}

}  // namespace

hipError_t launch_placement_accumulate(const PlacementArgs& a, hipStream_t stream) {
  const int n_chunks = (a.T + PLACEMENT_CHUNK - 1) / PLACEMENT_CHUNK;
  const dim3 grid((unsigned)((a.C + PL_TILE - 1) / PL_TILE), (unsigned)n_chunks, (unsigned)((a.M + PL_MB - 1) / PL_MB));
  hipLaunchKernelGGL(placement_accumulate_kernel, grid, dim3(PL_THREADS), 0, stream, a);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const int n_sum = (int)(((size_t)a.M * a.C + PL_THREADS - 1) / PL_THREADS);
  hipLaunchKernelGGL(placement_combine_kernel, dim3((unsigned)(n_sum + a.M)), dim3(PL_THREADS), 0, stream, a, n_sum,
                     n_chunks);
  return hipGetLastError();
}

hipError_t launch_placement_finish(const PlacementArgs& a, hipStream_t stream) {
  hipLaunchKernelGGL(placement_finish_kernel, dim3((unsigned)a.M), dim3(PL_THREADS), 0, stream, a);
  return hipGetLastError();
}

}  // namespace empose
