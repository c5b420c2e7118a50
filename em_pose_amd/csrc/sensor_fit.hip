// Model-free sensor fitting, gfx950 only: Adam on the sensor residual of a body plus priors.  The
// residual's value and gradient come from the SMPL evaluation (smpl_chain.hip / smpl_tile.hip); the kernels here are what one
// iteration does besides.  Per window w of F frames, live_t = t < seq_length,
//   J_w = sum_t s_t E_t + lambda_pose / 2 sum_{t live} |theta_t[3:66] - p_t[3:66]|^2 + lambda_shape / 2 |beta_w|^2
//         + lambda_smooth / 2 sum_{t >= 1, live} |theta_t - theta_{t-1}|^2,
// E_t the sum over the model's sensors of |pos - target| and |ori - target|_F, s_t = live_t [every sensor read is present].
//
//   fit_prepare  s, zero moments, iterate 0 from the caller's init (or zeros), best J = +inf
//   fit_step     J_w at iterate k, the gradients of the priors (the smoothness stencil gathers from iterate k only; iterate
//                k + 1 goes to the other buffer of a pair), the window sum of the shape gradient, Adam, keep-best
//   fit_finish   J_w at iterate K, best or last per window into the outputs
//   fit_energy   s_t E_t of given sensors
//
// One workgroup per window (256 lanes up to 64 frames, 1024 above); lanes stride over the window's frames and its (frame, parameter) items, so F is a
// loop bound and no LDS grows with it.  Every sum runs in a fixed order: a lane's items in ascending order, the wave by the
// xor exchange of lane_reduce.h (the pairs of v += shfl_xor(v, off), off = 32 .. 1), the workgroup's waves through LDS in wave
// order.  No atomics: a second launch gives the same bits, and a window gives the same bits alone as in a batch.
#include <hip/hip_runtime.h>

#include "fit_kernels.h"
#include "lane_reduce.h"

namespace empose {

namespace {

// Lanes per window: 256 up to 64 frames, 1024 above (a window of 256 frames is 16 896 (frame, parameter) items).  Measured
// at K = 50 (profiles/sensor_fit_lanes256_mi355x.txt, _lanes1024_): 1024 windows of 32 frames 38 us a step with 256 lanes and
// 53 us with 1024, one window of 256 frames 65 us and 27 us; between the two sizes the threshold is not tuned.  The choice depends on F
// alone, so a window's bits do not depend on the batch.
constexpr int FIT_THREADS_SHORT = 256, FIT_THREADS_LONG = 1024, FIT_LONG_FROM = 65;
constexpr int FIT_FLAT_THREADS = 256;   // the kernels with a lane per element or frame
constexpr int FIT_SUMS = 16;   // 10 shape-gradient sums | J | 5 unused (a power of two: the reduce-scatter halves it 4 times)
constexpr int FIT_J = 10;

__device__ __forceinline__ int window_length(const FitProblem& p, int b) {
  const int len = p.seq_lengths ? p.seq_lengths[b] : p.F;
  return len < 0 ? 0 : (len > p.F ? p.F : len);
}

// E_t: the sensors the model reads, in sensor order.
__device__ float frame_energy(const FitProblem& p, const float* pos, const float* ori, size_t t) {
  const float* row = p.tgt + t * p.ld_tgt;
  float e = 0.f;
#pragma unroll
  for (int m = 0; m < 12; ++m) {
    const int slot = p.used_slot[m];
    if (slot < 0) continue;
    const float* pm = pos + (t * 12 + m) * 3;
    const float* om = ori + (t * 12 + m) * 9;
    const float* tp = row + slot * 3;
    const float* to = row + p.n_markers * 3 + slot * 9;
    float sp = 0.f, so = 0.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) { const float d = pm[k] - tp[k]; sp += d * d; }
#pragma unroll
    for (int k = 0; k < 9; ++k) { const float d = om[k] - to[k]; so += d * d; }
    e += sqrtf(sp) + sqrtf(so);
  }
  return e;
}

// A lane's share of J_w: its frames' data terms, then its items' pose and smoothness terms, then its shape terms.
template <int FIT_THREADS>
__device__ float objective_partial(const FitProblem& p, const float* theta, const float* beta, const float* pos,
                                   const float* ori, float* energy, int b, int len, int tid) {
  const int F = p.F;
  const size_t t0 = (size_t)b * F;
  float part = 0.f;
  for (int f = tid; f < F; f += FIT_THREADS) {
    const size_t t = t0 + f;
    const float s = f < len ? p.s[t] : 0.f;
    const float e = s != 0.f ? s * frame_energy(p, pos, ori, t) : 0.f;   // (a frame without data may hold anything)
    if (energy) energy[t] = e;
    part += e;
  }
  for (int idx = tid; idx < len * 66; idx += FIT_THREADS) {
    const int f = idx / 66, i = idx - f * 66;
    const size_t at = (t0 + f) * 66 + i;
    const float th = theta[at];
    if (i >= 3) {
      const float d = th - (p.prior ? p.prior[at] : 0.f);
      part += 0.5f * p.lambda_pose * d * d;
    }
    if (f >= 1) {
      const float d = th - theta[at - 66];
      part += 0.5f * p.lambda_smooth * d * d;
    }
  }
  const int n_shape = p.shape_per_window ? 10 : len * 10;   // (one shape per window: its first row)
  for (int idx = tid; idx < n_shape; idx += FIT_THREADS) {
    const float x = beta[t0 * 10 + idx];
    part += 0.5f * p.lambda_shape * x * x;
  }
  return part;
}

// v[0 .. 16) summed over the workgroup in the fixed order; every lane returns with all 16 sums in `tot`.
template <int FIT_WAVES>
__device__ void window_sums(float (&v)[FIT_SUMS], float (*red)[FIT_SUMS], float* tot, int tid) {
  const int lane = tid & 63, wave = tid >> 6;
  int base = 0, count = 0;
  LaneReduceScatter<FIT_SUMS, 32, FIT_SUMS>::run(v, lane, base, count);   // -> one sum per lane: v[0] is sum `base`
  if ((lane & 3) == 0) red[wave][base] = v[0];
  __syncthreads();
  if (tid < FIT_SUMS) {
    float s = red[0][tid];
#pragma unroll
    for (int w = 1; w < FIT_WAVES; ++w) s += red[w][tid];
    tot[tid] = s;
  }
  __syncthreads();
}

__device__ __forceinline__ float adam(const FitStepArgs& a, float x, float g, float* m, float* v) {
  const float m1 = a.beta1 * *m + (1.f - a.beta1) * g;
  const float v1 = a.beta2 * *v + (1.f - a.beta2) * (g * g);
  *m = m1; *v = v1;
  return x - a.lr_k * (a.c1 * m1) / (sqrtf(a.c2 * v1) + a.eps);
}

__global__ void __launch_bounds__(FIT_FLAT_THREADS) fit_prepare_kernel(FitPrepareArgs a) {
  const FitProblem& p = a.p;
  const size_t T = (size_t)p.B * p.F, stride = (size_t)gridDim.x * FIT_FLAT_THREADS;
  const size_t first = (size_t)blockIdx.x * FIT_FLAT_THREADS + threadIdx.x;
  for (size_t i = first; i < a.n_moments; i += stride) a.moments[i] = 0.f;
  for (size_t i = first; i < T * 66; i += stride) a.theta[i] = a.pose_init ? a.pose_init[i] : 0.f;
  for (size_t i = first; i < T * 10; i += stride) {
    // one shape per window: the init of the window's first frame, in every row
    const size_t t = i / 10, c = i - t * 10, from = p.shape_per_window ? (t / p.F) * p.F * 10 + c : i;
    a.beta[i] = a.shape_init ? a.shape_init[from] : 0.f;
  }
  for (size_t t = first; t < T; t += stride) {
    const int b = (int)(t / p.F), f = (int)(t - (size_t)b * p.F);
    bool on = f < window_length(p, b);
    if (on && a.marker_masks)
      for (int m = 0; m < 12; ++m) on = on && (p.used_slot[m] < 0 || a.marker_masks[t * 12 + m] == 1.f);
    a.s[t] = on ? 1.f : 0.f;
  }
  for (size_t i = first; i < (size_t)p.B; i += stride) a.best_J[i] = __builtin_inff();
}

template <int FIT_THREADS>
__global__ void __launch_bounds__(FIT_THREADS) fit_step_kernel(FitStepArgs a) {
  constexpr int FIT_WAVES = FIT_THREADS / 64;
  __shared__ float red[FIT_WAVES][FIT_SUMS];
  __shared__ float tot[FIT_SUMS];
  __shared__ float beta_new[10];
  const FitProblem& p = a.p;
  const int b = (int)blockIdx.x, tid = (int)threadIdx.x, F = p.F;
  const int len = window_length(p, b);
  const size_t t0 = (size_t)b * F;

  float v[FIT_SUMS];
#pragma unroll
  for (int i = 0; i < FIT_SUMS; ++i) v[i] = 0.f;
  v[FIT_J] = objective_partial<FIT_THREADS>(p, a.theta, a.beta, a.pos, a.ori, a.energy, b, len, tid);
  if (p.shape_per_window)
    for (int f = tid; f < len; f += FIT_THREADS)
#pragma unroll
      for (int c = 0; c < 10; ++c) v[c] += a.g_beta[(t0 + f) * 10 + c];
  // (read before the barriers of window_sums: lane 0 overwrites it at the end of the kernel)
  const float best_so_far = a.best_J ? a.best_J[b] : 0.f;
  window_sums<FIT_WAVES>(v, red, tot, tid);
  const float J = tot[FIT_J];

  // keep-best looks at iterate k: its buffers are only read by this launch
  const bool better = a.best_J && J < best_so_far;
  if (better) {
    for (int idx = tid; idx < F * 66; idx += FIT_THREADS) a.best_theta[t0 * 66 + idx] = a.theta[t0 * 66 + idx];
    for (int idx = tid; idx < F * 10; idx += FIT_THREADS) a.best_beta[t0 * 10 + idx] = a.beta[t0 * 10 + idx];
  }

  // pose: data gradient + pose prior + smoothness stencil (gather form), Adam; padded frames as they are
  for (int idx = tid; idx < F * 66; idx += FIT_THREADS) {
    const int f = idx / 66, i = idx - f * 66;
    const size_t at = (t0 + f) * 66 + i;
    const float th = a.theta[at];
    if (f >= len) { a.theta_next[at] = th; continue; }
    float g = a.g_theta[at];
    if (i >= 3) g += p.lambda_pose * (th - (p.prior ? p.prior[at] : 0.f));
    float d = 0.f;
    if (f >= 1) d += th - a.theta[at - 66];
    if (f + 1 < len) d += th - a.theta[at + 66];
    g += p.lambda_smooth * d;
    a.theta_next[at] = adam(a, th, g, a.m_theta + at, a.v_theta + at);
  }

  if (p.shape_per_window) {
    if (tid < 10) {
      const size_t at = t0 * 10 + tid;
      const float x = a.beta[at];
      beta_new[tid] = adam(a, x, tot[tid] + p.lambda_shape * x, a.m_beta + at, a.v_beta + at);
    }
    __syncthreads();
    for (int idx = tid; idx < F * 10; idx += FIT_THREADS) a.beta_next[t0 * 10 + idx] = beta_new[idx % 10];
  } else {
    for (int idx = tid; idx < F * 10; idx += FIT_THREADS) {
      const size_t at = t0 * 10 + idx;
      const float x = a.beta[at];
      a.beta_next[at] = idx < len * 10 ? adam(a, x, a.g_beta[at] + p.lambda_shape * x, a.m_beta + at, a.v_beta + at) : x;
    }
  }
  if (tid == 0) {
    a.J[b] = J;
    if (better) a.best_J[b] = J;
  }
}

template <int FIT_THREADS>
__global__ void __launch_bounds__(FIT_THREADS) fit_finish_kernel(FitFinishArgs a) {
  constexpr int FIT_WAVES = FIT_THREADS / 64;
  __shared__ float red[FIT_WAVES][FIT_SUMS];
  __shared__ float tot[FIT_SUMS];
  const FitProblem& p = a.p;
  const int b = (int)blockIdx.x, tid = (int)threadIdx.x, F = p.F;
  const size_t t0 = (size_t)b * F;
  float v[FIT_SUMS];
#pragma unroll
  for (int i = 0; i < FIT_SUMS; ++i) v[i] = 0.f;
  v[FIT_J] = objective_partial<FIT_THREADS>(p, a.theta, a.beta, a.pos, a.ori, nullptr, b, window_length(p, b), tid);
  window_sums<FIT_WAVES>(v, red, tot, tid);
  const float J = tot[FIT_J];
  // the earliest of equal minima: iterate K only where it is strictly below the best of 0 .. K - 1
  const bool last = !a.best_J || J < a.best_J[b];
  const float* th = last ? a.theta : a.best_theta;
  const float* be = last ? a.beta : a.best_beta;
  for (int idx = tid; idx < F * 66; idx += FIT_THREADS) a.pose[t0 * 66 + idx] = th[t0 * 66 + idx];
  for (int idx = tid; idx < F * 10; idx += FIT_THREADS) a.shape[t0 * 10 + idx] = be[t0 * 10 + idx];
  if (tid == 0) {
    a.J_last[b] = J;
    a.J_out[b] = last ? J : a.best_J[b];
  }
}

__global__ void __launch_bounds__(FIT_FLAT_THREADS) fit_energy_kernel(FitProblem p, const float* pos, const float* ori,
                                                                      float* energy) {
  const size_t t = (size_t)blockIdx.x * FIT_FLAT_THREADS + threadIdx.x;
  if (t >= (size_t)p.B * p.F) return;
  const int b = (int)(t / p.F), f = (int)(t - (size_t)b * p.F);
  const float s = f < window_length(p, b) ? p.s[t] : 0.f;
  energy[t] = s != 0.f ? s * frame_energy(p, pos, ori, t) : 0.f;
}

}  // namespace

hipError_t launch_fit_prepare(const FitPrepareArgs& a, hipStream_t stream) {
  const size_t n = (size_t)a.p.B * a.p.F * 66;
  const size_t blocks = (n + FIT_FLAT_THREADS - 1) / FIT_FLAT_THREADS;
  hipLaunchKernelGGL(fit_prepare_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(FIT_FLAT_THREADS), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_fit_step(const FitStepArgs& a, hipStream_t stream) {
  if (a.p.F >= FIT_LONG_FROM)
    hipLaunchKernelGGL(fit_step_kernel<FIT_THREADS_LONG>, dim3((unsigned)a.p.B), dim3(FIT_THREADS_LONG), 0, stream, a);
  else
    hipLaunchKernelGGL(fit_step_kernel<FIT_THREADS_SHORT>, dim3((unsigned)a.p.B), dim3(FIT_THREADS_SHORT), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_fit_finish(const FitFinishArgs& a, hipStream_t stream) {
  if (a.p.F >= FIT_LONG_FROM)
    hipLaunchKernelGGL(fit_finish_kernel<FIT_THREADS_LONG>, dim3((unsigned)a.p.B), dim3(FIT_THREADS_LONG), 0, stream, a);
  else
    hipLaunchKernelGGL(fit_finish_kernel<FIT_THREADS_SHORT>, dim3((unsigned)a.p.B), dim3(FIT_THREADS_SHORT), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_fit_energy(const FitProblem& p, const float* pos, const float* ori, float* energy, hipStream_t stream) {
  const size_t T = (size_t)p.B * p.F;
  hipLaunchKernelGGL(fit_energy_kernel, dim3((unsigned)((T + FIT_FLAT_THREADS - 1) / FIT_FLAT_THREADS)), dim3(FIT_FLAT_THREADS), 0, stream,
                     p, pos, ori, energy);
  return hipGetLastError();
}

}  // namespace empose
