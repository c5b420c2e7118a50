// lgd_losses: the loss terms of IterativeErrorFeedback.backward (reference models.py:634-688, loss.py:13-41) and their
// cotangents in one pass, and the fixed-order reduction to the five loss values.
#include "train_kernels.h"

namespace empose {

// ---------------------------------------------------------------------------------------------------------------
// Losses of IterativeErrorFeedback.backward and their cotangents (reference models.py:634-688, loss.py:13-41):
//   total = (w_pose sum_i L1(pose_i) + w_shape sum_i L1(shape_i) + w_fk (N+1) FK(joints_N) + w_rec sum_i REC_i) / (N+1)
//   L1: |hat - gt| averaged over the features, summed over the valid frames / len_b, averaged over the batch
//   FK / REC: sum of Euclidean norms per frame (joints; sensor positions + 9-vector orientations of the sensors fed to
//   the network), frames with a missing sensor dropped, summed over the valid frames / len_b, averaged over the batch.
// 16 lanes per (history entry, frame): lane 0 pose, 1 shape, 2..13 one sensor each, 14 the joints (last entry only).
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void lgd_losses_kernel(LossArgs a) {
  const int T = a.B * a.F;
  const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long item = gid >> 4;
  const int part = (int)(gid & 15);
  const bool in_range = item < (long)a.N1 * T;
  const long it = in_range ? item : 0;
  const int i = (int)(it / T), t = (int)(it - (long)i * T);
  const int b = t / a.F, f = t - b * a.F;
  const int len = a.seq_lengths ? a.seq_lengths[b] : a.F;
  const bool live = in_range && f < len;
  bool frame_ok = true;
  if (a.masks)
    for (int m = 0; m < 12; ++m) frame_ok = frame_ok && a.masks[(size_t)t * 12 + m] != 0.f;
  const float inv = 1.f / ((float)len * (float)a.B);
  const float inv_n1 = 1.f / (float)a.N1;
  float l_pose = 0.f, l_shape = 0.f, l_rec = 0.f, l_fk = 0.f;
  const size_t row = (size_t)i * T + t;
  if (in_range && part == 0) {
    const float* h = a.pose_hist + row * 66;
    const float* g = a.pose_gt + (size_t)t * 66;
    float* d = a.d_pose + row * 66;
    const float k = live ? a.w_pose * inv_n1 * inv / 66.f : 0.f;
    const float kn = live ? -k : 0.f;   // a padding frame gets +0 whatever it holds (not -0 where df < 0, +0 where df is NaN)
    float s = 0.f;
    for (int c = 0; c < 66; ++c) {
      const float df = h[c] - g[c];
      s += fabsf(df);
      d[c] = df > 0.f ? k : (df < 0.f ? kn : 0.f);
    }
    l_pose = live ? s / 66.f * inv : 0.f;
  } else if (in_range && part == 1) {
    const float* h = a.shape_hist + row * 10;
    const float* g = a.shape_gt + (size_t)b * 10;
    float* d = a.d_shape + row * 10;
    const float k = live ? a.w_shape * inv_n1 * inv / 10.f : 0.f;
    const float kn = live ? -k : 0.f;
    float s = 0.f;
    for (int c = 0; c < 10; ++c) {
      const float df = h[c] - g[c];
      s += fabsf(df);
      d[c] = df > 0.f ? k : (df < 0.f ? kn : 0.f);
    }
    l_shape = live ? s / 10.f * inv : 0.f;
  } else if (in_range && part >= 2 && part < 14) {
    const int m = part - 2;
    const int slot = a.used_slot[m];
    float* dp = a.d_pos + (row * 12 + m) * 3;
    float* dq = a.d_ori + (row * 12 + m) * 9;
    const bool on = live && frame_ok && slot >= 0;
    if (!on) {
      for (int c = 0; c < 3; ++c) dp[c] = 0.f;
      for (int c = 0; c < 9; ++c) dq[c] = 0.f;
    } else {
      const float* hp = a.pos_hist + (row * 12 + m) * 3;
      const float* hq = a.ori_hist + (row * 12 + m) * 9;
      const float* gp = a.x_in + (size_t)t * a.ldx + slot * 3;
      const float* gq = a.x_in + (size_t)t * a.ldx + a.n_markers * 3 + slot * 9;
      const float k = a.w_rec * inv_n1 * inv;
      float r[9], q = 0.f;
      for (int c = 0; c < 3; ++c) { r[c] = hp[c] - gp[c]; q += r[c] * r[c]; }
      float nrm = sqrtf(q);
      for (int c = 0; c < 3; ++c) dp[c] = k * r[c] / nrm;
      l_rec = nrm * inv;
      q = 0.f;
      for (int c = 0; c < 9; ++c) { r[c] = hq[c] - gq[c]; q += r[c] * r[c]; }
      nrm = sqrtf(q);
      for (int c = 0; c < 9; ++c) dq[c] = k * r[c] / nrm;
      l_rec += nrm * inv;
    }
  } else if (in_range && part == 14 && i == a.N1 - 1 && a.d_joints) {
    float* d = a.d_joints + (size_t)t * 66;
    const bool on = live && frame_ok && a.joints_gt != nullptr;
    if (!on) {
      for (int c = 0; c < 66; ++c) d[c] = 0.f;
    } else {
      const float* h = a.joints_final + (size_t)t * 66;
      const float* g = a.joints_gt + (size_t)t * 66;
      const float k = a.w_fk * inv;   // added N + 1 times, divided by N + 1
      float s = 0.f;
      for (int j = 0; j < 22; ++j) {
        const float r0 = h[j * 3] - g[j * 3], r1 = h[j * 3 + 1] - g[j * 3 + 1], r2 = h[j * 3 + 2] - g[j * 3 + 2];
        const float nrm = sqrtf(r0 * r0 + r1 * r1 + r2 * r2);
        d[j * 3] = k * r0 / nrm; d[j * 3 + 1] = k * r1 / nrm; d[j * 3 + 2] = k * r2 / nrm;
        s += nrm;
      }
      l_fk = s * inv;
    }
  }
  // per (entry, frame) sums over the 16 lanes -> partial[kind][item]
#pragma unroll
  for (int off = 8; off >= 1; off >>= 1) {
    l_pose += __shfl_xor(l_pose, off, 16);
    l_shape += __shfl_xor(l_shape, off, 16);
    l_rec += __shfl_xor(l_rec, off, 16);
    l_fk += __shfl_xor(l_fk, off, 16);
  }
  if (in_range && part == 0) {
    const size_t n = (size_t)a.N1 * T;
    a.partial[item] = l_pose; a.partial[n + item] = l_shape; a.partial[2 * n + item] = l_rec; a.partial[3 * n + item] = l_fk;
  }
}

// loss_vals = (pose, shape, reconstruction, fk, total) from the per-frame contributions, summed in index order
__global__ __launch_bounds__(1024) void lgd_losses_reduce_kernel(LossArgs a) {
  // the four terms side by side: 256 threads each, eight loads in flight per thread, double accumulation in a fixed order
  // (one term after the other with one load at a time took 45 us at 256 windows)
  __shared__ double red[4][256];
  const size_t n = (size_t)a.N1 * a.B * a.F;
  const int k = threadIdx.x >> 8, t = threadIdx.x & 255;
  const float* src = a.partial + (size_t)k * n;
  double s = 0.0;
  size_t i = t;
  for (; i + 7 * 256 < n; i += 8 * 256) {
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = src[i + u * 256];
#pragma unroll
    for (int u = 0; u < 8; ++u) s += (double)v[u];
  }
  for (; i < n; i += 256) s += (double)src[i];
  red[k][t] = s;
  __syncthreads();
  for (int off = 128; off >= 1; off >>= 1) {
    if (t < off) red[k][t] += red[k][t + off];
    __syncthreads();
  }
  const double sums[4] = {red[0][0], red[1][0], red[2][0], red[3][0]};
  if (threadIdx.x == 0) {
    const double n1 = (double)a.N1;
    const double fk_sum = sums[3] * n1;   // the same FK term is added once per history entry
    a.loss_vals[0] = (float)(sums[0] / n1);
    a.loss_vals[1] = (float)(sums[1] / n1);
    a.loss_vals[2] = (float)(sums[2] / n1);
    a.loss_vals[3] = (float)(fk_sum / n1);
    a.loss_vals[4] = (float)((a.w_pose * sums[0] + a.w_fk * fk_sum + a.w_shape * sums[1] + a.w_rec * sums[2]) / n1);
  }
}

hipError_t launch_lgd_losses(const LossArgs& a, hipStream_t stream) {
  const long n = (long)a.N1 * a.B * a.F * 16;
  hipLaunchKernelGGL(lgd_losses_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, a);
  hipLaunchKernelGGL(lgd_losses_reduce_kernel, dim3(1), dim3(1024), 0, stream, a);
  return hipGetLastError();
}

}  // namespace empose
