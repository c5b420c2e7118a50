// Small kernels of the training step around the products (reference nn/models.py:634-688 runs it through torch.autograd).
//
//   transpose    W[N][K] -> W^T[K][N]: dX = dY . W runs on the forward GEMM kernels (A . W'^T with W' = W^T); called by
//                the training drivers of the update MLPs and of the LSTM.
//   add2, window_mean, axpby2d   elementwise pieces
//   lstm_cell_bwd  one time step of back-propagation through time: gate pre-activation gradients from (dh, dc) and the
//                activations saved by the forward kernels (LstmUnitArgs::sv_*); the recurrent product dh_{t-1} = dG_t W_hh
//                is a GEMM launch per step (gemm_rec.hip runs the same cell inside that product).
//   lgd_assemble / lgd_update / lgd_cotangent   the bookkeeping of the LGD loop around the update networks
#include "lstm_cell_bwd.h"
#include "train_kernels.h"

namespace empose {

// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void transpose_kernel(const float* src, int ld_src, float* dst, int ld_dst, int rows,
                                                        int cols) {
  __shared__ float tile[32][33];
  const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int r = r0 + ty + 8 * k, c = c0 + tx;
    tile[ty + 8 * k][tx] = (r < rows && c < cols) ? src[(size_t)r * ld_src + c] : 0.f;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int c = c0 + ty + 8 * k, r = r0 + tx;
    if (c < cols && r < rows) dst[(size_t)c * ld_dst + r] = tile[tx][ty + 8 * k];
  }
}

hipError_t launch_transpose(const float* src, int ld_src, float* dst, int ld_dst, int rows, int cols,
                            hipStream_t stream) {
  hipLaunchKernelGGL(transpose_kernel, dim3((cols + 31) / 32, (rows + 31) / 32), dim3(256), 0, stream, src, ld_src, dst,
                     ld_dst, rows, cols);
  return hipGetLastError();
}

// out[i] = a[i] + b[i]  (b_ih + b_hh)
__global__ void add2_kernel(const float* a, const float* b, float* out, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = a[i] + b[i];
}
hipError_t launch_add2(const float* a, const float* b, float* out, int n, hipStream_t stream) {
  hipLaunchKernelGGL(add2_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, a, b, out, n);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------
// One step of back-propagation through time of an LSTM layer (gate order i, f, g, o; PyTorch semantics for packed ragged
// rows: a step at or past a row's length does not exist -- its state passes through, its output is zero).
//   dh = dy[b][t] + dh_in[b]     (dh_in: from step t + 1, incl. the pass-through of rows that had ended there)
//   live:   do = dh tanh(c_t); dc = dc_in + dh o (1 - tanh(c_t)^2); di = dc g; dg = dc i; df = dc c_{t-1}
//           dG = (di i(1-i), df f(1-f), dg (1-g^2), do o(1-o));  dc_out = dc f;  carry = 0
//   ended:  dG = 0;  dc_out = dc_in;  carry = dh_in
// The caller then launches dh_in' = dG_t . W_hh + carry.
// ---------------------------------------------------------------------------------------------------------------
__global__ void lstm_cell_bwd_kernel(LstmCellBwdArgs a) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= a.B * a.H) return;
  lstm_cell_bwd_elem(a, idx, a.dh_in ? a.dh_in[idx] : 0.f);
}

hipError_t launch_lstm_cell_bwd(const LstmCellBwdArgs& a, hipStream_t stream) {
  const int n = a.B * a.H;
  hipLaunchKernelGGL(lstm_cell_bwd_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, a);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------
// Elementwise pieces of the training step
// ---------------------------------------------------------------------------------------------------------------
// out[t][c] = mean over the window of t (F consecutive rows) of in[.][c]; its adjoint is the same operator.
__global__ void window_mean_kernel(const float* in, int ld_in, float* out, int ld_out, int T, int F, int C) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= T * C) return;
  const int t = idx / C, c = idx - t * C;
  const int w0 = (t / F) * F;
  float s = 0.f;
  for (int f = 0; f < F; ++f) s += in[(size_t)(w0 + f) * ld_in + c];
  out[(size_t)t * ld_out + c] = s / (float)F;
}
hipError_t launch_window_mean(const float* in, int ld_in, float* out, int ld_out, int T, int F, int C, hipStream_t stream) {
  const long n = (long)T * C;
  hipLaunchKernelGGL(window_mean_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, in, ld_in, out, ld_out,
                     T, F, C);
  return hipGetLastError();
}

// out[r][c] = alpha * x[r][c] + beta * y[r][c] over a [rows][cols] block with row strides (out may alias x or y)
__global__ void axpby2d_kernel(int rows, int cols, float alpha, const float* x, int ldx, float beta, const float* y, int ldy,
                               float* out, int ldo) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)rows * cols) return;
  const int r = (int)(idx / cols), c = (int)(idx - (long)r * cols);
  const float xv = x ? x[(size_t)r * ldx + c] : 0.f;
  const float yv = y ? y[(size_t)r * ldy + c] : 0.f;
  out[(size_t)r * ldo + c] = alpha * xv + beta * yv;
}
hipError_t launch_axpby2d(int rows, int cols, float alpha, const float* x, int ldx, float beta, const float* y, int ldy,
                          float* out, int ldo, hipStream_t stream) {
  const long n = (long)rows * cols;
  hipLaunchKernelGGL(axpby2d_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, rows, cols, alpha, x, ldx,
                     beta, y, ldy, out, ldo);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------
// The bookkeeping of the LGD loop around the update networks, one launch each instead of a handful of axpby / mean
// launches (at the reference's training batch of 12 windows a step is launch-bound: every launch saved is ~5 us).
// Same operations in the same order as the separate kernels they replace.
// ---------------------------------------------------------------------------------------------------------------
// X[t] = [ x0[t] (d_in) | pose[t] (66) | shape[t] (10) | (the gradient columns are written by the body-model kernel) ]
__global__ void lgd_assemble_kernel(int T, int d_in, const float* x0, int ld0, const float* pose, const float* shape,
                                    float* X, int ldx) {
  const int w = d_in + 76;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)T * w) return;
  const int t = (int)(idx / w), c = (int)(idx - (long)t * w);
  float v;
  if (c < d_in) v = x0[(size_t)t * ld0 + c];
  else if (c < d_in + 66) v = pose[(size_t)t * 66 + (c - d_in)];
  else v = shape[(size_t)t * 10 + (c - d_in - 66)];
  X[(size_t)t * ldx + c] = v;
}
hipError_t launch_lgd_assemble(int T, int d_in, const float* x0, int ld0, const float* pose, const float* shape, float* X,
                               int ldx, hipStream_t stream) {
  const long n = (long)T * (d_in + 76);
  hipLaunchKernelGGL(lgd_assemble_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, T, d_in, x0, ld0, pose,
                     shape, X, ldx);
  return hipGetLastError();
}

// pose_next = pose + step * d_pose;  shape_next = shape + step * (shape_avg ? window mean of d_shape : d_shape).
// One workgroup per window of F frames (reference models.py:529-535, 588-600).
// (grid (B, 1 + LGD_POSE_PARTS): y = 0 the window's shape columns -- the only part that needs the whole window --, y >= 1 a
// slice of its F x 66 pose entries; one workgroup per window was a serial walk of ten loads deep, 12-18 us per launch at the
// reference's 12 windows.  Same arithmetic per element.)
constexpr int LGD_POSE_PARTS = 4;
__global__ __launch_bounds__(256) void lgd_update_kernel(int F, float step, int shape_avg, const float* pose,
                                                         const float* d_pose, const float* shape, const float* d_shape,
                                                         float* pose_next, float* shape_next) {
  __shared__ float mean[10];
  const size_t t0 = (size_t)blockIdx.x * F;
  if (blockIdx.y > 0) {
    const int n = F * 66, per = (n + LGD_POSE_PARTS - 1) / LGD_POSE_PARTS;
    const int lo = (blockIdx.y - 1) * per, hi = min(n, lo + per);
    for (int i = lo + threadIdx.x; i < hi; i += 256) pose_next[t0 * 66 + i] = step * d_pose[t0 * 66 + i] + pose[t0 * 66 + i];
    return;
  }
  if (shape_avg && threadIdx.x < 10) {
    float s = 0.f;
    for (int f = 0; f < F; ++f) s += d_shape[(t0 + f) * 10 + threadIdx.x];
    mean[threadIdx.x] = s / (float)F;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < F * 10; i += 256) {
    const int k = i % 10;
    const float d = shape_avg ? mean[k] : d_shape[t0 * 10 + i];
    shape_next[t0 * 10 + i] = step * d + shape[t0 * 10 + i];
  }
}
hipError_t launch_lgd_update(int B, int F, float step, int shape_avg, const float* pose, const float* d_pose,
                             const float* shape, const float* d_shape, float* pose_next, float* shape_next,
                             hipStream_t stream) {
  hipLaunchKernelGGL(lgd_update_kernel, dim3(B, 1 + LGD_POSE_PARTS), dim3(256), 0, stream, F, step, shape_avg, pose, d_pose,
                     shape, d_shape, pose_next, shape_next);
  return hipGetLastError();
}

// Reverse sweep, entry i of the histories: the running cotangents of the estimates
//   Dp = [Dp +] d_pose_i + vp_i [+ g_theta_i / T],   Ds likewise           (loss terms, body-model VJP, the reference's
//   in-forward E_i.backward() deposit, models.py:576)
// and, for i > 0, the cotangents of the update networks' outputs of iteration i - 1, zero-padded to the GEMM grid:
//   dpad[:, :66] = step * Dp,   dspad[:, :10] = step * (shape_avg ? window mean of Ds : Ds)   (adjoint of the mean = mean)
// (the padding columns are written too, so the destinations may be uninitialised memory: the stash slots of
// empose_mlp_train_bwd_deferred)
__global__ __launch_bounds__(256) void lgd_cotangent_kernel(int F, float inv_T, int first, const float* d_pose,
                                                            const float* d_shape, const float* vp, const float* vs,
                                                            const float* g_theta, int ld_g, const float* g_beta, int ld_gb,
                                                            float* Dp, float* Ds, float step, int shape_avg, float* dpad,
                                                            float* dspad) {
  extern __shared__ float sds[];   // [F][10]
  const size_t t0 = (size_t)blockIdx.x * F;
  if (blockIdx.y > 0) {            // a slice of the window's F x 66 pose entries (grid as lgd_update_kernel)
    const int n = F * 66, per = (n + LGD_POSE_PARTS - 1) / LGD_POSE_PARTS;
    const int lo = (blockIdx.y - 1) * per, hi = min(n, lo + per);
    for (int i = lo + threadIdx.x; i < hi; i += 256) {
      const int f = i / 66, c = i - f * 66;
      const size_t t = t0 + f;
      float v = d_pose[t * 66 + c];
      if (!first) v = v + Dp[t * 66 + c];
      v = vp[t * 66 + c] + v;
      if (g_theta) v = inv_T * g_theta[t * ld_g + c] + v;
      Dp[t * 66 + c] = v;
      if (dpad) {
        dpad[t * 68 + c] = step * v;
        if (c >= 64) dpad[t * 68 + c + 2] = 0.f;   // the two padding columns
      }
    }
    return;
  }
  for (int i = threadIdx.x; i < F * 10; i += 256) {
    const int f = i / 10, k = i - f * 10;
    const size_t t = t0 + f;
    float v = d_shape[t * 10 + k];
    if (!first) v = v + Ds[t * 10 + k];
    v = vs[t * 10 + k] + v;
    if (g_beta) v = inv_T * g_beta[t * ld_gb + k] + v;
    Ds[t * 10 + k] = v;
    sds[f * 10 + k] = v;
  }
  if (!dspad) return;
  __syncthreads();
  for (int i = threadIdx.x; i < F * 10; i += 256) {
    const int f = i / 10, k = i - f * 10;
    float v;
    if (shape_avg) {
      float s = 0.f;
      for (int ff = 0; ff < F; ++ff) s += sds[ff * 10 + k];
      v = s / (float)F;
    } else {
      v = sds[i];
    }
    dspad[(t0 + f) * 12 + k] = step * v;
    if (k >= 8) dspad[(t0 + f) * 12 + k + 2] = 0.f;   // padding columns
  }
}
hipError_t launch_lgd_cotangent(int B, int F, int first, const float* d_pose, const float* d_shape, const float* vp,
                                const float* vs, const float* g_theta, int ld_g, const float* g_beta, int ld_gb, float* Dp,
                                float* Ds, float step, int shape_avg, float* dpad, float* dspad, hipStream_t stream) {
  const float inv_T = 1.f / (float)((long)B * F);
  hipLaunchKernelGGL(lgd_cotangent_kernel, dim3(B, 1 + LGD_POSE_PARTS), dim3(256), (size_t)F * 10 * sizeof(float), stream, F, inv_T, first,
                     d_pose, d_shape, vp, vs, g_theta, ld_g, g_beta, ld_gb, Dp, Ds, step, shape_avg, dpad, dspad);
  return hipGetLastError();
}

}  // namespace empose
