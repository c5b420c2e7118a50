// The optimiser step of the training engine: Adam over a list of tensors in one launch.
#include "train_kernels.h"

namespace empose {

// ---------------------------------------------------------------------------------------------------------------
// Adam over a list of tensors in one launch (torch.optim.Adam semantics, amsgrad off, weight_decay 0):
//   m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g^2;  p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
// chunk c covers elements [off, off + ADAM_CHUNK) of tensor `tensor_of_chunk[c]`.
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void adam_kernel(AdamArgs a) {
  const int ch = blockIdx.x;
  const int ti = a.chunk_tensor[ch];
  const long base = (long)a.chunk_offset[ch];
  const long n = a.sizes[ti];
  float* p = reinterpret_cast<float*>(a.params[ti]);
  const float* g = reinterpret_cast<const float*>(a.grads[ti]);
  float* m = reinterpret_cast<float*>(a.exp_avg[ti]);
  float* v = reinterpret_cast<float*>(a.exp_avg_sq[ti]);
  for (int k = threadIdx.x; k < ADAM_CHUNK; k += 256) {
    const long i = base + k;
    if (i >= n) break;
    const float gi = g[i];
    const float mi = a.beta1 * m[i] + (1.f - a.beta1) * gi;
    const float vi = a.beta2 * v[i] + (1.f - a.beta2) * gi * gi;
    m[i] = mi; v[i] = vi;
    p[i] -= a.step_size * mi / (sqrtf(vi) * a.inv_sqrt_bc2 + a.eps);
  }
}
hipError_t launch_adam(const AdamArgs& a, int n_chunks, hipStream_t stream) {
  hipLaunchKernelGGL(adam_kernel, dim3(n_chunks), dim3(256), 0, stream, a);
  return hipGetLastError();
}

}  // namespace empose
