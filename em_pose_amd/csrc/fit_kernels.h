// Launch interfaces of the model-free sensor fit (sensor_fit.hip).  Internal, not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace empose {

// Model-free sensor fitting (sensor_fit.hip): first-order descent on the sensor residual plus priors, per window w
//   J_w = sum_t s_t E_t + lambda_pose / 2 sum_{t live} |theta_t[3:66] - p_t[3:66]|^2 + lambda_shape / 2 |beta_w|^2
//         + lambda_smooth / 2 sum_{t >= 1, live} |theta_t - theta_{t-1}|^2        
// What the three kernels share: the window batch, the readings and the weights of the terms.
struct FitProblem {
  const float* tgt; int ld_tgt;     // [T][ld_tgt]: n_markers * 3 positions, then n_markers * 9 orientations
  const float* s;                   // [T] frame weight of the data term (0 or 1)
  const int* seq_lengths;           // [B] or nullptr (= F everywhere)
  const float* prior;               // [T][66] or nullptr (zeros)
  int B, F, n_markers;
  int used_slot[12];                // sensor -> slot in a target row, -1: not read by the model
  float lambda_pose, lambda_shape, lambda_smooth;
  int shape_per_window;             // 1: one shape per window (every row of a window holds it), 0: one per frame
};
struct FitPrepareArgs {
  FitProblem p;
  const float* marker_masks;        // [T][12] or nullptr
  const float* pose_init; const float* shape_init;   // [T][66], [T][10] or nullptr (zeros)
  float* theta; float* beta;        // [T][66], [T][10]: the iterate 0
  float* moments; size_t n_moments; // zeroed
  float* s;                         // [T] written
  float* best_J;                    // [B] = +inf
};
struct FitStepArgs {
  FitProblem p;
  const float* theta; const float* beta;       // iterate k
  const float* g_theta; const float* g_beta;   // [T][66], [T][10] gradient of sum_t s_t E_t at iterate k
  const float* pos; const float* ori;          // [T][36], [T][108] sensors of iterate k
  float* m_theta; float* v_theta;              // [T][66] Adam moments, updated in place (live frames)
  float* m_beta; float* v_beta;                // [T][10]; one shape per window: the window's first row only
  float* theta_next; float* beta_next;         // iterate k + 1 (never the buffers of iterate k)
  float* energy;                               // [T] s_t E_t or nullptr
  float* J;                                    // [B] J_w at iterate k
  float* best_J; float* best_theta; float* best_beta;   // keep-best ([B], [T][66], [T][10]) or nullptr
  float lr_k, c1, c2, beta1, beta2, eps;       // lr decay^k, 1 / (1 - beta1^(k+1)), 1 / (1 - beta2^(k+1)): rounded by the host
};
struct FitFinishArgs {
  FitProblem p;
  const float* theta; const float* beta;       // iterate K
  const float* pos; const float* ori;          // its sensors
  const float* best_J; const float* best_theta; const float* best_beta;   // or nullptr: the last iterate is returned
  float* pose; float* shape;                   // [T][66], [T][10] what is returned
  float* J_last; float* J_out;                 // [B] J_w of iterate K, and of what is returned
};
hipError_t launch_fit_prepare(const FitPrepareArgs& a, hipStream_t stream);
hipError_t launch_fit_step(const FitStepArgs& a, hipStream_t stream);
hipError_t launch_fit_finish(const FitFinishArgs& a, hipStream_t stream);
// energy[t] = s_t E_t of given sensors (the optional per-frame output of the fit)
hipError_t launch_fit_energy(const FitProblem& p, const float* pos, const float* ori, float* energy, hipStream_t stream);

}  // namespace empose
