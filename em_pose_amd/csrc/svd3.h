// 3 x 3 singular value decomposition by one-sided Jacobi and the determinant, float64, as device functions: shared by the
// metrics kernel (metrics.hip, Procrustes alignment) and the offset statistics (offset_stats.hip, the rotation closest to
// a mean of rotations).
#pragma once
#include <hip/hip_runtime.h>

namespace empose {

__device__ inline void svd3_one_sided(double W[9], double V[9]) {
  // one-sided (Hestenes) Jacobi: rotate pairs of columns of W (= A on entry) until they are orthogonal; on return
  // W = A V = U S (columns u_c s_c) and V is orthogonal.  Works on A itself, not on A^T A, so a singular value is
  // resolved down to ~1e-16 of the largest one (A^T A squares the condition number: s3 below ~1e-8 s1 was noise)
  for (int i = 0; i < 9; ++i) V[i] = (i % 4 == 0) ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 30; ++sweep) {
    bool rotated = false;
    for (int p = 0; p < 2; ++p)
      for (int q = p + 1; q < 3; ++q) {
        double al = 0, be = 0, ga = 0;
        for (int r = 0; r < 3; ++r) {
          al += W[r * 3 + p] * W[r * 3 + p];
          be += W[r * 3 + q] * W[r * 3 + q];
          ga += W[r * 3 + p] * W[r * 3 + q];
        }
        if (!(fabs(ga) > 1e-15 * sqrt(al * be))) continue;   // orthogonal to rounding (or NaN: left as it is)
        rotated = true;
        const double zeta = (be - al) / (2.0 * ga);
        const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
        const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
        for (int r = 0; r < 3; ++r) {
          const double wp = W[r * 3 + p], wq = W[r * 3 + q];
          W[r * 3 + p] = c * wp - s * wq;
          W[r * 3 + q] = s * wp + c * wq;
          const double vp = V[r * 3 + p], vq = V[r * 3 + q];
          V[r * 3 + p] = c * vp - s * vq;
          V[r * 3 + q] = s * vp + c * vq;
        }
      }
    if (!rotated) break;
  }
}

__device__ inline double det3(const double* M) {
  return M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6]) + M[2] * (M[3] * M[7] - M[4] * M[6]);
}

}  // namespace empose
