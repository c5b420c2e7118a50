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

// The orthogonal part of a similarity Procrustes alignment from A = X0^T Y0 / (normX normY) (X0, Y0 the centred point
// sets as rows): Tm such that Y0 Tm is Y0 rotated onto X0, and the returned trace s1 + s2 + s3 (the scale is
// normX / normY times it).  The steps of metrics_rows_kernel (metrics.hip), which the joints use: singular values in
// descending order, U built right-handed so that A = U S V^T holds whatever s3 is, the last singular vector and value
// flipped by sign(det) (reference eval/metrics.py:18-66).  A NaN in A gives NaNs, in a bounded number of steps.
__device__ inline double procrustes_rotation(const double A[9], double Tm[9]) {
  double W[9], V[9], nrm[3];
  for (int i = 0; i < 9; ++i) W[i] = A[i];
  svd3_one_sided(W, V);
  for (int c = 0; c < 3; ++c) nrm[c] = sqrt(W[c] * W[c] + W[3 + c] * W[3 + c] + W[6 + c] * W[6 + c]);
  int ord[3] = {0, 1, 2};
  for (int i = 0; i < 2; ++i)
    for (int k = i + 1; k < 3; ++k)
      if (nrm[ord[k]] > nrm[ord[i]]) { const int tmp = ord[i]; ord[i] = ord[k]; ord[k] = tmp; }
  double Vs[9], U[9], S[3];
  for (int c = 0; c < 3; ++c) {
    S[c] = nrm[ord[c]];
    for (int r = 0; r < 3; ++r) Vs[r * 3 + c] = V[r * 3 + ord[c]];
  }
  double u1[3], u2[3];
  for (int r = 0; r < 3; ++r) u1[r] = S[0] > 0 ? W[r * 3 + ord[0]] / S[0] : (r == 0 ? 1.0 : 0.0);
  if (S[1] > 0) {
    for (int r = 0; r < 3; ++r) u2[r] = W[r * 3 + ord[1]] / S[1];
  } else {
    int k = 0;  // e_k with the smallest |u1_k|, minus its u1 part
    for (int r = 1; r < 3; ++r)
      if (fabs(u1[r]) < fabs(u1[k])) k = r;
    double n = 0;
    for (int r = 0; r < 3; ++r) {
      u2[r] = (r == k ? 1.0 : 0.0) - u1[k] * u1[r];
      n += u2[r] * u2[r];
    }
    n = sqrt(n);
    for (int r = 0; r < 3; ++r) u2[r] /= n;
  }
  const double u3[3] = {u1[1] * u2[2] - u1[2] * u2[1], u1[2] * u2[0] - u1[0] * u2[2], u1[0] * u2[1] - u1[1] * u2[0]};
  S[2] = u3[0] * W[ord[2]] + u3[1] * W[3 + ord[2]] + u3[2] * W[6 + ord[2]];
  for (int r = 0; r < 3; ++r) { U[r * 3] = u1[r]; U[r * 3 + 1] = u2[r]; U[r * 3 + 2] = u3[r]; }
  auto v_ut = [&]() {
    for (int i = 0; i < 3; ++i)
      for (int k = 0; k < 3; ++k) {
        double s = 0;
        for (int m = 0; m < 3; ++m) s += Vs[i * 3 + m] * U[k * 3 + m];
        Tm[i * 3 + k] = s;
      }
  };
  v_ut();
  if (det3(Tm) < 0) {  // make it a rotation
    for (int r = 0; r < 3; ++r) Vs[r * 3 + 2] = -Vs[r * 3 + 2];
    S[2] = -S[2];
    v_ut();
  }
  return S[0] + S[1] + S[2];
}

}  // namespace empose
