// Evaluation metrics on the device (reference empose/eval/metrics.py:18-66,110-162 and
// helpers/utils.py:165-199): per frame the Euclidean joint distances, the distances after a similarity Procrustes
// alignment of the prediction onto the ground truth (the reference runs a NumPy SVD per frame in a Python loop), and
// the geodesic angle between predicted and ground-truth GLOBAL joint orientations.
// One thread per frame, float64 arithmetic (the accumulated rows feed means / standard deviations on the host).
#include "data_kernels.h"
#include "svd3.h"

namespace empose {

constexpr int MJ = 22;

// reference helpers/so3.py:86-128 (clamped-angle Rodrigues), in float64
__device__ inline void exp_map(const float* r, double* R) {
  const double x = r[0], y = r[1], z = r[2];
  const double n2 = x * x + y * y + z * z;
  const double a = sqrt(n2 > 1e-4 ? n2 : 1e-4);
  const double f1 = sin(a) / a, f2 = (1.0 - cos(a)) / (a * a);
  const double K[9] = {0, -z, y, z, 0, -x, -y, x, 0};
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      double kk = 0;
      for (int k = 0; k < 3; ++k) kk += K[i * 3 + k] * K[k * 3 + j];
      R[i * 3 + j] = f1 * K[i * 3 + j] + f2 * kk + (i == j ? 1.0 : 0.0);
    }
}

__global__ void metrics_rows_kernel(MetricsArgs a) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= a.T) return;
  const float* X = a.joints_gt + (size_t)t * MJ * 3;
  const float* Y = a.joints_hat + (size_t)t * MJ * 3;
  double* row = a.rows + (size_t)t * 65;

  // ---- Euclidean distances and Procrustes (align Y onto X; metrics.py:18-66 with optimal scale)
  double muX[3] = {0, 0, 0}, muY[3] = {0, 0, 0};
  for (int j = 0; j < MJ; ++j)
    for (int c = 0; c < 3; ++c) { muX[c] += X[j * 3 + c]; muY[c] += Y[j * 3 + c]; }
  for (int c = 0; c < 3; ++c) { muX[c] /= MJ; muY[c] /= MJ; }
  double ssX = 0, ssY = 0, A[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int j = 0; j < MJ; ++j) {
    double dx[3], dy[3];
    for (int c = 0; c < 3; ++c) { dx[c] = X[j * 3 + c] - muX[c]; dy[c] = Y[j * 3 + c] - muY[c]; }
    for (int c = 0; c < 3; ++c) { ssX += dx[c] * dx[c]; ssY += dy[c] * dy[c]; }
    for (int i = 0; i < 3; ++i)
      for (int k = 0; k < 3; ++k) A[i * 3 + k] += dx[i] * dy[k];  // X0^T Y0 (un-normalised)
    const double ex = (double)X[j * 3] - Y[j * 3], ey = (double)X[j * 3 + 1] - Y[j * 3 + 1],
                 ez = (double)X[j * 3 + 2] - Y[j * 3 + 2];
    row[j] = sqrt(ex * ex + ey * ey + ez * ez);
  }
  const double normX = sqrt(ssX), normY = sqrt(ssY);
  for (int i = 0; i < 9; ++i) A[i] /= (normX * normY);
  // SVD A = U S V^T by one-sided Jacobi, singular values in descending order
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
  // U is built right-handed: u1, u2 from the columns (any unit vector orthogonal to u1 when s2 == 0: collinear points),
  // u3 = u1 x u2 and s3 = u3 . A v3 signed, so that A = U S V^T holds whatever s3 is (a normalised A v3 is rounding
  // noise, not orthogonal to u1 and u2, when s3 is tiny: near-planar ground truth).  A NaN A (no spread) stays NaN in S.
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
  double Tm[9];
  for (int i = 0; i < 3; ++i)
    for (int k = 0; k < 3; ++k) {
      double s = 0;
      for (int m = 0; m < 3; ++m) s += Vs[i * 3 + m] * U[k * 3 + m];
      Tm[i * 3 + k] = s;
    }
  if (det3(Tm) < 0) {  // make it a rotation (metrics.py:46-50)
    for (int r = 0; r < 3; ++r) Vs[r * 3 + 2] = -Vs[r * 3 + 2];
    S[2] = -S[2];
    for (int i = 0; i < 3; ++i)
      for (int k = 0; k < 3; ++k) {
        double s = 0;
        for (int m = 0; m < 3; ++m) s += Vs[i * 3 + m] * U[k * 3 + m];
        Tm[i * 3 + k] = s;
      }
  }
  const double trace = S[0] + S[1] + S[2];
  for (int j = 0; j < MJ; ++j) {
    double y0[3], z[3];
    for (int c = 0; c < 3; ++c) y0[c] = (Y[j * 3 + c] - muY[c]) / normY;
    for (int c = 0; c < 3; ++c)
      z[c] = normX * trace * (y0[0] * Tm[0 * 3 + c] + y0[1] * Tm[1 * 3 + c] + y0[2] * Tm[2 * 3 + c]) + muX[c];
    const double ex = X[j * 3] - z[0], ey = X[j * 3 + 1] - z[1], ez = X[j * 3 + 2] - z[2];
    row[22 + j] = sqrt(ex * ex + ey * ey + ez * ez);
  }

  // ---- global joint-angle error (root = identity; metrics.py:229-237, utils.py:165-199)
  if (!a.pose_gt) {
    for (int j = 0; j < MJ - 1; ++j) row[44 + j] = 0.0;
    return;
  }
  double Gg[MJ * 9], Gh[MJ * 9];
  for (int i = 0; i < 9; ++i) Gg[i] = Gh[i] = (i % 4 == 0) ? 1.0 : 0.0;
  const float* pg = a.pose_gt + (size_t)t * 63;
  const float* ph = a.pose_hat + (size_t)t * 63;
  for (int j = 1; j < MJ; ++j) {
    double Lg[9], Lh[9];
    exp_map(pg + (j - 1) * 3, Lg);
    exp_map(ph + (j - 1) * 3, Lh);
    const int p = a.parents[j];
    double tr = 0;
    for (int i = 0; i < 3; ++i)
      for (int k = 0; k < 3; ++k) {
        double sg = 0, sh = 0;
        for (int m = 0; m < 3; ++m) {
          sg += Gg[p * 9 + i * 3 + m] * Lg[m * 3 + k];
          sh += Gh[p * 9 + i * 3 + m] * Lh[m * 3 + k];
        }
        Gg[j * 9 + i * 3 + k] = sg;
        Gh[j * 9 + i * 3 + k] = sh;
      }
    for (int i = 0; i < 9; ++i) tr += Gg[j * 9 + i] * Gh[j * 9 + i];
    double cosv = (tr - 1.0) * 0.5;
    cosv = cosv > 1.0 ? 1.0 : (cosv < -1.0 ? -1.0 : cosv);
    row[44 + j - 1] = acos(cosv) * 57.29577951308232;
  }
}

hipError_t launch_metrics_rows(const MetricsArgs& a, hipStream_t stream) {
  hipLaunchKernelGGL(metrics_rows_kernel, dim3((a.T + 63) / 64), dim3(64), 0, stream, a);
  return hipGetLastError();
}

}  // namespace empose
