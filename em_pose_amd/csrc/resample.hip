// Resampling of motion sequences to another frame rate (reference scripts/preprocess_amass_3dpw.py:63-123), gfx950 only.
// A launch processes a ragged batch of S sequences: the table `seqs` gives, per sequence, its first input row, F_in, its
// first output row, F_out and its two rates.  Knots are uniform, ts_in[k] = k / fps_in; output frame k of a sequence is at
// t = k / fps_out, u = t * fps_in in knot units, segment i = min(floor(u), F_in - 2), tau = u - i.  tau exceeds 1 where
// t lies past the last knot (by less than one input interval): the last segment's formula extrapolates, nothing clamps.
// F_out comes from the host (np.arange's own count) and is trusted.  All I/O is float32, every thread computes in double
// (as the reverse of root_frame.hip, for the same reason: rotation vector <-> quaternion <-> log in float32 costs more
// than the float32 rounding of inputs and outputs); the work per thread is tiny.  An output frame finds its sequence by
// bisection over the table's output rows, so a result does not depend on what else is in the batch.
//
// Rotations, one thread per (output frame, joint), no LDS, no barrier: Shoemake's SQUAD on uniform knots,
//   s_i = q_i exp((log(q_{i-1}^-1 q_i) - log(q_i^-1 q_{i+1})) / 4)
//   out = slerp(slerp(q_i, q_{i+1}, tau), slerp(s_i, s_{i+1}, tau), 2 tau (1 - tau)),  slerp(a, b, t) = a exp(t log(a^-1 b))
// on the four knots i-1 .. i+2 made hemisphere-consistent from q_i outwards (q_{i+1} against q_i, q_{i+2} against the
// fixed q_{i+1}, q_{i-1} against q_i): the reference's sequential pass along time up to one common sign of the stencil,
// which does not change the rotation.  A knot that does not exist is the constant-velocity phantom q_{-1} = q_0 q_1^-1 q_0
// or q_F = q_{F-1} q_{F-2}^-1 q_{F-1}, for which the two logarithms of s cancel: s_0 = q_0 and s_{F-1} = q_{F-1}, set
// directly.  F_in = 2 is therefore plain slerp.  The output is the rotation vector of the result with w >= 0: |r| <= pi.
//
// Positions: the not-a-knot cubic spline of scipy.interpolate.CubicSpline(ts_in, x, axis=0), in two launches.
//   1. One thread per (sequence, channel) solves the first-derivative system D (in knot units, D = h x') by a serial
//      Thomas sweep, in double, into the workspace (one double per input row and channel):
//        D_0 + 2 D_1 = (5 d_0 + d_1) / 2,  D_{k-1} + 4 D_k + D_{k+1} = 3 (x_{k+1} - x_{k-1}),
//        2 D_{n-2} + D_{n-1} = (d_{n-3} + 5 d_{n-2}) / 2,   d_k = x_{k+1} - x_k.
//      Elimination needs no pivoting (pivots 1, 2, 3.5, ... -> 2 + sqrt 3, last 1 - 2 c ~ 0.46).  The ratios c_k =
//      1 / pivot_k do not depend on the data: c_0 = 2, c_k = 1 / (4 - c_{k-1}), a contraction by 0.072 per step, so beyond
//      32 knots c_k is the limit 2 - sqrt 3 to far less than a rounding; a compile-time table holds the first 32.
//      n = 2 is the straight line and n = 3 the parabola through the three points, scipy's special cases.
//   2. One thread per (output frame, channel) evaluates the Hermite form of segment i at tau (past the last knot: the
//      last polynomial, as scipy extrapolates).
// One fixed order, no atomics: repeated launches give the same bits.
#include <hip/hip_runtime.h>

#include "data_kernels.h"
#include "quat.h"

namespace empose {

namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_CP = 32;      // tabulated elimination ratios
constexpr int RS_CHUNK = 32;   // knots loaded ahead of the serial recurrence

struct CpTable { double v[RS_CP]; };
constexpr CpTable make_cp_table() {
  CpTable t{};
  t.v[0] = 2.0;
  for (int k = 1; k < RS_CP; ++k) t.v[k] = 1.0 / (4.0 - t.v[k - 1]);
  return t;
}
__constant__ CpTable rs_cp = make_cp_table();

// the sequence that owns output row `row`: the last one whose first output row is <= row
__device__ __forceinline__ int find_seq(const ResampleSeq* seqs, int S, long row) {
  int lo = 0, hi = S - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if ((long)seqs[mid].out_row <= row) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// segment and parameter of output frame k
__device__ __forceinline__ void locate(const ResampleSeq& q, long k, int& i, double& tau) {
  const double t = (double)k / q.fps_out, u = t * q.fps_in;
  double fl = floor(u);
  const double last = (double)(q.f_in - 2);
  if (fl > last) fl = last;
  if (fl < 0.0) fl = 0.0;
  i = (int)fl;
  tau = u - fl;
}

__global__ void __launch_bounds__(RS_THREADS) resample_rotations_kernel(ResampleArgs a) {
  const long g = (long)blockIdx.x * RS_THREADS + threadIdx.x;
  if (g >= a.out_rows * a.n) return;
  const long row = g / a.n;
  const int j = (int)(g - row * a.n);
  const ResampleSeq q = a.seqs[find_seq(a.seqs, a.S, row)];
  int i;
  double tau;
  locate(q, row - q.out_row, i, tau);
  const float* knot = a.in + ((long)q.in_row + i) * a.ld_in + j * 3;   // knot i of this joint
  const Quat q1 = q_from_rotvec(knot);
  const Quat q2 = q_toward(q1, q_from_rotvec(knot + a.ld_in));
  double l12[3];
  q_log(q_conj_mul(q1, q2), l12);
  Quat s1 = q1, s2 = q2;
  if (i > 0) {
    const Quat q0 = q_toward(q1, q_from_rotvec(knot - a.ld_in));
    double l01[3];
    q_log(q_conj_mul(q0, q1), l01);
    const double v[3] = {0.25 * (l01[0] - l12[0]), 0.25 * (l01[1] - l12[1]), 0.25 * (l01[2] - l12[2])};
    s1 = q_mul(q1, q_exp(v));
  }
  if (i + 2 < q.f_in) {
    const Quat q3 = q_toward(q2, q_from_rotvec(knot + 2L * a.ld_in));
    double l23[3];
    q_log(q_conj_mul(q2, q3), l23);
    const double v[3] = {0.25 * (l12[0] - l23[0]), 0.25 * (l12[1] - l23[1]), 0.25 * (l12[2] - l23[2])};
    s2 = q_mul(q2, q_exp(v));
  }
  const Quat A = q_step(q1, l12, tau);
  double ls[3], lab[3];
  q_log(q_conj_mul(s1, s2), ls);
  const Quat B = q_step(s1, ls, tau);
  q_log(q_conj_mul(A, B), lab);
  Quat r = q_step(A, lab, 2.0 * tau * (1.0 - tau));
  if (r.w < 0.0) r = {-r.w, -r.x, -r.y, -r.z};
  const double s = sqrt(r.x * r.x + r.y * r.y + r.z * r.z);
  const double k = s < 1e-8 ? 2.0 / r.w : 2.0 * atan2(s, r.w) / s;
  float* o = a.out + row * a.ld_out + j * 3;
  o[0] = (float)(k * r.x); o[1] = (float)(k * r.y); o[2] = (float)(k * r.z);
}

// ---- positions ----------------------------------------------------------------------------------------------------------
// The derivative system of one (sequence, channel): see the header.
__global__ void __launch_bounds__(RS_THREADS) resample_spline_solve_kernel(ResampleArgs a) {
  const long g = (long)blockIdx.x * RS_THREADS + threadIdx.x;
  if (g >= (long)a.S * a.n) return;
  const int s = (int)(g / a.n), c = (int)(g - (long)s * a.n);
  const ResampleSeq q = a.seqs[s];
  const int n = q.f_in, C = a.n;
  const float* __restrict__ x = a.in + (long)q.in_row * a.ld_in + c;
  double* __restrict__ D = a.ws + (long)q.in_row * C + c;
  const long ld = a.ld_in;
  if (n == 2) {
    D[0] = D[C] = (double)x[ld] - (double)x[0];
    return;
  }
  if (n == 3) {
    const double d0 = (double)x[ld] - (double)x[0], d1 = (double)x[2 * ld] - (double)x[ld];
    D[0] = 0.5 * (3.0 * d0 - d1);
    D[C] = 0.5 * (d0 + d1);
    D[2L * C] = 0.5 * (3.0 * d1 - d0);
    return;
  }
  const double cinf = rs_cp.v[RS_CP - 1];
  // forward: d'_k into D
  double dprev = 0.5 * (5.0 * ((double)x[ld] - (double)x[0]) + ((double)x[2 * ld] - (double)x[ld]));
  D[0] = dprev;
  for (int k0 = 1; k0 <= n - 2; k0 += RS_CHUNK) {
    double xv[RS_CHUNK + 2];   // x[k0 - 1 .. k0 + RS_CHUNK], rows past the end repeat the last (unused)
#pragma unroll
    for (int m = 0; m < RS_CHUNK + 2; ++m) {
      const int r = k0 - 1 + m;
      xv[m] = (double)x[(long)(r < n ? r : n - 1) * ld];
    }
#pragma unroll
    for (int m = 0; m < RS_CHUNK; ++m) {
      const int k = k0 + m;
      if (k <= n - 2) {
        const double ck = k < RS_CP ? rs_cp.v[k] : cinf;
        dprev = (3.0 * (xv[m + 2] - xv[m]) - dprev) * ck;
        D[(long)k * C] = dprev;
      }
    }
  }
  // last row, then back-substitution in place
  const double cl = (n - 2) < RS_CP ? rs_cp.v[n - 2] : cinf;
  const double xa = x[(long)(n - 3) * ld], xb = x[(long)(n - 2) * ld], xc = x[(long)(n - 1) * ld];
  double next = (0.5 * ((xb - xa) + 5.0 * (xc - xb)) - 2.0 * dprev) / (1.0 - 2.0 * cl);
  D[(long)(n - 1) * C] = next;
  for (int k0 = n - 2; k0 >= 0; k0 -= RS_CHUNK) {
    double dv[RS_CHUNK];
#pragma unroll
    for (int m = 0; m < RS_CHUNK; ++m) {
      const int r = k0 - m;
      dv[m] = D[(long)(r > 0 ? r : 0) * C];
    }
#pragma unroll
    for (int m = 0; m < RS_CHUNK; ++m) {
      const int k = k0 - m;
      if (k >= 0) {
        const double ck = k < RS_CP ? rs_cp.v[k] : cinf;
        next = dv[m] - ck * next;
        D[(long)k * C] = next;
      }
    }
  }
}

__global__ void __launch_bounds__(RS_THREADS) resample_spline_eval_kernel(ResampleArgs a) {
  const long g = (long)blockIdx.x * RS_THREADS + threadIdx.x;
  if (g >= a.out_rows * a.n) return;
  const long row = g / a.n;
  const int c = (int)(g - row * a.n);
  const ResampleSeq q = a.seqs[find_seq(a.seqs, a.S, row)];
  int i;
  double tau;
  locate(q, row - q.out_row, i, tau);
  const float* x = a.in + ((long)q.in_row + i) * a.ld_in + c;
  const double* D = a.ws + ((long)q.in_row + i) * a.n + c;
  const double x0 = x[0], d = (double)x[a.ld_in] - x0, D0 = D[0], D1 = D[a.n];
  const double c2 = 3.0 * d - 2.0 * D0 - D1, c3 = D0 + D1 - 2.0 * d;
  a.out[row * a.ld_out + c] = (float)(x0 + tau * (D0 + tau * (c2 + tau * c3)));
}

unsigned blocks_for(long threads) { return (unsigned)((threads + RS_THREADS - 1) / RS_THREADS); }

}  // namespace

hipError_t launch_resample_rotations(const ResampleArgs& a, hipStream_t stream) {
  hipLaunchKernelGGL(resample_rotations_kernel, dim3(blocks_for(a.out_rows * a.n)), dim3(RS_THREADS), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_resample_positions(const ResampleArgs& a, hipStream_t stream) {
  hipLaunchKernelGGL(resample_spline_solve_kernel, dim3(blocks_for((long)a.S * a.n)), dim3(RS_THREADS), 0, stream, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(resample_spline_eval_kernel, dim3(blocks_for(a.out_rows * a.n)), dim3(RS_THREADS), 0, stream, a);
  return hipGetLastError();
}

}  // namespace empose
