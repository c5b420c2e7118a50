// Root normalisation (reference bodymodels/smpl.py:112-119, data/transforms.py:247-254) and its vector-Jacobian product,
// gfx950 only, fp32.  Frames come in segments of seg_len consecutive rows; `first` is the first row of a frame's segment.
//
// Forward, one thread per frame t: R_t = exp(root[t]), R_0 = exp(root[first]) (recomputed by every thread: no LDS, no
// barrier), Rn = R_0^T R_t, root_out[t] = log(Rn) and, by the flags, trans_out[t] = R_0^T trans[t] - R_0^T trans[first]
// (the reference's order: rotate, then subtract the rotated first translation).  The first frame of a segment writes
// exact zeros for the orientation and, when the first translation is subtracted, for the translation.
//   exp  the guarded Rodrigues map of smpl_math.h, in the convention of the caller (EMPOSE_RODRIGUES_*)
//   log  accurate over [0, pi]: the angle is atan2(|w| / 2, (tr Rn - 1) / 2) with w = vee(Rn - Rn^T); below 0.01 rad the
//        factor angle / sin(angle) is a series; where cos(angle) < -1/2 the axis comes from the symmetric part
//        (Rn + Rn^T) / 2 = cos I + (1 - cos) n n^T, its sign from w (free at exactly pi), as transforms.py
//        matrix_to_rotvec does on the host
//
// Reverse: the derivative of the EXACT maps, through the left and right Jacobians of SO(3),
//   Jl(r) = I + a K + b K^2,  a = (1 - cos t) / t^2,  b = (t - sin t) / t^3,  K = hat(r), t = |r|,  Jr = Jl^T
//   Jl^-1(p) = I - K / 2 + c K^2,  c = (1 - (t / 2) cot(t / 2)) / t^2,  Jr^-1 = (Jl^-1)^T
// with series for a, b and c at small angles.  The reverse's per-frame arithmetic is double precision on quaternions
// (inputs, outputs and the sums stay float32): see the note at quat_exp.  With p = log(R_0^T R_t) of the exact maps:
//   g_root[t]      = Jl(root[t]) Jl^-1(p) d_root_out[t]
//   g_root[first]  = Jl(root[first]) sum_t ( -Jr^-1(p_t) d_root_out[t] + d_trans_out[t] x trans_out[t] )
//   g_trans[t]     = R_0 d_trans_out[t],   g_trans[first] = -sum_{t != first} R_0 d_trans_out[t]
// It is finite everywhere, also at Rn = I, where both Jacobians are the identity.  It is NOT the derivative of the
// reference's acos-based so3_log_map: d acos(x) / dx is infinite at x = 1, which every sequence meets at its first
// frame (Rn = I), and the factor in front of it is zero there, so the reference's backward computes 0 * inf.
// The first frame's own cotangent has no effect (its outputs are constants) and is skipped.
//
// The sums of a segment are taken in ascending frame order by one fixed tree: a wave covers 64 consecutive frames of
// one segment and reduces its nine sums over the lanes (lane_reduce.h), the partials of a segment's waves go to the
// workspace, and a second launch adds them in ascending order (a contiguous run per lane, then the same lane reduction)
// and writes the first frame's rows.  No atomics: repeated launches give the same bits.
#include <hip/hip_runtime.h>

#include "data_kernels.h"
#include "lane_reduce.h"
#include "smpl_math.h"

namespace empose {

namespace {

constexpr int RF_THREADS = 256;
constexpr int RF_SUMS = ROOT_FRAME_SUMS;   // per wave: 3 of -Jr^-1 d_root, 3 of d_trans x trans_out, 3 of R_0 d_trans

__device__ __forceinline__ void mat_t_vec(const float (&R)[9], const float* x, float* y) {   // y = R^T x
  y[0] = R[0] * x[0] + R[3] * x[1] + R[6] * x[2];
  y[1] = R[1] * x[0] + R[4] * x[1] + R[7] * x[2];
  y[2] = R[2] * x[0] + R[5] * x[1] + R[8] * x[2];
}

// log of a rotation matrix (to rounding): see the header
__device__ __forceinline__ void so3_log(const float (&R)[9], float* o) {
  const float w[3] = {R[7] - R[5], R[2] - R[6], R[3] - R[1]};
  const float sn = 0.5f * norm3(w), cs = 0.5f * (R[0] + R[4] + R[8] - 1.f);
  const float th = atan2f(sn, cs);
  if (cs > -0.5f) {
    const float t2 = th * th;
    const float k = th < 1e-2f ? 0.5f * (1.f + t2 * (1.f / 6.f + t2 * (7.f / 360.f))) : 0.5f * th / sn;
    o[0] = k * w[0]; o[1] = k * w[1]; o[2] = k * w[2];
    return;
  }
  const int k = (R[0] >= R[4] && R[0] >= R[8]) ? 0 : (R[4] >= R[8] ? 1 : 2);
  const float oc = 1.f - cs;
  const float nk = sqrtf(fmaxf((R[k * 4] - cs) / oc, 0.f));
  const float inv = 0.5f / (oc * nk);
  float n[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) n[i] = i == k ? nk : (R[i * 3 + k] + R[k * 3 + i]) * inv;
  float s = th / norm3(n);
  if (n[0] * w[0] + n[1] * w[1] + n[2] * w[2] < 0.f) s = -s;
  o[0] = s * n[0]; o[1] = s * n[1]; o[2] = s * n[2];
}

// ---- the reverse's arithmetic: double precision, exact maps through unit quaternions -------------------------------
// A float32 evaluation of p = log(Rn) carries ~2e-7 of absolute error into the point where the Jacobians are taken, which
// shows in the gradient at the level the tests hold it to; in double the only float32 rounding is the final store.
struct Quat { double w, x, y, z; };

__device__ __forceinline__ Quat quat_exp(const float* r) {
  const double x = r[0], y = r[1], z = r[2], t2 = x * x + y * y + z * z, t = sqrt(t2);
  const double k = t2 < 1e-8 ? 0.5 - t2 * (1.0 / 48.0) : sin(0.5 * t) / t;
  return {cos(0.5 * t), k * x, k * y, k * z};
}
__device__ __forceinline__ void cross3d(const double* a, const double* b, double* o) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}
// y = R(q) x for sign = 1, R(q)^T x for sign = -1
__device__ __forceinline__ void quat_rot(const Quat& q, double sign, const double* x, double* y) {
  const double v[3] = {sign * q.x, sign * q.y, sign * q.z};
  double t[3], u[3];
  cross3d(v, x, t);
  t[0] *= 2.0; t[1] *= 2.0; t[2] *= 2.0;
  cross3d(v, t, u);
#pragma unroll
  for (int i = 0; i < 3; ++i) y[i] = x[i] + q.w * t[i] + u[i];
}
// p = log(conj(q0) qt), |p| <= pi
__device__ __forceinline__ void quat_rel_log(const Quat& a, const Quat& b, double* p) {
  double w = a.w * b.w + a.x * b.x + a.y * b.y + a.z * b.z;
  double v[3] = {a.w * b.x - b.w * a.x - (a.y * b.z - a.z * b.y), a.w * b.y - b.w * a.y - (a.z * b.x - a.x * b.z),
                 a.w * b.z - b.w * a.z - (a.x * b.y - a.y * b.x)};
  if (w < 0.0) { w = -w; v[0] = -v[0]; v[1] = -v[1]; v[2] = -v[2]; }
  const double s = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
  const double k = s < 1e-8 ? 2.0 / w : 2.0 * atan2(s, w) / s;
  p[0] = k * v[0]; p[1] = k * v[1]; p[2] = k * v[2];
}

// y = Jl(r) x
__device__ __forceinline__ void so3_jl(const double* r, const double* x, double* y) {
  const double t2 = r[0] * r[0] + r[1] * r[1] + r[2] * r[2], t = sqrt(t2);
  double a, b;
  if (t < 0.25) {
    a = 0.5 + t2 * (-1.0 / 24.0 + t2 * (1.0 / 720.0 + t2 * (-1.0 / 40320.0 + t2 * (1.0 / 3628800.0))));
    b = 1.0 / 6.0 + t2 * (-1.0 / 120.0 + t2 * (1.0 / 5040.0 + t2 * (-1.0 / 362880.0 + t2 * (1.0 / 39916800.0))));
  } else {
    const double sh = sin(0.5 * t);
    a = 2.0 * sh * sh / t2;
    b = (t - sin(t)) / (t2 * t);
  }
  double k1[3], k2[3];
  cross3d(r, x, k1);
  cross3d(r, k1, k2);
#pragma unroll
  for (int i = 0; i < 3; ++i) y[i] = x[i] + a * k1[i] + b * k2[i];
}

// yl = Jl^-1(p) x, yr = Jr^-1(p) x; |p| <= pi
__device__ __forceinline__ void so3_jinv(const double* p, const double* x, double* yl, double* yr) {
  const double t2 = p[0] * p[0] + p[1] * p[1] + p[2] * p[2];
  double c;
  if (t2 < 0.0625) {
    c = 1.0 / 12.0 + t2 * (1.0 / 720.0 + t2 * (1.0 / 30240.0 + t2 * (1.0 / 1209600.0 + t2 * (1.0 / 47900160.0))));
  } else {
    const double t = sqrt(t2);
    c = (1.0 - 0.5 * t * cos(0.5 * t) / sin(0.5 * t)) / t2;
  }
  double k1[3], k2[3];
  cross3d(p, x, k1);
  cross3d(p, k1, k2);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    yl[i] = x[i] - 0.5 * k1[i] + c * k2[i];
    yr[i] = x[i] + 0.5 * k1[i] + c * k2[i];
  }
}

// What both directions compute for frame t of a segment starting at `first`: R_0 and the normalised root.
__device__ __forceinline__ void frame_fwd(const RootFrameArgs& a, long t, long first, float (&R0)[9], float* p) {
  const float* r0 = a.root + first * a.ld_root;
  Rod q;
  rodrigues(r0[0], r0[1], r0[2], a.rod_conv, q, R0);
  if (t == first) {
    p[0] = p[1] = p[2] = 0.f;
    return;
  }
  const float* rt = a.root + t * a.ld_root;
  float Rt[9], Rn[9];
  rodrigues(rt[0], rt[1], rt[2], a.rod_conv, q, Rt);
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) Rn[i * 3 + j] = R0[i] * Rt[j] + R0[3 + i] * Rt[3 + j] + R0[6 + i] * Rt[6 + j];
  so3_log(Rn, p);
}

// trans_out[t] by the flags
__device__ __forceinline__ void frame_trans(const RootFrameArgs& a, long t, long first, const float (&R0)[9], float* y) {
  const float* x = a.trans + t * 3;
  const bool rot = a.flags & ROOT_FRAME_ROTATE, sub = a.flags & ROOT_FRAME_SUBTRACT;
  if (sub && t == first) {
    y[0] = y[1] = y[2] = 0.f;
    return;
  }
  float f[3] = {0.f, 0.f, 0.f};
  if (rot) mat_t_vec(R0, x, y); else { y[0] = x[0]; y[1] = x[1]; y[2] = x[2]; }
  if (sub) {
    const float* x0 = a.trans + first * 3;
    if (rot) mat_t_vec(R0, x0, f); else { f[0] = x0[0]; f[1] = x0[1]; f[2] = x0[2]; }
  }
  y[0] -= f[0]; y[1] -= f[1]; y[2] -= f[2];
}

__global__ void __launch_bounds__(RF_THREADS) root_frame_fwd_kernel(RootFrameArgs a) {
  const long t = (long)blockIdx.x * RF_THREADS + threadIdx.x;
  if (t >= a.T) return;
  const long first = t / a.seg_len * a.seg_len;
  float R0[9], p[3];
  frame_fwd(a, t, first, R0, p);
  float* o = a.root_out + t * 3;
  o[0] = p[0]; o[1] = p[1]; o[2] = p[2];
  if (a.flags) {
    float y[3];
    frame_trans(a, t, first, R0, y);
    float* q = a.trans_out + t * 3;
    q[0] = y[0]; q[1] = y[1]; q[2] = y[2];
  }
}

// One wave per 64 consecutive frames of one segment: every frame's own rows, and the wave's nine sums to `part`.
__global__ void __launch_bounds__(RF_THREADS) root_frame_vjp_kernel(RootFrameArgs a) {
  const int lane = threadIdx.x & 63;
  const long wave = (long)blockIdx.x * (RF_THREADS / 64) + (threadIdx.x >> 6);
  const int wps = (a.seg_len + 63) / 64;
  const long seg = wave / wps;
  if (seg >= a.T / a.seg_len) return;   // the whole wave
  const int in_seg = (int)(wave % wps) * 64 + lane;
  const long first = seg * a.seg_len, t = first + in_seg;
  float v[RF_SUMS];
#pragma unroll
  for (int i = 0; i < RF_SUMS; ++i) v[i] = 0.f;
  if (in_seg < a.seg_len) {
    const float* r0 = a.root + first * a.ld_root;
    const float* rt = a.root + t * a.ld_root;
    const Quat q0 = quat_exp(r0);
    if (t != first) {
      double g[3] = {0.0, 0.0, 0.0};
      if (a.d_root_out) {
        const double d[3] = {a.d_root_out[t * 3], a.d_root_out[t * 3 + 1], a.d_root_out[t * 3 + 2]};
        const double r[3] = {rt[0], rt[1], rt[2]};
        double p[3], ul[3], ur[3];
        quat_rel_log(q0, quat_exp(rt), p);
        so3_jinv(p, d, ul, ur);
        so3_jl(r, ul, g);
        v[0] = (float)-ur[0]; v[1] = (float)-ur[1]; v[2] = (float)-ur[2];
      }
      float* o = a.g_root + t * 3;
      o[0] = (float)g[0]; o[1] = (float)g[1]; o[2] = (float)g[2];
    }
    const bool rot = a.flags & ROOT_FRAME_ROTATE, sub = a.flags & ROOT_FRAME_SUBTRACT;
    if (a.d_trans_out && !(sub && t == first)) {
      const double d[3] = {a.d_trans_out[t * 3], a.d_trans_out[t * 3 + 1], a.d_trans_out[t * 3 + 2]};
      double gt[3] = {d[0], d[1], d[2]};
      if (rot) {
        double x[3] = {a.trans[t * 3], a.trans[t * 3 + 1], a.trans[t * 3 + 2]}, y[3], c[3];
        if (sub) { x[0] -= a.trans[first * 3]; x[1] -= a.trans[first * 3 + 1]; x[2] -= a.trans[first * 3 + 2]; }
        quat_rot(q0, -1.0, x, y);   // trans_out[t]
        cross3d(d, y, c);
        v[3] = (float)c[0]; v[4] = (float)c[1]; v[5] = (float)c[2];
        quat_rot(q0, 1.0, d, gt);
      }
      if (sub) { v[6] = (float)gt[0]; v[7] = (float)gt[1]; v[8] = (float)gt[2]; }
      float* o = a.g_trans + t * 3;
      o[0] = (float)gt[0]; o[1] = (float)gt[1]; o[2] = (float)gt[2];
    }
  }
  int base = 0, count = 0;
  LaneReduceScatter<RF_SUMS, 32, RF_SUMS>::run(v, lane, base, count);   // nine is odd: every lane ends with all nine sums
  if (lane == 0) {
    float* o = a.part + wave * RF_SUMS;
#pragma unroll
    for (int i = 0; i < RF_SUMS; ++i) o[i] = v[i];
  }
}

// One wave per segment: the partials of its waves in ascending order, then the first frame's rows.
__global__ void __launch_bounds__(RF_THREADS) root_frame_vjp_first_kernel(RootFrameArgs a) {
  const int lane = threadIdx.x & 63;
  const long seg = (long)blockIdx.x * (RF_THREADS / 64) + (threadIdx.x >> 6);
  if (seg >= a.T / a.seg_len) return;   // the whole wave
  const int wps = (a.seg_len + 63) / 64, run = (wps + 63) / 64;
  const float* part = a.part + seg * wps * RF_SUMS;
  float v[RF_SUMS];
#pragma unroll
  for (int i = 0; i < RF_SUMS; ++i) v[i] = 0.f;
  for (int w = lane * run; w < wps && w < (lane + 1) * run; ++w)
#pragma unroll
    for (int i = 0; i < RF_SUMS; ++i) v[i] += part[(long)w * RF_SUMS + i];
  int base = 0, count = 0;
  LaneReduceScatter<RF_SUMS, 32, RF_SUMS>::run(v, lane, base, count);
  if (lane != 0) return;
  const long first = seg * a.seg_len;
  const float* r0 = a.root + first * a.ld_root;
  const double r[3] = {r0[0], r0[1], r0[2]};
  const double s[3] = {(double)v[0] + v[3], (double)v[1] + v[4], (double)v[2] + v[5]};
  double g[3];
  so3_jl(r, s, g);
  float* o = a.g_root + first * 3;
  o[0] = (float)g[0]; o[1] = (float)g[1]; o[2] = (float)g[2];
  if (a.d_trans_out && (a.flags & ROOT_FRAME_SUBTRACT)) {
    float* q = a.g_trans + first * 3;
    q[0] = -v[6]; q[1] = -v[7]; q[2] = -v[8];
  }
}

}  // namespace

hipError_t launch_root_frame_fwd(const RootFrameArgs& a, hipStream_t stream) {
  const unsigned grid = (unsigned)(((long)a.T + RF_THREADS - 1) / RF_THREADS);
  hipLaunchKernelGGL(root_frame_fwd_kernel, dim3(grid), dim3(RF_THREADS), 0, stream, a);
  return hipGetLastError();
}

long root_frame_vjp_waves(int T, int seg_len) { return (long)(T / seg_len) * ((seg_len + 63) / 64); }

hipError_t launch_root_frame_vjp(const RootFrameArgs& a, hipStream_t stream) {
  constexpr int WPB = RF_THREADS / 64;
  const long waves = root_frame_vjp_waves(a.T, a.seg_len), segs = a.T / a.seg_len;
  hipLaunchKernelGGL(root_frame_vjp_kernel, dim3((unsigned)((waves + WPB - 1) / WPB)), dim3(RF_THREADS), 0, stream, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(root_frame_vjp_first_kernel, dim3((unsigned)((segs + WPB - 1) / WPB)), dim3(RF_THREADS), 0, stream, a);
  return hipGetLastError();
}

}  // namespace empose
