// Unit quaternions in double on the device: what resample.hip (SQUAD) and smooth.hip (rotation filters) share.  Inputs
// and outputs of those kernels are fp32 rotation vectors; rotation vector <-> quaternion <-> log in float32 costs more
// than the float32 rounding of inputs and outputs, so everything here is double.  The helpers take the floating-point
// contraction mode of the file that includes them (smooth.hip turns contraction off before the include).
#pragma once
#include <hip/hip_runtime.h>

namespace empose {

struct Quat { double w, x, y, z; };

__device__ __forceinline__ Quat q_mul(const Quat& a, const Quat& b) {
  return {a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z, a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y,
          a.w * b.y - a.x * b.z + a.y * b.w + a.z * b.x, a.w * b.z + a.x * b.y - a.y * b.x + a.z * b.w};
}
__device__ __forceinline__ Quat q_conj_mul(const Quat& a, const Quat& b) {   // a^-1 b
  return q_mul({a.w, -a.x, -a.y, -a.z}, b);
}
__device__ __forceinline__ double q_dot(const Quat& a, const Quat& b) { return a.w * b.w + a.x * b.x + a.y * b.y + a.z * b.z; }
// b in the hemisphere of a
__device__ __forceinline__ Quat q_toward(const Quat& a, const Quat& b) {
  return q_dot(a, b) < 0.0 ? Quat{-b.w, -b.x, -b.y, -b.z} : b;
}
__device__ __forceinline__ Quat q_from_rotvec(const float* r) {
  const double x = r[0], y = r[1], z = r[2], t2 = x * x + y * y + z * z, t = sqrt(t2);
  const double k = t2 < 1e-8 ? 0.5 - t2 * (1.0 / 48.0) : sin(0.5 * t) / t;
  return {cos(0.5 * t), k * x, k * y, k * z};
}
// log of a unit quaternion: the half-angle vector; a series factor below a small angle
__device__ __forceinline__ void q_log(const Quat& q, double* v) {
  const double s = sqrt(q.x * q.x + q.y * q.y + q.z * q.z);
  const double k = (s < 1e-8 && q.w > 0.0) ? 1.0 / q.w : (s > 0.0 ? atan2(s, q.w) / s : 0.0);
  v[0] = k * q.x; v[1] = k * q.y; v[2] = k * q.z;
}
__device__ __forceinline__ Quat q_exp(const double* v) {
  const double a2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2], a = sqrt(a2);
  const double k = a2 < 1e-16 ? 1.0 - a2 * (1.0 / 6.0) : sin(a) / a;
  return {cos(a), k * v[0], k * v[1], k * v[2]};
}
// a exp(t * l)
__device__ __forceinline__ Quat q_step(const Quat& a, const double* l, double t) {
  const double v[3] = {t * l[0], t * l[1], t * l[2]};
  return q_mul(a, q_exp(v));
}
// the rotation vector of q / |q| for |q| near 1, with w >= 0: |r| <= pi
__device__ __forceinline__ void q_to_rotvec(Quat q, float* o) {
  if (q.w < 0.0) q = {-q.w, -q.x, -q.y, -q.z};
  const double s = sqrt(q.x * q.x + q.y * q.y + q.z * q.z);
  const double k = s < 1e-8 ? 2.0 / q.w : 2.0 * atan2(s, q.w) / s;
  o[0] = (float)(k * q.x); o[1] = (float)(k * q.y); o[2] = (float)(k * q.z);
}

}  // namespace empose
