// The local frame of one virtual sensor of one posed mesh, as a device function: the arithmetic of
// virtual_sensors_kernel (virtual_sensors.hip) in its operation order, for kernels that go on computing with the frame instead of
// storing it (sensor_sample.hip).  Same operations in the same order; which products the compiler contracts with a
// following sum is decided per kernel, so the last bits may differ (tests/test_sample_sensors.py bounds it).
#pragma once
#include <hip/hip_runtime.h>

#include "smpl_math.h"

namespace empose {

// V: the frame's vertices [n_vertices][3]; faces: the sensor's `deg` incident faces [deg][3] (ids into V).
// n: the mean of the faces' (v1 - v0) x (v2 - v0), un-normalised; ori: row-major 3 x 3 with the columns tangent
// (unit((nh x s) x nh)), bitangent (unit(nh x s)) and normal (nh = n / |n|), s = unit(v_helper - v_center).
__device__ __forceinline__ void sensor_frame(const float* V, const int* faces, int deg, int center, int helper,
                                             float (&n)[3], float (&ori)[9]) {
  n[0] = 0.f; n[1] = 0.f; n[2] = 0.f;
  for (int k = 0; k < deg; ++k) {
    const float* v0 = V + (size_t)faces[k * 3 + 0] * 3;
    const float* v1 = V + (size_t)faces[k * 3 + 1] * 3;
    const float* v2 = V + (size_t)faces[k * 3 + 2] * 3;
    const float e1[3] = {v1[0] - v0[0], v1[1] - v0[1], v1[2] - v0[2]};
    const float e2[3] = {v2[0] - v0[0], v2[1] - v0[1], v2[2] - v0[2]};
    float fn[3];
    cross3(e1, e2, fn);
    n[0] += fn[0]; n[1] += fn[1]; n[2] += fn[2];
  }
  const float fdeg = (float)deg;
  n[0] /= fdeg; n[1] /= fdeg; n[2] /= fdeg;
  const float nn = norm3(n);
  const float nh[3] = {n[0] / nn, n[1] / nn, n[2] / nn};
  const float* vc = V + (size_t)center * 3;
  const float* vh = V + (size_t)helper * 3;
  const float e[3] = {vh[0] - vc[0], vh[1] - vc[1], vh[2] - vc[2]};
  const float ne = norm3(e);
  const float sv[3] = {e[0] / ne, e[1] / ne, e[2] / ne};
  float bb[3];
  cross3(nh, sv, bb);
  const float nb = norm3(bb);
  const float tv[3] = {bb[0] / nb, bb[1] / nb, bb[2] / nb};
  float aa[3];
  cross3(tv, nh, aa);
  const float na = norm3(aa);
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    ori[r * 3 + 0] = aa[r] / na;
    ori[r * 3 + 1] = tv[r];
    ori[r * 3 + 2] = nh[r];
  }
}

}  // namespace empose
