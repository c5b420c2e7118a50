// C ABI (include/empose_hip.h), sensor-noise augmentation: the checks of the arguments and of the host copy of the plan,
// then the one launch of sensor_noise.hip.
#include "api_internal.h"
#include "data_kernels.h"

using namespace empose;
using namespace empose::api;

static_assert(EMPOSE_SENSOR_NOISE_SPHERICAL == SENSOR_NOISE_SPHERICAL && EMPOSE_SENSOR_NOISE_SUPPRESS == SENSOR_NOISE_SUPPRESS,
              "sensor-noise modes");

extern "C" {

int empose_sensor_noise(int mode, int N, int F, int M, int K, int window_len, const int* start_host,
                        const int* sensor_host, const int* start_dev, const int* sensor_dev, const float* u_r,
                        const float* theta, const float* phi, float max_r, int thigh_a, int thigh_b, float mask_value,
                        const float* pos, const float* ori, const float* normal, float* pos_out, float* ori_out,
                        float* normal_out, empose_stream_t stream_) {
  // Everything the launch relies on for staying inside its buffers.
  if (mode != EMPOSE_SENSOR_NOISE_SPHERICAL && mode != EMPOSE_SENSOR_NOISE_SUPPRESS)
    return fail(EMPOSE_EINVAL, "unknown sensor-noise mode %d", mode);
  const bool suppress = mode == EMPOSE_SENSOR_NOISE_SUPPRESS;
  if (N <= 0 || F <= 0 || M <= 0) return fail(EMPOSE_EINVAL, "N, F and M must be positive");
  if (15.0 * N * F * M > 549755813888.0) return fail(EMPOSE_EINVAL, "more than 2^39 floats: too large for one launch");
  if (K < 1 || K > M) return fail(EMPOSE_EINVAL, "K = %d affected sensors outside [1, M = %d]", K, M);
  if (window_len < 0 || window_len > F) return fail(EMPOSE_EINVAL, "window_len = %d outside [0, F = %d]", window_len, F);
  if (!start_host || !sensor_host || !start_dev || !sensor_dev) return fail(EMPOSE_EINVAL, "null plan pointer");
  if (!pos || !pos_out) return fail(EMPOSE_EINVAL, "null position buffer");
  if (pos == pos_out) return fail(EMPOSE_EINVAL, "pos_out must not be pos");
  if (suppress) {
    if (!ori || !normal || !ori_out || !normal_out)
      return fail(EMPOSE_EINVAL, "suppression needs the orientation and normal buffers");
    if (ori == ori_out || normal == normal_out) return fail(EMPOSE_EINVAL, "an output buffer must not be its input");
  } else {
    if (thigh_a < 0 || thigh_a >= M || thigh_b < 0 || thigh_b >= M)
      return fail(EMPOSE_EINVAL, "thigh sensors %d, %d outside [0, M = %d)", thigh_a, thigh_b, M);
    if (window_len > 0 && (!u_r || !theta || !phi)) return fail(EMPOSE_EINVAL, "null draws (u_r, theta, phi)");
  }
  for (int i = 0; i < N; ++i)
    if (start_host[i] < 0 || start_host[i] > F - window_len)
      return fail(EMPOSE_EINVAL, "window %d: start %d outside [0, %d]", i, start_host[i], F - window_len);
  const long n_ids = suppress ? (long)N * K : K;
  for (long i = 0; i < n_ids; ++i)
    if (sensor_host[i] < 0 || sensor_host[i] >= M)
      return fail(EMPOSE_EINVAL, "plan entry %ld: sensor id %d outside [0, M = %d)", i, sensor_host[i], M);

  SensorNoiseArgs a = {};
  a.pos = pos; a.ori = ori; a.normal = normal;
  a.pos_out = pos_out; a.ori_out = ori_out; a.normal_out = normal_out;
  a.start = start_dev; a.sensor = sensor_dev;
  a.u_r = u_r; a.theta = theta; a.phi = phi;
  a.N = N; a.F = F; a.M = M; a.K = K; a.window_len = window_len; a.mode = mode;
  a.thigh_a = thigh_a; a.thigh_b = thigh_b; a.max_r = max_r; a.mask_value = mask_value;
  HIP_CHECK(launch_sensor_noise(a, static_cast<hipStream_t>(stream_)), "sensor noise kernel");
  return EMPOSE_OK;
}

}  // extern "C"
