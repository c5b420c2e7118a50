// C ABI (include/empose_hip.h), smoothing of pose sequences: the checks of the arguments, then the launches of smooth.hip.
#include "api_internal.h"
#include "data_kernels.h"

#include <climits>
#include <cmath>

using namespace empose;
using namespace empose::api;

static_assert(SMOOTH_SEGMENT == EMPOSE_SMOOTH_SEGMENT, "the header's segment length is the kernel's");
static_assert(SMOOTH_MAX_RADIUS == EMPOSE_SMOOTH_MAX_RADIUS, "the header's largest radius is the kernel's");
static_assert(SMOOTH_STATE == EMPOSE_SMOOTH_STATE, "the header's state width is the kernel's");

namespace {

// What both filters check of the rows, and the arguments they share.
int smooth_rows_ok(int N, int F, int J, int C, const float* in, int ld_in, const float* out, int ld_out) {
  if (N <= 0) return fail(EMPOSE_EINVAL, "N must be positive (got %d)", N);
  if (F <= 0) return fail(EMPOSE_EINVAL, "F must be positive (got %d)", F);
  if (J < 0) return fail(EMPOSE_EINVAL, "J must not be negative (got %d)", J);
  if (C < 0) return fail(EMPOSE_EINVAL, "C must not be negative (got %d)", C);
  if (J == 0 && C == 0) return fail(EMPOSE_EINVAL, "J + C must be positive: nothing to filter");
  if (3L * J + C > (long)INT_MAX) return fail(EMPOSE_EINVAL, "3 J + C above 2^31 - 1");
  const int cols = 3 * J + C;
  if (ld_in < cols) return fail(EMPOSE_EINVAL, "ld_in must be at least 3 J + C = %d (got %d)", cols, ld_in);
  if (ld_out < cols) return fail(EMPOSE_EINVAL, "ld_out must be at least 3 J + C = %d (got %d)", cols, ld_out);
  if (!in) return fail(EMPOSE_EINVAL, "null in");
  if (!out) return fail(EMPOSE_EINVAL, "null out");
  if (out == in) return fail(EMPOSE_EINVAL, "out == in: the filters do not work in place");
  if ((double)N * F > (double)INT_MAX) return fail(EMPOSE_EINVAL, "N * F above 2^31 - 1: too large for one call");
  return EMPOSE_OK;
}

SmoothArgs smooth_args(int N, int F, int J, int C, const float* in, int ld_in, const unsigned char* valid, float* out,
                       int ld_out) {
  SmoothArgs a = {};
  a.in = in; a.out = out; a.valid = valid;
  a.N = N; a.F = F; a.J = J; a.C = C; a.ld_in = ld_in; a.ld_out = ld_out;
  return a;
}

bool positive_finite(double v) { return v > 0.0 && std::isfinite(v); }

}  // namespace

extern "C" {

int empose_smooth_window(int N, int F, int J, int C, const float* in, int ld_in, const unsigned char* valid, int R,
                         const double* taps_host, float* out, int ld_out, empose_stream_t stream_) {
  TRY(smooth_rows_ok(N, F, J, C, in, ld_in, out, ld_out));
  if (R < 0 || R > SMOOTH_MAX_RADIUS)
    return fail(EMPOSE_EINVAL, "R must be in [0, %d] (got %d)", SMOOTH_MAX_RADIUS, R);
  if (!taps_host) return fail(EMPOSE_EINVAL, "null taps_host");
  for (int k = 0; k <= R; ++k)
    if (!(taps_host[k] >= 0.0) || !std::isfinite(taps_host[k]))
      return fail(EMPOSE_EINVAL, "taps_host[%d] must be finite and not negative (got %g)", k, taps_host[k]);
  if (!(taps_host[0] > 0.0)) return fail(EMPOSE_EINVAL, "taps_host[0] must be positive (got %g)", taps_host[0]);
  if (smooth_window_blocks(N, F, J, C) > (long)INT_MAX)
    return fail(EMPOSE_EINVAL, "N, F, J and C need more than 2^31 - 1 workgroups: too large for one call");
  SmoothArgs a = smooth_args(N, F, J, C, in, ld_in, valid, out, ld_out);
  a.R = R;
  for (int k = 0; k <= R; ++k) a.taps[k] = taps_host[k];
  HIP_CHECK(launch_smooth_window(a, static_cast<hipStream_t>(stream_)), "smooth window kernel");
  return EMPOSE_OK;
}

int empose_smooth_one_euro(int N, int F, int J, int C, const float* in, int ld_in, const unsigned char* valid, double fps,
                           double min_cutoff, double beta, double d_cutoff, const double* state_in, double* state_out,
                           float* out, int ld_out, empose_stream_t stream_) {
  TRY(smooth_rows_ok(N, F, J, C, in, ld_in, out, ld_out));
  if (!positive_finite(fps)) return fail(EMPOSE_EINVAL, "fps must be positive and finite (got %g)", fps);
  if (!positive_finite(min_cutoff))
    return fail(EMPOSE_EINVAL, "min_cutoff must be positive and finite (got %g)", min_cutoff);
  if (!(beta >= 0.0) || !std::isfinite(beta)) return fail(EMPOSE_EINVAL, "beta must be finite and not negative (got %g)", beta);
  if (!positive_finite(d_cutoff)) return fail(EMPOSE_EINVAL, "d_cutoff must be positive and finite (got %g)", d_cutoff);
  if ((double)N * ((double)J + C) > (double)INT_MAX)
    return fail(EMPOSE_EINVAL, "N * (J + C) above 2^31 - 1: too large for one call");
  SmoothArgs a = smooth_args(N, F, J, C, in, ld_in, valid, out, ld_out);
  a.fps = fps; a.min_cutoff = min_cutoff; a.beta = beta; a.d_cutoff = d_cutoff;
  a.state_in = state_in; a.state_out = state_out;
  HIP_CHECK(launch_smooth_one_euro(a, static_cast<hipStream_t>(stream_)), "smooth one-euro kernel");
  return EMPOSE_OK;
}

}  // extern "C"
