// C ABI (include/empose_hip.h), temporal metrics: the checks of the arguments, then the launch of temporal.hip.
#include "api_internal.h"
#include "data_kernels.h"

#include <climits>
#include <cmath>

using namespace empose;
using namespace empose::api;

static_assert(TEMPORAL_SEGMENT == EMPOSE_TEMPORAL_SEGMENT, "the header's segment length is the kernel's");

extern "C" {

int empose_temporal_rows(int N, int F, int P, const float* x_gt, const float* x_hat, const unsigned char* valid, double fps,
                         int reduce, double* rows, unsigned char* defined, empose_stream_t stream_) {
  if (N <= 0) return fail(EMPOSE_EINVAL, "N must be positive (got %d)", N);
  if (F <= 0) return fail(EMPOSE_EINVAL, "F must be positive (got %d)", F);
  if (P <= 0) return fail(EMPOSE_EINVAL, "P must be positive (got %d)", P);
  if (!x_gt) return fail(EMPOSE_EINVAL, "null x_gt");
  if (!x_hat) return fail(EMPOSE_EINVAL, "null x_hat");
  if (!valid) return fail(EMPOSE_EINVAL, "null valid");
  if (!rows) return fail(EMPOSE_EINVAL, "null rows");
  if (!defined) return fail(EMPOSE_EINVAL, "null defined");
  if (!(fps > 0.0) || !std::isfinite(fps)) return fail(EMPOSE_EINVAL, "fps must be positive and finite (got %g)", fps);
  if (reduce != 0 && reduce != 1) return fail(EMPOSE_EINVAL, "reduce must be 0 or 1 (got %d)", reduce);
  if ((double)N * F > (double)INT_MAX) return fail(EMPOSE_EINVAL, "N * F above 2^31 - 1: too large for one call");
  if (temporal_rows_blocks(N, F, P, reduce) > (long)INT_MAX)
    return fail(EMPOSE_EINVAL, "N, F and P need more than 2^31 - 1 workgroups: too large for one call");
  TemporalArgs a = {};
  a.x_gt = x_gt; a.x_hat = x_hat; a.valid = valid; a.rows = rows; a.defined = defined;
  a.fps2 = fps * fps; a.fps3 = fps * fps * fps;
  a.N = N; a.F = F; a.P = P; a.reduce = reduce;
  HIP_CHECK(launch_temporal_rows(a, static_cast<hipStream_t>(stream_)), "temporal rows kernel");
  return EMPOSE_OK;
}

}  // extern "C"
