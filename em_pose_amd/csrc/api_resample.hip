// C ABI (include/empose_hip.h), resampling of ragged sequence batches to another frame rate: the checks of the host
// copy of the sequence table, then the launches of resample.hip.
#include "api_internal.h"
#include "data_kernels.h"

#include <cmath>
#include <cstddef>

using namespace empose;
using namespace empose::api;

static_assert(sizeof(empose_resample_seq) == sizeof(ResampleSeq) && offsetof(empose_resample_seq, fps_in) == offsetof(ResampleSeq, fps_in) &&
              offsetof(empose_resample_seq, out_row) == offsetof(ResampleSeq, out_row), "sequence table layout");

namespace {

// Everything a launch relies on for staying inside its buffers, on the host copy of the table.
int resample_args_ok(int S, const empose_resample_seq* seqs, const void* seqs_dev, int n, int floats_per, const void* in,
                     int ld_in, int in_rows, const void* out, int ld_out, int out_rows) {
  if (!seqs || !seqs_dev || !in || !out) return fail(EMPOSE_EINVAL, "null argument");
  if (S <= 0) return fail(EMPOSE_EINVAL, "S must be positive");
  if (n <= 0) return fail(EMPOSE_EINVAL, "the number of joints or channels must be positive");
  if (n > (1 << 20)) return fail(EMPOSE_EINVAL, "too many joints or channels");
  const int cols = n * floats_per;
  if (ld_in < cols || ld_out < cols) return fail(EMPOSE_EINVAL, "leading dimensions must be at least %d", cols);
  if (in_rows <= 0 || out_rows <= 0) return fail(EMPOSE_EINVAL, "in_rows and out_rows must be positive");
  long at = 0;
  for (int s = 0; s < S; ++s) {
    const empose_resample_seq& q = seqs[s];
    if (q.f_in < 2)
      return fail(EMPOSE_EINVAL, "sequence %d has %d frame(s): resampling needs at least two", s, q.f_in);
    if (q.f_out < 1) return fail(EMPOSE_EINVAL, "sequence %d: f_out must be positive", s);
    if (!(q.fps_in > 0.0) || !(q.fps_out > 0.0) || !std::isfinite(q.fps_in) || !std::isfinite(q.fps_out))
      return fail(EMPOSE_EINVAL, "sequence %d: rates must be positive and finite", s);
    if (q.in_row < 0 || (long)q.in_row + q.f_in > in_rows)
      return fail(EMPOSE_EINVAL, "sequence %d: input rows [%d, %ld) outside [0, %d)", s, q.in_row, (long)q.in_row + q.f_in, in_rows);
    if (q.out_row != at) return fail(EMPOSE_EINVAL, "sequence %d: output rows are not packed (out_row %d, expected %ld)", s, q.out_row, at);
    at += q.f_out;
    if (at > out_rows) break;
  }
  if (at != out_rows) return fail(EMPOSE_EINVAL, "the table's output rows do not sum to out_rows = %d", out_rows);
  return EMPOSE_OK;
}

ResampleArgs resample_args(int S, const empose_resample_seq* seqs_dev, int n, const float* in, int ld_in, float* out,
                           int ld_out, int out_rows) {
  ResampleArgs a = {};
  a.seqs = reinterpret_cast<const ResampleSeq*>(seqs_dev); a.S = S;
  a.in = in; a.ld_in = ld_in; a.out = out; a.ld_out = ld_out; a.n = n; a.out_rows = out_rows;
  return a;
}

}  // namespace

extern "C" {

int empose_resample_rotations(int S, const empose_resample_seq* seqs_host, const empose_resample_seq* seqs_dev, int J,
                              const float* in, int ld_in, int in_rows, float* out, int ld_out, int out_rows,
                              empose_stream_t stream_) {
  TRY(resample_args_ok(S, seqs_host, seqs_dev, J, 3, in, ld_in, in_rows, out, ld_out, out_rows));
  const ResampleArgs a = resample_args(S, seqs_dev, J, in, ld_in, out, ld_out, out_rows);
  HIP_CHECK(launch_resample_rotations(a, static_cast<hipStream_t>(stream_)), "resample rotations kernel");
  return EMPOSE_OK;
}

size_t empose_resample_positions_workspace_bytes(int in_rows, int C) {
  if (in_rows <= 0 || C <= 0) return 0;
  return align_up((size_t)in_rows * (size_t)C * sizeof(double));
}

int empose_resample_positions(int S, const empose_resample_seq* seqs_host, const empose_resample_seq* seqs_dev, int C,
                              const float* in, int ld_in, int in_rows, float* out, int ld_out, int out_rows,
                              void* workspace, size_t workspace_bytes, empose_stream_t stream_) {
  TRY(resample_args_ok(S, seqs_host, seqs_dev, C, 1, in, ld_in, in_rows, out, ld_out, out_rows));
  if (!workspace || workspace_bytes < empose_resample_positions_workspace_bytes(in_rows, C))
    return fail(EMPOSE_EINVAL, "workspace too small (empose_resample_positions_workspace_bytes)");
  ResampleArgs a = resample_args(S, seqs_dev, C, in, ld_in, out, ld_out, out_rows);
  a.ws = static_cast<double*>(workspace);
  HIP_CHECK(launch_resample_positions(a, static_cast<hipStream_t>(stream_)), "resample positions kernels");
  return EMPOSE_OK;
}

}  // extern "C"
