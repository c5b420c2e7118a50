// C ABI (include/empose_hip.h), sensor placement search: the checks of the arguments and of the host copy of the candidate
// list, then the launches of placement.hip.
#include "api_internal.h"
#include "data_kernels.h"

#include <climits>

using namespace empose;
using namespace empose::api;

namespace {

constexpr int MAX_GRID_ROWS = 65535;   // gridDim.y (chunks of frames) and gridDim.z (blocks of sensors)

size_t chunks_of(int T) { return ((size_t)T + PLACEMENT_CHUNK - 1) / PLACEMENT_CHUNK; }

// Everything the kernels rely on for staying inside the mesh, on the host copy of the list.
int candidates_ok(int V, int C, const int* cand) {
  for (int c = 0; c < C; ++c) {
    if (cand[c] < 0 || cand[c] >= V)
      return fail(EMPOSE_EINVAL, "candidate %d: vertex %d outside [0, %d)", c, cand[c], V);
    if (c > 0 && cand[c] <= cand[c - 1])
      return fail(EMPOSE_EINVAL, "candidate %d: vertex %d does not come after vertex %d before it (candidates must "
                  "ascend)", c, cand[c], cand[c - 1]);
  }
  return EMPOSE_OK;
}

}  // namespace

extern "C" {

size_t empose_placement_workspace_bytes(int T, int M, int C) {
  if (T <= 0 || M <= 0 || C <= 0) return 0;
  return align_up(chunks_of(T) * (size_t)M * (size_t)C * sizeof(double));
}

int empose_placement_accumulate(int T, int V, const float* vertices, int M, const float* p, const float* masks, int C,
                                const int* cand_host, const int* cand_dev, double* sums, int* counts, void* workspace,
                                size_t workspace_bytes, empose_stream_t stream_) {
  if (!vertices || !p) return fail(EMPOSE_EINVAL, "null vertex or reading pointer (vertices, p)");
  if (!sums || !counts) return fail(EMPOSE_EINVAL, "null running sums or counts");
  if (T <= 0 || V <= 0 || M <= 0 || C <= 0) return fail(EMPOSE_EINVAL, "T, V, M and C must be positive");
  if ((double)T * M > (double)INT_MAX) return fail(EMPOSE_EINVAL, "T * M above 2^31 - 1: too large for one call");
  if ((double)M * C > (double)INT_MAX) return fail(EMPOSE_EINVAL, "M * C above 2^31 - 1: too large for one call");
  if (chunks_of(T) > (size_t)MAX_GRID_ROWS)
    return fail(EMPOSE_EINVAL, "T above %d: split the frames into slabs", MAX_GRID_ROWS * PLACEMENT_CHUNK);
  if (M > MAX_GRID_ROWS * PLACEMENT_SENSORS) return fail(EMPOSE_EINVAL, "M above %d", MAX_GRID_ROWS * PLACEMENT_SENSORS);
  if ((cand_host == nullptr) != (cand_dev == nullptr))
    return fail(EMPOSE_EINVAL, "the candidate list needs its host and its device copy, or neither");
  if (!cand_host && C != V) return fail(EMPOSE_EINVAL, "without a candidate list C must equal V (%d, %d)", C, V);
  if (cand_host) TRY(candidates_ok(V, C, cand_host));
  if (!workspace || workspace_bytes < empose_placement_workspace_bytes(T, M, C))
    return fail(EMPOSE_EINVAL, "workspace too small (empose_placement_workspace_bytes)");
  PlacementArgs a = {};
  a.vertices = vertices; a.p = p; a.masks = masks; a.cand = cand_dev;
  a.part = static_cast<double*>(workspace); a.sums = sums; a.counts = counts;
  a.T = T; a.V = V; a.M = M; a.C = C;
  HIP_CHECK(launch_placement_accumulate(a, static_cast<hipStream_t>(stream_)), "placement accumulation kernels");
  return EMPOSE_OK;
}

int empose_placement_finish(int M, int C, const double* sums, const int* counts, const int* cand_dev, float* score,
                            int* best, float* best_score, empose_stream_t stream_) {
  if (!sums || !counts) return fail(EMPOSE_EINVAL, "null running sums or counts");
  if (!score || !best || !best_score) return fail(EMPOSE_EINVAL, "null output pointer (score, best, best_score)");
  if (M <= 0 || C <= 0) return fail(EMPOSE_EINVAL, "M and C must be positive");
  if ((double)M * C > (double)INT_MAX) return fail(EMPOSE_EINVAL, "M * C above 2^31 - 1: too large for one call");
  PlacementArgs a = {};
  a.sums = const_cast<double*>(sums); a.counts = const_cast<int*>(counts); a.cand = cand_dev;
  a.score = score; a.best = best; a.best_score = best_score;
  a.M = M; a.C = C;
  HIP_CHECK(launch_placement_finish(a, static_cast<hipStream_t>(stream_)), "placement finish kernel");
  return EMPOSE_OK;
}

}  // extern "C"
