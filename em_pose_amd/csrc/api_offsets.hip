// C ABI (include/empose_hip.h), per-subject sensor offsets from calibration recordings: the checks of the arguments and of
// the host copy of the group table, then the two launches of offset_stats.hip.
#include "api_internal.h"
#include "data_kernels.h"

#include <climits>
#include <cstddef>

using namespace empose;
using namespace empose::api;

static_assert(sizeof(empose_offset_group) == sizeof(OffsetGroup) &&
              offsetof(empose_offset_group, first_frame) == offsetof(OffsetGroup, first_frame) &&
              offsetof(empose_offset_group, n_frames) == offsetof(OffsetGroup, n_frames), "group table layout");

namespace {

// A group of k frames owns ceil(k / 256) chunks, a group of no frames none: at most ceil(T / 256) + G in all, since the
// groups do not overlap (every group but its last chunk is made of full chunks, and those hold at most T frames).
size_t chunk_bound(int T, int G) { return ((size_t)T + OFFSET_STATS_CHUNK - 1) / OFFSET_STATS_CHUNK + (size_t)G; }

// Everything the launches rely on for staying inside their buffers, on the host copy of the table; the number of chunks.
int groups_ok(int T, int G, const empose_offset_group* groups, int* n_chunks) {
  long at = 0, chunks = 0;
  for (int g = 0; g < G; ++g) {
    const empose_offset_group& q = groups[g];
    if (q.n_frames < 0) return fail(EMPOSE_EINVAL, "group %d: n_frames must not be negative (%d)", g, q.n_frames);
    if (q.first_frame < 0 || (long)q.first_frame + q.n_frames > T)
      return fail(EMPOSE_EINVAL, "group %d: frames [%d, %ld) outside [0, %d)", g, q.first_frame,
                  (long)q.first_frame + q.n_frames, T);
    if (q.first_frame < at)
      return fail(EMPOSE_EINVAL, "group %d: first_frame %d overlaps the groups before it, which end at frame %ld "
                  "(groups must ascend)", g, q.first_frame, at);
    at = (long)q.first_frame + q.n_frames;
    chunks += ((long)q.n_frames + OFFSET_STATS_CHUNK - 1) / OFFSET_STATS_CHUNK;   // long: n_frames may be near 2^31
  }
  *n_chunks = (int)chunks;
  return EMPOSE_OK;
}

}  // namespace

extern "C" {

size_t empose_offset_stats_workspace_bytes(int T, int G, int M) {
  if (T <= 0 || G <= 0 || M <= 0) return 0;
  return align_up(chunk_bound(T, G) * (size_t)M * OFFSET_STATS_SUMS * sizeof(double));
}

int empose_offset_stats(int T, int V, const float* vertices, int M, int max_deg, const int* center, const int* helper,
                        const int* deg, const int* faces, const float* p, const float* R, const float* masks, int G,
                        const empose_offset_group* groups_host, const empose_offset_group* groups_dev, float* means,
                        float* covs, float* r, float* r_trace, int* counts, float* local_f, float* q_f,
                        void* workspace, size_t workspace_bytes, empose_stream_t stream_) {
  if (!vertices || !center || !helper || !deg || !faces) return fail(EMPOSE_EINVAL, "null vertex or table pointer");
  if (!p || !R) return fail(EMPOSE_EINVAL, "null reading pointer (p, R)");
  if (!groups_host || !groups_dev) return fail(EMPOSE_EINVAL, "null group table (host and device copy are both needed)");
  if (!means || !covs || !r || !r_trace || !counts) return fail(EMPOSE_EINVAL, "null statistics output pointer");
  if (T <= 0 || V <= 0 || M <= 0 || max_deg <= 0 || G <= 0)
    return fail(EMPOSE_EINVAL, "T, V, M, max_deg and G must be positive");
  if ((double)T * M > (double)INT_MAX) return fail(EMPOSE_EINVAL, "T * M above 2^31 - 1: too large for one call");
  if ((double)G * M > (double)INT_MAX) return fail(EMPOSE_EINVAL, "G * M above 2^31 - 1: too large for one call");
  int n_chunks = 0;
  TRY(groups_ok(T, G, groups_host, &n_chunks));
  if (!workspace || workspace_bytes < empose_offset_stats_workspace_bytes(T, G, M))
    return fail(EMPOSE_EINVAL, "workspace too small (empose_offset_stats_workspace_bytes)");
  OffsetStatsArgs a;
  a.vertices = vertices; a.center = center; a.helper = helper; a.deg = deg; a.faces = faces;
  a.p = p; a.R = R; a.masks = masks;
  a.groups = reinterpret_cast<const OffsetGroup*>(groups_dev); a.G = G;
  a.sums = static_cast<double*>(workspace);
  a.local_f = local_f; a.q_f = q_f;
  a.means = means; a.covs = covs; a.r = r; a.r_trace = r_trace; a.counts = counts;
  a.T = T; a.V = V; a.M = M; a.max_deg = max_deg; a.n_chunks = n_chunks;
  HIP_CHECK(launch_offset_stats(a, static_cast<hipStream_t>(stream_)), "offset statistics kernels");
  return EMPOSE_OK;
}

}  // extern "C"
