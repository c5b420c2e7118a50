// C ABI (include/empose_hip.h), point-to-mesh queries: the checks of the descriptor and of the host copy of the face
// table, then the launch of surface_query.hip.
#include "api_internal.h"
#include "surface_kernels.h"

using namespace empose;
using namespace empose::api;

static_assert(EMPOSE_SURFACE_MAX_FRAMES == SURFACE_MAX_T && EMPOSE_SURFACE_MAX_VERTICES == SURFACE_MAX_V &&
              EMPOSE_SURFACE_MAX_FACES == SURFACE_MAX_F && EMPOSE_SURFACE_MAX_QUERIES == SURFACE_MAX_Q, "surface query caps");

extern "C" {

// A frame's partial results are combined inside its workgroup: the query needs no scratch memory for any shape.
size_t empose_surface_query_workspace_bytes(int T, int V, int F, int Q) {
  (void)T; (void)V; (void)F; (void)Q;
  return 0;
}

int empose_surface_query(const empose_surface_desc* d, void* workspace, size_t workspace_bytes, empose_stream_t stream_) {
  (void)workspace;
  if (!d) return fail(EMPOSE_EINVAL, "null surface descriptor");
  if (d->T <= 0 || d->V <= 0 || d->F <= 0 || d->Q <= 0) return fail(EMPOSE_EINVAL, "T, V, F and Q must be positive");
  if (d->T > SURFACE_MAX_T)
    return fail(EMPOSE_EINVAL, "T = %d above the cap of %d: split the frames into slabs", d->T, SURFACE_MAX_T);
  if (d->V > SURFACE_MAX_V) return fail(EMPOSE_EINVAL, "V = %d above the cap of %d", d->V, SURFACE_MAX_V);
  if (d->F > SURFACE_MAX_F) return fail(EMPOSE_EINVAL, "F = %d above the cap of %d", d->F, SURFACE_MAX_F);
  if (d->Q > SURFACE_MAX_Q) return fail(EMPOSE_EINVAL, "Q = %d above the cap of %d", d->Q, SURFACE_MAX_Q);
  if (!d->vertices || !d->points) return fail(EMPOSE_EINVAL, "null vertices or points");
  if (!d->faces_host || !d->faces_dev)
    return fail(EMPOSE_EINVAL, "the face table needs its host and its device copy (faces_host, faces_dev)");
  if (!d->dist) return fail(EMPOSE_EINVAL, "null dist");
  if (d->want_inside && !d->inside) return fail(EMPOSE_EINVAL, "want_inside without an inside output");
  for (long k = 0; k < (long)d->F * 3; ++k)
    if (d->faces_host[k] < 0 || d->faces_host[k] >= d->V)
      return fail(EMPOSE_EINVAL, "face %ld: vertex index %d outside [0, V = %d)", k / 3, d->faces_host[k], d->V);
  if (workspace_bytes < empose_surface_query_workspace_bytes(d->T, d->V, d->F, d->Q))
    return fail(EMPOSE_EINVAL, "workspace too small (empose_surface_query_workspace_bytes)");
  SurfaceArgs a = {};
  a.vertices = d->vertices; a.faces = d->faces_dev; a.points = d->points; a.mask = d->mask;
  a.dist = d->dist; a.face = d->face; a.bary = d->bary; a.closest = d->closest; a.inside = d->inside;
  a.T = d->T; a.V = d->V; a.F = d->F; a.Q = d->Q; a.want_inside = d->want_inside ? 1 : 0;
  HIP_CHECK(launch_surface_query(a, static_cast<hipStream_t>(stream_)), "surface query kernel");
  return EMPOSE_OK;
}

}  // extern "C"
