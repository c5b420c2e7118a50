// C ABI (include/empose_hip.h), mesh rendering: the checks of the descriptor, then the three launches of raster.hip slab
// by slab.
#include "api_internal.h"
#include "raster_kernels.h"

#include <cmath>

using namespace empose;
using namespace empose::api;

static_assert(EMPOSE_RENDER_MAX_IMAGE == RASTER_MAX_IMAGE, "render image cap");
static_assert(EMPOSE_RENDER_COLOR_UNIFORM == RASTER_COLOR_UNIFORM && EMPOSE_RENDER_COLOR_VERTEX == RASTER_COLOR_VERTEX &&
              EMPOSE_RENDER_COLOR_FRAME == RASTER_COLOR_FRAME, "render colour modes");

namespace {

constexpr size_t RENDER_SLAB_BYTES = (size_t)64 << 20;   // projected vertices + keys of one slab, unless one frame needs more
constexpr int RENDER_SLAB_MAX = 4096;                    // frames

// Frames per slab: what fits RENDER_SLAB_BYTES, at least one.  The sizes are positive and H, W within the cap.
int render_slab(int T, int V, int H, int W) {
  const size_t per_frame = (size_t)V * 3 * sizeof(float) + (size_t)H * W * sizeof(unsigned long long);
  size_t s = RENDER_SLAB_BYTES / per_frame;
  if (s > (size_t)RENDER_SLAB_MAX) s = RENDER_SLAB_MAX;
  if (s < 1) s = 1;
  return (size_t)T < s ? T : (int)s;
}

struct RenderWs { float* proj; unsigned long long* keys; };
RenderWs carve_render(Carver& c, int S, int V, int H, int W) {
  RenderWs w;
  w.proj = c.f((size_t)S * V * 3);
  w.keys = reinterpret_cast<unsigned long long*>(c.f((size_t)S * H * W * 2));
  return w;
}

bool sizes_ok(int T, int V, int H, int W) {
  return T > 0 && V > 0 && H > 0 && W > 0 && H <= RASTER_MAX_IMAGE && W <= RASTER_MAX_IMAGE && V <= (1 << 24);
}

}  // namespace

extern "C" {

size_t empose_render_workspace_bytes(int T, int V, int H, int W) {
  if (!sizes_ok(T, V, H, W)) return 0;
  return Carver::measure([&](Carver& c) { carve_render(c, render_slab(T, V, H, W), V, H, W); });
}

int empose_render_meshes(const empose_render_desc* d, void* workspace, size_t workspace_bytes, empose_stream_t stream_) {
  if (!d) return fail(EMPOSE_EINVAL, "null render descriptor");
  if (d->T <= 0 || d->V <= 0 || d->n_faces <= 0 || d->H <= 0 || d->W <= 0)
    return fail(EMPOSE_EINVAL, "T, V, n_faces, H and W must be positive");
  if (d->H > EMPOSE_RENDER_MAX_IMAGE || d->W > EMPOSE_RENDER_MAX_IMAGE)
    return fail(EMPOSE_EINVAL, "image %d x %d above the cap of %d x %d", d->H, d->W, EMPOSE_RENDER_MAX_IMAGE,
                EMPOSE_RENDER_MAX_IMAGE);
  if (d->V > (1 << 24)) return fail(EMPOSE_EINVAL, "V above 2^24");
  if (d->n_faces > (1 << 26)) return fail(EMPOSE_EINVAL, "n_faces above 2^26");
  if (d->slab_frames < 0) return fail(EMPOSE_EINVAL, "slab_frames must not be negative");
  if (!d->vertices || !d->faces || !d->colors || !d->cam_R || !d->cam_t || !d->rgb)
    return fail(EMPOSE_EINVAL, "null vertices, faces, colors, cam_R, cam_t or rgb");
  if (d->color_mode != EMPOSE_RENDER_COLOR_UNIFORM && d->color_mode != EMPOSE_RENDER_COLOR_VERTEX &&
      d->color_mode != EMPOSE_RENDER_COLOR_FRAME)
    return fail(EMPOSE_EINVAL, "unknown color_mode %d", d->color_mode);
  if (!(d->near > 0.f) || !std::isfinite(d->near)) return fail(EMPOSE_EINVAL, "near must be positive and finite");
  if (!std::isfinite(d->fx) || !std::isfinite(d->fy) || !std::isfinite(d->cx) || !std::isfinite(d->cy) || d->fx == 0.f ||
      d->fy == 0.f)
    return fail(EMPOSE_EINVAL, "fx, fy, cx, cy must be finite and fx, fy non-zero");
  if (!(d->ambient >= 0.f && d->ambient <= 1.f)) return fail(EMPOSE_EINVAL, "ambient outside [0, 1]");
  const double ll = std::sqrt((double)d->light[0] * d->light[0] + (double)d->light[1] * d->light[1] +
                              (double)d->light[2] * d->light[2]);
  if (!(ll > 0.0) || !std::isfinite(ll)) return fail(EMPOSE_EINVAL, "light must be a finite, non-zero direction");
  for (int c = 0; c < 3; ++c)
    if (!std::isfinite(d->background[c])) return fail(EMPOSE_EINVAL, "background must be finite");
  if (d->faces_host)
    for (long k = 0; k < (long)d->n_faces * 3; ++k)
      if (d->faces_host[k] < 0 || d->faces_host[k] >= d->V)
        return fail(EMPOSE_EINVAL, "face %ld: vertex index %d outside [0, V = %d)", k / 3, d->faces_host[k], d->V);
  if (!workspace || workspace_bytes < empose_render_workspace_bytes(d->T, d->V, d->H, d->W))
    return fail(EMPOSE_EINVAL, "workspace too small (empose_render_workspace_bytes)");

  hipStream_t stream = static_cast<hipStream_t>(stream_);
  int S = render_slab(d->T, d->V, d->H, d->W);
  if (d->slab_frames > 0 && d->slab_frames < S) S = d->slab_frames;   // (a smaller slab fits the same workspace)
  Carver carver(workspace);
  const RenderWs ws = carve_render(carver, S, d->V, d->H, d->W);
  RasterArgs a = {};
  a.faces = d->faces; a.proj = ws.proj; a.keys = ws.keys;
  a.fx = d->fx; a.fy = d->fy; a.cx = d->cx; a.cy = d->cy; a.near = d->near;
  for (int c = 0; c < 3; ++c) { a.light[c] = (float)(d->light[c] / ll); a.background[c] = d->background[c]; }
  a.ambient = d->ambient;
  a.V = d->V; a.n_faces = d->n_faces; a.H = d->H; a.W = d->W;
  a.color_mode = d->color_mode; a.camera_per_frame = d->camera_per_frame ? 1 : 0;
  const size_t HW = (size_t)d->H * d->W;
  for (int t0 = 0; t0 < d->T; t0 += S) {
    const size_t v_off = (size_t)t0 * d->V * 3;
    a.T = (d->T - t0) < S ? (d->T - t0) : S;
    a.vertices = d->vertices + v_off;
    a.normals = d->normals ? d->normals + v_off : nullptr;
    a.colors = d->colors + (d->color_mode == EMPOSE_RENDER_COLOR_FRAME ? v_off : 0);
    a.cam_R = d->cam_R + (a.camera_per_frame ? (size_t)t0 * 9 : 0);
    a.cam_t = d->cam_t + (a.camera_per_frame ? (size_t)t0 * 3 : 0);
    a.rgb = d->rgb + (size_t)t0 * HW * 3;
    a.face_id = d->face_id ? d->face_id + (size_t)t0 * HW : nullptr;
    a.depth = d->depth ? d->depth + (size_t)t0 * HW : nullptr;
    HIP_CHECK(launch_raster_project(a, stream), "raster project kernel");
    HIP_CHECK(launch_raster_faces(a, stream), "raster faces kernel");
    HIP_CHECK(launch_raster_shade(a, stream), "raster shade kernel");
  }
  return EMPOSE_OK;
}

}  // extern "C"
