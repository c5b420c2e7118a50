// C ABI (include/empose_hip.h), overlay primitives: the checks of the descriptor, then the two launches of overlay.hip slab
// by slab.
#include "api_internal.h"
#include "overlay_kernels.h"
#include "raster_kernels.h"

#include <cmath>

using namespace empose;
using namespace empose::api;

static_assert(EMPOSE_OVERLAY_MAX_PRIMS == OVERLAY_MAX_PRIMS, "overlay primitive cap");

namespace {

constexpr size_t OVERLAY_SLAB_BYTES = (size_t)16 << 20;   // camera-space primitives + boxes of one slab
constexpr int OVERLAY_SLAB_MAX = 4096;                    // frames (the pixel kernel's grid has a frame per y)

bool sizes_ok(int T, int P, int H, int W) {
  return T > 0 && P > 0 && H > 0 && W > 0 && P <= OVERLAY_MAX_PRIMS && H <= RASTER_MAX_IMAGE && W <= RASTER_MAX_IMAGE;
}

// Frames per slab: what fits OVERLAY_SLAB_BYTES, at least one.  The sizes are positive and P within the cap.
int overlay_slab(int T, int P) {
  const size_t per_frame = (size_t)P * (OVERLAY_PRIM_FLOATS * sizeof(float) + OVERLAY_BOX_INTS * sizeof(int));
  size_t s = OVERLAY_SLAB_BYTES / per_frame;
  if (s > (size_t)OVERLAY_SLAB_MAX) s = OVERLAY_SLAB_MAX;
  if (s < 1) s = 1;
  return (size_t)T < s ? T : (int)s;
}

struct OverlayWs { float* prims; int* boxes; };
OverlayWs carve_overlay(Carver& c, int S, int P) {
  OverlayWs w;
  w.prims = c.f((size_t)S * P * OVERLAY_PRIM_FLOATS);
  w.boxes = reinterpret_cast<int*>(c.f((size_t)S * P * OVERLAY_BOX_INTS));
  return w;
}

}  // namespace

extern "C" {

size_t empose_render_overlay_workspace_bytes(int T, int P, int H, int W) {
  if (!sizes_ok(T, P, H, W)) return 0;
  return Carver::measure([&](Carver& c) { carve_overlay(c, overlay_slab(T, P), P); });
}

int empose_render_overlay(const empose_overlay_desc* d, void* workspace, size_t workspace_bytes, empose_stream_t stream_) {
  if (!d) return fail(EMPOSE_EINVAL, "null overlay descriptor");
  if (d->T <= 0 || d->P <= 0 || d->H <= 0 || d->W <= 0) return fail(EMPOSE_EINVAL, "T, P, H and W must be positive");
  if (d->P > EMPOSE_OVERLAY_MAX_PRIMS)
    return fail(EMPOSE_EINVAL, "%d primitives above the cap of %d a frame", d->P, EMPOSE_OVERLAY_MAX_PRIMS);
  if (d->H > EMPOSE_RENDER_MAX_IMAGE || d->W > EMPOSE_RENDER_MAX_IMAGE)
    return fail(EMPOSE_EINVAL, "image %d x %d above the cap of %d x %d", d->H, d->W, EMPOSE_RENDER_MAX_IMAGE,
                EMPOSE_RENDER_MAX_IMAGE);
  if (d->slab_frames < 0) return fail(EMPOSE_EINVAL, "slab_frames must not be negative");
  if (!d->seg_a || !d->seg_b || !d->radius || !d->colors || !d->cam_R || !d->cam_t || !d->rgb)
    return fail(EMPOSE_EINVAL, "null seg_a, seg_b, radius, colors, cam_R, cam_t or rgb");
  if (!(d->near > 0.f) || !std::isfinite(d->near)) return fail(EMPOSE_EINVAL, "near must be positive and finite");
  if (!std::isfinite(d->fx) || !std::isfinite(d->fy) || !std::isfinite(d->cx) || !std::isfinite(d->cy) || d->fx == 0.f ||
      d->fy == 0.f)
    return fail(EMPOSE_EINVAL, "fx, fy, cx, cy must be finite and fx, fy non-zero");
  if (!(d->ambient >= 0.f && d->ambient <= 1.f)) return fail(EMPOSE_EINVAL, "ambient outside [0, 1]");
  if (!(d->hidden_alpha >= 0.f && d->hidden_alpha <= 1.f)) return fail(EMPOSE_EINVAL, "hidden_alpha outside [0, 1]");
  const double ll = std::sqrt((double)d->light[0] * d->light[0] + (double)d->light[1] * d->light[1] +
                              (double)d->light[2] * d->light[2]);
  if (!(ll > 0.0) || !std::isfinite(ll)) return fail(EMPOSE_EINVAL, "light must be a finite, non-zero direction");
  if (!workspace || workspace_bytes < empose_render_overlay_workspace_bytes(d->T, d->P, d->H, d->W))
    return fail(EMPOSE_EINVAL, "workspace too small (empose_render_overlay_workspace_bytes)");

  hipStream_t stream = static_cast<hipStream_t>(stream_);
  int S = overlay_slab(d->T, d->P);
  if (d->slab_frames > 0 && d->slab_frames < S) S = d->slab_frames;   // (a smaller slab fits the same workspace)
  Carver carver(workspace);
  const OverlayWs ws = carve_overlay(carver, S, d->P);
  OverlayArgs a = {};
  a.colors = d->colors; a.prims = ws.prims; a.boxes = ws.boxes;
  a.fx = d->fx; a.fy = d->fy; a.cx = d->cx; a.cy = d->cy; a.near = d->near;
  for (int c = 0; c < 3; ++c) a.light[c] = (float)(d->light[c] / ll);
  a.ambient = d->ambient; a.hidden_alpha = d->hidden_alpha;
  a.P = d->P; a.H = d->H; a.W = d->W;
  a.radius_per_frame = d->radius_per_frame ? 1 : 0; a.camera_per_frame = d->camera_per_frame ? 1 : 0;
  const size_t HW = (size_t)d->H * d->W;
  for (int t0 = 0; t0 < d->T; t0 += S) {
    const size_t p_off = (size_t)t0 * d->P;
    a.T = (d->T - t0) < S ? (d->T - t0) : S;
    a.seg_a = d->seg_a + p_off * 3;
    a.seg_b = d->seg_b + p_off * 3;
    a.radius = d->radius + (a.radius_per_frame ? p_off : 0);
    a.cam_R = d->cam_R + (a.camera_per_frame ? (size_t)t0 * 9 : 0);
    a.cam_t = d->cam_t + (a.camera_per_frame ? (size_t)t0 * 3 : 0);
    a.mesh_depth = d->mesh_depth ? d->mesh_depth + (size_t)t0 * HW : nullptr;
    a.rgb = d->rgb + (size_t)t0 * HW * 3;
    a.prim_id = d->prim_id ? d->prim_id + (size_t)t0 * HW : nullptr;
    a.prim_depth = d->prim_depth ? d->prim_depth + (size_t)t0 * HW : nullptr;
    HIP_CHECK(launch_overlay_setup(a, stream), "overlay setup kernel");
    HIP_CHECK(launch_overlay_pixels(a, stream), "overlay pixels kernel");
  }
  return EMPOSE_OK;
}

}  // extern "C"
