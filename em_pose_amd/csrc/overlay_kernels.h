// Launch interfaces of the overlay ray caster (overlay.hip): capsules and spheres drawn into rendered frames, one slab of
// frames at a time.  Internal, not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>

namespace empose {

constexpr int OVERLAY_MAX_PRIMS = 4096;    // EMPOSE_OVERLAY_MAX_PRIMS (include/empose_hip.h): primitives per frame at most
constexpr int OVERLAY_TILE = 16;           // a workgroup of the pixel kernel owns 16 x 16 pixels
constexpr int OVERLAY_PRIM_FLOATS = 8;     // camera-space a (3), b (3), radius (0: skipped), 1.0 for a sphere (a == b) else 0.0
constexpr int OVERLAY_BOX_INTS = 4;        // first row, last row, first column, last column; last < first: empty

// One slab of T frames; every per-frame pointer starts at the slab's first frame.
struct OverlayArgs {
  const float* seg_a;      // [T][P][3] world space
  const float* seg_b;      // [T][P][3]
  const float* radius;     // [P], or [T][P] (radius_per_frame)
  const float* colors;     // [P][3]
  const float* cam_R;      // [3][3] row-major, or [T][3][3] (camera_per_frame)
  const float* cam_t;      // [3] or [T][3]
  const float* mesh_depth; // [T][H][W] or nullptr (nothing hides)
  float* prims;            // [T][P][OVERLAY_PRIM_FLOATS]: written by the set-up, read by the pixel kernel
  int* boxes;              // [T][P][OVERLAY_BOX_INTS]
  unsigned char* rgb;      // [T][H][W][3], read and written
  int* prim_id;            // [T][H][W] or nullptr
  float* prim_depth;       // [T][H][W] or nullptr
  float fx, fy, cx, cy, near;
  float light[3], ambient, hidden_alpha;
  int T, P, H, W, radius_per_frame, camera_per_frame;
};

// Camera-space endpoints, skipped or not, and a conservative screen box of every (frame, primitive).
hipError_t launch_overlay_setup(const OverlayArgs& a, hipStream_t stream);
// The nearest primitive of every pixel, shaded into rgb; prim_id and prim_depth where asked for.
hipError_t launch_overlay_pixels(const OverlayArgs& a, hipStream_t stream);

}  // namespace empose
