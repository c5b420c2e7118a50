// Launch interfaces of the mesh rasteriser (raster.hip): projection, z-buffer rasterisation and shading of one slab of
// frames.  Internal, not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>

namespace empose {

constexpr int RASTER_MAX_IMAGE = 2048;      // EMPOSE_RENDER_MAX_IMAGE (include/empose_hip.h): H and W at most
constexpr int RASTER_COLOR_UNIFORM = 0;     // EMPOSE_RENDER_COLOR_*: colors [3]
constexpr int RASTER_COLOR_VERTEX = 1;      // colors [V][3]
constexpr int RASTER_COLOR_FRAME = 2;       // colors [T][V][3]
constexpr int RASTER_WAVE_PIXELS = 256;     // a face whose bounding box holds more pixel centres goes to its whole wave
constexpr unsigned long long RASTER_EMPTY = ~0ull;   // the key of a pixel no face covers

// One slab of T frames; every per-frame pointer starts at the slab's first frame.
struct RasterArgs {
  const float* vertices;   // [T][V][3]
  const int* faces;        // [n_faces][3]
  const float* normals;    // [T][V][3] un-normalised, or nullptr (flat shading)
  const float* colors;     // by color_mode
  const float* cam_R;      // [3][3] row-major, or [T][3][3] (camera_per_frame)
  const float* cam_t;      // [3] or [T][3]
  float* proj;             // [T][V][3] (x, y, Z): written by the projection, read by the other two
  unsigned long long* keys;   // [T][H * W]
  unsigned char* rgb;      // [T][H][W][3]
  int* face_id;            // [T][H][W] or nullptr
  float* depth;            // [T][H][W] or nullptr
  float fx, fy, cx, cy, near;
  float light[3], ambient, background[3];
  int T, V, n_faces, H, W, color_mode, camera_per_frame;
};

// Projects every vertex and sets every key to RASTER_EMPTY.
hipError_t launch_raster_project(const RasterArgs& a, hipStream_t stream);
// keys[t][pixel] = min over the covering faces of (bits of Z) << 32 | face id.
hipError_t launch_raster_faces(const RasterArgs& a, hipStream_t stream);
// rgb, face_id and depth from the keys.
hipError_t launch_raster_shade(const RasterArgs& a, hipStream_t stream);

}  // namespace empose
