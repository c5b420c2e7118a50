// Launch interface of the point-to-mesh query (surface_query.hip).  Internal, not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>

namespace empose {

constexpr int SURFACE_THREADS = 512;        // lanes of a workgroup: the stride of a lane's walk over the faces
constexpr int SURFACE_QUERY_BLOCK = 12;     // queries a workgroup carries through one pass over the faces
constexpr int SURFACE_LDS_MAX_V = 12288;    // a frame of at most this many vertices is staged in LDS (144 KB); above: L2
constexpr int SURFACE_MAX_T = 1 << 22;      // EMPOSE_SURFACE_MAX_FRAMES: gridDim.x, 2^31 lanes in that dimension
constexpr int SURFACE_MAX_V = 1 << 24;      // EMPOSE_SURFACE_MAX_VERTICES
constexpr int SURFACE_MAX_F = 1 << 26;      // EMPOSE_SURFACE_MAX_FACES
constexpr int SURFACE_MAX_Q = 4096;         // EMPOSE_SURFACE_MAX_QUERIES

struct SurfaceArgs {
  const float* vertices;   // [T][V][3]
  const int* faces;        // [F][3]
  const float* points;     // [T][Q][3]
  const float* mask;       // [T][Q] or nullptr
  float* dist;             // [T][Q]
  int* face;               // [T][Q] or nullptr
  float* bary;             // [T][Q][3] or nullptr
  float* closest;          // [T][Q][3] or nullptr
  unsigned char* inside;   // [T][Q] or nullptr
  int T, V, F, Q, want_inside;
};

// One workgroup per (frame, block of SURFACE_QUERY_BLOCK queries); writes every output of its queries.
hipError_t launch_surface_query(const SurfaceArgs& a, hipStream_t stream);

}  // namespace empose
