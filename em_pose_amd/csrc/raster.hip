// Headless mesh rendering: a z-buffer rasteriser for the posed body meshes, gfx950 only.  Three
// launches per slab of frames, every product and sum rounded on its own (no contraction), so the raster and the shading
// kernel form a pixel's edge functions with the same bits, and tests/raster_ref.py restates them operation by operation.
//
// raster_project_kernel, one lane per (frame, vertex): p_c = R p + t (R row-major, the camera looks along +z),
//   x = fx X / Z + cx, y = fy Y / Z + cy (image y points down; the pixel of row i, column j has its centre at
//   (j + 0.5, i + 0.5)); (x, y, Z) go to `proj`.  The same launch sets every key of the slab to RASTER_EMPTY.
// raster_faces_kernel, one lane per (frame, face): a face with a vertex at Z <= near is dropped WHOLE (there is no
//   clipping: a body that reaches through the near plane loses those faces), so is a face whose bounding box holds no
//   pixel centre of the image or whose screen area is exactly 0; no back-face culling.  With the edge functions
//     w0 = (x2 - x1)(py - y1) - (y2 - y1)(px - x1),  w1, w2 cyclic,  each times the sign of the area,
//   a pixel centre is covered when all three are >= 0 (edges are inclusive) and ws = (w0 + w1) + w2 > 0; its depth is
//   perspective-correct, Z = ws / ((w0 / Z0 + w1 / Z1) + w2 / Z2) = 1 / sum_k lambda_k / Z_k with lambda_k = w_k / ws.
//   The z-buffer holds one 64-bit key per pixel, (bits of Z) << 32 | face id -- positive floats order as their bit
//   patterns -- and is updated with a 64-bit integer atomicMin: the nearest face wins and, on an exact tie of the depth,
//   the lower face id, whatever order the lanes arrive in.  No floating-point atomics.  A face whose bounding box holds
//   more than RASTER_WAVE_PIXELS pixel centres is not walked by its lane alone: the wave takes such faces one after the
//   other, 64 pixels at a time, with the same per-pixel function and hence the same keys.
// raster_shade_kernel, one lane per pixel: face id and depth from the key, the barycentrics recomputed as above, the
//   normal n = sum_k lambda_k n_k of the given vertex normals (un-normalised, as SMPLLayer.vertex_normals returns them) or
//   the face normal (p1 - p0) x (p2 - p0), rotated by R; intensity = ambient + (1 - ambient) |n . l| / |n| (two-sided; l a
//   unit direction in camera space; a normal of length 0 gets `ambient`); colour = intensity times the base colour (one
//   RGB, per vertex, or per frame and vertex; per-vertex colours are interpolated like the normals); the byte is
//   floor(255 c + 0.5) clamped to 0 .. 255.  Pixels no face covers: face id -1, depth +inf, the background colour.
//
// A face index outside [0, V) is clamped into the range by both kernels that read faces (the host driver refuses such a
// table when it is given a host copy, api_render.hip).  Every pixel depends on its own frame alone: a frame gives the same
// bits alone, inside a batch and on either side of a slab edge, and so does a second launch.
#include <hip/hip_runtime.h>

#include "raster_kernels.h"

namespace empose {

namespace {

constexpr int RS_THREADS = 256;

struct Tri { float x0, y0, z0, x1, y1, z1, x2, y2, z2; };

__device__ __forceinline__ int clamp_index(int v, int V) { return v < 0 ? 0 : (v >= V ? V - 1 : v); }

__device__ __forceinline__ void face_of(const RasterArgs& a, int f, int& i0, int& i1, int& i2) {
  const int* fp = a.faces + (size_t)f * 3;
  i0 = clamp_index(fp[0], a.V); i1 = clamp_index(fp[1], a.V); i2 = clamp_index(fp[2], a.V);
}

__device__ __forceinline__ Tri tri_of(const float* proj, int i0, int i1, int i2) {
  const float* p0 = proj + (size_t)i0 * 3; const float* p1 = proj + (size_t)i1 * 3; const float* p2 = proj + (size_t)i2 * 3;
  Tri t;
  t.x0 = p0[0]; t.y0 = p0[1]; t.z0 = p0[2];
  t.x1 = p1[0]; t.y1 = p1[1]; t.z1 = p1[2];
  t.x2 = p2[0]; t.y2 = p2[1]; t.z2 = p2[2];
  return t;
}

__device__ __forceinline__ float tri_area(const Tri& t) {
#pragma clang fp contract(off)
  return (t.x1 - t.x0) * (t.y2 - t.y0) - (t.y1 - t.y0) * (t.x2 - t.x0);
}

// The oriented edge functions of the centre of pixel (row i, column j), their sum and the depth there; false where the
// centre is not covered.  The raster and the shading kernel both go through here.
__device__ __forceinline__ bool pixel_of(const Tri& t, float area, int i, int j, float w[3], float& ws, float& Z) {
#pragma clang fp contract(off)
  const float px = (float)j + 0.5f, py = (float)i + 0.5f;
  float w0 = (t.x2 - t.x1) * (py - t.y1) - (t.y2 - t.y1) * (px - t.x1);
  float w1 = (t.x0 - t.x2) * (py - t.y2) - (t.y0 - t.y2) * (px - t.x2);
  float w2 = (t.x1 - t.x0) * (py - t.y0) - (t.y1 - t.y0) * (px - t.x0);
  if (area < 0.f) { w0 = -w0; w1 = -w1; w2 = -w2; }
  if (!(w0 >= 0.f && w1 >= 0.f && w2 >= 0.f)) return false;
  ws = (w0 + w1) + w2;
  if (!(ws > 0.f)) return false;
  Z = ws / ((w0 / t.z0 + w1 / t.z1) + w2 / t.z2);
  w[0] = w0; w[1] = w1; w[2] = w2;
  return true;
}

// The rows and columns whose pixel centres lie inside the face's bounding box and the image; false for none.
__device__ __forceinline__ bool box_of(const Tri& t, int H, int W, int& i0, int& i1, int& j0, int& j1) {
#pragma clang fp contract(off)
  const float xmin = fminf(fminf(t.x0, t.x1), t.x2), xmax = fmaxf(fmaxf(t.x0, t.x1), t.x2);
  const float ymin = fminf(fminf(t.y0, t.y1), t.y2), ymax = fmaxf(fmaxf(t.y0, t.y1), t.y2);
  // clamped as floats: a projected coordinate may be far outside what an int holds
  const float jl = fmaxf(ceilf(xmin - 0.5f), 0.f), jh = fminf(floorf(xmax - 0.5f), (float)(W - 1));
  const float il = fmaxf(ceilf(ymin - 0.5f), 0.f), ih = fminf(floorf(ymax - 0.5f), (float)(H - 1));
  if (!(jl <= jh && il <= ih)) return false;
  j0 = (int)jl; j1 = (int)jh; i0 = (int)il; i1 = (int)ih;
  return true;
}

__device__ __forceinline__ void put_key(unsigned long long* keys, const Tri& t, float area, int i, int j, int W, int f) {
  float w[3], ws, Z;
  if (!pixel_of(t, area, i, j, w, ws, Z)) return;
  const unsigned long long key = ((unsigned long long)__float_as_uint(Z) << 32) | (unsigned)f;
  unsigned long long* at = keys + (size_t)i * W + j;
  // keys only fall: a key that is not below what the pixel holds now cannot win later either
  if (key < *at) atomicMin(at, key);
}

__global__ void __launch_bounds__(RS_THREADS) raster_project_kernel(RasterArgs a) {
#pragma clang fp contract(off)
  const long idx = (long)blockIdx.x * RS_THREADS + threadIdx.x;
  if (idx < (long)a.T * a.H * a.W) a.keys[idx] = RASTER_EMPTY;
  if (idx >= (long)a.T * a.V) return;
  const int t = (int)(idx / a.V);
  const float* R = a.cam_R + (a.camera_per_frame ? (size_t)t * 9 : 0);
  const float* c = a.cam_t + (a.camera_per_frame ? (size_t)t * 3 : 0);
  const float* p = a.vertices + (size_t)idx * 3;
  const float X = ((R[0] * p[0] + R[1] * p[1]) + R[2] * p[2]) + c[0];
  const float Y = ((R[3] * p[0] + R[4] * p[1]) + R[5] * p[2]) + c[1];
  const float Z = ((R[6] * p[0] + R[7] * p[1]) + R[8] * p[2]) + c[2];
  float* o = a.proj + (size_t)idx * 3;
  o[0] = (a.fx * X) / Z + a.cx;
  o[1] = (a.fy * Y) / Z + a.cy;
  o[2] = Z;
}

__global__ void __launch_bounds__(RS_THREADS) raster_faces_kernel(RasterArgs a) {
  const long idx = (long)blockIdx.x * RS_THREADS + threadIdx.x;
  const int HW = a.H * a.W;
  Tri tri = {};
  float area = 0.f;
  int t = 0, f = 0, i0 = 0, i1 = -1, j0 = 0, j1 = -1;
  bool have = false;
  if (idx < (long)a.T * a.n_faces) {
    t = (int)(idx / a.n_faces); f = (int)(idx - (long)t * a.n_faces);
    int v0, v1, v2;
    face_of(a, f, v0, v1, v2);
    tri = tri_of(a.proj + (size_t)t * a.V * 3, v0, v1, v2);
    area = tri_area(tri);
    have = tri.z0 > a.near && tri.z1 > a.near && tri.z2 > a.near && area != 0.f && box_of(tri, a.H, a.W, i0, i1, j0, j1);
  }
  const int bw = have ? j1 - j0 + 1 : 0, bh = have ? i1 - i0 + 1 : 0;   // at most RASTER_MAX_IMAGE each
  const int npix = bw * bh;
  const bool big = npix > RASTER_WAVE_PIXELS;
  if (have && !big) {
    unsigned long long* keys = a.keys + (size_t)t * HW;
    for (int i = i0; i <= i1; ++i)
      for (int j = j0; j <= j1; ++j) put_key(keys, tri, area, i, j, a.W, f);
  }
  // the large faces of the wave, lowest lane first, 64 pixels at a time (no lane has left: all reach the ballot)
  const int lane = threadIdx.x & 63;
  unsigned long long todo = __ballot(big);
  while (todo) {
    const int src = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    Tri s;
    s.x0 = __shfl(tri.x0, src); s.y0 = __shfl(tri.y0, src); s.z0 = __shfl(tri.z0, src);
    s.x1 = __shfl(tri.x1, src); s.y1 = __shfl(tri.y1, src); s.z1 = __shfl(tri.z1, src);
    s.x2 = __shfl(tri.x2, src); s.y2 = __shfl(tri.y2, src); s.z2 = __shfl(tri.z2, src);
    const float s_area = __shfl(area, src);
    const int s_t = __shfl(t, src), s_f = __shfl(f, src), s_i0 = __shfl(i0, src), s_j0 = __shfl(j0, src);
    const int s_bw = __shfl(bw, src), s_npix = __shfl(npix, src);
    unsigned long long* keys = a.keys + (size_t)s_t * HW;
    for (int p = lane; p < s_npix; p += 64) {
      const int r = p / s_bw;
      put_key(keys, s, s_area, s_i0 + r, s_j0 + (p - r * s_bw), a.W, s_f);
    }
  }
}

__device__ __forceinline__ unsigned char to_byte(float c) {
#pragma clang fp contract(off)
  const float v = fminf(fmaxf(255.f * c + 0.5f, 0.f), 255.f);
  return (unsigned char)floorf(v);
}

__global__ void __launch_bounds__(RS_THREADS) raster_shade_kernel(RasterArgs a) {
#pragma clang fp contract(off)
  const long idx = (long)blockIdx.x * RS_THREADS + threadIdx.x;
  const int HW = a.H * a.W;
  if (idx >= (long)a.T * HW) return;
  const int t = (int)(idx / HW), pix = (int)(idx - (long)t * HW);
  const int i = pix / a.W, j = pix - i * a.W;
  unsigned char* rgb = a.rgb + (size_t)idx * 3;
  const unsigned long long key = a.keys[idx];
  int v0, v1, v2;
  Tri tri;
  float w[3], ws = 0.f, Z = 0.f;
  bool hit = key != RASTER_EMPTY;
  const int f = (int)(unsigned)(key & 0xffffffffull);
  if (hit) {
    face_of(a, f, v0, v1, v2);
    tri = tri_of(a.proj + (size_t)t * a.V * 3, v0, v1, v2);
    hit = pixel_of(tri, tri_area(tri), i, j, w, ws, Z);   // (always covered: the raster kernel found it so with these bits)
  }
  if (!hit) {
    for (int c = 0; c < 3; ++c) rgb[c] = to_byte(a.background[c]);
    if (a.face_id) a.face_id[idx] = -1;
    if (a.depth) a.depth[idx] = __uint_as_float(0x7f800000u);
    return;
  }
  if (a.face_id) a.face_id[idx] = f;
  if (a.depth) a.depth[idx] = __uint_as_float((unsigned)(key >> 32));
  const float l0 = w[0] / ws, l1 = w[1] / ws, l2 = w[2] / ws;
  const size_t vt = (size_t)t * a.V * 3;
  float n[3];
  if (a.normals) {
    const float* n0 = a.normals + vt + (size_t)v0 * 3; const float* n1 = a.normals + vt + (size_t)v1 * 3;
    const float* n2 = a.normals + vt + (size_t)v2 * 3;
    for (int c = 0; c < 3; ++c) n[c] = (l0 * n0[c] + l1 * n1[c]) + l2 * n2[c];
  } else {
    const float* p0 = a.vertices + vt + (size_t)v0 * 3; const float* p1 = a.vertices + vt + (size_t)v1 * 3;
    const float* p2 = a.vertices + vt + (size_t)v2 * 3;
    const float e1[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]};
    const float e2[3] = {p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]};
    n[0] = e1[1] * e2[2] - e1[2] * e2[1];
    n[1] = e1[2] * e2[0] - e1[0] * e2[2];
    n[2] = e1[0] * e2[1] - e1[1] * e2[0];
  }
  const float* R = a.cam_R + (a.camera_per_frame ? (size_t)t * 9 : 0);
  float nc[3];
  for (int r = 0; r < 3; ++r) nc[r] = (R[r * 3] * n[0] + R[r * 3 + 1] * n[1]) + R[r * 3 + 2] * n[2];
  const float len = sqrtf((nc[0] * nc[0] + nc[1] * nc[1]) + nc[2] * nc[2]);
  const float dot = (nc[0] * a.light[0] + nc[1] * a.light[1]) + nc[2] * a.light[2];
  const float intensity = len > 0.f ? a.ambient + (1.f - a.ambient) * (fabsf(dot) / len) : a.ambient;
  float base[3];
  if (a.color_mode == RASTER_COLOR_UNIFORM) {
    for (int c = 0; c < 3; ++c) base[c] = a.colors[c];
  } else {
    const float* col = a.colors + (a.color_mode == RASTER_COLOR_FRAME ? vt : 0);
    const float* c0 = col + (size_t)v0 * 3; const float* c1 = col + (size_t)v1 * 3; const float* c2 = col + (size_t)v2 * 3;
    for (int c = 0; c < 3; ++c) base[c] = (l0 * c0[c] + l1 * c1[c]) + l2 * c2[c];
  }
  for (int c = 0; c < 3; ++c) rgb[c] = to_byte(base[c] * intensity);
}

inline unsigned blocks_of(long lanes) { return (unsigned)((lanes + RS_THREADS - 1) / RS_THREADS); }

}  // namespace

hipError_t launch_raster_project(const RasterArgs& a, hipStream_t stream) {
  const long lanes = (long)a.T * (a.V > a.H * a.W ? a.V : a.H * a.W);
  hipLaunchKernelGGL(raster_project_kernel, dim3(blocks_of(lanes)), dim3(RS_THREADS), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_raster_faces(const RasterArgs& a, hipStream_t stream) {
  hipLaunchKernelGGL(raster_faces_kernel, dim3(blocks_of((long)a.T * a.n_faces)), dim3(RS_THREADS), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_raster_shade(const RasterArgs& a, hipStream_t stream) {
  hipLaunchKernelGGL(raster_shade_kernel, dim3(blocks_of((long)a.T * a.H * a.W)), dim3(RS_THREADS), 0, stream, a);
  return hipGetLastError();
}

}  // namespace empose
