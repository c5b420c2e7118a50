// Overlay ray caster: thin solid primitives (capsules, spheres) drawn into the frames of the mesh renderer and depth-tested
// against the mesh, gfx950 only (include/empose_hip.h states the definition).  Two launches per slab
// of frames, no atomics, every product and sum rounded on its own (no contraction), so tests/overlay_ref.py restates a
// pixel operation by operation.
//
// overlay_setup_kernel, one lane per (frame, primitive): a_c = R a + t, b_c = R b + t (R row-major, as raster.hip); the
//   primitive is skipped (radius 0 in the workspace, empty box) when its radius is not > 0 or a component of a, b or the
//   radius is not finite; a == b in all three components marks a sphere.  The screen box is CONSERVATIVE and never part of
//   the definition: a primitive with max Z + r < near / 2 cannot pass the near test and gets an empty box; one that reaches
//   min Z - r <= near gets the whole image; otherwise both end spheres lie in front of the plane Z = near, the silhouette
//   of the capsule is the convex hull of theirs, and the box is the union of the two spheres' extents.  The extent of a
//   sphere (X, Z, r) along x is exact under perspective -- the two tangents through the eye in the X-Z plane have the slopes
//     (X Z -+ r sqrt(X^2 + Z^2 - r^2)) / ((Z - r)(Z + r)),
//   which is tan(theta -+ alpha) with theta = atan2(X, Z), alpha = asin(r / sqrt(X^2 + Z^2)), without the trigonometry --
//   and is widened by a pixel and a thousandth of its distance from the principal point; likewise y.
// overlay_pixels_kernel, a workgroup of 256 lanes per (frame, 16 x 16 tile), lane = pixel.  The frame's primitives are taken
//   in chunks of 256: each lane tests one box against the tile, the survivors are compacted into LDS in ascending index
//   order (wave ballot + prefix count), and every lane walks the list for its pixel through capsule_hit, keeping the
//   nearest (s, index); a strict < keeps the lower index on an exact tie.  The epilogue shades the winner and writes.
//
// capsule_hit.  The ray of the pixel is s d with d = (dx, dy, 1): s is camera-space Z.  The quadratics are NOT formed with
//   the eye as origin (primitives are centimetres thick and metres away: that cancels catastrophically in float32) but
//   with the point of the ray at the depth of the segment's midpoint, o = Z_m d, Z_m = (a_z + b_z) / 2; u = s - Z_m:
//     sphere about c, m = o - c:   (d.d) u^2 + 2 (m.d) u + (m.m - r^2) = 0
//     side surface, e = b - a, m = o - a:   |d x e|^2 u^2 + 2 (m x e).(d x e) u + (|m x e|^2 - r^2 e.e) = 0
//   (the cross-product form of the distance to the axis: no difference of large products); the smaller root of each where
//   the discriminant is >= 0; the side root counts only with |d x e|^2 > 0 and the axial coordinate m.e + u d.e strictly
//   inside (0, e.e).  s = Z_m + the smallest root; s <= near: the primitive does not cover the pixel.
#include <hip/hip_runtime.h>

#include "overlay_kernels.h"

namespace empose {

namespace {

constexpr int OV_THREADS = 256;
constexpr int OV_WAVES = OV_THREADS / 64;

__device__ __forceinline__ float pos_inf() { return __uint_as_float(0x7f800000u); }

// The extent of a sphere's silhouette along one image axis, in pixel coordinates: centre coordinate X, depth Z, Z - r > 0.
__device__ __forceinline__ void sphere_extent(float X, float Z, float r, float f, float c, float& lo, float& hi) {
#pragma clang fp contract(off)
  const float den = (Z - r) * (Z + r);
  const float root = r * sqrtf(fmaxf(X * X + den, 0.f));
  const float x0 = f * ((X * Z - root) / den) + c, x1 = f * ((X * Z + root) / den) + c;
  const float margin = 1.f + 1e-3f * fmaxf(fabsf(x0 - c), fabsf(x1 - c));
  lo = fminf(lo, fminf(x0, x1) - margin);
  hi = fmaxf(hi, fmaxf(x0, x1) + margin);
}

// [lo, hi] in pixel coordinates to the first and last index whose centre may lie inside, within [0, n); anything that is
// not finite gives the whole range.
__device__ __forceinline__ void index_range(float lo, float hi, int n, int& first, int& last) {
  float f0 = fmaxf(floorf(lo - 0.5f), 0.f), f1 = fminf(ceilf(hi - 0.5f), (float)(n - 1));
  if (!__builtin_isfinite(lo) || !__builtin_isfinite(hi)) { f0 = 0.f; f1 = (float)(n - 1); }
  if (f0 > f1) { first = 0; last = -1; return; }
  first = (int)f0; last = (int)f1;
}

__global__ void __launch_bounds__(OV_THREADS) overlay_setup_kernel(OverlayArgs a) {
#pragma clang fp contract(off)
  const long idx = (long)blockIdx.x * OV_THREADS + threadIdx.x;
  if (idx >= (long)a.T * a.P) return;
  const int t = (int)(idx / a.P), p = (int)(idx - (long)t * a.P);
  const float* A = a.seg_a + (size_t)idx * 3;
  const float* B = a.seg_b + (size_t)idx * 3;
  const float r = a.radius[a.radius_per_frame ? (size_t)idx : (size_t)p];
  bool ok = r > 0.f && __builtin_isfinite(r);
  for (int c = 0; c < 3; ++c) ok = ok && __builtin_isfinite(A[c]) && __builtin_isfinite(B[c]);
  const float* R = a.cam_R + (a.camera_per_frame ? (size_t)t * 9 : 0);
  const float* ct = a.cam_t + (a.camera_per_frame ? (size_t)t * 3 : 0);
  float ac[3], bc[3];
  for (int k = 0; k < 3; ++k) {
    ac[k] = ((R[k * 3] * A[0] + R[k * 3 + 1] * A[1]) + R[k * 3 + 2] * A[2]) + ct[k];
    bc[k] = ((R[k * 3] * B[0] + R[k * 3 + 1] * B[1]) + R[k * 3 + 2] * B[2]) + ct[k];
  }
  const bool sphere = A[0] == B[0] && A[1] == B[1] && A[2] == B[2];
  float* o = a.prims + (size_t)idx * OVERLAY_PRIM_FLOATS;
  int* box = a.boxes + (size_t)idx * OVERLAY_BOX_INTS;
  for (int k = 0; k < 3; ++k) { o[k] = ok ? ac[k] : 0.f; o[3 + k] = ok ? bc[k] : 0.f; }
  o[6] = ok ? r : 0.f;
  o[7] = sphere ? 1.f : 0.f;
  int i0 = 0, i1 = -1, j0 = 0, j1 = -1;
  const float zmin = fminf(ac[2], bc[2]), zmax = fmaxf(ac[2], bc[2]);
  if (ok && !(zmax + r < 0.5f * a.near)) {
#ifdef EMPOSE_OVERLAY_FULL_BOXES   // (lab builds of scripts/dev/bench_overlay.py: what the binning buys)
    const bool whole = true;
#else
    const bool whole = !(zmin - r > a.near);
#endif
    if (whole) {
      i0 = 0; i1 = a.H - 1; j0 = 0; j1 = a.W - 1;
    } else {
      float xlo = pos_inf(), xhi = -pos_inf(), ylo = pos_inf(), yhi = -pos_inf();
      sphere_extent(ac[0], ac[2], r, a.fx, a.cx, xlo, xhi);
      sphere_extent(bc[0], bc[2], r, a.fx, a.cx, xlo, xhi);
      sphere_extent(ac[1], ac[2], r, a.fy, a.cy, ylo, yhi);
      sphere_extent(bc[1], bc[2], r, a.fy, a.cy, ylo, yhi);
      index_range(xlo, xhi, a.W, j0, j1);
      index_range(ylo, yhi, a.H, i0, i1);
      if (j1 < j0 || i1 < i0) { i0 = 0; i1 = -1; j0 = 0; j1 = -1; }
    }
  }
  box[0] = i0; box[1] = i1; box[2] = j0; box[3] = j1;
}

struct Prim { float ax, ay, az, bx, by, bz, r, sphere; };

// The smaller root of A u^2 + 2 B u + C = 0 where its discriminant is >= 0.
__device__ __forceinline__ bool smaller_root(float A, float B, float C, float& u) {
#pragma clang fp contract(off)
  const float disc = B * B - A * C;
  if (!(disc >= 0.f)) return false;
  u = (-B - sqrtf(disc)) / A;
  return true;
}

// Where the ray d = (dx, dy, 1), dd = d.d, enters the primitive: u = s - Z_m and the depth s; false where it does not, or
// not beyond `near`.  The one hit function of the pixel kernel (see the head of this file).
__device__ __forceinline__ bool capsule_hit(const Prim& p, float dx, float dy, float dd, float near, float& u, float& s) {
#pragma clang fp contract(off)
  const float zm = (p.az + p.bz) * 0.5f;
  const float ox = zm * dx, oy = zm * dy;
  const float max_ = ox - p.ax, may = oy - p.ay, maz = zm - p.az;
  const float rr = p.r * p.r;
  bool any = false;
  float best = pos_inf(), root;
  if (smaller_root(dd, (max_ * dx + may * dy) + maz, ((max_ * max_ + may * may) + maz * maz) - rr, root)) {
    any = true; best = root;
  }
  if (p.sphere == 0.f) {
    const float mbx = ox - p.bx, mby = oy - p.by, mbz = zm - p.bz;
    if (smaller_root(dd, (mbx * dx + mby * dy) + mbz, ((mbx * mbx + mby * mby) + mbz * mbz) - rr, root)) {
      any = true; best = fminf(best, root);
    }
    const float ex = p.bx - p.ax, ey = p.by - p.ay, ez = p.bz - p.az;
    const float dex = dy * ez - ey, dey = ex - dx * ez, dez = dx * ey - dy * ex;                   // d x e
    const float mex = may * ez - maz * ey, mey = maz * ex - max_ * ez, mez = max_ * ey - may * ex;   // m x e
    const float A = (dex * dex + dey * dey) + dez * dez;
    const float L2 = (ex * ex + ey * ey) + ez * ez;
    if (A > 0.f && smaller_root(A, (mex * dex + mey * dey) + mez * dez, ((mex * mex + mey * mey) + mez * mez) - rr * L2,
                                root)) {
      const float y = ((max_ * ex + may * ey) + maz * ez) + root * ((dx * ex + dy * ey) + ez);
      if (y > 0.f && y < L2) { any = true; best = fminf(best, root); }
    }
  }
  if (!any) return false;
  u = best;
  s = best + zm;
  return s > near;
}

__device__ __forceinline__ unsigned char byte_of(float v) {
  return (unsigned char)floorf(fminf(fmaxf(v, 0.f), 255.f));
}

__global__ void __launch_bounds__(OV_THREADS) overlay_pixels_kernel(OverlayArgs a) {
#pragma clang fp contract(off)
  __shared__ float l_prim[OVERLAY_PRIM_FLOATS][OV_THREADS];
  __shared__ int l_id[OV_THREADS];
  __shared__ int l_count[OV_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tiles_x = (a.W + OVERLAY_TILE - 1) / OVERLAY_TILE;
  const int ti = (int)blockIdx.x / tiles_x, tj = (int)blockIdx.x - ti * tiles_x;
  const int t = blockIdx.y;
  const int row0 = ti * OVERLAY_TILE, col0 = tj * OVERLAY_TILE;
  const int row1 = min(row0 + OVERLAY_TILE - 1, a.H - 1), col1 = min(col0 + OVERLAY_TILE - 1, a.W - 1);
  const int i = row0 + (tid >> 4), j = col0 + (tid & 15);
  const bool inside = i < a.H && j < a.W;
  const float dx = (((float)j + 0.5f) - a.cx) / a.fx, dy = (((float)i + 0.5f) - a.cy) / a.fy;
  const float dd = (dx * dx + dy * dy) + 1.f;
  const float* prims = a.prims + (size_t)t * a.P * OVERLAY_PRIM_FLOATS;
  const int* boxes = a.boxes + (size_t)t * a.P * OVERLAY_BOX_INTS;

  float best_s = pos_inf(), best_u = 0.f;
  int best_id = -1;
  for (int c0 = 0; c0 < a.P; c0 += OV_THREADS) {
    const int p = c0 + tid;
    bool keep = false;
    if (p < a.P) {
      const int4 b = *reinterpret_cast<const int4*>(boxes + (size_t)p * OVERLAY_BOX_INTS);   // (i0, i1, j0, j1)
      keep = b.x <= b.y && b.z <= b.w && b.x <= row1 && b.y >= row0 && b.z <= col1 && b.w >= col0;
    }
    const unsigned long long votes = __ballot(keep);
    if (lane == 0) l_count[wave] = __popcll(votes);
    __syncthreads();
    int base = 0, n = 0;
    for (int w = 0; w < OV_WAVES; ++w) {
      const int cnt = l_count[w];
      if (w < wave) base += cnt;
      n += cnt;
    }
    if (keep) {
      const int slot = base + __popcll(votes & ((1ull << lane) - 1ull));   // ascending index order; slot < 256
      const float* src = prims + (size_t)p * OVERLAY_PRIM_FLOATS;
      for (int k = 0; k < OVERLAY_PRIM_FLOATS; ++k) l_prim[k][slot] = src[k];
      l_id[slot] = p;
    }
    __syncthreads();
    if (inside) {
      for (int k = 0; k < n; ++k) {
        Prim q;
        q.ax = l_prim[0][k]; q.ay = l_prim[1][k]; q.az = l_prim[2][k];
        q.bx = l_prim[3][k]; q.by = l_prim[4][k]; q.bz = l_prim[5][k];
        q.r = l_prim[6][k]; q.sphere = l_prim[7][k];
        float u, s;
        if (capsule_hit(q, dx, dy, dd, a.near, u, s) && s < best_s) { best_s = s; best_u = u; best_id = l_id[k]; }
      }
    }
    __syncthreads();   // the next chunk overwrites the list
  }
  if (!inside) return;
  const size_t pix = ((size_t)t * a.H + i) * a.W + j;
  if (a.prim_id) a.prim_id[pix] = best_id;
  if (a.prim_depth) a.prim_depth[pix] = best_s;
  if (best_id < 0) return;

  // the outward normal at the hit: the hit point minus the nearest point of the segment, over the radius
  const float* w = prims + (size_t)best_id * OVERLAY_PRIM_FLOATS;
  const float zm = (w[2] + w[5]) * 0.5f;
  const float qx = (zm * dx - w[0]) + best_u * dx, qy = (zm * dy - w[1]) + best_u * dy, qz = (zm - w[2]) + best_u;
  float nx = qx, ny = qy, nz = qz;
  if (w[7] == 0.f) {
    const float ex = w[3] - w[0], ey = w[4] - w[1], ez = w[5] - w[2];
    const float L2 = (ex * ex + ey * ey) + ez * ez;
    const float along = fminf(fmaxf(((qx * ex + qy * ey) + qz * ez) / L2, 0.f), 1.f);   // (0 / 0: the first endpoint)
    nx = qx - along * ex; ny = qy - along * ey; nz = qz - along * ez;
  }
  nx = nx / w[6]; ny = ny / w[6]; nz = nz / w[6];
  const float dot = (nx * a.light[0] + ny * a.light[1]) + nz * a.light[2];
  const float intensity = a.ambient + (1.f - a.ambient) * fabsf(dot);
  const float* col = a.colors + (size_t)best_id * 3;
  unsigned char* rgb = a.rgb + pix * 3;
  const bool visible = !a.mesh_depth || best_s < a.mesh_depth[pix];   // a tie goes to the mesh; +inf never hides
  if (visible) {
    for (int c = 0; c < 3; ++c) rgb[c] = byte_of(255.f * (col[c] * intensity) + 0.5f);
  } else if (a.hidden_alpha > 0.f) {
    const float keep_in = 1.f - a.hidden_alpha;
    for (int c = 0; c < 3; ++c)
      rgb[c] = byte_of((keep_in * (float)rgb[c] + a.hidden_alpha * (255.f * (col[c] * intensity))) + 0.5f);
  }
}

}  // namespace

hipError_t launch_overlay_setup(const OverlayArgs& a, hipStream_t stream) {
  const long lanes = (long)a.T * a.P;
  hipLaunchKernelGGL(overlay_setup_kernel, dim3((unsigned)((lanes + OV_THREADS - 1) / OV_THREADS)), dim3(OV_THREADS), 0,
                     stream, a);
  return hipGetLastError();
}

hipError_t launch_overlay_pixels(const OverlayArgs& a, hipStream_t stream) {
  const unsigned tiles = (unsigned)(((a.W + OVERLAY_TILE - 1) / OVERLAY_TILE) * ((a.H + OVERLAY_TILE - 1) / OVERLAY_TILE));
  hipLaunchKernelGGL(overlay_pixels_kernel, dim3(tiles, (unsigned)a.T), dim3(OV_THREADS), 0, stream, a);
  return hipGetLastError();
}

}  // namespace empose
