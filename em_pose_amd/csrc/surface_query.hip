// Point-to-mesh queries (eval/surface_metrics.py), gfx950 only: for every query point of a frame, the closest point of the
// frame's triangle mesh and whether the point lies inside it.  Both definitions are this project's own (DESIGN.md
// section 9, include/empose_hip.h).
//
// A workgroup of 512 lanes owns one frame and a block of up to 12 queries.  The frame's vertices go to LDS once (dynamic
// LDS, 12 bytes a vertex: 82.7 KB for the 6890 vertices of the body; frames above SURFACE_LDS_MAX_V vertices are gathered
// from L2 instead, the same code otherwise).  Lane l walks the faces l, l + 512, ...: it reads the face's three ids,
// gathers the corners, forms the two edges (and, for the inside test, the projected box, the orientation and which edges
// the face owns) once, and then runs the block's queries over it with a running best key per query in registers,
//   key = (bits of d^2) << 32 | face id,
// an unsigned 64-bit integer whose order is (d^2, face id) because d^2 >= 0.  The inside test keeps one parity bit per
// query.  At the end the keys are reduced by integer min and the parities by xor, over the wave with lane exchanges and
// over the 8 waves through LDS: both are exact in any order, so neither the lane a face lands on nor the block a query
// lands in can show in a result.  Lane k < 12 then evaluates query k on its winning face once more -- the same function,
// the same bits -- for the barycentric weights and the closest point.
// Floating-point contraction is off for the whole file and every fused multiply-add is written out, so the two
// instantiations of the pair function cannot be contracted differently.
#include <hip/hip_runtime.h>

#include "launch.h"
#include "surface_kernels.h"

#pragma clang fp contract(off)

namespace empose {

namespace {

constexpr int SQ_WAVES = SURFACE_THREADS / 64;
constexpr int QB = SURFACE_QUERY_BLOCK;
constexpr unsigned long long SQ_NO_KEY = ~0ull;

struct P3 { float x, y, z; };

__device__ __forceinline__ P3 sub(const P3 a, const P3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ float dot(const P3 a, const P3 b) { return fmaf(a.x, b.x, fmaf(a.y, b.y, a.z * b.z)); }
// a + s u
__device__ __forceinline__ P3 along(const P3 a, float s, const P3 u) {
  return {fmaf(s, u.x, a.x), fmaf(s, u.y, a.y), fmaf(s, u.z, a.z)};
}

struct Hit { float d2; P3 c; float bary[3]; };

// The closest point of the closed triangle (a, b, c) to p by Voronoi regions, in the order vertex a, vertex b, edge ab,
// vertex c, edge ac, edge bc, interior; every comparison includes its boundary, so a triangle without area ends in an edge
// or a vertex.  A quotient whose denominator is not positive is taken as 0.
__device__ __forceinline__ Hit closest_on_face(const P3 p, const P3 a, const P3 b, const P3 c) {
  const P3 ab = sub(b, a), ac = sub(c, a);
  const P3 ap = sub(p, a), bp = sub(p, b), cp = sub(p, c);
  const float d1 = dot(ab, ap), d2 = dot(ac, ap);
  const float d3 = dot(ab, bp), d4 = dot(ac, bp);
  const float d5 = dot(ab, cp), d6 = dot(ac, cp);
  const float vc = fmaf(d1, d4, -(d3 * d2));
  const float vb = fmaf(d5, d2, -(d1 * d6));
  const float va = fmaf(d3, d6, -(d5 * d4));
  Hit h;
  if (d1 <= 0.f && d2 <= 0.f) {
    h.c = a; h.bary[0] = 1.f; h.bary[1] = 0.f; h.bary[2] = 0.f;
  } else if (d3 >= 0.f && d4 <= d3) {
    h.c = b; h.bary[0] = 0.f; h.bary[1] = 1.f; h.bary[2] = 0.f;
  } else if (vc <= 0.f && d1 >= 0.f && d3 <= 0.f) {
    const float den = d1 - d3;
    const float t = den > 0.f ? d1 / den : 0.f;
    h.c = along(a, t, ab); h.bary[0] = 1.f - t; h.bary[1] = t; h.bary[2] = 0.f;
  } else if (d6 >= 0.f && d5 <= d6) {
    h.c = c; h.bary[0] = 0.f; h.bary[1] = 0.f; h.bary[2] = 1.f;
  } else if (vb <= 0.f && d2 >= 0.f && d6 <= 0.f) {
    const float den = d2 - d6;
    const float t = den > 0.f ? d2 / den : 0.f;
    h.c = along(a, t, ac); h.bary[0] = 1.f - t; h.bary[1] = 0.f; h.bary[2] = t;
  } else if (va <= 0.f && (d4 - d3) >= 0.f && (d5 - d6) >= 0.f) {
    const float num = d4 - d3;
    const float den = num + (d5 - d6);
    const float t = den > 0.f ? num / den : 0.f;
    h.c = along(b, t, sub(c, b)); h.bary[0] = 0.f; h.bary[1] = 1.f - t; h.bary[2] = t;
  } else {
    const float pa = fmaxf(va, 0.f), pb = fmaxf(vb, 0.f), pc = fmaxf(vc, 0.f);
    const float s = (pa + pb) + pc;
    const float v = s > 0.f ? pb / s : 0.f;
    const float w = s > 0.f ? pc / s : 0.f;
    h.c = along(along(a, v, ab), w, ac);
    h.bary[0] = fmaxf((1.f - v) - w, 0.f); h.bary[1] = v; h.bary[2] = w;
  }
  const P3 d = sub(p, h.c);
  h.d2 = dot(d, d);
  return h;
}

// The edge function of the directed edge f -> t (vertex ids idf, idt) at (px, py), float64 on the xy projection: the value
// is formed from the endpoint with the lower id to the one with the higher, and negated when the edge runs the other way,
// so the two faces that share an edge get the same number with opposite signs.
__device__ __forceinline__ double edge_fn(int idf, const P3 f, int idt, const P3 t, float px, float py) {
  const bool swap = idf > idt;
  const P3 lo = swap ? t : f, hi = swap ? f : t;
  const double e = ((double)hi.x - (double)lo.x) * ((double)py - (double)lo.y) -
                   ((double)hi.y - (double)lo.y) * ((double)px - (double)lo.x);
  return swap ? -e : e;
}
// The half-open rule: a point on the edge f -> t (oriented so that the face's area is positive) belongs to the face when
// the edge runs down in y, or level and towards +x -- the side the point displaced by (+eps, +eps^2) would fall on.
__device__ __forceinline__ bool owns_edge(const P3 f, const P3 t) { return t.y < f.y || (t.y == f.y && t.x > f.x); }

template <bool IN_LDS>
__global__ void __launch_bounds__(SURFACE_THREADS) surface_query_kernel(SurfaceArgs a) {
  extern __shared__ __attribute__((aligned(16))) float sv[];   // IN_LDS: the frame's vertices [V][3]
  __shared__ unsigned long long wave_key[SQ_WAVES][QB];
  __shared__ unsigned wave_par[SQ_WAVES];
  __shared__ float4 qp[QB];                                    // (p, 1 if the query counts else 0)
  const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const size_t t = blockIdx.x;
  const int q0 = (int)blockIdx.y * QB;
  const int nq = min(QB, a.Q - q0);
  const float* gv = a.vertices + t * (size_t)a.V * 3;

  if (tid < QB) {
    float x = 0.f, y = 0.f, z = 0.f, on = 0.f;
    if (tid < nq) {
      const size_t row = t * (size_t)a.Q + (size_t)(q0 + tid);
      if (!a.mask || a.mask[row] != 0.f) { x = a.points[row * 3]; y = a.points[row * 3 + 1]; z = a.points[row * 3 + 2]; on = 1.f; }
    }
    qp[tid] = make_float4(x, y, z, on);
  }
  __syncthreads();
  unsigned live = 0;   // the queries stay in LDS: every lane reads one at the same address, a broadcast
  unsigned long long best[QB];
#pragma unroll
  for (int k = 0; k < QB; ++k) {
    if (qp[k].w != 0.f) live |= 1u << k;
    best[k] = SQ_NO_KEY;
  }
  if (live == 0) {   // every query of the block is masked (a frame that does not count): nothing to stage or to walk
    if (tid < nq) {
      const size_t row = t * (size_t)a.Q + (size_t)(q0 + tid);
      a.dist[row] = __builtin_inff();
      if (a.face) a.face[row] = -1;
      if (a.bary) a.bary[row * 3] = a.bary[row * 3 + 1] = a.bary[row * 3 + 2] = 0.f;
      if (a.closest) a.closest[row * 3] = a.closest[row * 3 + 1] = a.closest[row * 3 + 2] = 0.f;
      if (a.want_inside && a.inside) a.inside[row] = 0;
    }
    return;
  }
  if (IN_LDS) {
    for (int i = tid; i < a.V * 3; i += SURFACE_THREADS) sv[i] = gv[i];
    __syncthreads();
  }
  const float* vsrc = IN_LDS ? sv : gv;
  auto corner = [&](int id) -> P3 { const float* v = vsrc + (size_t)id * 3; return {v[0], v[1], v[2]}; };
  auto clamp_id = [&](int id) -> int { return min(max(id, 0), a.V - 1); };   // (a table that was not checked stays inside)
  unsigned parity = 0;

  for (int f = tid; f < a.F; f += SURFACE_THREADS) {
    const int* fi = a.faces + (size_t)f * 3;
    const int i0 = clamp_id(fi[0]), i1 = clamp_id(fi[1]), i2 = clamp_id(fi[2]);
    const P3 A = corner(i0), B = corner(i1), C = corner(i2);
    // inside test, once per face: the projected box, the sign of the projected area, the edges the face owns
    float min_x = 0.f, max_x = 0.f, min_y = 0.f, max_y = 0.f;
    bool flat = true, neg = false, own0 = false, own1 = false, own2 = false;
    if (a.want_inside) {
      const double area = edge_fn(i0, A, i1, B, C.x, C.y);
      flat = !(area > 0.0) && !(area < 0.0);
      neg = area < 0.0;
      min_x = fminf(A.x, fminf(B.x, C.x)); max_x = fmaxf(A.x, fmaxf(B.x, C.x));
      min_y = fminf(A.y, fminf(B.y, C.y)); max_y = fmaxf(A.y, fmaxf(B.y, C.y));
      own0 = neg ? owns_edge(B, A) : owns_edge(A, B);
      own1 = neg ? owns_edge(C, B) : owns_edge(B, C);
      own2 = neg ? owns_edge(A, C) : owns_edge(C, A);
    }
#pragma unroll
    for (int k = 0; k < QB; ++k) {
      if (!((live >> k) & 1u)) continue;   // the same for every lane
      const float4 q = qp[k];
      const P3 p = {q.x, q.y, q.z};
      const Hit h = closest_on_face(p, A, B, C);
      const unsigned long long key = ((unsigned long long)__float_as_uint(h.d2) << 32) | (unsigned)f;
      best[k] = key < best[k] ? key : best[k];
      if (a.want_inside && !flat) {
        const float px = p.x, py = p.y;
        // strictly outside the projected box: outside the projected triangle, nothing to evaluate
        if (px < min_x || px > max_x || py < min_y || py > max_y) continue;
        double w0 = edge_fn(i0, A, i1, B, px, py);
        double w1 = edge_fn(i1, B, i2, C, px, py);
        double w2 = edge_fn(i2, C, i0, A, px, py);
        if (neg) { w0 = -w0; w1 = -w1; w2 = -w2; }
        const bool covered = (w0 > 0.0 || (w0 == 0.0 && own0)) && (w1 > 0.0 || (w1 == 0.0 && own1)) &&
                             (w2 > 0.0 || (w2 == 0.0 && own2));
        if (!covered) continue;
        // the ray's crossing of the face's plane lies above p: sum_k w_k (z of the opposite corner - p.z) > 0
        const double pz = (double)p.z;
        const double s = (w0 * ((double)C.z - pz) + w1 * ((double)A.z - pz)) + w2 * ((double)B.z - pz);
        if (s > 0.0) parity ^= 1u << k;
      }
    }
  }

  // the wave, then the waves: integer min and xor, exact in any order
#pragma unroll
  for (int k = 0; k < QB; ++k) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const unsigned long long o = __shfl_xor(best[k], off, 64);
      best[k] = o < best[k] ? o : best[k];
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) parity ^= __shfl_xor(parity, off, 64);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < QB; ++k) wave_key[wave][k] = best[k];
    wave_par[wave] = parity;
  }
  __syncthreads();
  if (tid >= nq) return;

  const int k = tid;
  const size_t row = t * (size_t)a.Q + (size_t)(q0 + k);
  const bool on = qp[k].w != 0.f;
  unsigned long long key = wave_key[0][k];
  unsigned par = wave_par[0];
  for (int w = 1; w < SQ_WAVES; ++w) {
    key = wave_key[w][k] < key ? wave_key[w][k] : key;
    par ^= wave_par[w];
  }
  Hit h;
  h.d2 = __builtin_inff(); h.c = {0.f, 0.f, 0.f}; h.bary[0] = h.bary[1] = h.bary[2] = 0.f;
  int face = -1;
  if (on && key != SQ_NO_KEY) {
    face = (int)(unsigned)(key & 0xffffffffull);
    const int* fi = a.faces + (size_t)face * 3;
    const P3 pk = {qp[k].x, qp[k].y, qp[k].z};
    h = closest_on_face(pk, corner(clamp_id(fi[0])), corner(clamp_id(fi[1])), corner(clamp_id(fi[2])));
    h.d2 = __uint_as_float((unsigned)(key >> 32));   // (the same bits: the same function on the same operands)
  }
  a.dist[row] = on ? sqrtf(h.d2) : __builtin_inff();
  if (a.face) a.face[row] = face;
  if (a.bary) { a.bary[row * 3] = h.bary[0]; a.bary[row * 3 + 1] = h.bary[1]; a.bary[row * 3 + 2] = h.bary[2]; }
  if (a.closest) { a.closest[row * 3] = h.c.x; a.closest[row * 3 + 1] = h.c.y; a.closest[row * 3 + 2] = h.c.z; }
  if (a.want_inside && a.inside) a.inside[row] = on ? (unsigned char)((par >> k) & 1u) : (unsigned char)0;
}

}  // namespace

hipError_t launch_surface_query(const SurfaceArgs& a, hipStream_t stream) {
  const dim3 grid((unsigned)a.T, (unsigned)((a.Q + QB - 1) / QB));
  if (a.V <= SURFACE_LDS_MAX_V)
    return launch_lds(surface_query_kernel<true>, grid, dim3(SURFACE_THREADS), (size_t)a.V * 3 * sizeof(float), stream, a);
  hipLaunchKernelGGL(surface_query_kernel<false>, grid, dim3(SURFACE_THREADS), 0, stream, a);
  return hipGetLastError();
}

}  // namespace empose
