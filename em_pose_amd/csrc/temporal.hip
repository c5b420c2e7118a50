// Temporal metrics (eval/temporal_metrics.py), gfx950 only: acceleration error and jitter of two point trajectories over a
// ragged batch of sequences.  The definitions are this project's own; backward stencils, so a chunked
// driver needs context on the left only:
//   acc[t]  = (x[t] - 2 x[t-1] + x[t-2]) fps^2              where frames t-2 .. t all count,
//   jerk[t] = (x[t] - 3 x[t-1] + 3 x[t-2] - x[t-3]) fps^3   where frames t-3 .. t all count,
// and per (frame, point) |acc_gt - acc_hat|, |jerk_hat|, |jerk_gt|.  Inputs are fp32; every difference, product and norm
// is float64, converted on load (a third difference times fps^3 = 216 000 has no fp32 bits to spare), without contraction
// into fused multiply-adds: a value is the same whichever launch, segment or slab computes it.
//
// The work is bound by memory.  A lane owns a point and walks one segment of TEMPORAL_SEGMENT frames of one row with the last
// three positions of both bodies in registers and the next two frames' loads in flight: each value is loaded once, plus three
// frames of lead-in per segment (3 / 32).  The lead-in also rebuilds the number of counting frames that end at the
// segment's first frame, so a stencil never reaches across a frame that does not count, and never across two rows.
//   per-point form (reduce == 0): a workgroup of 256 lanes holds 256 / min(P, 256) segments side by side (11 at the 22
//     joints), or one tile of 256 points of one segment; neighbouring lanes read neighbouring points and write
//     neighbouring doubles of a row.
//   reduced form (reduce == 1): a workgroup of 1024 lanes owns one segment and walks the points in tiles of 1024 (a mesh
//     slab of 1024 frames is 32 segments: the workgroups are few, so each brings 16 waves).  Per frame and tile each wave
//     sums its 64 lanes' six values (lane_reduce.h; the pairs of the butterfly), lanes 0 and 32 add the result to the
//     wave's slot in LDS -- tiles in ascending order -- and at the end the 16 waves are added in ascending order.
//     No atomics; the order follows from P alone, so a frame's row depends only on its own four frames.
// Every element of rows and defined is written; what is undefined is written as 0.
#include <hip/hip_runtime.h>

#include "data_kernels.h"
#include "lane_reduce.h"

#pragma clang fp contract(off)

namespace empose {

namespace {

constexpr int TP_THREADS = 256;        // per-point form
constexpr int TP_SUM_THREADS = 1024;   // reduced form: few workgroups (one per segment), so each brings 16 waves
constexpr int TP_SUM_WAVES = TP_SUM_THREADS / 64;
constexpr int TP_SUMS = 6;   // sum and sum of squares of the three quantities

// The last three positions of both bodies and the number of counting frames that end at the last one (at most 4).
struct Trail {
  double g1[3], g2[3], g3[3], h1[3], h2[3], h3[3];
  int run;
};

__device__ __forceinline__ void trail_reset(Trail& s) {
#pragma unroll
  for (int c = 0; c < 3; ++c) s.g1[c] = s.g2[c] = s.g3[c] = s.h1[c] = s.h2[c] = s.h3[c] = 0.0;
  s.run = 0;
}

__device__ __forceinline__ void load_point(const float* x, float (&v)[3]) {
  v[0] = x[0]; v[1] = x[1]; v[2] = x[2];
}

// One frame: the three values at this frame (0 where undefined: a select, a frame that does not count may hold anything)
// and the bits of `defined`; then the frame joins the trail.
__device__ __forceinline__ int trail_step(Trail& s, const float (&g)[3], const float (&h)[3], bool counts, double fps2,
                                          double fps3, double& err, double& jit_hat, double& jit_gt) {
  s.run = counts ? min(s.run + 1, 4) : 0;
  const bool has_acc = s.run >= 3, has_jerk = s.run >= 4;
  double se = 0.0, sh = 0.0, sg = 0.0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double g0 = (double)g[c], h0 = (double)h[c];
    const double ag = ((g0 - 2.0 * s.g1[c]) + s.g2[c]) * fps2;
    const double ah = ((h0 - 2.0 * s.h1[c]) + s.h2[c]) * fps2;
    const double jg = (((g0 - 3.0 * s.g1[c]) + 3.0 * s.g2[c]) - s.g3[c]) * fps3;
    const double jh = (((h0 - 3.0 * s.h1[c]) + 3.0 * s.h2[c]) - s.h3[c]) * fps3;
    const double d = ag - ah;
    se += d * d; sh += jh * jh; sg += jg * jg;
    s.g3[c] = s.g2[c]; s.g2[c] = s.g1[c]; s.g1[c] = g0;
    s.h3[c] = s.h2[c]; s.h2[c] = s.h1[c]; s.h1[c] = h0;
  }
  err = has_acc ? sqrt(se) : 0.0;
  jit_hat = has_jerk ? sqrt(sh) : 0.0;
  jit_gt = has_jerk ? sqrt(sg) : 0.0;
  return (has_acc ? TEMPORAL_DEFINED_ACC : 0) | (has_jerk ? TEMPORAL_DEFINED_JERK : 0);
}

// Walks point p of row n over the segment's frames [t0, t1) after its lead-in; emit(t, bits, err, jit_hat, jit_gt) per frame.
template <typename Emit>
__device__ __forceinline__ void walk_segment(const TemporalArgs& a, int n, int p, int t0, int t1, Emit emit) {
  const size_t row0 = (size_t)n * a.F;
  const int lead = max(t0 - 3, 0);
  const float* g = a.x_gt + ((row0 + lead) * a.P + p) * 3;
  const float* h = a.x_hat + ((row0 + lead) * a.P + p) * 3;
  const size_t step = (size_t)a.P * 3;
  Trail s;
  trail_reset(s);
  float gn[3], hn[3], gn2[3], hn2[3];   // the next frame and the one after it
  load_point(g, gn);
  load_point(h, hn);
  if (lead + 1 < t1) {
    load_point(g + step, gn2);
    load_point(h + step, hn2);
  }
  g += 2 * step; h += 2 * step;
  for (int t = lead; t < t1; ++t, g += step, h += step) {
    float gc[3], hc[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) { gc[c] = gn[c]; hc[c] = hn[c]; gn[c] = gn2[c]; hn[c] = hn2[c]; }
    if (t + 2 < t1) {   // two frames of loads in flight over this frame's arithmetic
      load_point(g, gn2);
      load_point(h, hn2);
    }
    const bool counts = a.valid[row0 + t] != 0;
    double err, jit_hat, jit_gt;
    const int bits = trail_step(s, gc, hc, counts, a.fps2, a.fps3, err, jit_hat, jit_gt);
    if (t >= t0) emit(t, bits, err, jit_hat, jit_gt);
  }
}

// reduce == 0.  lanes_per_seg = min(P, 256); a workgroup holds 256 / lanes_per_seg segments of one row, or one point tile.
__global__ void __launch_bounds__(TP_THREADS) temporal_points_kernel(TemporalArgs a, int lanes_per_seg, int segs_per_block,
                                                                     int n_seg, int seg_groups, int p_tiles) {
  unsigned b = blockIdx.x;
  const int tile = (int)(b % (unsigned)p_tiles); b /= (unsigned)p_tiles;
  const int group = (int)(b % (unsigned)seg_groups);
  const int n = (int)(b / (unsigned)seg_groups);
  const int tid = (int)threadIdx.x;
  const int sub = tid / lanes_per_seg;
  const int seg = group * segs_per_block + sub;
  const int p = tile * lanes_per_seg + (tid - sub * lanes_per_seg);
  if (sub >= segs_per_block || seg >= n_seg || p >= a.P) return;   // (no barrier in this kernel)
  const int t0 = seg * TEMPORAL_SEGMENT, t1 = min(t0 + TEMPORAL_SEGMENT, a.F);
  const size_t row0 = (size_t)n * a.F;
  walk_segment(a, n, p, t0, t1, [&](int t, int bits, double err, double jit_hat, double jit_gt) {
    double* out = a.rows + (row0 + t) * ((size_t)a.P * 3) + p;
    out[0] = err;
    out[a.P] = jit_hat;
    out[2 * (size_t)a.P] = jit_gt;
    if (p == 0) a.defined[row0 + t] = (unsigned char)bits;
  });
}

// reduce == 1.  One workgroup per (row, segment).
__global__ void __launch_bounds__(TP_SUM_THREADS) temporal_sums_kernel(TemporalArgs a, int n_seg) {
  __shared__ double part[TEMPORAL_SEGMENT][TP_SUM_WAVES][TP_SUMS];
  const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int seg = (int)(blockIdx.x % (unsigned)n_seg), n = (int)(blockIdx.x / (unsigned)n_seg);
  const int t0 = seg * TEMPORAL_SEGMENT, t1 = min(t0 + TEMPORAL_SEGMENT, a.F);
  const size_t row0 = (size_t)n * a.F;
  for (int i = tid; i < TEMPORAL_SEGMENT * TP_SUM_WAVES * TP_SUMS; i += TP_SUM_THREADS) (&part[0][0][0])[i] = 0.0;
  __syncthreads();
  for (int p0 = wave * 64; p0 < a.P; p0 += TP_SUM_THREADS) {   // the wave's tiles, ascending; the same for its 64 lanes
    const int p = p0 + lane;
    const bool live = p < a.P;
    walk_segment(a, n, live ? p : a.P - 1, t0, t1, [&](int t, int bits, double err, double jit_hat, double jit_gt) {
      if (p == 0) a.defined[row0 + t] = (unsigned char)bits;
      if (bits == 0) return;   // the same for every lane: nothing to add
      double v[TP_SUMS];
      v[0] = live ? err : 0.0;     v[1] = v[0] * v[0];
      v[2] = live ? jit_hat : 0.0; v[3] = v[2] * v[2];
      v[4] = live ? jit_gt : 0.0;  v[5] = v[4] * v[4];
      int base = 0, count = 0;
      LaneReduceScatter<TP_SUMS, 32, TP_SUMS, double>::run(v, lane, base, count);   // lanes < 32: sums 0 .. 2, the others 3 .. 5
      if ((lane & 31) == 0) {
        double* slot = &part[t - t0][wave][base];
#pragma unroll
        for (int k = 0; k < TP_SUMS / 2; ++k) slot[k] += v[k];
      }
    });
  }
  __syncthreads();
  for (int i = tid; i < (t1 - t0) * TP_SUMS; i += TP_SUM_THREADS) {
    const int f = i / TP_SUMS, q = i - f * TP_SUMS;
    double s = part[f][0][q];
    for (int w = 1; w < TP_SUM_WAVES; ++w) s += part[f][w][q];
    a.rows[(row0 + t0 + f) * TP_SUMS + q] = s;
  }
}

struct PointsShape { int lanes_per_seg, segs_per_block, n_seg, seg_groups, p_tiles; };

PointsShape points_shape(int F, int P) {
  PointsShape s;
  s.lanes_per_seg = P < TP_THREADS ? P : TP_THREADS;
  s.segs_per_block = TP_THREADS / s.lanes_per_seg;
  s.n_seg = (F + TEMPORAL_SEGMENT - 1) / TEMPORAL_SEGMENT;
  s.seg_groups = (s.n_seg + s.segs_per_block - 1) / s.segs_per_block;
  s.p_tiles = (P + s.lanes_per_seg - 1) / s.lanes_per_seg;
  return s;
}

}  // namespace

long temporal_rows_blocks(int N, int F, int P, int reduce) {
  const PointsShape s = points_shape(F, P);
  return reduce ? (long)N * s.n_seg : (long)N * s.seg_groups * s.p_tiles;
}

hipError_t launch_temporal_rows(const TemporalArgs& a, hipStream_t stream) {
  const PointsShape s = points_shape(a.F, a.P);
  const dim3 grid((unsigned)temporal_rows_blocks(a.N, a.F, a.P, a.reduce));
  if (a.reduce)
    hipLaunchKernelGGL(temporal_sums_kernel, grid, dim3(TP_SUM_THREADS), 0, stream, a, s.n_seg);
  else
    hipLaunchKernelGGL(temporal_points_kernel, grid, dim3(TP_THREADS), 0, stream, a, s.lanes_per_seg, s.segs_per_block,
                       s.n_seg, s.seg_groups, s.p_tiles);
  return hipGetLastError();
}

}  // namespace empose
