// Smoothing of estimated pose sequences (eval/smoothing.py), gfx950 only: a zero-phase FIR window for whole recordings and
// the causal One-Euro filter (Casiez, Roussel, Vogel 2012) for streaming.  A row of the input is
// [3 J rotation-vector columns | C linear columns | padding]; an *item* is one joint or one channel.  Rotations are
// filtered as rotations, on SO(3) through unit quaternions (quat.h), never as rotation-vector components, which jump at
// |r| = pi.  A frame counts where valid != 0 (valid == nullptr: everywhere); a *run* is a maximal stretch of consecutive
// counting frames of one row.  No filter reaches across a frame that does not count or across two rows; such a frame gets
// its input columns copied bit for bit, and what it holds (NaN included) never reaches another frame.  Inputs and outputs
// are fp32, all arithmetic is float64 without contraction into fused multiply-adds, there are no atomics: a row's result
// does not depend on the batch or the launch geometry, and repeated calls give the same bits.  Columns of `out` at or
// beyond 3 J + C are never written.  The definitions are this project's own.
//
// Window.  One side w[0 .. R] of a symmetric kernel, w[0] > 0, w[k] >= 0.  For a counting frame t of the run [a, b] the
// half-width shrinks symmetrically, r = min(R, t - a, b - t): the window never leaves the run and stays symmetric, so
// constant-velocity motion is reproduced, and the end frames of a run pass through.
//   channel:   acc = w0 x[t];  for k = 1 .. r ascending  acc += w_k (x[t-k] + x[t+k]),  wsum = w0, wsum += 2 w_k;
//              out = acc / wsum
//   rotation:  c = q(r[t]);  acc = w0 c;  acc += w_k (s- q(r[t-k]) + s+ q(r[t+k])),  s = -1 where the dot product with c
//              is negative, else +1;  out = the rotation vector of acc / |acc| with w >= 0, |out| <= pi.
//              This is the sign-aligned chordal mean; |acc| >= w0 > 0 by construction (every added term has a
//              non-negative dot product with c).
//   A workgroup owns (row, segment of SMOOTH_SEGMENT frames, tile of SW_ITEMS items).  It stages the segment and its halo
//   of R frames on either side in LDS -- a rotation vector becomes a quaternion once per workgroup, not once per tap --
//   as four doubles per (frame, item) (a channel uses the first): (64 + 2 * 32) * 8 * 32 B = 32 KiB, which is why the
//   columns are tiled.  Then a lane per (frame, item) walks k upwards until a frame on either side does not count.
//
// One-Euro.  alpha(fc) = 1 / (1 + fps / (2 pi fc)).  At the first counting frame of a run x^ = x, s^ = 0.  Afterwards
//   channel:   d = (x - x^) fps;  s^ += alpha(d_cutoff) (d - s^);  fc = min_cutoff + beta |s^|;  x^ += alpha(fc) (x - x^)
//   rotation:  q = q(r) in the hemisphere of x^;  delta = log(x^-1 q);  theta = 2 |delta| in [0, pi];  d = theta fps;
//              s^ and fc as above;  x^ <- x^ exp(alpha(fc) delta), renormalised;  out = its rotation vector, |out| <= pi.
//   A frame that does not count ends the run and clears the state.  A lane owns one (row, item) and walks the F frames
//   with the next two frames' loads in flight, as walk_segment of temporal.hip does.  The state ([N][J + C][6] doubles:
//   x^ as 4, s^, live flag) enters and leaves in full precision, so chunked feeding gives the bits of whole feeding.
#include <hip/hip_runtime.h>

#include "data_kernels.h"

#pragma clang fp contract(off)

#include "quat.h"

namespace empose {

namespace {

constexpr int SW_THREADS = 256;
constexpr int SW_ITEMS = 8;                                            // items per column tile
constexpr int SW_FRAMES = SMOOTH_SEGMENT + 2 * SMOOTH_MAX_RADIUS;      // staged frames at most
constexpr int SE_THREADS = 64;
constexpr double TWO_PI = 6.283185307179586476925286766559;

// the first column of item `it` and whether it is a rotation
__device__ __forceinline__ int item_col(int it, int J, bool& rot) {
  rot = it < J;
  return rot ? 3 * it : 3 * J + (it - J);
}

__device__ __forceinline__ void copy_item(const float* src, float* dst, bool rot) {
  dst[0] = src[0];
  if (rot) { dst[1] = src[1]; dst[2] = src[2]; }
}

__global__ void __launch_bounds__(SW_THREADS) smooth_window_kernel(SmoothArgs a, int n_seg, int n_tiles) {
  __shared__ double stage[SW_FRAMES][SW_ITEMS][4];
  __shared__ double w[SMOOTH_MAX_RADIUS + 1];
  __shared__ unsigned char ok[SW_FRAMES];
  unsigned b = blockIdx.x;
  const int tile = (int)(b % (unsigned)n_tiles); b /= (unsigned)n_tiles;
  const int seg = (int)(b % (unsigned)n_seg);
  const int n = (int)(b / (unsigned)n_seg);
  const int tid = (int)threadIdx.x;
  const int R = a.R, items = a.J + a.C;
  const int t0 = seg * SMOOTH_SEGMENT, t1 = min(t0 + SMOOTH_SEGMENT, a.F);
  const int lo = t0 - R, nf = (t1 - t0) + 2 * R;   // staged frame f is frame lo + f of the row
  const size_t row0 = (size_t)n * a.F;
  if (tid == 0) {
#pragma unroll
    for (int k = 0; k <= SMOOTH_MAX_RADIUS; ++k) w[k] = a.taps[k];   // (constant indices: no copy of the arguments in scratch)
  }
  for (int i = tid; i < nf * SW_ITEMS; i += SW_THREADS) {
    const int f = i / SW_ITEMS, it = tile * SW_ITEMS + (i - f * SW_ITEMS);
    const int g = lo + f;
    const bool counts = g >= 0 && g < a.F && (a.valid == nullptr || a.valid[row0 + g] != 0);
    if (i - f * SW_ITEMS == 0) ok[f] = counts ? 1 : 0;
    if (!counts || it >= items) continue;   // never read
    bool rot;
    const float* x = a.in + (row0 + g) * a.ld_in + item_col(it, a.J, rot);
    double* s = stage[f][i - f * SW_ITEMS];
    if (rot) {
      const Quat q = q_from_rotvec(x);
      s[0] = q.w; s[1] = q.x; s[2] = q.y; s[3] = q.z;
    } else {
      s[0] = (double)x[0];
    }
  }
  __syncthreads();
  for (int i = tid; i < (t1 - t0) * SW_ITEMS; i += SW_THREADS) {
    const int df = i / SW_ITEMS, slot = i - df * SW_ITEMS, it = tile * SW_ITEMS + slot;
    if (it >= items) continue;
    const int f = R + df;
    bool rot;
    const int col = item_col(it, a.J, rot);
    float* o = a.out + (row0 + t0 + df) * a.ld_out + col;
    if (!ok[f]) {
      copy_item(a.in + (row0 + t0 + df) * a.ld_in + col, o, rot);
      continue;
    }
    const double w0 = w[0];
    if (rot) {
      const double* cs = stage[f][slot];
      const Quat c = {cs[0], cs[1], cs[2], cs[3]};
      Quat acc = {w0 * c.w, w0 * c.x, w0 * c.y, w0 * c.z};
      for (int k = 1; k <= R; ++k) {
        if (!(ok[f - k] && ok[f + k])) break;
        const double* ps = stage[f - k][slot];
        const double* ns = stage[f + k][slot];
        const Quat p = {ps[0], ps[1], ps[2], ps[3]}, q = {ns[0], ns[1], ns[2], ns[3]};
        const double sp = q_dot(c, p) < 0.0 ? -1.0 : 1.0, sq = q_dot(c, q) < 0.0 ? -1.0 : 1.0;
        const double wk = w[k];
        acc.w += wk * (sp * p.w + sq * q.w);
        acc.x += wk * (sp * p.x + sq * q.x);
        acc.y += wk * (sp * p.y + sq * q.y);
        acc.z += wk * (sp * p.z + sq * q.z);
      }
      const double nrm = sqrt(q_dot(acc, acc));
      q_to_rotvec({acc.w / nrm, acc.x / nrm, acc.y / nrm, acc.z / nrm}, o);
    } else {
      double acc = w0 * stage[f][slot][0], wsum = w0;
      for (int k = 1; k <= R; ++k) {
        if (!(ok[f - k] && ok[f + k])) break;
        const double wk = w[k];
        acc += wk * (stage[f - k][slot][0] + stage[f + k][slot][0]);
        wsum += 2.0 * wk;
      }
      o[0] = (float)(acc / wsum);
    }
  }
}

__device__ __forceinline__ double euro_alpha(double fps, double fc) { return 1.0 / (1.0 + fps / (TWO_PI * fc)); }

__device__ __forceinline__ void load_item(const float* x, bool rot, float (&v)[3]) {
  v[0] = x[0];
  if (rot) { v[1] = x[1]; v[2] = x[2]; }
}

__global__ void __launch_bounds__(SE_THREADS) smooth_one_euro_kernel(SmoothArgs a) {
  const int items = a.J + a.C;
  const long g = (long)blockIdx.x * SE_THREADS + threadIdx.x;
  if (g >= (long)a.N * items) return;   // (no barrier in this kernel)
  const int n = (int)(g / items), it = (int)(g - (long)n * items);
  bool rot;
  const int col = item_col(it, a.J, rot);
  const size_t row0 = (size_t)n * a.F;
  Quat x = {0.0, 0.0, 0.0, 0.0};   // a channel's value is x.w
  double s = 0.0;
  bool live = false;
  if (a.state_in) {
    const double* st = a.state_in + (size_t)g * SMOOTH_STATE;
    x = {st[0], st[1], st[2], st[3]};
    s = st[4];
    live = st[5] != 0.0;
  }
  const double alpha_d = euro_alpha(a.fps, a.d_cutoff);
  const float* in = a.in + row0 * a.ld_in + col;
  float* out = a.out + row0 * a.ld_out + col;
  const unsigned char* valid = a.valid ? a.valid + row0 : nullptr;
  float vn[3] = {0.f, 0.f, 0.f}, vn2[3] = {0.f, 0.f, 0.f};   // the next frame and the one after it
  unsigned char cn = 1, cn2 = 1;
  load_item(in, rot, vn);
  if (valid) cn = valid[0];
  if (1 < a.F) {
    load_item(in + a.ld_in, rot, vn2);
    if (valid) cn2 = valid[1];
  }
  in += 2 * (size_t)a.ld_in;
  for (int t = 0; t < a.F; ++t, in += a.ld_in, out += a.ld_out) {
    float v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) { v[c] = vn[c]; vn[c] = vn2[c]; }
    const bool counts = cn != 0;
    cn = cn2;
    if (t + 2 < a.F) {   // two frames of loads in flight over this frame's arithmetic
      load_item(in, rot, vn2);
      if (valid) cn2 = valid[t + 2];
    }
    if (!counts) {
      live = false;
      x = {0.0, 0.0, 0.0, 0.0};
      s = 0.0;
      copy_item(v, out, rot);
      continue;
    }
    if (rot) {
      if (!live) {
        x = q_from_rotvec(v);
        s = 0.0;
        live = true;
      } else {
        const Quat q = q_toward(x, q_from_rotvec(v));
        double delta[3];
        q_log(q_conj_mul(x, q), delta);
        const double theta = 2.0 * sqrt(delta[0] * delta[0] + delta[1] * delta[1] + delta[2] * delta[2]);
        const double d = theta * a.fps;
        s += alpha_d * (d - s);
        const double fc = a.min_cutoff + a.beta * fabs(s);
        const Quat y = q_step(x, delta, euro_alpha(a.fps, fc));
        const double nrm = sqrt(q_dot(y, y));
        x = {y.w / nrm, y.x / nrm, y.y / nrm, y.z / nrm};
      }
      q_to_rotvec(x, out);
    } else {
      const double xv = (double)v[0];
      if (!live) {
        x.w = xv;
        s = 0.0;
        live = true;
      } else {
        const double d = (xv - x.w) * a.fps;
        s += alpha_d * (d - s);
        const double fc = a.min_cutoff + a.beta * fabs(s);
        x.w += euro_alpha(a.fps, fc) * (xv - x.w);
      }
      out[0] = (float)x.w;
    }
  }
  if (a.state_out) {
    double* st = a.state_out + (size_t)g * SMOOTH_STATE;
    st[0] = x.w; st[1] = x.x; st[2] = x.y; st[3] = x.z;
    st[4] = s;
    st[5] = live ? 1.0 : 0.0;
  }
}

int window_tiles(int J, int C) { return (J + C + SW_ITEMS - 1) / SW_ITEMS; }
int window_segments(int F) { return (F + SMOOTH_SEGMENT - 1) / SMOOTH_SEGMENT; }

}  // namespace

long smooth_window_blocks(int N, int F, int J, int C) { return (long)N * window_segments(F) * window_tiles(J, C); }

hipError_t launch_smooth_window(const SmoothArgs& a, hipStream_t stream) {
  const dim3 grid((unsigned)smooth_window_blocks(a.N, a.F, a.J, a.C));
  hipLaunchKernelGGL(smooth_window_kernel, grid, dim3(SW_THREADS), 0, stream, a, window_segments(a.F), window_tiles(a.J, a.C));
  return hipGetLastError();
}

hipError_t launch_smooth_one_euro(const SmoothArgs& a, hipStream_t stream) {
  const long lanes = (long)a.N * (a.J + a.C);
  hipLaunchKernelGGL(smooth_one_euro_kernel, dim3((unsigned)((lanes + SE_THREADS - 1) / SE_THREADS)), dim3(SE_THREADS), 0,
                     stream, a);
  return hipGetLastError();
}

}  // namespace empose
