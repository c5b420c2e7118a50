// The epilogue of the train-mode layer products (train_fused.hip): shared by the fp32 tile kernel (gemm_f32.hip, ROLE 2 - 4)
// and the three-piece bf16 kernel (gemm_train_x3.hip), whose accumulators have the same layout. Internal, gfx950 only.
#pragma once
#include "gemm_epilogue.h"
#include "gemm_kernels.h"

namespace empose {

// Train-mode epilogues of a wave's WM x WN grid of 32 x 32 tiles (C/D layout: col = lane & 31, row = (r & 3) +
// 8 (r >> 2) + 4 (lane >> 5)).  Forward: C = acc + shift, and per 32-row block and column the sum and the centred sum of
// squares -> stat_part [M / 32][2][N].  Backward (e_y set): the product is dA; C = dyh = dA * PReLU'(e_s y + e_t) and
// stat_part [M / 32][3][N] = sums of dyh, dyh (y - mean) rstd, (yhat <= 0) dA yhat.
// Addressing as in gemm_epilogue.h: a wave-uniform base plus a 32-bit per-lane byte offset, row bounds resolved outside
// the loops (FULL) -- the straightforward form of this epilogue cost 15-20 us per 8192 x 512 launch.
template <int WM, int WN, bool FULL, bool BWD, bool CFULL>   // FULL / CFULL: no row / column of the wave's block is outside the matrix
__device__ __forceinline__ void train_epilogue_mode(float* __restrict__ C, float* __restrict__ part,
                                                    const float* __restrict__ shift, const float* __restrict__ ey,
                                                    const float* __restrict__ e_s, const float* __restrict__ e_t,
                                                    const float* __restrict__ e_mean, const float* __restrict__ e_rstd,
                                                    float slope, int M, int N, long ldc, long ldy,
                                                    const f32x16 (&acc)[WM][WN], int mw0, int nw0, int l31, int lh) {
  epi_gbyte_t cb = (epi_gbyte_t)(C + (long)mw0 * ldc);
  epi_cgbyte_t yb = BWD ? (epi_cgbyte_t)(ey + (long)mw0 * ldy) : nullptr;
  const unsigned ldc4 = (unsigned)ldc * 4u, ldy4 = (unsigned)ldy * 4u;
  // Every load of the epilogue -- the per-column constants and, reverse, the wave's whole block of y -- is issued before
  // the first store: loads and stores share one counter here (vmcnt), so a load that follows a tile's stores makes the
  // wave wait for those stores to drain -- one memory round trip per tile column (measured: the statistics epilogue cost
  // 10 us per 8192 x 512 x 512 launch that way).
  float sh[WN], es[WN], et[WN], mu[WN], rs[WN];
  bool col_ok[WN];
#pragma unroll
  for (int j = 0; j < WN; ++j) {
    const int n = nw0 + j * 32 + l31;
    col_ok[j] = CFULL || n < N;
    const int nc = col_ok[j] ? n : N - 1;
    sh[j] = (!BWD && shift) ? shift[nc] : 0.f;
    es[j] = BWD ? e_s[nc] : 0.f; et[j] = BWD ? e_t[nc] : 0.f; mu[j] = BWD ? e_mean[nc] : 0.f; rs[j] = BWD ? e_rstd[nc] : 0.f;
  }
  float yv[BWD ? WM : 1][BWD ? WN : 1][16];
  if (BWD) {
#pragma unroll
    for (int j = 0; j < WN; ++j) {
      const int n = nw0 + j * 32 + l31;
      const unsigned y_lane = (unsigned)(4 * lh) * ldy4 + (unsigned)(col_ok[j] ? n : N - 1) * 4u;
#pragma unroll
      for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int dm = i * 32 + (r & 3) + 8 * (r >> 2);
          yv[BWD ? i : 0][BWD ? j : 0][r] =
              (FULL || mw0 + 4 * lh + dm < M) ? *(epi_cgfloat_t)(yb + (y_lane + (unsigned)dm * ldy4)) : 0.f;
        }
    }
  }
  float ps[WM][WN][3];   // the partial sums: stored after the block's last row (a store under a branch in between makes
                         // the next tile column wait for everything issued so far)
#pragma unroll
  for (int j = 0; j < WN; ++j) {
    const int n = nw0 + j * 32 + l31;
    if (!CFULL && !col_ok[j]) continue;
    const unsigned c_lane = (unsigned)(4 * lh) * ldc4 + (unsigned)n * 4u;
#pragma unroll
    for (int i = 0; i < WM; ++i) {
      const int mb = mw0 + i * 32;
      const int rows_valid = FULL ? 32 : min(32, M - mb);
      if (!FULL && rows_valid <= 0) continue;
      if (!BWD) {
        float s1 = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int dm = i * 32 + (r & 3) + 8 * (r >> 2);
          if (!FULL && mw0 + 4 * lh + dm >= M) continue;
          const float y = acc[i][j][r] + sh[j];
          *(epi_gfloat_t)(cb + (c_lane + (unsigned)dm * ldc4)) = y;
          s1 += y;
        }
        // the block's sum and centred sum of squares (the two halves of the wave hold 16 rows each)
        s1 += __shfl_xor(s1, 32, 64);
        const float shift_mean = sh[j] - s1 * (1.f / (float)rows_valid);   // y - mean = acc + (sh - mean)
        float s2 = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int dm = i * 32 + (r & 3) + 8 * (r >> 2);
          const float d = acc[i][j][r] + shift_mean;
          if (FULL || mw0 + 4 * lh + dm < M) s2 += d * d;
        }
        s2 += __shfl_xor(s2, 32, 64);
        ps[i][j][0] = s1; ps[i][j][1] = s2; ps[i][j][2] = 0.f;
      } else {
        float sb = 0.f, sg = 0.f, sa = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int dm = i * 32 + (r & 3) + 8 * (r >> 2);
          if (!FULL && mw0 + 4 * lh + dm >= M) continue;
          const float y = yv[BWD ? i : 0][BWD ? j : 0][r];
          const float yh = es[j] * y + et[j];
          const float dA = acc[i][j][r];
          const float dyh = yh > 0.f ? dA : slope * dA;
          *(epi_gfloat_t)(cb + (c_lane + (unsigned)dm * ldc4)) = dyh;
          sb += dyh;
          sg += dyh * ((y - mu[j]) * rs[j]);
          sa += yh > 0.f ? 0.f : dA * yh;
        }
        sb += __shfl_xor(sb, 32, 64);
        sg += __shfl_xor(sg, 32, 64);
        sa += __shfl_xor(sa, 32, 64);
        ps[i][j][0] = sb; ps[i][j][1] = sg; ps[i][j][2] = sa;
      }
    }
  }
  if (lh == 0 && part) {
#pragma unroll
    for (int j = 0; j < WN; ++j) {
      const int n = nw0 + j * 32 + l31;
      if (!CFULL && !col_ok[j]) continue;
#pragma unroll
      for (int i = 0; i < WM; ++i) {
        const int mb = mw0 + i * 32;
        if (!FULL && mb >= M) continue;
        float* pp = part + (size_t)(mb >> 5) * (BWD ? 3 : 2) * N;
        pp[n] = ps[i][j][0];
        pp[N + n] = ps[i][j][1];
        if (BWD) pp[2 * N + n] = ps[i][j][2];
      }
    }
  }
}

template <int WM, int WN, bool BWD>   // BWD: the reverse epilogue (ROLE 3), else the forward one (ROLE 2)
__device__ __forceinline__ void train_epilogue(const GemmProb& p, const f32x16 (&acc)[WM][WN], int mw0, int nw0, int l31,
                                               int lh) {
  float* C = p.C; float* part = p.stat_part;
  const float* shift = p.shift; const float* ey = p.e_y;
  const float* e_s = p.e_s; const float* e_t = p.e_t; const float* e_mean = p.e_mean; const float* e_rstd = p.e_rstd;
  const long ldc = p.ldc, ldy = p.ld_ey;
  const int M = p.M, N = p.N;
  const float slope = BWD ? p.e_slope[0] : 0.f;
  mw0 = __builtin_amdgcn_readfirstlane(mw0);
  nw0 = __builtin_amdgcn_readfirstlane(nw0);
  const bool full = mw0 + 32 * WM <= M, cfull = nw0 + 32 * WN <= N;
#define EMPOSE_TEPI(FULL, BWD, CFULL) \
  train_epilogue_mode<WM, WN, FULL, BWD, CFULL>(C, part, shift, ey, e_s, e_t, e_mean, e_rstd, slope, M, N, ldc, ldy, acc, mw0, nw0, l31, lh)
  if (full && cfull) EMPOSE_TEPI(true, BWD, true); else if (full) EMPOSE_TEPI(true, BWD, false); else EMPOSE_TEPI(false, BWD, false);
#undef EMPOSE_TEPI
}

}  // namespace empose
