// Global -> LDS staging of an operand block, shared by the fused MLP kernels (mlp_fused.hip, mlp_fused_x3.hip) and the
// single-layer row-block kernels.  Internal, gfx950 only.
//
// A workgroup that stages its block runs alone on its SIMDs (one wave each) and nothing hides a load's latency from it, so
// the copy is shaped around the number of round trips to memory:
//   * a thread moves 16-byte chunks; ALL of its loads of a batch (up to BATCH = 32 chunks: 128 registers, free before the
//     K loop) are issued back to back, then one wait, then the LDS writes.  A block of up to 32 chunks per thread -- the
//     64 x 320 input of the update MLPs is 20, the heads' 64 x 512 is 32 -- costs one round trip instead of one per chunk;
//   * everything the loop needs is copied out of the (kernarg-resident) descriptor by the CALLER and arrives by value: as
//     far as the compiler knows an LDS store could alias the descriptor, which otherwise costs a scalar reload and a wait
//     per chunk (gemm_epilogue.h has the same note);
//   * no division in the loop: chunk i = tid + u NT of a thread is (row, 16-byte column) = (i / c4n, i % c4n); the pair is
//     derived once and advanced by the wave-uniform (NT / c4n, NT % c4n) with one conditional carry;
//   * the zero fill of the pad columns and the clamping of rows past the end are selects: every lane issues every load
//     (a pad chunk re-reads the row's last real chunk), no branch depends on a lane.
// The chunk order, and with it what lands in which LDS word, is that of the plain loop `for (i = tid; ..; i += NT)`.
#pragma once
#include "gemm_epilogue.h"

namespace empose {
namespace stage {

typedef const __attribute__((address_space(1))) char* gbyte_t;
typedef const __attribute__((address_space(1))) f32x4* gvec_t;

constexpr int MAX_BATCH = 32;

// `n` chunks per thread (wave-uniform, even) in batches of BATCH: load() returns the thread's next chunk as it lies in
// memory, store(v) puts the thread's next chunk.  Both advance their own running position; a select on the loaded value
// belongs into store(), behind the wait.
template <int BATCH, class Load, class Store>
__device__ __forceinline__ void batches(int n, Load&& load, Store&& store) {
  static_assert(BATCH >= 2 && BATCH % 2 == 0 && BATCH <= MAX_BATCH, "pairs of chunks, at most 128 registers");
  for (int u0 = 0; u0 < n; u0 += BATCH) {
    f32x4 v[BATCH];
#pragma unroll
    for (int u = 0; u < BATCH; u += 2)
      if (u0 + u < n) {          // wave-uniform: a scalar branch
        v[u] = load();
        v[u + 1] = load();
      }
#pragma unroll
    for (int u = 0; u < BATCH; u += 2)
      if (u0 + u < n) {
        store(v[u]);
        store(v[u + 1]);
      }
  }
}

// Row-major x[M][ldx], rows m0 .. m0 + ROWS - 1, columns [0, K0) -> act[ROWS][lda]; columns [K0, kpad) are zero, rows
// past M - 1 repeat row M - 1 (never stored by the callers).  K0 % 4 == 0, kpad % 32 == 0, ldx % 4 == 0, m0 < M.
template <int ROWS, int NT, int BATCH = MAX_BATCH>
__device__ __forceinline__ void rows(const float* x, int ldx, int m0, int M, int K0, int kpad, float* act, int lda) {
  static_assert((ROWS * 8) % (NT * 2) == 0, "an even number of chunks per thread for every kpad % 32 == 0");
  const int tid = threadIdx.x;
  const int c4n = kpad >> 2, k4 = K0 >> 2;          // chunks per staged row; the first pad chunk
  const int n = ROWS * c4n / NT;                    // exact
  const int dr = NT / c4n, dc = NT - dr * c4n;      // wave-uniform
  const int r0 = tid / c4n, c0 = tid - r0 * c4n;    // the only per-lane division
  const int r_max = M - 1 - m0;
  const gbyte_t xb = (gbyte_t)(x + (size_t)m0 * ldx);   // wave-uniform base + 32-bit lane offset
  const unsigned ldx4 = (unsigned)ldx * 4u;
  auto advance = [&](int& r, int& c) {
    c += dc;
    const bool carry = c >= c4n;
    c -= carry ? c4n : 0;
    r += dr + (carry ? 1 : 0);
  };
  int lr = r0, lc = c0, sr = r0, sc = c0;
  batches<BATCH>(
      n,
      [&]() {
        const int rr = lr < r_max ? lr : r_max;
        const int cc = lc < k4 ? lc : k4 - 1;
        const f32x4 v = *(gvec_t)(xb + ((unsigned)rr * ldx4 + (unsigned)cc * 16u));
        advance(lr, lc);
        return v;
      },
      [&](const f32x4& v) {
        const bool pad = sc >= k4;
        *reinterpret_cast<f32x4*>(act + sr * lda + sc * 4) =
            f32x4{pad ? 0.f : v[0], pad ? 0.f : v[1], pad ? 0.f : v[2], pad ? 0.f : v[3]};
        advance(sr, sc);
      });
}

// Tile layout x_t[tile][ldx][64] -> act[kpad][64] as it lies (K-major): rows of k past K0 are zero.  kpad % 32 == 0.
template <int NT, int BATCH = MAX_BATCH>
__device__ __forceinline__ void tile(const float* x_t, int ldx, int tile_index, int K0, int kpad, float* act) {
  static_assert((32 * 16) % (NT * 2) == 0, "an even number of chunks per thread for every kpad % 32 == 0");
  const int n = kpad * 16 / NT;                     // exact
  const int i_end = K0 * 16;                        // the first pad chunk
  const gbyte_t xb = (gbyte_t)(x_t + (size_t)tile_index * ldx * 64);
  int li = threadIdx.x, si = threadIdx.x;
  batches<BATCH>(
      n,
      [&]() {
        const int ii = li < i_end ? li : i_end - 1;
        li += NT;
        return *(gvec_t)(xb + (unsigned)ii * 16u);
      },
      [&](const f32x4& v) {
        const bool pad = si >= i_end;
        reinterpret_cast<f32x4*>(act)[si] = f32x4{pad ? 0.f : v[0], pad ? 0.f : v[1], pad ? 0.f : v[2], pad ? 0.f : v[3]};
        si += NT;
      });
}

}  // namespace stage
}  // namespace empose
