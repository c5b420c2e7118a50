// Per-vertex error between two posed bodies, sum_v |v_A - v_B| and sum_v |v_A - v_B|^2 per frame (PVE / MPVPE, the
// surface counterpart of MPJPE; this project's addition, the reference has no such metric), gfx950 only.
//
// mesh_pair_error_kernel is mesh_rows_kernel (mesh_rows.hip) with the 64 staged rows used as 32 frames twice: rows 0..31 are
// the frames f0 .. f0+31 of body A (the ground truth), rows 32..63 the same frames of body B (the estimate), each body
// with its own features, bone transforms and translations.  The K loop is the original's -- fp32 matrix cores, packed
// coefficient tiles from L2 through the five-slot ring -- and since the accumulator layout puts frame
// (r & 3) + 8 (r >> 2) + 4 (lane >> 5) of vertex lane & 31 into element r of acc[0] and of acc[1], a lane holds the same
// (frame, vertex) of A and of B.  It skins both in registers, keeps d = |v_A - v_B| and d^2, and no vertex is written:
// the 32 lanes of a half-wave are summed with one fixed exchange pattern (lane_reduce.h, the pairs of the xor butterfly
// 16, 8, 4, 2, 1) and every (frame, tile) gets one partial pair, part[frame][tile][2] -- 1.7 KB per frame at V = 6890
// against 166 KB for two meshes.  Lanes past V contribute an exact 0 (the packed tables are padded to whole tiles).
// mesh_err_sum_kernel adds a frame's tile partials in ascending tile order in double.  Every sum has one fixed order that
// involves nothing but its frame, so a frame's two numbers do not depend on T, on the frame's place in a block or slab,
// on the grid.y split or on the rest of the batch.
// The three-piece bf16 form of the contraction (mesh_x3.hip) is left out on purpose: this kernel stores partials between
// K loops, which is the situation DESIGN.md section 4 documents as corrupting a bf16 32x32x16 accumulator.
//
// The Procrustes-aligned error (PA-PVE: the same two sums after the similarity transform that best maps B onto A, the
// convention of PA-MPJPE in metrics.hip) is not a function of moments, so the bodies are evaluated twice, both times in
// registers -- the kernel has three modes (template parameter MODE, one K loop):
//   PLAIN    as above.
//   MOMENTS  as above, and per (frame, tile) the 17 sums the alignment needs, part_m[frame][tile][17]: a, b, a b^T, |a|^2,
//            |b|^2 with a = v_A - pivot_A, b = v_B - pivot_B.  The pivots are the posed root joints, which the chain has
//            written before the sweep: the alignment is translation invariant, and about the root the second moments stay
//            at the body's extent instead of its distance from the origin.  19 values x 16 frames do not fit a lane, so
//            they are not kept: the distances go the plain form's way (v[32], one reduce-scatter after the loop, the
//            same bits), and the 16 moments a .. |a|^2 of a frame are reduced as soon as they are formed (a
//            reduce-scatter of 16 values, 16 exchanges, one sum per lane pair, stored at once); |b|^2 is carried for four
//            frames and reduced four at a time (6 exchanges).  Same exchange pairs as the butterfly throughout.  The
//            280 further exchanges per tile are LDS-pipe instructions (ds_bpermute_b32) in a phase whose 428 16-byte
//            LDS reads already fill that pipe: the sweep takes 27 % longer than PLAIN; reducing two
//            frames at a time (31 exchanges in five dependent steps) changed nothing, so it is their number, not their
//            latency.  Open: the xor 16, 8, 2 and 1 steps as lane permutes and DPP moves, off the LDS pipe.
//   ALIGNED  stages the frame's 15 floats from mesh_pa_solve_kernel (M = sR, c_A, c_B) with the per-frame data and
//            reduces d = |(v_A - c_A) - (v_B - c_B) M| and d^2 exactly as PLAIN reduces its distances.  Its bone
//            transforms come from a float64 prologue (mesh_chain.hip launch_mesh_chain_f64: Rodrigues, rest joints and
//            chain in double, rounded once): with the float32 ones, which MOMENTS needs for the plain columns' bits, the
//            aligned sums carried the float32 rotations' and rest joints' error, three times what is left without it.
//            The sum of squares is stationary in the alignment, so moments of the float32 vertices serve.
// mesh_pa_solve_kernel, one lane per frame in float64, adds the tile partials in ascending order, centres and normalises
// them and runs the 3 x 3 alignment of the joints (svd3.h).  No atomics; plain vector stores only.
// Registers, four-bone forms (hipcc -Rpass-analysis=kernel-resource-usage): PLAIN and ALIGNED 242 VGPRs, nothing spilled;
// MOMENTS 256 VGPRs with 8 spilled -- store offsets written once ahead of the tile loop and read back in the skinning
// phase, six reads per tile; its K loop touches no scratch memory.
#include <hip/hip_runtime.h>

#include "gemm_epilogue.h"
#include "lane_reduce.h"
#include "launch.h"
#include "mesh_kernels.h"
#include "smpl_kernels.h"
#include "svd3.h"

namespace empose {

typedef float f32x2 __attribute__((ext_vector_type(2)));

namespace me {
constexpr int BF = 32;              // frames per workgroup
constexpr int BM = 2 * BF;          // staged rows: the frames of A, then of B
constexpr int NW = 8;               // waves per workgroup
constexpr int K = 200, KG = K / 8;  // 25 k-groups of 8
constexpr int LDA = K + 4;
constexpr int RING = 5;             // KG % RING == 0: a k-group's ring slot does not depend on the tile
constexpr int A_FLOATS = BM * LDA;
constexpr int XF_FLOATS = BM * NB * 12;
constexpr int TR_FLOATS = BM * 4;
constexpr int PV_FLOATS = BF * 16;   // per frame: the two pivots (MOMENTS) or the alignment (ALIGNED)
constexpr size_t LDS_BYTES = (size_t)(A_FLOATS + XF_FLOATS + TR_FLOATS + PV_FLOATS) * sizeof(float) + 64;
constexpr int TILE_FLOATS = KG * 3 * 256;   // one 32-vertex tile of the packed coefficients
static_assert(KG % RING == 0, "ring slots must line up across tiles");
}  // namespace me

#define ME_SGB(mask, n) __builtin_amdgcn_sched_group_barrier(mask, n, 0);
#define ME_MFMA 0x008
#define ME_VMEM_RD 0x020
#define ME_DS_RD 0x100

// EXTRA: body models with more than four bones per vertex (not SMPL-H).  That form spills registers in its skinning phase
// (the run-time bone loop sits inside the unrolled pairs while the ring, the accumulators and the 32 distances are
// live); its K loop and the whole of the four-bone form do not.
template <bool EXTRA, int MODE>
__global__ __launch_bounds__(me::NW * 64) void mesh_pair_error_kernel(MeshPairErrorArgs a) {
  using namespace me;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* As = lds;
  float* XFs = lds + A_FLOATS;
  float* TRs = XFs + XF_FLOATS;
  float* PVs = TRs + TR_FLOATS;
  const int T = a.T, V = a.V;
  const int f0 = blockIdx.x * BF;
  const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, lh = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

  // ---- staging: features, relative transforms and translations of the block's frames, body A then body B (frames
  // past T repeat frame T-1; their results are never stored)
  {
    for (int i = tid; i < BM * (K / 4); i += NW * 64) {
      const int r = i / (K / 4), c = (i % (K / 4)) * 4;
      const int fr = f0 + (r & (BF - 1)), row = fr < T ? fr : T - 1;
      const float* __restrict__ feat = r < BF ? a.feat_a : a.feat_b;
      *reinterpret_cast<f32x4*>(As + r * LDA + c) = *reinterpret_cast<const f32x4*>(feat + (size_t)row * K + c);
    }
    if (tid < BM) *reinterpret_cast<f32x4*>(As + tid * LDA + K) = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int i = tid; i < BM * NB * 3; i += NW * 64) {
      const int r = i / (NB * 3), c = i % (NB * 3);
      const int fr = f0 + (r & (BF - 1)), row = fr < T ? fr : T - 1;
      const float* __restrict__ xf = r < BF ? a.xf_a : a.xf_b;
      *reinterpret_cast<f32x4*>(XFs + i * 4) = *reinterpret_cast<const f32x4*>(xf + ((size_t)row * NB * 3 + c) * 4);
    }
    if (tid < BM) {
      const int fr = f0 + (tid & (BF - 1)), row = fr < T ? fr : T - 1;
      const float* __restrict__ trans = tid < BF ? a.trans_a : a.trans_b;
      f32x4 t{0.f, 0.f, 0.f, 0.f};
      if (trans) { t[0] = trans[(size_t)row * 3]; t[1] = trans[(size_t)row * 3 + 1]; t[2] = trans[(size_t)row * 3 + 2]; }
      *reinterpret_cast<f32x4*>(TRs + tid * 4) = t;
    }
    if (MODE == MESH_PAIR_MOMENTS && tid < BM) {   // frame r: floats 0..2 the pivot of A, 4..6 that of B
      const int fr = f0 + (tid & (BF - 1)), row = fr < T ? fr : T - 1;
      const float* __restrict__ pv = (tid < BF ? a.pivot_a : a.pivot_b) + (size_t)row * a.ld_pivot;
      *reinterpret_cast<f32x4*>(PVs + (tid & (BF - 1)) * 16 + (tid < BF ? 0 : 4)) = f32x4{pv[0], pv[1], pv[2], 0.f};
    }
    if (MODE == MESH_PAIR_ALIGNED && tid < BF * 4) {
      const int fr = f0 + (tid >> 2), row = fr < T ? fr : T - 1;
      *reinterpret_cast<f32x4*>(PVs + tid * 4) =
          *reinterpret_cast<const f32x4*>(a.align + (size_t)row * MESH_PA_ALIGN + (tid & 3) * 4);
    }
  }
  __syncthreads();

  // ---- this wave's tiles: vt = first + wave, + NW, ... below `end` (no barrier follows: a wave without a tile leaves)
  const int n_tiles = (V + 31) / 32;
  const int per_block = (n_tiles + gridDim.y - 1) / gridDim.y;
  const int first = blockIdx.y * per_block;
  const int end = min(first + per_block, n_tiles);
  int vt = first + wave;
  if (vt >= end) return;

  epi_cgbyte_t wbase = (epi_cgbyte_t)a.wc_frag;
  const unsigned lane16 = (unsigned)lane * 16u;
  auto tile_base = [&](int t) { return wbase + (size_t)t * (TILE_FLOATS * 4); };
  auto bload = [&](f32x4 (&dst)[3], epi_cgbyte_t base, int g) {
#pragma unroll
    for (int c = 0; c < 3; ++c)
      dst[c] = *(const __attribute__((address_space(1))) f32x4*)(base + ((unsigned)((g * 3 + c) * 1024) + lane16));
  };

  f32x4 ring[RING][3];
  {
    epi_cgbyte_t b0 = tile_base(vt);
#pragma unroll
    for (int g = 0; g < RING - 1; ++g) bload(ring[g], b0, g);
  }

  const float* a_lane = As + l31 * LDA + lh * 4;
  // A fragments: read one k-group ahead into three slots (k-groups u = 0..4 of a ring pass use slots 0,1,0,1,2, so the
  // slot being filled is never the one being consumed although a pass has an odd number of k-groups)
#define ME_FA_SLOT(u) ((u) == RING - 1 ? 2 : ((u) & 1))
  f32x4 fa[3][2];
  fa[0][0] = *reinterpret_cast<const f32x4*>(a_lane);
  fa[0][1] = *reinterpret_cast<const f32x4*>(a_lane + 32 * LDA);
  const int kb = a.kb;
  float* __restrict__ part = a.part;
  epi_gfloat_t pm_block = (epi_gfloat_t)(a.part_m + (size_t)f0 * ((V + 31) / 32) * MESH_PA_MOMENTS);   // MOMENTS

  for (; vt < end; vt += NW) {
    epi_cgbyte_t bcur = tile_base(vt);
    // the prefetch runs into the wave's next tile; past the last one it re-reads this tile (never consumed)
    epi_cgbyte_t bnext = vt + NW < end ? tile_base(vt + NW) : bcur;
    const int s = vt * 32 + l31;            // this lane's vertex (the packed tables are padded to whole tiles)
    const int4 bone4 = *reinterpret_cast<const int4*>(a.skin_idx4 + (size_t)s * 4);
    const f32x4 w4 = *reinterpret_cast<const f32x4*>(a.skin_w4 + (size_t)s * 4);

    f32x16 acc[2][3];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][c][r] = 0.f;

#pragma unroll 1
    for (int g0 = 0; g0 < KG; g0 += RING) {
#pragma unroll
      for (int u = 0; u < RING; ++u) {
        const int g = g0 + u;
        {
          // A fragments of the next k-group (k-group 0 again after the last one: the next tile starts there)
          const int gn = g + 1 < KG ? g + 1 : 0;
          f32x4 (&fn)[2] = fa[u + 1 == RING ? 0 : ME_FA_SLOT(u + 1)];
          fn[0] = *reinterpret_cast<const f32x4*>(a_lane + gn * 8);
          fn[1] = *reinterpret_cast<const f32x4*>(a_lane + 32 * LDA + gn * 8);
          const int gp = g + RING - 1;   // k-group to prefetch: this tile's, or the first ones of the next tile
          epi_cgbyte_t src = gp < KG ? bcur : bnext - (size_t)KG * 3 * 1024;
          bload(ring[(u + RING - 1) % RING], src, gp);
        }
        const f32x4 (&fc)[2] = fa[ME_FA_SLOT(u)];
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int c = 0; c < 3; ++c)
              acc[i][c] = __builtin_amdgcn_mfma_f32_32x32x2f32(fc[i][e], ring[u][c][e], acc[i][c], 0, 0, 0);
        // 24 MFMAs with the two fragment reads and the three weight loads spread between them
        ME_SGB(ME_MFMA, 2) ME_SGB(ME_DS_RD, 1) ME_SGB(ME_MFMA, 2) ME_SGB(ME_DS_RD, 1)
        ME_SGB(ME_MFMA, 2) ME_SGB(ME_VMEM_RD, 1) ME_SGB(ME_MFMA, 2) ME_SGB(ME_VMEM_RD, 1)
        ME_SGB(ME_MFMA, 2) ME_SGB(ME_VMEM_RD, 1) ME_SGB(ME_MFMA, 14)
      }
    }

    // ---- skinning of the lane's 16 (frame, vertex) pairs of both bodies (as mesh_rows_kernel: blended 3x4 transform,
    // then one mat-vec, reference order T = sum_k w_k G_k, v = T . [v_posed, 1] + trans), then their distance.  Every
    // lane takes part -- the exchange below needs all 32 of a half-wave -- and a lane past V, whose padded tables are
    // zeros, has its distances replaced by an exact 0.
    const bool live = s < V;
    const size_t sx = (size_t)(live ? s : 0) * kb;   // skin_idx / skin_w are not padded: a lane past V reads vertex 0's
    const char* xfl = reinterpret_cast<const char*>(XFs) + lh * (4 * NB * 48);
    const char* xk[4] = {xfl + bone4.x * 48, xfl + bone4.y * 48, xfl + bone4.z * 48, xfl + bone4.w * 48};
    const f32x2 wp[4] = {{w4[0], w4[0]}, {w4[1], w4[1]}, {w4[2], w4[2]}, {w4[3], w4[3]}};
    const char* trl = reinterpret_cast<const char*>(TRs) + lh * 64;
    const char* pvl = reinterpret_cast<const char*>(PVs) + lh * 256;
    float v[32];   // [0..15]: d of accumulator element r, [16..31]: d^2
    float w[4];    // MOMENTS: |b|^2 of four consecutive accumulator elements
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float out[2][3];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int dm = i * BF + (r & 3) + 8 * (r >> 2);   // staged row, less 4 * lh: body i, frame (r & 3) + 8 (r >> 2)
        const float vx = acc[i][0][r], vy = acc[i][1][r], vz = acc[i][2][r];
        const f32x4 tr = *reinterpret_cast<const f32x4*>(trl + dm * 16);
#pragma unroll
        for (int row = 0; row < 3; ++row) {
          // (T0, T1) and (T2, T3) as register pairs: two packed FMAs per bone on the halves of the 16-byte read
          f32x4 gk = *reinterpret_cast<const f32x4*>(xk[0] + dm * (NB * 48) + row * 16);
          f32x2 Ta = wp[0] * f32x2{gk[0], gk[1]}, Tb = wp[0] * f32x2{gk[2], gk[3]};
#pragma unroll
          for (int k = 1; k < 4; ++k) {
            gk = *reinterpret_cast<const f32x4*>(xk[k] + dm * (NB * 48) + row * 16);
            Ta = __builtin_elementwise_fma(wp[k], f32x2{gk[0], gk[1]}, Ta);
            Tb = __builtin_elementwise_fma(wp[k], f32x2{gk[2], gk[3]}, Tb);
          }
          if (EXTRA)
            for (int k = 4; k < kb; ++k) {
              const int b = a.skin_idx[sx + k];
              const float wk = a.skin_w[sx + k];
              gk = *reinterpret_cast<const f32x4*>(xfl + b * 48 + dm * (NB * 48) + row * 16);
              Ta = __builtin_elementwise_fma(f32x2{wk, wk}, f32x2{gk[0], gk[1]}, Ta);
              Tb = __builtin_elementwise_fma(f32x2{wk, wk}, f32x2{gk[2], gk[3]}, Tb);
            }
          out[i][row] = __builtin_fmaf(Ta[0], vx, __builtin_fmaf(Ta[1], vy, __builtin_fmaf(Tb[0], vz, Tb[1]))) + tr[row];
        }
      }
      float d2;
      if (MODE == MESH_PAIR_ALIGNED) {
        // the frame's alignment: e_A - e_B M with e = v - c, M = sR as the joints' alignment applies it (row vector times M)
        const char* al = pvl + ((r & 3) + 8 * (r >> 2)) * 64;
        const f32x4 q0 = *reinterpret_cast<const f32x4*>(al), q1 = *reinterpret_cast<const f32x4*>(al + 16),
                    q2 = *reinterpret_cast<const f32x4*>(al + 32), q3 = *reinterpret_cast<const f32x4*>(al + 48);
        const float ax = out[0][0] - q2[1], ay = out[0][1] - q2[2], az = out[0][2] - q2[3];
        const float bx = out[1][0] - q3[0], by = out[1][1] - q3[1], bz = out[1][2] - q3[2];
        const float dx = ax - __builtin_fmaf(bz, q1[2], __builtin_fmaf(by, q0[3], bx * q0[0]));
        const float dy = ay - __builtin_fmaf(bz, q1[3], __builtin_fmaf(by, q1[0], bx * q0[1]));
        const float dz = az - __builtin_fmaf(bz, q2[0], __builtin_fmaf(by, q1[1], bx * q0[2]));
        d2 = __builtin_fmaf(dx, dx, __builtin_fmaf(dy, dy, dz * dz));
      } else {
        const float dx = out[0][0] - out[1][0], dy = out[0][1] - out[1][1], dz = out[0][2] - out[1][2];
        d2 = __builtin_fmaf(dx, dx, __builtin_fmaf(dy, dy, dz * dz));
      }
      v[r] = live ? __builtin_sqrtf(d2) : 0.f;
      v[16 + r] = live ? d2 : 0.f;
      if (MODE == MESH_PAIR_MOMENTS) {
        // the frame's 16 moments a, b, a b^T, |a|^2 about the pivots, summed over the half-wave at once: 16 values in,
        // one per lane pair out (16 exchanges), stored and gone before the next frame's are formed
        const char* pl = pvl + ((r & 3) + 8 * (r >> 2)) * 64;
        const f32x4 pa = *reinterpret_cast<const f32x4*>(pl), pb = *reinterpret_cast<const f32x4*>(pl + 16);
        const float av[3] = {out[0][0] - pa[0], out[0][1] - pa[1], out[0][2] - pa[2]};
        const float bv[3] = {out[1][0] - pb[0], out[1][1] - pb[1], out[1][2] - pb[2]};
        float m[16];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          m[i] = live ? av[i] : 0.f;
          m[3 + i] = live ? bv[i] : 0.f;
#pragma unroll
          for (int k = 0; k < 3; ++k) m[6 + i * 3 + k] = live ? av[i] * bv[k] : 0.f;
        }
        m[15] = live ? __builtin_fmaf(av[0], av[0], __builtin_fmaf(av[1], av[1], av[2] * av[2])) : 0.f;
        w[r & 3] = live ? __builtin_fmaf(bv[0], bv[0], __builtin_fmaf(bv[1], bv[1], bv[2] * bv[2])) : 0.f;
        int mb = 0, mc = 0;
        LaneReduceScatter<16, 16, 16>::run(m, lane, mb, mc);
        // (a 32-bit offset from the block's rows: the frame's part is wave-uniform but for lh, nothing to keep per frame)
        const int fl = 4 * lh + (r & 3) + 8 * (r >> 2);
        if (f0 + fl < T && !(lane & 1)) pm_block[(unsigned)((fl * n_tiles + vt) * MESH_PA_MOMENTS + mb)] = m[0];
        if ((r & 3) == 3) {   // the 17th, |b|^2, every four frames: four values in, sum `wb` out (6 exchanges)
          int wb = 0, wc = 0;
          LaneReduceScatter<4, 16, 4>::run(w, lane, wb, wc);
          const int fw = 4 * lh + wb + 8 * (r >> 2);
          if (f0 + fw < T && !(lane & 7)) pm_block[(unsigned)((fw * n_tiles + vt) * MESH_PA_MOMENTS + 16)] = w[0];
        }
      }
    }
    // ---- the 32 sums over the vertex lanes of each half-wave: afterwards a lane holds one of them, sum `base`
    int base = 0, count = 0;
    LaneReduceScatter<32, 16, 32>::run(v, lane, base, count);
    {
      const int r = base & 15;
      const int frame = f0 + 4 * lh + (r & 3) + 8 * (r >> 2);
      if (frame < T) {
        epi_gfloat_t o = (epi_gfloat_t)(part + ((size_t)frame * n_tiles + vt) * 2 + (base >> 4));
        *o = v[0];
      }
    }
  }
}

// One thread per frame: the frame's tile partials in ascending tile order, in double.
__global__ __launch_bounds__(256) void mesh_err_sum_kernel(const float* __restrict__ part, int n_tiles, int T,
                                                           double* __restrict__ out, int ld_out) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= T) return;
  const f32x2* __restrict__ p = reinterpret_cast<const f32x2*>(part) + (size_t)t * n_tiles;
  double s1 = 0.0, s2 = 0.0;
  for (int i = 0; i < n_tiles; ++i) {
    const f32x2 x = p[i];
    s1 += (double)x[0];
    s2 += (double)x[1];
  }
  out[(size_t)t * ld_out] = s1;
  out[(size_t)t * ld_out + 1] = s2;
}

// One lane per frame, float64 (mesh_kernels.h MeshPaSolveArgs).  With n = V points and the sums about the pivots:
// mean = S / n, X0^T Y0 = S_ab - S_a S_b^T / n, |X0|^2 = S_aa - |S_a|^2 / n -- the pivots keep S_ab and S_aa at the
// body's extent, so the subtraction costs no digits -- then the alignment of the joints (svd3.h).
__global__ __launch_bounds__(64) void mesh_pa_solve_kernel(MeshPaSolveArgs a) {
  const int t = blockIdx.x * 64 + threadIdx.x;
  if (t >= a.T) return;
  const int n_tiles = (a.V + 31) / 32;
  const float* __restrict__ p = a.part + (size_t)t * n_tiles * 2;
  const float* __restrict__ pm = a.part_m + (size_t)t * n_tiles * MESH_PA_MOMENTS;
  double s1 = 0.0, s2 = 0.0, S[MESH_PA_MOMENTS];
  for (int k = 0; k < MESH_PA_MOMENTS; ++k) S[k] = 0.0;
  for (int i = 0; i < n_tiles; ++i) {
    s1 += (double)p[i * 2];
    s2 += (double)p[i * 2 + 1];
#pragma unroll
    for (int k = 0; k < MESH_PA_MOMENTS; ++k) S[k] += (double)pm[i * MESH_PA_MOMENTS + k];
  }
  a.sums[(size_t)t * 4] = s1;
  a.sums[(size_t)t * 4 + 1] = s2;
  const double n = (double)a.V;
  double A[9], ssX = S[15], ssY = S[16];
  for (int i = 0; i < 3; ++i) {
    ssX -= S[i] * S[i] / n;
    ssY -= S[3 + i] * S[3 + i] / n;
    for (int k = 0; k < 3; ++k) A[i * 3 + k] = S[6 + i * 3 + k] - S[i] * S[3 + k] / n;
  }
  const double normX = sqrt(ssX), normY = sqrt(ssY);
  for (int i = 0; i < 9; ++i) A[i] /= (normX * normY);
  double Tm[9];
  const double scale = normX * procrustes_rotation(A, Tm) / normY;
  float* __restrict__ o = a.align + (size_t)t * MESH_PA_ALIGN;
  for (int i = 0; i < 9; ++i) o[i] = (float)(scale * Tm[i]);
  for (int c = 0; c < 3; ++c) {
    o[9 + c] = (float)((double)a.pivot_a[(size_t)t * a.ld_pivot + c] + S[c] / n);
    o[12 + c] = (float)((double)a.pivot_b[(size_t)t * a.ld_pivot + c] + S[3 + c] / n);
  }
  o[15] = 0.f;
}

hipError_t launch_mesh_pair_error(const MeshPairErrorArgs& a, hipStream_t stream) {
  const int bx = (a.T + me::BF - 1) / me::BF;
  const int n_tiles = (a.V + 31) / 32;
  if (a.T <= 0 || n_tiles <= 0) return hipErrorInvalidValue;
  // fewer than one workgroup per CU: split the mesh's tiles over grid.y (at least one tile per wave), as launch_mesh_rows
  int by = bx >= 256 ? 1 : (256 + bx - 1) / bx;
  const int max_by = (n_tiles + me::NW - 1) / me::NW;
  if (by > max_by) by = max_by;
  const dim3 grid(bx, by), block(me::NW * 64);
  const bool extra = a.kb > 4;
  switch (a.mode) {
    case MESH_PAIR_PLAIN:
      return extra ? launch_lds(mesh_pair_error_kernel<true, MESH_PAIR_PLAIN>, grid, block, me::LDS_BYTES, stream, a)
                   : launch_lds(mesh_pair_error_kernel<false, MESH_PAIR_PLAIN>, grid, block, me::LDS_BYTES, stream, a);
    case MESH_PAIR_MOMENTS:
      if (!a.pivot_a || !a.pivot_b || a.ld_pivot < 3 || !a.part_m) return hipErrorInvalidValue;
      return extra ? launch_lds(mesh_pair_error_kernel<true, MESH_PAIR_MOMENTS>, grid, block, me::LDS_BYTES, stream, a)
                   : launch_lds(mesh_pair_error_kernel<false, MESH_PAIR_MOMENTS>, grid, block, me::LDS_BYTES, stream, a);
    case MESH_PAIR_ALIGNED:
      if (!a.align) return hipErrorInvalidValue;
      return extra ? launch_lds(mesh_pair_error_kernel<true, MESH_PAIR_ALIGNED>, grid, block, me::LDS_BYTES, stream, a)
                   : launch_lds(mesh_pair_error_kernel<false, MESH_PAIR_ALIGNED>, grid, block, me::LDS_BYTES, stream, a);
  }
  return hipErrorInvalidValue;
}

hipError_t launch_mesh_err_sum(const float* part, int n_tiles, int T, double* out, hipStream_t stream, int ld_out) {
  if (T <= 0 || n_tiles <= 0 || ld_out < 2) return hipErrorInvalidValue;
  hipLaunchKernelGGL(mesh_err_sum_kernel, dim3((T + 255) / 256), dim3(256), 0, stream, part, n_tiles, T, out, ld_out);
  return hipGetLastError();
}

hipError_t launch_mesh_pa_solve(const MeshPaSolveArgs& a, hipStream_t stream) {
  if (a.T <= 0 || a.V <= 0 || a.ld_pivot < 3) return hipErrorInvalidValue;
  hipLaunchKernelGGL(mesh_pa_solve_kernel, dim3((a.T + 63) / 64), dim3(64), 0, stream, a);
  return hipGetLastError();
}

}  // namespace empose
