// SMPL-H on the sensor sub-mesh, general path: everything of one body-model evaluation between the two blend products.
//
//   chain_sensors  22-joint kinematic chain, linear blend skinning of the ~84 needed vertices, vertex normals and
//                  sensor frames (reference virtual_sensors.py:16-38, utils.py:126-146), sensor offsets
//                  (reference models.py:478-479), the reconstruction residual (reference loss.py:23-41) and its
//                  hand-derived reverse pass down to d v_posed, d J and d R (oracle/analytic_np.py is the blueprint)
//
// chain_sensors runs a small tile of frames per workgroup; all per-frame state (rotations, rest joints, global
// transforms, skinned vertices and their cotangents, per-bone force/moment sums) lives in LDS and every phase is a
// flat parallel-for over (frame, item) so that no lane idles on the serial structure of the skeleton: the forward
// chain is a per-(joint,row) walk down the root path, the reverse chain uses the world-space form
// dR_j = G_p^T (sum_subtree M_b - F_b (x) t_j) G_j, which needs subtree sums instead of a level-by-level sweep.
#include "launch.h"
#include "smpl_kernels.h"
#include "smpl_math.h"

namespace empose {

// ---------------------------------------------------------------------------------------------------------------
// chain + skinning + sensors (+ reverse)
//
// Workgroup = CH_FRAMES frames.  Phase list (each a flat parallel-for over (frame, item), barrier in between):
//   P0  stage the packed index/weight tables (once per block) and each frame's rot | out row into LDS
//   P2  forward chain: (joint,row) walks the root path given as a bit mask (joints are topologically ordered)
//   P3  skinning of the needed vertices
//   P4a face normals, one (sensor,face) per lane      P4b per sensor: normal sum (in face order, as the reference),
//       frame, offsets, outputs, residual and its reverse down to (d centre, d helper, d face-normal)
//   P4c per (sensor,face): d e1, d e2                 P4d per vertex coordinate: gather its incident contributions
//   P5  d v_posed -> global;  per-bone force/moment partial sums over chunks of <= 16 (vertex,weight) pairs
//   P5c combine chunks per bone                       P6 subtree sums (bit mask)      P7 d R, d J -> global
// Every accumulation is a gather in a fixed order: results are bitwise reproducible and independent of the batch.
// ---------------------------------------------------------------------------------------------------------------
// Two shapes of the workgroup, picked by the launch (launch_chain_sensors): 4 frames on 256 threads from 4096 frames up
// (the 24 KB of tables are staged once per four frames and the narrow phases fill more lanes: 231 us against 253 for the
// other shape at T = 32768, 126 against 137 at 16384, 69 against 74 at 8192; whole forwards at 128 / 256 / 512 windows
// 1-2 % faster), 2 frames on 192 threads below (twice as many workgroups for the short launches of the streaming drivers).
// Measured and rejected: 3 x 192 (236), 3 x 256 (241), 4 x 192 (257), 4 x 224 (243), 5 x 256 (261), 8 x 512 (255),
// anything with more than 256 threads per workgroup (320-390 us: the register budget halves).

// (frame, item) of flat index i < FR * n without an integer division (n is a run-time value in most phases, and
// a division costs ~25 instructions in a kernel whose limit is instruction issue).
template <int FR>
__device__ __forceinline__ void frame_split_t(int i, int n, int& f, int& o) {
  static_assert(FR >= 1 && FR <= 8, "a chain of compares");
  f = 0;
#pragma unroll
  for (int k = 1; k < FR; ++k) f += i >= k * n ? 1 : 0;
  o = i - f * n;
}
constexpr int CHUNK = CHAIN_CHUNK;  // (vertex, weight) pairs per partial-sum chunk, lists padded with weight 0

size_t chain_lds_bytes(const SmplTables& tab, int frames_per_block) {
  const ChainLds l = chain_layout(tab.nv, tab.ncp, tab.max_deg, tab.n_chunks);
  return ((size_t)l.total * frames_per_block + ((tab.off.total + 3) & ~3)) * sizeof(float);
}

#ifdef EMPOSE_CHAIN_TRACE   // dev build only (scripts/dev/chain_trace.sh): shader-clock stamps of two blocks per phase
__device__ long long g_chain_trace[2][32];
#define CH_STAMP(i) \
  if (threadIdx.x == 0 && (blockIdx.x == 0 || blockIdx.x == 9000)) g_chain_trace[blockIdx.x != 0][(i)] = clock64();
#else
#define CH_STAMP(i)
#endif

template <int CH_FRAMES, int CH_THREADS>
__global__ __launch_bounds__(CH_THREADS) void chain_sensors_kernel(ChainArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  auto frame_split = [](int i, int n, int& f, int& o) { frame_split_t<CH_FRAMES>(i, n, f, o); };
  CH_STAMP(0)
  const SmplTables& tb = a.tab;
  const ChainTabs& O = tb.off;
  const ChainLds L = chain_layout(tb.nv, tb.ncp, tb.max_deg, tb.n_chunks);
  const int tid = threadIdx.x;
  const int t0 = blockIdx.x * CH_FRAMES;
  const int nf = min(CH_FRAMES, a.T - t0);
  const int nv3 = tb.nv * 3;
  const int md = tb.max_deg;
  const uint32_t md_magic = 65536u / (uint32_t)md + 1u;   // floor(x * magic / 65536) == x / md for x < 12 * md (md <= 64)
  const bool cot = a.cot_pos != nullptr;          // external cotangents (training) instead of the residual
  const bool bwd = a.tgt != nullptr || cot;
  float* frames = smem;
  const uint32_t* TI = reinterpret_cast<const uint32_t*>(smem + (size_t)L.total * CH_FRAMES);  // tables (ints)
  const float* TF = reinterpret_cast<const float*>(TI);                                        // tables (floats)

  // ---- P0: tables + per-frame rot | out.  Every global load of the phase (16-byte pieces of the table blob, the
  // frames' rot | out rows) is issued before the first LDS store, so the phase costs one round trip instead of one per
  // copy-loop iteration; tables or frame rows larger than one batch fall through to the batched loops below.
  {
    uint4* dst = reinterpret_cast<uint4*>(smem + (size_t)L.total * CH_FRAMES);
    const uint4* src = reinterpret_cast<const uint4*>(tb.blob);
    const int n16 = (O.total + 3) >> 2;   // the blob is padded to a multiple of 4 words
    const int row = NB * 9 + tb.ncp;
    const int n = nf * row;
    // 8 x 192 x 16 B = 24 KB of tables; CH_FRAMES frames x (198 + ncp ~ 320) floats over the workgroup's threads
    constexpr int TB = (8 * 192 + CH_THREADS - 1) / CH_THREADS, FB = (CH_FRAMES * 520 + CH_THREADS - 1) / CH_THREADS;
    auto frame_src = [&](int i) -> float {
      int f, o;
      frame_split(i, row, f, o);
      return o < NB * 9 ? a.rot[(size_t)(t0 + f) * (NB * 9) + o] : a.out[(size_t)(t0 + f) * tb.ncp + (o - NB * 9)];
    };
    auto frame_dst = [&](int i, float v) {
      int f, o;
      frame_split(i, row, f, o);
      frames[f * L.total + (o < NB * 9 ? L.rot + o : L.out + (o - NB * 9))] = v;
    };
    uint4 tv[TB];
    float fv[FB];
#pragma unroll
    for (int u = 0; u < TB; ++u) { const int i = tid + u * CH_THREADS; tv[u] = i < n16 ? src[i] : uint4{0u, 0u, 0u, 0u}; }
#pragma unroll
    for (int u = 0; u < FB; ++u) { const int i = tid + u * CH_THREADS; fv[u] = i < n ? frame_src(i) : 0.f; }
#pragma unroll
    for (int u = 0; u < TB; ++u) { const int i = tid + u * CH_THREADS; if (i < n16) dst[i] = tv[u]; }
#pragma unroll
    for (int u = 0; u < FB; ++u) { const int i = tid + u * CH_THREADS; if (i < n) frame_dst(i, fv[u]); }
    for (int i0 = tid + TB * CH_THREADS; i0 < n16; i0 += TB * CH_THREADS) {
#pragma unroll
      for (int u = 0; u < TB; ++u) { const int i = i0 + u * CH_THREADS; tv[u] = i < n16 ? src[i] : uint4{0u, 0u, 0u, 0u}; }
#pragma unroll
      for (int u = 0; u < TB; ++u) { const int i = i0 + u * CH_THREADS; if (i < n16) dst[i] = tv[u]; }
    }
    for (int i0 = tid + FB * CH_THREADS; i0 < n; i0 += FB * CH_THREADS) {
#pragma unroll
      for (int u = 0; u < FB; ++u) { const int i = i0 + u * CH_THREADS; fv[u] = i < n ? frame_src(i) : 0.f; }
#pragma unroll
      for (int u = 0; u < FB; ++u) { const int i = i0 + u * CH_THREADS; if (i < n) frame_dst(i, fv[u]); }
    }
  }
  __syncthreads();
  CH_STAMP(1)

  // ---- P2: forward chain
  for (int i = tid; i < nf * NB * 3; i += CH_THREADS) {
    int f, jr;
    frame_split(i, NB * 3, f, jr);
    const int j = jr / 3, r = jr % 3;
    float* S = frames + f * L.total;
    const float* sR = S + L.rot;
    const float* sJ = S + L.out + tb.j_off;
    float row0 = sR[r * 3 + 0], row1 = sR[r * 3 + 1], row2 = sR[r * 3 + 2];  // root rotation, row r
    float tr = sJ[r];
    int prev = 0;
    uint32_t pm = TI[O.path_mask + j] & ~1u;
    while (pm) {
      const int q = __ffs(pm) - 1;
      pm &= pm - 1;
      const float* Jq = sJ + q * 3;
      const float* Jp = sJ + prev * 3;
      tr = row0 * (Jq[0] - Jp[0]) + row1 * (Jq[1] - Jp[1]) + row2 * (Jq[2] - Jp[2]) + tr;
      const float* Rq = sR + q * 9;
      const float n0 = row0 * Rq[0] + row1 * Rq[3] + row2 * Rq[6];
      const float n1 = row0 * Rq[1] + row1 * Rq[4] + row2 * Rq[7];
      const float n2 = row0 * Rq[2] + row1 * Rq[5] + row2 * Rq[8];
      row0 = n0; row1 = n1; row2 = n2;
      prev = q;
    }
    float* G = S + L.g + j * 12;
    G[r * 3 + 0] = row0; G[r * 3 + 1] = row1; G[r * 3 + 2] = row2;
    G[9 + r] = tr;
    const float* Jj = sJ + j * 3;
    S[L.at + j * 3 + r] = tr - (row0 * Jj[0] + row1 * Jj[1] + row2 * Jj[2]);
    const size_t go = (size_t)(t0 + f) * 66 + j * 3 + r;
    a.joints[go] = tr;
    if (a.joints2) a.joints2[go] = tr;
  }
  __syncthreads();
  CH_STAMP(2)

  // ---- P3: linear blend skinning of the needed vertices, one (vertex, coordinate) per lane
  for (int i = tid; i < nf * nv3; i += CH_THREADS) {
    int f, sr;
    frame_split(i, nv3, f, sr);
    const int s = sr / 3, r = sr % 3;
    float* S = frames + f * L.total;
    const float* vp = S + L.out + s * 3;
    float T0 = 0.f, T1 = 0.f, T2 = 0.f, T3 = 0.f;  // row r of the blended 3x4 transform
#pragma unroll 4
    for (int k = 0; k < tb.kb; ++k) {  // padding entries have weight 0 / bone 0: no branch, loads can be batched
      const float w = TF[O.skin_w + s * tb.kb + k];
      const int b = TI[O.skin_idx + s * tb.kb + k];
      const float* G = S + L.g + b * 12 + r * 3;
      T0 += w * G[0]; T1 += w * G[1]; T2 += w * G[2];
      T3 += w * S[L.at + b * 3 + r];
    }
    S[L.v + sr] = T0 * vp[0] + T1 * vp[1] + T2 * vp[2] + T3;
  }
  __syncthreads();
  CH_STAMP(3)

  // ---- P4a: un-normalised face normals
  for (int i = tid; i < nf * 12 * md; i += CH_THREADS) {
    int f, mk;
    frame_split(i, 12 * md, f, mk);
    float* S = frames + f * L.total;
    const float* V = S + L.v;
    const uint32_t* fc = TI + O.s_faces + mk * 3;  // padding faces are (c,c,c): zero normal, zero cotangent
    const float* v0 = V + fc[0] * 3;
    const float* v1 = V + fc[1] * 3;
    const float* v2 = V + fc[2] * 3;
    const float e1[3] = {v1[0] - v0[0], v1[1] - v0[1], v1[2] - v0[2]};
    const float e2[3] = {v2[0] - v0[0], v2[1] - v0[1], v2[2] - v0[2]};
    cross3(e1, e2, S + L.fn + mk * 3);
  }
  __syncthreads();
  CH_STAMP(4)

  // ---- P4b: per sensor
  for (int i = tid; i < nf * 12; i += CH_THREADS) {
    int f, m;
    frame_split(i, 12, f, m);
    const int t = t0 + f;
    float* S = frames + f * L.total;
    const float* V = S + L.v;
    const int c = TI[O.s_center + m], h = TI[O.s_helper + m], deg = TI[O.s_deg + m];
    // Everything this sensor reads from global memory is requested up front: the stores of pos / ori further down
    // would otherwise sit between two dependent round trips (offsets, then targets).
    const int w = t / a.F;
    float Ro[9], to[3];
    {
      const float* pr = a.offset_r + ((size_t)w * 12 + m) * 9;
      const float* pt = a.offset_t + ((size_t)w * 12 + m) * 3;
#pragma unroll
      for (int k = 0; k < 9; ++k) Ro[k] = pr[k];
#pragma unroll
      for (int k = 0; k < 3; ++k) to[k] = pt[k];
    }
    const int slot_m = a.used_slot[m];
    float tp[3] = {0.f, 0.f, 0.f}, tori[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, scale = 0.f;
    if (bwd && !cot && slot_m >= 0) {
      const float* p3 = a.tgt + (size_t)t * a.ld_tgt + slot_m * 3;
      const float* p9 = a.tgt + (size_t)t * a.ld_tgt + a.n_markers * 3 + slot_m * 9;
#pragma unroll
      for (int k = 0; k < 3; ++k) tp[k] = p3[k];
#pragma unroll
      for (int k = 0; k < 9; ++k) tori[k] = p9[k];
      scale = a.frame_scale[t];
    }
    float n[3] = {0.f, 0.f, 0.f};
    for (int k = 0; k < deg; ++k) {
      const float* fn = S + L.fn + (m * md + k) * 3;
      n[0] += fn[0]; n[1] += fn[1]; n[2] += fn[2];
    }
    // One (IEEE) reciprocal per normalisation, then multiplications: the per-sensor arithmetic runs on 24 of the 192
    // lanes, so its instruction count is the phase's latency.
    const float inv_deg = 1.f / (float)deg;
    n[0] *= inv_deg; n[1] *= inv_deg; n[2] *= inv_deg;
    const float inv_nn = 1.f / norm3(n);
    const float nh[3] = {n[0] * inv_nn, n[1] * inv_nn, n[2] * inv_nn};
    const float* vc = V + c * 3;
    const float* vh = V + h * 3;
    const float e[3] = {vh[0] - vc[0], vh[1] - vc[1], vh[2] - vc[2]};
    const float inv_ne = 1.f / norm3(e);
    const float sv[3] = {e[0] * inv_ne, e[1] * inv_ne, e[2] * inv_ne};
    float bb[3];
    cross3(nh, sv, bb);
    const float inv_nb = 1.f / norm3(bb);
    const float tv[3] = {bb[0] * inv_nb, bb[1] * inv_nb, bb[2] * inv_nb};
    float aa[3];
    cross3(tv, nh, aa);
    const float inv_na = 1.f / norm3(aa);
    const float s2[3] = {aa[0] * inv_na, aa[1] * inv_na, aa[2] * inv_na};
    // R_m columns (s2, tv, nh)
    const float Rm[9] = {s2[0], tv[0], nh[0], s2[1], tv[1], nh[1], s2[2], tv[2], nh[2]};
    float ori[9], pos[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
      for (int cc = 0; cc < 3; ++cc)
        ori[r * 3 + cc] = Rm[r * 3 + 0] * Ro[cc] + Rm[r * 3 + 1] * Ro[3 + cc] + Rm[r * 3 + 2] * Ro[6 + cc];
      pos[r] = vc[r] + (Rm[r * 3 + 0] * to[0] + Rm[r * 3 + 1] * to[1] + Rm[r * 3 + 2] * to[2]);
    }
    {
      float* po = a.pos + ((size_t)t * 12 + m) * 3;
      float* oo = a.ori + ((size_t)t * 12 + m) * 9;
      po[0] = pos[0]; po[1] = pos[1]; po[2] = pos[2];
#pragma unroll
      for (int k = 0; k < 9; ++k) oo[k] = ori[k];
      if (a.pos2) {
        float* p2 = a.pos2 + ((size_t)t * 12 + m) * 3;
        float* o2 = a.ori2 + ((size_t)t * 12 + m) * 9;
        p2[0] = pos[0]; p2[1] = pos[1]; p2[2] = pos[2];
#pragma unroll
        for (int k = 0; k < 9; ++k) o2[k] = ori[k];
      }
    }
    if (!bwd) continue;
    float* scr = S + L.scr + m * 9;  // d face-normal (3) | d centre (3) | d helper (3)
    float dpos[3], dori[9];
    if (cot) {
      const float* cp = a.cot_pos + ((size_t)t * 12 + m) * 3;
      const float* co = a.cot_ori + ((size_t)t * 12 + m) * 9;
      dpos[0] = cp[0]; dpos[1] = cp[1]; dpos[2] = cp[2];
#pragma unroll
      for (int k = 0; k < 9; ++k) dori[k] = co[k];
    } else {
      if (slot_m < 0 || scale == 0.f) {
#pragma unroll
        for (int k = 0; k < 9; ++k) scr[k] = 0.f;
        continue;
      }
      const float r0 = pos[0] - tp[0], r1 = pos[1] - tp[1], r2 = pos[2] - tp[2];
      const float sp = scale / sqrtf(r0 * r0 + r1 * r1 + r2 * r2);
      dpos[0] = r0 * sp; dpos[1] = r1 * sp; dpos[2] = r2 * sp;
      float q = 0.f;
#pragma unroll
      for (int k = 0; k < 9; ++k) { dori[k] = ori[k] - tori[k]; q += dori[k] * dori[k]; }
      const float so = scale / sqrtf(q);
#pragma unroll
      for (int k = 0; k < 9; ++k) dori[k] *= so;
    }
    // dR_m = dori Ro^T + dpos (x) to
    float dRm[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int cc = 0; cc < 3; ++cc)
        dRm[r * 3 + cc] = dori[r * 3 + 0] * Ro[cc * 3 + 0] + dori[r * 3 + 1] * Ro[cc * 3 + 1] +
                          dori[r * 3 + 2] * Ro[cc * 3 + 2] + dpos[r] * to[cc];
    float ds2[3] = {dRm[0], dRm[3], dRm[6]};
    float dt[3] = {dRm[1], dRm[4], dRm[7]};
    float dnh[3] = {dRm[2], dRm[5], dRm[8]};
    float da[3], tmp[3];
    unit_bwd(ds2, s2, inv_na, da);   // a = t x nh
    cross3(nh, da, tmp); dt[0] += tmp[0]; dt[1] += tmp[1]; dt[2] += tmp[2];
    cross3(da, tv, tmp); dnh[0] += tmp[0]; dnh[1] += tmp[1]; dnh[2] += tmp[2];
    float db[3];
    unit_bwd(dt, tv, inv_nb, db);    // b = nh x s
    cross3(sv, db, tmp); dnh[0] += tmp[0]; dnh[1] += tmp[1]; dnh[2] += tmp[2];
    float dsv[3];
    cross3(db, nh, dsv);
    float de[3];
    unit_bwd(dsv, sv, inv_ne, de);
    float dn[3];
    unit_bwd(dnh, nh, inv_nn, dn);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      scr[k] = dn[k] * inv_deg;
      scr[3 + k] = dpos[k] - de[k];
      scr[6 + k] = de[k];
    }
  }
  if (!bwd) return;
  __syncthreads();
  CH_STAMP(5)

  // ---- P4c: per (sensor, face): cotangents of the two edge vectors
  for (int i = tid; i < nf * 12 * md; i += CH_THREADS) {
    int f, mk;
    frame_split(i, 12 * md, f, mk);
    const int m = (int)(((uint32_t)mk * md_magic) >> 16);   // mk / md for mk < 12 * md <= 4096
    float* S = frames + f * L.total;
    const float* V = S + L.v;
    const uint32_t* fc = TI + O.s_faces + mk * 3;
    const float* v0 = V + fc[0] * 3;
    const float* v1 = V + fc[1] * 3;
    const float* v2 = V + fc[2] * 3;
    const float e1[3] = {v1[0] - v0[0], v1[1] - v0[1], v1[2] - v0[2]};
    const float e2[3] = {v2[0] - v0[0], v2[1] - v0[1], v2[2] - v0[2]};
    const float* dfn = S + L.scr + m * 9;
    float* fg = S + L.fg + mk * 6;
    cross3(e2, dfn, fg);      // d e1
    cross3(dfn, e1, fg + 3);  // d e2
  }
  __syncthreads();
  CH_STAMP(6)

  // ---- P4d: gather the vertex cotangents (fixed order => deterministic).  Every incidence is one packed word
  // (a:13 | b:13 | use_b:1 | negate:1 | null:1, offsets into the frame's LDS record): contribution = +-(S[a+r] + S[b+r]);
  // lists are padded to a multiple of 4 with null words, so four independent LDS round trips are in flight.
  for (int i = tid; i < nf * nv3; i += CH_THREADS) {
    int f, sr;
    frame_split(i, nv3, f, sr);
    const int s = sr / 3, r = sr % 3;
    float* S = frames + f * L.total;
    float acc = 0.f;
    const int q0 = TI[O.inc_ptr + s], q1 = TI[O.inc_ptr + s + 1];
    for (int q = q0; q < q1; q += 4) {
      uint32_t code[4];
      float x[4], y[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) code[u] = TI[O.inc_code + q + u];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        x[u] = S[(code[u] & 0x1fffu) + r];
        y[u] = S[((code[u] >> 13) & 0x1fffu) + r];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float v = x[u] + ((code[u] >> 26) & 1u ? y[u] : 0.f);
        const float sg = (code[u] >> 28) & 1u ? 0.f : ((code[u] >> 27) & 1u ? -1.f : 1.f);
        acc += sg * v;
      }
    }
    S[L.dv + sr] = acc;
  }
  __syncthreads();
  CH_STAMP(7)

  // ---- P5: d v_posed (to global) and per-chunk force / world-space moment partial sums
  for (int i = tid; i < nf * tb.ncp; i += CH_THREADS) {
    int f, col;
    frame_split(i, tb.ncp, f, col);
    if (col >= tb.j_off && col < tb.j_off + NB * 3) continue;  // d J is written in P7
    float acc = 0.f;
    if (col < nv3) {
      const int s = col / 3, cc = col % 3;
      const float* S = frames + f * L.total;
      const float* dv = S + L.dv + s * 3;
#pragma unroll 4
      for (int k = 0; k < tb.kb; ++k) {
        const float w = TF[O.skin_w + s * tb.kb + k];
        const float* G = S + L.g + TI[O.skin_idx + s * tb.kb + k] * 12;
        acc += w * (G[0 + cc] * dv[0] + G[3 + cc] * dv[1] + G[6 + cc] * dv[2]);
      }
    }
    a.d_out[(size_t)(t0 + f) * tb.ncp + col] = acc;
  }
  for (int i = tid; i < nf * tb.n_chunks; i += CH_THREADS) {
    int f, ch;
    frame_split(i, tb.n_chunks, f, ch);
    float* S = frames + f * L.total;
    const int b = TI[O.chunk_bone + ch];
    const int q0 = TI[O.chunk_beg + ch];
    float G[12];
#pragma unroll
    for (int k = 0; k < 9; ++k) G[k] = S[L.g + b * 12 + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) G[9 + k] = S[L.at + b * 3 + k];
    float acc[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) acc[k] = 0.f;
#pragma unroll
    for (int q = 0; q < CHUNK; ++q) {  // chunks are padded to CHUNK pairs with weight 0
      const int sidx = TI[O.bone_vert + q0 + q];
      const float wq = TF[O.bone_w + q0 + q];
      const float* vp = S + L.out + sidx * 3;
      const float* dv = S + L.dv + sidx * 3;
      const float d0 = wq * dv[0], d1 = wq * dv[1], d2 = wq * dv[2];
      const float x0 = G[0] * vp[0] + G[1] * vp[1] + G[2] * vp[2] + G[9];
      const float x1 = G[3] * vp[0] + G[4] * vp[1] + G[5] * vp[2] + G[10];
      const float x2 = G[6] * vp[0] + G[7] * vp[1] + G[8] * vp[2] + G[11];
      acc[0] += d0 * x0; acc[1] += d0 * x1; acc[2] += d0 * x2;
      acc[3] += d1 * x0; acc[4] += d1 * x1; acc[5] += d1 * x2;
      acc[6] += d2 * x0; acc[7] += d2 * x1; acc[8] += d2 * x2;
      acc[9] += d0; acc[10] += d1; acc[11] += d2;
    }
#pragma unroll
    for (int k = 0; k < 12; ++k) S[L.part + ch * 12 + k] = acc[k];
  }
  __syncthreads();
  CH_STAMP(8)

  // ---- P5c: per bone: sum its chunks (chunks of a bone are contiguous)
  for (int i = tid; i < nf * NB * 12; i += CH_THREADS) {
    int f, be;
    frame_split(i, NB * 12, f, be);
    const int b = be / 12, e = be % 12;
    float* S = frames + f * L.total;
    float acc = 0.f;
    for (int ch = TI[O.bone_chunk_ptr + b]; ch < (int)TI[O.bone_chunk_ptr + b + 1]; ++ch) acc += S[L.part + ch * 12 + e];
    if (a.cot_joints) {
      // joint j (position G_j^t) moves rigidly with its parent's frame: force d_j at point t_j on bone parent(j)
      const float* dj = a.cot_joints + (size_t)(t0 + f) * 66;
      for (int j = 1; j < NB; ++j) {
        if ((int)TI[O.parents + j] != b) continue;
        if (e < 9) acc += dj[j * 3 + e / 3] * S[L.g + j * 12 + 9 + e % 3];
        else acc += dj[j * 3 + (e - 9)];
      }
    }
    S[L.m + (int)TI[O.dfs_pos + b] * 12 + e] = acc;   // stored in depth-first order for the prefix sums below
  }
  __syncthreads();
  CH_STAMP(9)

  // ---- P6: subtree sums  X_j = sum_sub M_b - Fs_j (x) t_j.  With the bones in depth-first pre-order a subtree is a
  // contiguous range, so the sum is a difference of two prefix sums; the prefix runs in fp64 (22 additions per lane), so
  // the difference, rounded once to fp32, is the correctly rounded subtree sum.
  for (int i = tid; i < nf * 12; i += CH_THREADS) {
    int f, e;
    frame_split(i, 12, f, e);
    float* S = frames + f * L.total;
    double* P = reinterpret_cast<double*>(S + L.pd);
    float mv[NB];
#pragma unroll
    for (int k = 0; k < NB; ++k) mv[k] = S[L.m + k * 12 + e];
    double run = 0.0;
    P[e] = 0.0;
#pragma unroll
    for (int k = 0; k < NB; ++k) { run += (double)mv[k]; P[(k + 1) * 12 + e] = run; }
  }
  __syncthreads();
  for (int i = tid; i < nf * NB * 12; i += CH_THREADS) {
    int f, je;
    frame_split(i, NB * 12, f, je);
    const int j = je / 12, e = je % 12;
    float* S = frames + f * L.total;
    const double* P = reinterpret_cast<const double*>(S + L.pd);
    const int p0 = TI[O.dfs_pos + j], p1 = p0 + (int)TI[O.sub_size + j];
    const int ar = e < 9 ? e / 3 : e - 9, cc = e % 3;
    const float fs = (float)(P[p1 * 12 + 9 + ar] - P[p0 * 12 + 9 + ar]);
    if (e < 9) {
      const float ms = (float)(P[p1 * 12 + e] - P[p0 * 12 + e]);
      S[L.x + je] = ms - fs * S[L.g + j * 12 + 9 + cc];
    } else {
      S[L.x + je] = fs;
    }
  }
  __syncthreads();
  CH_STAMP(10)

  // ---- P7: d R_j = G_p^T X_j G_j  and  d J_j = (G_p - G_j)^T Fs_j
  for (int i = tid; i < nf * NB * 12; i += CH_THREADS) {
    int f, je;
    frame_split(i, NB * 12, f, je);
    const int j = je / 12, e = je % 12;
    const float* S = frames + f * L.total;
    const float* Gj = S + L.g + j * 12;
    const float* X = S + L.x + j * 12;
    const int p = (int)TI[O.parents + j];
    const float* Gp = S + L.g + (p < 0 ? 0 : p) * 12;
    if (e < 9) {
      const int r = e / 3, cc = e % 3;
      float acc = 0.f;
#pragma unroll
      for (int ar = 0; ar < 3; ++ar) {
        const float xg = X[ar * 3 + 0] * Gj[0 + cc] + X[ar * 3 + 1] * Gj[3 + cc] + X[ar * 3 + 2] * Gj[6 + cc];
        const float gp = p < 0 ? (ar == r ? 1.f : 0.f) : Gp[ar * 3 + r];
        acc += gp * xg;
      }
      a.d_rot[((size_t)(t0 + f) * NB + j) * 9 + e] = acc;
    } else {
      const int cc = e - 9;
      float acc = 0.f;
#pragma unroll
      for (int ar = 0; ar < 3; ++ar) {
        const float gp = p < 0 ? (ar == cc ? 1.f : 0.f) : Gp[ar * 3 + cc];
        acc += (gp - Gj[ar * 3 + cc]) * X[9 + ar];
        if (a.cot_joints) acc += gp * a.cot_joints[(size_t)(t0 + f) * 66 + j * 3 + ar];
      }
      a.d_out[(size_t)(t0 + f) * tb.ncp + tb.j_off + j * 3 + cc] = acc;
    }
  }
  CH_STAMP(11)
}

template <int FR, int NT>
static hipError_t launch_chain_cfg(const ChainArgs& a, hipStream_t stream) {
  const size_t lds = chain_lds_bytes(a.tab, FR);
  const int blocks = (a.T + FR - 1) / FR;
  return launch_lds(chain_sensors_kernel<FR, NT>, dim3(blocks), dim3(NT), lds, stream, a);
}

hipError_t launch_chain_sensors(const ChainArgs& a, hipStream_t stream) {
  if (a.T >= 4096 && chain_lds_bytes(a.tab, 4) <= 64 * 1024) return launch_chain_cfg<4, 256>(a, stream);
  return launch_chain_cfg<2, 192>(a, stream);
}

}  // namespace empose

#ifdef EMPOSE_CHAIN_TRACE
extern "C" int empose_debug_chain_trace(long long* out) {
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(empose::g_chain_trace), sizeof(long long) * 64);
}
#endif
