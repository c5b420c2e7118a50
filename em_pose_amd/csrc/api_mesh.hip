// C ABI (include/empose_hip.h), full mesh: packing and evaluation of the posed vertices and joints, the metrics rows,
// the virtual sensors and the root normalisation.
#include "api_internal.h"
#include "data_kernels.h"
#include "gemm_kernels.h"
#include "mesh_kernels.h"
#include "options.h"
#include "smpl_kernels.h"

#include <algorithm>

using namespace empose;
using namespace empose::api;

struct empose_mesh {
  std::vector<void*> allocs;
  int V = 0, j_off = 0, ncp = 0, kb = 0;
  int n_joints = 22;            // posed joints returned (22 body, or all 52 of SMPL-H)
  int rod_conv = 0;             // EMPOSE_RODRIGUES_*
  float* wc = nullptr;
  float* wc_frag = nullptr;     // vertex rows of wc in matrix-core fragment order, per 32-vertex tile (mesh_rows.hip)
  int* skin_idx = nullptr;
  float* skin_w = nullptr;
  int* skin_idx4 = nullptr;     // first four bones / weights per vertex, padded to whole tiles
  float* skin_w4 = nullptr;
  int* parents = nullptr;
  unsigned short* wc_bf16 = nullptr;   // split-bf16 pieces of wc in fragment order (only when the handle asked for them)
  unsigned short* wc_x3 = nullptr;     // three bf16 pieces of wc in fragment order (mesh_x3.hip), kb <= 4
  unsigned short* skin_bf16 = nullptr; // dense skin weights per 32-vertex tile, bf16 hi + lo, B-fragment order (ditto)
  float* wc_vjp = nullptr;      // vertex rows of wc in the VJP feat sweep's B-fragment order (mesh_vjp.hip)
  float* skin_dense = nullptr;  // dense skin weights per tile in the VJP bone sweep's B-fragment order (ditto)
  float* wj_t = nullptr;        // rest-joint rows of wc transposed: [200][jw4], the reverse of the rest-joint gemm
  int jw4 = 0;                  // ncp - j_off rounded up to 4
};

namespace {

// Tables of mesh_rows_kernel: for every 32-vertex tile, k-group of 8 and coordinate c, lane (v = lane & 31,
// half = lane >> 5) owns wc[(tile * 32 + v) * 3 + c][kg * 8 + half * 4 .. + 3] -- the three coordinate planes of a tile
// are separate 32-column operands, so a lane's accumulators hold x, y and z of the same vertex.  Vertices past V are
// zero.  Skinning tables: the first four (bone, weight) pairs per vertex, zero-padded.
int pack_mesh_tiles(empose_mesh* m, const empose_mesh_desc* d) {
  const int V = d->n_vertices, NT = (V + 31) / 32, KG = 25, K = 200;
  std::vector<float> buf((size_t)NT * KG * 3 * 256, 0.f);
  for (int t = 0; t < NT; ++t)
    for (int kg = 0; kg < KG; ++kg)
      for (int c = 0; c < 3; ++c)
        for (int lane = 0; lane < 64; ++lane) {
          const int v = t * 32 + (lane & 31);
          if (v >= V) continue;
          const float* src = d->wc + ((size_t)v * 3 + c) * K + kg * 8 + (lane >> 5) * 4;
          float* dst = &buf[((((size_t)t * KG + kg) * 3 + c) * 64 + lane) * 4];
          for (int e = 0; e < 4; ++e) dst[e] = src[e];
        }
  TRY(upload(m->allocs, buf.data(), buf.size(), &m->wc_frag));
  std::vector<int> idx4((size_t)NT * 32 * 4, 0);
  std::vector<float> w4((size_t)NT * 32 * 4, 0.f);
  for (int v = 0; v < V; ++v)
    for (int k = 0; k < 4 && k < d->kb; ++k) {
      idx4[(size_t)v * 4 + k] = d->skin_idx[(size_t)v * d->kb + k];
      w4[(size_t)v * 4 + k] = d->skin_w[(size_t)v * d->kb + k];
    }
  TRY(upload(m->allocs, idx4.data(), idx4.size(), &m->skin_idx4));
  TRY(upload(m->allocs, w4.data(), w4.size(), &m->skin_w4));
  return EMPOSE_OK;
}

// Tables of mesh_rows_x3_kernel (mesh_x3.hip): per 32-vertex tile, k-step of 16, coordinate plane c and piece p one
// fragment of 1 KB -- lane (v = lane & 31, half = lane >> 5) owns the eight values k = kstep * 16 + half * 8 .. + 7 of
// row (tile * 32 + v) * 3 + c, as piece p of their three-piece bf16 split (bf16x3.h); k >= 200 and vertices past V are zero.
int pack_mesh_tiles_x3(empose_mesh* m, const empose_mesh_desc* d) {
  const int V = d->n_vertices, NT = (V + 31) / 32, K = 200, KS = 13;
  static_assert(MESH_X3_TILE_BYTES == KS * 3 * 3 * 1024, "a tile is [k-step][plane] fragments of three pieces");
  return upload_bf16(m->allocs, pack_fragments_x3((size_t)NT * KS * 3, K, [&](size_t f, int lane, const float** row, int* k0) {
    const int c = (int)(f % 3), ks = (int)(f / 3 % KS), v = (int)(f / 3 / KS) * 32 + (lane & 31);
    if (v >= V) return false;
    *row = d->wc + ((size_t)v * 3 + c) * K;
    *k0 = ks * 16 + (lane >> 5) * 8;
    return true;
  }), &m->wc_x3);
}

// Tables of mesh_rows_bf16_kernel: per 32-vertex tile, k-step of 16, coordinate plane and (hi, lo) piece, lane
// (v = lane & 31, half = lane >> 5) owns the eight values k = kstep * 16 + half * 8 .. + 7 of row (tile * 32 + v) * 3 + c.
// Columns (mesh_bf16.hip): 0..188 pose, (hi, lo) = (w0, w1); 189..199 shape/template, (b0, b2); 200..210 the same
// coefficients again, (b1, b0); zero up to 223.
int pack_mesh_tiles_bf16(empose_mesh* m, const empose_mesh_desc* d) {
  const int V = d->n_vertices, NT = (V + 31) / 32, K = 200, KS = 14;
  const size_t tile_shorts = MESH_BF16_TILE_BYTES / 2;
  std::vector<unsigned short> buf((size_t)NT * tile_shorts, 0);
  for (int t = 0; t < NT; ++t)
    for (int lane = 0; lane < 64; ++lane) {
      const int v = t * 32 + (lane & 31), half = lane >> 5;
      if (v >= V) continue;
      for (int c = 0; c < 3; ++c) {
        const float* row = d->wc + ((size_t)v * 3 + c) * K;
        for (int ks = 0; ks < KS; ++ks)
          for (int e = 0; e < 8; ++e) {
            const int k = ks * 16 + half * 8 + e;
            if (k >= 211) continue;
            unsigned short p[3];
            split3(row[k < 200 ? k : k - 11], p);
            unsigned short* dst = &buf[(size_t)t * tile_shorts + ((size_t)((ks * 3 + c) * 2) * 64 + lane) * 8 + e];
            dst[0] = k < 200 ? p[0] : p[1];                            // hi: w0 | b0 | b1
            dst[64 * 8] = k < 189 ? p[1] : (k < 200 ? p[2] : p[0]);    // lo: w1 | b2 | b0
          }
      }
    }
  TRY(upload_bf16(m->allocs, buf, &m->wc_bf16));
  // The skin weights as a dense [32 bone slots][32 vertices] block per tile for the bone blend on the matrix cores
  // (mesh_bf16.hip mesh_rows_bf16s_kernel): k-step ks, piece p, lane (vertex = lane & 31, half = lane >> 5) holds the eight
  // weights of bones 16 ks + 8 half + 0..7 -- hi = bf16(w), lo = bf16(w - hi); bones a vertex does not have, and the
  // slots past the 22 body bones, are zero.  Weights of the same bone listed twice add up.
  {
    const size_t tile = MESH_SKIN_BF16_TILE_BYTES / 2;
    std::vector<unsigned short> sk((size_t)NT * tile, 0);
    std::vector<float> dense(32);
    for (int t = 0; t < NT; ++t)
      for (int lane = 0; lane < 64; ++lane) {
        const int v = t * 32 + (lane & 31), half = lane >> 5;
        if (v >= V) continue;
        std::fill(dense.begin(), dense.end(), 0.f);
        for (int k = 0; k < d->kb; ++k) {
          const int b = d->skin_idx[(size_t)v * d->kb + k];
          if (b < 0 || b >= NB) return fail(EMPOSE_EINVAL, "skin index %d of vertex %d outside the %d body bones", b, v, NB);
          dense[b] += d->skin_w[(size_t)v * d->kb + k];
        }
        for (int ks = 0; ks < 2; ++ks)
          for (int e = 0; e < 8; ++e) {
            unsigned short p[3];   // hi, lo: the first two pieces
            split3(dense[ks * 16 + half * 8 + e], p);
            unsigned short* dst = &sk[(size_t)t * tile + ((size_t)(ks * 2) * 64 + lane) * 8 + e];
            dst[0] = p[0];
            dst[64 * 8] = p[1];
          }
      }
    TRY(upload_bf16(m->allocs, sk, &m->skin_bf16));
  }
  return EMPOSE_OK;
}

// Tables of the vector-Jacobian product (mesh_vjp.hip, api: empose_mesh_vjp), packed with the handle:
//   wc_vjp     per tile, vertex pair p (vertices p and 16 + p), q < 6, lane (j = lane & 31, h = lane >> 5), e < 4: the
//              entry q * 4 + e = c * 8 + ct is wc[(tile * 32 + 16 h + p) * 3 + c][ct * 32 + j] (ct = 7, features past 200
//              and vertices past V: zero)
//   skin_dense per tile, q < 4, lane (j, h), e < 4: the summed weight of bone j at vertex tile * 32 + e + 8 q + 4 h; slots
//              past the 22 bones zero
//   wj_t       [200][jw4]: wj_t[k][i] = wc[j_off + i][k], zero for i >= ncp - j_off
int pack_mesh_vjp(empose_mesh* m, const empose_mesh_desc* d) {
  const int V = d->n_vertices, NT = (V + 31) / 32, K = 200;
  std::vector<float> wv((size_t)NT * MESH_VJP_WC_TILE_FLOATS, 0.f);
  for (int t = 0; t < NT; ++t)
    for (int p = 0; p < 16; ++p)
      for (int q = 0; q < 6; ++q)
        for (int lane = 0; lane < 64; ++lane)
          for (int e = 0; e < 4; ++e) {
            const int idx = q * 4 + e, c = idx / 8, ct = idx % 8, col = ct * 32 + (lane & 31);
            const int v = t * 32 + 16 * (lane >> 5) + p;
            if (ct == 7 || col >= K || v >= V) continue;
            wv[(size_t)t * MESH_VJP_WC_TILE_FLOATS + (((size_t)p * 6 + q) * 64 + lane) * 4 + e] =
                d->wc[((size_t)v * 3 + c) * K + col];
          }
  TRY(upload(m->allocs, wv.data(), wv.size(), &m->wc_vjp));
  std::vector<float> sd((size_t)NT * MESH_VJP_SKIN_TILE_FLOATS, 0.f);
  for (int t = 0; t < NT; ++t)
    for (int q = 0; q < 4; ++q)
      for (int lane = 0; lane < 64; ++lane)
        for (int e = 0; e < 4; ++e) {
          const int v = t * 32 + e + 8 * q + 4 * (lane >> 5), j = lane & 31;
          if (v >= V) continue;
          float w = 0.f;
          for (int k = 0; k < d->kb && j < NB; ++k) {
            const int b = d->skin_idx[(size_t)v * d->kb + k];
            if (b < 0 || b >= NB) return fail(EMPOSE_EINVAL, "skin index %d of vertex %d outside the %d body bones", b, v, NB);
            if (b == j) w += d->skin_w[(size_t)v * d->kb + k];
          }
          sd[(size_t)t * MESH_VJP_SKIN_TILE_FLOATS + ((size_t)q * 64 + lane) * 4 + e] = w;
        }
  TRY(upload(m->allocs, sd.data(), sd.size(), &m->skin_dense));
  const int jw = d->ncp - d->j_off;
  m->jw4 = (jw + 3) / 4 * 4;
  std::vector<float> wj((size_t)K * m->jw4, 0.f);
  for (int k = 0; k < K; ++k)
    for (int i = 0; i < jw; ++i) wj[(size_t)k * m->jw4 + i] = d->wc[((size_t)d->j_off + i) * K + k];
  return upload(m->allocs, wj.data(), wj.size(), &m->wj_t);
}

const int MESH_SLAB = 16384;  // frames per pass: bounds the scratch (rot, feat, rest joints, transforms)

struct MeshWs { float *rot, *feat, *jrest, *xf; };
MeshWs carve_mesh(Carver& c, const empose_mesh* mesh, size_t S) {
  MeshWs w;
  w.rot = c.f(S * 198); w.feat = c.f(S * 200); w.jrest = c.f(S * (size_t)(mesh->ncp - mesh->j_off));
  w.xf = c.f(S * 264);
  return w;
}

// The forward prologue of the slab of n frames from t0: Rodrigues + feature row, rest joints (the joint rows of wc) and,
// when `joints` says where the posed joints go, the kinematic chain (all n_joints posed joints + the 22 skinning
// transforms in w.xf); `trans`: the slab's translations, or null when none applies.
int mesh_slab_prologue(const empose_mesh* mesh, const MeshWs& w, const float* poses, const float* betas, int t0, int n,
                       const float* trans, float* joints, hipStream_t stream) {
  const int jw = mesh->ncp - mesh->j_off;
  FeatArgs fa = plain_feat_args(poses + (size_t)t0 * 66, 66, betas + (size_t)t0 * 10, 10);
  fa.rot = w.rot; fa.feat = w.feat; fa.T = n; fa.F = 1; fa.rod_conv = mesh->rod_conv;
  HIP_CHECK(launch_update_feat(fa, stream), "update_feat kernel");
  GemmBatch b;
  b.count = 1;
  b.p[0] = plain_prob(w.feat, 200, mesh->wc + (size_t)mesh->j_off * 200, 200, w.jrest, jw, n, jw, 200);
  HIP_CHECK(launch_gemm(b, stream), "rest-joint gemm");
  if (!joints) return EMPOSE_OK;
  MeshChainArgs ca;
  ca.rot = w.rot; ca.out = w.jrest; ca.ncp = jw; ca.j_off = 0; ca.parents = mesh->parents;
  ca.trans = trans; ca.xf = w.xf; ca.joints = joints; ca.T = n; ca.n_joints = mesh->n_joints;
  HIP_CHECK(launch_mesh_chain(ca, stream), "mesh chain");
  return EMPOSE_OK;
}

// The three forward entry points, checked: slab by slab the prologue and, with `want_vertices`, the full-mesh kernel --
// the default arithmetic, or with `bf16x3` the two-piece bf16 variant.
int mesh_fwd(const empose_mesh_t* mesh, int T, const float* poses, const float* betas, const float* trans,
             bool want_vertices, float* vertices, float* joints, void* workspace, size_t workspace_bytes,
             empose_stream_t stream_, bool bf16x3) {
  if (!mesh || !poses || !betas || (want_vertices && !vertices) || !joints || !workspace)
    return fail(EMPOSE_EINVAL, "null argument");
  if (bf16x3 && !mesh->wc_bf16) return fail(EMPOSE_EINVAL, "the mesh handle was created without with_bf16x3");
  if (T <= 0) return fail(EMPOSE_EINVAL, "T must be positive");
  if (workspace_bytes < empose_mesh_workspace_bytes(mesh, T)) return fail(EMPOSE_ENOMEM, "workspace too small");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const int S = T < MESH_SLAB ? T : MESH_SLAB;
  Carver c(workspace);
  const MeshWs w = carve_mesh(c, mesh, (size_t)S);
  for (int t0 = 0; t0 < T; t0 += S) {
    const int n = (T - t0) < S ? (T - t0) : S;
    const float* tr = trans ? trans + (size_t)t0 * 3 : nullptr;
    TRY(mesh_slab_prologue(mesh, w, poses, betas, t0, n, tr, joints + (size_t)t0 * mesh->n_joints * 3, stream));
    if (!want_vertices) continue;
    MeshSkinArgs sa;
    sa.feat = w.feat; sa.wc = mesh->wc; sa.xf = w.xf; sa.skin_idx = mesh->skin_idx; sa.skin_w = mesh->skin_w;
    sa.kb = mesh->kb; sa.trans = tr; sa.vertices = vertices + (size_t)t0 * mesh->V * 3; sa.T = n; sa.V = mesh->V;
    sa.wc_frag = mesh->wc_frag; sa.skin_idx4 = mesh->skin_idx4; sa.skin_w4 = mesh->skin_w4;
    sa.wc_bf16 = mesh->wc_bf16; sa.skin_bf16 = mesh->skin_bf16; sa.wc_x3 = mesh->wc_x3;
    // default: the three-piece bf16 contraction (fp32-equivalent); `bf16x3`: the explicitly selected two-piece variant
    hipError_t e;
    if (bf16x3)
      e = options().mesh_skin_mfma && mesh->skin_bf16 ? launch_mesh_rows_bf16s(sa, stream) : launch_mesh_rows_bf16(sa, stream);
    else if (options().mesh_x3 != 0 && mesh->wc_x3 && mesh->kb <= 4) {
      sa.stagger = options().mesh_x3 == 1;
      e = launch_mesh_rows_x3(sa, options().mesh_x3 == 3, stream);
    }
    else
      e = launch_mesh_rows(sa, stream);
    if (e != hipSuccess) return fail(EMPOSE_EHIP, "fused mesh kernel: %s", hipGetErrorString(e));
  }
  return EMPOSE_OK;
}

// Scratch of empose_mesh_vjp for a slab of S frames: the forward's, then the reverse's cotangents; `part` holds the
// per-slice partial sums of a vertex sweep split over grid.y (small slabs only).
struct MeshVjpWs { MeshWs f; float *dfeat_v, *dA, *part, *drot, *djrest, *dfeat; double* dtrans; };
size_t vjp_part_floats(const empose_mesh* mesh, int n) {
  if (n <= 0) return 0;
  const int sf = mesh_vjp_feat_split(n, mesh->V), sb = mesh_vjp_bone_split(n, mesh->V);
  return std::max(sf > 1 ? (size_t)sf * 200 : 0, sb > 1 ? (size_t)sb * MESH_VJP_DA : 0) * n;
}
MeshVjpWs carve_mesh_vjp(Carver& c, const empose_mesh* mesh, int T) {
  const int S = T < MESH_SLAB ? T : MESH_SLAB;
  MeshVjpWs w;
  w.f = carve_mesh(c, mesh, (size_t)S);
  w.dfeat_v = c.f((size_t)S * 200);
  w.dA = c.f((size_t)S * MESH_VJP_DA);
  // sized for the full slabs and for the last, shorter one (a smaller slab may split its sweeps further)
  const size_t part = std::max(vjp_part_floats(mesh, S), vjp_part_floats(mesh, T % S));
  w.part = part ? c.f(part) : nullptr;
  const int ns = std::max(mesh_vjp_feat_split(S, mesh->V), T % S ? mesh_vjp_feat_split(T % S, mesh->V) : 1);
  w.dtrans = reinterpret_cast<double*>(c.f((size_t)ns * S * 3 * 2));
  w.drot = c.f((size_t)S * NB * 9);
  w.djrest = c.f((size_t)S * mesh->jw4);
  w.dfeat = c.f((size_t)S * 200);
  return w;
}

}  // namespace

// Frames per pass of empose_virtual_sensors_vjp (and of empose_sample_sensors_vjp, api_sample.hip): the scratch (nine
// floats per frame and sensor) stays below 128 MB whatever T and M, and a slab never exceeds MESH_SLAB frames.
int empose::api::sensors_vjp_slab(int T, int M) {
  const size_t cap = ((size_t)128 << 20) / (sizeof(float) * SENSOR_VJP_ROW * (size_t)M);
  const size_t s = std::min<size_t>({(size_t)T, (size_t)MESH_SLAB, std::max<size_t>(cap, 1)});
  return (int)s;
}

extern "C" {

int empose_virtual_sensors_fwd(int T, int V, const float* vertices, int M, int max_deg, const int* center,
                               const int* helper, const int* deg, const int* faces, float* pos, float* ori,
                               float* normals, empose_stream_t stream_) {
  if (!vertices || !center || !helper || !deg || !faces || !pos || !ori) return fail(EMPOSE_EINVAL, "null argument");
  if (T <= 0 || V <= 0 || M <= 0 || max_deg <= 0) return fail(EMPOSE_EINVAL, "sizes must be positive");
  VirtualSensorArgs a;
  a.vertices = vertices; a.center = center; a.helper = helper; a.deg = deg; a.faces = faces;
  a.pos = pos; a.ori = ori; a.normals = normals; a.T = T; a.V = V; a.M = M; a.max_deg = max_deg;
  HIP_CHECK(launch_virtual_sensors(a, static_cast<hipStream_t>(stream_)), "virtual sensors kernel");
  return EMPOSE_OK;
}

// ---- virtual sensors: vector-Jacobian product --------------------------------------------------------------------
size_t empose_virtual_sensors_vjp_workspace_bytes(int T, int M) {
  if (T <= 0 || M <= 0) return 0;
  return Carver::measure([&](Carver& c) { c.f((size_t)sensors_vjp_slab(T, M) * M * SENSOR_VJP_ROW); });
}

int empose_virtual_sensors_vjp(int T, int V, const float* vertices, int M, int max_deg, const int* center,
                               const int* helper, const int* deg, const int* faces, int n_sub_faces,
                               const int* sub_faces, const int* face_ptr, const int* face_sensors, const int* vf_ptr,
                               const int* vf_corner, const int* vs_ptr, const int* vs_role, int n_touched,
                               const int* touched, const float* d_pos, const float* d_ori, const float* d_normals,
                               float* d_vertices, void* workspace, size_t workspace_bytes, empose_stream_t stream_) {
  if (!vertices || !center || !helper || !deg || !faces || !sub_faces || !face_ptr || !face_sensors || !vf_ptr ||
      !vf_corner || !vs_ptr || !vs_role || !touched || !d_vertices)
    return fail(EMPOSE_EINVAL, "null argument");
  if (T <= 0 || V <= 0 || M <= 0 || max_deg <= 0 || n_sub_faces <= 0 || n_touched <= 0)
    return fail(EMPOSE_EINVAL, "sizes must be positive");
  if (!d_pos && !d_ori && !d_normals) return fail(EMPOSE_EINVAL, "d_pos, d_ori and d_normals are all NULL");
  if (!workspace || workspace_bytes < empose_virtual_sensors_vjp_workspace_bytes(T, M))
    return fail(EMPOSE_EINVAL, "workspace too small (empose_virtual_sensors_vjp_workspace_bytes)");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const int S = sensors_vjp_slab(T, M);
  SensorVjpArgs a;
  a.center = center; a.helper = helper; a.deg = deg; a.faces = faces;
  a.sub_faces = sub_faces; a.face_ptr = face_ptr; a.face_sensors = face_sensors;
  a.vf_ptr = vf_ptr; a.vf_corner = vf_corner; a.vs_ptr = vs_ptr; a.vs_role = vs_role;
  a.touched = touched; a.n_touched = n_touched;
  a.scratch = static_cast<float*>(workspace);
  a.V = V; a.M = M; a.max_deg = max_deg;
  for (int t0 = 0; t0 < T; t0 += S) {
    const size_t r = (size_t)t0 * M;
    a.T = (T - t0) < S ? (T - t0) : S;
    a.vertices = vertices + (size_t)t0 * V * 3;
    a.d_vertices = d_vertices + (size_t)t0 * V * 3;
    a.d_pos = d_pos ? d_pos + r * 3 : nullptr;
    a.d_ori = d_ori ? d_ori + r * 9 : nullptr;
    a.d_normals = d_normals ? d_normals + r * 3 : nullptr;
    HIP_CHECK(launch_sensors_vjp(a, stream), "virtual sensors VJP kernels");
  }
  return EMPOSE_OK;
}

int empose_metrics_rows(int T, const float* joints_gt, const float* joints_hat, const float* pose_gt,
                        const float* pose_hat, const int* parents_host, double* rows, empose_stream_t stream_) {
  if (!joints_gt || !joints_hat || !parents_host || !rows) return fail(EMPOSE_EINVAL, "null argument");
  if ((pose_gt == nullptr) != (pose_hat == nullptr)) return fail(EMPOSE_EINVAL, "pose_gt and pose_hat go together");
  if (T <= 0) return fail(EMPOSE_EINVAL, "T must be positive");
  MetricsArgs a;
  a.joints_gt = joints_gt; a.joints_hat = joints_hat; a.pose_gt = pose_gt; a.pose_hat = pose_hat; a.rows = rows; a.T = T;
  for (int j = 0; j < 22; ++j) {
    if (parents_host[j] >= j) return fail(EMPOSE_EINVAL, "parents must be topologically ordered");
    a.parents[j] = parents_host[j] < 0 ? 0 : parents_host[j];
  }
  HIP_CHECK(launch_metrics_rows(a, static_cast<hipStream_t>(stream_)), "metrics kernel");
  return EMPOSE_OK;
}

// ---- full mesh -----------------------------------------------------------------------------------------------
void empose_mesh_destroy(empose_mesh_t* mesh) {
  if (!mesh) return;
  for (void* p : mesh->allocs) (void)hipFree(p);
  delete mesh;
}

int empose_mesh_create(const empose_mesh_desc* d, empose_mesh_t** out) {
  if (!d || !out) return fail(EMPOSE_EINVAL, "null argument");
  *out = nullptr;
  const int nj = d->n_joints == 0 ? 22 : d->n_joints;
  if (nj < 22 || nj > MESH_MAX_JOINTS) return fail(EMPOSE_EINVAL, "n_joints must be in [22, %d]", MESH_MAX_JOINTS);
  if (d->rodrigues != EMPOSE_RODRIGUES_SMPLX && d->rodrigues != EMPOSE_RODRIGUES_SO3)
    return fail(EMPOSE_EINVAL, "unknown Rodrigues convention %d", d->rodrigues);
  if (d->n_vertices <= 0 || d->ncp % 4 != 0 || d->j_off != d->n_vertices * 3 || d->j_off + nj * 3 > d->ncp ||
      d->ncp - d->j_off > nj * 3 + 3 || d->kb <= 0 || !d->parents)
    return fail(EMPOSE_EINVAL, "inconsistent mesh table sizes");
  for (int j = 0; j < nj; ++j)
    if (d->parents[j] >= j || (j > 0 && d->parents[j] < 0))
      return fail(EMPOSE_EINVAL, "parents must be topologically ordered with a single root");
  empose_mesh* m = new empose_mesh();
  m->V = d->n_vertices; m->j_off = d->j_off; m->ncp = d->ncp; m->kb = d->kb;
  m->n_joints = nj; m->rod_conv = d->rodrigues;
  int rc;
  if ((rc = upload(m->allocs, d->wc, (size_t)d->ncp * 200, &m->wc)) ||
      (rc = upload(m->allocs, d->skin_idx, (size_t)d->n_vertices * d->kb, &m->skin_idx)) ||
      (rc = upload(m->allocs, d->skin_w, (size_t)d->n_vertices * d->kb, &m->skin_w)) ||
      (rc = upload(m->allocs, d->parents, (size_t)nj, &m->parents)) || (rc = pack_mesh_tiles(m, d)) ||
      (d->kb <= 4 && (rc = pack_mesh_tiles_x3(m, d))) ||
      (d->with_bf16x3 && (rc = pack_mesh_tiles_bf16(m, d))) || (rc = pack_mesh_vjp(m, d))) {
    empose_mesh_destroy(m);
    return rc;
  }
  *out = m;
  return EMPOSE_OK;
}

int empose_mesh_n_joints(const empose_mesh_t* mesh) { return mesh ? mesh->n_joints : 0; }

size_t empose_mesh_workspace_bytes(const empose_mesh_t* mesh, int T) {
  if (!mesh || T <= 0) return 0;
  return Carver::measure([&](Carver& c) { carve_mesh(c, mesh, T < MESH_SLAB ? T : MESH_SLAB); });
}

int empose_mesh_vertices_fwd(const empose_mesh_t* mesh, int T, const float* poses, const float* betas,
                             const float* trans, float* vertices, float* joints, void* workspace,
                             size_t workspace_bytes, empose_stream_t stream_) {
  return mesh_fwd(mesh, T, poses, betas, trans, true, vertices, joints, workspace, workspace_bytes, stream_, false);
}

int empose_mesh_vertices_fwd_bf16x3(const empose_mesh_t* mesh, int T, const float* poses, const float* betas,
                                    const float* trans, float* vertices, float* joints, void* workspace,
                                    size_t workspace_bytes, empose_stream_t stream_) {
  return mesh_fwd(mesh, T, poses, betas, trans, true, vertices, joints, workspace, workspace_bytes, stream_, true);
}

int empose_mesh_joints_fwd(const empose_mesh_t* mesh, int T, const float* poses, const float* betas,
                           const float* trans, float* joints, void* workspace, size_t workspace_bytes,
                           empose_stream_t stream_) {
  return mesh_fwd(mesh, T, poses, betas, trans, false, nullptr, joints, workspace, workspace_bytes, stream_, false);
}

// ---- full-mesh vector-Jacobian product -------------------------------------------------------------------------
size_t empose_mesh_vjp_workspace_bytes(const empose_mesh_t* mesh, int T) {
  if (!mesh || T <= 0) return 0;
  return Carver::measure([&](Carver& c) { carve_mesh_vjp(c, mesh, T); });
}

int empose_mesh_vjp(const empose_mesh_t* mesh, int T, const float* poses, const float* betas, const float* d_vertices,
                    const float* d_joints, float* g_poses, float* g_betas, float* g_trans, void* workspace,
                    size_t workspace_bytes, empose_stream_t stream_) {
  if (!mesh || !poses || !betas || !g_poses || !g_betas) return fail(EMPOSE_EINVAL, "null argument");
  if (T <= 0) return fail(EMPOSE_EINVAL, "T must be positive");
  if (!d_vertices && !d_joints) return fail(EMPOSE_EINVAL, "d_vertices and d_joints are both NULL");
  if (!workspace || workspace_bytes < empose_mesh_vjp_workspace_bytes(mesh, T))
    return fail(EMPOSE_EINVAL, "workspace too small (empose_mesh_vjp_workspace_bytes)");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const int S = T < MESH_SLAB ? T : MESH_SLAB;
  const int jw = mesh->ncp - mesh->j_off, nj = mesh->n_joints;
  Carver c(workspace);
  const MeshVjpWs w = carve_mesh_vjp(c, mesh, T);
  for (int t0 = 0; t0 < T; t0 += S) {
    const int n = (T - t0) < S ? (T - t0) : S;
    // the forward's rotations, features and rest joints, and for the vertex sweeps the transforms: their posed joints are
    // not needed and land in the reverse's scratch, which is written later
    const float* dv = d_vertices ? d_vertices + (size_t)t0 * mesh->V * 3 : nullptr;
    static_assert(MESH_MAX_JOINTS * 3 <= 200, "posed joints fit a feature row");
    TRY(mesh_slab_prologue(mesh, w.f, poses, betas, t0, n, nullptr, dv ? w.dfeat : nullptr, stream));
    if (dv) {
      MeshVjpArgs va;
      va.feat = w.f.feat; va.xf = w.f.xf; va.dv = dv;
      va.wc_frag = mesh->wc_frag; va.wc_vjp = mesh->wc_vjp; va.skin_dense = mesh->skin_dense;
      va.skin_idx4 = mesh->skin_idx4; va.skin_w4 = mesh->skin_w4; va.skin_idx = mesh->skin_idx; va.skin_w = mesh->skin_w;
      va.kb = mesh->kb; va.part = w.part; va.dtrans = w.dtrans; va.T = n; va.V = mesh->V;
      va.out = w.dfeat_v;
      HIP_CHECK(launch_mesh_vjp_feat(va, stream), "mesh VJP feat sweep");
      va.out = w.dA;
      HIP_CHECK(launch_mesh_vjp_bone(va, stream), "mesh VJP bone sweep");
    }
    MeshChainBwdArgs cb;
    cb.rot = w.f.rot; cb.jrest = w.f.jrest; cb.ld_j = jw; cb.parents = mesh->parents;
    cb.dA = dv ? w.dA : nullptr;
    cb.dtrans = dv ? w.dtrans : nullptr; cb.n_slices = mesh_vjp_feat_split(n, mesh->V);
    cb.dJ = d_joints ? d_joints + (size_t)t0 * nj * 3 : nullptr;
    cb.d_rot = w.drot; cb.d_jrest = w.djrest; cb.ld_dj = mesh->jw4;
    cb.g_trans = g_trans ? g_trans + (size_t)t0 * 3 : nullptr;
    cb.T = n; cb.n_joints = nj;
    HIP_CHECK(launch_mesh_chain_bwd(cb, stream), "mesh chain reverse");
    // d_feat = (vertex sweep) + d_jrest . wc[j_off:]
    GemmBatch g;
    g.count = 1;
    g.p[0] = plain_prob(w.djrest, mesh->jw4, mesh->wj_t, mesh->jw4, w.dfeat, 200, n, 200, mesh->jw4);
    g.p[0].resid = dv ? w.dfeat_v : nullptr; g.p[0].ldr = 200;
    HIP_CHECK(launch_gemm(g, stream), "rest-joint reverse gemm");
    RodBwdArgs ra;
    ra.theta = poses + (size_t)t0 * 66; ra.ld_theta = 66; ra.d_rot = w.drot; ra.d_feat = w.dfeat;
    ra.g_theta = g_poses + (size_t)t0 * 66; ra.ld_g = 66; ra.g_beta = g_betas + (size_t)t0 * 10; ra.ld_gb = 10;
    ra.trace_g_theta = ra.trace_g_beta = nullptr; ra.T = n; ra.rod_conv = mesh->rod_conv;
    HIP_CHECK(launch_rodrigues_bwd(ra, stream), "rodrigues_bwd kernel");
  }
  return EMPOSE_OK;
}

// ---- per-vertex error between two bodies -------------------------------------------------------------------------
// Scratch for a slab of S frames: the forward's for each body, the posed joints the chain writes on its way to the
// transforms (not returned), and the pair kernel's per-tile partials.
struct MeshErrWs { MeshWs a, b; float *joints, *part; };
static MeshErrWs carve_mesh_err(Carver& c, const empose_mesh* mesh, size_t S) {
  MeshErrWs w;
  w.a = carve_mesh(c, mesh, S);
  w.b = carve_mesh(c, mesh, S);
  w.joints = c.f(S * (size_t)mesh->n_joints * 3);
  w.part = c.f(S * (size_t)((mesh->V + 31) / 32) * 2);
  return w;
}

size_t empose_mesh_vertex_error_workspace_bytes(const empose_mesh_t* mesh, int T) {
  if (!mesh || T <= 0) return 0;
  return Carver::measure([&](Carver& c) { carve_mesh_err(c, mesh, T < MESH_SLAB ? T : MESH_SLAB); });
}

int empose_mesh_vertex_error(const empose_mesh_t* mesh, int T, const float* poses_a, const float* betas_a,
                             const float* trans_a, const float* poses_b, const float* betas_b, const float* trans_b,
                             double* sums, void* workspace, size_t workspace_bytes, empose_stream_t stream_) {
  if (!mesh) return fail(EMPOSE_EINVAL, "mesh is NULL");
  if (!poses_a) return fail(EMPOSE_EINVAL, "poses_a is NULL");
  if (!betas_a) return fail(EMPOSE_EINVAL, "betas_a is NULL");
  if (!poses_b) return fail(EMPOSE_EINVAL, "poses_b is NULL");
  if (!betas_b) return fail(EMPOSE_EINVAL, "betas_b is NULL");
  if (!sums) return fail(EMPOSE_EINVAL, "sums is NULL");
  if (!workspace) return fail(EMPOSE_EINVAL, "workspace is NULL");
  if (T <= 0) return fail(EMPOSE_EINVAL, "T must be positive");
  if (workspace_bytes < empose_mesh_vertex_error_workspace_bytes(mesh, T))
    return fail(EMPOSE_ENOMEM, "workspace too small (empose_mesh_vertex_error_workspace_bytes)");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const int S = T < MESH_SLAB ? T : MESH_SLAB;
  const int n_tiles = (mesh->V + 31) / 32;
  Carver c(workspace);
  const MeshErrWs w = carve_mesh_err(c, mesh, (size_t)S);
  for (int t0 = 0; t0 < T; t0 += S) {
    const int n = (T - t0) < S ? (T - t0) : S;
    const float* tra = trans_a ? trans_a + (size_t)t0 * 3 : nullptr;
    const float* trb = trans_b ? trans_b + (size_t)t0 * 3 : nullptr;
    TRY(mesh_slab_prologue(mesh, w.a, poses_a, betas_a, t0, n, tra, w.joints, stream));
    TRY(mesh_slab_prologue(mesh, w.b, poses_b, betas_b, t0, n, trb, w.joints, stream));
    MeshPairErrorArgs pa;
    pa.feat_a = w.a.feat; pa.xf_a = w.a.xf; pa.trans_a = tra;
    pa.feat_b = w.b.feat; pa.xf_b = w.b.xf; pa.trans_b = trb;
    pa.skin_idx = mesh->skin_idx; pa.skin_w = mesh->skin_w; pa.kb = mesh->kb; pa.T = n; pa.V = mesh->V;
    pa.wc_frag = mesh->wc_frag; pa.skin_idx4 = mesh->skin_idx4; pa.skin_w4 = mesh->skin_w4; pa.part = w.part;
    HIP_CHECK(launch_mesh_pair_error(pa, stream), "mesh pair error kernel");
    HIP_CHECK(launch_mesh_err_sum(w.part, n_tiles, n, sums + (size_t)t0 * 2, stream), "mesh error sum kernel");
  }
  return EMPOSE_OK;
}

// ---- ... and after a Procrustes alignment of B onto A --------------------------------------------------------------
// Scratch for a slab of S frames: as above with the posed joints of each body kept apart (their roots are the pivots of
// the moments), the 17 moment partials per frame and tile and the 16 floats per frame from the solve to the second sweep.
struct MeshErrPaWs { MeshWs a, b; float *joints_a, *joints_b, *part, *part_m, *align; double *rot64, *jrest64; };
static MeshErrPaWs carve_mesh_err_pa(Carver& c, const empose_mesh* mesh, size_t S) {
  const size_t n_tiles = (size_t)((mesh->V + 31) / 32);
  MeshErrPaWs w;
  w.a = carve_mesh(c, mesh, S);
  w.b = carve_mesh(c, mesh, S);
  w.joints_a = c.f(S * (size_t)mesh->n_joints * 3);
  w.joints_b = c.f(S * (size_t)mesh->n_joints * 3);
  w.part = c.f(S * n_tiles * 2);
  w.part_m = c.f(S * n_tiles * MESH_PA_MOMENTS);
  w.align = c.f(S * MESH_PA_ALIGN);
  w.rot64 = reinterpret_cast<double*>(c.f(S * NB * 9 * 2));
  w.jrest64 = reinterpret_cast<double*>(c.f(S * NB * 3 * 2));
  return w;
}

size_t empose_mesh_vertex_error_pa_workspace_bytes(const empose_mesh_t* mesh, int T) {
  if (!mesh || T <= 0) return 0;
  return Carver::measure([&](Carver& c) { carve_mesh_err_pa(c, mesh, T < MESH_SLAB ? T : MESH_SLAB); });
}

int empose_mesh_vertex_error_pa(const empose_mesh_t* mesh, int T, const float* poses_a, const float* betas_a,
                                const float* trans_a, const float* poses_b, const float* betas_b, const float* trans_b,
                                double* sums, void* workspace, size_t workspace_bytes, empose_stream_t stream_) {
  if (!mesh) return fail(EMPOSE_EINVAL, "mesh is NULL");
  if (!poses_a) return fail(EMPOSE_EINVAL, "poses_a is NULL");
  if (!betas_a) return fail(EMPOSE_EINVAL, "betas_a is NULL");
  if (!poses_b) return fail(EMPOSE_EINVAL, "poses_b is NULL");
  if (!betas_b) return fail(EMPOSE_EINVAL, "betas_b is NULL");
  if (!sums) return fail(EMPOSE_EINVAL, "sums is NULL");
  if (!workspace) return fail(EMPOSE_EINVAL, "workspace is NULL");
  if (T <= 0) return fail(EMPOSE_EINVAL, "T must be positive");
  if (workspace_bytes < empose_mesh_vertex_error_pa_workspace_bytes(mesh, T))
    return fail(EMPOSE_ENOMEM, "workspace too small (empose_mesh_vertex_error_pa_workspace_bytes)");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const int S = T < MESH_SLAB ? T : MESH_SLAB;
  const int n_tiles = (mesh->V + 31) / 32, ld_j = mesh->n_joints * 3;
  Carver c(workspace);
  const MeshErrPaWs w = carve_mesh_err_pa(c, mesh, (size_t)S);
  for (int t0 = 0; t0 < T; t0 += S) {
    const int n = (T - t0) < S ? (T - t0) : S;
    const float* tra = trans_a ? trans_a + (size_t)t0 * 3 : nullptr;
    const float* trb = trans_b ? trans_b + (size_t)t0 * 3 : nullptr;
    TRY(mesh_slab_prologue(mesh, w.a, poses_a, betas_a, t0, n, tra, w.joints_a, stream));
    TRY(mesh_slab_prologue(mesh, w.b, poses_b, betas_b, t0, n, trb, w.joints_b, stream));
    MeshPairErrorArgs pa;
    pa.feat_a = w.a.feat; pa.xf_a = w.a.xf; pa.trans_a = tra;
    pa.feat_b = w.b.feat; pa.xf_b = w.b.xf; pa.trans_b = trb;
    pa.skin_idx = mesh->skin_idx; pa.skin_w = mesh->skin_w; pa.kb = mesh->kb; pa.T = n; pa.V = mesh->V;
    pa.wc_frag = mesh->wc_frag; pa.skin_idx4 = mesh->skin_idx4; pa.skin_w4 = mesh->skin_w4; pa.part = w.part;
    // the posed root joints (translation included), the first of each frame's joints, are the pivots
    pa.mode = MESH_PAIR_MOMENTS; pa.pivot_a = w.joints_a; pa.pivot_b = w.joints_b; pa.ld_pivot = ld_j; pa.part_m = w.part_m;
    HIP_CHECK(launch_mesh_pair_error(pa, stream), "mesh pair moments kernel");
    MeshPaSolveArgs so;
    so.part = w.part; so.part_m = w.part_m; so.pivot_a = w.joints_a; so.pivot_b = w.joints_b; so.ld_pivot = ld_j;
    so.align = w.align; so.sums = sums + (size_t)t0 * 4; so.T = n; so.V = mesh->V;
    HIP_CHECK(launch_mesh_pa_solve(so, stream), "mesh alignment solve kernel");
    // the aligned sweep on transforms from a float64 prologue (the moments sweep is done with the float32 ones, which it
    // needs for the plain columns): the sums of squares are stationary in the alignment, so the two go together
    MeshChainF64Args cf;
    cf.wj = mesh->wc + (size_t)mesh->j_off * 200; cf.parents = mesh->parents; cf.rot = w.rot64; cf.jrest = w.jrest64;
    cf.T = n; cf.rod_conv = mesh->rod_conv;
    cf.poses = poses_a + (size_t)t0 * 66; cf.betas = betas_a + (size_t)t0 * 10; cf.xf = w.a.xf;
    HIP_CHECK(launch_mesh_chain_f64(cf, stream), "mesh chain in float64, body A");
    cf.poses = poses_b + (size_t)t0 * 66; cf.betas = betas_b + (size_t)t0 * 10; cf.xf = w.b.xf;
    HIP_CHECK(launch_mesh_chain_f64(cf, stream), "mesh chain in float64, body B");
    pa.mode = MESH_PAIR_ALIGNED; pa.align = w.align;
    HIP_CHECK(launch_mesh_pair_error(pa, stream), "mesh pair aligned kernel");
    HIP_CHECK(launch_mesh_err_sum(w.part, n_tiles, n, sums + (size_t)t0 * 4 + 2, stream, 4), "mesh error sum kernel");
  }
  return EMPOSE_OK;
}

// ---- root normalisation -----------------------------------------------------------------------------------------
static int root_frame_args_ok(int T, int seg_len, int rodrigues, int ld_root, int flags) {
  if (T <= 0 || seg_len <= 0) return fail(EMPOSE_EINVAL, "T and seg_len must be positive");
  if (T % seg_len != 0) return fail(EMPOSE_EINVAL, "T = %d is not a multiple of seg_len = %d", T, seg_len);
  if (ld_root < 3) return fail(EMPOSE_EINVAL, "ld_root must be at least 3");
  if (rodrigues != EMPOSE_RODRIGUES_SMPLX && rodrigues != EMPOSE_RODRIGUES_SO3)
    return fail(EMPOSE_EINVAL, "unknown Rodrigues convention %d", rodrigues);
  if (flags & ~(EMPOSE_ROOT_FRAME_ROTATE | EMPOSE_ROOT_FRAME_SUBTRACT)) return fail(EMPOSE_EINVAL, "unknown flags %d", flags);
  return EMPOSE_OK;
}

int empose_root_frame_fwd(int T, int seg_len, int rodrigues, const float* root, int ld_root, const float* trans,
                          float* root_out, float* trans_out, int flags, empose_stream_t stream_) {
  if (!root || !root_out || (flags && (!trans || !trans_out))) return fail(EMPOSE_EINVAL, "null argument");
  TRY(root_frame_args_ok(T, seg_len, rodrigues, ld_root, flags));
  static_assert(EMPOSE_ROOT_FRAME_ROTATE == ROOT_FRAME_ROTATE && EMPOSE_ROOT_FRAME_SUBTRACT == ROOT_FRAME_SUBTRACT, "flags");
  RootFrameArgs a = {};
  a.root = root; a.ld_root = ld_root; a.trans = trans; a.root_out = root_out; a.trans_out = trans_out;
  a.T = T; a.seg_len = seg_len; a.rod_conv = rodrigues; a.flags = flags;
  HIP_CHECK(launch_root_frame_fwd(a, static_cast<hipStream_t>(stream_)), "root frame kernel");
  return EMPOSE_OK;
}

size_t empose_root_frame_vjp_workspace_bytes(int T, int seg_len) {
  if (T <= 0 || seg_len <= 0 || T % seg_len != 0) return 0;
  return Carver::measure([&](Carver& c) { c.f((size_t)root_frame_vjp_waves(T, seg_len) * ROOT_FRAME_SUMS); });
}

int empose_root_frame_vjp(int T, int seg_len, int rodrigues, const float* root, int ld_root, const float* trans,
                          const float* d_root_out, const float* d_trans_out, float* g_root, float* g_trans, int flags,
                          void* workspace, size_t workspace_bytes, empose_stream_t stream_) {
  if (!root || !g_root || (flags && !trans) || (d_trans_out && !g_trans)) return fail(EMPOSE_EINVAL, "null argument");
  TRY(root_frame_args_ok(T, seg_len, rodrigues, ld_root, flags));
  if (!d_root_out && !d_trans_out) return fail(EMPOSE_EINVAL, "d_root_out and d_trans_out are both NULL");
  if (d_trans_out && !flags) return fail(EMPOSE_EINVAL, "d_trans_out needs flags != 0");
  if (!workspace || workspace_bytes < empose_root_frame_vjp_workspace_bytes(T, seg_len))
    return fail(EMPOSE_EINVAL, "workspace too small (empose_root_frame_vjp_workspace_bytes)");
  RootFrameArgs a = {};
  a.root = root; a.ld_root = ld_root; a.trans = trans; a.d_root_out = d_root_out; a.d_trans_out = d_trans_out;
  a.g_root = g_root; a.g_trans = g_trans; a.part = static_cast<float*>(workspace);
  a.T = T; a.seg_len = seg_len; a.rod_conv = rodrigues; a.flags = flags;
  HIP_CHECK(launch_root_frame_vjp(a, static_cast<hipStream_t>(stream_)), "root frame VJP kernels");
  return EMPOSE_OK;
}

}  // extern "C"
