// Vector-Jacobian product of virtual_sensors_kernel (virtual_sensors.hip): the virtual sensors of arbitrary full-mesh vertices
// under autograd (data/virtual_sensors.py), gfx950 only.
//
// Forward, per (frame, sensor m): n = (sum over the deg_m incident faces of (v1 - v0) x (v2 - v0)) / deg_m, nh = n/|n|,
// s = unit(v_helper - v_center), t = unit(nh x s), s2 = unit(t x nh); ori = [s2 | t | nh] (columns), pos = v_center,
// normals = n.  The reverse runs in two launches and sums every destination in one fixed order (no atomics: repeated
// calls give the same bits, whatever vertices the sensors share):
//   sensor pass  one lane per (frame, sensor): the frame math backwards -> dn_m / deg_m, the center's and the helper's
//                cotangents, nine floats per (frame, sensor) in the workspace
//   vertex pass  one lane per (frame, mesh vertex u), every vertex of the mesh: over u's (sub-face f, corner k) entries
//                in ascending f, (v_{k+1} - v_{k+2}) x g_f with g_f = sum of dn_m / deg_m over the sensors incident to f
//                in ascending m (the gradient of g.((v1 - v0) x (v2 - v0)) with respect to v_k), then the center and
//                helper terms of u in ascending (sensor, role).  Two forms: when more than a quarter of the mesh
//                has terms (vertex normals over the whole mesh), every vertex gets a lane, those without entries write
//                zeros, and a workgroup's 256 contiguous rows leave through LDS as 16-byte stores; otherwise
//                (a few sensors) d_vertices is cleared and only the touched vertices get lanes.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mesh_kernels.h"
#include "smpl_math.h"

namespace empose {

namespace {

constexpr int SP_THREADS = 128;
constexpr int VP_THREADS = 256;

__global__ void sensors_vjp_sensor_kernel(SensorVjpArgs a) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= a.T * a.M) return;
  const int t = idx / a.M, m = idx % a.M;
  const float* V = a.vertices + (size_t)t * a.V * 3;
  const int deg = a.deg[m];
  const int* faces = a.faces + (size_t)m * a.max_deg * 3;
  // the forward's arithmetic, in the forward's order
  float n[3] = {0.f, 0.f, 0.f};
  for (int k = 0; k < deg; ++k) {
    const float* v0 = V + (size_t)faces[k * 3 + 0] * 3;
    const float* v1 = V + (size_t)faces[k * 3 + 1] * 3;
    const float* v2 = V + (size_t)faces[k * 3 + 2] * 3;
    const float e1[3] = {v1[0] - v0[0], v1[1] - v0[1], v1[2] - v0[2]};
    const float e2[3] = {v2[0] - v0[0], v2[1] - v0[1], v2[2] - v0[2]};
    float fn[3];
    cross3(e1, e2, fn);
    n[0] += fn[0]; n[1] += fn[1]; n[2] += fn[2];
  }
  const float fdeg = (float)deg;
  n[0] /= fdeg; n[1] /= fdeg; n[2] /= fdeg;
  const float nn = norm3(n);
  const float nh[3] = {n[0] / nn, n[1] / nn, n[2] / nn};
  const float* vc = V + (size_t)a.center[m] * 3;
  const float* vh = V + (size_t)a.helper[m] * 3;
  const float e[3] = {vh[0] - vc[0], vh[1] - vc[1], vh[2] - vc[2]};
  const float ne = norm3(e);
  const float sv[3] = {e[0] / ne, e[1] / ne, e[2] / ne};
  float bb[3];
  cross3(nh, sv, bb);
  const float nb = norm3(bb);
  const float tv[3] = {bb[0] / nb, bb[1] / nb, bb[2] / nb};
  float aa[3];
  cross3(tv, nh, aa);
  const float na = norm3(aa);
  const float s2[3] = {aa[0] / na, aa[1] / na, aa[2] / na};
  // cotangents of the outputs (a NULL one is zero)
  const size_t row = (size_t)idx;   // the caller's pointers start at the slab
  float dpos[3] = {0.f, 0.f, 0.f}, ds2[3] = {0.f, 0.f, 0.f}, dt[3] = {0.f, 0.f, 0.f}, dnh[3] = {0.f, 0.f, 0.f};
  float dn[3] = {0.f, 0.f, 0.f};
  if (a.d_pos)
    for (int r = 0; r < 3; ++r) dpos[r] = a.d_pos[row * 3 + r];
  if (a.d_ori)
    for (int r = 0; r < 3; ++r) {
      ds2[r] = a.d_ori[row * 9 + r * 3 + 0];
      dt[r] = a.d_ori[row * 9 + r * 3 + 1];
      dnh[r] = a.d_ori[row * 9 + r * 3 + 2];
    }
  float de[3] = {0.f, 0.f, 0.f};
  if (a.d_ori) {
    float da[3], tmp[3];
    unit_bwd(ds2, s2, 1.f / na, da);   // a = t x nh
    cross3(nh, da, tmp); dt[0] += tmp[0]; dt[1] += tmp[1]; dt[2] += tmp[2];
    cross3(da, tv, tmp); dnh[0] += tmp[0]; dnh[1] += tmp[1]; dnh[2] += tmp[2];
    float db[3];
    unit_bwd(dt, tv, 1.f / nb, db);    // b = nh x s
    cross3(sv, db, tmp); dnh[0] += tmp[0]; dnh[1] += tmp[1]; dnh[2] += tmp[2];
    float dsv[3];
    cross3(db, nh, dsv);
    unit_bwd(dsv, sv, 1.f / ne, de);   // s = e / |e|, e = v_helper - v_center
    unit_bwd(dnh, nh, 1.f / nn, dn);   // nh = n / |n|
  }
  if (a.d_normals)
    for (int r = 0; r < 3; ++r) dn[r] += a.d_normals[row * 3 + r];
  float* o = a.scratch + (size_t)idx * SENSOR_VJP_ROW;
  for (int r = 0; r < 3; ++r) {
    o[r] = dn[r] / fdeg;           // g contribution of every incident face
    o[3 + r] = dpos[r] - de[r];    // center
    o[6 + r] = de[r];              // helper
  }
}

// The cotangent of vertex u of slab frame t (every term, in the fixed order).
__device__ __forceinline__ void vertex_grad(const SensorVjpArgs& a, int t, int u, float (&acc)[3]) {
  const float* V = a.vertices + (size_t)t * a.V * 3;
  const float* S = a.scratch + (size_t)t * a.M * SENSOR_VJP_ROW;
  for (int i = a.vf_ptr[u], end = a.vf_ptr[u + 1]; i < end; ++i) {
    const int fk = a.vf_corner[i], f = fk / 3, k = fk - 3 * f;
    float gf[3] = {0.f, 0.f, 0.f};
    for (int j = a.face_ptr[f], je = a.face_ptr[f + 1]; j < je; ++j) {
      const float* d = S + (size_t)a.face_sensors[j] * SENSOR_VJP_ROW;
      gf[0] += d[0]; gf[1] += d[1]; gf[2] += d[2];
    }
    const int* fv = a.sub_faces + (size_t)f * 3;
    const int k1 = k == 2 ? 0 : k + 1, k2 = k == 0 ? 2 : k - 1;
    const float* p = V + (size_t)fv[k1] * 3;
    const float* q = V + (size_t)fv[k2] * 3;
    const float w[3] = {p[0] - q[0], p[1] - q[1], p[2] - q[2]};
    float c[3];
    cross3(w, gf, c);
    acc[0] += c[0]; acc[1] += c[1]; acc[2] += c[2];
  }
  for (int i = a.vs_ptr[u], end = a.vs_ptr[u + 1]; i < end; ++i) {
    const int mr = a.vs_role[i], m = mr >> 1, role = mr & 1;
    const float* d = S + (size_t)m * SENSOR_VJP_ROW + 3 + 3 * role;
    acc[0] += d[0]; acc[1] += d[1]; acc[2] += d[2];
  }
}

// Dense form: one lane per (frame, vertex) of the slab, flattened: the workgroup's 256 rows of 3 floats are contiguous
// in d_vertices (768 floats), staged in LDS and stored as float4 when the destination is 16-byte aligned.
__global__ void __launch_bounds__(VP_THREADS) sensors_vjp_vertex_kernel(SensorVjpArgs a) {
  __shared__ float stage[VP_THREADS * 3];
  const size_t total = (size_t)a.T * a.V;
  const size_t g0 = (size_t)blockIdx.x * VP_THREADS;
  const size_t g = g0 + threadIdx.x;
  // one division per workgroup (uniform): a lane's frame is the workgroup's first or one of the next few
  const int t0 = (int)(g0 / (size_t)a.V);
  float acc[3] = {0.f, 0.f, 0.f};
  if (g < total) {
    int t = t0, u = (int)(g0 - (size_t)t0 * a.V) + (int)threadIdx.x;
    while (u >= a.V) { u -= a.V; ++t; }
    vertex_grad(a, t, u, acc);
  }
  float* out = a.d_vertices + g0 * 3;
  const size_t n_out = (total - g0 < (size_t)VP_THREADS ? total - g0 : (size_t)VP_THREADS) * 3;
  if (n_out == (size_t)VP_THREADS * 3 && (reinterpret_cast<uintptr_t>(out) & 15) == 0) {
    for (int r = 0; r < 3; ++r) stage[threadIdx.x * 3 + r] = acc[r];
    __syncthreads();
    if (threadIdx.x < VP_THREADS * 3 / 4)
      reinterpret_cast<float4*>(out)[threadIdx.x] = reinterpret_cast<const float4*>(stage)[threadIdx.x];
  } else if (g < total) {
    for (int r = 0; r < 3; ++r) out[threadIdx.x * 3 + r] = acc[r];
  }
}

// Sparse form (few touched vertices): d_vertices is cleared first, then one lane per (frame, touched vertex) writes
// that vertex's row.
__global__ void sensors_vjp_touched_kernel(SensorVjpArgs a) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= a.T * a.n_touched) return;
  const int t = idx / a.n_touched, u = a.touched[idx % a.n_touched];
  float acc[3] = {0.f, 0.f, 0.f};
  vertex_grad(a, t, u, acc);
  float* out = a.d_vertices + ((size_t)t * a.V + u) * 3;
  for (int r = 0; r < 3; ++r) out[r] = acc[r];
}

}  // namespace

hipError_t launch_sensors_vjp(const SensorVjpArgs& a, hipStream_t stream) {
  const long ns = (long)a.T * a.M;
  hipLaunchKernelGGL(sensors_vjp_sensor_kernel, dim3((unsigned)((ns + SP_THREADS - 1) / SP_THREADS)), dim3(SP_THREADS),
                     0, stream, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const size_t nv = (size_t)a.T * a.V;
  if ((size_t)a.n_touched * 4 > (size_t)a.V) {   // most vertices have terms: the dense form writes each row once
    hipLaunchKernelGGL(sensors_vjp_vertex_kernel, dim3((unsigned)((nv + VP_THREADS - 1) / VP_THREADS)),
                       dim3(VP_THREADS), 0, stream, a);
    return hipGetLastError();
  }
  // few: a store-only clear runs at the write rate, the dense form waited on its table loads before every store
  e = hipMemsetAsync(a.d_vertices, 0, nv * 3 * sizeof(float), stream);
  if (e != hipSuccess) return e;
  const long nt = (long)a.T * a.n_touched;
  hipLaunchKernelGGL(sensors_vjp_touched_kernel, dim3((unsigned)((nt + SP_THREADS - 1) / SP_THREADS)),
                     dim3(SP_THREADS), 0, stream, a);
  return hipGetLastError();
}

}  // namespace empose
