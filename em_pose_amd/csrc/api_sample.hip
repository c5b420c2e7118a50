// C ABI (include/empose_hip.h), synthetic sensor sampling: the checks of the arguments, then the one launch of the
// forward (sensor_sample.hip), or for the reverse the fold of the cotangents and the two passes of sensors_vjp.hip, slab
// by slab.
#include "api_internal.h"
#include "data_kernels.h"
#include "mesh_kernels.h"

#include <climits>

using namespace empose;
using namespace empose::api;

static_assert(EMPOSE_SAMPLE_LOCAL_NONE == SAMPLE_LOCAL_NONE && EMPOSE_SAMPLE_LOCAL_WINDOW == SAMPLE_LOCAL_WINDOW &&
              EMPOSE_SAMPLE_LOCAL_FRAME == SAMPLE_LOCAL_FRAME, "sample-sensors modes");

namespace {

// What both entry points ask of the sizes, the mode and the constants.
int check_sample(int N, int F, int V, int M, int max_deg, int mode, const float* local) {
  if (N <= 0 || F <= 0 || V <= 0 || M <= 0 || max_deg <= 0) return fail(EMPOSE_EINVAL, "N, F, V, M and max_deg must be positive");
  if ((double)N * F * M > (double)INT_MAX) return fail(EMPOSE_EINVAL, "N * F * M above 2^31 - 1: too large for one call");
  if (mode != EMPOSE_SAMPLE_LOCAL_NONE && mode != EMPOSE_SAMPLE_LOCAL_WINDOW && mode != EMPOSE_SAMPLE_LOCAL_FRAME)
    return fail(EMPOSE_EINVAL, "unknown sample-sensors mode %d", mode);
  if (mode != EMPOSE_SAMPLE_LOCAL_NONE && !local) return fail(EMPOSE_EINVAL, "mode %d needs `local`", mode);
  return EMPOSE_OK;
}

// Scratch of the sensor pass, then the folded cotangents of pos and ori, for one slab of S frames.
struct SampleVjpWs { float* scratch; float* d_pos; float* d_ori; };
SampleVjpWs carve_sample_vjp(Carver& c, int S, int M) {
  SampleVjpWs w;
  w.scratch = c.f((size_t)S * M * SENSOR_VJP_ROW);
  w.d_pos = c.f((size_t)S * M * 3);
  w.d_ori = c.f((size_t)S * M * 9);
  return w;
}

}  // namespace

extern "C" {

int empose_sample_sensors_fwd(int N, int F, int V, const float* vertices, int M, int max_deg, const int* center,
                              const int* helper, const int* deg, const int* faces, int mode, const float* local,
                              const float* r, float* pos, float* ori, float* normals, float* pos_synth,
                              float* ori_synth, float* normal_synth, empose_stream_t stream_) {
  if (!vertices || !center || !helper || !deg || !faces) return fail(EMPOSE_EINVAL, "null vertex or table pointer");
  TRY(check_sample(N, F, V, M, max_deg, mode, local));
  if (!pos && !ori && !normals && !pos_synth && !ori_synth && !normal_synth)
    return fail(EMPOSE_EINVAL, "all six outputs are NULL");
  SampleSensorsArgs a;
  a.vertices = vertices; a.center = center; a.helper = helper; a.deg = deg; a.faces = faces;
  a.local = mode == EMPOSE_SAMPLE_LOCAL_NONE ? nullptr : local; a.r = r;
  a.pos = pos; a.ori = ori; a.normals = normals;
  a.pos_synth = pos_synth; a.ori_synth = ori_synth; a.normal_synth = normal_synth;
  a.T = N * F; a.F = F; a.V = V; a.M = M; a.max_deg = max_deg; a.mode = mode;
  HIP_CHECK(launch_sample_sensors(a, static_cast<hipStream_t>(stream_)), "sample sensors kernel");
  return EMPOSE_OK;
}

size_t empose_sample_sensors_vjp_workspace_bytes(int T, int M) {
  if (T <= 0 || M <= 0) return 0;
  return Carver::measure([&](Carver& c) { carve_sample_vjp(c, sensors_vjp_slab(T, M), M); });
}

int empose_sample_sensors_vjp(int N, int F, int V, const float* vertices, int M, int max_deg, const int* center,
                              const int* helper, const int* deg, const int* faces, int n_sub_faces,
                              const int* sub_faces, const int* face_ptr, const int* face_sensors, const int* vf_ptr,
                              const int* vf_corner, const int* vs_ptr, const int* vs_role, int n_touched,
                              const int* touched, int mode, const float* local, const float* r, const float* d_pos,
                              const float* d_ori, const float* d_normals, const float* d_pos_synth,
                              const float* d_ori_synth, const float* d_normal_synth, float* d_vertices,
                              void* workspace, size_t workspace_bytes, empose_stream_t stream_) {
  if (!vertices || !center || !helper || !deg || !faces || !sub_faces || !face_ptr || !face_sensors || !vf_ptr ||
      !vf_corner || !vs_ptr || !vs_role || !touched || !d_vertices)
    return fail(EMPOSE_EINVAL, "null vertex, table or d_vertices pointer");
  TRY(check_sample(N, F, V, M, max_deg, mode, local));
  if (n_sub_faces <= 0 || n_touched <= 0) return fail(EMPOSE_EINVAL, "n_sub_faces and n_touched must be positive");
  if (!d_pos && !d_ori && !d_normals && !d_pos_synth && !d_ori_synth && !d_normal_synth)
    return fail(EMPOSE_EINVAL, "all six cotangents are NULL");
  const int T = N * F;
  if (!workspace || workspace_bytes < empose_sample_sensors_vjp_workspace_bytes(T, M))
    return fail(EMPOSE_EINVAL, "workspace too small (empose_sample_sensors_vjp_workspace_bytes)");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const int S = sensors_vjp_slab(T, M);
  Carver carver(workspace);
  const SampleVjpWs ws = carve_sample_vjp(carver, S, M);
  const bool with_local = mode != EMPOSE_SAMPLE_LOCAL_NONE;
  const bool any_pos = d_pos || d_pos_synth;
  const bool any_ori = d_ori || d_ori_synth || d_normal_synth || (with_local && d_pos_synth);

  SampleFoldArgs fa;
  fa.local = with_local ? local : nullptr; fa.r = r;
  fa.d_pos_out = any_pos ? ws.d_pos : nullptr; fa.d_ori_out = any_ori ? ws.d_ori : nullptr;
  fa.F = F; fa.M = M; fa.mode = mode;
  SensorVjpArgs a;
  a.center = center; a.helper = helper; a.deg = deg; a.faces = faces;
  a.sub_faces = sub_faces; a.face_ptr = face_ptr; a.face_sensors = face_sensors;
  a.vf_ptr = vf_ptr; a.vf_corner = vf_corner; a.vs_ptr = vs_ptr; a.vs_role = vs_role;
  a.touched = touched; a.n_touched = n_touched;
  a.scratch = ws.scratch;
  a.d_pos = fa.d_pos_out; a.d_ori = fa.d_ori_out;
  a.V = V; a.M = M; a.max_deg = max_deg;
  auto at = [](const float* p, size_t off) { return p ? p + off : nullptr; };
  for (int t0 = 0; t0 < T; t0 += S) {
    const size_t row = (size_t)t0 * M;
    fa.T = a.T = (T - t0) < S ? (T - t0) : S;
    fa.t0 = t0;
    fa.d_pos = at(d_pos, row * 3); fa.d_ori = at(d_ori, row * 9);
    fa.d_pos_synth = at(d_pos_synth, row * 3); fa.d_ori_synth = at(d_ori_synth, row * 9);
    fa.d_normal_synth = at(d_normal_synth, row * 3);
    if (any_pos || any_ori) HIP_CHECK(launch_sample_fold(fa, stream), "sample sensors fold kernel");
    a.vertices = vertices + (size_t)t0 * V * 3;
    a.d_vertices = d_vertices + (size_t)t0 * V * 3;
    a.d_normals = at(d_normals, row * 3);
    HIP_CHECK(launch_sensors_vjp(a, stream), "virtual sensors VJP kernels");
  }
  return EMPOSE_OK;
}

}  // extern "C"
