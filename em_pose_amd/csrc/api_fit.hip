// C ABI (include/empose_hip.h), model-free sensor fitting: the checks of the arguments, then the descent loop -- the SMPL
// evaluation of empose_smpl_sensors_fwd_bwd (smpl_sensors_eval, api_internal.h) and one launch of sensor_fit.hip, K times.
// No host synchronisation, no allocation and no copy inside: the whole call is launches on the caller's stream.
#include "api_internal.h"
#include "fit_kernels.h"

#include <cmath>

using namespace empose;
using namespace empose::api;

namespace {

constexpr int FIT_MAX_FRAMES = 1 << 24;   // B * F: keeps F * 66 and every frame index of the kernels inside an int

struct FitWs {
  void* smpl; size_t smpl_bytes;
  float* theta[2]; float* beta[2];   // the iterates, in turn
  float *g_theta, *g_beta;
  float *moments; size_t n_moments;  // m_theta | v_theta | m_beta | v_beta: one block, zeroed by the prepare launch
  float *m_theta, *v_theta, *m_beta, *v_beta;
  float *s, *best_theta, *best_beta, *best_J, *J;
};
FitWs carve_fit(Carver& c, const empose_model* m, int B, int F) {
  FitWs w;
  const size_t T = (size_t)B * F;
  w.smpl_bytes = align_up(empose_smpl_workspace_bytes(m, (int)T));
  w.smpl = c.f(w.smpl_bytes / sizeof(float));
  for (int i = 0; i < 2; ++i) { w.theta[i] = c.f(T * 66); w.beta[i] = c.f(T * 10); }
  w.g_theta = c.f(T * 66);
  w.g_beta = c.f(T * 10);
  w.n_moments = T * 152;
  w.moments = c.f(w.n_moments);
  w.m_theta = w.moments; w.v_theta = w.moments + T * 66; w.m_beta = w.moments + T * 132; w.v_beta = w.moments + T * 142;
  w.s = c.f(T);
  w.best_theta = c.f(T * 66);
  w.best_beta = c.f(T * 10);
  w.best_J = c.f((size_t)B);
  w.J = c.f((size_t)B * 2);
  return w;
}

bool positive(float x) { return std::isfinite(x) && x > 0.f; }
bool not_negative(float x) { return std::isfinite(x) && x >= 0.f; }
bool a_beta(float x) { return std::isfinite(x) && x >= 0.f && x < 1.f; }

// What empose_sensor_fit and empose_sensor_fit_step both rely on.
int check_problem(const empose_model* m, const empose_fit_io* io) {
  if (!m) return fail(EMPOSE_EINVAL, "sensor fit: null model");
  if (!io) return fail(EMPOSE_EINVAL, "sensor fit: null io");
  if (io->B <= 0 || io->F <= 0) return fail(EMPOSE_EINVAL, "sensor fit: B and F must be positive (B = %d, F = %d)", io->B, io->F);
  if ((long)io->B * io->F > FIT_MAX_FRAMES)
    return fail(EMPOSE_EINVAL, "sensor fit: B * F = %ld above %d: too large for one call", (long)io->B * io->F, FIT_MAX_FRAMES);
  if (!io->tgt) return fail(EMPOSE_EINVAL, "sensor fit: null tgt");
  if (io->ld_tgt < 12 * m->n_markers)
    return fail(EMPOSE_EINVAL, "sensor fit: ld_tgt = %d is shorter than a row of %d sensors (%d)", io->ld_tgt, m->n_markers,
                12 * m->n_markers);
  if (!positive(io->lr)) return fail(EMPOSE_EINVAL, "sensor fit: lr must be finite and positive");
  if (!positive(io->lr_decay)) return fail(EMPOSE_EINVAL, "sensor fit: lr_decay must be finite and positive");
  if (!a_beta(io->beta1)) return fail(EMPOSE_EINVAL, "sensor fit: beta1 must lie in [0, 1)");
  if (!a_beta(io->beta2)) return fail(EMPOSE_EINVAL, "sensor fit: beta2 must lie in [0, 1)");
  if (!not_negative(io->eps)) return fail(EMPOSE_EINVAL, "sensor fit: eps must be finite and not negative");
  if (!not_negative(io->lambda_pose)) return fail(EMPOSE_EINVAL, "sensor fit: lambda_pose must be finite and not negative");
  if (!not_negative(io->lambda_shape)) return fail(EMPOSE_EINVAL, "sensor fit: lambda_shape must be finite and not negative");
  if (!not_negative(io->lambda_smooth)) return fail(EMPOSE_EINVAL, "sensor fit: lambda_smooth must be finite and not negative");
  return EMPOSE_OK;
}

FitProblem problem_of(const empose_model* m, const empose_fit_io* io, const float* s) {
  FitProblem p;
  p.tgt = io->tgt; p.ld_tgt = io->ld_tgt; p.s = s; p.seq_lengths = io->seq_lengths; p.prior = io->pose_prior;
  p.B = io->B; p.F = io->F; p.n_markers = m->n_markers;
  for (int i = 0; i < 12; ++i) p.used_slot[i] = m->used_slot[i];
  p.lambda_pose = io->lambda_pose; p.lambda_shape = io->lambda_shape; p.lambda_smooth = io->lambda_smooth;
  p.shape_per_window = io->shape_per_window ? 1 : 0;
  return p;
}

// The factors of iteration k, in double, each rounded once: the device raises nothing to a power.
void step_factors(const empose_fit_io* io, int k, FitStepArgs* a) {
  a->lr_k = (float)((double)io->lr * std::pow((double)io->lr_decay, (double)k));
  a->c1 = (float)(1.0 / (1.0 - std::pow((double)io->beta1, (double)(k + 1))));
  a->c2 = (float)(1.0 / (1.0 - std::pow((double)io->beta2, (double)(k + 1))));
  a->beta1 = io->beta1; a->beta2 = io->beta2; a->eps = io->eps;
}

}  // namespace

extern "C" {

size_t empose_sensor_fit_workspace_bytes(const empose_model_t* m, int B, int F) {
  if (!m || B <= 0 || F <= 0 || (long)B * F > FIT_MAX_FRAMES) return 0;
  return Carver::measure([&](Carver& c) { carve_fit(c, m, B, F); });
}

int empose_sensor_fit_step(const empose_model_t* m, const empose_fit_io* io, int k, const float* theta, const float* beta,
                           const float* g_theta, const float* g_beta, const float* pos, const float* ori, const float* s,
                           float* m_theta, float* v_theta, float* m_beta, float* v_beta, float* theta_next,
                           float* beta_next, float* energy, float* J, float* best_J, float* best_theta, float* best_beta,
                           empose_stream_t stream_) {
  TRY(check_problem(m, io));
  if (k < 0) return fail(EMPOSE_EINVAL, "sensor fit step: k must not be negative (%d)", k);
  if (!theta || !beta || !g_theta || !g_beta || !pos || !ori || !s)
    return fail(EMPOSE_EINVAL, "sensor fit step: null input (theta, beta, g_theta, g_beta, pos, ori, s)");
  if (!m_theta || !v_theta || !m_beta || !v_beta) return fail(EMPOSE_EINVAL, "sensor fit step: null moment buffer");
  if (!theta_next || !beta_next || !J) return fail(EMPOSE_EINVAL, "sensor fit step: null output (theta_next, beta_next, J)");
  if (theta_next == theta || beta_next == beta)
    return fail(EMPOSE_EINVAL, "sensor fit step: theta_next / beta_next must not be the buffers of the iterate read");
  if ((best_J != nullptr) != (best_theta != nullptr) || (best_J != nullptr) != (best_beta != nullptr))
    return fail(EMPOSE_EINVAL, "sensor fit step: best_J, best_theta and best_beta go together");
  FitStepArgs a;
  a.p = problem_of(m, io, s);
  a.theta = theta; a.beta = beta; a.g_theta = g_theta; a.g_beta = g_beta; a.pos = pos; a.ori = ori;
  a.m_theta = m_theta; a.v_theta = v_theta; a.m_beta = m_beta; a.v_beta = v_beta;
  a.theta_next = theta_next; a.beta_next = beta_next; a.energy = energy; a.J = J;
  a.best_J = best_J; a.best_theta = best_theta; a.best_beta = best_beta;
  step_factors(io, k, &a);
  HIP_CHECK(launch_fit_step(a, static_cast<hipStream_t>(stream_)), "sensor fit step kernel");
  return EMPOSE_OK;
}

int empose_sensor_fit(const empose_model_t* m, const empose_fit_io* io, void* workspace, size_t workspace_bytes,
                      empose_stream_t stream_) {
  TRY(check_problem(m, io));
  if (io->K < 0) return fail(EMPOSE_EINVAL, "sensor fit: K must not be negative (%d)", io->K);
  if (!io->offset_r || !io->offset_t) return fail(EMPOSE_EINVAL, "sensor fit: null offset_r / offset_t");
  if (!io->pose || !io->shape || !io->joints || !io->pos || !io->ori)
    return fail(EMPOSE_EINVAL, "sensor fit: null output (pose, shape, joints, pos, ori)");
  if (!workspace) return fail(EMPOSE_EINVAL, "sensor fit: null workspace");
  if (workspace_bytes < empose_sensor_fit_workspace_bytes(m, io->B, io->F))
    return fail(EMPOSE_ENOMEM, "sensor fit: workspace too small (empose_sensor_fit_workspace_bytes)");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const int B = io->B, F = io->F, T = B * F, K = io->K;
  Carver c(workspace);
  const FitWs w = carve_fit(c, m, B, F);
  const FitProblem p = problem_of(m, io, w.s);
  const bool keep_best = io->keep_best != 0;
  auto J_row = [&](int k) { return io->objective ? io->objective + (size_t)k * B : w.J + (size_t)(k > K ? 1 : 0) * B; };
  // forward (+ reverse against the readings, with the weights s) of an iterate, as the public call does it at this T
  auto evaluate = [&](const float* theta, const float* beta, bool reverse) {
    return smpl_sensors_eval(m, T, F, theta, 66, beta, 10, io->offset_r, io->offset_t, reverse ? io->tgt : nullptr,
                             io->ld_tgt, reverse ? w.s : nullptr, io->pos, io->ori, io->joints,
                             reverse ? w.g_theta : nullptr, 66, reverse ? w.g_beta : nullptr, 10, w.smpl, stream);
  };

  FitPrepareArgs pa;
  pa.p = p; pa.marker_masks = io->marker_masks; pa.pose_init = io->pose_init; pa.shape_init = io->shape_init;
  pa.theta = w.theta[0]; pa.beta = w.beta[0]; pa.moments = w.moments; pa.n_moments = w.n_moments;
  pa.s = w.s; pa.best_J = w.best_J;
  HIP_CHECK(launch_fit_prepare(pa, stream), "sensor fit prepare kernel");

  for (int k = 0; k < K; ++k) {
    const int cur = k & 1;
    TRY(evaluate(w.theta[cur], w.beta[cur], true));
    FitStepArgs a;
    a.p = p;
    a.theta = w.theta[cur]; a.beta = w.beta[cur]; a.g_theta = w.g_theta; a.g_beta = w.g_beta; a.pos = io->pos; a.ori = io->ori;
    a.m_theta = w.m_theta; a.v_theta = w.v_theta; a.m_beta = w.m_beta; a.v_beta = w.v_beta;
    a.theta_next = w.theta[cur ^ 1]; a.beta_next = w.beta[cur ^ 1]; a.energy = nullptr; a.J = J_row(k);
    a.best_J = keep_best ? w.best_J : nullptr;
    a.best_theta = keep_best ? w.best_theta : nullptr; a.best_beta = keep_best ? w.best_beta : nullptr;
    step_factors(io, k, &a);
    HIP_CHECK(launch_fit_step(a, stream), "sensor fit step kernel");
  }

  const int last = K & 1;
  TRY(evaluate(w.theta[last], w.beta[last], false));
  FitFinishArgs fa;
  fa.p = p; fa.theta = w.theta[last]; fa.beta = w.beta[last]; fa.pos = io->pos; fa.ori = io->ori;
  fa.best_J = keep_best ? w.best_J : nullptr;
  fa.best_theta = keep_best ? w.best_theta : nullptr; fa.best_beta = keep_best ? w.best_beta : nullptr;
  fa.pose = io->pose; fa.shape = io->shape; fa.J_last = J_row(K); fa.J_out = J_row(K + 1);
  HIP_CHECK(launch_fit_finish(fa, stream), "sensor fit finish kernel");

  TRY(evaluate(io->pose, io->shape, false));
  if (io->energy) HIP_CHECK(launch_fit_energy(p, io->pos, io->ori, io->energy, stream), "sensor fit energy kernel");
  return EMPOSE_OK;
}

}  // extern "C"
