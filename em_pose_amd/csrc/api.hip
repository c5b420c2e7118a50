// C ABI (include/empose_hip.h), core: the error state, the profiler, the kernel-variant options, the poll-timeout word,
// dynamic LDS and co-residency, version.  The entry points of the subsystems live in api_model.hip, api_lstm.hip,
// api_train.hip and api_mesh.hip.
#include "api_internal.h"
#include "gemm_kernels.h"
#include "launch.h"
#include "options.h"
#include "train_kernels.h"

#include <cstdarg>
#include <cstdio>
#include <map>
#include <mutex>
#include <string>

using namespace empose;
using namespace empose::api;

namespace {
thread_local std::string g_err;

const char* const kProfNames[P_NTAGS] = {"pack_inputs", "lstm_step", "init_heads_gemm",
                                         "update_feat", "blend_gemm", "chain_sensors", "blend_T_gemm",
                                         "rodrigues_bwd", "mlp_in_gemm", "mlp_hidden_gemm", "mlp_out_gemm",
                                         "mlp_fused", "init_mlp_gemm", "copies", "event_pair", "end"};
struct Profiler {
  bool on = false;
  int only = -1;            // >= 0: bracket launches of this tag only (and one empty event pair per forward: P_EVENT_PAIR)
  std::vector<hipEvent_t> ev;
  std::vector<int> tags;
  size_t used = 0;
};
Profiler g_prof;

// The name of every option and where it lives in Options (EMPOSE_OPTIONS, options.h); nullptr for an unknown name.
int* option_slot(const char* name) {
  static const struct { const char* name; int Options::*field; } table[] = {
#define EMPOSE_OPTION_ENTRY(name, default_value) {#name, &Options::name},
      EMPOSE_OPTIONS(EMPOSE_OPTION_ENTRY)
#undef EMPOSE_OPTION_ENTRY
  };
  for (const auto& e : table)
    if (std::strcmp(name, e.name) == 0) return &(options().*e.field);
  return nullptr;
}
}  // namespace

namespace empose {
namespace api {

int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

void prof_mark(int tag, hipStream_t stream) {
  if (!g_prof.on) return;
  // Single-kernel mode: events go around the launches of ONE tag (start, then P_END right after the launch), so the
  // rest of the step runs unperturbed; P_EVENT_PAIR / P_END pairs with nothing in between measure what the two event
  // packets themselves cost (the caller subtracts it).
  if (g_prof.only >= 0 && tag != g_prof.only && tag != P_EVENT_PAIR &&
      !(tag == P_END && !g_prof.tags.empty() && (g_prof.tags.back() == g_prof.only || g_prof.tags.back() == P_EVENT_PAIR)))
    return;
  if (g_prof.used == g_prof.ev.size()) {
    hipEvent_t e;
    if (hipEventCreate(&e) != hipSuccess) return;
    g_prof.ev.push_back(e);
  }
  (void)hipEventRecord(g_prof.ev[g_prof.used++], stream);
  g_prof.tags.push_back(tag);
}

void prof_end_forward(hipStream_t stream) {
  prof_mark(P_END, stream);
  if (g_prof.on && g_prof.only >= 0) {   // calibration: two event packets with nothing in between
    prof_mark(P_EVENT_PAIR, stream);
    prof_mark(P_END, stream);
  }
}

int earlier_poll_timeouts() {
  if (const unsigned n = poll_timeouts_peek())
    return fail(EMPOSE_ETIMEOUT, "%u poll(s) of a cooperative kernel (whole-sequence LSTM / one-launch training layer) launched by an earlier call timed out waiting for "
                "another workgroup's exchange word; that call's outputs are NaN (the state it carried too); "
                "empose_async_status() reports and clears this", n);
  return EMPOSE_OK;
}

}  // namespace api

Options& options() {
  static Options o;
  return o;
}

namespace {
unsigned* g_timeout_host = nullptr;   // host-mapped, device-visible (fine-grained): written by kernels, read here
unsigned* g_timeout_dev = nullptr;
}  // namespace
int poll_spin_limit(int kernel_default) { return options().spin_limit > 0 ? options().spin_limit : kernel_default; }
unsigned* poll_timeout_word() {
  static std::once_flag once;
  std::call_once(once, [] {
    void* h = nullptr;
    // (Portable: the word is pinned for every device of the process, not only the one that happens to be current here)
    if (hipHostMalloc(&h, 64, hipHostMallocMapped | hipHostMallocPortable) != hipSuccess) { (void)hipGetLastError(); return; }
    std::memset(h, 0, 64);
    void* d = nullptr;
    if (hipHostGetDevicePointer(&d, h, 0) != hipSuccess) { (void)hipGetLastError(); (void)hipHostFree(h); return; }
    g_timeout_host = static_cast<unsigned*>(h);
    g_timeout_dev = static_cast<unsigned*>(d);
  });
  return g_timeout_dev;
}
unsigned poll_timeouts_take() {
  if (!g_timeout_host) return 0;
  return __atomic_exchange_n(g_timeout_host, 0u, __ATOMIC_RELAXED);
}
unsigned poll_timeouts_peek() {
  if (!g_timeout_host) return 0;
  return __atomic_load_n(g_timeout_host, __ATOMIC_RELAXED);
}

hipError_t coresident_blocks(const void* fn, int threads, size_t lds_bytes, int* blocks) {
  int dev = 0;
  if (hipError_t e = hipGetDevice(&dev)) return e;
  struct Entry { size_t lds = 0; int blocks = -1; };
  static std::mutex mu;
  static std::map<std::pair<int, const void*>, Entry> cache;
  std::lock_guard<std::mutex> lock(mu);
  Entry& c = cache[{dev, fn}];
  if (c.blocks < 0 || lds_bytes > c.lds) {   // (a figure computed for more LDS is a safe one for less)
    if (hipError_t e = allow_dynamic_lds(fn, lds_bytes)) return e;
    int per_cu = 0;
    hipDeviceProp_t prop;
    hipError_t e = hipGetDeviceProperties(&prop, dev);
    if (e == hipSuccess) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, threads, lds_bytes);
    if (e != hipSuccess) return e;
    c.lds = lds_bytes;
    c.blocks = per_cu * prop.multiProcessorCount;
  }
  *blocks = c.blocks;
  return hipSuccess;
}

hipError_t allow_dynamic_lds(const void* fn, size_t bytes) {
  if (bytes > LDS_BYTES_PER_CU) return hipErrorInvalidValue;
  int dev = 0;
  if (hipError_t e = hipGetDevice(&dev)) return e;
  static std::mutex mu;
  static std::map<std::pair<int, const void*>, size_t> allowed;
  std::lock_guard<std::mutex> lock(mu);
  size_t& have = allowed[{dev, fn}];
  if (bytes <= have) return hipSuccess;
  if (hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes)) return e;
  have = bytes;
  return hipSuccess;
}
}  // namespace empose

extern "C" {

const char* empose_last_error(void) { return g_err.c_str(); }

int empose_set_option(const char* name, int value) {
  if (!name) return fail(EMPOSE_EINVAL, "null option name");
  int* slot = option_slot(name);
  if (!slot) return fail(EMPOSE_EINVAL, "unknown option '%s'", name);
  *slot = value;
  return EMPOSE_OK;
}

int empose_get_option(const char* name) {
  const int* slot = name ? option_slot(name) : nullptr;
  return slot ? *slot : -1;
}

size_t empose_pack_weight_x3_bytes(int N, int K) {
  if (N <= 0 || K <= 0) return 0;
  return pack_x3_elems(N, K) * sizeof(unsigned short);
}

int empose_pack_weight_x3(const float* W, int ldw, int N, int K, void* out, empose_stream_t stream_) {
  if (!W || !out) return fail(EMPOSE_EINVAL, "null argument");
  if (N <= 0 || K <= 0 || K % 4 != 0 || ldw < K) return fail(EMPOSE_EINVAL, "bad sizes");
  HIP_CHECK(launch_pack_x3(W, ldw, N, K, static_cast<unsigned short*>(out), static_cast<hipStream_t>(stream_)), "weight pack");
  return EMPOSE_OK;
}

int empose_async_status(void) {
  if (const unsigned n = poll_timeouts_take())
    return fail(EMPOSE_ETIMEOUT, "%u poll(s) of a cooperative kernel (whole-sequence LSTM / one-launch training layer) timed out waiting for another workgroup's exchange "
                "word; the outputs of that call are NaN", n);
  return EMPOSE_OK;
}

int empose_reset_options(void) {
  options() = Options{};
  return EMPOSE_OK;
}

int empose_version(void) { return 3; }   // 2: empose_lgd_io gained suppress_missing / mask_value; 3 (round 6): empose_mlp_params gained
                                         // weight_x3 / weight_t_x3, empose_lstm_grads gained d_h0 / d_c0 (appended fields)
const char* empose_arch(void) { return "gfx950"; }

int empose_profile_enable(int on) {
  g_prof.on = on != 0;
  g_prof.only = -1;
  g_prof.used = 0;
  g_prof.tags.clear();
  return EMPOSE_OK;
}

int empose_profile_enable_only(const char* tag_name) {
  if (!tag_name) return fail(EMPOSE_EINVAL, "null tag name");
  for (int i = 0; i < P_NTAGS; ++i)
    if (std::strcmp(tag_name, kProfNames[i]) == 0) {
      g_prof.on = true;
      g_prof.only = i;
      g_prof.used = 0;
      g_prof.tags.clear();
      return EMPOSE_OK;
    }
  return fail(EMPOSE_EINVAL, "unknown profile tag '%s'", tag_name);
}

int empose_profile_ntags(void) { return P_NTAGS; }

const char* empose_profile_tag_name(int tag) { return (tag >= 0 && tag < P_NTAGS) ? kProfNames[tag] : ""; }

const char* empose_profile_gemm_kernel_name(int M, int N, int K, int count, int role) {
  return gemm_kernel_name(M, N, K, count < 1 ? 1 : (count > 2 ? 2 : count), role);
}

int empose_profile_read(double* total_ms, long long* count) {
  if (!total_ms || !count) return fail(EMPOSE_EINVAL, "null argument");
  for (int i = 0; i < P_NTAGS; ++i) { total_ms[i] = 0.0; count[i] = 0; }
  if (g_prof.used == 0) return EMPOSE_OK;
  HIP_TRY(hipEventSynchronize(g_prof.ev[g_prof.used - 1]));
  for (size_t i = 0; i + 1 < g_prof.used; ++i) {
    const int tag = g_prof.tags[i];
    if (tag == P_END) continue;  // gap between two forwards
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, g_prof.ev[i], g_prof.ev[i + 1]));
    total_ms[tag] += ms;
    count[tag] += 1;
  }
  g_prof.used = 0;
  g_prof.tags.clear();
  return EMPOSE_OK;
}

}  // extern "C"
