// Launch support every kernel family shares (api.hip): the poll-timeout word of the cooperative kernels, dynamic LDS above
// 64 KB, co-residency.  Internal, not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace empose {

// Dynamic LDS above the 64 KB a kernel may use by default: hipFuncAttributeMaxDynamicSharedMemorySize of `fn` on the
// CURRENT device, raised when `bytes` exceeds what was already allowed there (cached per (device, kernel): a process that
// drives several GPUs sets it on each).  More than a CU has (LDS_BYTES_PER_CU) is refused here instead of at the launch.
// The cooperative whole-sequence LSTM kernels poll exchange words written by other workgroups; a poll that exceeds its
// spin limit gives up, poisons the outputs with NaN (it does not hang) and counts itself in ONE host-mapped word that the
// entry points read without synchronising: the next empose_* call that runs a recurrence returns EMPOSE_ETIMEOUT, and
// empose_async_status() reports it to a caller that has synchronised.  Option "spin_limit" (0 = the kernels' own limits)
// forces a limit, for tests.
unsigned* poll_timeout_word();          // device-visible address of the counter
unsigned poll_timeouts_take();          // host: read and clear
unsigned poll_timeouts_peek();          // host: read
int poll_spin_limit(int kernel_default);   // option "spin_limit" where it is set, else the polling kernel's own limit
constexpr size_t LDS_BYTES_PER_CU = 160 * 1024;
hipError_t allow_dynamic_lds(const void* fn, size_t bytes);
// A launch of a kernel with a large dynamic-LDS request: raises the limit of `fn` (above), launches, returns the launch's
// error.  `args` convert to the kernel's parameter types here, as they would at a direct launch.
template <typename... Params, typename... Args>
inline hipError_t launch_lds(void (*fn)(Params...), dim3 grid, dim3 block, size_t lds_bytes, hipStream_t stream,
                             const Args&... args) {
  if (hipError_t e = allow_dynamic_lds(reinterpret_cast<const void*>(fn), lds_bytes)) return e;
  hipLaunchKernelGGL(fn, grid, block, lds_bytes, stream, static_cast<Params>(args)...);
  return hipGetLastError();
}
// Workgroups of `fn` (block size `threads`, `lds_bytes` of dynamic LDS) that can be resident at once on the CURRENT device:
// what a cooperative launch may ask for.  Cached per (device, kernel); the attribute above is set on the way.
hipError_t coresident_blocks(const void* fn, int threads, size_t lds_bytes, int* blocks);

}  // namespace empose
