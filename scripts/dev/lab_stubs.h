// What the stand-alone labs need from api.hip (options, dynamic LDS, co-residency, the poll-timeout word) when they
// #include a production kernel file directly.
#pragma once
#include "../../em_pose_amd/csrc/launch.h"
#include "../../em_pose_amd/csrc/options.h"
namespace empose {
#ifndef EMPOSE_LAB_HAS_OPTIONS
Options& options() { static Options o; return o; }
#endif
hipError_t allow_dynamic_lds(const void* fn, size_t bytes) {
  return hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}
hipError_t coresident_blocks(const void* fn, int threads, size_t lds, int* blocks) {
  if (hipError_t e = allow_dynamic_lds(fn, lds)) return e;
  int per_cu = 0, dev = 0;
  hipDeviceProp_t prop;
  (void)hipGetDevice(&dev);
  (void)hipGetDeviceProperties(&prop, dev);
  hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, threads, lds);
  *blocks = per_cu * prop.multiProcessorCount;
  return e;
}
unsigned* poll_timeout_word() { static unsigned* p = nullptr; if (!p) (void)hipMalloc(&p, 64); return p; }
int poll_spin_limit(int kernel_default) { return options().spin_limit > 0 ? options().spin_limit : kernel_default; }
unsigned poll_timeouts_take() { return 0; }
unsigned poll_timeouts_peek() { return 0; }
}  // namespace empose
