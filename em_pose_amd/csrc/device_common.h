// Small device helpers that more than one kernel file uses: the LSTM cell's gate non-linearities and the
// instruction-group masks of sched_group_barrier.  Internal, gfx950 only.
#pragma once
#include <hip/hip_runtime.h>

namespace empose {

// Fast cell non-linearities: v_exp_f32 / v_rcp_f32 (about 1 ulp each); absolute error ~1e-7, far inside the 1e-4 parity
// budget, and the unit finish is no longer a visible fraction of the launch.
__device__ __forceinline__ float fast_sigmoid(float x) { return __builtin_amdgcn_rcpf(1.f + __expf(-x)); }
__device__ __forceinline__ float fast_tanh(float x) { return 1.f - 2.f * __builtin_amdgcn_rcpf(1.f + __expf(2.f * x)); }

// SGB(mask, n): the next n instructions of the groups in `mask` are scheduled here, in program order of the SGB calls.
constexpr int SG_VALU = 0x002, SG_MFMA = 0x008, SG_VMEM_RD = 0x020, SG_DS_RD = 0x100, SG_DS_WR = 0x200;
#define SGB(mask, n) __builtin_amdgcn_sched_group_barrier(mask, n, 0)

}  // namespace empose
