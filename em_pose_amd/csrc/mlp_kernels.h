// Launch interfaces of the fused update MLPs (mlp_fused.hip, mlp_fused_x3.hip).  Internal, not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>

namespace empose {

// One or two whole MLPs (all layers) in one launch: a workgroup keeps the activations of 64 rows in LDS from the first
// layer to the last (mlp_fused.hip).
constexpr int FUSED_MAX_LAYERS = 8;
constexpr int FUSED_MAX_WIDTH = 512;     // widest layer output the four 128-column waves cover
struct FusedLayer {
  const float* W; int K, N;              // weights in fragment order (api_model.hip pack_fragments), K % 4 == 0, N <= FUSED_MAX_WIDTH
  const float* scale; const float* shift;
  float slope; int act;                  // 0 none, 1 PReLU
  const float* wexp = nullptr;           // pair16 only: [N] the inverse of the power-of-two scale W's columns were packed with
};
struct FusedNet {
  const float* x; int ldx;
  float* out; int ld_out;
  int n_layers;                          // the last layer writes `out`, the others stay in LDS
  FusedLayer layer[FUSED_MAX_LAYERS];
};
struct FusedMlpArgs { FusedNet net[2]; int count; int M; };
hipError_t launch_mlp_fused(const FusedMlpArgs& args, hipStream_t stream);
// The form the products of that launch take, and with it the order FusedLayer::W is packed in (api_model.hip
// pack_fragments keeps one table per form):
//   fp32    the fp32 MFMA instruction (mlp_fused.hip, launch_mlp_fused);
//   x3_32   three bf16 pieces per operand on v_mfma_f32_32x32x16_bf16, six products (mlp_fused_x3_kernel<32>);
//   x3_16   the same pieces on v_mfma_f32_16x16x32_bf16 (mlp_fused_x3_kernel<16>);
//   pair16  two f16 pieces per operand under power-of-two scales on v_mfma_f32_16x16x32_f16, three products
//           (mlp_fused_x3_kernel<PAIR16>, f16pair.h), FusedLayer::wexp set.
enum class FusedForm { fp32, x3_32, x3_16, pair16 };
constexpr int FUSED_FORMS = 4;
// The same launch in one of the piece forms (mlp_fused_x3.hip; `form` is not fp32).  Hidden widths must be multiples of 64.
hipError_t launch_mlp_fused_x3(const FusedMlpArgs& args, FusedForm form, hipStream_t stream);

}  // namespace empose
