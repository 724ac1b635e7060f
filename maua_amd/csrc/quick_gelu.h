// QuickGELU (clip/model.py: x * sigmoid(1.702 x)) and its derivative s + 1.702 x s (1 - s), one definition for every kernel that
// applies them: transformer.hip's element-wise kernels and gemm_dma.hip's GEMM epilogues (GemmArgs.epi).  Both sides call the same inline
// expression, so a fused epilogue and the separate kernel give the same bits by construction.  exact: expf (f32 networks) or __expf
// (bf16 networks).
#pragma once

#include <hip/hip_runtime.h>

namespace maua {

__device__ __forceinline__ float sigmoid_f(float x, bool exact) { return 1.f / (1.f + (exact ? expf(-x) : __expf(-x))); }
__device__ __forceinline__ float quick_gelu_f(float v, bool exact) { return v * sigmoid_f(1.702f * v, exact); }
__device__ __forceinline__ float quick_gelu_grad_f(float v, bool exact) {
  const float s = sigmoid_f(1.702f * v, exact);
  return s * (1.f + 1.702f * v * (1.f - s));
}

}  // namespace maua
