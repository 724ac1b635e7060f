// The float64 matrix-core fragment maps (v_mfma_f64_16x16x4_f64).  Kept apart from mma.h on purpose: the Mma<T> trait there encodes the
// 32 x 32 C/D map that every other format shares, and the f64 instruction does not use it.
//
//   A operand: one f64 per lane, A[row = lane & 15][k = lane >> 4]
//   B operand: one f64 per lane, B[k = lane >> 4][col = lane & 15]
//   C / D:     four f64 per lane, D[row = (lane >> 4) + 4 r][col = lane & 15],  r = 0 .. 3
#pragma once
#include "common.h"

namespace maua {

typedef __attribute__((ext_vector_type(4))) double f64x4;

struct MmaF64 {
  static constexpr int kM = 16, kN = 16, kK = 4;
  __device__ static __forceinline__ int a_row(int lane) { return lane & 15; }
  __device__ static __forceinline__ int b_col(int lane) { return lane & 15; }
  __device__ static __forceinline__ int k_of(int lane) { return lane >> 4; }
  __device__ static __forceinline__ int d_row(int lane, int r) { return (lane >> 4) + 4 * r; }
  __device__ static __forceinline__ int d_col(int lane) { return lane & 15; }
  __device__ static __forceinline__ void step(f64x4& acc, double a, double b) {
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
  }
};

}  // namespace maua
