// The matrix-core operand trait of the convolution, GEMM and attention kernels, and the split-f32 operand format.
//
// Mma<T>::step(acc, a, b) is one 32-byte K-step of a 32 x 32 accumulator block: v_mfma_f32_32x32x16_{bf16,f16} for the 16-bit formats
// (16 k), four v_mfma_f32_32x32x2_f32 for float (exact f32 parity mode, 8 k).  Both operands are raw 16-byte register quads, read as
// identical 16-byte-per-lane LDS fragments whatever T is.  Mma<T>::scale(v, sv) multiplies a 16-byte piece of T by the f32 styles of
// its channels (sv: 8 values for the 16-bit formats, 4 for the 32-bit ones) and rounds to nearest even - the modulation of the
// kernels that stage x * s themselves.
#pragma once
#include "common.h"

namespace maua {

// MAUA_F32_SPLIT: float32 tensors, products on the bf16 matrix cores.  x = hi + lo, hi = bf16(x) (round to nearest even),
// lo = bf16(x - hi) (x - hi is exact in f32).  Every aligned group of 8 floats (two 16-byte pieces: what the two lane halves of one
// k-step hold) is kept in LDS - and, for the weights, in HBM: launch_f32_split_inplace after launch_prep_weights - as
// [hi0 .. hi7 | lo0 .. lo7] bf16: piece 2 j = the eight hi parts, piece 2 j + 1 = the eight lo parts.  The pixel side is split ONCE
// per element when the halo tile is staged (scale() + one exchange between the two lanes that hold a group); a k-step of the
// convolution is then three full v_mfma_f32_32x32x16_bf16 over 16 real k:
//     w_hi x_hi  +  w_hi x_lo  +  w_lo x_hi          (w_lo x_lo, <= 2^-16 of the product, is dropped)
// 96 matrix-core cycles per 16 k where the exact path's eight v_mfma_f32_32x32x2_f32 take 512 (a first form with [hi x 4 | lo x 4] per
// piece spent one of four operand slots on zeros: 128 cycles).
__device__ __forceinline__ u32x4 f32_split4(const f32x4& f) {
  const uint32_t h0 = pack2bf(f[0], f[1]), h1 = pack2bf(f[2], f[3]);
  return u32x4{h0, h1, pack2bf(f[0] - __uint_as_float(h0 << 16), f[1] - __uint_as_float(h0 & 0xffff0000u)),
               pack2bf(f[2] - __uint_as_float(h1 << 16), f[3] - __uint_as_float(h1 & 0xffff0000u))};
}
// {hi x 4 | lo x 4} of this lane's piece q and of lane ^ 1's piece q ^ 1 -> this lane's piece of the group format above
__device__ __forceinline__ u32x4 f32_split_pair(const u32x4& v, int q) {
  const bool odd = q & 1;
  const uint32_t r0 = __shfl_xor(odd ? v[0] : v[2], 1), r1 = __shfl_xor(odd ? v[1] : v[3], 1);   // even lanes receive hi, odd lanes lo
  return odd ? u32x4{r0, r1, v[2], v[3]} : u32x4{v[0], v[1], r0, r1};
}
template <typename T> struct IsSplit { static constexpr bool value = false; };
template <> struct IsSplit<f32s_t> { static constexpr bool value = true; };

template <typename T> struct Mma;
template <> struct Mma<bf16_t> {
  __device__ static __forceinline__ void step(f32x16& acc, const u32x4& a, const u32x4& b) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), acc, 0, 0, 0);
  }
  // scale 8 bf16 by 8 f32 styles, round to nearest even
  __device__ static __forceinline__ u32x4 scale(const u32x4& v, const float* sv) {
    u32x4 o;
#pragma unroll
    for (int k = 0; k < 4; k++)
      o[k] = pack2bf(bf2f((bf16_t)(v[k] & 0xffff)) * sv[2 * k], bf2f((bf16_t)(v[k] >> 16)) * sv[2 * k + 1]);
    return o;
  }
};
template <> struct Mma<f16_t> {
  __device__ static __forceinline__ void step(f32x16& acc, const u32x4& a, const u32x4& b) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), acc, 0, 0, 0);
  }
  // scale 8 halves by 8 f32 styles, round to nearest even (the styles arrive pre-normalised, |s| <= 1: the product cannot overflow)
  __device__ static __forceinline__ u32x4 scale(const u32x4& v, const float* sv) {
    u32x4 o;
#pragma unroll
    for (int k = 0; k < 4; k++) o[k] = pack2h(Fmt16<f16_t>::lo(v[k]) * sv[2 * k], Fmt16<f16_t>::hi(v[k]) * sv[2 * k + 1]);
    return o;
  }
};
template <> struct Mma<float> {
  // lane half h holds k = 8j+4h+e (e = 0..3): MFMA e consumes element e of both operands, so A and B see the
  // same K permutation and the sum is over the same set of products.
  __device__ static __forceinline__ void step(f32x16& acc, const u32x4& a, const u32x4& b) {
    f32x4 af = __builtin_bit_cast(f32x4, a), bf = __builtin_bit_cast(f32x4, b);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af[0], bf[0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af[1], bf[1], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af[2], bf[2], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af[3], bf[3], acc, 0, 0, 0);
  }
  __device__ static __forceinline__ u32x4 scale(const u32x4& v, const float* sv) {
    f32x4 f = __builtin_bit_cast(f32x4, v);
    f[0] *= sv[0]; f[1] *= sv[1]; f[2] *= sv[2]; f[3] *= sv[3];
    return __builtin_bit_cast(u32x4, f);
  }
};
template <> struct Mma<f32s_t> {
  __device__ static __forceinline__ void step(f32x16& acc, const u32x4& w, const u32x4& x) {   // (one of the three products of a k-step)
    Mma<bf16_t>::step(acc, w, x);
  }
  // the halo tile's 4 floats x 4 styles -> {hi x 4 | lo x 4} (the staging code then exchanges halves with the neighbouring lane)
  __device__ static __forceinline__ u32x4 scale(const u32x4& v, const float* sv) {
    return f32_split4(__builtin_bit_cast(f32x4, Mma<float>::scale(v, sv)));
  }
};

}  // namespace maua
