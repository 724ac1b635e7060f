// Weight preparation for the modulated convolutions of modconv.hip and its siblings: the per-tap (and, for up = 2, per-phase) weight
// planes with the squared-weight sums the demodulation needs, the in-place split of a prepared float32 buffer (MAUA_F32_SPLIT, mma.h)
// and the weight half of the reference's FP16 pre-normalisation.
//
// Replaces (reference): the weight side of ops.py:146-186 modulated_conv2d (:161-165 pre-normalisation, :168-171 the sum of squares
// under the demodulation) and of :189-233 conv2d_resample's up = 2 branch (flip, transposed convolution, 4x4 FIR folded into phase kernels).
#include "common.h"
#include "internal.h"
#include "mma.h"

namespace maua {

// f32 [Co][Ci][k][k] -> T [k*k][phases][Cop][Cip] (zero padded; the phase is part of a 'virtual' output-channel
// index n_v = phase*Cop + co, so one workgroup can produce several output parities from one input halo) and
// Wsq[co][ci] = sum_taps W^2.
// up == 2 (k == 3): phase kernels from K = full_conv2d(flip(W), 4f), f = outer([1,3,3,1])/64.
template <typename T>
__global__ __launch_bounds__(256) void prep_weights_kernel(const float* __restrict__ w, T* __restrict__ wt,
                                                           float* __restrict__ wsq, int Co, int Ci, int k, int up,
                                                           int flip, int Cop, int Cip) {
  long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)Cop * Cip) return;
  int co = (int)(idx / Cip), ci = (int)(idx - (long)co * Cip);
  const int kk = k * k;
  float wv[9];
  bool real = co < Co && ci < Ci;
  float sq = 0.f;
  for (int t = 0; t < kk; t++) {
    wv[t] = real ? w[((long)co * Ci + ci) * kk + t] : 0.f;
    sq += wv[t] * wv[t];
  }
  if (wsq && real) wsq[(long)co * Ci + ci] = sq;
  const long plane = (long)Cop * Cip;
  if (up == 1) {
    for (int t = 0; t < kk; t++) Elem<T>::store(wt + (long)t * plane + idx, wv[t]);
    return;
  }
  // up == 2, k == 3
  const float g4[4] = {0.25f, 0.75f, 0.75f, 0.25f};  // 2 * [1,3,3,1]/8 per axis  (4f = outer(g4, g4))
  float K[6][6];
  for (int u = 0; u < 6; u++)
    for (int v = 0; v < 6; v++) {
      float s = 0.f;
      for (int i = 0; i < 3; i++) {
        int fu = u - i;
        if (fu < 0 || fu > 3) continue;
        for (int j = 0; j < 3; j++) {
          int fv = v - j;
          if (fv < 0 || fv > 3) continue;
          // A = flip(W) in-tree (no flip before the transposed conv), A = W under nv_compat
          float aij = flip ? wv[i * 3 + j] : wv[(2 - i) * 3 + (2 - j)];
          s += aij * g4[fu] * g4[fv];
        }
      }
      K[u][v] = s;
    }
  for (int pa = 0; pa < 2; pa++)
    for (int pb = 0; pb < 2; pb++)
      for (int ky = 0; ky < 3; ky++)
        for (int kx = 0; kx < 3; kx++) {
          int ph = pa * 2 + pb, t = ky * 3 + kx;
          Elem<T>::store(wt + ((long)t * 4 + ph) * plane + idx, K[2 * ky + 1 - pa][2 * kx + 1 - pb]);
        }
}

size_t prepped_weight_elems(int k, int up, int Cop, int Cip) { return (size_t)up * up * k * k * Cop * Cip; }

int launch_prep_weights(hipStream_t stream, int dtype, const float* w, void* wt, float* wsq, int Co, int Ci, int k,
                        int up, int flip, int Cop, int Cip) {
  MAUA_REQUIRE(k == 1 || k == 3, "prep_weights: kernel size must be 1 or 3");
  MAUA_REQUIRE(up == 1 || (up == 2 && k == 3), "prep_weights: up=2 needs a 3x3 kernel");
  long n = (long)Cop * Cip;
  dim3 grid((unsigned)((n + 255) / 256));
  return dispatch_dtype<bf16_t, f16_t, float>(dtype, "prep_weights", [&](auto t) {
    hipLaunchKernelGGL(prep_weights_kernel<decltype(t)>, grid, dim3(256), 0, stream, w, (decltype(t)*)wt, wsq, Co, Ci, k, up, flip, Cop, Cip);
    MAUA_HIP_CHECK(hipGetLastError());
    return MAUA_OK;
  });
}

// dst[i][o][k] = src[o][i][kk - 1 - k]: a convolution's (kk = 9) / linear layer's (kk = 1) weight for its input gradient
__global__ __launch_bounds__(256) void transpose_flip_kernel(const float* __restrict__ src, float* __restrict__ dst, int Co, int Ci, int kk) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)Co * Ci * kk) return;
  const int k = (int)(idx % kk);
  const long oi = idx / kk;
  const int i = (int)(oi % Ci), o = (int)(oi / Ci);
  dst[((long)i * Co + o) * kk + (kk - 1 - k)] = src[idx];
}
int launch_transpose_flip(hipStream_t stream, const float* w, float* w_t, int Co, int Ci, int kk) {
  const long n = (long)Co * Ci * kk;
  if (n == 0) return MAUA_OK;
  hipLaunchKernelGGL(transpose_flip_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, w, w_t, Co, Ci, kk);
  MAUA_HIP_CHECK(hipGetLastError());
  return MAUA_OK;
}

// a prepared float32 weight buffer (launch_prep_weights, MAUA_F32) -> the split form above, in place: n floats, n % 8 == 0 (K, the
// innermost dimension, is a multiple of 32 channels)
__global__ __launch_bounds__(256) void f32_split_inplace_kernel(float* __restrict__ w, long n8) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n8) return;
  const u32x4 a = f32_split4(*reinterpret_cast<const f32x4*>(w + 8 * i)), b = f32_split4(*reinterpret_cast<const f32x4*>(w + 8 * i + 4));
  *reinterpret_cast<u32x4*>(w + 8 * i) = u32x4{a[0], a[1], b[0], b[1]};        // hi of floats 0 .. 7
  *reinterpret_cast<u32x4*>(w + 8 * i + 4) = u32x4{a[2], a[3], b[2], b[3]};    // lo of floats 0 .. 7
}
int launch_f32_split_inplace(hipStream_t stream, void* w, long n) {
  MAUA_REQUIRE(w && n >= 0 && n % 8 == 0, "f32_split_inplace: bad argument");
  if (n == 0) return MAUA_OK;
  hipLaunchKernelGGL(f32_split_inplace_kernel, dim3((unsigned)((n / 8 + 255) / 256)), dim3(256), 0, stream, (float*)w, n / 8);
  MAUA_HIP_CHECK(hipGetLastError());
  return MAUA_OK;
}

// ---- ops.py:161-165, the FP16 pre-normalisation of a demodulated convolution ("Pre-normalize inputs to avoid FP16 overflow"):
//   weight = weight / (amax |weight| over (ci, ky, kx) per output channel * sqrt(Ci k k));  styles = styles / amax |styles| per sample
// Demodulation makes the layer's output invariant to both factors (up to its 1e-8); what they buy is range: with |s| <= 1 the
// modulated activation x * s, which this library rounds to the network dtype, cannot leave the half range when x did not.
// One workgroup per output channel
__global__ __launch_bounds__(256) void f16_prenorm_weights_kernel(const float* __restrict__ w, float* __restrict__ out, int row,
                                                                  float rsqrt_fan) {
  __shared__ float red[4];
  const float* src = w + (long)blockIdx.x * row;
  float m = 0.f;
  for (int i = threadIdx.x; i < row; i += 256) m = fmaxf(m, fabsf(src[i]));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  const float k = rsqrt_fan / m;   // (an all-zero channel divides by zero, as the reference does)
  for (int i = threadIdx.x; i < row; i += 256) out[(long)blockIdx.x * row + i] = src[i] * k;
}
int launch_f16_prenorm_weights(hipStream_t stream, const float* w, float* out, int Co, int Ci, int kk) {
  if (Co == 0) return MAUA_OK;
  hipLaunchKernelGGL(f16_prenorm_weights_kernel, dim3(Co), dim3(256), 0, stream, w, out, Ci * kk, 1.f / sqrtf((float)(Ci * kk)));
  MAUA_HIP_CHECK(hipGetLastError());
  return MAUA_OK;
}

}  // namespace maua
