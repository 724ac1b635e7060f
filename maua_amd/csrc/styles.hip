// Styles and demodulation coefficients of every layer of a synthesis network, two launches per batch.
//
// Replaces (reference): stylegan2.py:48-58, :230, :269 (the affine layers that turn w into per-layer styles), ops.py:168-171 (the
// demodulation coefficients) and :161-165 (the styles half of the FP16 pre-normalisation); toRGB layers get their pre-modulated weights.
#include "common.h"
#include "internal.h"

namespace maua {

// Two launches per batch for ALL layers (17 conv + 9 toRGB at 1024^2): (1) s = affine(w) (stylegan2.py:48-58,:230,
// :269), (2) demod coefficients (ops.py:168-171) / pre-modulated toRGB weights.  Both are small GEMMs
// out[row][sample] = sum_k M[row][k] * vec[sample][k] (rows = channels, <= 32 samples per pass), done with the exact
// f32 MFMA (v_mfma_f32_32x32x2_f32): a workgroup owns 32 matrix rows of one layer for all samples, its 4 waves split
// K and reduce through LDS.  A sample is a column of the MFMA, so its arithmetic does not depend on where it sits in
// the batch (frames stay bit-identical under any batching / sharding).
//   lane (r = l & 31, h = l >> 5) feeds M[row0 + r][k8 + 4h + v] and vec[n = r][k8 + 4h + v] to MFMA number v of
//   the 8-column block k8: one float4 load per operand per lane per block.
template <typename VecLoad, typename Store>
__device__ __forceinline__ void rows_times_samples(const float* __restrict__ M, int K, int row0, int rows_valid, int B,
                                                   VecLoad vec_load, Store store, float* red /* LDS [4][16][64] */) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int kq = (K / 4 + 7) / 8 * 8;  // K columns per wave, a multiple of the 8-column block
  const int k_lo = wave * kq, k_hi = min(K, k_lo + kq);
  const bool row_ok = r < rows_valid;
  const float* mrow = M + (long)(row0 + (row_ok ? r : 0)) * K;
  for (int b0 = 0; b0 < B; b0 += 32) {
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; e++) acc[e] = 0.f;
    const bool smp_ok = b0 + r < B;
#pragma unroll 4
    for (int k8 = k_lo; k8 < k_hi; k8 += 8) {
      const int k = k8 + 4 * h;
      float4 a = make_float4(0.f, 0.f, 0.f, 0.f), v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (row_ok && k < K) a = *reinterpret_cast<const float4*>(mrow + k);
      if (smp_ok && k < K) v = vec_load(b0 + r, k);
      // (the raw builtin, not Mma<float>::step of mma.h: the operands are float4 members here, and going through a 16-byte register
      // quad changes this kernel's register allocation)
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, v.x, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, v.y, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, v.z, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, v.w, acc, 0, 0, 0);
    }
    // K-split reduction, fixed order wave 0 + 1 + 2 + 3
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 16; e++) red[(wave * 16 + e) * 64 + lane] = acc[e];
    __syncthreads();
    if (wave == 0) {
#pragma unroll
      for (int e = 0; e < 16; e++) {
        const float t = ((red[e * 64 + lane] + red[(16 + e) * 64 + lane]) + red[(32 + e) * 64 + lane]) + red[(48 + e) * 64 + lane];
        const int row = (e & 3) + 8 * (e >> 2) + 4 * h;  // D layout: lane = column (sample), 16 rows per lane
        if (row < rows_valid && smp_ok) store(b0 + r, row0 + row, t);
      }
    }
  }
}

__global__ __launch_bounds__(256) void styles_affine_kernel(const StyleLayer* __restrict__ layers,
                                                            const float* __restrict__ ws, int num_ws, int w_dim, int B) {
  __shared__ float red[4 * 16 * 64];
  const StyleLayer L = layers[blockIdx.x];
  const int c0 = blockIdx.y * 32;
  if (c0 >= L.Cs) return;
  const float wgain = rsqrtf((float)w_dim);
  const float* wbase = ws + (long)L.w_index * w_dim;
  const long wstride = (long)num_ws * w_dim;
  rows_times_samples(
      L.affine_w, w_dim, c0, min(32, L.Cin - c0), B,
      [&](int b, int k) { return *reinterpret_cast<const float4*>(wbase + b * wstride + k); },
      [&](int b, int ci, float t) { L.s[(long)b * L.Cs + ci] = (t * wgain + L.affine_b[ci]) * L.scale; }, red);
  // channel padding of the styles buffer
  for (int i = threadIdx.x; i < B * 32; i += blockDim.x) {
    const int b = i >> 5, ci = c0 + (i & 31);
    if (ci >= L.Cin && ci < L.Cs) L.s[(long)b * L.Cs + ci] = 0.f;
  }
}

__global__ __launch_bounds__(256) void styles_demod_kernel(const StyleLayer* __restrict__ layers, int B) {
  __shared__ float red[4 * 16 * 64];
  const StyleLayer L = layers[blockIdx.x];
  if (L.d) {
    const int c0 = blockIdx.y * 32;
    if (c0 >= L.Cd) return;
    rows_times_samples(
        L.wsq, L.Cin, c0, min(32, L.Co - c0), B,
        [&](int b, int k) {
          const float4 v = *reinterpret_cast<const float4*>(L.s + (long)b * L.Cs + k);
          return make_float4(v.x * v.x, v.y * v.y, v.z * v.z, v.w * v.w);
        },
        [&](int b, int co, float t) { L.d[(long)b * L.Cd + co] = rsqrtf(t + 1e-8f); }, red);
    for (int i = threadIdx.x; i < B * 32; i += blockDim.x) {
      const int b = i >> 5, co = c0 + (i & 31);
      if (co >= L.Co && co < L.Cd) L.d[(long)b * L.Cd + co] = 0.f;
    }
  } else if (L.wmod) {
    const int n = B * 3 * L.Cin;
    for (int i = blockIdx.y * blockDim.x + threadIdx.x; i < n; i += gridDim.y * blockDim.x) {
      const int b = i / (3 * L.Cin), r = i - b * 3 * L.Cin;
      L.wmod[i] = L.wrgb[r] * L.s[(long)b * L.Cs + (r % L.Cin)];
    }
  }
}

// the styles half of the FP16 pre-normalisation (ops.py:161-165; the weight half and what the pair buys: modconv_prep.hip)
// one wave per (layer, sample): s[b][0 .. Cin) /= max |s[b][.]|, for the layers that demodulate (L.d != NULL)
__global__ __launch_bounds__(64) void f16_prenorm_styles_kernel(const StyleLayer* __restrict__ layers, int B) {
  const StyleLayer L = layers[blockIdx.x];
  if (!L.d) return;
  float* sp = L.s + (long)blockIdx.y * L.Cs;
  float m = 0.f;
  for (int i = threadIdx.x; i < L.Cin; i += 64) m = fmaxf(m, fabsf(sp[i]));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  for (int i = threadIdx.x; i < L.Cin; i += 64) sp[i] = sp[i] / m;
}
// the same for one plain styles tensor [B][Cs] (operator-level entry point)
__global__ __launch_bounds__(64) void f16_prenorm_styles_plain_kernel(float* __restrict__ s, int Cs, int Cin) {
  float* sp = s + (long)blockIdx.x * Cs;
  float m = 0.f;
  for (int i = threadIdx.x; i < Cin; i += 64) m = fmaxf(m, fabsf(sp[i]));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  for (int i = threadIdx.x; i < Cin; i += 64) sp[i] = sp[i] / m;
}
int launch_f16_prenorm_styles(hipStream_t stream, float* s, int B, int Cs, int Cin) {
  if (B == 0) return MAUA_OK;
  hipLaunchKernelGGL(f16_prenorm_styles_plain_kernel, dim3(B), dim3(64), 0, stream, s, Cs, Cin);
  MAUA_HIP_CHECK(hipGetLastError());
  return MAUA_OK;
}

int launch_styles(hipStream_t stream, const StyleLayer* layers_dev, int n_layers, const float* ws, int num_ws,
                  int w_dim, int B, int max_channels, int f16_prenorm) {
  if (B == 0 || n_layers == 0) return MAUA_OK;
  MAUA_REQUIRE(w_dim % 4 == 0 && max_channels % 4 == 0, "styles: w_dim and channel counts must be multiples of 4");
  const int ny = cdiv(std::max(max_channels, 32), 32);
  hipLaunchKernelGGL(styles_affine_kernel, dim3(n_layers, ny), dim3(256), 0, stream, layers_dev, ws, num_ws, w_dim, B);
  if (f16_prenorm) hipLaunchKernelGGL(f16_prenorm_styles_kernel, dim3(n_layers, B), dim3(64), 0, stream, layers_dev, B);
  hipLaunchKernelGGL(styles_demod_kernel, dim3(n_layers, ny), dim3(256), 0, stream, layers_dev, B);
  MAUA_HIP_CHECK(hipGetLastError());
  return MAUA_OK;
}

}  // namespace maua
