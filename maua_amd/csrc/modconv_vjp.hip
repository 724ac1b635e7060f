// The gradient of one StyleGAN2 synthesis layer to its input and its styles (maua_modconv_vjp_ex, maua_torgb_vjp_ex, and what
// synth_vjp.hip's walk launches).  No reference counterpart in code: the reference gets these from torch.autograd on
// inference/ops.py:146-186 modulated_conv2d + :65-84 bias_act (sampling/langevin.py differentiates the generator through them).
//
// Forward (maua_modconv_ex), NHWC, s = styles, d = demodulation coefficients:
//   u = conv(W, s x)     up 1: 3x3 correlation, pad 1;  up 2: conv_transpose(stride 2) -> t [2H + 1][2W + 1], then the [1, 3, 3, 1] FIR (gain 4)
//   v = d u + noise strength + bias,   y = clamp(lrelu(v) gain)
// Backward from g_y and the KEPT y (u is not kept; where the gradient passes the epilogue is invertible):
//   act_vjp      g_v = g_y gain (y > 0 ? 1 : alpha) (|y| < clamp);  u = (lrelu^-1(y / gain) - noise strength - bias) / d;
//                g_u = d g_v (stored in the network dtype);  chunk sums of g_d[b][co] = sum_p g_v u
//   fir_adjoint  up 2: g_t = FIR^T g_u (pad 2, the same symmetric filter: [2H] -> [2H + 1])
//   conv_vjp     g_xm[p][ci] = sum_{t, co} Wg[t][ci][co] src[p'(p, t)][co] on the matrix cores (Mma<T>: bf16 or exact f32), f32 out.
//                up 1: src = g_u, p' = p + 1 - tap (zero outside);  up 2: src = g_t, p' = 2 p + tap - the stride-2 implicit GEMM,
//                M = H W pixels, N = Ci, K = 9 Co per sample
//   finish       g_x (+)= s g_xm;  chunk sums of sum_p x g_xm
//   finalize     g_s[b][ci] = sum_p x g_xm - s[b][ci] sum_co g_d d^3 Wsq[co][ci]
// Every reduction is two fixed-order stages (a chunk's 8 pixel lanes, then the chunks): two calls give the same bits, no atomics.
#include <algorithm>

#include "common.h"
#include "internal.h"
#include "mma.h"

namespace maua {
namespace {

// pixels per reduction chunk: at most ~1024 chunks per sample, at least 64 pixels each, whole groups of the 8 pixel lanes
int vjp_ppc(long P) { return (int)((std::max<long>(64, (P + 1023) / 1024) + 7) / 8 * 8); }
int vjp_nchunk(long P) { return (int)((P + vjp_ppc(P) - 1) / vjp_ppc(P)); }

// grid (chunks, Co / 32, B); thread = (pixel lane 0 .. 7, channel 0 .. 31).  GN: also npart[b][group][p] = sum of g_v over the group's 32
// channels (a pixel's channels are the 32 lanes of half a wave: five xor steps, the same tree every time), the gradient to the noise
// before the sum over the groups (noise_grad_kernel)
template <typename T, bool GN>
__global__ __launch_bounds__(256) void act_vjp_kernel(const T* __restrict__ y, const T* __restrict__ g_y, const float* __restrict__ d,
                                                      const float* __restrict__ noise, long noise_bstride, float strength,
                                                      const float* __restrict__ bias, T* __restrict__ g_u, float* __restrict__ part,
                                                      float* __restrict__ npart, int P, int Co, int ppc, int act, float alpha, float gain,
                                                      float clamp) {
  __shared__ float red[8][32];
  const int c = threadIdx.x & 31, pl = threadIdx.x >> 5;
  const int co = blockIdx.y * 32 + c, b = blockIdx.z, chunk = blockIdx.x;
  const int p0 = chunk * ppc, p1 = min(P, p0 + ppc);
  const float dv = d ? d[(long)b * Co + co] : 1.f;
  const float bv = bias ? bias[co] : 0.f;
  const float* nz = noise ? noise + (long)b * noise_bstride : nullptr;
  const long base = (long)b * P * Co + co;
  const bool lrelu = act == MAUA_ACT_LRELU;
  float acc = 0.f;
  for (int q = p0; q < p1; q += 8) {   // (every lane makes every trip: the channel sum below crosses lanes)
    const int p = q + pl;
    float gv = 0.f;
    if (p < p1) {
      const long e = base + (long)p * Co;
      const float o = Elem<T>::load(y + e);
      const bool neg = lrelu && !(o > 0.f);
      gv = Elem<T>::load(g_y + e) * gain * (neg ? alpha : 1.f);
      if (clamp >= 0.f && !(fabsf(o) < clamp)) gv = 0.f;
      if (d && gv != 0.f) {
        float v = o / gain;
        if (neg) v /= alpha;
        acc += gv * ((v - (nz ? nz[p] * strength : 0.f) - bv) / dv);
      }
      Elem<T>::store(g_u + e, gv * dv);
    }
    if constexpr (GN) {
      float t = gv;
#pragma unroll
      for (int m = 16; m >= 1; m >>= 1) t += __shfl_xor(t, m);
      if (c == 0 && p < p1) npart[((long)b * gridDim.y + blockIdx.y) * P + p] = t;
    }
  }
  red[pl][c] = acc;
  __syncthreads();
  if (pl == 0 && part) {
    float t = red[0][c];
#pragma unroll
    for (int i = 1; i < 8; i++) t += red[i][c];
    part[((long)b * gridDim.x + chunk) * Co + co] = t;
  }
}

// out[b][c] = sum over the chunks, in chunk order; grid (cdiv(C, 256), B)
__global__ __launch_bounds__(256) void sum_chunks_kernel(const float* __restrict__ part, float* __restrict__ out, int nchunk, int C) {
  const int c = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (c >= C) return;
  float t = 0.f;
  for (int k = 0; k < nchunk; k++) t += part[((long)b * nchunk + k) * C + c];
  out[(long)b * C + c] = t;
}

// g_noise[b][p] = strength * sum_g npart[b][g][p], the groups in order; nb == 1 with B > 1 (one shared map): the samples' sums added
// in batch order before the product.  grid (cdiv(P, 256), nb)
__global__ __launch_bounds__(256) void noise_grad_kernel(const float* __restrict__ npart, float* __restrict__ g_noise, long g_bstride, float strength,
                                                         int P, int G, int B, int shared) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= P) return;
  const int b0 = shared ? 0 : blockIdx.y, b1 = shared ? B : b0 + 1;
  float t = 0.f;
  for (int b = b0; b < b1; b++) {
    float tb = npart[(long)b * G * P + p];
    for (int g = 1; g < G; g++) tb += npart[((long)b * G + g) * P + p];
    t = b == b0 ? tb : t + tb;
  }
  g_noise[(long)b0 * g_bstride + p] = strength * t;
}

// g_t[b][r][c][co] = sum_{a, e} f[a] f[e] g_u[b][r - a + 1][c - e + 1][co], r in [0, H2], c in [0, W2]; f = [1, 3, 3, 1] / 4
template <typename T>
__global__ __launch_bounds__(256) void fir_adjoint_kernel(const T* __restrict__ g_u, T* __restrict__ g_t, int H2, int W2, int Co, long total) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int co = (int)(i % Co);
  long q = i / Co;
  const int c = (int)(q % (W2 + 1));
  q /= W2 + 1;
  const int r = (int)(q % (H2 + 1)), b = (int)(q / (H2 + 1));
  const float f[4] = {0.25f, 0.75f, 0.75f, 0.25f};
  float acc = 0.f;
#pragma unroll
  for (int a = 0; a < 4; a++) {
    const int yy = r - a + 1;
    if (yy < 0 || yy >= H2) continue;
#pragma unroll
    for (int e = 0; e < 4; e++) {
      const int xx = c - e + 1;
      if (xx < 0 || xx >= W2) continue;
      acc += f[a] * f[e] * Elem<T>::load(g_u + (((long)b * H2 + yy) * W2 + xx) * Co + co);
    }
  }
  Elem<T>::store(g_t + i, acc);
}

// The input-gradient convolution as an implicit GEMM on the matrix cores.  A wave owns 32 output pixels x NT x 32 input channels;
// lane (r = lane & 31, h = lane >> 5) feeds the 16-byte piece h of a 32-byte K step (K = the forward's OUTPUT channels) of weight
// row ci0 + r and of source pixel p'(m0 + r, tap): Mma<T>::step's D layout then has lane r = pixel, 16 channels per lane.  Source
// pixel of output pixel (i, j) under tap (kh, kw): (st i + sg kh + off, st j + sg kw + off) on the Hs x Ws source grid, zero outside.
// grid (cdiv(H W, 128), Ci / (32 NT), B)
template <typename T, int NT>
__global__ __launch_bounds__(256) void conv_vjp_kernel(const T* __restrict__ src, const T* __restrict__ wg, float* __restrict__ g_xm, int H,
                                                       int W, int Hs, int Ws, int Ci, int Co, int st, int sg, int off) {
  constexpr int EPC = 16 / (int)sizeof(T), KS = 2 * EPC;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
  const int P = H * W, m = (blockIdx.x * 4 + wave) * 32 + r;
  const int ci0 = blockIdx.y * NT * 32, b = blockIdx.z;
  const bool ok = m < P;
  const int i = ok ? m / W : 0, j = ok ? m - i * W : 0;
  const T* sb = src + (long)b * Hs * Ws * Co;
  f32x16 acc[NT];
#pragma unroll
  for (int n = 0; n < NT; n++)
#pragma unroll
    for (int e = 0; e < 16; e++) acc[n][e] = 0.f;
  for (int t = 0; t < 9; t++) {
    const int kh = t / 3, kw = t - 3 * kh;
    const int sy = st * i + sg * kh + off, sx = st * j + sg * kw + off;
    const bool v = ok && sy >= 0 && sy < Hs && sx >= 0 && sx < Ws;
    const T* xp = sb + ((long)(v ? sy : 0) * Ws + (v ? sx : 0)) * Co + h * EPC;
    const T* wp = wg + ((long)t * Ci + ci0 + r) * Co + h * EPC;
    for (int k = 0; k < Co; k += KS) {
      u32x4 xa = u32x4{0u, 0u, 0u, 0u};
      if (v) xa = *reinterpret_cast<const u32x4*>(xp + k);
#pragma unroll
      for (int n = 0; n < NT; n++) Mma<T>::step(acc[n], *reinterpret_cast<const u32x4*>(wp + (long)n * 32 * Co + k), xa);
    }
  }
  if (!ok) return;
  float* o = g_xm + ((long)b * P + m) * Ci + ci0 + 4 * h;
#pragma unroll
  for (int n = 0; n < NT; n++)
#pragma unroll
    for (int qd = 0; qd < 4; qd++)
      *reinterpret_cast<float4*>(o + n * 32 + 8 * qd) =
          make_float4(acc[n][qd * 4 + 0], acc[n][qd * 4 + 1], acc[n][qd * 4 + 2], acc[n][qd * 4 + 3]);
}

// grid (chunks, Ci / 32, B)
template <typename T>
__global__ __launch_bounds__(256) void finish_vjp_kernel(const float* __restrict__ g_xm, const T* __restrict__ x, long x_bstride,
                                                         const float* __restrict__ s, T* __restrict__ g_x, int accumulate,
                                                         float* __restrict__ part, int P, int Ci, int ppc) {
  __shared__ float red[8][32];
  const int c = threadIdx.x & 31, pl = threadIdx.x >> 5;
  const int ci = blockIdx.y * 32 + c, b = blockIdx.z, chunk = blockIdx.x;
  const int p0 = chunk * ppc, p1 = min(P, p0 + ppc);
  const float sv = s[(long)b * Ci + ci];
  const T* xb = x + (long)b * x_bstride + ci;
  const long base = (long)b * P * Ci + ci;
  float acc = 0.f;
  for (int p = p0 + pl; p < p1; p += 8) {
    const float gm = g_xm[base + (long)p * Ci];
    acc += Elem<T>::load(xb + (long)p * Ci) * gm;
    if (g_x) {
      float o = sv * gm;
      if (accumulate) o += Elem<T>::load(g_x + base + (long)p * Ci);
      Elem<T>::store(g_x + base + (long)p * Ci, o);
    }
  }
  red[pl][c] = acc;
  __syncthreads();
  if (pl == 0) {
    float t = red[0][c];
#pragma unroll
    for (int i = 1; i < 8; i++) t += red[i][c];
    part[((long)b * gridDim.x + chunk) * Ci + ci] = t;
  }
}

// grid (cdiv(Ci, 256), B)
__global__ __launch_bounds__(256) void styles_finalize_kernel(const float* __restrict__ part, int nchunk, const float* __restrict__ g_d,
                                                              const float* __restrict__ d, const float* __restrict__ wsq,
                                                              const float* __restrict__ s, float* __restrict__ g_s, int Ci, int Co) {
  const int ci = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (ci >= Ci) return;
  float acc = 0.f;
  for (int k = 0; k < nchunk; k++) acc += part[((long)b * nchunk + k) * Ci + ci];
  if (d) {   // d = (sum_ci s^2 Wsq + eps)^-1/2: d d / d s_ci = -d^3 s_ci Wsq[co][ci]
    float t = 0.f;
    for (int co = 0; co < Co; co++) {
      const float dd = d[(long)b * Co + co];
      t += g_d[(long)b * Co + co] * dd * dd * dd * wsq[(long)co * Ci + ci];
    }
    acc -= s[(long)b * Ci + ci] * t;
  }
  g_s[(long)b * Ci + ci] = acc;
}

// thread = one (tap, ci, co), co fastest
template <typename T>
__global__ __launch_bounds__(256) void prep_vjp_weights_kernel(const float* __restrict__ w, T* __restrict__ wg, float* __restrict__ wsq, int Co,
                                                               int Ci, int flip) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= 9L * Ci * Co) return;
  const int co = (int)(idx % Co);
  const long q = idx / Co;
  const int ci = (int)(q % Ci), t = (int)(q / Ci);
  const float* wv = w + ((long)co * Ci + ci) * 9;
  Elem<T>::store(wg + idx, wv[flip ? 8 - t : t]);
  if (wsq && t == 0) {
    float sq = 0.f;
    for (int k = 0; k < 9; k++) sq += wv[k] * wv[k];
    wsq[(long)co * Ci + ci] = sq;
  }
}

// the same from prepared weights: up 1 [9][Co][Ci]; up 2 the transposed convolution's [slot 4][Co / 32][class 4][32][Ci]
// (modconv_tconv.hip prep_tconv_weights_kernel: tap k of an axis sits in class k == 1, slot half 1 - (k == 1 ? 0 : k / 2))
template <typename T>
__global__ __launch_bounds__(256) void vjp_weights_from_prepared_kernel(const T* __restrict__ prepared, T* __restrict__ wg, int Co, int Ci, int up) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= 9L * Ci * Co) return;
  const int co = (int)(idx % Co);
  const long q = idx / Co;
  const int ci = (int)(q % Ci), t = (int)(q / Ci);
  long src;
  if (up == 1) {
    src = ((long)t * Co + co) * Ci + ci;
  } else {
    const int ky = t / 3, kx = t - 3 * ky;
    const int ap = ky == 1, p = ky == 1 ? 0 : ky / 2, bp = kx == 1, qq = kx == 1 ? 0 : kx / 2;
    const int slot = (1 - p) * 2 + (1 - qq), cls = ap * 2 + bp;
    src = ((((long)slot * (Co / 32) + (co >> 5)) * 4 + cls) * 32 + (co & 31)) * Ci + ci;
  }
  wg[idx] = prepared[src];
}

// toRGB.  grid (chunks, B).  Phase 1: four lanes per pixel recompute y and leave the masked g_y in LDS; phase 2: thread = (pixel
// lane, channel), g_x and the chunk's sum_p x g_y per 32-channel group
constexpr int RGB_PPC_MAX = 1024;
int rgb_ppc(long P) { return (int)std::min<long>(RGB_PPC_MAX, (std::max<long>(64, (P + 1023) / 1024) + 63) / 64 * 64); }
int rgb_nchunk(long P) { return (int)((P + rgb_ppc(P) - 1) / rgb_ppc(P)); }

template <typename T>
__global__ __launch_bounds__(256) void torgb_vjp_kernel(const T* __restrict__ x, const float* __restrict__ wmod, const float* __restrict__ bias,
                                                        const float* __restrict__ g_img, T* __restrict__ g_x, int accumulate,
                                                        float* __restrict__ part, int P, int C, int ppc, float clamp) {
  __shared__ float gy[3][RGB_PPC_MAX];
  __shared__ float red[8][3][32];
  const int chunk = blockIdx.x, b = blockIdx.y;
  const int p0 = chunk * ppc, n = min(ppc, P - p0);
  const float* wm = wmod + (long)b * 3 * C;
  const T* xb = x + ((long)b * P + p0) * C;
  for (int base = 0; base < n; base += 64) {
    const int pix = base + (threadIdx.x >> 2), sub = threadIdx.x & 3;
    const bool valid = pix < n;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    if (valid)
      for (int ch = sub; ch < C; ch += 4) {
        const float xv = Elem<T>::load(xb + (long)pix * C + ch);
        a0 += xv * wm[ch]; a1 += xv * wm[C + ch]; a2 += xv * wm[2 * C + ch];
      }
    a0 += __shfl_xor(a0, 1); a1 += __shfl_xor(a1, 1); a2 += __shfl_xor(a2, 1);
    a0 += __shfl_xor(a0, 2); a1 += __shfl_xor(a1, 2); a2 += __shfl_xor(a2, 2);
    if (valid && sub == 0) {
      const float yv[3] = {a0 + bias[0], a1 + bias[1], a2 + bias[2]};
#pragma unroll
      for (int k = 0; k < 3; k++)
        gy[k][pix] = (clamp < 0.f || fabsf(yv[k]) < clamp) ? g_img[((long)b * 3 + k) * P + p0 + pix] : 0.f;
    }
  }
  __syncthreads();
  const int cl = threadIdx.x & 31, pl = threadIdx.x >> 5;
  T* gxb = g_x + ((long)b * P + p0) * C;
  for (int ch = cl; ch < C; ch += 32) {   // (C % 32 == 0: every thread makes the same number of trips)
    const float w0 = wm[ch], w1 = wm[C + ch], w2 = wm[2 * C + ch];
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
    for (int p = pl; p < n; p += 8) {
      const float xv = Elem<T>::load(xb + (long)p * C + ch);
      const float g0 = gy[0][p], g1 = gy[1][p], g2 = gy[2][p];
      float o = w0 * g0 + w1 * g1 + w2 * g2;
      if (accumulate) o += Elem<T>::load(gxb + (long)p * C + ch);
      Elem<T>::store(gxb + (long)p * C + ch, o);
      s0 += xv * g0; s1 += xv * g1; s2 += xv * g2;
    }
    __syncthreads();
    red[pl][0][cl] = s0; red[pl][1][cl] = s1; red[pl][2][cl] = s2;
    __syncthreads();
    if (pl < 3) {
      float t = red[0][pl][cl];
#pragma unroll
      for (int i = 1; i < 8; i++) t += red[i][pl][cl];
      part[(((long)b * gridDim.x + chunk) * 3 + pl) * C + ch] = t;
    }
  }
}

// g_prev[b][c][i][j] = sum_{a, e} f[a] f[e] g_img[b][c][2 i + a - 1][2 j + e - 1] (upfirdn2d with down 2, padding (1, 2, 1, 2), gain 4)
__global__ __launch_bounds__(256) void skip_vjp_kernel(const float* __restrict__ g_img, float* __restrict__ g_prev, int h, int w, long total) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int j = (int)(idx % w);
  const long q = idx / w;
  const int i = (int)(q % h);
  const long plane = q / h;
  const float f[4] = {0.25f, 0.75f, 0.75f, 0.25f};
  const float* g = g_img + plane * 4L * h * w;
  float acc = 0.f;
#pragma unroll
  for (int a = 0; a < 4; a++) {
    const int yy = 2 * i + a - 1;
    if (yy < 0 || yy >= 2 * h) continue;
#pragma unroll
    for (int e = 0; e < 4; e++) {
      const int xx = 2 * j + e - 1;
      if (xx < 0 || xx >= 2 * w) continue;
      acc += f[a] * f[e] * g[(long)yy * 2 * w + xx];
    }
  }
  g_prev[idx] = acc;
}

// grid (cdiv(w_dim, 256), B)
__global__ __launch_bounds__(256) void affine_vjp_kernel(const float* __restrict__ g_s, int ld, const float* __restrict__ affine_w, float scale,
                                                         float* __restrict__ g_ws, int w_index, int num_ws, int w_dim, int C) {
  const int k = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (k >= w_dim) return;
  float t = 0.f;
  for (int c = 0; c < C; c++) t += g_s[(long)b * ld + c] * affine_w[(long)c * w_dim + k];
  g_ws[((long)b * num_ws + w_index) * w_dim + k] += scale * t;
}

__global__ __launch_bounds__(256) void rgb_styles_vjp_kernel(const float* __restrict__ g_wmod, const float* __restrict__ wrgb,
                                                             float* __restrict__ g_s, int C) {
  const int c = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (c >= C) return;
  const float* g = g_wmod + (long)b * 3 * C;
  g_s[(long)b * C + c] = (wrgb[c] * g[c] + wrgb[C + c] * g[C + c]) + wrgb[2 * C + c] * g[2 * C + c];
}

template <typename T>
int launch_modconv_vjp_t(hipStream_t st, const ModconvVjpArgs& a) {
  const int Ho = a.H * a.up, Wo = a.W * a.up;
  const long Po = (long)Ho * Wo, Pi = (long)a.H * a.W;
  const int nco = vjp_nchunk(Po), nci = vjp_nchunk(Pi);
  if (a.g_noise) {
    hipLaunchKernelGGL((act_vjp_kernel<T, true>), dim3(nco, a.Co / 32, a.B), dim3(256), 0, st, (const T*)a.y, (const T*)a.g_y, a.d, a.noise,
                       a.noise_bstride, a.noise_strength, a.bias, (T*)a.g_u, a.d ? a.part : nullptr, a.npart, (int)Po, a.Co, vjp_ppc(Po),
                       a.act, a.alpha, a.gain, a.clamp);
    const int shared = a.g_noise_bstride == 0;
    hipLaunchKernelGGL(noise_grad_kernel, dim3(cdiv((int)Po, 256), shared ? 1 : a.B), dim3(256), 0, st, a.npart, a.g_noise, a.g_noise_bstride,
                       a.noise_strength, (int)Po, a.Co / 32, a.B, shared);
  } else {
    hipLaunchKernelGGL((act_vjp_kernel<T, false>), dim3(nco, a.Co / 32, a.B), dim3(256), 0, st, (const T*)a.y, (const T*)a.g_y, a.d, a.noise,
                       a.noise_bstride, a.noise_strength, a.bias, (T*)a.g_u, a.d ? a.part : nullptr, nullptr, (int)Po, a.Co, vjp_ppc(Po),
                       a.act, a.alpha, a.gain, a.clamp);
  }
  if (a.d) hipLaunchKernelGGL(sum_chunks_kernel, dim3(cdiv(a.Co, 256), a.B), dim3(256), 0, st, a.part, a.g_d, nco, a.Co);
  const T* src = (const T*)a.g_u;
  int Hs = a.H, Ws = a.W, stp = 1, sg = -1, off = 1;
  if (a.up == 2) {
    const long total = (long)a.B * (Ho + 1) * (Wo + 1) * a.Co;
    hipLaunchKernelGGL(fir_adjoint_kernel<T>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (const T*)a.g_u, (T*)a.g_t, Ho, Wo,
                       a.Co, total);
    src = (const T*)a.g_t;
    Hs = Ho + 1; Ws = Wo + 1; stp = 2; sg = 1; off = 0;
  }
  const dim3 block(256);
  const unsigned gm = (unsigned)((Pi + 127) / 128);
  if (a.Ci % 128 == 0)
    hipLaunchKernelGGL((conv_vjp_kernel<T, 4>), dim3(gm, a.Ci / 128, a.B), block, 0, st, src, (const T*)a.wg, a.g_xm, a.H, a.W, Hs, Ws, a.Ci,
                       a.Co, stp, sg, off);
  else if (a.Ci % 64 == 0)
    hipLaunchKernelGGL((conv_vjp_kernel<T, 2>), dim3(gm, a.Ci / 64, a.B), block, 0, st, src, (const T*)a.wg, a.g_xm, a.H, a.W, Hs, Ws, a.Ci,
                       a.Co, stp, sg, off);
  else
    hipLaunchKernelGGL((conv_vjp_kernel<T, 1>), dim3(gm, a.Ci / 32, a.B), block, 0, st, src, (const T*)a.wg, a.g_xm, a.H, a.W, Hs, Ws, a.Ci,
                       a.Co, stp, sg, off);
  hipLaunchKernelGGL(finish_vjp_kernel<T>, dim3(nci, a.Ci / 32, a.B), dim3(256), 0, st, a.g_xm, (const T*)a.x, a.x_bstride, a.s, (T*)a.g_x,
                     a.accumulate, a.part, (int)Pi, a.Ci, vjp_ppc(Pi));
  hipLaunchKernelGGL(styles_finalize_kernel, dim3(cdiv(a.Ci, 256), a.B), dim3(256), 0, st, a.part, nci, a.g_d, a.d, a.wsq, a.s, a.g_s, a.Ci,
                     a.Co);
  MAUA_HIP_CHECK(hipGetLastError());
  return MAUA_OK;
}

template <typename T>
int launch_torgb_vjp_t(hipStream_t st, const RgbVjpArgs& a) {
  const long P = (long)a.H * a.W;
  const int nc = rgb_nchunk(P);
  hipLaunchKernelGGL(torgb_vjp_kernel<T>, dim3(nc, a.B), dim3(256), 0, st, (const T*)a.x, a.wmod, a.bias, a.g_img, (T*)a.g_x, a.accumulate,
                     a.part, (int)P, a.C, rgb_ppc(P), a.clamp);
  hipLaunchKernelGGL(sum_chunks_kernel, dim3(cdiv(3 * a.C, 256), a.B), dim3(256), 0, st, a.part, a.g_wmod, nc, 3 * a.C);
  MAUA_HIP_CHECK(hipGetLastError());
  return MAUA_OK;
}

// the forward descriptor -> the launcher's arguments (workspaces and prepared weights are the caller's)
ModconvVjpArgs vjp_args(const maua_modconv_desc* f, const void* g_y, void* g_x, float* g_s) {
  ModconvVjpArgs a{};
  a.x = f->x; a.x_bstride = f->x_bstride; a.y = f->y; a.g_y = g_y; a.s = f->s; a.d = f->d;
  a.noise = f->noise; a.noise_bstride = f->noise_bstride; a.noise_strength = f->noise_strength; a.bias = f->bias;
  a.g_x = g_x; a.g_s = g_s; a.B = f->B; a.H = f->H; a.W = f->W; a.Ci = f->Ci; a.Co = f->Co; a.up = f->up;
  a.act = f->act; a.alpha = f->alpha; a.gain = f->gain; a.clamp = f->clamp;
  return a;
}
int vjp_desc_check(const maua_modconv_desc* f, const void* g_y, float* g_s, int dtype) {
  MAUA_REQUIRE(f, "maua_modconv_vjp: desc is NULL");
  MAUA_REQUIRE(dtype != MAUA_F16, "maua_modconv_vjp: MAUA_F16 is not differentiated (its pre-normalisation of weights and styles is not)");
  MAUA_REQUIRE(f->w && g_y && g_s, "maua_modconv_vjp: NULL w / g_y / g_s");
  MAUA_REQUIRE(!f->noise_scale, "maua_modconv_vjp: per-sample noise scales are not differentiated");
  MAUA_REQUIRE(!f->out_scale && !f->y_scaled && !f->rgb_out && !f->rgb8_out,
               "maua_modconv_vjp: describe the plain layer (no out_scale / y_scaled / fused toRGB)");
  return modconv_vjp_check(dtype, vjp_args(f, g_y, nullptr, g_s));
}

}  // namespace

ModconvVjpWorkspace modconv_vjp_workspace(int dtype, int B, int H, int W, int Ci, int Co, int up) {
  const size_t es = elem_bytes(dtype);
  const long Po = (long)H * up * W * up, Pi = (long)H * W;
  ModconvVjpWorkspace w;
  w.g_u = (size_t)B * Po * Co * es;
  w.g_t = up == 2 ? (size_t)B * (2 * H + 1) * (2 * W + 1) * Co * es : 0;
  w.g_xm = (size_t)B * Pi * Ci * 4;
  w.part = (size_t)B * std::max((size_t)vjp_nchunk(Po) * Co, (size_t)vjp_nchunk(Pi) * Ci) * 4;
  w.g_d = (size_t)B * Co * 4;
  return w;
}

size_t modconv_vjp_noise_part_bytes(int B, int H, int W, int Co, int up) { return (size_t)B * (Co / 32) * H * up * W * up * 4; }

int modconv_vjp_check(int dtype, const ModconvVjpArgs& a) {
  MAUA_REQUIRE(dtype == MAUA_F32 || dtype == MAUA_BF16, "maua_modconv_vjp: dtype must be MAUA_F32 or MAUA_BF16");
  MAUA_REQUIRE(a.B >= 0 && a.H > 0 && a.W > 0 && a.Ci > 0 && a.Co > 0, "maua_modconv_vjp: bad shape");
  MAUA_REQUIRE(a.up == 1 || a.up == 2, "maua_modconv_vjp: up must be 1 or 2");
  MAUA_REQUIRE(a.Ci % 32 == 0 && a.Co % 32 == 0, "maua_modconv_vjp: channel counts must be multiples of 32");
  MAUA_REQUIRE(a.x && a.y && a.g_y && a.s && a.g_s, "maua_modconv_vjp: NULL x / y / g_y / s / g_s");
  MAUA_REQUIRE(a.x_bstride == 0 || a.x_bstride >= (long)a.H * a.W * a.Ci, "maua_modconv_vjp: samples of x overlap");
  MAUA_REQUIRE(a.act == MAUA_ACT_LINEAR || a.act == MAUA_ACT_LRELU, "maua_modconv_vjp: the activation must be linear or lrelu");
  MAUA_REQUIRE(a.gain > 0.f && (a.act != MAUA_ACT_LRELU || a.alpha >= 0.f), "maua_modconv_vjp: gain must be positive, alpha not negative");
  MAUA_REQUIRE((2L * a.H + 1) * (2L * a.W + 1) * a.Co < (1L << 31) && (long)a.H * a.W * a.Ci < (1L << 31) && 9L * a.Ci * a.Co < (1L << 31),
               "maua_modconv_vjp: 32-bit offsets");
  MAUA_REQUIRE(a.B <= 65535, "maua_modconv_vjp: grid too large");
  return MAUA_OK;
}

int launch_modconv_vjp(hipStream_t st, int dtype, const ModconvVjpArgs& a) {
  if (int rc = modconv_vjp_check(dtype, a)) return rc;
  MAUA_REQUIRE(a.wg && a.g_u && a.g_xm && a.part && (a.up == 1 || a.g_t) && (!a.d || (a.g_d && a.wsq)) && (!a.g_noise || a.npart),
               "maua_modconv_vjp: NULL workspace");
  MAUA_REQUIRE(!a.g_noise || a.g_noise_bstride == 0 || a.g_noise_bstride >= (long)a.H * a.up * a.W * a.up, "maua_modconv_vjp: samples of g_noise overlap");
  if (a.B == 0) return MAUA_OK;
  return dispatch_dtype<bf16_t, float>(dtype, "maua_modconv_vjp", [&](auto t) { return launch_modconv_vjp_t<decltype(t)>(st, a); });
}

int launch_prep_vjp_weights(hipStream_t st, int dtype, const float* w, void* wg, float* wsq, int Co, int Ci, int flip) {
  const unsigned grid = (unsigned)((9L * Ci * Co + 255) / 256);
  return dispatch_dtype<bf16_t, float>(dtype, "prep_vjp_weights", [&](auto t) {
    hipLaunchKernelGGL(prep_vjp_weights_kernel<decltype(t)>, dim3(grid), dim3(256), 0, st, w, (decltype(t)*)wg, wsq, Co, Ci, flip);
    MAUA_HIP_CHECK(hipGetLastError());
    return MAUA_OK;
  });
}

int launch_vjp_weights_from_prepared(hipStream_t st, int dtype, const void* prepared, void* wg, int Co, int Ci, int up) {
  MAUA_REQUIRE(Co % 32 == 0, "vjp_weights_from_prepared: Co must be a multiple of 32");
  const unsigned grid = (unsigned)((9L * Ci * Co + 255) / 256);
  return dispatch_dtype<bf16_t, float>(dtype, "vjp_weights_from_prepared", [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(vjp_weights_from_prepared_kernel<T>, dim3(grid), dim3(256), 0, st, (const T*)prepared, (T*)wg, Co, Ci, up);
    MAUA_HIP_CHECK(hipGetLastError());
    return MAUA_OK;
  });
}

size_t torgb_vjp_part_bytes(int B, int H, int W, int C) { return (size_t)B * rgb_nchunk((long)H * W) * 3 * C * 4; }

int torgb_vjp_check(int dtype, const RgbVjpArgs& a) {
  MAUA_REQUIRE(dtype != MAUA_F16, "maua_torgb_vjp: MAUA_F16 is not differentiated (its pre-normalisation of weights and styles is not)");
  MAUA_REQUIRE(dtype == MAUA_F32 || dtype == MAUA_BF16, "maua_torgb_vjp: dtype must be MAUA_F32 or MAUA_BF16");
  MAUA_REQUIRE(a.x && a.wmod && a.bias && a.g_img && a.g_x && a.g_wmod, "maua_torgb_vjp: NULL argument");
  MAUA_REQUIRE(a.B >= 0 && a.H > 0 && a.W > 0 && a.C > 0, "maua_torgb_vjp: bad shape");
  MAUA_REQUIRE(a.C % 32 == 0, "maua_torgb_vjp: the channel count must be a multiple of 32");
  MAUA_REQUIRE((long)a.H * a.W < (1L << 31) / a.C && a.B <= 65535, "maua_torgb_vjp: 32-bit offsets");
  return MAUA_OK;
}

int launch_torgb_vjp(hipStream_t st, int dtype, const RgbVjpArgs& a) {
  if (int rc = torgb_vjp_check(dtype, a)) return rc;
  MAUA_REQUIRE(a.part, "maua_torgb_vjp: NULL workspace");
  if (a.B == 0) return MAUA_OK;
  return dispatch_dtype<bf16_t, float>(dtype, "maua_torgb_vjp", [&](auto t) { return launch_torgb_vjp_t<decltype(t)>(st, a); });
}

int launch_skip_vjp(hipStream_t st, const float* g_img, float* g_prev, int B, int h, int w) {
  const long total = (long)B * 3 * h * w;
  if (total == 0) return MAUA_OK;
  hipLaunchKernelGGL(skip_vjp_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, g_img, g_prev, h, w, total);
  MAUA_HIP_CHECK(hipGetLastError());
  return MAUA_OK;
}

int launch_affine_vjp(hipStream_t st, const float* g_s, int ld, const float* affine_w, float scale, float* g_ws, int w_index, int num_ws,
                      int w_dim, int B, int C) {
  if (B == 0) return MAUA_OK;
  hipLaunchKernelGGL(affine_vjp_kernel, dim3(cdiv(w_dim, 256), B), dim3(256), 0, st, g_s, ld, affine_w, scale, g_ws, w_index, num_ws, w_dim, C);
  MAUA_HIP_CHECK(hipGetLastError());
  return MAUA_OK;
}

int launch_rgb_styles_vjp(hipStream_t st, const float* g_wmod, const float* wrgb, float* g_s, int B, int C) {
  if (B == 0) return MAUA_OK;
  hipLaunchKernelGGL(rgb_styles_vjp_kernel, dim3(cdiv(C, 256), B), dim3(256), 0, st, g_wmod, wrgb, g_s, C);
  MAUA_HIP_CHECK(hipGetLastError());
  return MAUA_OK;
}

}  // namespace maua

using namespace maua;

extern "C" int maua_modconv_vjp_check(const maua_modconv_desc* fwd, const void* g_y, float* g_s, int dtype) {
  return vjp_desc_check(fwd, g_y, g_s, dtype);
}

extern "C" int maua_modconv_vjp_ex(maua_ctx* ctx, const maua_modconv_desc* fwd, const void* g_y, void* g_x, float* g_s, int dtype) {
  MAUA_REQUIRE(ctx, "maua_modconv_vjp_ex: ctx is NULL");
  if (int rc = vjp_desc_check(fwd, g_y, g_s, dtype)) return rc;
  if (fwd->B == 0) return MAUA_OK;
  const ModconvVjpWorkspace ws = modconv_vjp_workspace(dtype, fwd->B, fwd->H, fwd->W, fwd->Ci, fwd->Co, fwd->up);
  const size_t wg_bytes = 9 * (size_t)fwd->Ci * fwd->Co * elem_bytes(dtype), wsq_bytes = (size_t)fwd->Ci * fwd->Co * 4;
  ModconvVjpArgs a = vjp_args(fwd, g_y, g_x, g_s);
  char* wg;
  float* wsq;
  if (int rc = carve_scratch(ctx, [&](Scratch& s) {
        a.wg = wg = s.take<char>(wg_bytes); a.wsq = wsq = s.take<float>(wsq_bytes / 4); a.g_u = s.take<char>(ws.g_u); a.g_t = s.take<char>(ws.g_t);
        a.g_xm = s.take<float>(ws.g_xm / 4); a.part = s.take<float>(ws.part / 4); a.g_d = s.take<float>(ws.g_d / 4);
      }))
    return rc;
  if (int rc = launch_prep_vjp_weights(ctx->stream, dtype, fwd->w, wg, wsq, fwd->Co, fwd->Ci, fwd->up == 2 ? fwd->flip : 0)) return rc;
  return launch_modconv_vjp(ctx->stream, dtype, a);
}

static RgbVjpArgs rgb_vjp_args(const void* x, const float* wmod, const float* bias, const float* g_img, void* g_x, float* g_wmod, int B, int H,
                               int W, int C, float clamp, int accumulate) {
  RgbVjpArgs a{};
  a.x = x; a.wmod = wmod; a.bias = bias; a.g_img = g_img; a.g_x = g_x; a.g_wmod = g_wmod; a.accumulate = accumulate;
  a.B = B; a.H = H; a.W = W; a.C = C; a.clamp = clamp;
  return a;
}

extern "C" int maua_torgb_vjp_check(const void* x, const float* wmod, const float* bias, const float* g_img, void* g_x, float* g_wmod, int B,
                                    int H, int W, int C, int dtype) {
  return torgb_vjp_check(dtype, rgb_vjp_args(x, wmod, bias, g_img, g_x, g_wmod, B, H, W, C, -1.f, 0));
}

extern "C" int maua_torgb_vjp_ex(maua_ctx* ctx, const void* x, const float* wmod, const float* bias, const float* g_img, void* g_x,
                                 float* g_wmod, int B, int H, int W, int C, float clamp, int accumulate, int dtype) {
  MAUA_REQUIRE(ctx, "maua_torgb_vjp_ex: ctx is NULL");
  RgbVjpArgs a = rgb_vjp_args(x, wmod, bias, g_img, g_x, g_wmod, B, H, W, C, clamp, accumulate);
  if (int rc = torgb_vjp_check(dtype, a)) return rc;
  if (B == 0) return MAUA_OK;
  if (int rc = carve_scratch(ctx, [&](Scratch& s) { a.part = s.take<float>(torgb_vjp_part_bytes(B, H, W, C) / 4); })) return rc;
  return launch_torgb_vjp(ctx->stream, dtype, a);
}
