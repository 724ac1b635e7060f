// The convolution, pooling and stem kernels of the ResNet backbones (resnet.hip: the SwAV ResNet-50 feature extractor of the GAN
// metrics; the same forms are what CLIP's ResNet towers would run).
//
// Replaces (reference): maua/GAN/metrics/extractors/swav.py - conv1x1 / conv3x3 (:20-36) with the BatchNorm that follows folded into
// weight and bias by the caller, the ReLU of Bottleneck.forward (:119-139) INCLUDING the one after `out += identity`, the stem
// `ConstantPad2d(1, 0) + Conv2d(3, C, 7, stride 2, padding 2)` (:165, :183), `MaxPool2d(3, 2, 1)` (:186) and `AdaptiveAvgPool2d((1, 1))`
// + flatten (:200, :298-299).
//
// One implicit GEMM serves every convolution: rows = output pixels (b, oh, ow), columns = output channels, K = (tap, input channel)
// in 128-byte chunks of one tap - a chunk never straddles taps because Ci is a multiple of 64.  The A rows are gathered from NHWC
// activations with the stride and the zero border applied in the address (an out-of-range pixel stages zeros); the stem gathers its
// K = 147 = (c, r, s) values one by one from the planar float32 image and rounds them to the network dtype, K padded with zeros to
// whole chunks.  Operands are staged through registers into LDS rows of 128 + 16 bytes (conflict-free ds_read_b128 fragments) while
// the previous chunk is multiplied - the structure of gemm.hip's 128 x 128 kernel, whose LDS-direct sibling cannot zero a row that
// lies outside the image.  Products are Mma<T>::step (mma.h): v_mfma_f32_32x32x16_bf16 or four exact v_mfma_f32_32x32x2_f32.
//
// Epilogue: v = acc + bias (+ residual, read in the storage dtype, added in float32), ReLU last, ONE rounding on the store.
// The summation order of an output element is fixed by the shape alone (K order, then bias, then residual): no atomics, no split-K.
//
// Tiles (sconv_route, the one routing function): 128 pixels x 128 channels per 256-thread workgroup (four waves of 64 x 64), or
// 64 x 64 (four waves of 32 x 32) where the large tile would leave fewer workgroups than the 256 compute units - the layer-3 / layer-4
// shapes at batch 64 (M = 3136, N = 512: 100 workgroups of 128 x 128, 392 of 64 x 64; LDS 18 KB: several stay resident per unit).
// The stem runs 128 pixels x 64 channels.
#include "common.h"
#include "internal.h"
#include "mma.h"

namespace maua {

namespace {

constexpr int SKCB = 128, SRS = SKCB + 16;   // K chunk and LDS row stride in bytes
constexpr int STEM_K = 147;                  // 3 x 7 x 7

// MI x NJ: 32 x 32 accumulator blocks per wave along pixels / channels; the four waves sit 2 x 2
template <typename T, int MI, int NJ, bool STEM>
__global__ __launch_bounds__(256) void sconv_kernel(SConvArgs a) {
  constexpr int KC = SKCB / (int)sizeof(T), EPC = 16 / (int)sizeof(T);
  constexpr int BM = 64 * MI, BN = 64 * NJ;
  __shared__ __attribute__((aligned(16))) char a_s[BM * SRS];
  __shared__ __attribute__((aligned(16))) char b_s[BN * SRS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int wm = wave >> 1, wn = wave & 1;
  const int Ho = (a.H + 2 * a.pad - a.k) / a.stride + 1, Wo = (a.W + 2 * a.pad - a.k) / a.stride + 1;
  const long M = (long)a.B * Ho * Wo;
  const long m0 = (long)blockIdx.x * BM;
  const int n0 = blockIdx.y * BN;
  const int q = tid & 7, row0 = tid >> 3;   // staging role: 16-byte piece q of rows row0 + 32 i, A and W alike
  const int cpt = STEM ? 1 : a.Ci / KC;     // chunks per tap
  const int stages = STEM ? a.kpad / KC : a.k * a.k * cpt;
  const T* w = reinterpret_cast<const T*>(a.w);

  // this thread's A rows: top-left input pixel of the window and the sample's first pixel (stem: first float)
  int ih0[2 * MI], iw0[2 * MI];
  long boff[2 * MI];
#pragma unroll
  for (int i = 0; i < 2 * MI; i++) {
    const long m = m0 + row0 + 32 * i;
    if (m < M) {
      const long b = m / ((long)Ho * Wo);
      const int rem = (int)(m - b * Ho * Wo), oh = rem / Wo, ow = rem - oh * Wo;
      ih0[i] = oh * a.stride - a.pad;
      iw0[i] = ow * a.stride - a.pad;
      boff[i] = b * (STEM ? 3L : 1L) * a.H * a.W;
    } else {
      ih0[i] = iw0[i] = -(1 << 20);   // (every tap of it is out of range: zeros)
      boff[i] = 0;
    }
  }

  u32x4 areg[2 * MI], breg[2 * NJ];
  auto load = [&](int s) {
    if constexpr (STEM) {
      const float* img = reinterpret_cast<const float*>(a.x);
      const int k0 = s * KC + q * EPC;
#pragma unroll
      for (int i = 0; i < 2 * MI; i++) {
        float v[EPC];
#pragma unroll
        for (int e = 0; e < EPC; e++) {
          const int kk = k0 + e, c = kk / 49, t = kk - c * 49, ky = t / 7, kx = t - ky * 7;
          const int ih = ih0[i] + ky, iw = iw0[i] + kx;
          v[e] = 0.f;
          if (kk < STEM_K && (unsigned)ih < (unsigned)a.H && (unsigned)iw < (unsigned)a.W)
            v[e] = img[boff[i] + ((long)c * a.H + ih) * a.W + iw];
        }
        if constexpr (sizeof(T) == 2)
          areg[i] = u32x4{pack2bf(v[0], v[1]), pack2bf(v[2], v[3]), pack2bf(v[EPC - 4], v[EPC - 3]), pack2bf(v[EPC - 2], v[EPC - 1])};
        else
          areg[i] = u32x4{__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3])};
      }
#pragma unroll
      for (int i = 0; i < 2 * NJ; i++) {
        const int n = n0 + row0 + 32 * i;
        breg[i] = u32x4{0u, 0u, 0u, 0u};
        if (n < a.Co) breg[i] = *reinterpret_cast<const u32x4*>(w + (long)n * a.kpad + k0);
      }
    } else {
      const T* x = reinterpret_cast<const T*>(a.x);
      const int t = s / cpt, c0 = (s - t * cpt) * KC + q * EPC;
      const int ky = t / a.k, kx = t - ky * a.k;
#pragma unroll
      for (int i = 0; i < 2 * MI; i++) {
        const int ih = ih0[i] + ky, iw = iw0[i] + kx;
        areg[i] = u32x4{0u, 0u, 0u, 0u};
        if ((unsigned)ih < (unsigned)a.H && (unsigned)iw < (unsigned)a.W)
          areg[i] = *reinterpret_cast<const u32x4*>(x + (boff[i] + (long)ih * a.W + iw) * a.Ci + c0);
      }
#pragma unroll
      for (int i = 0; i < 2 * NJ; i++) {
        const int n = n0 + row0 + 32 * i;
        breg[i] = u32x4{0u, 0u, 0u, 0u};
        if (n < a.Co) breg[i] = *reinterpret_cast<const u32x4*>(w + ((long)t * a.Co + n) * a.Ci + c0);
      }
    }
  };

  f32x16 acc[MI][NJ];
#pragma unroll
  for (int i = 0; i < MI; i++)
#pragma unroll
    for (int j = 0; j < NJ; j++)
#pragma unroll
      for (int e = 0; e < 16; e++) acc[i][j][e] = 0.f;

  load(0);
  for (int s = 0; s < stages; s++) {
    __syncthreads();   // the previous chunk's fragment reads are done
#pragma unroll
    for (int i = 0; i < 2 * MI; i++) *reinterpret_cast<u32x4*>(a_s + (row0 + 32 * i) * SRS + q * 16) = areg[i];
#pragma unroll
    for (int i = 0; i < 2 * NJ; i++) *reinterpret_cast<u32x4*>(b_s + (row0 + 32 * i) * SRS + q * 16) = breg[i];
    __syncthreads();
    if (s + 1 < stages) load(s + 1);   // flies during the MFMAs
#pragma unroll
    for (int ks = 0; ks < SKCB / 32; ks++) {
      u32x4 af[MI], bf[NJ];
#pragma unroll
      for (int i = 0; i < MI; i++) af[i] = *reinterpret_cast<const u32x4*>(a_s + ((wm * MI + i) * 32 + r) * SRS + ks * 32 + h * 16);
#pragma unroll
      for (int j = 0; j < NJ; j++) bf[j] = *reinterpret_cast<const u32x4*>(b_s + ((wn * NJ + j) * 32 + r) * SRS + ks * 32 + h * 16);
#pragma unroll
      for (int i = 0; i < MI; i++)
#pragma unroll
        for (int j = 0; j < NJ; j++) Mma<T>::step(acc[i][j], bf[j], af[i]);   // rows = channels n, columns = pixels m
    }
  }

  // a lane owns pixel m and runs of four channels: bias, residual (f32 sum), ReLU, one rounding
  T* y = reinterpret_cast<T*>(a.y);
  const T* res = reinterpret_cast<const T*>(a.res);
#pragma unroll
  for (int i = 0; i < MI; i++) {
    const long m = m0 + (wm * MI + i) * 32 + r;
    if (m >= M) continue;
#pragma unroll
    for (int j = 0; j < NJ; j++)
#pragma unroll
      for (int qd = 0; qd < 4; qd++) {
        const int n = n0 + (wn * NJ + j) * 32 + 8 * qd + 4 * h;
        if (n >= a.Co) continue;   // (Co % 64 == 0: a run is inside or outside as a whole)
        float v[4] = {acc[i][j][qd * 4], acc[i][j][qd * 4 + 1], acc[i][j][qd * 4 + 2], acc[i][j][qd * 4 + 3]};
        if (a.bias) {
          const float4 bv = *reinterpret_cast<const float4*>(a.bias + n);
          v[0] += bv.x; v[1] += bv.y; v[2] += bv.z; v[3] += bv.w;
        }
        if (res) {
#pragma unroll
          for (int e = 0; e < 4; e++) v[e] += Elem<T>::load(res + m * a.Co + n + e);
        }
        if (a.relu) {
#pragma unroll
          for (int e = 0; e < 4; e++) v[e] = v[e] > 0.f ? v[e] : 0.f;
        }
        if constexpr (sizeof(T) == 2)
          *reinterpret_cast<uint2*>(y + m * a.Co + n) = make_uint2(pack2bf(v[0], v[1]), pack2bf(v[2], v[3]));
        else
          *reinterpret_cast<float4*>(y + m * a.Co + n) = make_float4(v[0], v[1], v[2], v[3]);
      }
  }
}

// f32 [Co][147] -> T [Co][kpad], zero padded
template <typename T>
__global__ __launch_bounds__(256) void prep_stem_weights_kernel(const float* __restrict__ w, T* __restrict__ wt, int Co, int kpad) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)Co * kpad) return;
  const int co = (int)(idx / kpad), k = (int)(idx - (long)co * kpad);
  Elem<T>::store(wt + idx, k < STEM_K ? w[(long)co * STEM_K + k] : 0.f);
}

// MaxPool2d(3, 2, 1) on NHWC: one thread per output pixel and 16-byte piece; taps outside the image are left out (the window's
// centre row / column always lies inside, so every window has a tap)
template <typename T>
__global__ __launch_bounds__(256) void maxpool3x3s2_kernel(const T* __restrict__ x, T* __restrict__ y, int B, int H, int W, int C, int Ho,
                                                           int Wo) {
  constexpr int EPC = 16 / (int)sizeof(T);
  const int pieces = C / EPC;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)B * Ho * Wo * pieces) return;
  const int pc = (int)(idx % pieces);
  const long p = idx / pieces;
  const int ow = (int)(p % Wo), oh = (int)((p / Wo) % Ho);
  const long b = p / ((long)Wo * Ho);
  float best[EPC];
  bool any = false;
  for (int ky = 0; ky < 3; ky++) {
    const int ih = oh * 2 - 1 + ky;
    if ((unsigned)ih >= (unsigned)H) continue;
    for (int kx = 0; kx < 3; kx++) {
      const int iw = ow * 2 - 1 + kx;
      if ((unsigned)iw >= (unsigned)W) continue;
      const u32x4 v = *reinterpret_cast<const u32x4*>(x + ((b * H + ih) * W + iw) * C + pc * EPC);
      float f[EPC];
      if constexpr (sizeof(T) == 2) {
#pragma unroll
        for (int e = 0; e < 4; e++) { f[2 * e] = Fmt16<bf16_t>::lo(v[e]); f[2 * e + 1] = Fmt16<bf16_t>::hi(v[e]); }
      } else {
#pragma unroll
        for (int e = 0; e < 4; e++) f[e] = __uint_as_float(v[e]);
      }
#pragma unroll
      for (int e = 0; e < EPC; e++) best[e] = any ? fmaxf(best[e], f[e]) : f[e];
      any = true;
    }
  }
  u32x4 o;
  if constexpr (sizeof(T) == 2) {
#pragma unroll
    for (int e = 0; e < 4; e++) o[e] = pack2bf(best[2 * e], best[2 * e + 1]);   // (values of the input: the rounding is exact)
  } else {
#pragma unroll
    for (int e = 0; e < 4; e++) o[e] = __float_as_uint(best[e]);
  }
  *reinterpret_cast<u32x4*>(y + p * C + pc * EPC) = o;
}

// NHWC -> f32 [B][C]: one thread per (sample, channel), the pixels summed in index order, one multiply by 1 / (H W)
template <typename T>
__global__ __launch_bounds__(256) void global_avgpool_kernel(const T* __restrict__ x, float* __restrict__ out, int B, long HW, int C, float inv) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)B * C) return;
  const long b = idx / C;
  const int c = (int)(idx - b * C);
  const T* p = x + b * HW * C + c;
  float s = 0.f;
  for (long i = 0; i < HW; i++) s += Elem<T>::load(p + i * C);
  out[idx] = s * inv;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

int stem_kpad(int dtype) {
  const int kc = elems_per_chunk(dtype, SKCB);
  return kc ? (STEM_K + kc - 1) / kc * kc : 0;
}

int sconv_out(int n, int k, int stride, int pad) { return (n + 2 * pad - k) / stride + 1; }

// The routing of every convolution of the backbone - the stride-1 1 x 1 layers included: they run on this kernel, whose k = 1 form IS
// the plain GEMM loop, because the ReLU-after-residual epilogue lives here and gemm.hip's kernels (pinned bit for bit) stay untouched.
int sconv_route(const SConvArgs& a) {
  if (a.stem) return 1;
  const long M = (long)a.B * sconv_out(a.H, a.k, a.stride, a.pad) * sconv_out(a.W, a.k, a.stride, a.pad);
  const long wide = ((M + 127) / 128) * ((a.Co + 127) / 128);
  return a.Co % 128 == 0 && wide >= 256 ? 2 : 3;   // fewer workgroups than compute units: quarter tiles
}

int sconv_check(int dtype, const SConvArgs& a) {
  MAUA_REQUIRE(dtype == MAUA_F32 || dtype == MAUA_BF16, "conv_strided: unsupported dtype");
  MAUA_REQUIRE(a.x && a.w && a.y, "conv_strided: NULL x / w / y");
  MAUA_REQUIRE(a.B >= 0 && a.H > 0 && a.W > 0, "conv_strided: bad shape");
  MAUA_REQUIRE(a.Co > 0 && a.Co % 64 == 0, "conv_strided: Co must be a multiple of 64");
  if (a.stem) {
    MAUA_REQUIRE(a.k == 7 && a.stride == 2 && a.pad == 3 && a.Ci == 3, "conv_strided: the stem is 7x7, stride 2, padding 3, 3 channels");
    MAUA_REQUIRE(!a.res, "conv_strided: the stem takes no residual");
    MAUA_REQUIRE(a.kpad == stem_kpad(dtype), "conv_strided: stem weights must be padded to stem_kpad");
  } else {
    const bool form = (a.k == 1 && a.pad == 0 && (a.stride == 1 || a.stride == 2)) || (a.k == 3 && a.pad == 1 && (a.stride == 1 || a.stride == 2));
    MAUA_REQUIRE(form, "conv_strided: (k, stride, padding) must be (1, 1, 0), (1, 2, 0), (3, 1, 1), (3, 2, 1) or the 7x7 stem");
    MAUA_REQUIRE(a.Ci > 0 && a.Ci % 64 == 0, "conv_strided: Ci must be a multiple of 64");
  }
  const long M = (long)a.B * sconv_out(a.H, a.k, a.stride, a.pad) * sconv_out(a.W, a.k, a.stride, a.pad);
  MAUA_REQUIRE((M + 63) / 64 <= 0x7fffffffL, "conv_strided: grid too large");
  MAUA_REQUIRE(aligned16(a.x) && aligned16(a.w) && aligned16(a.y) && aligned16(a.res) && aligned16(a.bias),
               "conv_strided: x, w, bias, res and y must be 16-byte aligned");
  return MAUA_OK;
}

int launch_sconv(hipStream_t st, int dtype, const SConvArgs& a) {
  if (int rc = sconv_check(dtype, a)) return rc;
  if (a.B == 0) return MAUA_OK;
  const long M = (long)a.B * sconv_out(a.H, a.k, a.stride, a.pad) * sconv_out(a.W, a.k, a.stride, a.pad);
  const int route = sconv_route(a);
  return dispatch_dtype<bf16_t, float>(dtype, "conv_strided", [&](auto t) {
    using T = decltype(t);
    if (route == 1)
      hipLaunchKernelGGL((sconv_kernel<T, 2, 1, true>), dim3((unsigned)((M + 127) / 128), a.Co / 64), dim3(256), 0, st, a);
    else if (route == 2)
      hipLaunchKernelGGL((sconv_kernel<T, 2, 2, false>), dim3((unsigned)((M + 127) / 128), a.Co / 128), dim3(256), 0, st, a);
    else
      hipLaunchKernelGGL((sconv_kernel<T, 1, 1, false>), dim3((unsigned)((M + 63) / 64), a.Co / 64), dim3(256), 0, st, a);
    MAUA_HIP_CHECK(hipGetLastError());
    return MAUA_OK;
  });
}

int launch_prep_stem_weights(hipStream_t st, int dtype, const float* w, void* wt, int Co) {
  const int kpad = stem_kpad(dtype);
  const long n = (long)Co * kpad;
  return dispatch_dtype<bf16_t, float>(dtype, "prep_stem_weights", [&](auto t) {
    using T = decltype(t);
    if (n == 0) return MAUA_OK;
    hipLaunchKernelGGL(prep_stem_weights_kernel<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, w, (T*)wt, Co, kpad);
    MAUA_HIP_CHECK(hipGetLastError());
    return MAUA_OK;
  });
}

int pool_check(const char* who, int dtype, const void* x, const void* y, int B, int H, int W, int C) {
  MAUA_REQUIRE(dtype == MAUA_F32 || dtype == MAUA_BF16, std::string(who) + ": unsupported dtype");
  MAUA_REQUIRE(x && y, std::string(who) + ": NULL argument");
  MAUA_REQUIRE(B >= 0 && H > 0 && W > 0 && C > 0 && C % 8 == 0, std::string(who) + ": bad shape (C must be a multiple of 8)");
  MAUA_REQUIRE(aligned16(x) && aligned16(y), std::string(who) + ": x and y must be 16-byte aligned");
  MAUA_REQUIRE(((long)B * H * W * (C / 4) + 255) / 256 <= 0x7fffffffL, std::string(who) + ": grid too large");
  return MAUA_OK;
}

int launch_maxpool3x3s2(hipStream_t st, int dtype, const void* x, void* y, int B, int H, int W, int C) {
  if (int rc = pool_check("maxpool3x3s2", dtype, x, y, B, H, W, C)) return rc;
  if (B == 0) return MAUA_OK;
  const int Ho = sconv_out(H, 3, 2, 1), Wo = sconv_out(W, 3, 2, 1);
  return dispatch_dtype<bf16_t, float>(dtype, "maxpool3x3s2", [&](auto t) {
    using T = decltype(t);
    const long n = (long)B * Ho * Wo * (C / (16 / (int)sizeof(T)));
    hipLaunchKernelGGL(maxpool3x3s2_kernel<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const T*)x, (T*)y, B, H, W, C, Ho, Wo);
    MAUA_HIP_CHECK(hipGetLastError());
    return MAUA_OK;
  });
}

int launch_global_avgpool(hipStream_t st, int dtype, const void* x, float* out, int B, int H, int W, int C) {
  if (int rc = pool_check("global_avgpool", dtype, x, out, B, H, W, C)) return rc;
  if (B == 0) return MAUA_OK;
  return dispatch_dtype<bf16_t, float>(dtype, "global_avgpool", [&](auto t) {
    using T = decltype(t);
    const long n = (long)B * C;
    hipLaunchKernelGGL(global_avgpool_kernel<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const T*)x, out, B, (long)H * W, C,
                       1.f / (float)((long)H * W));
    MAUA_HIP_CHECK(hipGetLastError());
    return MAUA_OK;
  });
}

}  // namespace maua

using namespace maua;

extern "C" int maua_conv_strided_ex(maua_ctx* ctx, const maua_sconv_desc* d, int dtype) {
  MAUA_REQUIRE(ctx && d, "maua_conv_strided_ex: NULL argument");
  SConvArgs a{};
  a.x = d->x; a.bias = d->bias; a.res = d->res; a.y = d->y;
  a.B = d->B; a.H = d->H; a.W = d->W; a.Ci = d->Ci; a.Co = d->Co; a.k = d->k; a.stride = d->stride; a.pad = d->pad;
  a.relu = d->relu != 0; a.stem = d->k == 7;
  a.kpad = a.stem ? stem_kpad(dtype) : 0;
  a.w = d->w;   // (checked for NULL with the rest; replaced by the prepared copy below)
  if (int rc = sconv_check(dtype, a)) return rc;
  if (d->B == 0) return MAUA_OK;
  const size_t es = elem_bytes(dtype);
  const size_t wt_bytes = (a.stem ? (size_t)d->Co * a.kpad : prepped_weight_elems(d->k, 1, d->Co, d->Ci)) * es;
  char* wt;
  if (int rc = carve_scratch(ctx, [&](Scratch& s) { wt = s.take<char>(wt_bytes); })) return rc;
  hipStream_t st = ctx->stream;
  if (a.stem) {
    if (int rc = launch_prep_stem_weights(st, dtype, d->w, wt, d->Co)) return rc;
  } else {
    if (int rc = launch_prep_weights(st, dtype, d->w, wt, nullptr, d->Co, d->Ci, d->k, 1, 0, d->Co, d->Ci)) return rc;
  }
  a.w = wt;
  return launch_sconv(st, dtype, a);
}

extern "C" int maua_maxpool3x3s2(maua_ctx* ctx, const void* x, void* y, int B, int H, int W, int C, int dtype) {
  MAUA_REQUIRE(ctx, "maua_maxpool3x3s2: ctx is NULL");
  return launch_maxpool3x3s2(ctx->stream, dtype, x, y, B, H, W, C);
}

extern "C" int maua_global_avgpool(maua_ctx* ctx, const void* x, float* out, int B, int H, int W, int C, int dtype) {
  MAUA_REQUIRE(ctx, "maua_global_avgpool: ctx is NULL");
  return launch_global_avgpool(ctx->stream, dtype, x, out, B, H, W, C);
}
