// The optical-flow operators of the video pipeline around guided diffusion (maua/diffusion/video.py, maua/flow/): the warp of an image
// along a flow, the forward / backward consistency map, the bilinear resize of flows and maps, the per-frame composition (warp, blend
// under the mask, wrap-around fade, injected noise) in one launch, the turbo in-between frame, and Farneback's dense flow estimator.
//
// Replaces (reference): flow/lib.py:51-63 flow_warp_map + diffusion/video.py:161-162 warp (F.grid_sample bilinear, reflection,
// align_corners=False; the grid is never materialised); flow/consistency.py:78-127 check_consistency with torchvision's
// gaussian_blur(kernel_size=3); diffusion/video.py:153-157 F.interpolate(mode="bilinear"); :248-277 the composition; :221-238 the turbo
// blend; flow/__init__.py:35-55 cv2.calcOpticalFlowFarneback(pyr_scale 0.8, levels 15, winsize 15, iterations 15, poly_n 7,
// poly_sigma 1.5, flags 10) on the host - here restated from the published algorithm (G. Farneback, "Two-frame motion estimation based
// on polynomial expansion", SCIA 2003; stage by stage as DESIGN 5e lists them), both directions of a pair in one batched launch per
// stage (grid z = direction).
//
// Planar f32 images [B][3][H][W], flows [B][H][W][2] in (x, y) order.  Every kernel is a gather with a fixed summation order: no
// atomics, a rerun is bit-identical.  No entry point allocates: the estimator's workspace is planned when its handle is created.
#include "common.h"
#include "internal.h"
#include "philox.h"

namespace maua {

namespace {

// ---------------------------------------------------------------------------------------------------------------- sampling rules
// torch.linspace(-1, 1, n)[i] in float32 (ATen: step = (end - start) / (n - 1); the first half counts up from start, the second down from end)
__device__ __forceinline__ float linspace_pm1(int i, int n) {
  if (n <= 1) return -1.f;
  const float step = 2.f / (float)(n - 1);
  return i < n / 2 ? __fadd_rn(-1.f, __fmul_rn(step, (float)i)) : __fsub_rn(1.f, __fmul_rn(step, (float)(n - i - 1)));
}

// grid_sample's reflection for align_corners=False: unnormalise ((g + 1) size - 1) / 2, reflect about -0.5 and size - 0.5, clip to
// [0, size - 1] (ATen grid_sampler_compute_source_index; resize.hip's reflect_coord is the align_corners=True form)
__device__ __forceinline__ float reflect_half_pixel(float g, int size) {
  float x = __fmul_rn(__fsub_rn(__fmul_rn(__fadd_rn(g, 1.f), (float)size), 1.f), 0.5f);
  const float span = (float)size;
  x = fabsf(__fadd_rn(x, 0.5f));
  const float extra = fmodf(x, span);
  const int flips = (int)floorf(x / span);
  x = (flips & 1) ? __fsub_rn(__fsub_rn(span, extra), 0.5f) : __fsub_rn(extra, 0.5f);
  return fminf(fmaxf(x, 0.f), (float)(size - 1));
}

struct WarpTaps {
  int x0, y0;
  float wnw, wne, wsw, wse;
};

// the sampling position of output pixel (x, y): grid = linspace(-1, 1, W)[x] + e flow_x / W (the reference divides by W and H, not by
// W / 2 and H / 2: flow/lib.py:53-54), then the reflection rule
__device__ __forceinline__ WarpTaps warp_taps(const float* __restrict__ flow, int x, int y, int H, int W, float e) {
  const float2 f = *reinterpret_cast<const float2*>(flow + ((long)y * W + x) * 2);
  const float gx = __fadd_rn(linspace_pm1(x, W), __fmul_rn(f.x, e) / (float)W);
  const float gy = __fadd_rn(linspace_pm1(y, H), __fmul_rn(f.y, e) / (float)H);
  const float sx = reflect_half_pixel(gx, W), sy = reflect_half_pixel(gy, H);
  const float fx = floorf(sx), fy = floorf(sy);
  const float tx = sx - fx, ty = sy - fy;
  WarpTaps t;
  t.x0 = (int)fx; t.y0 = (int)fy;
  t.wnw = (1.f - tx) * (1.f - ty); t.wne = tx * (1.f - ty); t.wsw = (1.f - tx) * ty; t.wse = tx * ty;
  return t;
}

__device__ __forceinline__ float warp_gather(const float* __restrict__ plane, const WarpTaps& t, int H, int W) {
  auto at = [&](int yy, int xx) -> float { return (yy >= 0 && yy < H && xx >= 0 && xx < W) ? plane[(long)yy * W + xx] : 0.f; };
  // grid_sample's order: nw, ne, sw, se
  float v = __fmul_rn(at(t.y0, t.x0), t.wnw);
  v = __fadd_rn(v, __fmul_rn(at(t.y0, t.x0 + 1), t.wne));
  v = __fadd_rn(v, __fmul_rn(at(t.y0 + 1, t.x0), t.wsw));
  return __fadd_rn(v, __fmul_rn(at(t.y0 + 1, t.x0 + 1), t.wse));
}

// ---------------------------------------------------------------------------------------------------------------- warp
__global__ __launch_bounds__(256) void warp_kernel(const float* __restrict__ img, const float* __restrict__ flow, float* __restrict__ out, int B,
                                                   int C, int H, int W, float e) {
  const long hw = (long)H * W, total = (long)B * hw;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int x = (int)(idx % W), y = (int)((idx / W) % H), b = (int)(idx / hw);
  const WarpTaps t = warp_taps(flow + (long)b * hw * 2, x, y, H, W, e);
  for (int c = 0; c < C; c++) {
    const long plane = ((long)b * C + c) * hw;
    out[plane + (long)y * W + x] = warp_gather(img + plane, t, H, W);
  }
}

// ---------------------------------------------------------------------------------------------------------------- consistency
__device__ __forceinline__ float clampf(float v, float c) { return fminf(fmaxf(v, -c), c); }

// check_consistency's classification (flow/consistency.py:94-124) of one pixel -> 1, 0 (motion boundary / overshoot) or -0.75 (missed)
__global__ __launch_bounds__(256) void consistency_classify_kernel(const float* __restrict__ fwd, const float* __restrict__ bwd, float* __restrict__ out,
                                                                   int B, int H, int W, float clampv) {
  const long hw = (long)H * W, total = (long)B * hw;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int x = (int)(idx % W), y = (int)((idx / W) % H);
  const float* fw = fwd + (idx / hw) * hw * 2;
  const float* bw = bwd + (idx / hw) * hw * 2;
  auto B2 = [&](int yy, int xx, int c) -> float { return (yy >= 0 && yy < H && xx >= 0 && xx < W) ? clampf(bw[((long)yy * W + xx) * 2 + c], clampv) : 0.f; };
  auto F2 = [&](int yy, int xx, int c) -> float { return (yy >= 0 && yy < H && xx >= 0 && xx < W) ? clampf(fw[((long)yy * W + xx) * 2 + c], clampv) : 0.f; };
  // central differences with zero "same" padding; the repeat(2, 2, 1, 1) kernel sums both input channels into each of the two output
  // channels, and cat([f_x, f_y]).square().sum() adds the two equal channels of each
  const float fxs = __fadd_rn(__fmul_rn(__fsub_rn(B2(y, x - 1, 0), B2(y, x + 1, 0)), 0.5f), __fmul_rn(__fsub_rn(B2(y, x - 1, 1), B2(y, x + 1, 1)), 0.5f));
  const float fys = __fadd_rn(__fmul_rn(__fsub_rn(B2(y - 1, x, 0), B2(y + 1, x, 0)), 0.5f), __fmul_rn(__fsub_rn(B2(y - 1, x, 1), B2(y + 1, x, 1)), 0.5f));
  const float motionedge = __fadd_rn(__fadd_rn(__fmul_rn(fxs, fxs), __fmul_rn(fxs, fxs)), __fadd_rn(__fmul_rn(fys, fys), __fmul_rn(fys, fys)));
  const float bx = B2(y, x, 0), by = B2(y, x, 1);
  const float p0x = __fadd_rn((float)x, bx), p0y = __fadd_rn((float)y, by);
  // sample(): grid = p0 / (max_pos / 2) - 1, grid_sample(bilinear, zeros, align_corners=True): ((g + 1) / 2) (size - 1)
  const float mx = (float)(W - 1), my = (float)(H - 1);
  const float ix = __fmul_rn(__fadd_rn(__fsub_rn(p0x / (mx / 2.f), 1.f), 1.f) / 2.f, mx);
  const float iy = __fmul_rn(__fadd_rn(__fsub_rn(p0y / (my / 2.f), 1.f), 1.f) / 2.f, my);
  float v0x = 0.f, v0y = 0.f;
  if (isfinite(ix) && isfinite(iy)) {
    const float flx = floorf(ix), fly = floorf(iy);
    const float tx = ix - flx, ty = iy - fly;
    // (int) of a float beyond the int range is undefined: positions that far out sample nothing
    if (flx > -2.f && flx < (float)W + 1.f && fly > -2.f && fly < (float)H + 1.f) {
      const int x0 = (int)flx, y0 = (int)fly;
      const float wnw = (1.f - tx) * (1.f - ty), wne = tx * (1.f - ty), wsw = (1.f - tx) * ty, wse = tx * ty;
      v0x = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(F2(y0, x0, 0), wnw), __fmul_rn(F2(y0, x0 + 1, 0), wne)), __fmul_rn(F2(y0 + 1, x0, 0), wsw)), __fmul_rn(F2(y0 + 1, x0 + 1, 0), wse));
      v0y = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(F2(y0, x0, 1), wnw), __fmul_rn(F2(y0, x0 + 1, 1), wne)), __fmul_rn(F2(y0 + 1, x0, 1), wsw)), __fmul_rn(F2(y0 + 1, x0 + 1, 1), wse));
    }
  }
  const float r1x = floorf(p0x), r1y = floorf(p0y);
  const bool overshoot = r1x < 0.f || __fadd_rn(r1x, 1.f) > mx || r1y < 0.f || __fadd_rn(r1y, 1.f) > my;
  const float ddx = __fsub_rn(__fadd_rn(p0x, v0x), (float)x), ddy = __fsub_rn(__fadd_rn(p0y, v0y), (float)y);
  const float lhs = __fadd_rn(__fmul_rn(ddx, ddx), __fmul_rn(ddy, ddy));
  // torch.stack([v1_back, v0]).square().sum(dim=(0, 1)): the four squares
  const float mag = __fadd_rn(__fadd_rn(__fmul_rn(bx, bx), __fmul_rn(by, by)), __fadd_rn(__fmul_rn(v0x, v0x), __fmul_rn(v0y, v0y)));
  const bool missed = lhs >= __fadd_rn(__fmul_rn(mag, 0.01f), 0.5f);
  const bool boundary = motionedge >= __fadd_rn(__fmul_rn(__fadd_rn(__fmul_rn(bx, bx), __fmul_rn(by, by)), 0.01f), 0.002f);
  float r = 1.f;
  if (boundary) r = 0.f;
  if (missed) r = -0.75f;
  if (overshoot) r = 0.f;
  out[idx] = r;
}

__device__ __forceinline__ int reflect101(int p, int n) {
  if (n == 1) return 0;
  const int period = 2 * (n - 1);
  int q = p % period;
  if (q < 0) q += period;
  return q < n ? q : period - q;
}

// torchvision gaussian_blur(kernel_size=3): sigma 0.8, taps exp(-0.5 (x / sigma)^2) at x = -1, 0, 1 normalised, reflect padding; clip(0, 1)
__global__ __launch_bounds__(256) void consistency_blur_kernel(const float* __restrict__ cls, float* __restrict__ out, int B, int H, int W, float k0, float k1) {
  const long hw = (long)H * W, total = (long)B * hw;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int x = (int)(idx % W), y = (int)((idx / W) % H);
  const float* p = cls + (idx / hw) * hw;
  const int xs[3] = {reflect101(x - 1, W), x, reflect101(x + 1, W)};
  const float kk[3] = {k1, k0, k1};
  float acc = 0.f;
#pragma unroll
  for (int j = 0; j < 3; j++) {
    const float* row = p + (long)reflect101(y - 1 + j, H) * W;
    const float h = row[xs[0]] * k1 + row[xs[1]] * k0 + row[xs[2]] * k1;
    acc += h * kk[j];
  }
  out[idx] = fminf(fmaxf(acc, 0.f), 1.f);
}

// ---------------------------------------------------------------------------------------------------------------- bilinear resize
// F.interpolate(mode="bilinear", align_corners=False) of channels-last [B][H][W][C] (ATen upsample_bilinear2d: source index
// max(0, (o + 0.5) in / out - 0.5), the right / lower tap clamped to the image); taps clamped to +-clampv, the result times mul
__global__ __launch_bounds__(256) void resize_bilinear_kernel(const float* __restrict__ src, float* __restrict__ dst, int B, int H, int W, int C, int Ho,
                                                              int Wo, float mul, float clampv) {
  const long total = (long)B * Ho * Wo * C;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int c = (int)(idx % C);
  long r = idx / C;
  const int ox = (int)(r % Wo); r /= Wo;
  const int oy = (int)(r % Ho);
  const int b = (int)(r / Ho);
  const float sy = fmaxf(__fsub_rn(__fmul_rn((float)oy + 0.5f, (float)H / (float)Ho), 0.5f), 0.f);
  const float sx = fmaxf(__fsub_rn(__fmul_rn((float)ox + 0.5f, (float)W / (float)Wo), 0.5f), 0.f);
  const int y0 = min((int)sy, H - 1), x0 = min((int)sx, W - 1);
  const int y1 = min(y0 + 1, H - 1), x1 = min(x0 + 1, W - 1);
  const float ly = sy - (float)y0, lx = sx - (float)x0;
  const float* p = src + (long)b * H * W * C + c;
  auto at = [&](int yy, int xx) -> float { return clampf(p[((long)yy * W + xx) * C], clampv); };
  const float top = (1.f - lx) * at(y0, x0) + lx * at(y0, x1);
  const float bot = (1.f - lx) * at(y1, x0) + lx * at(y1, x1);
  dst[idx] = ((1.f - ly) * top + ly * bot) * mul;
}

// ---------------------------------------------------------------------------------------------------------------- composition
struct ComposeArgs {
  const float* frame;        // [B][3][H][W]
  const float* prev;         // image to warp, or NULL (blend <= 0: init = frame)
  const float* flow;         // [B][H][W][2]
  const float* consistency;  // [B][H][W] or NULL (consistency_trust <= 0: mask = blend)
  const float* cached;       // wrap-around partner or NULL
  float* out;
  int B, H, W;
  float e, trust, blend, fade, noise_scale;
  uint32_t s0, s1;
};

// diffusion/video.py:248-277, four consecutive elements of [B][3][H][W] per thread (= one Philox counter of stream 0 of the seed:
// element i of the image is element i of maua_philox_normal(seed, stream 0))
__global__ __launch_bounds__(256) void compose_kernel(ComposeArgs a) {
  const long hw = (long)a.H * a.W, total = (long)a.B * 3 * hw;
  const unsigned long long cnt = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long base = (long)(cnt << 2);
  if (base >= total) return;
  float z[4] = {0.f, 0.f, 0.f, 0.f};
  if (a.noise_scale != 0.f) {
    const U4 v = philox4x32_10((uint32_t)cnt, (uint32_t)(cnt >> 32), 0u, 0u, a.s0, a.s1);
    box_muller(v.x, v.y, z[0], z[1]);
    box_muller(v.z, v.w, z[2], z[3]);
  }
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const long i = base + k;
    if (i >= total) break;
    const int x = (int)(i % a.W), y = (int)((i / a.W) % a.H);
    const long plane = i / hw;            // b * 3 + c
    const long b = plane / 3;
    float v = a.frame[i];
    if (a.prev) {
      float mask = a.blend;
      if (a.consistency) mask = __fmul_rn(__fadd_rn(__fmul_rn(a.consistency[b * hw + (long)y * a.W + x], a.trust), __fsub_rn(1.f, a.trust)), a.blend);
      const WarpTaps t = warp_taps(a.flow + b * hw * 2, x, y, a.H, a.W, a.e);
      const float w = warp_gather(a.prev + plane * hw, t, a.H, a.W);
      v = __fadd_rn(v, __fmul_rn(mask, w)) / __fadd_rn(1.f, mask);
    }
    if (a.cached) v = __fadd_rn(__fmul_rn(a.fade, v), __fmul_rn(__fsub_rn(1.f, a.fade), a.cached[i]));
    if (a.noise_scale != 0.f) v = __fadd_rn(v, __fmul_rn(a.noise_scale, z[k]));
    a.out[i] = v;
  }
}

// ---------------------------------------------------------------------------------------------------------------- turbo
// diffusion/video.py:225-235 for one skipped frame: prev_out = warp(prev), next_out = warp(next) when warp_next, img = prev_out (1 - b) +
// next b (the warped next, or next as it is), or next alone without a prev
__global__ __launch_bounds__(256) void turbo_kernel(const float* __restrict__ prev, const float* __restrict__ next, const float* __restrict__ flow,
                                                    float* __restrict__ prev_out, float* __restrict__ next_out, float* __restrict__ img, int B, int H, int W,
                                                    float e, int warp_next, float bt) {
  const long hw = (long)H * W, total = (long)B * hw;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int x = (int)(idx % W), y = (int)((idx / W) % H);
  const long b = idx / hw;
  const WarpTaps t = warp_taps(flow + b * hw * 2, x, y, H, W, e);
  for (int c = 0; c < 3; c++) {
    const long plane = (b * 3 + c) * hw, o = plane + (long)y * W + x;
    float n = warp_next ? warp_gather(next + plane, t, H, W) : next[o];
    if (warp_next) next_out[o] = n;
    if (prev) {
      const float p = warp_gather(prev + plane, t, H, W);
      prev_out[o] = p;
      n = __fadd_rn(__fmul_rn(p, __fsub_rn(1.f, bt)), __fmul_rn(n, bt));
    }
    img[o] = n;
  }
}

// ---------------------------------------------------------------------------------------------------------------- Farneback
constexpr int FB_POLY_N = 7, FB_WIN = 15, FB_WIN_R = 7, FB_ITERS = 15, FB_MAX_LEVELS = 15, FB_MIN_SIZE = 32;
// the widest pyramid blur: 15 levels down, scale 0.8^15, sigma 13.7, round(5 sigma) | 1 = 69 taps
constexpr int FB_MAX_TAPS = 71;
constexpr double FB_PYR_SCALE = 0.8, FB_POLY_SIGMA = 1.5;

struct Taps {
  float t[FB_MAX_TAPS];
  int radius;
};
struct PolyTaps {
  float g[FB_POLY_N + 1], xg[FB_POLY_N + 1], xxg[FB_POLY_N + 1];
  float ig11, ig03, ig33, ig55;
};

// luminance(im).mul(255).byte() (flow/__init__.py:41-42 with ops/image.py:176-177) as float32; z = image of the pair.  The byte is a
// truncation, so the float32 value has to be torch's to the last bit: every product and sum is rounded on its own.  __fmul_rn / __fadd_rn
// are plain operators inside a header to this compiler and were contracted into an fma (0.7152 g + 0.2126 r in one rounding), which
// moved a luminance one ulp below an integer and the pixel one grey level down; the pragma governs the operators written in this body.
__global__ __launch_bounds__(256) void fb_gray_kernel(const float* __restrict__ im_a, const float* __restrict__ im_b, float* __restrict__ gray, long hw) {
#pragma clang fp contract(off)
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= hw) return;
  const float* im = blockIdx.z == 0 ? im_a : im_b;
  const float lum = (0.2126f * im[idx] + 0.7152f * im[hw + idx]) + 0.0722f * im[2 * hw + idx];
  const float v = fminf(fmaxf(lum * 255.f, 0.f), 255.f);
  gray[(long)blockIdx.z * hw + idx] = (float)(int)v;
}

// one axis of the pyramid's Gaussian blur, reflect-101 border; z = image
template <int AXIS>
__global__ __launch_bounds__(256) void fb_blur_kernel(const float* __restrict__ src, float* __restrict__ dst, int H, int W, Taps taps) {
  const long hw = (long)H * W;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= hw) return;
  const int x = (int)(idx % W), y = (int)(idx / W);
  const float* p = src + (long)blockIdx.z * hw;
  float acc = 0.f;
  for (int k = -taps.radius; k <= taps.radius; k++) {
    const int sy = AXIS == 0 ? reflect101(y + k, H) : y, sx = AXIS == 1 ? reflect101(x + k, W) : x;
    acc += p[(long)sy * W + sx] * taps.t[k + taps.radius];
  }
  dst[(long)blockIdx.z * hw + idx] = acc;
}

// bilinear resize with pixel-centre mapping and a replicated edge (src = (dst + 0.5) in / out - 0.5; below 0: the first sample, at or past
// the last: the last) of channels-last [z][Hs][Ws][C], times mul; columns first, then rows
__global__ __launch_bounds__(256) void fb_resize_kernel(const float* __restrict__ src, float* __restrict__ dst, int Hs, int Ws, int Hd, int Wd, int C, float mul) {
  const long total = (long)Hd * Wd * C;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int c = (int)(idx % C), ox = (int)((idx / C) % Wd), oy = (int)(idx / ((long)C * Wd));
  auto coord = [](int o, int n_in, int n_out, int& i0, float& t) {
    const float f = (float)(((double)o + 0.5) * ((double)n_in / (double)n_out) - 0.5);
    i0 = (int)floorf(f);
    t = f - (float)i0;
    if (i0 < 0) { i0 = 0; t = 0.f; }
    if (i0 >= n_in - 1) { i0 = n_in - 1; t = 0.f; }
  };
  int x0, y0;
  float tx, ty;
  coord(ox, Ws, Wd, x0, tx);
  coord(oy, Hs, Hd, y0, ty);
  const int x1 = min(x0 + 1, Ws - 1), y1 = min(y0 + 1, Hs - 1);
  const float* p = src + (long)blockIdx.z * Hs * Ws * C + c;
  const float top = p[((long)y0 * Ws + x0) * C] * (1.f - tx) + p[((long)y0 * Ws + x1) * C] * tx;
  const float bot = p[((long)y1 * Ws + x0) * C] * (1.f - tx) + p[((long)y1 * Ws + x1) * C] * tx;
  dst[(long)blockIdx.z * total + idx] = (top * (1.f - ty) + bot * ty) * mul;
}

// polynomial expansion, vertical pass: I [z][h][w] -> T [z][3][h][w] = (g, y g, y^2 g) * I along y, replicated border
__global__ __launch_bounds__(256) void fb_poly_v_kernel(const float* __restrict__ I, float* __restrict__ T, int h, int w, PolyTaps pt) {
  const long hw = (long)h * w;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= hw) return;
  const int x = (int)(idx % w), y = (int)(idx / w);
  const float* p = I + (long)blockIdx.z * hw;
  float t0 = p[idx] * pt.g[0], t1 = 0.f, t2 = 0.f;
#pragma unroll
  for (int k = 1; k <= FB_POLY_N; k++) {
    const float lo = p[(long)max(y - k, 0) * w + x], hi = p[(long)min(y + k, h - 1) * w + x];
    const float s = lo + hi;
    t0 += pt.g[k] * s;
    t1 += pt.xg[k] * (hi - lo);
    t2 += pt.xxg[k] * s;
  }
  float* o = T + (long)blockIdx.z * 3 * hw;
  o[idx] = t0; o[hw + idx] = t1; o[2 * hw + idx] = t2;
}

// ... horizontal pass: T -> R [z][5][h][w] = the coefficients of x, y, x^2, y^2, xy, scaled by the inverted moment matrix's entries
__global__ __launch_bounds__(256) void fb_poly_h_kernel(const float* __restrict__ T, float* __restrict__ R, int h, int w, PolyTaps pt) {
  const long hw = (long)h * w;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= hw) return;
  const int x = (int)(idx % w), y = (int)(idx / w);
  const float* r0 = T + (long)blockIdx.z * 3 * hw + (long)y * w;
  const float *r1 = r0 + hw, *r2 = r0 + 2 * hw;
  float b1 = r0[x] * pt.g[0], b2 = 0.f, b3 = r1[x] * pt.g[0], b4 = 0.f, b5 = r2[x] * pt.g[0], b6 = 0.f;
#pragma unroll
  for (int k = 1; k <= FB_POLY_N; k++) {
    const int xl = max(x - k, 0), xr = min(x + k, w - 1);
    const float tg = r0[xr] + r0[xl];
    b1 += tg * pt.g[k];
    b4 += tg * pt.xxg[k];
    b2 += (r0[xr] - r0[xl]) * pt.xg[k];
    b3 += (r1[xr] + r1[xl]) * pt.g[k];
    b6 += (r1[xr] - r1[xl]) * pt.xg[k];
    b5 += (r2[xr] + r2[xl]) * pt.g[k];
  }
  float* o = R + (long)blockIdx.z * 5 * hw + idx;
  o[0] = b2 * pt.ig11;
  o[hw] = b3 * pt.ig11;
  o[2 * hw] = b1 * pt.ig03 + b4 * pt.ig33;
  o[3 * hw] = b1 * pt.ig03 + b5 * pt.ig33;
  o[4 * hw] = b6 * pt.ig55;
}

// the update matrices of one pixel from the first image's coefficients R0, the second's R1 sampled at (x + dx, y + dy), and the flow
__device__ __forceinline__ void fb_matrices(const float* __restrict__ R0, const float* __restrict__ R1, int x, int y, int h, int w, float dx, float dy,
                                            float (&m)[5]) {
  const long hw = (long)h * w, o = (long)y * w + x;
  const float fx = (float)x + dx, fy = (float)y + dy;
  const float flx = floorf(fx), fly = floorf(fy);
  float r2, r3, r4, r5, r6;
  if (flx >= 0.f && flx < (float)(w - 1) && fly >= 0.f && fly < (float)(h - 1)) {
    const int x1 = (int)flx, y1 = (int)fly;
    const float tx = fx - flx, ty = fy - fly;
    const float a00 = (1.f - tx) * (1.f - ty), a01 = tx * (1.f - ty), a10 = (1.f - tx) * ty, a11 = tx * ty;
    const long q = (long)y1 * w + x1;
    auto s = [&](int c) -> float { const float* p = R1 + c * hw + q; return a00 * p[0] + a01 * p[1] + a10 * p[w] + a11 * p[w + 1]; };
    r2 = s(0);
    r3 = s(1);
    r4 = (R0[2 * hw + o] + s(2)) * 0.5f;
    r5 = (R0[3 * hw + o] + s(3)) * 0.5f;
    r6 = (R0[4 * hw + o] + s(4)) * 0.25f;
  } else {
    r2 = r3 = 0.f;
    r4 = R0[2 * hw + o];
    r5 = R0[3 * hw + o];
    r6 = R0[4 * hw + o] * 0.5f;
  }
  r2 = (R0[o] - r2) * 0.5f;
  r3 = (R0[hw + o] - r3) * 0.5f;
  r2 += r4 * dx + r6 * dy;
  r3 += r6 * dx + r5 * dy;
  const float border[5] = {0.14f, 0.14f, 0.4472f, 0.4472f, 0.4472f};
  if (x < 5 || x >= w - 5 || y < 5 || y >= h - 5) {
    const float sc = (x < 5 ? border[x] : 1.f) * (x >= w - 5 ? border[w - x - 1] : 1.f) * (y < 5 ? border[y] : 1.f) * (y >= h - 5 ? border[h - y - 1] : 1.f);
    r2 *= sc; r3 *= sc; r4 *= sc; r5 *= sc; r6 *= sc;
  }
  m[0] = r4 * r4 + r6 * r6;
  m[1] = (r4 + r5) * r6;
  m[2] = r5 * r5 + r6 * r6;
  m[3] = r4 * r2 + r6 * r3;
  m[4] = r6 * r2 + r5 * r3;
}

// R [2][5][h][w] (image 0, image 1), flow [2][h][w][2], M [2][5][h][w]; z = direction: 0 first image -> second, 1 the reverse
__global__ __launch_bounds__(256) void fb_matrices_kernel(const float* __restrict__ R, const float* __restrict__ flow, float* __restrict__ M, int h, int w) {
  const long hw = (long)h * w;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= hw) return;
  const int d = blockIdx.z;
  const float2 f = *reinterpret_cast<const float2*>(flow + ((long)d * hw + idx) * 2);
  float m[5];
  fb_matrices(R + (long)d * 5 * hw, R + (long)(1 - d) * 5 * hw, (int)(idx % w), (int)(idx / w), h, w, f.x, f.y, m);
#pragma unroll
  for (int c = 0; c < 5; c++) M[((long)d * 5 + c) * hw + idx] = m[c];
}

// One iteration: the 15 x 15 box sum of M (replicated border) through an LDS band - the tile and its halo of 7 are loaded per channel,
// summed along x into a second band, then along y - the 2 x 2 solve, the flow store, and (all iterations but the last) the update
// matrices of the new flow into M_out.  M_out is a second buffer: a neighbouring tile's halo still reads M_in.
constexpr int FB_TW = 32, FB_TH = 8, FB_LW = FB_TW + 2 * FB_WIN_R, FB_LH = FB_TH + 2 * FB_WIN_R;

__global__ __launch_bounds__(FB_TW * FB_TH) void fb_iterate_kernel(const float* __restrict__ M_in, float* __restrict__ M_out, const float* __restrict__ R,
                                                                   float* __restrict__ flow, int h, int w, int update) {
  __shared__ float tile[FB_LH][FB_LW];
  __shared__ float hsum[FB_LH][FB_TW];
  const long hw = (long)h * w;
  const int d = blockIdx.z, tx = threadIdx.x, ty = threadIdx.y, tid = ty * FB_TW + tx;
  const int x0 = blockIdx.x * FB_TW, y0 = blockIdx.y * FB_TH;
  const int x = x0 + tx, y = y0 + ty;
  float g[5];
  for (int c = 0; c < 5; c++) {
    const float* p = M_in + ((long)d * 5 + c) * hw;
    for (int i = tid; i < FB_LH * FB_LW; i += FB_TW * FB_TH) {
      const int ly = i / FB_LW, lx = i % FB_LW;
      const int sy = min(max(y0 - FB_WIN_R + ly, 0), h - 1), sx = min(max(x0 - FB_WIN_R + lx, 0), w - 1);
      tile[ly][lx] = p[(long)sy * w + sx];
    }
    __syncthreads();
    for (int i = tid; i < FB_LH * FB_TW; i += FB_TW * FB_TH) {
      const int ly = i / FB_TW, lx = i % FB_TW;
      float s = 0.f;
#pragma unroll
      for (int k = 0; k < FB_WIN; k++) s += tile[ly][lx + k];
      hsum[ly][lx] = s;
    }
    __syncthreads();
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < FB_WIN; k++) s += hsum[ty + k][tx];
    g[c] = s * (1.f / (float)(FB_WIN * FB_WIN));
    // (the next channel's tile store is ordered behind this read by the barrier after it; hsum's by the one after that)
  }
  if (x >= w || y >= h) return;
  const float idet = 1.f / (g[0] * g[2] - g[1] * g[1] + 1e-3f);
  const float fx = (g[2] * g[3] - g[1] * g[4]) * idet, fy = (g[0] * g[4] - g[1] * g[3]) * idet;
  const long o = (long)y * w + x;
  *reinterpret_cast<float2*>(flow + ((long)d * hw + o) * 2) = make_float2(fx, fy);
  if (update) {
    float m[5];
    fb_matrices(R + (long)d * 5 * hw, R + (long)(1 - d) * 5 * hw, x, y, h, w, fx, fy, m);
#pragma unroll
    for (int c = 0; c < 5; c++) M_out[((long)d * 5 + c) * hw + o] = m[c];
  }
}

inline unsigned blocks(long n) { return (unsigned)((n + 255) / 256); }

inline long round_half_even(double v) { return (long)nearbyint(v); }

// entries (1,1), (0,3), (3,3), (5,5) of the inverse of the 6 x 6 moment matrix of the basis 1, x, y, x^2, y^2, xy under the separable
// Gaussian applicability, in double
void poly_setup(PolyTaps& pt) {
  const int n = FB_POLY_N;
  double g[2 * FB_POLY_N + 1], s = 0;
  for (int x = -n; x <= n; x++) s += g[x + n] = std::exp(-x * x / (2 * FB_POLY_SIGMA * FB_POLY_SIGMA));
  for (int x = -n; x <= n; x++) g[x + n] /= s;
  // the taps are rounded to float32 first, and the moments are taken of the rounded taps
  float gf[2 * FB_POLY_N + 1];
  for (int x = -n; x <= n; x++) gf[x + n] = (float)g[x + n];
  for (int k = 0; k <= n; k++) {
    pt.g[k] = gf[k + n];
    pt.xg[k] = (float)(k * (double)gf[k + n]);
    pt.xxg[k] = (float)(k * k * (double)gf[k + n]);
  }
  double G[6][6] = {};
  for (int y = -n; y <= n; y++)
    for (int x = -n; x <= n; x++) {
      const double wgt = (double)gf[y + n] * (double)gf[x + n];
      G[0][0] += wgt;
      G[1][1] += wgt * x * x;
      G[3][3] += wgt * x * x * x * x;
      G[5][5] += wgt * x * x * y * y;
    }
  G[2][2] = G[0][3] = G[0][4] = G[3][0] = G[4][0] = G[1][1];
  G[4][4] = G[3][3];
  G[3][4] = G[4][3] = G[5][5];
  // Gauss-Jordan inverse (symmetric positive definite, 6 x 6)
  double A[6][12];
  for (int i = 0; i < 6; i++)
    for (int j = 0; j < 12; j++) A[i][j] = j < 6 ? G[i][j] : (j - 6 == i ? 1.0 : 0.0);
  for (int i = 0; i < 6; i++) {
    int piv = i;
    for (int r = i + 1; r < 6; r++)
      if (std::fabs(A[r][i]) > std::fabs(A[piv][i])) piv = r;
    if (piv != i)
      for (int j = 0; j < 12; j++) std::swap(A[i][j], A[piv][j]);
    const double inv = 1.0 / A[i][i];
    for (int j = 0; j < 12; j++) A[i][j] *= inv;
    for (int r = 0; r < 6; r++)
      if (r != i) {
        const double f = A[r][i];
        for (int j = 0; j < 12; j++) A[r][j] -= f * A[i][j];
      }
  }
  pt.ig11 = (float)A[1][7];
  pt.ig03 = (float)A[0][9];
  pt.ig33 = (float)A[3][9];
  pt.ig55 = (float)A[5][11];
}

// the pyramid blur's taps for a level: exp(-x^2 / 2 sigma^2) normalised, size max(round(5 sigma) | 1, 3); sigma 0: [0.25, 0.5, 0.25]
void blur_taps(double sigma, Taps& t) {
  int ksize = (int)(round_half_even(sigma * 5) | 1);
  if (ksize < 3) ksize = 3;
  t.radius = ksize / 2;
  if (sigma <= 0) {
    t.t[0] = 0.25f; t.t[1] = 0.5f; t.t[2] = 0.25f;
    return;
  }
  double v[FB_MAX_TAPS], s = 0;
  for (int i = 0; i < ksize; i++) {
    const double x = i - t.radius;
    s += v[i] = std::exp(-x * x / (2 * sigma * sigma));
  }
  for (int i = 0; i < ksize; i++) t.t[i] = (float)(v[i] / s);
}

int pyramid_levels(int H, int W) {
  int k = 0;
  double scale = 1;
  for (; k < FB_MAX_LEVELS; k++) {
    scale *= FB_PYR_SCALE;
    if (W * scale < FB_MIN_SIZE || H * scale < FB_MIN_SIZE) break;
  }
  return k;
}

}  // namespace

}  // namespace maua

using namespace maua;

struct maua_farneback {
  int device = 0, max_h = 0, max_w = 0;
  DevBuf ws;   // float
  PolyTaps poly;
};

extern "C" {

int maua_flow_warp(maua_ctx* ctx, const float* img, const float* flow, float exaggeration, int B, int C, int H, int W, float* out) {
  MAUA_REQUIRE(ctx, "maua_flow_warp: ctx is NULL");
  MAUA_REQUIRE(B >= 0 && C >= 0 && H >= 0 && W >= 0, "maua_flow_warp: negative size");
  const long total = (long)B * H * W;
  if (total == 0 || C == 0) return MAUA_OK;
  MAUA_REQUIRE(img && flow && out && img != out, "maua_flow_warp: NULL or aliased argument");
  hipLaunchKernelGGL(warp_kernel, dim3(blocks(total)), dim3(256), 0, ctx->stream, img, flow, out, B, C, H, W, exaggeration);
  MAUA_HIP_CHECK(hipGetLastError());
  return MAUA_OK;
}

int maua_flow_consistency(maua_ctx* ctx, const float* forward, const float* backward, int B, int H, int W, float clamp, float* classes, float* out) {
  MAUA_REQUIRE(ctx, "maua_flow_consistency: ctx is NULL");
  MAUA_REQUIRE(B >= 0 && H >= 0 && W >= 0, "maua_flow_consistency: negative size");
  const long total = (long)B * H * W;
  if (total == 0) return MAUA_OK;
  MAUA_REQUIRE(forward && backward && classes && out && classes != out, "maua_flow_consistency: NULL or aliased argument");
  MAUA_REQUIRE(H >= 2 && W >= 2, "maua_flow_consistency: the map needs at least 2 x 2 pixels");
  MAUA_REQUIRE(clamp > 0, "maua_flow_consistency: clamp must be positive (INFINITY: none)");
  // torchvision _get_gaussian_kernel1d(3, 0.8) in float32
  const float e = std::exp(-0.5f * (1.f / 0.8f) * (1.f / 0.8f)), s = 1.f + 2.f * e;
  hipLaunchKernelGGL(consistency_classify_kernel, dim3(blocks(total)), dim3(256), 0, ctx->stream, forward, backward, classes, B, H, W, clamp);
  hipLaunchKernelGGL(consistency_blur_kernel, dim3(blocks(total)), dim3(256), 0, ctx->stream, (const float*)classes, out, B, H, W, 1.f / s, e / s);
  MAUA_HIP_CHECK(hipGetLastError());
  return MAUA_OK;
}

int maua_flow_resize_bilinear(maua_ctx* ctx, const float* src, int B, int H, int W, int C, float* dst, int out_h, int out_w, float multiplier,
                              float clamp) {
  MAUA_REQUIRE(ctx, "maua_flow_resize_bilinear: ctx is NULL");
  MAUA_REQUIRE(B >= 0 && C >= 0 && out_h >= 0 && out_w >= 0, "maua_flow_resize_bilinear: negative size");
  const long total = (long)B * out_h * out_w * C;
  if (total == 0) return MAUA_OK;
  MAUA_REQUIRE(src && dst && src != dst && H > 0 && W > 0, "maua_flow_resize_bilinear: NULL, aliased or empty input");
  MAUA_REQUIRE(clamp > 0, "maua_flow_resize_bilinear: clamp must be positive (INFINITY: none)");
  hipLaunchKernelGGL(resize_bilinear_kernel, dim3(blocks(total)), dim3(256), 0, ctx->stream, src, dst, B, H, W, C, out_h, out_w, multiplier, clamp);
  MAUA_HIP_CHECK(hipGetLastError());
  return MAUA_OK;
}

int maua_flow_compose(maua_ctx* ctx, const float* frame, const float* prev, const float* flow, const float* consistency, const float* cached,
                      int B, int H, int W, float exaggeration, float trust, float blend, float fade, float noise_scale, unsigned long long seed,
                      float* out) {
  MAUA_REQUIRE(ctx, "maua_flow_compose: ctx is NULL");
  MAUA_REQUIRE(B >= 0 && H >= 0 && W >= 0, "maua_flow_compose: negative size");
  const long total = (long)B * 3 * H * W;
  if (total == 0) return MAUA_OK;
  MAUA_REQUIRE(frame && out, "maua_flow_compose: NULL argument");
  MAUA_REQUIRE(!prev || (flow && prev != out), "maua_flow_compose: a previous image needs its flow and must not be the output");
  MAUA_REQUIRE(!consistency || prev, "maua_flow_compose: a consistency map goes with a previous image");
  ComposeArgs a{frame, prev, flow, consistency, cached, out, B, H, W, exaggeration, trust, blend, fade, noise_scale, (uint32_t)seed,
                (uint32_t)(seed >> 32)};
  hipLaunchKernelGGL(compose_kernel, dim3(blocks((total + 3) / 4)), dim3(256), 0, ctx->stream, a);
  MAUA_HIP_CHECK(hipGetLastError());
  return MAUA_OK;
}

int maua_flow_turbo(maua_ctx* ctx, const float* prev, const float* next, const float* flow, int B, int H, int W, float exaggeration, int warp_next,
                    float blend_t, float* prev_out, float* next_out, float* img) {
  MAUA_REQUIRE(ctx, "maua_flow_turbo: ctx is NULL");
  MAUA_REQUIRE(B >= 0 && H >= 0 && W >= 0, "maua_flow_turbo: negative size");
  const long total = (long)B * H * W;
  if (total == 0) return MAUA_OK;
  MAUA_REQUIRE(next && flow && img && img != next && img != prev, "maua_flow_turbo: NULL or aliased argument");
  MAUA_REQUIRE(!prev || (prev_out && prev_out != prev && prev_out != next && prev_out != img), "maua_flow_turbo: prev needs a separate prev_out");
  MAUA_REQUIRE(!warp_next || (next_out && next_out != next && next_out != prev && next_out != img && next_out != prev_out),
               "maua_flow_turbo: warp_next needs a separate next_out");
  hipLaunchKernelGGL(turbo_kernel, dim3(blocks(total)), dim3(256), 0, ctx->stream, prev, next, flow, prev_out, next_out, img, B, H, W, exaggeration,
                     warp_next, blend_t);
  MAUA_HIP_CHECK(hipGetLastError());
  return MAUA_OK;
}

// floats of workspace per pixel of the largest pair: gray 2, blur scratch 2 + 2, level images 2, polynomial scratch 6, coefficients 10,
// two flow buffers 4 + 4, two matrix buffers 10 + 10
static constexpr long FB_WS_FLOATS_PER_PIXEL = 52;

int maua_farneback_levels(int H, int W) { return (H > 0 && W > 0) ? pyramid_levels(H, W) + 1 : 0; }

int maua_farneback_create(maua_ctx* ctx, int max_h, int max_w, maua_farneback** out) {
  MAUA_REQUIRE(ctx && out, "maua_farneback_create: NULL argument");
  MAUA_REQUIRE(max_h >= 2 * FB_POLY_N + 1 && max_w >= 2 * FB_POLY_N + 1 && (long)max_h * max_w <= (1L << 26),
               "maua_farneback_create: the largest image must be between 15 x 15 and 2^26 pixels");
  MAUA_HIP_CHECK(hipSetDevice(ctx->device));
  auto* h = new maua_farneback();
  h->device = ctx->device; h->max_h = max_h; h->max_w = max_w;
  if (h->ws.alloc((size_t)FB_WS_FLOATS_PER_PIXEL * max_h * max_w * sizeof(float))) {
    delete h;
    return fail_in("maua_farneback_create");
  }
  poly_setup(h->poly);
  *out = h;
  return MAUA_OK;
}

int maua_farneback_destroy(maua_farneback* h) {
  if (!h) return MAUA_OK;
  delete h;
  return MAUA_OK;
}

namespace {

// the size of pyramid level k and the standard deviation of its blur, as the launcher computes them
void level_geometry(int H, int W, int k, int& h, int& w, double& sigma) {
  double scale = 1;
  for (int i = 0; i < k; i++) scale *= FB_PYR_SCALE;
  sigma = (1. / scale - 1) * 0.5;
  w = (int)round_half_even(W * scale);
  h = (int)round_half_even(H * scale);
}

// every refusal of the estimator, in front of the first launch; fb NULL: the descriptor alone (no handle exists without a device).
// The levels of the range and the iteration count go out through hi / lo / iters.
int farneback_check(const maua_farneback* fb, const maua_farneback_desc* d, int& hi, int& lo, int& iters) {
  MAUA_REQUIRE(d, "maua_farneback: the descriptor is NULL");
  MAUA_REQUIRE(d->im_a && d->im_b && d->flow_ab && d->flow_ba && d->flow_ab != d->flow_ba && d->flow_ab != d->im_a && d->flow_ab != d->im_b &&
                   d->flow_ba != d->im_a && d->flow_ba != d->im_b,
               "maua_farneback: NULL or aliased argument");
  MAUA_REQUIRE(d->H >= 2 * FB_POLY_N + 1 && d->W >= 2 * FB_POLY_N + 1, "maua_farneback: the image must be at least 15 x 15");
  MAUA_REQUIRE((long)d->H * d->W <= (1L << 26), "maua_farneback: the image exceeds 2^26 pixels");
  MAUA_REQUIRE(!fb || (long)d->H * d->W <= (long)fb->max_h * fb->max_w, "maua_farneback: the image exceeds the size the handle was created for");
  const int top = pyramid_levels(d->H, d->W);
  hi = d->level_hi, lo = d->level_lo;
  if (hi == -1 && lo == -1) { hi = top; lo = 0; }
  MAUA_REQUIRE(lo >= 0 && hi >= lo, "maua_farneback: level_hi .. level_lo must run downwards to a level >= 0 (-1, -1: every level)");
  MAUA_REQUIRE(hi <= top, "maua_farneback: level_hi is above the top level of this size (maua_farneback_levels - 1)");
  MAUA_REQUIRE(d->iterations >= 0 && d->iterations <= FB_ITERS, "maua_farneback: iterations must be 1 .. 15 (0: 15)");
  iters = d->iterations ? d->iterations : FB_ITERS;
  MAUA_REQUIRE((d->init_ab != nullptr) == (d->init_ba != nullptr), "maua_farneback: init_ab and init_ba go together");
  MAUA_REQUIRE(!d->init_ab || (d->init_ab != d->init_ba && d->init_ab != d->flow_ab && d->init_ab != d->flow_ba && d->init_ba != d->flow_ab &&
                               d->init_ba != d->flow_ba),
               "maua_farneback: the initial flows must not alias each other or the outputs");
  for (int k = hi; k >= lo; k--) {
    int h, w;
    double sigma;
    level_geometry(d->H, d->W, k, h, w, sigma);
    int ksize = (int)(round_half_even(sigma * 5) | 1);
    if (ksize < 3) ksize = 3;
    MAUA_REQUIRE(ksize <= FB_MAX_TAPS && ksize / 2 < d->H && ksize / 2 < d->W, "maua_farneback: pyramid blur wider than the image");
  }
  return MAUA_OK;
}

}  // namespace

int maua_farneback_level_size(int H, int W, int level, int* h, int* w) {
  MAUA_REQUIRE(h && w, "maua_farneback_level_size: NULL argument");
  MAUA_REQUIRE(H > 0 && W > 0 && level >= 0 && level <= pyramid_levels(H, W), "maua_farneback_level_size: no such level at this size");
  double sigma;
  level_geometry(H, W, level, *h, *w, sigma);
  return MAUA_OK;
}

int maua_farneback_check(const maua_farneback* fb, const maua_farneback_desc* d) {
  int hi, lo, iters;
  return farneback_check(fb, d, hi, lo, iters);
}

int maua_farneback_pair_ex(maua_farneback* fb, maua_ctx* ctx, const maua_farneback_desc* d) {
  MAUA_REQUIRE(fb && ctx, "maua_farneback: NULL handle or ctx");
  MAUA_REQUIRE(ctx->device == fb->device, "maua_farneback: the handle belongs to another device");
  int hi, lo, iters;
  if (farneback_check(fb, d, hi, lo, iters) != MAUA_OK) return MAUA_ERR;
  const int H = d->H, W = d->W;
  hipStream_t st = ctx->stream;
  const long n = (long)H * W;
  float* p = fb->ws.as<float>();
  float* gray = p;  p += 2 * n;
  float* tmp = p;   p += 2 * n;
  float* blur = p;  p += 2 * n;
  float* lvl = p;   p += 2 * n;
  float* pt = p;    p += 6 * n;
  float* R = p;     p += 10 * n;
  float* fl[2];
  fl[0] = p;        p += 4 * n;
  fl[1] = p;        p += 4 * n;
  float* M[2];
  M[0] = p;         p += 10 * n;
  M[1] = p;
  // a dump: a device-to-device copy out of the workspace behind the stage that filled it (stream order)
  auto dump = [&](float* dst, const float* src, long floats) -> hipError_t {
    return dst ? hipMemcpyAsync(dst, src, (size_t)floats * sizeof(float), hipMemcpyDeviceToDevice, st) : hipSuccess;
  };
  hipLaunchKernelGGL(fb_gray_kernel, dim3(blocks(n), 1, 2), dim3(256), 0, st, d->im_a, d->im_b, gray, n);
  MAUA_HIP_CHECK(dump(d->gray, gray, 2 * n));
  int cur = 0, ph = 0, pw = 0;
  long hw = 0;
  for (int k = hi; k >= lo; k--) {
    int h, w;
    double sigma;
    level_geometry(H, W, k, h, w, sigma);
    hw = (long)h * w;
    Taps taps;
    blur_taps(sigma, taps);
    float* flow = fl[cur];
    if (k == hi) {
      if (d->init_ab) {
        MAUA_HIP_CHECK(hipMemcpyAsync(flow, d->init_ab, (size_t)2 * hw * sizeof(float), hipMemcpyDeviceToDevice, st));
        MAUA_HIP_CHECK(hipMemcpyAsync(flow + 2 * hw, d->init_ba, (size_t)2 * hw * sizeof(float), hipMemcpyDeviceToDevice, st));
      } else {
        MAUA_HIP_CHECK(hipMemsetAsync(flow, 0, (size_t)4 * hw * sizeof(float), st));
      }
    } else {
      hipLaunchKernelGGL(fb_resize_kernel, dim3(blocks(hw * 2), 1, 2), dim3(256), 0, st, (const float*)fl[cur ^ 1], flow, ph, pw, h, w, 2,
                         (float)(1. / FB_PYR_SCALE));
    }
    hipLaunchKernelGGL(fb_blur_kernel<1>, dim3(blocks(n), 1, 2), dim3(256), 0, st, (const float*)gray, tmp, H, W, taps);
    hipLaunchKernelGGL(fb_blur_kernel<0>, dim3(blocks(n), 1, 2), dim3(256), 0, st, (const float*)tmp, blur, H, W, taps);
    hipLaunchKernelGGL(fb_resize_kernel, dim3(blocks(hw), 1, 2), dim3(256), 0, st, (const float*)blur, lvl, H, W, h, w, 1, 1.f);
    hipLaunchKernelGGL(fb_poly_v_kernel, dim3(blocks(hw), 1, 2), dim3(256), 0, st, (const float*)lvl, pt, h, w, fb->poly);
    hipLaunchKernelGGL(fb_poly_h_kernel, dim3(blocks(hw), 1, 2), dim3(256), 0, st, (const float*)pt, R, h, w, fb->poly);
    hipLaunchKernelGGL(fb_matrices_kernel, dim3(blocks(hw), 1, 2), dim3(256), 0, st, (const float*)R, (const float*)flow, M[0], h, w);
    if (k == lo) {
      MAUA_HIP_CHECK(dump(d->blur, blur, 2 * n));
      MAUA_HIP_CHECK(dump(d->level, lvl, 2 * hw));
      MAUA_HIP_CHECK(dump(d->coef, R, 10 * hw));
      MAUA_HIP_CHECK(dump(d->flow_in, flow, 4 * hw));
      MAUA_HIP_CHECK(dump(d->mat, M[0], 10 * hw));
    }
    const dim3 grid((w + FB_TW - 1) / FB_TW, (h + FB_TH - 1) / FB_TH, 2);
    for (int i = 0; i < iters; i++)
      hipLaunchKernelGGL(fb_iterate_kernel, grid, dim3(FB_TW, FB_TH), 0, st, (const float*)M[i & 1], M[(i + 1) & 1], (const float*)R, flow, h, w,
                         (int)(i < iters - 1));
    ph = h; pw = w;
    cur ^= 1;
  }
  const float* last = fl[cur ^ 1];
  MAUA_HIP_CHECK(hipMemcpyAsync(d->flow_ab, last, (size_t)2 * hw * sizeof(float), hipMemcpyDeviceToDevice, st));
  MAUA_HIP_CHECK(hipMemcpyAsync(d->flow_ba, last + 2 * hw, (size_t)2 * hw * sizeof(float), hipMemcpyDeviceToDevice, st));
  MAUA_HIP_CHECK(hipGetLastError());
  return MAUA_OK;
}

// the default descriptor: every level of the size, 15 iterations, zero initial flow, no dumps
int maua_farneback_pair(maua_farneback* fb, maua_ctx* ctx, const float* im_a, const float* im_b, int H, int W, float* flow_ab, float* flow_ba) {
  maua_farneback_desc d = {};
  d.im_a = im_a; d.im_b = im_b; d.H = H; d.W = W; d.flow_ab = flow_ab; d.flow_ba = flow_ba;
  d.level_hi = d.level_lo = -1;
  return maua_farneback_pair_ex(fb, ctx, &d);
}

}  // extern "C"
