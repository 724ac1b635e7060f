// Image operators of the multi-resolution pipeline around guided diffusion (maua/diffusion/image.py:61-74, 132-214): what runs
// between two scales of MultiResolutionDiffusionProcessor.forward, as library calls on planar float32 [B][3][H][W] images.
//
// Replaces (reference):
//   resize       resize_right.resize(img, out_shape=..., interp_method=lanczos3 | cubic) (diffusion/image.py:66-71, :180) - the package is
//                absent from the reference tree (parity unpinned); the published algorithm as csrc/cutouts.hip runs it for cutouts:
//                separable 1-D passes, kernel stretched by 1 / scale when shrinking, weights normalised per output sample, zero padding.
//   destitch /   maua/ops/image.py:15-62 (destitch, smoothstep, blend_weight1d, restitch)
//   restitch
//   histogram    maua/ops/image.py:105-173 (get_histogram, match_histogram mode "avg")
//   sharpen      maua/ops/image.py:70-71 (torchvision adjust_sharpness on (x + 1) / 2)
//   perlin       maua/ops/noise.py:90-132 (interp, perlin, perlin_ms, create_perlin_noise)
//
// MI355X design: every operator is one pass over an image that is read once and written once (HBM bound; a 512² RGB image is 3 MB,
// so these are launch-latency sized beside a sampler step).  All are gathers: each output element is produced by one thread that sums
// its inputs in a fixed order, no float atomics - results are bit-identical from run to run.
//   resize     the tap tables (first source index + weights per output coordinate) come from the host, which evaluates the published
//              float32 arithmetic once per (in, out, kernel) pair.  A workgroup = one (plane, band of output rows): vertical pass
//              from the image (coalesced along x) into an LDS band [rows][W], horizontal pass out of it.  The band's row count shrinks
//              with W so that it stays within 64 KB (a 4096-wide perlin plane: 4 rows).
//   restitch   a thread per output pixel walks the tile grid in the reference's order (rows, then columns) and accumulates
//              tile * (wy * wx) and wy * wx exactly as the reference's in-place adds do, then divides.
//   histogram  moments: a workgroup sums 11 numbers (3 sums, 6 products, min, max) over a fixed slice of pixels in a fixed tree; the
//              slices' partials go to the host, which finishes mean / covariance and the two 3x3 square roots in float64.
//   perlin     pass 1 evaluates the octave sum per pixel with individually rounded float32 operations (contraction off) in the reference's order and
//              quantises to 8 bits (to_pil_image), writing per-workgroup min / max; pass 2 (one workgroup per channel) collapses them to
//              the channel's extremes; pass 3 builds autocontrast's table from those and writes to_tensor's floats.  (Three
//              launches, not one: the table needs the whole image's extremes, and every workgroup re-reducing the per-workgroup
//              table would read 512 KB per workgroup on a 4096² plane.)
#include <cmath>

#include "common.h"
#include "internal.h"

namespace maua {

namespace {

constexpr int IM_BAND = 16;           // most output rows per resize workgroup
constexpr int IM_BAND_FLOATS = 16384;  // LDS band budget (64 KB)
constexpr int IM_MAX_GRID = 64;       // most tile rows / columns of destitch / restitch
constexpr int IM_MAX_OCT = 16;        // most perlin octaves

// ---------------------------------------------------------------------------------------------------------------- resize
struct ImResizeArgs {
  const float* src;
  float* dst;
  const int* left_y;    // [Ho]; nullptr: the rows are kept (H == Ho)
  const float* w_y;     // [Ho][taps_y]
  const int* left_x;    // [Wo]; nullptr: the columns are kept
  const float* w_x;     // [Wo][taps_x]
  int H, W, Ho, Wo, taps_y, taps_x, band;
  int accumulate;       // dst = (dst + resized) + add instead of resized + add
  float add;
};

// grid (bands, planes); LDS [band][W] floats
__global__ __launch_bounds__(256) void image_resize_kernel(ImResizeArgs a) {
  extern __shared__ float band_s[];
  const long plane = blockIdx.y;
  const int y0 = blockIdx.x * a.band;
  const int rows = min(a.band, a.Ho - y0);
  const float* src = a.src + plane * a.H * a.W;
  for (int e = threadIdx.x; e < rows * a.W; e += 256) {
    const int yl = e / a.W, X = e - yl * a.W, y = y0 + yl;
    float acc;
    if (a.left_y) {
      const int l = a.left_y[y];
      const float* wt = a.w_y + (long)y * a.taps_y;
      acc = 0.f;
      for (int i = 0; i < a.taps_y; i++) {
        const int Y = l + i;
        if (Y >= 0 && Y < a.H) acc = fmaf(wt[i], src[(long)Y * a.W + X], acc);
      }
    } else {
      acc = src[(long)y * a.W + X];
    }
    band_s[yl * a.W + X] = acc;
  }
  __syncthreads();
  float* dst = a.dst + plane * a.Ho * a.Wo;
  for (int e = threadIdx.x; e < rows * a.Wo; e += 256) {
    const int yl = e / a.Wo, x = e - yl * a.Wo;
    float acc;
    if (a.left_x) {
      const int l = a.left_x[x];
      const float* wt = a.w_x + (long)x * a.taps_x;
      acc = 0.f;
      for (int j = 0; j < a.taps_x; j++) {
        const int X = l + j;
        if (X >= 0 && X < a.W) acc = fmaf(wt[j], band_s[yl * a.W + X], acc);
      }
    } else {
      acc = band_s[yl * a.W + x];
    }
    float* o = dst + (long)(y0 + yl) * a.Wo + x;
    *o = a.accumulate ? (*o + acc) + a.add : acc + a.add;
  }
}

// ---------------------------------------------------------------------------------------------------------------- tiles
struct TileGrid {
  int n_rows, n_cols;
  int ys[IM_MAX_GRID], xs[IM_MAX_GRID];
};

// out[(r * n_cols + c) * B + b][ch][y][x] = img[b][ch][ys[r] + y][xs[c] + x]; grid (ceil(T * T / 256), 3 * B, tiles)
__global__ __launch_bounds__(256) void destitch_kernel(const float* __restrict__ img, float* __restrict__ out, TileGrid g, int B, int H,
                                                       int W, int T) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= T * T) return;
  const int y = e / T, x = e - y * T;
  const int bc = blockIdx.y, tile = blockIdx.z;
  const int r = tile / g.n_cols, c = tile - r * g.n_cols;
  const int b = bc / 3, ch = bc - b * 3;
  out[(((long)tile * B + b) * 3 + ch) * T * T + e] = img[(((long)b * 3 + ch) * H + g.ys[r] + y) * W + g.xs[c] + x];
}

// out[0][ch][Y][X] = sum_tiles tile * (wy * wx) / sum_tiles (wy * wx), tiles visited in the reference's order; grid (ceil(W / 256), H, 3)
__global__ __launch_bounds__(256) void restitch_kernel(const float* __restrict__ tiles, const float* __restrict__ wy,
                                                       const float* __restrict__ wx, float* __restrict__ out, TileGrid g, int H, int W,
                                                       int T) {
#pragma clang fp contract(off)   // the reference's order: weight, product and both sums each round once
  const int X = blockIdx.x * 256 + threadIdx.x, Y = blockIdx.y, ch = blockIdx.z;
  if (X >= W) return;
  float acc = 0.f, norm = 0.f;
  for (int r = 0; r < g.n_rows; r++) {
    const int y = Y - g.ys[r];
    if (y < 0 || y >= T) continue;
    const float vy = wy[r * T + y];
    for (int c = 0; c < g.n_cols; c++) {
      const int x = X - g.xs[c];
      if (x < 0 || x >= T) continue;
      const float w = vy * wx[c * T + x];
      const float t = tiles[(((long)(r * g.n_cols + c) * 3 + ch) * T + y) * T + x];
      acc = acc + t * w;
      norm = norm + w;
    }
  }
  out[((long)ch * H + Y) * W + X] = acc / norm;
}

// ---------------------------------------------------------------------------------------------------------------- sharpen
// grid (ceil(W / 256), H, 3 * B)
__global__ __launch_bounds__(256) void sharpen_kernel(const float* __restrict__ img, float* __restrict__ out, int H, int W, float strength) {
  const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
  if (x >= W) return;
  const float* p = img + (long)blockIdx.z * H * W;
  auto px = [&](int yy, int xx) { return (p[(long)yy * W + xx] + 1.f) / 2.f; };
  const float v = px(y, x);
  if (H <= 2 || W <= 2) {   // adjust_sharpness returns such an image as it is: no blend, no clamp
    out[(long)blockIdx.z * H * W + (long)y * W + x] = v * 2.f - 1.f;
    return;
  }
  float blur = v;   // border pixels keep their value
  if (y > 0 && y < H - 1 && x > 0 && x < W - 1) {
    const float k1 = 1.f / 13.f, k5 = 5.f / 13.f;
    float acc = 0.f;
    for (int dy = -1; dy <= 1; dy++)
      for (int dx = -1; dx <= 1; dx++) acc = fmaf(dy == 0 && dx == 0 ? k5 : k1, px(y + dy, x + dx), acc);
    blur = acc;
  }
  float r = strength * v + (1.f - strength) * blur;   // _blend: ratio * img + (1 - ratio) * degenerate
  r = fminf(fmaxf(r, 0.f), 1.f);
  out[(long)blockIdx.z * H * W + (long)y * W + x] = r * 2.f - 1.f;
}

// ---------------------------------------------------------------------------------------------------------------- histogram
constexpr int HM_SLICE = 4096;   // pixels per moments workgroup
constexpr int HM_REC = 11;       // sums [3], products 00 01 02 11 12 22, min, max

// partial[frame][slice][11]; value(pixel) = mean over `navg` images (source.mean(0)) + noise_scale * noise; min / max over the raw
// images without noise.  grid (slices, frames): frame f reads images f * navg .. f * navg + navg - 1
__global__ __launch_bounds__(256) void moments_kernel(const float* __restrict__ img, const float* __restrict__ noise, float noise_scale,
                                                      float* __restrict__ partial, int navg, long HW) {
  __shared__ float red[256 * HM_REC];
  const int frame = blockIdx.y;
  const long p0 = (long)blockIdx.x * HM_SLICE;
  float s[HM_REC];
  for (int k = 0; k < 9; k++) s[k] = 0.f;
  s[9] = INFINITY; s[10] = -INFINITY;
  for (int i = threadIdx.x; i < HM_SLICE; i += 256) {
    const long p = p0 + i;
    if (p >= HW) break;
    float v[3];
    for (int c = 0; c < 3; c++) {
      float sum = 0.f;
      for (int n = 0; n < navg; n++) {
        const float x = img[(((long)frame * navg + n) * 3 + c) * HW + p];
        sum = sum + x;
        s[9] = fminf(s[9], x); s[10] = fmaxf(s[10], x);
      }
      v[c] = navg > 1 ? sum / (float)navg : sum;
      if (noise) v[c] = v[c] + noise_scale * noise[((long)frame * 3 + c) * HW + p];
    }
    s[0] += v[0]; s[1] += v[1]; s[2] += v[2];
    s[3] = fmaf(v[0], v[0], s[3]); s[4] = fmaf(v[0], v[1], s[4]); s[5] = fmaf(v[0], v[2], s[5]);
    s[6] = fmaf(v[1], v[1], s[6]); s[7] = fmaf(v[1], v[2], s[7]); s[8] = fmaf(v[2], v[2], s[8]);
  }
  for (int k = 0; k < HM_REC; k++) red[threadIdx.x * HM_REC + k] = s[k];
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {   // fixed tree: the same order on every run
    if ((int)threadIdx.x < o) {
      float* a = red + threadIdx.x * HM_REC;
      const float* b = red + (threadIdx.x + o) * HM_REC;
      for (int k = 0; k < 9; k++) a[k] += b[k];
      a[9] = fminf(a[9], b[9]); a[10] = fmaxf(a[10], b[10]);
    }
    __syncthreads();
  }
  if (threadIdx.x < HM_REC) partial[((long)frame * gridDim.x + blockIdx.x) * HM_REC + threadIdx.x] = red[threadIdx.x];
}

struct MatchArgs {
  float m[9], mu_t[3], mu_s[3];   // out = m (x + noise_scale * noise - mu_t) + mu_s
  float noise_scale, scale, lo, hi;
  int accumulate, clamp;
};

// grid (ceil(HW / 256), 1, 1): one frame [3][HW]
__global__ __launch_bounds__(256) void match_apply_kernel(const float* __restrict__ img, const float* __restrict__ noise,
                                                          float* __restrict__ out, MatchArgs a, long HW) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= HW) return;
  float v[3];
  for (int c = 0; c < 3; c++) {
    v[c] = img[c * HW + p];
    if (noise) v[c] = v[c] + a.noise_scale * noise[c * HW + p];
    v[c] -= a.mu_t[c];
  }
  for (int c = 0; c < 3; c++) {
    float r = fmaf(a.m[3 * c + 2], v[2], fmaf(a.m[3 * c + 1], v[1], a.m[3 * c] * v[0])) + a.mu_s[c];
    r *= a.scale;
    if (a.accumulate) r += out[c * HW + p];
    if (a.clamp) r = fminf(fmaxf(r, a.lo), a.hi);
    out[c * HW + p] = r;
  }
}

// ---------------------------------------------------------------------------------------------------------------- perlin
struct PerlinArgs {
  const float* grads;             // per channel, per octave: gx [(w + 1)][(h + 1)], then gy
  long offs[3 * IM_MAX_OCT];      // offset of (channel, octave)'s gx
  float oct[IM_MAX_OCT];          // octave amplitudes (float32, as the tensor arithmetic rounds them)
  int n_oct, width, height, scale0, channels;   // channels: 1 (grayscale) or 3
  int S_r, S_c;                   // width * scale0, height * scale0
};

// The order of these three functions is the contract with the reference (every operation rounds once, in ops/noise.py's order): plain
// operators with contraction switched off in each body - the pragma is lexical, it does not reach a helper from its caller, and the
// __f*_rn intrinsics do not stop the compiler from fusing a product into the sum that follows.
__device__ __forceinline__ float perlin_interp(float t) {   // noise.py:90-91: 3 t^2 - 2 t^3
#pragma clang fp contract(off)
  const float t2 = t * t, t3 = t2 * t;
  return 3.f * t2 - 2.f * t3;
}

// one octave's value at pixel (R, Cc): noise.py:94-106
__device__ __forceinline__ float perlin_at(const float* gx, const float* gy, int h1, int scale, int R, int Cc) {
#pragma clang fp contract(off)
  const int i = R / scale, a = R - i * scale, j = Cc / scale, b = Cc - j * scale;
  const float xs = (float)a / (float)scale, ys = (float)b / (float)scale;   // exact: scale is a power of two
  const float wx = 1.f - perlin_interp(xs), wy = 1.f - perlin_interp(ys);
  const float x1 = 1.f - xs, y1 = 1.f - ys, wx1 = 1.f - wx, wy1 = 1.f - wy;
  const int i00 = i * h1 + j, i10 = (i + 1) * h1 + j, i01 = i * h1 + j + 1, i11 = (i + 1) * h1 + j + 1;
  float d = 0.f;
  d = d + (wx * wy) * (gx[i00] * xs + gy[i00] * ys);
  d = d + (wx1 * wy) * (-gx[i10] * x1 + gy[i10] * ys);
  d = d + (wx * wy1) * (gx[i01] * xs - gy[i01] * y1);
  d = d + (wx1 * wy1) * (-gx[i11] * x1 - gy[i11] * y1);
  return d;
}

// pass 1: octave sum (noise.py:109-121), clamp(0, 1), mul(255).byte() (to_pil_image); per-workgroup min / max of the bytes
// grid (ceil(S_r * S_c / 256), channels)
__global__ __launch_bounds__(256) void perlin_octaves_kernel(PerlinArgs a, float* __restrict__ raw, uint8_t* __restrict__ q,
                                                             int* __restrict__ minmax) {
#pragma clang fp contract(off)
  __shared__ int lo_s[256], hi_s[256];
  const long n = (long)a.S_r * a.S_c;
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  const int ch = blockIdx.y;
  int lo = 255, hi = 0;
  if (e < n) {
    const int R = (int)(e / a.S_c), Cc = (int)(e - (long)R * a.S_c);
    float v = 0.5f;
    int scale = a.scale0, w = a.width, h = a.height;
    for (int k = 0; k < a.n_oct; k++) {
      const float* gx = a.grads + a.offs[ch * IM_MAX_OCT + k];
      const float* gy = gx + (long)(w + 1) * (h + 1);
      v = v + perlin_at(gx, gy, h + 1, scale, R, Cc) * a.oct[k];
      scale >>= 1; w <<= 1; h <<= 1;
    }
    if (raw) raw[ch * n + e] = v;
    const float c = fminf(fmaxf(v, 0.f), 1.f);
    const int b = (int)(c * 255.f);   // .byte(): truncation
    q[ch * n + e] = (uint8_t)b;
    lo = hi = b;
  }
  lo_s[threadIdx.x] = lo; hi_s[threadIdx.x] = hi;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      lo_s[threadIdx.x] = min(lo_s[threadIdx.x], lo_s[threadIdx.x + o]);
      hi_s[threadIdx.x] = max(hi_s[threadIdx.x], hi_s[threadIdx.x + o]);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    minmax[((long)ch * gridDim.x + blockIdx.x) * 2] = lo_s[0];
    minmax[((long)ch * gridDim.x + blockIdx.x) * 2 + 1] = hi_s[0];
  }
}

// pass 2: the per-workgroup min / max table of a channel -> one (lo, hi) pair; grid (channels), fixed tree
__global__ __launch_bounds__(256) void perlin_extremes_kernel(const int* __restrict__ minmax, int n_parts, int* __restrict__ lohi) {
  __shared__ int lo_s[256], hi_s[256];
  const int ch = blockIdx.x;
  int lo = 255, hi = 0;
  for (int i = threadIdx.x; i < n_parts; i += 256) {
    lo = min(lo, minmax[((long)ch * n_parts + i) * 2]);
    hi = max(hi, minmax[((long)ch * n_parts + i) * 2 + 1]);
  }
  lo_s[threadIdx.x] = lo; hi_s[threadIdx.x] = hi;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      lo_s[threadIdx.x] = min(lo_s[threadIdx.x], lo_s[threadIdx.x + o]);
      hi_s[threadIdx.x] = max(hi_s[threadIdx.x], hi_s[threadIdx.x + o]);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) { lohi[2 * ch] = lo_s[0]; lohi[2 * ch + 1] = hi_s[0]; }
}

// pass 3: ImageOps.autocontrast (cutoff 0: lut[i] = int(i * scale + offset) clipped, scale = 255 / (hi - lo), identity when hi <= lo)
// and to_tensor (byte / 255); a grayscale image is written to all three planes (convert("RGB")).  grid (ceil(n / 256), 3)
__global__ __launch_bounds__(256) void perlin_autocontrast_kernel(const uint8_t* __restrict__ q, const int* __restrict__ minmax,
                                                                  int n_parts, int channels, long n, float* __restrict__ out) {
  __shared__ int lo_s[256], hi_s[256];
  __shared__ float lut[256];
  const int ch = blockIdx.y, sc = channels == 1 ? 0 : ch;
  int lo = 255, hi = 0;
  for (int i = threadIdx.x; i < n_parts; i += 256) {
    lo = min(lo, minmax[((long)sc * n_parts + i) * 2]);
    hi = max(hi, minmax[((long)sc * n_parts + i) * 2 + 1]);
  }
  lo_s[threadIdx.x] = lo; hi_s[threadIdx.x] = hi;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      lo_s[threadIdx.x] = min(lo_s[threadIdx.x], lo_s[threadIdx.x + o]);
      hi_s[threadIdx.x] = max(hi_s[threadIdx.x], hi_s[threadIdx.x + o]);
    }
    __syncthreads();
  }
  lo = lo_s[0]; hi = hi_s[0];
  int m = threadIdx.x;
  if (hi > lo) {
    const double scale = 255.0 / (double)(hi - lo), offset = -(double)lo * scale;
    m = (int)((double)threadIdx.x * scale + offset);   // int(): towards zero
    m = min(max(m, 0), 255);
  }
  lut[threadIdx.x] = (float)m / 255.f;
  __syncthreads();
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e < n) out[ch * n + e] = lut[q[sc * n + e]];
}

int fill_grid(TileGrid& g, const int* ys, int n_rows, const int* xs, int n_cols, int H, int W, int T, const char* who) {
  MAUA_REQUIRE(ys && xs && n_rows > 0 && n_cols > 0 && n_rows <= IM_MAX_GRID && n_cols <= IM_MAX_GRID,
               std::string(who) + ": 1 .. 64 tile rows and columns");
  g.n_rows = n_rows; g.n_cols = n_cols;
  for (int r = 0; r < n_rows; r++) {
    MAUA_REQUIRE(ys[r] >= 0 && ys[r] + T <= H, std::string(who) + ": a tile row leaves the image");
    g.ys[r] = ys[r];
  }
  for (int c = 0; c < n_cols; c++) {
    MAUA_REQUIRE(xs[c] >= 0 && xs[c] + T <= W, std::string(who) + ": a tile column leaves the image");
    g.xs[c] = xs[c];
  }
  return MAUA_OK;
}

}  // namespace

}  // namespace maua

using namespace maua;

extern "C" int maua_image_resize(maua_ctx* ctx, const float* src, int planes, int H, int W, float* dst, int Ho, int Wo, const int* left_y,
                                 const float* w_y, int taps_y, const int* left_x, const float* w_x, int taps_x, int accumulate, float add) {
  MAUA_REQUIRE(ctx, "maua_image_resize: ctx is NULL");
  MAUA_REQUIRE(planes >= 0 && H > 0 && W > 0 && Ho > 0 && Wo > 0, "maua_image_resize: bad shape");
  if (planes == 0) return MAUA_OK;
  MAUA_REQUIRE(src && dst && src != dst, "maua_image_resize: NULL or aliased images");
  MAUA_REQUIRE(left_y ? (w_y && taps_y > 0) : H == Ho, "maua_image_resize: rows need a tap table unless H == Ho");
  MAUA_REQUIRE(left_x ? (w_x && taps_x > 0) : W == Wo, "maua_image_resize: columns need a tap table unless W == Wo");
  MAUA_REQUIRE(W <= IM_BAND_FLOATS && planes <= 65535, "maua_image_resize: at most 16384 columns and 65535 planes");
  ImResizeArgs a{};
  a.src = src; a.dst = dst; a.left_y = left_y; a.w_y = w_y; a.left_x = left_x; a.w_x = w_x;
  a.H = H; a.W = W; a.Ho = Ho; a.Wo = Wo; a.taps_y = taps_y; a.taps_x = taps_x;
  a.band = std::max(1, std::min(IM_BAND, IM_BAND_FLOATS / W));
  a.accumulate = accumulate; a.add = add;
  const size_t smem = (size_t)a.band * W * 4;
  MAUA_HIP_CHECK(hipFuncSetAttribute((const void*)image_resize_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
  hipLaunchKernelGGL(image_resize_kernel, dim3((unsigned)cdiv(Ho, a.band), (unsigned)planes), dim3(256), smem, ctx->stream, a);
  MAUA_HIP_CHECK(hipGetLastError());
  return MAUA_OK;
}

extern "C" int maua_image_destitch(maua_ctx* ctx, const float* img, int B, int H, int W, int tile_size, const int* ys, int n_rows,
                                   const int* xs, int n_cols, float* out) {
  MAUA_REQUIRE(ctx, "maua_image_destitch: ctx is NULL");
  MAUA_REQUIRE(B >= 0 && H > 0 && W > 0 && tile_size > 0 && tile_size <= H && tile_size <= W, "maua_image_destitch: bad shape");
  if (B == 0) return MAUA_OK;
  MAUA_REQUIRE(img && out, "maua_image_destitch: NULL argument");
  MAUA_REQUIRE(3 * B <= 65535, "maua_image_destitch: batch too large");
  TileGrid g{};
  if (int rc = fill_grid(g, ys, n_rows, xs, n_cols, H, W, tile_size, "maua_image_destitch")) return rc;
  hipLaunchKernelGGL(destitch_kernel, dim3((unsigned)cdiv(tile_size * tile_size, 256), (unsigned)(3 * B), (unsigned)(n_rows * n_cols)),
                     dim3(256), 0, ctx->stream, img, out, g, B, H, W, tile_size);
  MAUA_HIP_CHECK(hipGetLastError());
  return MAUA_OK;
}

extern "C" int maua_image_restitch(maua_ctx* ctx, const float* tiles, int tile_size, const int* ys, int n_rows, const int* xs, int n_cols,
                                   const float* wy, const float* wx, float* out, int H, int W) {
  MAUA_REQUIRE(ctx, "maua_image_restitch: ctx is NULL");
  MAUA_REQUIRE(H > 0 && W > 0 && tile_size > 0 && tile_size <= H && tile_size <= W && H <= 65535, "maua_image_restitch: bad shape");
  MAUA_REQUIRE(tiles && wy && wx && out, "maua_image_restitch: NULL argument");
  TileGrid g{};
  if (int rc = fill_grid(g, ys, n_rows, xs, n_cols, H, W, tile_size, "maua_image_restitch")) return rc;
  // every pixel must lie under a tile: consecutive origins at most a tile apart, the first at 0, the last flush with the edge
  MAUA_REQUIRE(g.ys[0] == 0 && g.xs[0] == 0 && g.ys[n_rows - 1] + tile_size == H && g.xs[n_cols - 1] + tile_size == W,
               "maua_image_restitch: the tiles do not reach the image's edges");
  for (int r = 1; r < n_rows; r++) MAUA_REQUIRE(g.ys[r] - g.ys[r - 1] <= tile_size && g.ys[r] >= g.ys[r - 1], "maua_image_restitch: gap between tile rows");
  for (int c = 1; c < n_cols; c++) MAUA_REQUIRE(g.xs[c] - g.xs[c - 1] <= tile_size && g.xs[c] >= g.xs[c - 1], "maua_image_restitch: gap between tile columns");
  hipLaunchKernelGGL(restitch_kernel, dim3((unsigned)cdiv(W, 256), (unsigned)H, 3), dim3(256), 0, ctx->stream, tiles, wy, wx, out, g, H, W,
                     tile_size);
  MAUA_HIP_CHECK(hipGetLastError());
  return MAUA_OK;
}

extern "C" int maua_image_sharpen(maua_ctx* ctx, const float* img, int B, int H, int W, float strength, float* out) {
  MAUA_REQUIRE(ctx, "maua_image_sharpen: ctx is NULL");
  MAUA_REQUIRE(B >= 0 && H > 0 && W > 0 && H <= 65535 && 3 * B <= 65535, "maua_image_sharpen: bad shape");
  if (B == 0) return MAUA_OK;
  MAUA_REQUIRE(img && out && img != out, "maua_image_sharpen: NULL or aliased images");
  hipLaunchKernelGGL(sharpen_kernel, dim3((unsigned)cdiv(W, 256), (unsigned)H, (unsigned)(3 * B)), dim3(256), 0, ctx->stream, img, out, H, W,
                     strength);
  MAUA_HIP_CHECK(hipGetLastError());
  return MAUA_OK;
}

extern "C" int maua_image_moments_slices(long HW) { return (int)((HW + HM_SLICE - 1) / HM_SLICE); }

extern "C" int maua_image_moments(maua_ctx* ctx, const float* img, int frames, int navg, long HW, const float* noise, float noise_scale,
                                  float* partial) {
  MAUA_REQUIRE(ctx, "maua_image_moments: ctx is NULL");
  MAUA_REQUIRE(frames >= 0 && navg > 0 && HW > 0 && frames <= 65535, "maua_image_moments: bad shape");
  if (frames == 0) return MAUA_OK;
  MAUA_REQUIRE(img && partial, "maua_image_moments: NULL argument");
  hipLaunchKernelGGL(moments_kernel, dim3((unsigned)maua_image_moments_slices(HW), (unsigned)frames), dim3(256), 0, ctx->stream, img, noise,
                     noise_scale, partial, navg, HW);
  MAUA_HIP_CHECK(hipGetLastError());
  return MAUA_OK;
}

extern "C" int maua_image_match_apply(maua_ctx* ctx, const float* img, const float* noise, float noise_scale, long HW, const float* m,
                                      const float* mu_t, const float* mu_s, float scale, int accumulate, int clamp, float lo, float hi,
                                      float* out) {
  MAUA_REQUIRE(ctx, "maua_image_match_apply: ctx is NULL");
  MAUA_REQUIRE(img && m && mu_t && mu_s && out && HW > 0, "maua_image_match_apply: bad arguments");
  MatchArgs a{};
  for (int k = 0; k < 9; k++) a.m[k] = m[k];
  for (int k = 0; k < 3; k++) { a.mu_t[k] = mu_t[k]; a.mu_s[k] = mu_s[k]; }
  a.noise_scale = noise_scale; a.scale = scale; a.accumulate = accumulate; a.clamp = clamp; a.lo = lo; a.hi = hi;
  hipLaunchKernelGGL(match_apply_kernel, dim3((unsigned)((HW + 255) / 256)), dim3(256), 0, ctx->stream, img, noise, out, a, HW);
  MAUA_HIP_CHECK(hipGetLastError());
  return MAUA_OK;
}

extern "C" int maua_image_perlin(maua_ctx* ctx, const float* grads, const long* offsets, const float* octaves, int n_octaves, int width,
                                 int height, int grayscale, float* raw, float* out) {
  MAUA_REQUIRE(ctx, "maua_image_perlin: ctx is NULL");
  MAUA_REQUIRE(grads && offsets && octaves && out, "maua_image_perlin: NULL argument");
  MAUA_REQUIRE(n_octaves > 0 && n_octaves <= IM_MAX_OCT && width > 0 && height > 0, "maua_image_perlin: 1 .. 16 octaves, positive grid");
  PerlinArgs a{};
  a.grads = grads; a.n_oct = n_octaves; a.width = width; a.height = height; a.scale0 = 1 << n_octaves; a.channels = grayscale ? 1 : 3;
  const long S_r = (long)width << n_octaves, S_c = (long)height << n_octaves;
  MAUA_REQUIRE(S_r <= 16384 && S_c <= 16384, "maua_image_perlin: image larger than 16384 on a side");
  a.S_r = (int)S_r; a.S_c = (int)S_c;
  for (int c = 0; c < a.channels; c++)
    for (int k = 0; k < n_octaves; k++) a.offs[c * IM_MAX_OCT + k] = offsets[c * n_octaves + k];
  for (int k = 0; k < n_octaves; k++) a.oct[k] = octaves[k];
  const long n = S_r * S_c;
  const int parts = (int)((n + 255) / 256);
  uint8_t* q;
  int *minmax, *lohi;
  if (int rc = carve_scratch(ctx, [&](Scratch& s) {
        q = s.take<uint8_t>((size_t)a.channels * n); minmax = s.take<int>((size_t)a.channels * parts * 2); lohi = s.take<int>(2 * a.channels);
      }))
    return rc;
  hipLaunchKernelGGL(perlin_octaves_kernel, dim3((unsigned)parts, (unsigned)a.channels), dim3(256), 0, ctx->stream, a, raw, q, minmax);
  MAUA_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(perlin_extremes_kernel, dim3((unsigned)a.channels), dim3(256), 0, ctx->stream, minmax, parts, lohi);
  MAUA_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(perlin_autocontrast_kernel, dim3((unsigned)parts, 3), dim3(256), 0, ctx->stream, q, lohi, 1, a.channels, n, out);
  MAUA_HIP_CHECK(hipGetLastError());
  return MAUA_OK;
}
