// The fused GroupNorm pass of the NHWC networks: GroupNorm32 (+ scale-shift) (+ SiLU) (+ the ResBlock's up / down resampling) in one
// pass that writes the next convolution's input, its statistics passes, and the one launcher everything comes through
// (maua::launch_group_norm: the diffusion UNet, CLIP's and the perceptors' callers, groupnorm_api.hip).  Its input gradient is
// groupnorm_vjp.hip.
//
// Replaces (reference): `GroupNorm32(32, C)` / `normalization(C)` of guided_diffusion's ResBlock and AttentionBlock (nn.py), with the
// `h * (1 + scale) + shift` of use_scale_shift_norm, the SiLU and the Upsample / Downsample of resblock_updown that follow it, as
// built by maua/diffusion/processors/guided.py:164-209.
#include <algorithm>

#include "common.h"
#include "internal.h"

using namespace maua;

namespace {

// ------------------------------------------------------------------------------------------------------ GroupNorm
// Statistics in float64 (sum and sum of squares of exactly representable f32 products): no cancellation whatever the
// mean / spread ratio; fixed summation order (bit-reproducible).  Pass 1: per (sample, pixel chunk, row slot) per-channel
// partial sums; pass 2: per (sample, group) mean and 1 / sqrt(var + eps).
template <typename T>
__global__ void gn_partial_kernel(const T* __restrict__ x0, int C0, const T* __restrict__ x1, int C1, long HW, int ppc,
                                  double* __restrict__ part) {
  constexpr int EPC = 16 / (int)sizeof(T);
  const int C = C0 + C1, PPP = C / EPC;
  const int pc = threadIdx.x % PPP, ry = threadIdx.x / PPP, RY = blockDim.x / PPP;
  const int chunk = blockIdx.x, b = blockIdx.y;
  if (ry >= RY) return;
  const int c = pc * EPC;
  const T* src;
  long stride;
  if (c < C0) { src = x0 + (long)b * HW * C0 + c; stride = C0; }
  else { src = x1 + (long)b * HW * C1 + (c - C0); stride = C1; }
  const long p0 = (long)chunk * ppc, p1 = p0 + ppc < HW ? p0 + ppc : HW;
  double s[EPC], ss[EPC];
#pragma unroll
  for (int e = 0; e < EPC; e++) s[e] = ss[e] = 0.0;
  for (long p = p0 + ry; p < p1; p += RY) {
    const u32x4 v = *reinterpret_cast<const u32x4*>(src + p * stride);
#pragma unroll
    for (int e = 0; e < EPC; e++) {
      float f;
      if constexpr (sizeof(T) == 2) f = bf2f((bf16_t)((v[e >> 1] >> ((e & 1) * 16)) & 0xffffu));
      else f = __uint_as_float(v[e]);
      const double d = (double)f;
      s[e] += d;
      ss[e] += d * d;
    }
  }
  double* dst = part + ((((long)b * gridDim.x + chunk) * RY + ry) * C + c) * 2;
#pragma unroll
  for (int e = 0; e < EPC; e++) { dst[2 * e] = s[e]; dst[2 * e + 1] = ss[e]; }
}

__global__ __launch_bounds__(256) void gn_finalize_kernel(const double* __restrict__ part, int rows, int C, long HW, float eps,
                                                          float* __restrict__ stats) {
  __shared__ double red[2][256];
  const int g = blockIdx.x, b = blockIdx.y;
  const int cpg = C / 32;
  const long n = (long)rows * cpg;
  double s = 0.0, ss = 0.0;
  for (long i = threadIdx.x; i < n; i += 256) {
    const long row = i / cpg;
    const int c = g * cpg + (int)(i - row * cpg);
    const double* p = part + (((long)b * rows + row) * C + c) * 2;
    s += p[0];
    ss += p[1];
  }
  red[0][threadIdx.x] = s;
  red[1][threadIdx.x] = ss;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      red[0][threadIdx.x] += red[0][threadIdx.x + o];
      red[1][threadIdx.x] += red[1][threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double cnt = (double)HW * cpg;
    const double mean = red[0][0] / cnt;
    double var = red[1][0] / cnt - mean * mean;
    if (var < 0.0) var = 0.0;
    stats[((long)b * 32 + g) * 2] = (float)mean;
    stats[((long)b * 32 + g) * 2 + 1] = (float)(1.0 / sqrt(var + (double)eps));
  }
}

// y = [silu]( gn(x) [* (1 + scale) + shift] ), optionally resampled (mode 1: 2x2 average of the activated values - the
// ResBlock's Downsample sits BEHIND norm + SiLU; mode 2: nearest x2), written dense NHWC as the next convolution's input.
// xr (optional, modes 1 / 2): the same resampling of the raw input (the block's x_upd, its residual branch).
template <typename T>
__global__ __launch_bounds__(256) void gn_apply_kernel(const T* __restrict__ x0, int C0, const T* __restrict__ x1, int C1,
                                                       const float* __restrict__ stats, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, const float* __restrict__ ss, long ss_ld,
                                                       int silu, int mode, T* __restrict__ y, T* __restrict__ xr, int B, int H,
                                                       int W) {
  constexpr int EPC = 16 / (int)sizeof(T);
  const int C = C0 + C1, PPP = C / EPC, cpg = C / 32;
  const int Ho = mode == 1 ? H / 2 : (mode == 2 ? H * 2 : H), Wo = mode == 1 ? W / 2 : (mode == 2 ? W * 2 : W);
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)B * Ho * Wo * PPP) return;
  const int pc = (int)(idx % PPP);
  long p = idx / PPP;
  const int ox = (int)(p % Wo); p /= Wo;
  const int oy = (int)(p % Ho);
  const int b = (int)(p / Ho);
  const int c = pc * EPC;
  const T* src;
  long stride;
  if (c < C0) { src = x0 + (long)b * H * W * C0 + c; stride = C0; }
  else { src = x1 + (long)b * H * W * C1 + (c - C0); stride = C1; }
  float ca[EPC], cb[EPC], sc[EPC], sh[EPC];
#pragma unroll
  for (int e = 0; e < EPC; e++) {
    const int g = (c + e) / cpg;
    const float mean = stats[((long)b * 32 + g) * 2], rstd = stats[((long)b * 32 + g) * 2 + 1];
    ca[e] = rstd * gamma[c + e];
    cb[e] = beta[c + e] - mean * ca[e];
    sc[e] = ss ? 1.f + ss[(long)b * ss_ld + c + e] : 1.f;
    sh[e] = ss ? ss[(long)b * ss_ld + C + c + e] : 0.f;
  }
  float acc[EPC], raw[EPC];
#pragma unroll
  for (int e = 0; e < EPC; e++) acc[e] = raw[e] = 0.f;
  const int taps = mode == 1 ? 4 : 1;
  for (int t = 0; t < taps; t++) {
    int iy, ix;
    if (mode == 1) { iy = 2 * oy + (t >> 1); ix = 2 * ox + (t & 1); }
    else if (mode == 2) { iy = oy >> 1; ix = ox >> 1; }
    else { iy = oy; ix = ox; }
    const u32x4 v = *reinterpret_cast<const u32x4*>(src + ((long)iy * W + ix) * stride);
#pragma unroll
    for (int e = 0; e < EPC; e++) {
      float f;
      if constexpr (sizeof(T) == 2) f = bf2f((bf16_t)((v[e >> 1] >> ((e & 1) * 16)) & 0xffffu));
      else f = __uint_as_float(v[e]);
      raw[e] += f;
      float u = fmaf(f, ca[e], cb[e]);
      if (ss) u = fmaf(u, sc[e], sh[e]);
      if (silu) u = u / (1.f + expf(-u));
      acc[e] += u;
    }
  }
  const float norm = mode == 1 ? 0.25f : 1.f;
  u32x4 o, ro;
  if constexpr (sizeof(T) == 2) {
#pragma unroll
    for (int k = 0; k < 4; k++) {
      o[k] = pack2bf(acc[2 * k] * norm, acc[2 * k + 1] * norm);
      ro[k] = pack2bf(raw[2 * k] * norm, raw[2 * k + 1] * norm);
    }
  } else {
#pragma unroll
    for (int k = 0; k < 4; k++) { o[k] = __float_as_uint(acc[k] * norm); ro[k] = __float_as_uint(raw[k] * norm); }
  }
  const long opix = ((long)b * Ho + oy) * Wo + ox;
  *reinterpret_cast<u32x4*>(y + opix * C + c) = o;
  if (xr) *reinterpret_cast<u32x4*>(xr + opix * C + c) = ro;
}

// ---- fast path (C / 32 channels per group a multiple of the 16-byte piece: every real layer of the network; the
// per-channel kernels above serve narrow test networks).  Same arithmetic, organised for the memory system:
//   * partial sums per GROUP, reduced inside the workgroup (LDS, fixed order) -> one row of 32 (sum, sumsq) pairs per
//     pixel chunk; a finalize launch of B x 32 threads adds the <= 128 chunk rows;
//   * the apply pass indexes (sample, row) by blockIdx.y and (pixel, piece) by 32-bit arithmetic, loads its piece's
//     coefficients as float4s, and in bf16 mode uses the hardware exp / reciprocal for SiLU (exact in f32 mode).
// (Folding the finalize into this kernel - the last workgroup of a sample, found by an atomic ticket, adds the chunk rows - was
//  built and measured in round 3: 26.7 -> 35.3 ms per UNet step at B = 8.  A device-scope release fence per workgroup writes
//  the XCD's L2 back (8 XCDs, one L2 each): far dearer than the ~5 us launch it saves.  The finalize stays its own launch.)
template <typename T>
__global__ void gn_partial_group_kernel(const T* __restrict__ x0, int C0, const T* __restrict__ x1, int C1, long HW, int ppc,
                                        double* __restrict__ part) {
  constexpr int EPC = 16 / (int)sizeof(T);
  __shared__ double red[2][1024];
  const int C = C0 + C1, PPP = C / EPC;
  const int pc = threadIdx.x % PPP, ry = threadIdx.x / PPP, RY = blockDim.x / PPP;
  const int chunk = blockIdx.x, b = blockIdx.y;
  const int c = pc * EPC;
  const T* src;
  long stride;
  if (c < C0) { src = x0 + (long)b * HW * C0 + c; stride = C0; }
  else { src = x1 + (long)b * HW * C1 + (c - C0); stride = C1; }
  const long p0 = (long)chunk * ppc, p1 = p0 + ppc < HW ? p0 + ppc : HW;
  double s = 0.0, ss = 0.0;
  for (long p = p0 + ry; p < p1; p += RY) {
    const u32x4 v = *reinterpret_cast<const u32x4*>(src + p * stride);
    float fs = 0.f, fq = 0.f;   // 8 (4) values: exact enough in f32 before they join the f64 sums
#pragma unroll
    for (int e = 0; e < EPC; e++) {
      float f;
      if constexpr (sizeof(T) == 2) f = bf2f((bf16_t)((v[e >> 1] >> ((e & 1) * 16)) & 0xffffu));
      else f = __uint_as_float(v[e]);
      if constexpr (sizeof(T) == 2) { fs += f; fq = fmaf(f, f, fq); }
      else { s += (double)f; ss += (double)f * (double)f; }
    }
    if constexpr (sizeof(T) == 2) { s += (double)fs; ss += (double)fq; }
  }
  red[0][threadIdx.x] = s;
  red[1][threadIdx.x] = ss;
  __syncthreads();
  if (threadIdx.x < 32) {
    const int g = threadIdx.x, ppg = PPP / 32;
    double ts = 0.0, tq = 0.0;
    for (int r = 0; r < RY; r++)
      for (int j = 0; j < ppg; j++) {
        ts += red[0][r * PPP + g * ppg + j];
        tq += red[1][r * PPP + g * ppg + j];
      }
    double* dst = part + (((long)b * gridDim.x + chunk) * 32 + g) * 2;
    dst[0] = ts;
    dst[1] = tq;
  }
}

__global__ __launch_bounds__(256) void gn_finalize_group_kernel(const double* __restrict__ part, int nchunk, double cnt,
                                                                float eps, float* __restrict__ stats) {
  // 32 groups x 8 lanes: lane j adds chunks j, j + 8, ... (independent loads in flight), then a fixed-order LDS tree
  __shared__ double red[2][256];
  const int g = threadIdx.x & 31, j = threadIdx.x >> 5, b = blockIdx.x;
  double s = 0.0, ss = 0.0;
  for (int k = j; k < nchunk; k += 8) {
    const double* p = part + (((long)b * nchunk + k) * 32 + g) * 2;
    s += p[0];
    ss += p[1];
  }
  red[0][threadIdx.x] = s;
  red[1][threadIdx.x] = ss;
  __syncthreads();
  if (j == 0) {
#pragma unroll
    for (int q = 1; q < 8; q++) { s += red[0][q * 32 + g]; ss += red[1][q * 32 + g]; }
    const double mean = s / cnt;
    double var = ss / cnt - mean * mean;
    if (var < 0.0) var = 0.0;
    stats[((long)b * 32 + g) * 2] = (float)mean;
    stats[((long)b * 32 + g) * 2 + 1] = (float)(1.0 / sqrt(var + (double)eps));
  }
}

// Statistics from the piece sums a producing convolution left behind (ConvArgs.psum: per 8 x 32-pixel tile and 8-channel
// piece, sums and sums of squares of the stored values) - the tensor itself is not read again.  Two sources like everywhere
// (the decoder's virtual concatenation); 32 groups x 8 lanes, rows j, j + 8, ... per lane, fixed-order LDS tree.
__global__ __launch_bounds__(256) void gn_finalize_psum_kernel(const float* __restrict__ ps0, int rows0, int C0,
                                                               const float* __restrict__ ps1, int rows1, int C1, double cnt,
                                                               float eps, float* __restrict__ stats) {
  __shared__ double red[2][256];
  const int g = threadIdx.x & 31, j = threadIdx.x >> 5, b = blockIdx.x;
  const int np0 = C0 >> 3, np1 = C1 >> 3, ppg = (np0 + np1) >> 5;
  double s = 0.0, ss = 0.0;
  for (int pi = 0; pi < ppg; pi++) {
    const int piece = g * ppg + pi;
    const bool first = piece < np0;
    const float* src = first ? ps0 : ps1;
    const int rows = first ? rows0 : rows1, np = first ? np0 : np1, pc = first ? piece : piece - np0;
    for (int r = j; r < rows; r += 8) {
      const float4* p = reinterpret_cast<const float4*>(src + (((long)b * rows + r) * np + pc) * 16);
      const float4 a0 = p[0], a1 = p[1], q0 = p[2], q1 = p[3];
      s += (double)a0.x + (double)a0.y + (double)a0.z + (double)a0.w + (double)a1.x + (double)a1.y + (double)a1.z + (double)a1.w;
      ss += (double)q0.x + (double)q0.y + (double)q0.z + (double)q0.w + (double)q1.x + (double)q1.y + (double)q1.z + (double)q1.w;
    }
  }
  red[0][threadIdx.x] = s;
  red[1][threadIdx.x] = ss;
  __syncthreads();
  if (j == 0) {
#pragma unroll
    for (int q = 1; q < 8; q++) { s += red[0][q * 32 + g]; ss += red[1][q * 32 + g]; }
    const double mean = s / cnt;
    double var = ss / cnt - mean * mean;
    if (var < 0.0) var = 0.0;
    stats[((long)b * 32 + g) * 2] = (float)mean;
    stats[((long)b * 32 + g) * 2 + 1] = (float)(1.0 / sqrt(var + (double)eps));
  }
}

// A thread owns one 16-byte channel piece and walks GN_PX output pixels of its row with it (round 5: one pixel per thread spent
// 136 bytes of parameter loads - gamma, beta, scale, shift, statistics - on 16 bytes of data and ran at 1.7 TB/s).
constexpr int GN_PX = 8;
template <typename T>
__global__ __launch_bounds__(256) void gn_apply_group_kernel(const T* __restrict__ x0, int C0, const T* __restrict__ x1, int C1,
                                                             const float* __restrict__ stats, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, const float* __restrict__ ss,
                                                             long ss_ld, int silu, int mode, T* __restrict__ y,
                                                             T* __restrict__ xr, int H, int W, int Ho, int Wo) {
  constexpr int EPC = 16 / (int)sizeof(T);
  const unsigned C = C0 + C1, PPP = C / EPC, cpg = C / 32;
  const unsigned li = blockIdx.x * 256u + threadIdx.x;
  const unsigned nxg = ((unsigned)Wo + GN_PX - 1) / GN_PX;
  if (li >= nxg * PPP) return;
  const unsigned oxg = li / PPP, pc = li - oxg * PPP;
  const unsigned b = blockIdx.y / (unsigned)Ho, oy = blockIdx.y - b * (unsigned)Ho;
  const unsigned c = pc * EPC;
  const T* src;
  unsigned stride;
  if (c < (unsigned)C0) { src = x0 + (long)b * H * W * C0 + c; stride = C0; }
  else { src = x1 + (long)b * H * W * C1 + (c - C0); stride = C1; }
  const unsigned g = c / cpg;
  const float2 mr = *reinterpret_cast<const float2*>(stats + ((long)b * 32 + g) * 2);
  float ca[EPC], cb[EPC], sc[EPC], sh[EPC];
#pragma unroll
  for (int q4 = 0; q4 < EPC / 4; q4++) {
    const float4 gm = *reinterpret_cast<const float4*>(gamma + c + 4 * q4);
    const float4 bt = *reinterpret_cast<const float4*>(beta + c + 4 * q4);
    const float gv[4] = {gm.x, gm.y, gm.z, gm.w}, bv[4] = {bt.x, bt.y, bt.z, bt.w};
    float sv[4] = {1.f, 1.f, 1.f, 1.f}, hv[4] = {0.f, 0.f, 0.f, 0.f};
    if (ss) {
      const float4 s4 = *reinterpret_cast<const float4*>(ss + (long)b * ss_ld + c + 4 * q4);
      const float4 h4 = *reinterpret_cast<const float4*>(ss + (long)b * ss_ld + C + c + 4 * q4);
      sv[0] = 1.f + s4.x; sv[1] = 1.f + s4.y; sv[2] = 1.f + s4.z; sv[3] = 1.f + s4.w;
      hv[0] = h4.x; hv[1] = h4.y; hv[2] = h4.z; hv[3] = h4.w;
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int e = 4 * q4 + k;
      ca[e] = mr.y * gv[k];
      cb[e] = bv[k] - mr.x * ca[e];
      sc[e] = sv[k];
      sh[e] = hv[k];
    }
  }
  const int taps = mode == 1 ? 4 : 1;
  const float norm = mode == 1 ? 0.25f : 1.f;
  // the pixel group's loads are requested together (mode 0 / 2: one per pixel; the 4-tap average pool walks pixel by pixel)
  u32x4 vin[GN_PX];
  if (taps == 1) {
#pragma unroll
    for (int k = 0; k < GN_PX; k++) {
      const unsigned ox = min(oxg * GN_PX + k, (unsigned)Wo - 1);
      const unsigned iy = mode == 2 ? oy >> 1 : oy, ix = mode == 2 ? ox >> 1 : ox;
      vin[k] = *reinterpret_cast<const u32x4*>(src + (long)(iy * (unsigned)W + ix) * stride);
    }
  }
#pragma unroll
  for (int k = 0; k < GN_PX; k++) {
    const unsigned ox = oxg * GN_PX + k;
    if (ox >= (unsigned)Wo) break;
    float acc[EPC], raw[EPC];
#pragma unroll
    for (int e = 0; e < EPC; e++) acc[e] = raw[e] = 0.f;
    for (int t = 0; t < taps; t++) {
      u32x4 v;
      if (taps == 1) v = vin[k];
      else v = *reinterpret_cast<const u32x4*>(src + (long)((2 * oy + (t >> 1)) * (unsigned)W + 2 * ox + (t & 1)) * stride);
#pragma unroll
      for (int e = 0; e < EPC; e++) {
        float f;
        if constexpr (sizeof(T) == 2) f = bf2f((bf16_t)((v[e >> 1] >> ((e & 1) * 16)) & 0xffffu));
        else f = __uint_as_float(v[e]);
        raw[e] += f;
        float u = fmaf(f, ca[e], cb[e]);
        if (ss) u = fmaf(u, sc[e], sh[e]);
        if (silu) {
          if constexpr (sizeof(T) == 2) u = __fdividef(u, 1.f + __expf(-u));
          else u = u / (1.f + expf(-u));
        }
        acc[e] += u;
      }
    }
    u32x4 o, ro;
    if constexpr (sizeof(T) == 2) {
#pragma unroll
      for (int q = 0; q < 4; q++) {
        o[q] = pack2bf(acc[2 * q] * norm, acc[2 * q + 1] * norm);
        ro[q] = pack2bf(raw[2 * q] * norm, raw[2 * q + 1] * norm);
      }
    } else {
#pragma unroll
      for (int q = 0; q < 4; q++) { o[q] = __float_as_uint(acc[q] * norm); ro[q] = __float_as_uint(raw[q] * norm); }
    }
    const long opix = ((long)b * Ho + oy) * Wo + ox;
    *reinterpret_cast<u32x4*>(y + opix * C + c) = o;
    if (xr) *reinterpret_cast<u32x4*>(xr + opix * C + c) = ro;
  }
}

// workspace (bytes) of one GroupNorm over [B][HW][C]: partial sums + the [B][32][2] statistics
struct GnPlan { int fast, RY, ppc; long nchunk; size_t part_bytes; };
static GnPlan gn_plan(int B, int C, long HW, int esize) {
  GnPlan p;
  const int EPC = 16 / esize, PPP = C / EPC, cpg = C / 32;
  p.fast = cpg % EPC == 0 && PPP <= 1024;
  p.RY = std::max(1, 512 / PPP);
  long nchunk = HW / ((long)p.RY * 4);
  nchunk = std::max(1L, std::min(128L, nchunk));
  p.ppc = (int)((HW + nchunk - 1) / nchunk);
  p.nchunk = (HW + p.ppc - 1) / p.ppc;
  p.part_bytes = p.fast ? (size_t)B * p.nchunk * 32 * 16 : (size_t)B * p.nchunk * p.RY * C * 16;
  return p;
}
static void gn_out_size(const GnArgs& a, int* Ho, int* Wo) {
  *Ho = a.mode == 1 ? a.H / 2 : (a.mode == 2 ? a.H * 2 : a.H);
  *Wo = a.mode == 1 ? a.W / 2 : (a.mode == 2 ? a.W * 2 : a.W);
}

// the launches of maua::launch_group_norm (which has checked `a`) as maua::group_norm_plan describes them
template <typename T>
static int gn_launch(hipStream_t st, const GnArgs& a, const GnPlanInfo& pl, double* part, float* stats) {
  constexpr int EPC = 16 / (int)sizeof(T);
  const T *x0 = (const T*)a.x0, *x1 = (const T*)a.x1;
  T *y = (T*)a.y, *xr = (T*)a.xr;
  const int C0 = a.C0, C1 = a.C1, C = C0 + C1, PPP = C / EPC, B = a.B, H = a.H, W = a.W;
  const long HW = (long)H * W;
  int Ho, Wo;
  gn_out_size(a, &Ho, &Wo);
  if (pl.route == 0) {
    if (pl.stats_source == 1) {
      // every source's producer left its piece sums: no statistics pass over the tensor
      hipLaunchKernelGGL(gn_finalize_psum_kernel, dim3(B), dim3(256), 0, st, a.ps0, a.rows0, C0, a.ps1, a.rows1, C1,
                         (double)HW * (C / 32), 1e-5f, stats);
    } else {
      hipLaunchKernelGGL(gn_partial_group_kernel<T>, dim3((unsigned)pl.nchunk, B), dim3(PPP * pl.RY), 0, st, x0, C0, x1, C1, HW,
                         pl.ppc, part);
      hipLaunchKernelGGL(gn_finalize_group_kernel, dim3(B), dim3(256), 0, st, part, pl.nchunk, (double)HW * (C / 32), 1e-5f,
                         stats);
    }
    hipLaunchKernelGGL(gn_apply_group_kernel<T>, dim3((unsigned)(((long)((Wo + GN_PX - 1) / GN_PX) * PPP + 255) / 256), (unsigned)(B * Ho)),
                       dim3(256), 0, st, x0, C0, x1, C1, stats, a.gamma, a.beta, a.ss, a.ss_ld, a.silu, a.mode, y, xr, H, W, Ho, Wo);
  } else {
    hipLaunchKernelGGL(gn_partial_kernel<T>, dim3((unsigned)pl.nchunk, B), dim3(PPP * pl.RY), 0, st, x0, C0, x1, C1, HW, pl.ppc,
                       part);
    hipLaunchKernelGGL(gn_finalize_kernel, dim3(32, B), dim3(256), 0, st, part, pl.nchunk * pl.RY, C, HW, 1e-5f, stats);
    const long total = (long)B * Ho * Wo * PPP;
    hipLaunchKernelGGL(gn_apply_kernel<T>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, x0, C0, x1, C1, stats, a.gamma,
                       a.beta, a.ss, a.ss_ld, a.silu, a.mode, y, xr, B, H, W);
  }
  MAUA_HIP_CHECK(hipGetLastError());
  return MAUA_OK;
}
static size_t gn_part_bytes(int B, int C, long HW, int esize) {
  // (the per-channel layout is the larger one and also serves the fall-back of a fast-path shape with too many rows)
  const GnPlan p = gn_plan(B, C, HW, esize);
  return std::max(p.part_bytes, (size_t)B * p.nchunk * p.RY * C * 16);
}

}  // namespace

// ---- the one GroupNorm launcher: the network (Runner::gn), maua_group_norm_nhwc and maua_group_norm_ex all come through here
static inline bool gn_aligned16(const void* p) { return ((size_t)p & 15) == 0; }

int maua::group_norm_check(int dtype, const GnArgs& a) {
  MAUA_REQUIRE(dtype == MAUA_BF16 || dtype == MAUA_F32, "group_norm: unsupported dtype");
  const int EPC = elems_per_piece(dtype);
  MAUA_REQUIRE(a.x0 && a.gamma && a.beta && a.y, "group_norm: NULL argument");
  MAUA_REQUIRE(a.B >= 0 && a.H > 0 && a.W > 0 && a.C0 > 0 && a.C1 >= 0, "group_norm: bad shape");
  const long C = (long)a.C0 + a.C1;
  MAUA_REQUIRE(C % 32 == 0 && C / EPC <= 1024 && a.C0 % EPC == 0, "group_norm: C % 32 == 0, at most 1024 16-byte pieces per pixel");
  MAUA_REQUIRE(a.C1 == 0 || a.x1, "group_norm: x1 is NULL with C1 > 0");
  MAUA_REQUIRE(a.mode >= 0 && a.mode <= 2 && (a.mode != 1 || (a.H >= 2 && a.W >= 2)), "group_norm: bad resample mode");
  MAUA_REQUIRE(!a.ss || a.ss_ld == 0 || a.ss_ld >= 2 * C, "group_norm: ss_ld is 0 (one row for all samples) or at least 2 C");
  MAUA_REQUIRE(gn_aligned16(a.x0) && gn_aligned16(a.x1) && gn_aligned16(a.y) && gn_aligned16(a.xr) && gn_aligned16(a.gamma) &&
                   gn_aligned16(a.beta) && gn_aligned16(a.ss) && gn_aligned16(a.ps0) && gn_aligned16(a.ps1) && a.ss_ld % 4 == 0,
               "group_norm: pointers and ss_ld must be whole 16-byte pieces");
  int Ho, Wo;
  gn_out_size(a, &Ho, &Wo);
  // (blockIdx.y carries the sample in the statistics kernels; the apply kernels index pixels of a sample in 32 bits)
  MAUA_REQUIRE(a.B <= 65535 && (long)Ho * Wo <= 0x7fffffffL && (long)a.H * a.W <= 0x7fffffffL &&
                   ((long)a.B * Ho * Wo * (C / EPC) + 255) / 256 <= 0x7fffffffL,
               "group_norm: grid too large");
  MAUA_REQUIRE(!a.ps1 || a.C1 > 0, "group_norm: ps1 without a second source");
  MAUA_REQUIRE((!a.ps0 && !a.ps1) || dtype == MAUA_BF16, "group_norm: piece sums are bf16 only");
  const bool tiles = a.H % 8 == 0 && a.W % 32 == 0;
  const int rows = (a.H / 8) * (a.W / 32);
  MAUA_REQUIRE((!a.ps0 || (tiles && a.C0 % 128 == 0 && a.rows0 == rows)) && (!a.ps1 || (tiles && a.C1 % 128 == 0 && a.rows1 == rows)),
               "group_norm: piece sums need H % 8 == 0, W % 32 == 0, C % 128 == 0 of their source and rows == (H / 8) * (W / 32)");
  return MAUA_OK;
}

GnPlanInfo maua::group_norm_plan(int dtype, const GnArgs& a) {
  const int esize = elem_bytes(dtype), C = a.C0 + a.C1;
  const GnPlan p = gn_plan(a.B, C, (long)a.H * a.W, esize);
  int Ho, Wo;
  gn_out_size(a, &Ho, &Wo);
  GnPlanInfo pl;
  // (the group kernels carry (sample, output row) in blockIdx.y; a shape with more rows runs the per-channel kernels on the same chunks)
  pl.route = p.fast && (long)a.B * Ho <= 65535 && a.force_route != 1 ? 0 : 1;
  pl.RY = p.RY;
  pl.ppc = p.ppc;
  pl.nchunk = (int)p.nchunk;
  pl.stats_source = pl.route == 0 && a.ps0 && (a.C1 == 0 || a.ps1) && dtype == MAUA_BF16 ? 1 : 0;
  return pl;
}

size_t maua::group_norm_workspace(int B, int C, long HW, int esize) { return gn_part_bytes(B, C, HW, esize); }

int maua::launch_group_norm(hipStream_t stream, int dtype, const GnArgs& a, double* part, float* stats) {
  if (int rc = group_norm_check(dtype, a)) return rc;
  MAUA_REQUIRE(part && stats, "group_norm: NULL workspace");
  if (a.B == 0) return MAUA_OK;
  const GnPlanInfo pl = group_norm_plan(dtype, a);
  return dispatch_dtype<bf16_t, float>(dtype, "group_norm", [&](auto t) { return gn_launch<decltype(t)>(stream, a, pl, part, stats); });
}

// the statistics passes alone (per-channel kernels: any C % 32 == 0)
int maua::launch_group_norm_stats(hipStream_t st, int dtype, const void* x, int C, int B, int H, int W, double* part, float* stats) {
  const int esize = elem_bytes(dtype), PPP = C / (16 / esize);
  const long HW = (long)H * W;
  MAUA_REQUIRE(C % 32 == 0 && PPP <= 1024, "group_norm: C % 32 == 0, at most 1024 16-byte pieces per pixel");
  const GnPlan p = gn_plan(B, C, HW, esize);
  const dim3 grid((unsigned)p.nchunk, B), block(PPP * p.RY);
  if (int rc = dispatch_dtype<bf16_t, float>(dtype, "group_norm", [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(gn_partial_kernel<T>, grid, block, 0, st, (const T*)x, C, (const T*)nullptr, 0, HW, p.ppc, part);
      }))
    return rc;
  hipLaunchKernelGGL(gn_finalize_kernel, dim3(32, B), dim3(256), 0, st, part, (int)(p.nchunk * p.RY), C, HW, 1e-5f, stats);
  MAUA_HIP_CHECK(hipGetLastError());
  return MAUA_OK;
}
