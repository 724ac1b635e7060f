// Audio-reactivity instruments (include/maua_hip.h: "video features and matrix correlations").
//
// 1. Per-frame visual features (selfsupervised/features/video.py:12-75): the six normalised histograms R, G, B, H, S, V with
//    torch.histc's own range and bin rule, the unbiased variance and the summed absolute frame difference.  Two reads of a frame, the
//    second one out of the caches: a chunk of frames goes through the statistics pass (minimum / maximum of every channel, the sums),
//    then straight through the binning pass.  Counts and the uint8 sums are integers from start to finish (LDS integer atomics on per-wave
//    sub-histograms, integer adds across workgroups): no result depends on the order of arrival, a rerun is bit-identical.  The float
//    arithmetic of HSV and of the bin rule is kept uncontracted and correctly rounded so that it agrees with a float32 host restatement
//    to the bit.
// 2. Matrix correlations (selfsupervised/features/correlation.py:14-56, 72-121, 278-282, 353-382) from second moments over the time
//    axis: no T x T matrix is formed.  Float64 accumulation in a fixed order, no atomics.
#include <cmath>
#include <type_traits>

#include "common.h"

#pragma clang fp contract(off)

namespace maua {
namespace {

constexpr int VF_THREADS = 256;                  // 4 waves
constexpr int VF_PPT = 16;                       // pixels per thread
constexpr int VF_SPAN = VF_THREADS * VF_PPT;     // pixels per workgroup
constexpr int VF_MAX_BINS = 256;
constexpr long VF_MAX_PIXELS = 1L << 24;         // a bin count stays exact in float32
constexpr long VF_CHUNK_BYTES = 64L << 20;       // frames per statistics + binning round: what the second read finds in the Infinity Cache
constexpr int VF_MAX_CHUNK = 1024;

// ---- pixel access: layout 0 uint8 HWC, 1 uint8 CHW, 2 float32 CHW -------------------------------------------------------------------
template <int L> struct Frame;
template <> struct Frame<MAUA_VFEAT_U8_HWC> {
  static constexpr bool kU8 = true;
  static constexpr int kEsize = 1;
  __device__ static __forceinline__ void load(const void* f, long P, long i, int& r, int& g, int& b) {
    const uint8_t* p = (const uint8_t*)f + 3 * i;
    r = p[0]; g = p[1]; b = p[2];
  }
};
template <> struct Frame<MAUA_VFEAT_U8_CHW> {
  static constexpr bool kU8 = true;
  static constexpr int kEsize = 1;
  __device__ static __forceinline__ void load(const void* f, long P, long i, int& r, int& g, int& b) {
    const uint8_t* p = (const uint8_t*)f + i;
    r = p[0]; g = p[P]; b = p[2 * P];
  }
};
template <> struct Frame<MAUA_VFEAT_F32_CHW> {
  static constexpr bool kU8 = false;
  static constexpr int kEsize = 4;
  __device__ static __forceinline__ void load(const void* f, long P, long i, float& r, float& g, float& b) {
    const float* p = (const float*)f + i;
    r = p[0]; g = p[P]; b = p[2 * P];
  }
};

// rgb_to_hsv in its published form (kornia.color.rgb_to_hsv, eps = 1e-8), every step a correctly rounded float32 operation:
// v = max; s = (max - min) / (max + eps); the hue of the FIRST maximal channel (torch.max on the CPU), h = 2 pi ((h_k / deltac / 6) % 1)
// with torch's remainder (the sign of the divisor), not C's fmodf
__device__ __forceinline__ void hsv_of(float r, float g, float b, float& h, float& s, float& v) {
  float mx = r;
  int k = 0;
  if (g > mx) { mx = g; k = 1; }
  if (b > mx) { mx = b; k = 2; }
  const float mn = fminf(fminf(r, g), b);
  const float dc = mx - mn;
  v = mx;
  s = dc / (mx + 1e-8f);
  const float d = dc == 0.f ? 1.f : dc;
  const float rc = mx - r, gc = mx - g, bc = mx - b;
  const float hk = k == 0 ? (bc - gc) : k == 1 ? (rc - bc) + 2.f * d : (gc - rc) + 4.f * d;
  const float q = (hk / d) / 6.f;
  float m = q - truncf(q);       // fmodf(q, 1), exact
  if (m < 0.f) m += 1.f;         // torch.remainder: a non-zero result takes the divisor's sign
  h = 6.2831855f * m;            // float32(2 pi)
}

// torch.histc's bin of x in [mn, mx]: int((x - mn) * bins / (mx - mn)) in float32 in that order, the right edge folded into the last bin;
// -1 for a value outside the range (NaN), which torch ignores too
__device__ __forceinline__ int bin_of(float x, float mn, float mx, int bins) {
  int pos = (int)((x - mn) * (float)bins / (mx - mn));
  if (pos == bins) pos = bins - 1;
  return (pos >= 0 && pos < bins) ? pos : -1;
}

__device__ __forceinline__ float wave_min(float v) {
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}
template <typename T> __device__ __forceinline__ T wave_sum(T v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// ---- pass 1: per (frame, workgroup) the minimum and maximum of R, G, B, H, S, V and the three sums.  uint8 frames: sum k, sum k^2,
// sum |k - k_prev| as 64-bit integers; float32 frames: sum x, sum x^2, sum |x - x_prev| (the difference in float32, as torch.diff
// forms it) accumulated in float64.  part_mm [frame][nblk][12] (6 minima, 6 maxima), part_sum [frame][nblk][3] (8-byte words).
template <int L>
__global__ __launch_bounds__(VF_THREADS) void vf_stats_kernel(const void* frames, const void* carry, int b0, long P, int nblk, float* part_mm,
                                                              unsigned long long* part_sum) {
  using F = Frame<L>;
  using Acc = typename std::conditional<F::kU8, unsigned long long, double>::type;
  __shared__ float lut[256];
  __shared__ float red_mm[4][12];
  __shared__ Acc red_sum[4][3];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = b0 + blockIdx.y;
  const char* cur = (const char*)frames + (size_t)b * P * 3 * F::kEsize;
  const char* prev = b > 0 ? cur - (size_t)P * 3 * F::kEsize : (const char*)carry;
  if (F::kU8) {
    lut[tid] = (float)tid / 255.f;   // the value a byte stands for: a true division, as decord's .div(255) gives
    __syncthreads();
  }
  float mn[6], mx[6];
  for (int c = 0; c < 6; c++) { mn[c] = INFINITY; mx[c] = -INFINITY; }
  Acc s1 = 0, s2 = 0, sd = 0;
  const long base = (long)blockIdx.x * VF_SPAN;
  for (int j = 0; j < VF_PPT; j++) {
    const long i = base + (long)j * VF_THREADS + tid;
    if (i >= P) break;
    float x[6];
    if constexpr (F::kU8) {
      int r, g, bl;
      F::load(cur, P, i, r, g, bl);
      x[0] = lut[r]; x[1] = lut[g]; x[2] = lut[bl];
      s1 += (unsigned)(r + g + bl);
      s2 += (unsigned)(r * r + g * g + bl * bl);
      if (prev) {
        int pr, pg, pb;
        F::load(prev, P, i, pr, pg, pb);
        sd += (unsigned)(abs(r - pr) + abs(g - pg) + abs(bl - pb));
      }
    } else {
      F::load(cur, P, i, x[0], x[1], x[2]);
      for (int c = 0; c < 3; c++) {
        s1 += (double)x[c];
        s2 += (double)x[c] * (double)x[c];
      }
      if (prev) {
        float p[3];
        F::load(prev, P, i, p[0], p[1], p[2]);
        for (int c = 0; c < 3; c++) sd += (double)fabsf(x[c] - p[c]);
      }
    }
    hsv_of(x[0], x[1], x[2], x[3], x[4], x[5]);
    for (int c = 0; c < 6; c++) { mn[c] = fminf(mn[c], x[c]); mx[c] = fmaxf(mx[c], x[c]); }
  }
  for (int c = 0; c < 6; c++) {
    const float a = wave_min(mn[c]), z = wave_max(mx[c]);
    if (lane == 0) { red_mm[wave][c] = a; red_mm[wave][6 + c] = z; }
  }
  s1 = wave_sum(s1); s2 = wave_sum(s2); sd = wave_sum(sd);
  if (lane == 0) { red_sum[wave][0] = s1; red_sum[wave][1] = s2; red_sum[wave][2] = sd; }
  __syncthreads();
  const size_t slot = (size_t)b * nblk + blockIdx.x;
  if (tid < 12) {
    float v = red_mm[0][tid];
    for (int w = 1; w < 4; w++) v = tid < 6 ? fminf(v, red_mm[w][tid]) : fmaxf(v, red_mm[w][tid]);
    part_mm[slot * 12 + tid] = v;
  } else if (tid < 15) {
    const int q = tid - 12;
    Acc v = red_sum[0][q];
    for (int w = 1; w < 4; w++) v += red_sum[w][q];   // fixed order
    unsigned long long bits;
    if constexpr (F::kU8) bits = v; else bits = (unsigned long long)__double_as_longlong(v);
    part_sum[slot * 3 + q] = bits;
  }
}

// ---- between the passes, one workgroup per frame: the frame's ranges (min == max widened to [v - 1, v + 1], as torch.histc does),
// variance and difference, and the frame's counts cleared for the binning pass.  mm [frame][12]: (mn, mx) per channel.
__global__ __launch_bounds__(256) void vf_frame_kernel(int b0, long P, int nblk, int u8, int bins, int first_has_prev, const float* part_mm,
                                                       const unsigned long long* part_sum, float* mm, int* counts, float* variance, float* diff) {
  __shared__ float s_mm[12][256];
  __shared__ unsigned long long s_i[3][256];
  __shared__ double s_f[3][256];
  const int tid = threadIdx.x;
  const int b = b0 + blockIdx.x;
  for (int i = tid; i < 6 * bins; i += 256) counts[(size_t)b * 6 * bins + i] = 0;
  const float* pm = part_mm + (size_t)b * nblk * 12;
  const unsigned long long* ps = part_sum + (size_t)b * nblk * 3;
  // thread t takes the workgroups t, t + 256, ...; then a tree over the 256 threads: a fixed order (the float64 sums of float32 frames need one)
  float lo[6], hi[6];
  unsigned long long si[3] = {0, 0, 0};
  double sf[3] = {0, 0, 0};
  for (int c = 0; c < 6; c++) { lo[c] = INFINITY; hi[c] = -INFINITY; }
  for (int k = tid; k < nblk; k += 256) {
    for (int c = 0; c < 6; c++) {
      lo[c] = fminf(lo[c], pm[(size_t)k * 12 + c]);
      hi[c] = fmaxf(hi[c], pm[(size_t)k * 12 + 6 + c]);
    }
    for (int q = 0; q < 3; q++) {
      if (u8) si[q] += ps[(size_t)k * 3 + q];
      else sf[q] += __longlong_as_double((long long)ps[(size_t)k * 3 + q]);
    }
  }
  for (int c = 0; c < 6; c++) { s_mm[c][tid] = lo[c]; s_mm[6 + c][tid] = hi[c]; }
  for (int q = 0; q < 3; q++) { s_i[q][tid] = si[q]; s_f[q][tid] = sf[q]; }
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) {
      for (int c = 0; c < 6; c++) {
        s_mm[c][tid] = fminf(s_mm[c][tid], s_mm[c][tid + s]);
        s_mm[6 + c][tid] = fmaxf(s_mm[6 + c][tid], s_mm[6 + c][tid + s]);
      }
      for (int q = 0; q < 3; q++) { s_i[q][tid] += s_i[q][tid + s]; s_f[q][tid] += s_f[q][tid + s]; }
    }
    __syncthreads();
  }
  if (tid < 6) {
    float mn = s_mm[tid][0], mx = s_mm[6 + tid][0];
    if (mn == mx) { mn = mn - 1.f; mx = mx + 1.f; }
    mm[(size_t)b * 12 + 2 * tid] = mn;
    mm[(size_t)b * 12 + 2 * tid + 1] = mx;
  } else if (tid == 64) {
    const double N = 3.0 * (double)P;
    const bool has_prev = b > 0 || first_has_prev;
    if (u8) {
      const unsigned long long S1 = s_i[0][0], S2 = s_i[1][0], D = s_i[2][0];
      // N S2 - S1^2 >= 0 as an exact 128-bit integer: no cancellation reaches the floating-point result
      const unsigned long long n = 3ull * (unsigned long long)P;
      const unsigned long long alo = n * S2, ahi = __umul64hi(n, S2), blo = S1 * S1, bhi = __umul64hi(S1, S1);
      const unsigned long long lo128 = alo - blo, hi128 = ahi - bhi - (alo < blo ? 1ull : 0ull);
      const double num = (double)hi128 * 18446744073709551616.0 + (double)lo128;
      variance[b] = (float)(num / (N * (N - 1.0) * 65025.0));
      diff[b] = has_prev ? (float)((double)D / 255.0) : 0.f;
    } else {
      const double S1 = s_f[0][0], S2 = s_f[1][0], D = s_f[2][0];
      variance[b] = (float)((S2 - S1 * S1 / N) / (N - 1.0));
      diff[b] = has_prev ? (float)D : 0.f;
    }
  }
}

// ---- pass 2: the six bins of every pixel, counted on per-wave LDS sub-histograms and merged into the frame's counts with integer adds.
// uint8 frames: R, G, B and V live on the 256-point lattice, so their bin is a table look-up (the table built with the same bin_of).
template <int L>
__global__ __launch_bounds__(VF_THREADS) void vf_bin_kernel(const void* frames, int b0, long P, int bins, const float* mm, int* counts) {
  using F = Frame<L>;
  __shared__ float lut[256];
  __shared__ short binlut[4][256];
  __shared__ int sub[4][6 * VF_MAX_BINS];
  const int tid = threadIdx.x, wave = tid >> 6;
  const int b = b0 + blockIdx.y;
  const char* cur = (const char*)frames + (size_t)b * P * 3 * F::kEsize;
  const float* m = mm + (size_t)b * 12;
  for (int i = tid; i < 4 * 6 * VF_MAX_BINS; i += VF_THREADS) (&sub[0][0])[i] = 0;
  if (F::kU8) {
    const float x = (float)tid / 255.f;
    lut[tid] = x;
    binlut[0][tid] = (short)bin_of(x, m[0], m[1], bins);
    binlut[1][tid] = (short)bin_of(x, m[2], m[3], bins);
    binlut[2][tid] = (short)bin_of(x, m[4], m[5], bins);
    binlut[3][tid] = (short)bin_of(x, m[10], m[11], bins);
  }
  __syncthreads();
  int* mine = sub[wave];
  const long base = (long)blockIdx.x * VF_SPAN;
  for (int j = 0; j < VF_PPT; j++) {
    const long i = base + (long)j * VF_THREADS + tid;
    if (i >= P) break;
    float x[6];
    int pos[6];
    if constexpr (F::kU8) {
      int r, g, bl;
      F::load(cur, P, i, r, g, bl);
      x[0] = lut[r]; x[1] = lut[g]; x[2] = lut[bl];
      pos[0] = binlut[0][r]; pos[1] = binlut[1][g]; pos[2] = binlut[2][bl];
      pos[5] = binlut[3][max(max(r, g), bl)];
      hsv_of(x[0], x[1], x[2], x[3], x[4], x[5]);
    } else {
      F::load(cur, P, i, x[0], x[1], x[2]);
      hsv_of(x[0], x[1], x[2], x[3], x[4], x[5]);
      pos[0] = bin_of(x[0], m[0], m[1], bins);
      pos[1] = bin_of(x[1], m[2], m[3], bins);
      pos[2] = bin_of(x[2], m[4], m[5], bins);
      pos[5] = bin_of(x[5], m[10], m[11], bins);
    }
    pos[3] = bin_of(x[3], m[6], m[7], bins);
    pos[4] = bin_of(x[4], m[8], m[9], bins);
    // a flat image region sends a whole wave to the same counter: one add of the lane count then, instead of 64 serialised ones
    const unsigned long long act = __ballot(1);
    const int nact = __popcll(act);
    const bool leader = (tid & 63) == __ffsll((long long)act) - 1;
    for (int c = 0; c < 6; c++) {
      const int p = pos[c], f = __builtin_amdgcn_readfirstlane(p);
      if (__all(p == f)) {
        if (leader && f >= 0) atomicAdd(&mine[c * bins + f], nact);
      } else if (p >= 0) {
        atomicAdd(&mine[c * bins + p], 1);
      }
    }
  }
  __syncthreads();
  int* out = counts + (size_t)b * 6 * bins;
  for (int i = tid; i < 6 * bins; i += VF_THREADS) {
    const int v = sub[0][i] + sub[1][i] + sub[2][i] + sub[3][i];
    if (v) atomicAdd(&out[i], v);
  }
}

// ---- hist = counts / max(counts) per (frame, channel) (video.py:14: hist / hist.max(dim=1)); counts_out optional
__global__ __launch_bounds__(256) void vf_hist_kernel(const int* counts, int bins, float* hist, int* counts_out) {
  __shared__ int red[256];
  const int tid = threadIdx.x;
  const size_t row = ((size_t)blockIdx.y * 6 + blockIdx.x) * bins;
  const int c = tid < bins ? counts[row + tid] : 0;
  red[tid] = c;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) red[tid] = max(red[tid], red[tid + s]);
    __syncthreads();
  }
  if (tid < bins) {
    hist[row + tid] = (float)c / (float)red[0];
    if (counts_out) counts_out[row + tid] = c;
  }
}


// every refusal of a push, in front of the first launch
int vfeat_check(int H, int W, int bins, int max_batch, const void* frames, int layout, int B, const float* hist, const float* variance,
                const float* diff) {
  MAUA_REQUIRE(H >= 1 && W >= 1 && (long)H * W <= VF_MAX_PIXELS, "maua_vfeat: a frame must have between 1 and 2^24 pixels");
  MAUA_REQUIRE(bins >= 1 && bins <= VF_MAX_BINS, "maua_vfeat: bins must be 1 .. 256");
  MAUA_REQUIRE(max_batch >= 1 && max_batch <= 65535, "maua_vfeat: max_batch must be 1 .. 65535");
  MAUA_REQUIRE(layout == MAUA_VFEAT_U8_HWC || layout == MAUA_VFEAT_U8_CHW || layout == MAUA_VFEAT_F32_CHW,
               "maua_vfeat: layout must be 0 (uint8 HWC), 1 (uint8 CHW) or 2 (float32 CHW)");
  MAUA_REQUIRE(B >= 0 && B <= max_batch, "maua_vfeat: the batch exceeds max_batch");
  if (B == 0) return MAUA_OK;
  MAUA_REQUIRE(frames && hist && variance && diff, "maua_vfeat: NULL argument");
  MAUA_REQUIRE(layout != MAUA_VFEAT_F32_CHW || ((size_t)frames & 3) == 0, "maua_vfeat: float32 frames must be 4-byte aligned");
  return MAUA_OK;
}

}  // namespace
}  // namespace maua

using namespace maua;

struct maua_vfeat {
  int device = 0, H = 0, W = 0, bins = 0, max_batch = 0, nblk = 0;
  DevBuf ws;          // one set, carved at creation into the pieces below
  float* part_mm = nullptr;
  unsigned long long* part_sum = nullptr;
  float* mm = nullptr;
  int* counts = nullptr;
  void* carry = nullptr;
  int carry_layout = -1;   // -1: no carried frame
};

namespace {

template <int L>
void vfeat_round(maua_vfeat* h, hipStream_t st, const void* frames, int b0, int nb, int first_has_prev, float* variance, float* diff) {
  const long P = (long)h->H * h->W;
  hipLaunchKernelGGL(vf_stats_kernel<L>, dim3(h->nblk, nb), dim3(VF_THREADS), 0, st, frames, first_has_prev ? (const void*)h->carry : nullptr, b0, P,
                     h->nblk, h->part_mm, h->part_sum);
  hipLaunchKernelGGL(vf_frame_kernel, dim3(nb), dim3(256), 0, st, b0, P, h->nblk, Frame<L>::kU8 ? 1 : 0, h->bins, first_has_prev, h->part_mm,
                     h->part_sum, h->mm, h->counts, variance, diff);
  hipLaunchKernelGGL(vf_bin_kernel<L>, dim3(h->nblk, nb), dim3(VF_THREADS), 0, st, frames, b0, P, h->bins, h->mm, h->counts);
}

}  // namespace

extern "C" {

int maua_vfeat_create(maua_ctx* ctx, int H, int W, int bins, int max_batch, maua_vfeat** out) {
  MAUA_REQUIRE(ctx && out, "maua_vfeat_create: NULL argument");
  if (vfeat_check(H, W, bins, max_batch, nullptr, MAUA_VFEAT_U8_HWC, 0, nullptr, nullptr, nullptr) != MAUA_OK) return MAUA_ERR;
  const long P = (long)H * W;
  const int nblk = (int)((P + VF_SPAN - 1) / VF_SPAN);
  MAUA_HIP_CHECK(hipSetDevice(ctx->device));
  auto* h = new maua_vfeat();
  h->device = ctx->device; h->H = H; h->W = W; h->bins = bins; h->max_batch = max_batch; h->nblk = nblk;
  auto layout = [&](Scratch& s) {
    h->part_mm = s.take<float>((size_t)max_batch * nblk * 12);
    h->part_sum = s.take<unsigned long long>((size_t)max_batch * nblk * 3);
    h->mm = s.take<float>((size_t)max_batch * 12);
    h->counts = s.take<int>((size_t)max_batch * 6 * bins);
    h->carry = s.take<char>((size_t)P * 3 * sizeof(float));
  };
  if (carve_into(h->ws, layout)) {
    delete h;
    return fail_in("maua_vfeat_create");
  }
  *out = h;
  return MAUA_OK;
}

int maua_vfeat_destroy(maua_vfeat* h) {
  if (!h) return MAUA_OK;
  delete h;
  return MAUA_OK;
}

int maua_vfeat_reset(maua_vfeat* h) {
  MAUA_REQUIRE(h, "maua_vfeat_reset: NULL handle");
  h->carry_layout = -1;
  return MAUA_OK;
}

int maua_vfeat_check(const maua_vfeat* h, int H, int W, int bins, int max_batch, const void* frames, int layout, int B, const float* hist,
                     const int* counts, const float* variance, const float* diff) {
  (void)counts;
  if (h) {
    MAUA_REQUIRE(H == h->H && W == h->W, "maua_vfeat: the frame size differs from the size the handle was created for");
    bins = h->bins;
    max_batch = h->max_batch;
  }
  if (vfeat_check(H, W, bins, max_batch, frames, layout, B, hist, variance, diff) != MAUA_OK) return MAUA_ERR;
  MAUA_REQUIRE(!h || h->carry_layout < 0 || h->carry_layout == layout, "maua_vfeat: the layout changed inside a stream (maua_vfeat_reset first)");
  return MAUA_OK;
}

int maua_vfeat_push(maua_vfeat* h, maua_ctx* ctx, const void* frames, int layout, int B, int H, int W, float* hist, int* counts, float* variance,
                    float* diff) {
  MAUA_REQUIRE(h && ctx, "maua_vfeat: NULL handle or ctx");
  MAUA_REQUIRE(ctx->device == h->device, "maua_vfeat: the handle belongs to another device");
  if (maua_vfeat_check(h, H, W, 0, 0, frames, layout, B, hist, counts, variance, diff) != MAUA_OK) return MAUA_ERR;
  if (B == 0) return MAUA_OK;
  hipStream_t st = ctx->stream;
  const long P = (long)H * W;
  const size_t frame_bytes = (size_t)P * 3 * (layout == MAUA_VFEAT_F32_CHW ? 4 : 1);
  long chunk = VF_CHUNK_BYTES / (long)frame_bytes;
  chunk = chunk < 1 ? 1 : chunk > VF_MAX_CHUNK ? VF_MAX_CHUNK : chunk;
  for (int b0 = 0; b0 < B; b0 += (int)chunk) {
    const int nb = B - b0 < chunk ? B - b0 : (int)chunk;
    const int first_has_prev = h->carry_layout >= 0 ? 1 : 0;
    if (layout == MAUA_VFEAT_U8_HWC) vfeat_round<MAUA_VFEAT_U8_HWC>(h, st, frames, b0, nb, first_has_prev, variance, diff);
    else if (layout == MAUA_VFEAT_U8_CHW) vfeat_round<MAUA_VFEAT_U8_CHW>(h, st, frames, b0, nb, first_has_prev, variance, diff);
    else vfeat_round<MAUA_VFEAT_F32_CHW>(h, st, frames, b0, nb, first_has_prev, variance, diff);
  }
  hipLaunchKernelGGL(vf_hist_kernel, dim3(6, B), dim3(256), 0, st, (const int*)h->counts, h->bins, hist, counts);
  MAUA_HIP_CHECK(hipGetLastError());
  MAUA_HIP_CHECK(hipMemcpyAsync(h->carry, (const char*)frames + (size_t)(B - 1) * frame_bytes, frame_bytes, hipMemcpyDeviceToDevice, st));
  h->carry_layout = layout;
  return MAUA_OK;
}

}  // extern "C"

// =====================================================================================================================================
// Matrix correlations from second moments.  Z = [X | Y] ([T][Fx] and [T][Fy] float32), F = Fx + Fy.
//   mean [F]            column means
//   rn [T][2]           squared norms of the centred rows of X and of Y
//   G [F][F]            Zc^T Zc of the centred columns
//   Gn [F][F], cs [F]   the same of the centred, row-normalised matrices (autocorrcorr only), and their column sums
// Everything float64, summed over T in slabs of CR_SLAB rows in a fixed order.
namespace maua {
namespace {

constexpr int CR_SLAB = 64;
constexpr int CR_TILE = 16;
constexpr int CR_MAX_F = 1024;

struct CorrWs { double *mean, *rn, *G, *Gn, *cs, *col; };

__device__ __forceinline__ double block_sum(double v, double* red) {   // 256 threads, fixed order
  const int tid = threadIdx.x;
  red[tid] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

__device__ __forceinline__ double z_at(const float* x, const float* y, int Fx, int Fy, long t, int j) {
  return j < Fx ? (double)x[t * Fx + j] : (double)y[t * Fy + (j - Fx)];
}

// column j: mode 0 the mean; mode 1 the sum of the centred, row-normalised column
__global__ __launch_bounds__(256) void corr_col_kernel(const float* x, const float* y, int T, int Fx, int Fy, int mode, const double* mean,
                                                       const double* rn, double* out) {
  __shared__ double red[256];
  const int j = blockIdx.x, side = j < Fx ? 0 : 1;
  double s = 0;
  for (long t = threadIdx.x; t < T; t += 256) {
    const double v = z_at(x, y, Fx, Fy, t, j);
    s += mode ? (v - mean[j]) / sqrt(rn[t * 2 + side]) : v;
  }
  s = block_sum(s, red);
  if (threadIdx.x == 0) out[j] = mode ? s : s / T;
}

// row t: the squared norms of its centred X and Y parts
__global__ __launch_bounds__(256) void corr_row_kernel(const float* x, const float* y, int T, int Fx, int Fy, const double* mean, double* rn) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= T) return;
  double a = 0, b = 0;
  for (int j = 0; j < Fx; j++) { const double v = (double)x[t * Fx + j] - mean[j]; a += v * v; }
  for (int j = 0; j < Fy; j++) { const double v = (double)y[t * Fy + j] - mean[Fx + j]; b += v * v; }
  rn[t * 2] = a;
  rn[t * 2 + 1] = b;
}

// one 16 x 16 tile of Zc^T Zc (normalised: of the row-normalised matrices) per workgroup, the rows staged through LDS a slab at a time
__global__ __launch_bounds__(256) void corr_gram_kernel(const float* x, const float* y, int T, int Fx, int Fy, int normalised, const double* mean,
                                                        const double* rn, double* G) {
  __shared__ double a[CR_SLAB][CR_TILE + 1], b[CR_SLAB][CR_TILE + 1];
  const int F = Fx + Fy, tid = threadIdx.x, ti = tid / CR_TILE, tj = tid % CR_TILE;
  const int i0 = blockIdx.y * CR_TILE, j0 = blockIdx.x * CR_TILE;
  double acc = 0;
  for (int t0 = 0; t0 < T; t0 += CR_SLAB) {
    for (int e = tid; e < CR_SLAB * CR_TILE; e += 256) {
      const int r = e / CR_TILE, c = e % CR_TILE;
      const long t = t0 + r;
      double va = 0, vb = 0;
      if (t < T) {
        if (i0 + c < F) {
          va = z_at(x, y, Fx, Fy, t, i0 + c) - mean[i0 + c];
          if (normalised) va = va / sqrt(rn[t * 2 + (i0 + c < Fx ? 0 : 1)]);
        }
        if (j0 + c < F) {
          vb = z_at(x, y, Fx, Fy, t, j0 + c) - mean[j0 + c];
          if (normalised) vb = vb / sqrt(rn[t * 2 + (j0 + c < Fx ? 0 : 1)]);
        }
      }
      a[r][c] = va;
      b[r][c] = vb;
    }
    __syncthreads();
    for (int r = 0; r < CR_SLAB; r++) acc += a[r][ti] * b[r][tj];
    __syncthreads();
  }
  if (i0 + ti < F && j0 + tj < F) G[(size_t)(i0 + ti) * F + j0 + tj] = acc;
}

// sum over a block of a Gram matrix of g^2 (sq) or of its diagonal (the blocks XX, XY, YY start at (r0, c0))
__device__ double gram_sq(const double* G, int F, int r0, int nr, int c0, int nc, double* red) {
  double s = 0;
  for (long e = threadIdx.x; e < (long)nr * nc; e += 256) {
    const double g = G[(size_t)(r0 + e / nc) * F + c0 + e % nc];
    s += g * g;
  }
  return block_sum(s, red);
}

// the finishing step: one workgroup, the metric out of the moments
__global__ __launch_bounds__(256) void corr_finish_kernel(int T, int Fx, int Fy, int metric, CorrWs w, float* out) {
  __shared__ double red[256];
  __shared__ int any_nan;
  const int tid = threadIdx.x, F = Fx + Fy;
  const double* G = w.G;
  double val = 0;
  if (metric == MAUA_CORR_PEARSON || metric == MAUA_CORR_CONCORDANCE) {
    // per column pair (correlation.py:14-56), then torch.median's lower median (:353-362) by rank counting
    if (tid == 0) any_nan = 0;
    __syncthreads();
    for (int j = tid; j < Fx; j += 256) {
      const double sx = sqrt(G[(size_t)j * F + j] / (T - 1)), sy = sqrt(G[(size_t)(Fx + j) * F + Fx + j] / (T - 1));
      const double r = G[(size_t)j * F + Fx + j] / (T - 1) / (sx * sy);
      double v = r;
      if (metric == MAUA_CORR_CONCORDANCE) {
        const double dm = w.mean[j] - w.mean[Fx + j], bct = (double)(T - 1) / T;
        v = 2 * r * sx * sy / (sx * sx + sy * sy + dm * dm / bct);
      }
      w.col[j] = v;
      if (v != v) any_nan = 1;
    }
    __syncthreads();
    for (int j = tid; j < Fx; j += 256) {
      const double v = w.col[j];
      int rank = 0;
      for (int k = 0; k < Fx; k++) rank += (w.col[k] < v || (w.col[k] == v && k < j)) ? 1 : 0;
      if (rank == (Fx - 1) / 2 || any_nan) out[0] = any_nan ? NAN : (float)v;
    }
    return;
  }
  if (metric == MAUA_CORR_R1) {   // trace(X Y^T) / sqrt(trace(X X^T) trace(Y Y^T)) (:278-282)
    double a = 0, b = 0, c = 0;
    for (int j = tid; j < Fx; j += 256) {
      a += G[(size_t)j * F + Fx + j];
      b += G[(size_t)j * F + j];
      c += G[(size_t)(Fx + j) * F + Fx + j];
    }
    a = block_sum(a, red); b = block_sum(b, red); c = block_sum(c, red);
    val = a / sqrt(b * c);
  } else if (metric == MAUA_CORR_RV || metric == MAUA_CORR_RV2) {
    // trace(XX^T YY^T) = |X^T Y|_F^2; modified (:108-109): minus the diagonals' products, sum_t |x_t|^2 |y_t|^2
    double xy = gram_sq(G, F, 0, Fx, Fx, Fy, red), xx = gram_sq(G, F, 0, Fx, 0, Fx, red), yy = gram_sq(G, F, Fx, Fy, Fx, Fy, red);
    if (metric == MAUA_CORR_RV2) {
      double dxy = 0, dxx = 0, dyy = 0;
      for (long t = tid; t < T; t += 256) {
        const double a = w.rn[t * 2], b = w.rn[t * 2 + 1];
        dxy += a * b; dxx += a * a; dyy += b * b;
      }
      xy -= block_sum(dxy, red); xx -= block_sum(dxx, red); yy -= block_sum(dyy, red);
    }
    val = xy / sqrt(xx * yy);
  } else {   // MAUA_CORR_AUTOCORRCORR (:72-86): Pearson over the pairs i < j of the two cosine matrices, from five sums
    const double* Gn = w.Gn;
    double ca = 0, cb = 0;
    for (int j = tid; j < F; j += 256) {
      const double c = w.cs[j] * w.cs[j];
      if (j < Fx) ca += c; else cb += c;
    }
    ca = block_sum(ca, red); cb = block_sum(cb, red);
    const double aa = gram_sq(Gn, F, 0, Fx, 0, Fx, red), bb = gram_sq(Gn, F, Fx, Fy, Fx, Fy, red), ab = gram_sq(Gn, F, 0, Fx, Fx, Fy, red);
    const double n = 0.5 * (double)T * (T - 1);
    const double Sa = 0.5 * (ca - T), Sb = 0.5 * (cb - T), Saa = 0.5 * (aa - T), Sbb = 0.5 * (bb - T), Sab = 0.5 * (ab - T);
    val = (Sab - Sa * Sb / n) / sqrt((Saa - Sa * Sa / n) * (Sbb - Sb * Sb / n));
  }
  if (tid == 0) out[0] = (float)val;
}

CorrWs corr_ws(Scratch& s, long T, int F) {
  return CorrWs{s.take<double>(F), s.take<double>(2 * (size_t)T), s.take<double>((size_t)F * F), s.take<double>((size_t)F * F),
                s.take<double>(F), s.take<double>(F)};
}

int corr_check(const void* x, const void* y, int T, int Fx, int Fy, int metric, const void* ws, size_t ws_bytes, const void* out) {
  MAUA_REQUIRE(metric >= MAUA_CORR_PEARSON && metric <= MAUA_CORR_R1, "maua_correlation: unknown metric id");
  MAUA_REQUIRE(Fx >= 1 && Fy >= 1 && Fx + Fy <= CR_MAX_F, "maua_correlation: Fx and Fy must be at least 1 and Fx + Fy at most 1024");
  MAUA_REQUIRE(T >= 2 && T <= (1 << 24), "maua_correlation: T must be 2 .. 2^24");
  MAUA_REQUIRE(metric != MAUA_CORR_AUTOCORRCORR || T >= 3, "maua_correlation: autocorrcorr needs T >= 3 (at least two pairs i < j)");
  MAUA_REQUIRE((metric != MAUA_CORR_PEARSON && metric != MAUA_CORR_CONCORDANCE && metric != MAUA_CORR_R1) || Fx == Fy,
               "maua_correlation: pearson, concordance and r1 need Fx == Fy");
  MAUA_REQUIRE(x && y && ws && out, "maua_correlation: NULL argument");
  MAUA_REQUIRE(((size_t)ws & 255) == 0 && ws_bytes >= scratch_bytes(corr_ws, T, Fx + Fy),
               "maua_correlation: the workspace must be 256-byte aligned and hold maua_correlation_workspace() bytes");
  return MAUA_OK;
}

}  // namespace
}  // namespace maua

extern "C" {

long maua_correlation_workspace(int T, int Fx, int Fy) {
  if (T < 1 || Fx < 1 || Fy < 1 || Fx + Fy > CR_MAX_F) return 0;
  return (long)scratch_bytes(corr_ws, T, Fx + Fy);
}

int maua_correlation_check(const float* x, const float* y, int T, int Fx, int Fy, int metric, const void* ws, long ws_bytes, const float* out) {
  return corr_check(x, y, T, Fx, Fy, metric, ws, ws_bytes < 0 ? 0 : (size_t)ws_bytes, out);
}

int maua_correlation(maua_ctx* ctx, const float* x, const float* y, int T, int Fx, int Fy, int metric, void* ws, long ws_bytes, float* out) {
  MAUA_REQUIRE(ctx, "maua_correlation: ctx is NULL");
  if (corr_check(x, y, T, Fx, Fy, metric, ws, ws_bytes < 0 ? 0 : (size_t)ws_bytes, out) != MAUA_OK) return MAUA_ERR;
  hipStream_t st = ctx->stream;
  const int F = Fx + Fy;
  Scratch place(ws);
  const CorrWs w = corr_ws(place, T, F);
  const dim3 tiles(cdiv(F, CR_TILE), cdiv(F, CR_TILE));
  hipLaunchKernelGGL(corr_col_kernel, dim3(F), dim3(256), 0, st, x, y, T, Fx, Fy, 0, (const double*)nullptr, (const double*)nullptr, w.mean);
  hipLaunchKernelGGL(corr_row_kernel, dim3(cdiv(T, 256)), dim3(256), 0, st, x, y, T, Fx, Fy, (const double*)w.mean, w.rn);
  if (metric == MAUA_CORR_AUTOCORRCORR) {
    hipLaunchKernelGGL(corr_col_kernel, dim3(F), dim3(256), 0, st, x, y, T, Fx, Fy, 1, (const double*)w.mean, (const double*)w.rn, w.cs);
    hipLaunchKernelGGL(corr_gram_kernel, tiles, dim3(256), 0, st, x, y, T, Fx, Fy, 1, (const double*)w.mean, (const double*)w.rn, w.Gn);
  } else {
    hipLaunchKernelGGL(corr_gram_kernel, tiles, dim3(256), 0, st, x, y, T, Fx, Fy, 0, (const double*)w.mean, (const double*)w.rn, w.G);
  }
  hipLaunchKernelGGL(corr_finish_kernel, dim3(1), dim3(256), 0, st, T, Fx, Fy, metric, w, out);
  MAUA_HIP_CHECK(hipGetLastError());
  return MAUA_OK;
}

}  // extern "C"
