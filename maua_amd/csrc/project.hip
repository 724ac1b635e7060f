// The arithmetic of latent-space projection around the generator and its gradient (maua_amd/projection.py): the noise regulariser
// and its gradient, one Adam update, the noise maps' renormalisation, and the w -> ws expansion with its adjoint.  Restated from the
// published algorithm (Karras et al. 2020, "Analyzing and Improving the Image Quality of StyleGAN", appendix D); the reference leaves
// maua/parameterizations/stylegan.py empty, and the published projector.py is not among its files, so parity with that code is unpinned.
//
// Every operation here is rounded on its own (no contraction into fused multiply-adds; IEEE division and square root), and every
// reduction runs in one stated order, so tests/projection_ref.py restates each entry in float32 to the bit:
//   a sum over a range of elements is cut into chunks of RED_CHUNK = 4096; inside a chunk thread t of 256 adds elements t, t + 256, ...
//   in that order, the 256 sums fold as a[t] += a[t + s] for s = 128, 64, .. 1, and the chunks' sums are added in chunk order.
#include "common.h"
#include "internal.h"

#pragma clang fp contract(off)

namespace maua {
namespace {

constexpr int RED_CHUNK = 4096;
constexpr int REG_MAX_LEVELS = 16;

// the sum of f(i), i in [i0, i1) (at most RED_CHUNK of them), in the order the header states; every thread of the 256 gets it
template <typename F>
__device__ __forceinline__ float chunk_sum(long i0, long i1, float* red, F f) {
  float acc = 0.f;
  for (long i = i0 + threadIdx.x; i < i1; i += 256) acc += f(i);
  __syncthreads();   // (red may still be read from the sum before)
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int s = 128; s >= 1; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  return red[0];
}

// the chunks' sums in chunk order (one thread's work: at most a few hundred adds)
__device__ __forceinline__ float sum_in_order(const float* p, int n, int stride) {
  float t = p[0];
  for (int k = 1; k < n; k++) t += p[(long)k * stride];
  return t;
}

// ---- noise regulariser ----------------------------------------------------------------------------------------------------------------
struct RegPlan {
  int K;                          // levels
  int R[REG_MAX_LEVELS];          // side of level k
  int nchunk[REG_MAX_LEVELS];     // chunks of level k's R^2 elements
  int poff[REG_MAX_LEVELS];       // first chunk of level k among a sample's chunks
  long loff[REG_MAX_LEVELS];      // first element of level k among a sample's coarse levels (k >= 1)
  int chunks;                     // per sample
  long coarse;                    // elements of levels 1 .. K - 1 per sample
};

RegPlan reg_plan(int R) {
  RegPlan p{};
  int r = R, chunks = 0;
  long coarse = 0;
  for (int k = 0; k < REG_MAX_LEVELS; k++) {
    p.R[k] = r;
    p.nchunk[k] = (int)(((long)r * r + RED_CHUNK - 1) / RED_CHUNK);
    p.poff[k] = chunks;
    chunks += p.nchunk[k];
    p.loff[k] = coarse;
    if (k > 0) coarse += (long)r * r;
    p.K = k + 1;
    if (r <= 8) break;
    r /= 2;
  }
  p.chunks = chunks;
  p.coarse = coarse;
  return p;
}

size_t align256(size_t b) { return (b + 255) / 256 * 256; }
struct RegWorkspace { size_t pyr, gpyr, part, means, total; };
RegWorkspace reg_workspace(int B, const RegPlan& p) {
  RegWorkspace w;
  w.pyr = align256((size_t)B * p.coarse * 4);
  w.gpyr = w.pyr;
  w.part = align256((size_t)B * p.chunks * 2 * 4);
  w.means = align256((size_t)B * p.K * 2 * 4);
  w.total = w.pyr + w.gpyr + w.part + w.means;
  return w;
}

// dst[b][i][j] = ((src[2i][2j] + src[2i][2j+1]) + (src[2i+1][2j] + src[2i+1][2j+1])) / 4; r = side of dst.  grid (cdiv(r r, 256), B)
__global__ __launch_bounds__(256) void reg_pool_kernel(const float* __restrict__ src, long src_bstride, float* __restrict__ dst, long dst_bstride,
                                                       int r) {
  const int idx = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (idx >= r * r) return;
  const int i = idx / r, j = idx - i * r;
  const float* s = src + (long)b * src_bstride + (long)(2 * i) * (2 * r) + 2 * j;
  const float top = s[0] + s[1], bot = s[2 * r] + s[2 * r + 1];
  dst[(long)b * dst_bstride + idx] = (top + bot) * 0.25f;
}

// part[b][chunk][0 / 1] = the chunk's sum of n[i][j] n[i][j - 1] / of n[i][j] n[i - 1][j] (indices mod r).  grid (nchunk, B)
__global__ __launch_bounds__(256) void reg_sums_kernel(const float* __restrict__ n, long bstride, int r, float* __restrict__ part, int chunks,
                                                       int poff) {
  __shared__ float red[256];
  const int b = blockIdx.y, chunk = blockIdx.x;
  const float* nb = n + (long)b * bstride;
  const long N = (long)r * r, i0 = (long)chunk * RED_CHUNK, i1 = i0 + RED_CHUNK < N ? i0 + RED_CHUNK : N;
  const int mask = r - 1;
  const float sx = chunk_sum(i0, i1, red, [&](long e) {
    const int i = (int)(e / r), j = (int)(e - (long)i * r);
    return nb[e] * nb[(long)i * r + ((j - 1) & mask)];
  });
  const float sy = chunk_sum(i0, i1, red, [&](long e) {
    const int i = (int)(e / r), j = (int)(e - (long)i * r);
    return nb[e] * nb[(long)((i - 1) & mask) * r + j];
  });
  if (threadIdx.x == 0) {
    float* o = part + ((long)b * chunks + poff + chunk) * 2;
    o[0] = sx;
    o[1] = sy;
  }
}

// means[b][k][dir] = (the level's chunks in order) / R_k^2;  loss[b] = sum over k in order of (mx mx, then my my).  grid (B), 64 threads
__global__ __launch_bounds__(64) void reg_means_kernel(const float* __restrict__ part, RegPlan p, float* __restrict__ means, float* __restrict__ loss) {
  __shared__ float m[2 * REG_MAX_LEVELS];
  const int b = blockIdx.x, t = threadIdx.x;
  if (t < 2 * p.K) {
    const int k = t >> 1, dir = t & 1;
    const float s = sum_in_order(part + ((long)b * p.chunks + p.poff[k]) * 2 + dir, p.nchunk[k], 2);
    m[t] = s / (float)((long)p.R[k] * p.R[k]);
    means[(long)b * p.K * 2 + t] = m[t];
  }
  __syncthreads();
  if (t == 0 && loss) {
    float l = 0.f;
    for (int k = 0; k < p.K; k++) {
      l += m[2 * k] * m[2 * k];
      l += m[2 * k + 1] * m[2 * k + 1];
    }
    loss[b] = l;
  }
}

// g_k[i][j] = cx (n[i][j-1] + n[i][j+1]) + cy (n[i-1][j] + n[i+1][j]) (+ g_{k+1}[i/2][j/2] / 4: the pooling's adjoint), cx = 2 mx / R^2;
// the finest level: out (+)= weight g_0.  grid (cdiv(r r, 256), B)
__global__ __launch_bounds__(256) void reg_grad_kernel(const float* __restrict__ n, long bstride, int r, const float* __restrict__ means, int K,
                                                       int k, const float* __restrict__ g_coarse, long gc_bstride, float* __restrict__ g,
                                                       long g_bstride, int finest, float weight, int accumulate) {
  const int idx = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (idx >= r * r) return;
  const int i = idx / r, j = idx - i * r, mask = r - 1;
  const float* nb = n + (long)b * bstride;
  const float N = (float)((long)r * r);
  const float cx = (2.f * means[((long)b * K + k) * 2]) / N, cy = (2.f * means[((long)b * K + k) * 2 + 1]) / N;
  const float hx = nb[(long)i * r + ((j - 1) & mask)] + nb[(long)i * r + ((j + 1) & mask)];
  const float hy = nb[(long)((i - 1) & mask) * r + j] + nb[(long)((i + 1) & mask) * r + j];
  float v = cx * hx + cy * hy;
  if (g_coarse) v = v + 0.25f * g_coarse[(long)b * gc_bstride + (long)(i >> 1) * (r >> 1) + (j >> 1)];
  float* o = g + (long)b * g_bstride + idx;
  if (!finest) {
    *o = v;
  } else {
    const float wv = weight * v;
    *o = accumulate ? *o + wv : wv;
  }
}

int noise_reg_check(const float* n, int B, int R, const float* loss, const float* grad, const void* ws, long ws_bytes) {
  MAUA_REQUIRE(B >= 0, "maua_noise_reg: the batch must not be negative");
  MAUA_REQUIRE(R >= 4 && R <= 16384 && (R & (R - 1)) == 0, "maua_noise_reg: the map side must be a power of two, at least 4 and at most 16384");
  MAUA_REQUIRE(B <= 65535, "maua_noise_reg: grid too large");
  MAUA_REQUIRE(n && (loss || grad), "maua_noise_reg: NULL maps, or neither loss nor grad wanted");
  MAUA_REQUIRE(ws && ws_bytes >= (long)reg_workspace(B, reg_plan(R)).total, "maua_noise_reg: the workspace is NULL or shorter than maua_noise_reg_workspace_bytes()");
  MAUA_REQUIRE(((size_t)ws & 255) == 0, "maua_noise_reg: the workspace must be 256-byte aligned");
  return MAUA_OK;
}

// ---- Adam -----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ param, const float* __restrict__ grad, float* __restrict__ m,
                                                   float* __restrict__ v, long n, float beta1, float beta2, float eps, float step,
                                                   float inv_sqrt_bc2) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float g = grad[i];
  const float omb1 = 1.f - beta1, omb2 = 1.f - beta2;
  const float mi = m[i] + omb1 * (g - m[i]);
  const float vi = beta2 * v[i] + (omb2 * g) * g;
  const float denom = sqrtf(vi) * inv_sqrt_bc2 + eps;
  m[i] = mi;
  v[i] = vi;
  param[i] = param[i] - (step * mi) / denom;
}

int adam_check(const float* param, const float* grad, const float* m, const float* v, long n, float beta1, float beta2, float eps) {
  MAUA_REQUIRE(n >= 0 && n < (1L << 39), "maua_adam_step: bad element count");
  MAUA_REQUIRE(n == 0 || (param && grad && m && v), "maua_adam_step: NULL argument");
  MAUA_REQUIRE(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f, "maua_adam_step: the betas must lie in [0, 1)");
  MAUA_REQUIRE(eps >= 0.f, "maua_adam_step: eps must not be negative");
  return MAUA_OK;
}

// ---- renormalisation ------------------------------------------------------------------------------------------------------------------
// pass 0: part[map][chunk] = chunk sums of n;  pass 1: n -= mean, part2[map][chunk] = chunk sums of the new n^2;  pass 2: n *= 1 / sqrt(mean
// of squares).  mean = (chunks in order) / N.  grid (nchunk, maps)
__global__ __launch_bounds__(256) void renorm_kernel(float* __restrict__ n, long N, int nchunk, float* __restrict__ part, float* __restrict__ part2,
                                                     int pass) {
  __shared__ float red[256];
  __shared__ float bc;
  const int map = blockIdx.y, chunk = blockIdx.x;
  float* nm = n + (long)map * N;
  const long i0 = (long)chunk * RED_CHUNK, i1 = i0 + RED_CHUNK < N ? i0 + RED_CHUNK : N;
  if (pass == 0) {
    const float s = chunk_sum(i0, i1, red, [&](long e) { return nm[e]; });
    if (threadIdx.x == 0) part[(long)map * nchunk + chunk] = s;
    return;
  }
  if (threadIdx.x == 0) {
    const float s = sum_in_order((pass == 1 ? part : part2) + (long)map * nchunk, nchunk, 1) / (float)N;
    bc = pass == 1 ? s : 1.f / sqrtf(s);
  }
  __syncthreads();
  const float c = bc;
  if (pass == 1) {
    const float s = chunk_sum(i0, i1, red, [&](long e) {
      const float x = nm[e] - c;
      nm[e] = x;
      return x * x;
    });
    if (threadIdx.x == 0) part2[(long)map * nchunk + chunk] = s;
  } else {
    for (long e = i0 + threadIdx.x; e < i1; e += 256) nm[e] = nm[e] * c;
  }
}

long renorm_chunks(long N) { return (N + RED_CHUNK - 1) / RED_CHUNK; }
size_t renorm_workspace(int maps, long N) { return 2 * align256((size_t)maps * renorm_chunks(N) * 4); }

int renorm_check(const float* n, int maps, long N, const void* ws, long ws_bytes) {
  MAUA_REQUIRE(maps >= 0 && maps <= 65535, "maua_noise_renorm: the number of maps must lie in 0 .. 65535");
  MAUA_REQUIRE(N > 0 && N <= (1L << 31), "maua_noise_renorm: a map must have between 1 and 2^31 elements");
  MAUA_REQUIRE(n, "maua_noise_renorm: NULL maps");
  MAUA_REQUIRE(ws && ws_bytes >= (long)renorm_workspace(maps, N), "maua_noise_renorm: the workspace is NULL or shorter than maua_noise_renorm_workspace_bytes()");
  MAUA_REQUIRE(((size_t)ws & 255) == 0, "maua_noise_renorm: the workspace must be 256-byte aligned");
  return MAUA_OK;
}

// ---- w -> ws and back -----------------------------------------------------------------------------------------------------------------
// ws[b][r][k] = w[b][r_in][k] + scale eps[b][r_in][k], r_in = 0 (w_rows == 1) or r; thread = one element of ws
__global__ __launch_bounds__(256) void latent_expand_kernel(const float* __restrict__ w, const float* __restrict__ eps, float scale,
                                                            float* __restrict__ ws, int w_rows, int num_ws, int w_dim, long total) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int k = (int)(idx % w_dim);
  const long q = idx / w_dim;
  const int r = (int)(q % num_ws);
  const long b = q / num_ws;
  const long src = (b * w_rows + (w_rows == 1 ? 0 : r)) * w_dim + k;
  float v = w[src];
  if (eps) v = v + scale * eps[src];
  ws[idx] = v;
}

// g_w[b][k] = sum_r g_ws[b][r][k], rows in order; thread = one element of g_w
__global__ __launch_bounds__(256) void latent_reduce_kernel(const float* __restrict__ g_ws, float* __restrict__ g_w, int num_ws, int w_dim,
                                                            long total) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int k = (int)(idx % w_dim);
  const long b = idx / w_dim;
  const float* g = g_ws + b * num_ws * w_dim + k;
  float t = g[0];
  for (int r = 1; r < num_ws; r++) t += g[(long)r * w_dim];
  g_w[idx] = t;
}

int latent_expand_check(const float* w, int w_rows, const float* ws, int B, int num_ws, int w_dim) {
  MAUA_REQUIRE(B >= 0 && num_ws > 0 && w_dim > 0, "maua_latent_expand: bad shape");
  MAUA_REQUIRE(w_rows == 1 || w_rows == num_ws, "maua_latent_expand: w must have one row (space w) or num_ws rows (space w+)");
  MAUA_REQUIRE((long)B * num_ws * w_dim < (1L << 39), "maua_latent_expand: too many elements");
  MAUA_REQUIRE(B == 0 || (w && ws), "maua_latent_expand: NULL argument");
  return MAUA_OK;
}

int latent_reduce_check(const float* g_ws, const float* g_w, int B, int num_ws, int w_dim) {
  MAUA_REQUIRE(B >= 0 && num_ws > 0 && w_dim > 0, "maua_latent_reduce: bad shape");
  MAUA_REQUIRE((long)B * w_dim < (1L << 39), "maua_latent_reduce: too many elements");
  MAUA_REQUIRE(B == 0 || (g_ws && g_w), "maua_latent_reduce: NULL argument");
  return MAUA_OK;
}

}  // namespace
}  // namespace maua

using namespace maua;

extern "C" {

long maua_noise_reg_workspace_bytes(int B, int R) {
  if (B < 0 || R < 4 || R > 16384 || (R & (R - 1))) return 0;
  return (long)reg_workspace(B, reg_plan(R)).total;
}

int maua_noise_reg_levels(int R) {
  if (R < 4 || R > 16384 || (R & (R - 1))) return 0;
  return reg_plan(R).K;
}

int maua_noise_reg_check(const float* n, int B, int R, const float* loss, const float* grad, const void* ws, long ws_bytes) {
  return noise_reg_check(n, B, R, loss, grad, ws, ws_bytes);
}

int maua_noise_reg(maua_ctx* ctx, const float* n, int B, int R, float weight, float* loss, float* grad, int accumulate, void* ws,
                   long ws_bytes) {
  MAUA_REQUIRE(ctx, "maua_noise_reg: ctx is NULL");
  if (int rc = noise_reg_check(n, B, R, loss, grad, ws, ws_bytes)) return rc;
  if (B == 0) return MAUA_OK;
  const RegPlan p = reg_plan(R);
  const RegWorkspace w = reg_workspace(B, p);
  hipStream_t st = ctx->stream;
  float* pyr = (float*)ws;
  float* gpyr = (float*)((char*)ws + w.pyr);
  float* part = (float*)((char*)ws + w.pyr + w.gpyr);
  float* means = (float*)((char*)ws + w.pyr + w.gpyr + w.part);
  auto level = [&](int k) -> const float* { return k == 0 ? n : pyr + p.loff[k]; };
  auto bstride = [&](int k) -> long { return k == 0 ? (long)R * R : p.coarse; };
  for (int k = 0; k < p.K; k++) {
    const int r = p.R[k];
    if (k > 0)
      hipLaunchKernelGGL(reg_pool_kernel, dim3(cdiv(r * r, 256), B), dim3(256), 0, st, level(k - 1), bstride(k - 1), pyr + p.loff[k], p.coarse, r);
    hipLaunchKernelGGL(reg_sums_kernel, dim3(p.nchunk[k], B), dim3(256), 0, st, level(k), bstride(k), r, part, p.chunks, p.poff[k]);
  }
  hipLaunchKernelGGL(reg_means_kernel, dim3(B), dim3(64), 0, st, part, p, means, loss);
  if (grad)
    for (int k = p.K - 1; k >= 0; k--) {
      const int r = p.R[k];
      const float* gc = k + 1 < p.K ? gpyr + p.loff[k + 1] : nullptr;
      hipLaunchKernelGGL(reg_grad_kernel, dim3(cdiv(r * r, 256), B), dim3(256), 0, st, level(k), bstride(k), r, means, p.K, k, gc, p.coarse,
                         k == 0 ? grad : gpyr + p.loff[k], k == 0 ? (long)R * R : p.coarse, k == 0, weight, accumulate);
    }
  MAUA_HIP_CHECK(hipGetLastError());
  return MAUA_OK;
}

int maua_adam_step_check(const float* param, const float* grad, const float* m, const float* v, long n, float beta1, float beta2, float eps) {
  return adam_check(param, grad, m, v, n, beta1, beta2, eps);
}

int maua_adam_step(maua_ctx* ctx, float* param, const float* grad, float* m, float* v, long n, float beta1, float beta2, float eps,
                   float step, float inv_sqrt_bc2) {
  MAUA_REQUIRE(ctx, "maua_adam_step: ctx is NULL");
  if (int rc = adam_check(param, grad, m, v, n, beta1, beta2, eps)) return rc;
  if (n == 0) return MAUA_OK;
  hipLaunchKernelGGL(adam_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, param, grad, m, v, n, beta1, beta2, eps, step,
                     inv_sqrt_bc2);
  MAUA_HIP_CHECK(hipGetLastError());
  return MAUA_OK;
}

long maua_noise_renorm_workspace_bytes(int maps, long N) {
  if (maps < 0 || N <= 0) return 0;
  return (long)renorm_workspace(maps, N);
}

int maua_noise_renorm_check(const float* n, int maps, long N, const void* ws, long ws_bytes) { return renorm_check(n, maps, N, ws, ws_bytes); }

int maua_noise_renorm(maua_ctx* ctx, float* n, int maps, long N, void* ws, long ws_bytes) {
  MAUA_REQUIRE(ctx, "maua_noise_renorm: ctx is NULL");
  if (int rc = renorm_check(n, maps, N, ws, ws_bytes)) return rc;
  if (maps == 0) return MAUA_OK;
  const int nchunk = (int)renorm_chunks(N);
  float* part = (float*)ws;
  float* part2 = (float*)((char*)ws + renorm_workspace(maps, N) / 2);
  for (int pass = 0; pass < 3; pass++)
    hipLaunchKernelGGL(renorm_kernel, dim3(nchunk, maps), dim3(256), 0, ctx->stream, n, N, nchunk, part, part2, pass);
  MAUA_HIP_CHECK(hipGetLastError());
  return MAUA_OK;
}

int maua_latent_expand_check(const float* w, int w_rows, const float* eps, const float* ws, int B, int num_ws, int w_dim) {
  (void)eps;
  return latent_expand_check(w, w_rows, ws, B, num_ws, w_dim);
}

int maua_latent_expand(maua_ctx* ctx, const float* w, int w_rows, const float* eps, float scale, float* ws, int B, int num_ws, int w_dim) {
  MAUA_REQUIRE(ctx, "maua_latent_expand: ctx is NULL");
  if (int rc = latent_expand_check(w, w_rows, ws, B, num_ws, w_dim)) return rc;
  const long total = (long)B * num_ws * w_dim;
  if (total == 0) return MAUA_OK;
  hipLaunchKernelGGL(latent_expand_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, w, eps, scale, ws, w_rows, num_ws,
                     w_dim, total);
  MAUA_HIP_CHECK(hipGetLastError());
  return MAUA_OK;
}

int maua_latent_reduce_check(const float* g_ws, const float* g_w, int B, int num_ws, int w_dim) {
  return latent_reduce_check(g_ws, g_w, B, num_ws, w_dim);
}

int maua_latent_reduce(maua_ctx* ctx, const float* g_ws, float* g_w, int B, int num_ws, int w_dim) {
  MAUA_REQUIRE(ctx, "maua_latent_reduce: ctx is NULL");
  if (int rc = latent_reduce_check(g_ws, g_w, B, num_ws, w_dim)) return rc;
  const long total = (long)B * w_dim;
  if (total == 0) return MAUA_OK;
  hipLaunchKernelGGL(latent_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, g_ws, g_w, num_ws, w_dim, total);
  MAUA_HIP_CHECK(hipGetLastError());
  return MAUA_OK;
}

}  // extern "C"
