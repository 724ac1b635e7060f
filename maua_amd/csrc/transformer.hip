// What CLIP's two towers share: LayerNorm and QuickGELU with their input gradients, the residual block
//   x += out_proj(attention(in_proj(ln_1(x))));  x += c_proj(QuickGELU(c_fc(ln_2(x))))
// forwards and backwards, and the loading of a block's parameters.  clip.hip's header describes the design; the towers differ in
// what a BlockRun says: the GEMM route, the causal mask, and which statistics / log-sum-exp rows are kept.
#include <cmath>
#include <cstring>

#include "clip_internal.h"
#include "quick_gelu.h"

using namespace maua;

namespace maua {
namespace {

// y = LayerNorm(x) * g + b per row of C values (float32 statistics, eps 1e-5: clip/model.py LayerNorm); stats[row] = (mean, rstd)
// one wave per row, 4 rows per workgroup
template <typename T>
__global__ __launch_bounds__(256) void layer_norm_kernel(const T* __restrict__ x, const float* __restrict__ g, const float* __restrict__ b,
                                                         T* __restrict__ y, float* __restrict__ stats, long rows, int C) {
  constexpr int E = Pc<T>::N;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  const int pieces = C / E;
  float v[LN_MAXP][E];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < LN_MAXP; i++) {
    const int p = lane + 64 * i;
    if (p < pieces) {
      Pc<T>::load(x + row * C + (long)p * E, v[i]);
#pragma unroll
      for (int e = 0; e < E; e++) s += v[i][e];
    }
  }
  const float mean = wave_sum(s) / (float)C;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < LN_MAXP; i++)
    if (lane + 64 * i < pieces) {
#pragma unroll
      for (int e = 0; e < E; e++) { const float d = v[i][e] - mean; q = fmaf(d, d, q); }
    }
  const float rstd = rsqrtf(wave_sum(q) / (float)C + 1e-5f);
  if (stats && lane == 0) { stats[2 * row] = mean; stats[2 * row + 1] = rstd; }
#pragma unroll
  for (int i = 0; i < LN_MAXP; i++) {
    const int p = lane + 64 * i;
    if (p < pieces) {
      float o[E];
#pragma unroll
      for (int e = 0; e < E; e++) o[e] = fmaf((v[i][e] - mean) * rstd, g[p * E + e], b[p * E + e]);
      Pc<T>::store(y + row * C + (long)p * E, o);
    }
  }
}

// dx = rstd * (g dy - mean(g dy) - xhat mean(g dy xhat)) (+ add): the input gradient of the kernel above.  drop_T > 0: rows are tokens
// [image][drop_T]; the class token's row (t == 0) is not written and the others are stored densely [image][drop_T - 1] (ln_pre: what
// flows on to the patch embedding)
template <typename T>
__global__ __launch_bounds__(256) void layer_norm_vjp_kernel(const T* __restrict__ x, const float* __restrict__ stats,
                                                             const float* __restrict__ g, const T* __restrict__ dy,
                                                             const T* __restrict__ add, T* __restrict__ dx, long rows, int C, int drop_T) {
  constexpr int E = Pc<T>::N;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  long orow = row;
  if (drop_T > 0) {
    const long im = row / drop_T;
    const int t = (int)(row - im * drop_T);
    if (t == 0) return;
    orow = im * (drop_T - 1) + t - 1;
  }
  const int pieces = C / E;
  const float mean = stats[2 * row], rstd = stats[2 * row + 1];
  float xh[LN_MAXP][E], gd[LN_MAXP][E];
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int i = 0; i < LN_MAXP; i++) {
    const int p = lane + 64 * i;
    if (p < pieces) {
      float xv[E], dv[E];
      Pc<T>::load(x + row * C + (long)p * E, xv);
      Pc<T>::load(dy + row * C + (long)p * E, dv);
#pragma unroll
      for (int e = 0; e < E; e++) {
        xh[i][e] = (xv[e] - mean) * rstd;
        gd[i][e] = dv[e] * g[p * E + e];
        s1 += gd[i][e];
        s2 = fmaf(gd[i][e], xh[i][e], s2);
      }
    }
  }
  const float m1 = wave_sum(s1) / (float)C, m2 = wave_sum(s2) / (float)C;
#pragma unroll
  for (int i = 0; i < LN_MAXP; i++) {
    const int p = lane + 64 * i;
    if (p < pieces) {
      float o[E];
#pragma unroll
      for (int e = 0; e < E; e++) o[e] = rstd * (gd[i][e] - m1 - xh[i][e] * m2);
      if (add) {
        float av[E];
        Pc<T>::load(add + row * C + (long)p * E, av);
#pragma unroll
        for (int e = 0; e < E; e++) o[e] += av[e];
      }
      Pc<T>::store(dx + orow * C + (long)p * E, o);
    }
  }
}

// a = h * sigmoid(1.702 h)   |   dh = da * (s + 1.702 h s (1 - s))
template <typename T>
__global__ __launch_bounds__(256) void quick_gelu_kernel(const T* __restrict__ h, T* __restrict__ a, long pieces) {
  constexpr int E = Pc<T>::N;
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= pieces) return;
  float v[E];
  Pc<T>::load(h + p * E, v);
#pragma unroll
  for (int e = 0; e < E; e++) v[e] = quick_gelu_f(v[e], sizeof(T) == 4);
  Pc<T>::store(a + p * E, v);
}
template <typename T>
__global__ __launch_bounds__(256) void quick_gelu_vjp_kernel(const T* __restrict__ h, const T* da, T* dh, long pieces) {   // (dh may be da)
  constexpr int E = Pc<T>::N;
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= pieces) return;
  float v[E], d[E];
  Pc<T>::load(h + p * E, v);
  Pc<T>::load(da + p * E, d);
#pragma unroll
  for (int e = 0; e < E; e++) d[e] *= quick_gelu_grad_f(v[e], sizeof(T) == 4);
  Pc<T>::store(dh + p * E, d);
}

}  // namespace

// the one place the element type of each of these kernels is chosen
void launch_layer_norm(hipStream_t st, int dtype, const void* x, const float* g, const float* b, void* y, float* stats, long rows, int C) {
  const dim3 grid((unsigned)((rows + 3) / 4));
  dispatch_dtype<bf16_t, float>(dtype, "layer_norm", [&](auto t) {
    hipLaunchKernelGGL(layer_norm_kernel<decltype(t)>, grid, dim3(256), 0, st, (const decltype(t)*)x, g, b, (decltype(t)*)y, stats, rows, C);
  });
}
void launch_layer_norm_vjp(hipStream_t st, int dtype, const void* x, const float* stats, const float* g, const void* dy, const void* add,
                           void* dx, long rows, int C, int drop_T) {
  const dim3 grid((unsigned)((rows + 3) / 4));
  dispatch_dtype<bf16_t, float>(dtype, "layer_norm_vjp", [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(layer_norm_vjp_kernel<T>, grid, dim3(256), 0, st, (const T*)x, stats, g, (const T*)dy, (const T*)add, (T*)dx, rows, C, drop_T);
  });
}
void launch_quick_gelu(hipStream_t st, int dtype, const void* h, void* a, long count) {
  const long pieces = count / elems_per_piece(dtype);
  const dim3 grid((unsigned)((pieces + 255) / 256));
  dispatch_dtype<bf16_t, float>(dtype, "quick_gelu", [&](auto t) {
    hipLaunchKernelGGL(quick_gelu_kernel<decltype(t)>, grid, dim3(256), 0, st, (const decltype(t)*)h, (decltype(t)*)a, pieces);
  });
}
void launch_quick_gelu_vjp(hipStream_t st, int dtype, const void* h, const void* da, void* dh, long count) {
  const long pieces = count / elems_per_piece(dtype);
  const dim3 grid((unsigned)((pieces + 255) / 256));
  dispatch_dtype<bf16_t, float>(dtype, "quick_gelu_vjp", [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(quick_gelu_vjp_kernel<T>, grid, dim3(256), 0, st, (const T*)h, (const T*)da, (T*)dh, pieces);
  });
}

int block_gemm(const BlockRun& r, const void* a, long M, int K, const void* w, int N, const float* bias, const void* res, void* c, int epi,
               void* c2, const void* aux) {
  GemmArgs g{};
  g.a0 = a; g.lda0 = K; g.K0 = K; g.w = w; g.bias = bias; g.res = res; g.ldr = N; g.c = c; g.ldc = N; g.M = M; g.N = N;
  g.prefer_dma = r.prefer_dma;
  if (epi && r.prefer_dma) {
    GemmArgs f = g;
    f.epi = epi; f.c2 = c2; f.ldc2 = N; f.aux = aux; f.ldaux = N;
    if (gemm_dma_supported(r.dtype, f)) return launch_gemm_nt(r.st, r.dtype, f);
  }
  return launch_gemm_nt(r.st, r.dtype, g);
}
// QuickGELU / its derivative rides on this GEMM's epilogue (else: a pass of its own behind the plain GEMM)
static bool gemm_fuses(const BlockRun& r, long M, int K, int N) {
  GemmArgs g{};
  int dummy;
  g.a0 = &dummy; g.lda0 = K; g.K0 = K; g.w = &dummy; g.c = &dummy; g.ldc = N; g.M = M; g.N = N; g.epi = 1; g.c2 = &dummy; g.ldc2 = N;
  return r.prefer_dma && gemm_dma_supported(r.dtype, g);
}

int block_forward(const BlockRun& r, const BlockWeights& l, const void* x, const BlockActs& k, void* lno, void* act, void* xn) {
  const int w = r.width;
  const long M = r.gemm_rows;
  // x -> ln_1 -> in_proj -> attention -> out_proj (+ x) = xm
  launch_layer_norm(r.st, r.dtype, x, l.ln1_g.as<float>(), l.ln1_b.as<float>(), lno, k.st1, r.rows, w);
  if (int rc = block_gemm(r, lno, M, w, l.w_qkv.get(), 3 * w, l.b_qkv.as<float>(), nullptr, k.qkv)) return rc;
  AttnArgs a{};
  a.qkv = k.qkv; a.out = k.ao; a.B = (int)r.N; a.T = r.Tk; a.heads = r.heads; a.D = w / r.heads; a.ld_qkv = 3 * w; a.ld_out = w;
  a.scale = 1.f / std::sqrt((float)a.D); a.lse = k.lse; a.causal = r.causal;
  if (int rc = launch_attention(r.st, r.dtype, a)) return rc;
  if (int rc = block_gemm(r, k.ao, M, w, l.w_out.get(), w, l.b_out.as<float>(), x, k.xm)) return rc;
  // xm -> ln_2 -> c_fc -> QuickGELU -> c_proj (+ xm) = next x
  launch_layer_norm(r.st, r.dtype, k.xm, l.ln2_g.as<float>(), l.ln2_b.as<float>(), lno, k.st2, r.rows, w);
  if (gemm_fuses(r, M, w, 4 * w)) {
    if (int rc = block_gemm(r, lno, M, w, l.w_fc.get(), 4 * w, l.b_fc.as<float>(), nullptr, k.h, 1, act)) return rc;
  } else {
    if (int rc = block_gemm(r, lno, M, w, l.w_fc.get(), 4 * w, l.b_fc.as<float>(), nullptr, k.h)) return rc;
    launch_quick_gelu(r.st, r.dtype, k.h, act, r.rows * 4 * w);
  }
  return block_gemm(r, act, M, 4 * w, l.w_pr.get(), w, l.b_pr.as<float>(), k.xm, xn);
}

int block_backward(const BlockRun& r, const BlockWeights& l, const BlockActs& k, void* dx, void* other, void* dqkv, void* dwide, void* dtmp,
                   float* delta) {
  const int w = r.width;
  const long M = r.gemm_rows;
  // MLP: d act = dx W_pr ; d h = d act * QuickGELU'(h) ; d ln2 = d h W_fc ; dxm = dx + LN2'(d ln2)
  if (gemm_fuses(r, M, w, 4 * w)) {
    if (int rc = block_gemm(r, dx, M, w, l.w_pr_t.get(), 4 * w, nullptr, nullptr, dwide, 2, nullptr, k.h)) return rc;
  } else {
    if (int rc = block_gemm(r, dx, M, w, l.w_pr_t.get(), 4 * w, nullptr, nullptr, dwide)) return rc;
    launch_quick_gelu_vjp(r.st, r.dtype, k.h, dwide, dwide, r.rows * 4 * w);
  }
  if (int rc = block_gemm(r, dwide, M, 4 * w, l.w_fc_t.get(), w, nullptr, nullptr, dtmp)) return rc;
  launch_layer_norm_vjp(r.st, r.dtype, k.xm, k.st2, l.ln2_g.as<float>(), dtmp, dx, other, r.rows, w, 0);   // other = d xm
  // attention: d ao = dxm W_out ; d qkv = attention'(d ao) ; d ln1 = d qkv W_qkv ; d x = dxm + LN1'(d ln1)
  if (int rc = block_gemm(r, other, M, w, l.w_out_t.get(), w, nullptr, nullptr, dtmp)) return rc;
  AttnVjpArgs v{};
  v.qkv = k.qkv; v.out = k.ao; v.d_out = dtmp; v.lse = k.lse; v.d_qkv = dqkv; v.delta = delta;
  v.B = (int)r.N; v.T = r.Tk; v.heads = r.heads; v.D = w / r.heads; v.ld_qkv = 3 * w; v.ld_out = w; v.scale = 1.f / std::sqrt((float)v.D);
  if (int rc = launch_attention_vjp(r.st, r.dtype, v)) return rc;
  if (int rc = block_gemm(r, dqkv, M, 3 * w, l.w_qkv_t.get(), w, nullptr, nullptr, dtmp)) return rc;
  launch_layer_norm_vjp(r.st, r.dtype, k.x, k.st1, l.ln1_g.as<float>(), dtmp, other, dx, r.rows, w, 0);
  return MAUA_OK;
}

// host float matrix [R][C] -> device T [R][C] (and optionally its transpose [C][R]); rows permuted by `perm` when given
int upload_matrix(int dtype, size_t esize, const float* h, int R, int C, const int* perm, DevBuf* dev, DevBuf* dev_t) {
  std::vector<float> a((size_t)R * C);
  for (int r = 0; r < R; r++) memcpy(&a[(size_t)r * C], h + (size_t)(perm ? perm[r] : r) * C, (size_t)C * 4);
  auto put = [&](const std::vector<float>& src, DevBuf* d) -> int {
    if (!*d)
      if (int rc = d->alloc(src.size() * esize)) return rc;
    if (dtype == MAUA_F32) {
      MAUA_HIP_CHECK(hipMemcpy(d->get(), src.data(), src.size() * 4, hipMemcpyHostToDevice));
    } else {
      std::vector<uint16_t> b(src.size());
      for (size_t i = 0; i < src.size(); i++) {   // round to nearest even
        uint32_t u;
        memcpy(&u, &src[i], 4);
        if ((u & 0x7f800000u) == 0x7f800000u) b[i] = (uint16_t)(u >> 16);
        else b[i] = (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
      }
      MAUA_HIP_CHECK(hipMemcpy(d->get(), b.data(), b.size() * 2, hipMemcpyHostToDevice));
    }
    return MAUA_OK;
  };
  if (int rc = put(a, dev)) return rc;
  if (dev_t) {
    std::vector<float> t((size_t)R * C);
    for (int r = 0; r < R; r++)
      for (int c = 0; c < C; c++) t[(size_t)c * R + r] = a[(size_t)r * C + c];
    if (int rc = put(t, dev_t)) return rc;
  }
  return MAUA_OK;
}
int upload_vec(const float* h, size_t count, const int* perm, DevBuf* dev) {
  std::vector<float> a(count);
  for (size_t i = 0; i < count; i++) a[i] = h[perm ? perm[i] : i];
  if (!*dev)
    if (int rc = dev->alloc(count * 4)) return rc;
  MAUA_HIP_CHECK(hipMemcpy(dev->get(), a.data(), count * 4, hipMemcpyHostToDevice));
  return MAUA_OK;
}

// the keys of CLIP's residual blocks, "transformer.resblocks.<i>.<par>" (the image tower below "visual.", the text tower at the top
// level).  with_t: the transposed weights too (the image tower's way back)
bool is_block_key(const std::string& s) { return s.compare(0, 22, "transformer.resblocks.") == 0; }

int load_block(std::vector<BlockWeights>& L, int dtype, size_t esize, int width, int heads, const char* who, const std::string& s,
               const float* host, size_t count, bool with_t) {
  const size_t p0 = 22;   // strlen("transformer.resblocks.")
  const int w = width;
  auto need = [&](size_t c) -> int {
    if (count != c) return fail(std::string(who) + ": " + s + ": wrong size");
    return MAUA_OK;
  };
  const size_t dot = s.find('.', p0);
  if (dot == std::string::npos) return fail(std::string(who) + ": unknown parameter name: " + s);
  const int i = atoi(s.substr(p0, dot - p0).c_str());
  if (i < 0 || i >= (int)L.size()) return fail(std::string(who) + ": no such block: " + s);
  BlockWeights& l = L[i];
  const std::string par = s.substr(dot + 1);
  // in_proj rows [q | k | v] x [head][d] -> head-major [head][q | k | v][d]: the layout attention.hip reads
  const int D = w / heads;
  std::vector<int> perm(3 * w);
  for (int h = 0; h < heads; h++)
    for (int part = 0; part < 3; part++)
      for (int d = 0; d < D; d++) perm[(h * 3 + part) * D + d] = part * w + h * D + d;
  auto t = [&](DevBuf* p) { return with_t ? p : nullptr; };
  if (par == "attn.in_proj_weight") { if (int rc = need((size_t)3 * w * w)) return rc; return upload_matrix(dtype, esize, host, 3 * w, w, perm.data(), &l.w_qkv, t(&l.w_qkv_t)); }
  if (par == "attn.in_proj_bias") { if (int rc = need((size_t)3 * w)) return rc; return upload_vec(host, 3 * w, perm.data(), &l.b_qkv); }
  if (par == "attn.out_proj.weight") { if (int rc = need((size_t)w * w)) return rc; return upload_matrix(dtype, esize, host, w, w, nullptr, &l.w_out, t(&l.w_out_t)); }
  if (par == "attn.out_proj.bias") { if (int rc = need(w)) return rc; return upload_vec(host, w, nullptr, &l.b_out); }
  if (par == "mlp.c_fc.weight") { if (int rc = need((size_t)4 * w * w)) return rc; return upload_matrix(dtype, esize, host, 4 * w, w, nullptr, &l.w_fc, t(&l.w_fc_t)); }
  if (par == "mlp.c_fc.bias") { if (int rc = need((size_t)4 * w)) return rc; return upload_vec(host, 4 * w, nullptr, &l.b_fc); }
  if (par == "mlp.c_proj.weight") { if (int rc = need((size_t)4 * w * w)) return rc; return upload_matrix(dtype, esize, host, w, 4 * w, nullptr, &l.w_pr, t(&l.w_pr_t)); }
  if (par == "mlp.c_proj.bias") { if (int rc = need(w)) return rc; return upload_vec(host, w, nullptr, &l.b_pr); }
  if (par == "ln_1.weight") { if (int rc = need(w)) return rc; return upload_vec(host, w, nullptr, &l.ln1_g); }
  if (par == "ln_1.bias") { if (int rc = need(w)) return rc; return upload_vec(host, w, nullptr, &l.ln1_b); }
  if (par == "ln_2.weight") { if (int rc = need(w)) return rc; return upload_vec(host, w, nullptr, &l.ln2_g); }
  if (par == "ln_2.bias") { if (int rc = need(w)) return rc; return upload_vec(host, w, nullptr, &l.ln2_b); }
  return fail(std::string(who) + ": unknown parameter name: " + s);
}

bool blocks_loaded(const std::vector<BlockWeights>& L) {
  bool ok = true;
  for (auto& l : L)
    ok = ok && l.w_qkv && l.w_out && l.w_fc && l.w_pr && l.b_qkv && l.b_out && l.b_fc && l.b_pr && l.ln1_g && l.ln1_b && l.ln2_g && l.ln2_b;
  return ok;
}

}  // namespace maua

extern "C" {

// nn.LayerNorm over the last dimension of [rows][C] (float32 statistics, eps 1e-5) and its input gradient; stats: [rows][2] f32
int maua_layer_norm(maua_ctx* ctx, const void* x, const float* gamma, const float* beta, long rows, int C, int dtype, void* y, float* stats) {
  MAUA_REQUIRE(ctx && x && gamma && beta && y, "maua_layer_norm: NULL argument");
  MAUA_REQUIRE(dtype == MAUA_BF16 || dtype == MAUA_F32, "maua_layer_norm: f32 / bf16");
  const int epc = elems_per_piece(dtype);
  MAUA_REQUIRE(C % epc == 0 && C / epc <= 64 * LN_MAXP, "maua_layer_norm: C must be a multiple of 16 bytes and at most 4096 (bf16) / 2048 (f32)");
  if (rows == 0) return MAUA_OK;
  launch_layer_norm(ctx->stream, dtype, x, gamma, beta, y, stats, rows, C);
  MAUA_HIP_CHECK(hipGetLastError());
  return MAUA_OK;
}
int maua_layer_norm_vjp(maua_ctx* ctx, const void* x, const float* stats, const float* gamma, const void* dy, const void* add, long rows, int C,
                        int dtype, void* dx) {
  MAUA_REQUIRE(ctx && x && stats && gamma && dy && dx, "maua_layer_norm_vjp: NULL argument");
  MAUA_REQUIRE(dtype == MAUA_BF16 || dtype == MAUA_F32, "maua_layer_norm_vjp: f32 / bf16");
  const int epc = elems_per_piece(dtype);
  MAUA_REQUIRE(C % epc == 0 && C / epc <= 64 * LN_MAXP, "maua_layer_norm_vjp: C must be a multiple of 16 bytes and at most 4096 (bf16) / 2048 (f32)");
  if (rows == 0) return MAUA_OK;
  launch_layer_norm_vjp(ctx->stream, dtype, x, stats, gamma, dy, add, dx, rows, C, 0);
  MAUA_HIP_CHECK(hipGetLastError());
  return MAUA_OK;
}

}  // extern "C"
