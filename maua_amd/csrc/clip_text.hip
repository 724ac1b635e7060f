// CLIP's text tower (CLIP.encode_text): forward only - prompts are constants of the guided loop.
//   tokens [N][ctx] int32 -> x = token_embedding[tokens] + positional_embedding -> L x { x += out_proj(causal attention(in_proj(ln_1(x))));
//   x += c_proj(QuickGELU(c_fc(ln_2(x)))) } -> ln_final(x[n, argmax(tokens[n])]) @ text_projection -> [N][E] f32
// The blocks are the image tower's (transformer.hip's block_forward) with the causal mask (build_attention_mask: triu(-inf, 1)) and no
// kept activations.
#include <cmath>

#include "clip_internal.h"

using namespace maua;

namespace maua {
namespace {

// x[n][t][c] = token_embedding[tokens[n][t]][c] + positional_embedding[t][c], rounded to T once
template <typename T>
__global__ __launch_bounds__(256) void text_tokens_kernel(const int* __restrict__ tokens, const float* __restrict__ emb, const float* __restrict__ pos,
                                                          T* __restrict__ x, long N, int Tk, int C, int vocab) {
  constexpr int E = Pc<T>::N;
  const int ppr = C / E;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= N * Tk * ppr) return;
  const int pc = (int)(idx % ppr);
  const long nt = idx / ppr;
  const int t = (int)(nt % Tk);
  const int id = min(max(tokens[nt], 0), vocab - 1);   // (the host validates the ids; this keeps a bad one inside the table)
  const float* er = emb + (long)id * C + pc * E;
  const float* pr = pos + (long)t * C + pc * E;
  float v[E];
#pragma unroll
  for (int e = 0; e < E; e++) v[e] = er[e] + pr[e];
  Pc<T>::store(x + nt * C + (long)pc * E, v);
}

// per sequence, one workgroup, float32: eot = argmax(tokens[n]) (the first maximum, as torch.argmax), ln_final of that row only (a
// LayerNorm is per row: the same as CLIP's ln_final over every row followed by the gather), @ text_projection -> embed[n]
template <typename T>
__global__ __launch_bounds__(256) void text_head_kernel(const int* __restrict__ tokens, const T* __restrict__ x, const float* __restrict__ g,
                                                        const float* __restrict__ b, const float* __restrict__ proj, float* __restrict__ embed,
                                                        int Tk, int w, int E) {
  extern __shared__ float sm[];
  float* z = sm;               // [w]
  float* red = z + w;          // [4]
  int* eot = (int*)(red + 4);  // [1]
  const int tid = threadIdx.x;
  const long n = blockIdx.x;
  if (tid < 64) {
    const int* row = tokens + n * Tk;
    int best = row[0], at = 0;
    for (int t = tid; t < Tk; t += 64)
      if (row[t] > best) { best = row[t]; at = t; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const int ob = __shfl_xor(best, o), oa = __shfl_xor(at, o);
      if (ob > best || (ob == best && oa < at)) { best = ob; at = oa; }
    }
    if (tid == 0) *eot = at;
  }
  __syncthreads();
  const T* xr = x + (n * Tk + *eot) * w;
  float s = 0.f;
  for (int c = tid; c < w; c += 256) { const float v = Elem<T>::load(xr + c); z[c] = v; s += v; }
  const float mean = block_sum(s, red) / (float)w;
  float q = 0.f;
  for (int c = tid; c < w; c += 256) { const float d = z[c] - mean; q = fmaf(d, d, q); }
  const float rstd = rsqrtf(block_sum(q, red) / (float)w + 1e-5f);
  for (int c = tid; c < w; c += 256) z[c] = fmaf((z[c] - mean) * rstd, g[c], b[c]);
  __syncthreads();
  for (int j = tid; j < E; j += 256) {
    float acc = 0.f;
    for (int c = 0; c < w; c++) acc = fmaf(z[c], proj[(long)c * E + j], acc);
    embed[n * E + j] = acc;
  }
}

// The text tower's GEMMs run on ONE kernel for every batch size - gemm.hip's 128 x 128 register-staged kernel, never the LDS-direct
// one (chosen by the row count) nor the small-M one - over at least TEXT_MIN_ROWS rows (the rows past N * ctx are workspace, zeroed
// at allocation, never read back): a prompt's embedding then does not depend on what else is in the batch, so prompts embedded one by
// one, in a batch, or from the cache agree bit for bit.  (The tower runs once per prompt set, off the guided loop.)  In the run's
// terms: prefer_dma = 0 - which also keeps QuickGELU off the GEMM epilogue - and gemm_rows = text_rows().
constexpr long TEXT_MIN_ROWS = 128;

long text_rows(const maua_clip_text* n, long N) { return std::max<long>(N * n->ctx_len, TEXT_MIN_ROWS); }

// sequences per pass: 32-bit byte offsets inside the GEMM operands (the MLP's [M][4 w]), <= 65535 (attention's grid)
long text_chunk(const maua_clip_text* n) {
  return std::max<long>(1, std::min<long>(65535, ((1L << 32) - 1) / ((long)n->ctx_len * 4 * n->width * (long)n->esize)));
}

// workspaces for N sequences, all allocated before the first launch of a pass
int ensure_text_ws(maua_clip_text* n, long N) {
  if (N <= n->cap) return MAUA_OK;
  MAUA_HIP_CHECK(hipStreamSynchronize(n->ctx->stream));
  n->cap = 0;
  const size_t es = n->esize, M = (size_t)text_rows(n, N), w = n->width;
  auto layout = [&](Scratch& s) {
    auto take = [&](size_t cols) -> void* { return s.take<char>(M * cols * w * es); };   // (columns in units of the width)
    n->xa = take(1); n->xb = take(1); n->lno = take(1);
    n->k.qkv = take(3); n->k.ao = take(1); n->k.xm = take(1); n->k.h = take(4);
    n->act = take(4);
  };
  if (carve_into(n->ws, layout)) return fail("maua_clip_text: out of device memory for the text tower's activations");
  MAUA_HIP_CHECK(hipMemset(n->ws.get(), 0, n->ws.bytes()));
  n->cap = N;
  return MAUA_OK;
}

int text_forward(maua_clip_text* n, const int* tokens, long N, float* embeds) {
  const int w = n->width, Tk = n->ctx_len;
  const BlockRun r{n->ctx->stream, n->dtype, w, n->heads, N, Tk, N * Tk, text_rows(n, N), 0, 1};
  const long total = r.rows * (w / elems_per_piece(n->dtype));
  const dim3 tgrid((unsigned)((total + 255) / 256));
  dispatch_dtype<bf16_t, float>(n->dtype, "maua_clip_text", [&](auto t) {
    hipLaunchKernelGGL(text_tokens_kernel<decltype(t)>, tgrid, dim3(256), 0, r.st, tokens, n->tok_emb.as<float>(), n->pos.as<float>(), (decltype(t)*)n->xa, N, Tk, w, n->vocab);
  });
  void* x = n->xa;
  void* other = n->xb;
  for (int i = 0; i < n->layers; i++) {
    if (int rc = block_forward(r, n->L[i], x, n->k, n->lno, n->act, other)) return rc;
    std::swap(x, other);
  }
  const size_t smem = ((size_t)w + 8) * 4;
  dispatch_dtype<bf16_t, float>(n->dtype, "maua_clip_text", [&](auto t) {
    hipLaunchKernelGGL(text_head_kernel<decltype(t)>, dim3((unsigned)N), dim3(256), smem, r.st, tokens, (const decltype(t)*)x, n->lnf_g.as<float>(), n->lnf_b.as<float>(),
                       n->proj.as<float>(), embeds, Tk, w, n->E);
  });
  MAUA_HIP_CHECK(hipGetLastError());
  return MAUA_OK;
}

}  // namespace
}  // namespace maua

extern "C" {

int maua_clip_text_create(maua_ctx* ctx, int context_length, int vocab_size, int width, int layers, int heads, int embed_dim, int dtype,
                          maua_clip_text** out) {
  MAUA_REQUIRE(ctx && out, "maua_clip_text_create: NULL argument");
  MAUA_REQUIRE(dtype == MAUA_BF16 || dtype == MAUA_F32, "maua_clip_text_create: dtype must be MAUA_BF16 or MAUA_F32");
  MAUA_REQUIRE(context_length > 0 && vocab_size > 0, "maua_clip_text_create: bad context length / vocabulary size");
  MAUA_REQUIRE(width > 0 && heads > 0 && width % heads == 0 && attention_supported(width / heads), "maua_clip_text_create: head width must be 32 or 64");
  const int epc = elems_per_piece(dtype), kc = elems_per_chunk(dtype, 64);
  MAUA_REQUIRE(width % 32 == 0 && width % kc == 0 && width / epc <= 64 * LN_MAXP, "maua_clip_text_create: width must be a multiple of 32 (at most 4096 / 2048)");
  MAUA_REQUIRE(layers > 0 && embed_dim > 0, "maua_clip_text_create: bad layer count / embedding size");
  maua_clip_text* n = new maua_clip_text();
  n->ctx = ctx; n->dtype = dtype; n->esize = elem_bytes(dtype);
  n->ctx_len = context_length; n->vocab = vocab_size; n->width = width; n->layers = layers; n->heads = heads; n->E = embed_dim;
  n->L.resize(layers);
  *out = n;
  return MAUA_OK;
}

void maua_clip_text_destroy(maua_clip_text* n) {
  if (!n) return;
  hipStreamSynchronize(n->ctx->stream);
  delete n;
}

// name: a text-half key of CLIP's state dict ("token_embedding.weight", "positional_embedding", "transformer.resblocks.<i>.*",
// "ln_final.weight", "ln_final.bias", "text_projection"); host float32 data in the checkpoint's layout
int maua_clip_text_load(maua_clip_text* n, const char* name, const float* host, size_t count) {
  MAUA_REQUIRE(n && name && host, "maua_clip_text_load: NULL argument");
  MAUA_HIP_CHECK(hipStreamSynchronize(n->ctx->stream));
  const std::string s(name);
  const int w = n->width;
  auto need = [&](size_t c) -> int {
    if (count != c) return fail("maua_clip_text_load: " + s + ": wrong size");
    return MAUA_OK;
  };
  if (s == "token_embedding.weight") { if (int rc = need((size_t)n->vocab * w)) return rc; return upload_vec(host, (size_t)n->vocab * w, nullptr, &n->tok_emb); }
  if (s == "positional_embedding") { if (int rc = need((size_t)n->ctx_len * w)) return rc; return upload_vec(host, (size_t)n->ctx_len * w, nullptr, &n->pos); }
  if (s == "ln_final.weight") { if (int rc = need(w)) return rc; return upload_vec(host, w, nullptr, &n->lnf_g); }
  if (s == "ln_final.bias") { if (int rc = need(w)) return rc; return upload_vec(host, w, nullptr, &n->lnf_b); }
  if (s == "text_projection") { if (int rc = need((size_t)w * n->E)) return rc; return upload_vec(host, (size_t)w * n->E, nullptr, &n->proj); }
  if (is_block_key(s)) return load_block(n->L, n->dtype, n->esize, w, n->heads, "maua_clip_text_load", s, host, count, false);
  return fail("maua_clip_text_load: unknown parameter name: " + s);
}

// CLIP.encode_text: tokens device int32 [N][context_length] (ids in [0, vocab_size): out-of-range ids are the caller's error - they are
// clamped, never read outside the table) -> embeds device f32 [N][embed_dim]
int maua_clip_text_encode(maua_clip_text* n, const int* tokens, int N, float* embeds) {
  MAUA_REQUIRE(n && N >= 0, "maua_clip_text_encode: bad arguments");
  if (N == 0) return MAUA_OK;
  MAUA_REQUIRE(tokens && embeds, "maua_clip_text_encode: NULL argument");
  if (!(n->tok_emb && n->pos && n->lnf_g && n->lnf_b && n->proj && blocks_loaded(n->L)))
    return fail("maua_clip_text: parameters missing (maua_clip_text_load every key of the text tower first)");
  const long chunk = text_chunk(n);
  if (int rc = ensure_text_ws(n, std::min<long>(N, chunk))) return rc;
  for (long n0 = 0; n0 < N; n0 += chunk) {
    const long nn = std::min<long>(chunk, N - n0);
    const int* tk = tokens + n0 * n->ctx_len;
    float* em = embeds + n0 * n->E;
    if (int rc = text_forward(n, tk, nn, em)) return rc;
  }
  return MAUA_OK;
}

}  // extern "C"
