// Text-prompt guidance: the CLIP image tower forward and its gradient back to the images (this file), the residual block it shares
// with the text tower (transformer.hip, clip_text.hip), and CLIPGrads' loss around it (clip_guide.hip).
//
// Replaces (reference): maua/grad.py:96-165 `CLIPGrads` - per sampler step, `cutout_batches` times: cutouts of the current image
// estimate (cutouts.hip), `clip_model.encode_image` (OpenAI CLIP's VisionTransformer, clip/model.py - a pip dependency that is absent
// from the reference tree and this image: published architecture restated, **parity unpinned**), `spherical_dist_loss` to the target
// embeddings (maua/loss.py:22-25, pinned by g33), the weighted sum over prompts / mean over cutouts, and `torch.autograd.grad(loss, img)`.
// The library has no autograd: the gradient is the network walked backwards by hand, activations only (the perceptor's weights are
// frozen, `requires_grad_(False)`, :106).
//
//   forward   patch rows [N * G^2][kpp >= 3 p p]  --GEMM conv1-->  [N * G^2][w]  -> tokens [N][T = G^2 + 1][w] (class token, + positional
//             embedding) -> ln_pre -> L x { x += out_proj(attention(in_proj(ln_1(x))));  x += c_proj(QuickGELU(c_fc(ln_2(x)))) }
//             -> ln_post(class token) @ proj -> embedding [N][E]
//   head      per image, one workgroup, float32: ln_post, projection, F.normalize, distance 2 asin(|e - y| / 2)^2 to each target,
//             the weighted loss, and the whole way back to the class token's gradient (loss -> e -> ln_post -> x[0])
//   backward  the same chain in reverse on the transposed weights (prepared at load): every Linear's input gradient is a GEMM against
//             W^T, LayerNorm / QuickGELU have element-wise input-gradient kernels, attention the flash-style backward of
//             attention_vjp.hip (P rebuilt from the forward's log-sum-exp rows), residuals add.
//
// MI355X design.  A text-guided step is ~19 TFLOP per sample (256 cutouts x (35 forward + 37 backward) GFLOP) against 2.2 for the
// diffusion UNet, 95 % of it in eight plain GEMMs per layer with M = N * 197 ~ 200 000 rows: those run on gemm_dma.hip's LDS-direct
// 256 x 128 tiles; the in-projection's rows are permuted at load into the head-major [q | k | v] layout attention.hip reads, so the
// fused attention kernels of the diffusion UNet serve unchanged (T = 197 is masked in their last key block).  Activations are kept
// for the way back instead of recomputed (10 x [M][w] per layer: 37 GB at 1024 images - sized for 288 GB of HBM, not for 80);
// QuickGELU and its derivative ride on the GEMM epilogues (GemmArgs.epi) where the LDS-direct kernel takes the shape, and are
// separate 16-byte streaming kernels elsewhere (f32 parity mode, narrow test towers).  LayerNorm: one wave per token, values held in
// registers between the two statistics passes, float32 statistics kept for the gradient.
#include <atomic>
#include <cstring>

#include "clip_internal.h"

using namespace maua;

namespace maua {
namespace {

// tok[n][t][c] = (t == 0 ? class_embedding[c] : pe[n][t - 1][c]) + positional_embedding[t][c]
template <typename T>
__global__ __launch_bounds__(256) void tokens_kernel(const T* __restrict__ pe, const float* __restrict__ cls, const float* __restrict__ pos,
                                                     T* __restrict__ tok, long N, int Tk, int C) {
  constexpr int E = Pc<T>::N;
  const int ppr = C / E;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= N * Tk * ppr) return;
  const int pc = (int)(idx % ppr);
  const long nt = idx / ppr;
  const int t = (int)(nt % Tk);
  const long n = nt / Tk;
  float v[E];
  if (t == 0) {
#pragma unroll
    for (int e = 0; e < E; e++) v[e] = cls[pc * E + e];
  } else {
    Pc<T>::load(pe + (n * (Tk - 1) + t - 1) * C + (long)pc * E, v);
  }
#pragma unroll
  for (int e = 0; e < E; e++) v[e] += pos[(long)t * C + pc * E + e];
  Pc<T>::store(tok + nt * C + (long)pc * E, v);
}

// planar f32 images [N][3][R][R] <-> patch rows [N * G * G][ld] (k = c p p + ky p + kx < 3 p p: conv1.weight flattened); the patch
// convolution has stride = kernel, so this is a permutation and its transpose.  ld >= 3 p p: the row stride (maua_clip::kpp); the
// columns past 3 p p are not touched here (zeroed when the buffer is allocated / zeros out of the backward GEMM)
template <typename T>
__global__ __launch_bounds__(256) void im2patch_kernel(const float* __restrict__ img, T* __restrict__ rows, long N, int R, int p, int ld) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= N * 3 * R * R) return;
  const int x = (int)(idx % R), y = (int)((idx / R) % R), c = (int)((idx / ((long)R * R)) % 3);
  const long n = idx / ((long)3 * R * R);
  const int G = R / p;
  Elem<T>::store(rows + (n * G * G + (long)(y / p) * G + x / p) * ld + c * p * p + (y % p) * p + x % p, img[idx]);
}
template <typename T>
__global__ __launch_bounds__(256) void patch2im_kernel(const T* __restrict__ rows, float* __restrict__ img, long N, int R, int p, int ld) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= N * 3 * R * R) return;
  const int x = (int)(idx % R), y = (int)((idx / R) % R), c = (int)((idx / ((long)R * R)) % 3);
  const long n = idx / ((long)3 * R * R);
  const int G = R / p;
  img[idx] = Elem<T>::load(rows + (n * G * G + (long)(y / p) * G + x / p) * ld + c * p * p + (y % p) * p + x % p);
}

// ------------------------------------------------------------------------------------------------ the head (per image, float32)
struct HeadArgs {
  const void* x;            // [N][Tk][w] (T): the last block's output; row 0 of each image is read
  const float *g, *b;       // ln_post
  const float* proj;        // [w][E]
  const float* tgt;         // [S][P][E] unit vectors
  const float* twt;         // [S][P] normalised prompt weights
  const int* sel;           // [B] target set of each sample, or NULL (set 0)
  float* embed;             // [N][E] or NULL
  float* loss;              // [N] or NULL: sum_p w_p dist_p of this image
  const float* d_embed;     // [N][E] or NULL: an upstream gradient instead of the loss's (maua_clip_encode_image_vjp)
  void* dx;                 // [N][Tk][w] (T) or NULL: row 0 of each image receives the gradient (the other rows are the caller's to zero)
  int Tk, w, E, P, B;
  float coef;               // d total / d (sum_p w_p dist_p) of one image: scale / cutn / cutout_batches
  const float* mult;        // [n_cut] or NULL: how many identical cutouts each image of cutout n stands for (coef is multiplied by it)
};

template <typename T>
__global__ __launch_bounds__(256) void clip_head_kernel(HeadArgs a) {
  extern __shared__ float sm[];
  float* z = sm;               // [w] ln_post output, later d z
  float* xh = z + a.w;         // [w] normalised input
  float* e = xh + a.w;         // [E] embedding, later unit embedding
  float* de = e + a.E;         // [E]
  float* gp = de + a.E;        // [P] per-target factors
  float* red = gp + a.P;       // [4]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long n = blockIdx.x;
  const T* xr = reinterpret_cast<const T*>(a.x) + n * a.Tk * a.w;
  float s = 0.f;
  for (int c = tid; c < a.w; c += 256) { const float v = Elem<T>::load(xr + c); xh[c] = v; s += v; }
  const float mean = block_sum(s, red) / (float)a.w;
  float q = 0.f;
  for (int c = tid; c < a.w; c += 256) { const float d = xh[c] - mean; q = fmaf(d, d, q); }
  const float rstd = rsqrtf(block_sum(q, red) / (float)a.w + 1e-5f);
  for (int c = tid; c < a.w; c += 256) {
    xh[c] = (xh[c] - mean) * rstd;
    z[c] = fmaf(xh[c], a.g[c], a.b[c]);
  }
  __syncthreads();
  for (int j = tid; j < a.E; j += 256) {
    float acc = 0.f;
    for (int c = 0; c < a.w; c++) acc = fmaf(z[c], a.proj[(long)c * a.E + j], acc);
    e[j] = acc;
    if (a.embed) a.embed[n * a.E + j] = acc;
  }
  __syncthreads();
  if (!a.dx) return;
  if (a.d_embed) {
    for (int j = tid; j < a.E; j += 256) de[j] = a.d_embed[n * a.E + j];
    __syncthreads();
  } else {
    // F.normalize (eps 1e-12), distances, and d loss / d e
    float ss = 0.f;
    for (int j = tid; j < a.E; j += 256) ss = fmaf(e[j], e[j], ss);
    const float ne = fmaxf(sqrtf(block_sum(ss, red)), 1e-12f);
    for (int j = tid; j < a.E; j += 256) e[j] /= ne;
    __syncthreads();
    const int set = a.sel ? a.sel[n % a.B] : 0;
    const float* tg = a.tgt + (long)set * a.P * a.E;
    const float* tw = a.twt + (long)set * a.P;
    float lsum = 0.f;
    for (int p = wave; p < a.P; p += 4) {
      float u2 = 0.f;
      for (int j = lane; j < a.E; j += 64) { const float d = e[j] - tg[(long)p * a.E + j]; u2 = fmaf(d, d, u2); }
      u2 = wave_sum(u2);
      const float u = sqrtf(u2), hu = fminf(0.5f * u, 1.f);
      const float as = asinf(hu);
      // d/du [2 asin(u / 2)^2] = 2 asin(u / 2) / sqrt(1 - u^2 / 4); d u / d e = (e - y) / u
      const float f = u > 1e-20f ? tw[p] * 2.f * as / (sqrtf(fmaxf(1.f - hu * hu, 1e-12f)) * u) : 0.f;
      if (lane == 0) gp[p] = f;
      lsum += tw[p] * 2.f * as * as;
    }
    __syncthreads();
    float lw = (lane == 0) ? lsum : 0.f;   // (a wave's lanes hold the same partial sum over the wave's targets)
    const float ltot = block_sum(lw, red);
    if (a.loss && tid == 0) a.loss[n] = ltot;
    float gsum = 0.f;
    for (int p = 0; p < a.P; p++) gsum += gp[p];
    float dot = 0.f;
    for (int j = tid; j < a.E; j += 256) {
      float acc = 0.f;
      for (int p = 0; p < a.P; p++) acc = fmaf(gp[p], tg[(long)p * a.E + j], acc);
      const float dj = a.coef * (a.mult ? a.mult[n / a.B] : 1.f) * (e[j] * gsum - acc);   // d / d ehat
      de[j] = dj;
      dot = fmaf(dj, e[j], dot);
    }
    dot = block_sum(dot, red);
    for (int j = tid; j < a.E; j += 256) de[j] = (de[j] - e[j] * dot) / ne;   // through x / |x|
    __syncthreads();
  }
  // d z = proj de (one wave per row of proj), then ln_post backwards
  for (int c = wave; c < a.w; c += 4) {
    float acc = 0.f;
    for (int j = lane; j < a.E; j += 64) acc = fmaf(a.proj[(long)c * a.E + j], de[j], acc);
    acc = wave_sum(acc);
    if (lane == 0) z[c] = acc * a.g[c];    // g dy
  }
  __syncthreads();
  float s1 = 0.f, s2 = 0.f;
  for (int c = tid; c < a.w; c += 256) { s1 += z[c]; s2 = fmaf(z[c], xh[c], s2); }
  const float m1 = block_sum(s1, red) / (float)a.w;
  const float m2 = block_sum(s2, red) / (float)a.w;
  T* dr = reinterpret_cast<T*>(a.dx) + n * a.Tk * a.w;
  for (int c = tid; c < a.w; c += 256) Elem<T>::store(dr + c, rstd * (z[c] - m1 - xh[c] * m2));
}

__global__ __launch_bounds__(256) void zero16_kernel(u32x4* __restrict__ p, long pieces) {   // (a kernel, not a memset node: the
  const long i = (long)blockIdx.x * 256 + threadIdx.x;                                        //  guided loop is captured as a hipGraph)
  if (i < pieces) p[i] = u32x4{0u, 0u, 0u, 0u};
}

}  // namespace

int ensure_ws(maua_clip* n, long N, int keep) {
  if (N <= n->cap && keep <= n->keep) return MAUA_OK;
  MAUA_HIP_CHECK(hipStreamSynchronize(n->ctx->stream));
  N = std::max(N, n->cap);
  keep = std::max(keep, n->keep);
  n->cap = 0; n->keep = 0; n->kept_N = 0;
  n->epoch++;   // (every piece moves)
  const size_t es = n->esize, w = n->width, M = (size_t)N * n->Tk, Mp = (size_t)N * n->G * n->G;
  auto layout = [&](Scratch& s) {
    auto take = [&](size_t elems) -> void* { return s.take<char>(elems * es); };
    n->patches = take(Mp * n->kpp);
    n->pe = take(Mp * w);
    n->tok = take(M * w);
    n->x_last = take(M * w);
    n->lno = take(M * w);
    n->act = take(M * 4 * w);
    n->st_pre = s.take<float>(M * 2);
    n->embed = s.take<float>((size_t)N * n->E);
    n->loss = s.take<float>((size_t)N);
    n->dxa = keep ? take(M * w) : nullptr;
    n->dxb = keep ? take(M * w) : nullptr;
    n->dqkv = keep ? take(M * 3 * w) : nullptr;
    n->dwide = keep ? take(std::max(M * 4 * w, Mp * n->kpp)) : nullptr;   // (d act [M][4 w], later d patches [Mp][kpp])
    n->dtmp = keep ? take(M * w) : nullptr;
    n->delta = keep ? s.take<float>((size_t)N * n->heads * n->Tk) : nullptr;
    for (int i = 0; i < n->layers; i++) {   // the kept activations: per layer, or one set for all
      BlockActs& l = n->K[i];
      const bool have = keep || i == 0;
      l.x = have ? take(M * w) : nullptr;
      l.qkv = have ? take(M * 3 * w) : nullptr;
      l.ao = have ? take(M * w) : nullptr;
      l.xm = have ? take(M * w) : nullptr;
      l.h = have ? take(M * 4 * w) : nullptr;
      l.st1 = have ? s.take<float>(M * 2) : nullptr;
      l.st2 = have ? s.take<float>(M * 2) : nullptr;
      l.lse = have ? s.take<float>((size_t)N * n->heads * n->Tk) : nullptr;
    }
  };
  if (carve_into(n->ws, layout)) return fail("maua_clip: out of device memory for the image tower's activations");
  if (n->kpp != n->kp) {   // the pad columns of the patch rows: zero from here on (no writer touches them); a kernel, like zero_dx
    const long pieces = (long)(Mp * n->kpp * es / 16);
    hipLaunchKernelGGL(zero16_kernel, dim3((unsigned)((pieces + 255) / 256)), dim3(256), 0, n->ctx->stream, (u32x4*)n->patches, pieces);
    MAUA_HIP_CHECK(hipGetLastError());
    MAUA_HIP_CHECK(hipStreamSynchronize(n->ctx->stream));
  }
  n->cap = N; n->keep = keep;
  return MAUA_OK;
}

// bytes ensure_ws(N, keep = 1) allocates per image (every buffer there is a multiple of the image count)
size_t ws_bytes_per_image(const maua_clip* n) {
  const size_t es = n->esize, w = n->width, T = n->Tk, Gp = (size_t)n->G * n->G, hd = n->heads;
  size_t b = Gp * n->kpp * es + Gp * w * es + 3 * T * w * es + T * 4 * w * es + T * 8 + (size_t)n->E * 4 + 4;       // forward
  b += 3 * T * w * es + T * 3 * w * es + std::max(T * 4 * w, Gp * n->kpp) * es + hd * T * 4;                      // backward
  b += (size_t)n->layers * (10 * T * w * es + T * 16 + hd * T * 4);                                              // kept, per layer
  return b;
}

static BlockRun tower_run(const maua_clip* n, long N) {
  return BlockRun{n->ctx->stream, n->dtype, n->width, n->heads, N, n->Tk, N * n->Tk, N * n->Tk, n->ctx->gemm_dma, 0};
}

int run_forward(maua_clip* n, long N, bool keep) {
  const BlockRun r = tower_run(n, N);
  const int w = n->width, Tk = n->Tk;
  const long M = N * Tk, Mp = N * n->G * n->G;
  // patch embedding (conv1, no bias) -> tokens -> ln_pre
  if (int rc = block_gemm(r, n->patches, Mp, n->kpp, n->w_conv.get(), w, nullptr, nullptr, n->pe)) return rc;
  const long total = M * (w / elems_per_piece(n->dtype));
  const dim3 tgrid((unsigned)((total + 255) / 256));
  dispatch_dtype<bf16_t, float>(n->dtype, "maua_clip", [&](auto t) {
    hipLaunchKernelGGL(tokens_kernel<decltype(t)>, tgrid, dim3(256), 0, r.st, (const decltype(t)*)n->pe, n->cls.as<float>(), n->pos.as<float>(), (decltype(t)*)n->tok, N, Tk, w);
  });
  void* x = n->K[0].x;
  launch_layer_norm(r.st, r.dtype, n->tok, n->lnpre_g.as<float>(), n->lnpre_b.as<float>(), x, n->st_pre, M, w);
  for (int i = 0; i < n->layers; i++) {
    // without kept activations the residual stream alternates between K[0].x and x_last, ending in x_last
    void* xn = i + 1 < n->layers ? (keep ? n->K[i + 1].x : (void*)((x == n->K[0].x) ? n->x_last : n->K[0].x)) : n->x_last;
    if (int rc = block_forward(r, n->L[i], x, n->K[keep ? i : 0], n->lno, n->act, xn)) return rc;
    x = xn;
  }
  MAUA_HIP_CHECK(hipGetLastError());
  n->kept_N = keep ? N : 0;
  return MAUA_OK;
}

int run_head(maua_clip* n, long N, bool with_grad, const float* d_embed, int B, float coef, bool write_loss, const float* mult) {
  HeadArgs h{};
  h.x = n->x_last; h.g = n->lnpost_g.as<float>(); h.b = n->lnpost_b.as<float>(); h.proj = n->proj.as<float>(); h.tgt = n->tgt.as<float>(); h.twt = n->twt.as<float>();
  h.sel = n->sel_B > 0 ? n->sel.as<int>() : nullptr;
  h.embed = n->embed; h.loss = write_loss ? n->loss : nullptr; h.d_embed = d_embed; h.dx = with_grad ? n->dxa : nullptr;
  h.Tk = n->Tk; h.w = n->width; h.E = n->E; h.P = n->P; h.B = B > 0 ? B : 1; h.coef = coef; h.mult = mult;
  const size_t smem = ((size_t)2 * n->width + 2 * n->E + std::max(n->P, 1) + 8) * 4;
  MAUA_REQUIRE(smem <= 64 * 1024, "maua_clip: too many targets / too wide a tower for the head kernel's LDS");
  dispatch_dtype<bf16_t, float>(n->dtype, "maua_clip", [&](auto t) {
    hipLaunchKernelGGL(clip_head_kernel<decltype(t)>, dim3((unsigned)N), dim3(256), smem, n->ctx->stream, h);
  });
  MAUA_HIP_CHECK(hipGetLastError());
  return MAUA_OK;
}

// d x_last (in dxa: row 0 per image set by the head, the rest zero) -> d patches (in n->patches' layout, written to n->dwide)
int run_backward(maua_clip* n, long N) {
  const BlockRun r = tower_run(n, N);
  for (int i = n->layers - 1; i >= 0; i--)
    if (int rc = block_backward(r, n->L[i], n->K[i], n->dxa, n->dxb, n->dqkv, n->dwide, n->dtmp, n->delta)) return rc;
  // ln_pre backwards (dropping the class token: its inputs are parameters), then the patch embedding's transpose
  launch_layer_norm_vjp(r.st, r.dtype, n->tok, n->st_pre, n->lnpre_g.as<float>(), n->dxa, nullptr, n->dtmp, r.rows, n->width, n->Tk);
  if (int rc = block_gemm(r, n->dtmp, N * n->G * n->G, n->width, n->w_conv_t.get(), n->kpp, nullptr, nullptr, n->dwide)) return rc;
  MAUA_HIP_CHECK(hipGetLastError());
  return MAUA_OK;
}

int zero_dx(maua_clip* n, long N) {
  const long pieces = N * n->Tk * n->width * (long)n->esize / 16;
  hipLaunchKernelGGL(zero16_kernel, dim3((unsigned)((pieces + 255) / 256)), dim3(256), 0, n->ctx->stream, (u32x4*)n->dxa, pieces);
  MAUA_HIP_CHECK(hipGetLastError());
  return MAUA_OK;
}

int clip_loaded(maua_clip* n) {
  if (!(n->w_conv && n->cls && n->pos && n->lnpre_g && n->lnpre_b && n->lnpost_g && n->lnpost_b && n->proj && blocks_loaded(n->L)))
    return fail("maua_clip: parameters missing (maua_clip_load every key of the image tower first)");
  return MAUA_OK;
}

}  // namespace maua

extern "C" {

int maua_clip_create(maua_ctx* ctx, int input_resolution, int patch_size, int width, int layers, int heads, int output_dim, int dtype,
                     maua_clip** out) {
  MAUA_REQUIRE(ctx && out, "maua_clip_create: NULL argument");
  MAUA_REQUIRE(dtype == MAUA_BF16 || dtype == MAUA_F32, "maua_clip_create: dtype must be MAUA_BF16 or MAUA_F32");
  MAUA_REQUIRE(input_resolution > 0 && patch_size > 0 && input_resolution % patch_size == 0, "maua_clip_create: the input is a whole number of patches");
  MAUA_REQUIRE(width > 0 && heads > 0 && width % heads == 0 && attention_supported(width / heads), "maua_clip_create: head width must be 32 or 64");
  const int epc = elems_per_piece(dtype), kc = elems_per_chunk(dtype, 64);
  MAUA_REQUIRE(width % 32 == 0 && width % kc == 0 && width / epc <= 64 * LN_MAXP, "maua_clip_create: width must be a multiple of 32 (at most 4096 / 2048)");
  MAUA_REQUIRE(layers > 0 && output_dim > 0, "maua_clip_create: bad layer count / embedding size");
  maua_clip* n = new maua_clip();
  static std::atomic<unsigned long long> next_uid{1};
  n->uid = next_uid.fetch_add(1);
  n->ctx = ctx; n->dtype = dtype; n->esize = elem_bytes(dtype);
  n->res = input_resolution; n->patch = patch_size; n->width = width; n->layers = layers; n->heads = heads; n->E = output_dim;
  n->G = input_resolution / patch_size; n->Tk = n->G * n->G + 1; n->kp = 3 * patch_size * patch_size;
  n->kpp = (n->kp + 63) / 64 * 64;
  n->L.resize(layers);
  n->K.resize(layers);
  *out = n;
  return MAUA_OK;
}

void maua_clip_destroy(maua_clip* n) {
  if (!n) return;
  hipStreamSynchronize(n->ctx->stream);
  delete n;
}

// bytes one pass through the tower may take in a guidance call (kept activations, workspace, cutout scratch); 0: automatic
int maua_clip_set_workspace_limit(maua_clip* n, size_t bytes) {
  MAUA_REQUIRE(n, "maua_clip_set_workspace_limit: NULL argument");
  if (bytes != n->ws_limit) { n->ws_limit = bytes; n->grp = 0; }   // the next guidance call fixes the group size anew
  return MAUA_OK;
}

// name: a key of CLIP's state dict below "visual." ("conv1.weight", "class_embedding", "positional_embedding", "ln_pre.weight", ...,
// "transformer.resblocks.<i>.attn.in_proj_weight", ..., "ln_post.bias", "proj"); host float32 data in the checkpoint's layout
int maua_clip_load(maua_clip* n, const char* name, const float* host, size_t count) {
  MAUA_REQUIRE(n && name && host, "maua_clip_load: NULL argument");
  MAUA_HIP_CHECK(hipStreamSynchronize(n->ctx->stream));
  const std::string s(name);
  const int w = n->width;
  auto need = [&](size_t c) -> int {
    if (count != c) return fail("maua_clip_load: " + s + ": wrong size");
    return MAUA_OK;
  };
  if (s == "conv1.weight") {   // rows padded with zeros to kpp: [w][kpp] and its transpose [kpp][w]
    if (int rc = need((size_t)w * n->kp)) return rc;
    if (n->kpp == n->kp) return upload_matrix(n->dtype, n->esize, host, w, n->kp, nullptr, &n->w_conv, &n->w_conv_t);
    std::vector<float> padded((size_t)w * n->kpp, 0.f);
    for (int r = 0; r < w; r++) memcpy(&padded[(size_t)r * n->kpp], host + (size_t)r * n->kp, (size_t)n->kp * 4);
    return upload_matrix(n->dtype, n->esize, padded.data(), w, n->kpp, nullptr, &n->w_conv, &n->w_conv_t);
  }
  if (s == "class_embedding") { if (int rc = need(w)) return rc; return upload_vec(host, w, nullptr, &n->cls); }
  if (s == "positional_embedding") { if (int rc = need((size_t)n->Tk * w)) return rc; return upload_vec(host, (size_t)n->Tk * w, nullptr, &n->pos); }
  if (s == "ln_pre.weight") { if (int rc = need(w)) return rc; return upload_vec(host, w, nullptr, &n->lnpre_g); }
  if (s == "ln_pre.bias") { if (int rc = need(w)) return rc; return upload_vec(host, w, nullptr, &n->lnpre_b); }
  if (s == "ln_post.weight") { if (int rc = need(w)) return rc; return upload_vec(host, w, nullptr, &n->lnpost_g); }
  if (s == "ln_post.bias") { if (int rc = need(w)) return rc; return upload_vec(host, w, nullptr, &n->lnpost_b); }
  if (s == "proj") { if (int rc = need((size_t)w * n->E)) return rc; return upload_vec(host, (size_t)w * n->E, nullptr, &n->proj); }
  if (is_block_key(s)) return load_block(n->L, n->dtype, n->esize, w, n->heads, "maua_clip_load", s, host, count, true);
  return fail("maua_clip_load: unknown parameter name: " + s);
}

// VisionTransformer.forward: images [N][3][R][R] f32 (already normalised), device -> embeds [N][E] f32.  keep != 0: the activations
// stay for maua_clip_encode_image_vjp
int maua_clip_encode_image(maua_clip* n, const float* images, int N, int keep, float* embeds) {
  MAUA_REQUIRE(n && images && embeds, "maua_clip_encode_image: NULL argument");
  MAUA_REQUIRE(N >= 0 && N <= 65535, "maua_clip_encode_image: 0 .. 65535 images per call");
  if (int rc = clip_loaded(n)) return rc;
  if (N == 0) return MAUA_OK;
  if (int rc = ensure_ws(n, N, keep ? 1 : 0)) return rc;
  hipStream_t st = n->ctx->stream;
  const long total = (long)N * 3 * n->res * n->res;
  dispatch_dtype<bf16_t, float>(n->dtype, "maua_clip_encode_image", [&](auto t) {
    hipLaunchKernelGGL(im2patch_kernel<decltype(t)>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, images, (decltype(t)*)n->patches,
                       (long)N, n->res, n->patch, n->kpp);
  });
  if (int rc = run_forward(n, N, keep != 0)) return rc;
  if (int rc = run_head(n, N, false, nullptr, 1, 0.f, false)) return rc;
  MAUA_HIP_CHECK(hipMemcpyAsync(embeds, n->embed, (size_t)N * n->E * 4, hipMemcpyDeviceToDevice, st));
  return MAUA_OK;
}

// (d embeds / d images)^T d_embeds for the images of the last maua_clip_encode_image(keep = 1): [N][E] -> [N][3][R][R] f32
int maua_clip_encode_image_vjp(maua_clip* n, const float* d_embeds, int N, float* d_images) {
  MAUA_REQUIRE(n && d_embeds && d_images, "maua_clip_encode_image_vjp: NULL argument");
  MAUA_REQUIRE(N > 0 && n->kept_N == N, "maua_clip_encode_image_vjp: no kept forward of that many images (maua_clip_encode_image with keep = 1)");
  hipStream_t st = n->ctx->stream;
  if (int rc = zero_dx(n, N)) return rc;
  if (int rc = run_head(n, N, true, d_embeds, 1, 0.f, false)) return rc;
  if (int rc = run_backward(n, N)) return rc;
  const long total = (long)N * 3 * n->res * n->res;
  dispatch_dtype<bf16_t, float>(n->dtype, "maua_clip_encode_image_vjp", [&](auto t) {
    hipLaunchKernelGGL(patch2im_kernel<decltype(t)>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (const decltype(t)*)n->dwide,
                       d_images, (long)N, n->res, n->patch, n->kpp);
  });
  MAUA_HIP_CHECK(hipGetLastError());
  return MAUA_OK;
}

}  // extern "C"
