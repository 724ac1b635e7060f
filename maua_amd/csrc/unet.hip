// Guided-diffusion UNet forward + DDIM step for BASELINE configs[3] ("guided-diffusion 256x256, 100-step DDIM").
//
// Replaces (reference): the model maua/diffusion/processors/guided.py:164-209 `create_models` builds (OpenAI
// guided-diffusion `UNetModel`: num_channels 256, num_res_blocks 2, attention at 32 / 16 / 8 with 64-channel heads,
// learn_sigma, resblock_updown, use_scale_shift_norm; fp16 there, bf16 operands / f32 accumulate here) and the sampler
// step `diffusion.ddim_sample(..., cond_fn=...)` that guided.py:277-339 `GuidedDiffusion.forward` loops over.  The network
// and sampler sources are the git submodule maua/submodules/guided_diffusion - EMPTY in the reference checkout, no pinned
// revision: the published architecture is restated (oracle/diffusion.py says the same), PARITY UNPINNED.
//
//   ResBlock : h = conv(resample(silu(gn(x))));  h = gn(h) * (1 + scale) + shift  [scale | shift = linear(silu(emb))];
//              out = skip(resample(x)) + conv(silu(h))          resample = avg_pool 2 / nearest x2 / identity
//   Attention: x + proj(attn(qkv(gn(x))))                        QKVAttentionLegacy, softmax in f32
//   UNet     : emb = linear(silu(linear(timestep_embedding(t)))); encoder blocks push their outputs, decoder blocks
//              read cat([h, hs.pop()]); out = conv(silu(gn(h)))
//
// MI355X design: activations NHWC in the network dtype (a 1x1 convolution is a plain row-major GEMM, GroupNorm's 32 groups
// are contiguous channel runs of a pixel); every 3x3 convolution runs on the MFMA implicit-GEMM kernels written for the
// StyleGAN2 path (LDS-direct-load kernel at >= 32-wide grids, the batch-wide split-K gather GEMM on the 16^2 / 8^2 levels,
// generic kernel elsewhere) with bias and the block's residual in the epilogue; GroupNorm + scale-shift + SiLU + the
// block's up / down resampling are ONE pass that writes the convolution's input; the decoder's channel concatenation is
// never materialised (GroupNorm and the 1x1 skip GEMM read both tensors); all ResBlocks' timestep projections are one
// batched GEMV at the top of the forward.  A forward is a fixed sequence of launches on one stream over a
// pre-planned arena (no allocation, no host sync), so maua_ddim_sample_loop (sampler.hip) can capture the whole sampler in a hipGraph.
// The fused GroupNorm pass is groupnorm.hip; the network's state and what the sampler loops use of it: unet_internal.h.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "common.h"
#include "internal.h"
#include "unet_internal.h"

using namespace maua;

namespace {

// ------------------------------------------------------------------------------------------------ small f32 kernels
// nn.py timestep_embedding: e[b] = [cos(t_b * f_i) | sin(t_b * f_i)], f_i = exp(-ln(10000) * i / half)
// (freqs: the host's float32 table when it was uploaded - the frequencies multiply timesteps up to 1000, so one ulp of
//  difference between two exp implementations would show up as 6e-5 in the embedding)
__global__ void timestep_embedding_kernel(const float* __restrict__ t, const float* __restrict__ freqs, float* __restrict__ e,
                                          int B, int dim) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  const int half = dim / 2;
  if (idx >= B * half) return;
  const int b = idx / half, i = idx - b * half;
  const float freq = freqs ? freqs[i] : expf(-logf(10000.0f) * (float)i / (float)half);
  const float arg = t[b] * freq;
  e[(long)b * dim + i] = cosf(arg);
  e[(long)b * dim + half + i] = sinf(arg);
  if ((dim & 1) && i == 0) e[(long)b * dim + dim - 1] = 0.f;
}

// y[b][n] = act_out(W[n] . act_in(x[b]) + bias[n]); one wave per output row n (W streamed once, coalesced), all B
// samples per row (8 samples per pass; W is read again for every further 8).  act: 0 none, 1 SiLU.  The timestep MLP and every ResBlock's emb_layers (all in
// f32 like the reference, whose convert_to_fp16 leaves nn.Linear alone).
__global__ __launch_bounds__(256) void linear_rows_kernel(const float* __restrict__ x, const float* __restrict__ W,
                                                          const float* __restrict__ bias, float* __restrict__ y, int B, int K,
                                                          int N, int act_in, int act_out) {
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= N) return;
  const float* wr = W + (long)n * K;
  for (int b0 = 0; b0 < B; b0 += 8) {
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; j++) acc[j] = 0.f;
    for (int k = lane; k < K; k += 64) {
      const float w = wr[k];
#pragma unroll
      for (int j = 0; j < 8; j++) {
        if (b0 + j < B) {
          float v = x[(long)(b0 + j) * K + k];
          if (act_in) v = v / (1.f + expf(-v));
          acc[j] = fmaf(w, v, acc[j]);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 8; j++) {
      float v = acc[j];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
      if (lane == 0 && b0 + j < B) {
        v += bias ? bias[n] : 0.f;
        if (act_out) v = v / (1.f + expf(-v));
        y[(long)(b0 + j) * N + n] = v;
      }
    }
  }
}

}  // namespace

namespace {

template <typename P>
int own(maua_unet* n, P** p, size_t bytes, bool zero = true) {   // a parameter buffer of n->owned, handed out as *p
  DevBuf b;
  if (int rc = b.alloc(bytes, zero)) return rc;
  *p = b.as<P>();
  n->owned.push_back(std::move(b));
  return MAUA_OK;
}

int make_gn(maua_unet* n, UGN& g, int C, const std::string& name) {
  g.C = C;
  if (int rc = own(n, &g.gamma, (size_t)C * 4)) return rc;
  if (int rc = own(n, &g.beta, (size_t)C * 4)) return rc;
  n->params[name + ".weight"] = PRef{P_GN_G, &g};
  n->params[name + ".bias"] = PRef{P_GN_B, &g};
  return MAUA_OK;
}
int make_conv(maua_unet* n, PlainConv& c, int Ci, int Co, const std::string& name) {
  if (int rc = c.alloc(Ci, Co, (Ci + 31) / 32 * 32, (Co + 31) / 32 * 32, n->esize, false)) return rc;   // (freed by maua_unet_destroy)
  n->params[name + ".weight"] = PRef{P_CONV_W, &c};
  n->params[name + ".bias"] = PRef{P_CONV_B, &c};
  return MAUA_OK;
}
int make_lin(maua_unet* n, ULin& l, int K, int N, const std::string& name) {
  l.K = K; l.N = N;
  if (int rc = own(n, &l.w, (size_t)N * K * n->esize)) return rc;
  if (int rc = own(n, &l.bias, (size_t)N * 4)) return rc;
  n->params[name + ".weight"] = PRef{P_LIN_W, &l};
  n->params[name + ".bias"] = PRef{P_LIN_B, &l};
  return MAUA_OK;
}

// UNetModel.__init__: the module tree (same walk as oracle/diffusion.py unet_structure and maua_amd/diffusion.py)
int build_structure(maua_unet* n) {
  const int mc = n->mc;
  int ch = (int)(n->mult[0] * mc);
  int rc;
  if ((rc = make_conv(n, n->conv_in, n->in_ch, ch, "input_blocks.0.0"))) return rc;
  std::vector<int> chans{ch};
  {
    UBlock b;
    b.layers.push_back({0, 0});
    b.out_ch = ch;
    n->input.push_back(b);
  }
  // (vectors of parameter structs are referenced by pointer from the name table: reserve so they never move)
  const size_t nlev = n->mult.size();
  n->res.reserve(nlev * (2 * n->nrb + 3) + 4);
  n->attn.reserve(nlev * (2 * n->nrb + 1) + 2);
  auto is_attn = [&](int ds) {
    for (int a : n->attn_ds)
      if (a == ds) return true;
    return false;
  };
  auto add_res = [&](UBlock& b, const std::string& name, int cin, int cout, int updown) -> int {
    n->res.emplace_back();
    URes& r = n->res.back();
    r.Cin = cin; r.Cout = cout; r.updown = updown; r.skip = cin != cout;
    int rc2;
    if ((rc2 = make_gn(n, r.n1, cin, name + ".in_layers.0"))) return rc2;
    if ((rc2 = make_conv(n, r.c1, cin, cout, name + ".in_layers.2"))) return rc2;
    r.emb_off = n->emb_total;
    n->emb_total += 2 * cout;
    n->params[name + ".emb_layers.1.weight"] = PRef{P_F32, &r, nullptr, (size_t)2 * cout * n->emb_dim};
    n->params[name + ".emb_layers.1.bias"] = PRef{P_F32, &r, nullptr, (size_t)2 * cout};
    if ((rc2 = make_gn(n, r.n2, cout, name + ".out_layers.0"))) return rc2;
    if ((rc2 = make_conv(n, r.c2, cout, cout, name + ".out_layers.3"))) return rc2;
    if (r.skip && (rc2 = make_lin(n, r.sk, cin, cout, name + ".skip_connection"))) return rc2;
    b.layers.push_back({1, (int)n->res.size() - 1});
    b.out_ch = cout;
    return MAUA_OK;
  };
  auto add_attn = [&](UBlock& b, const std::string& name, int c) -> int {
    n->attn.emplace_back();
    UAttn& a = n->attn.back();
    a.C = c; a.heads = c / n->head_ch;
    int rc2;
    if ((rc2 = make_gn(n, a.n, c, name + ".norm"))) return rc2;
    if ((rc2 = make_lin(n, a.qkv, c, 3 * c, name + ".qkv"))) return rc2;
    if ((rc2 = make_lin(n, a.proj, c, c, name + ".proj_out"))) return rc2;
    b.layers.push_back({2, (int)n->attn.size() - 1});
    return MAUA_OK;
  };
  int ds = 1, bi = 1;
  for (size_t level = 0; level < nlev; level++) {
    for (int i = 0; i < n->nrb; i++) {
      UBlock b;
      const std::string pfx = "input_blocks." + std::to_string(bi);
      const int co = (int)(n->mult[level] * mc);
      if ((rc = add_res(b, pfx + ".0", ch, co, 0))) return rc;
      ch = co;
      if (is_attn(ds) && (rc = add_attn(b, pfx + ".1", ch))) return rc;
      n->input.push_back(b);
      chans.push_back(ch);
      bi++;
    }
    if (level != nlev - 1) {
      UBlock b;
      if ((rc = add_res(b, "input_blocks." + std::to_string(bi) + ".0", ch, ch, 1))) return rc;
      n->input.push_back(b);
      chans.push_back(ch);
      ds *= 2;
      bi++;
    }
  }
  if ((rc = add_res(n->middle, "middle_block.0", ch, ch, 0))) return rc;
  if ((rc = add_attn(n->middle, "middle_block.1", ch))) return rc;
  if ((rc = add_res(n->middle, "middle_block.2", ch, ch, 0))) return rc;
  bi = 0;
  for (int level = (int)nlev - 1; level >= 0; level--) {
    for (int i = 0; i <= n->nrb; i++) {
      UBlock b;
      const std::string pfx = "output_blocks." + std::to_string(bi);
      const int ich = chans.back();
      chans.pop_back();
      const int co = (int)(mc * n->mult[level]);
      int li = 0;
      if ((rc = add_res(b, pfx + "." + std::to_string(li++), ch + ich, co, 0))) return rc;
      ch = co;
      if (is_attn(ds) && (rc = add_attn(b, pfx + "." + std::to_string(li++), ch))) return rc;
      if (level && i == n->nrb) {
        if ((rc = add_res(b, pfx + "." + std::to_string(li++), ch, ch, 2))) return rc;
        ds /= 2;
      }
      n->output.push_back(b);
      bi++;
    }
  }
  n->final_ch = ch;
  if ((rc = make_gn(n, n->out_norm, ch, "out.0"))) return rc;
  if ((rc = make_conv(n, n->conv_out, ch, n->out_ch, "out.2"))) return rc;
  // f32 timestep path
  const int E = n->emb_dim;
  if ((rc = own(n, &n->te0_w, (size_t)E * mc * 4))) return rc;
  if ((rc = own(n, &n->te0_b, (size_t)E * 4))) return rc;
  if ((rc = own(n, &n->te2_w, (size_t)E * E * 4))) return rc;
  if ((rc = own(n, &n->te2_b, (size_t)E * 4))) return rc;
  if ((rc = own(n, &n->embw, (size_t)n->emb_total * E * 4))) return rc;
  if ((rc = own(n, &n->embb, (size_t)n->emb_total * 4))) return rc;
  if ((rc = own(n, &n->freqs, (size_t)(mc / 2) * 4))) return rc;
  n->params["timestep_embedding.freqs"] = PRef{P_F32, nullptr, n->freqs, (size_t)(mc / 2)};
  n->params["time_embed.0.weight"] = PRef{P_F32, nullptr, n->te0_w, (size_t)E * mc};
  n->params["time_embed.0.bias"] = PRef{P_F32, nullptr, n->te0_b, (size_t)E};
  n->params["time_embed.2.weight"] = PRef{P_F32, nullptr, n->te2_w, (size_t)E * E};
  n->params["time_embed.2.bias"] = PRef{P_F32, nullptr, n->te2_b, (size_t)E};
  for (auto& kv : n->params) {
    if (kv.second.kind != P_F32 || kv.second.f32) continue;
    const URes* r = (const URes*)kv.second.obj;
    const bool is_w = kv.first.size() > 7 && kv.first.compare(kv.first.size() - 7, 7, ".weight") == 0;
    kv.second.f32 = is_w ? n->embw + (size_t)r->emb_off * E : n->embb + r->emb_off;
  }
  n->max_ch = 0;
  for (auto& r : n->res) n->max_ch = std::max(n->max_ch, std::max(r.Cin, r.Cout));
  n->max_ch = std::max(n->max_ch, 32);
  return MAUA_OK;
}

}  // namespace

// Which kernel a plain 3x3 convolution of the network runs on (see internal.h); a function of the shape and the batch only.
UnetConvRoute maua::unet_conv_route(int dtype, int route, int B, int H, int W, int Ci, int Co) {
  UnetConvRoute r{1, false, 0};
  if (route == 1) return r;
  const bool bf = dtype == MAUA_BF16;
  const bool dma_wide = bf && dma_conv_supported(dtype, Ci, Co, 1, H, W);
  const bool dma_narrow = bf && dma_conv_narrow_supported(dtype, Ci, Co, H, W);
  const bool gather = gather_conv_supported(dtype, Ci, Co, H, W) && gather_conv_workspace(dtype, B, H, W, Ci, Co) > 0;
  // enough workgroups for the chip on the LDS-direct kernel (8 x 32 pixel tiles x N tiles of 256 / 128 / Co channels)?
  const long tiles = (long)B * (H / 8) * (W / 32);
  long dma_wgs = dma_wide ? tiles * (Co % 256 == 0 ? Co / 256 : Co / 128) : tiles;
  if (dma_wide && Co % 256 == 0 && dma_wgs < 512) {  // fewer than two rounds of big tiles: 128-channel tiles, 2 per CU
    r.variant = 128;
    dma_wgs *= 2;
  }
  r.wide = dma_wide;
  if ((dma_wide || dma_narrow) && (dma_wgs >= 128 || !gather || route == 2)) r.kernel = 2;
  else if (gather && route != 2) r.kernel = 3;
  else if (dma_wide || dma_narrow) r.kernel = 2;
  if (r.kernel != 2) { r.wide = false; r.variant = 0; }
  return r;
}

namespace {

// ------------------------------------------------------------------------------------------------------ forward
template <typename T>
struct Runner {
  maua_unet* n;
  hipStream_t st;
  int B;
  bool plan;
  Arena& ar;
  float* emb_all = nullptr;  // [B][emb_total]
  // piece sums left by the LDS-direct convolution for the GroupNorm that reads its output: tensor -> (buffer, rows per sample)
  std::unordered_map<const void*, std::pair<const float*, int>> psums;
  float* gather_ws = nullptr;
  size_t gather_ws_bytes = 0;
  bool keep = false;         // record the tape and keep what the input gradient needs out of the per-layer scratch
  int g_channels = 0;        // backward: channels of the output gradient handed in (0: all of them)
  std::vector<TapeOp>* tape = nullptr;
  // gradients known so far, by forward tensor (backward pass)
  std::unordered_map<const void*, T*> grads;

  Runner(maua_unet* n_, hipStream_t s, int B_, bool plan_, bool keep_ = false) : n(n_), st(s), B(B_), plan(plan_), ar(n_->arena), keep(keep_) {}
  float* stats_alloc() { return keep ? (float*)ar.get((size_t)B * 32 * 2 * 4) : nullptr; }

  T* alloc(long px, int C) { return (T*)ar.get((size_t)px * C * sizeof(T)); }
  // room for the piece sums of a [B][H][W][C] tensor an LDS-direct convolution may produce (NULL where it cannot)
  float* psum_alloc(int H, int W, int C) {
    if (sizeof(T) != 2 || n->psum_off || H % 8 || W % 32 || C % 128) return nullptr;
    return (float*)ar.get((size_t)B * (H / 8) * (W / 32) * (C / 8) * 64);
  }

  // y = conv3x3(x) + bias (+ res); x, y, res dense NHWC [B][H][W][.]
  int conv(const PlainConv& c, const T* x, T* y, int H, int W, const T* res, float* psum = nullptr) {
    return conv(ConvView{c.Cip, c.Cop, c.wt.get(), c.bias.as<float>()}, x, y, H, W, res, psum);
  }
  struct ConvView { int Cip, Cop; const void* wt; const float* bias; };   // the forward's weights, or the input gradient's
  int conv(const ConvView& c, const T* x, T* y, int H, int W, const T* res, float* psum) {
    const size_t ws_need = gather_conv_supported(n->dtype, c.Cip, c.Cop, H, W) ? gather_conv_workspace(n->dtype, B, H, W, c.Cip, c.Cop) : 0;
    if (plan) {
      if (ws_need > gather_ws_bytes) gather_ws_bytes = ws_need;
      return MAUA_OK;
    }
    psums.erase(y);
    ConvArgs a{};
    a.x = x; a.x_bstride = (long)H * W * c.Cip; a.w = c.wt; a.s = nullptr; a.d = nullptr; a.noise = nullptr; a.bias = c.bias;
    a.y = y; a.B = B; a.H = H; a.W = W; a.Ci = c.Cip; a.Co = c.Cop; a.up = 1;
    a.act = MAUA_ACT_LINEAR; a.alpha = 1.f; a.gain = 1.f; a.clamp = -1.f;
    a.res = res; a.res_pstride = c.Cop; a.res_bstride = (long)H * W * c.Cop;
    const UnetConvRoute r = unet_conv_route(n->dtype, n->route, B, H, W, c.Cip, c.Cop);
    if (r.kernel == 2) {
      a.variant = r.variant;
      if (r.wide && psum) {   // the wide tiles can leave the statistics of what they store
        a.psum = psum;
        psums[y] = {psum, dma_psum_rows(a)};
      }
      return launch_modconv_dma(st, a);
    }
    if (r.kernel == 3) return launch_conv_gather(st, n->dtype, a, gather_ws);
    a.s = n->ones.p();
    return launch_modconv3x3(st, n->dtype, a);
  }

  // GroupNorm (+ scale-shift) (+ SiLU) (+ resample) of [x0 | x1] -> y (dense, C0 + C1 channels); xr: resampled raw x0
  int gn(const UGN& g, const T* x0, int C0, const T* x1, int C1, int H, int W, const float* ss, int silu, int mode, T* y,
         T* xr, float* stats_keep = nullptr) {
    const size_t mark = ar.top;
    float* stats = stats_keep ? stats_keep : (float*)ar.get((size_t)B * 32 * 2 * 4);
    double* part = (double*)ar.get(group_norm_workspace(B, C0 + C1, (long)H * W, (int)sizeof(T)));
    int rc = MAUA_OK;
    if (!plan) {
      const float *ps0 = nullptr, *ps1 = nullptr;
      int rows0 = 0, rows1 = 0;
      auto it0 = psums.find(x0);
      if (it0 != psums.end()) { ps0 = it0->second.first; rows0 = it0->second.second; }
      if (x1) {
        auto it1 = psums.find(x1);
        if (it1 != psums.end()) { ps1 = it1->second.first; rows1 = it1->second.second; }
      }
      GnArgs a{};
      a.x0 = x0; a.C0 = C0; a.x1 = x1; a.C1 = C1; a.B = B; a.H = H; a.W = W; a.gamma = g.gamma; a.beta = g.beta; a.ss = ss;
      a.ss_ld = n->emb_row ? 0L : (long)n->emb_total; a.silu = silu; a.mode = mode; a.y = y; a.xr = xr;
      a.ps0 = ps0; a.rows0 = rows0; a.ps1 = ps1; a.rows1 = rows1;
      rc = launch_group_norm(st, n->dtype, a, part, stats);
    }
    ar.top = mark;
    return rc;
  }

  // ResBlock on [x0 | x1] (H x W) -> out (dense, Cout channels at the resampled size)
  int resblock(const URes& r, const T* x0, int C0, const T* x1, int C1, int H, int W, T* out, float* out_psum) {
    const int Ho = r.updown == 1 ? H / 2 : (r.updown == 2 ? H * 2 : H), Wo = r.updown == 1 ? W / 2 : (r.updown == 2 ? W * 2 : W);
    const long opx = (long)B * Ho * Wo;
    // (kept forward: conv1's output and both GroupNorms' statistics outlive the block's scratch)
    T* h1_keep = keep ? alloc(opx, r.Cout) : nullptr;
    float *st1 = stats_alloc(), *st2 = stats_alloc();
    const size_t mark = ar.top;
    T* a1 = alloc(opx, r.Cin);
    T* xr = r.updown ? alloc(opx, r.Cin) : nullptr;
    int rc;
    if ((rc = gn(r.n1, x0, C0, x1, C1, H, W, nullptr, 1, r.updown, a1, xr, st1))) return rc;
    T* h1 = keep ? h1_keep : alloc(opx, r.Cout);
    float* ps1 = psum_alloc(Ho, Wo, r.Cout);
    if ((rc = conv(r.c1, a1, h1, Ho, Wo, nullptr, ps1))) return rc;
    T* a2 = alloc(opx, r.Cout);
    if ((rc = gn(r.n2, h1, r.Cout, nullptr, 0, Ho, Wo, emb_all + r.emb_off, 1, 0, a2, nullptr, st2))) return rc;
    if (keep) {
      TapeOp op{};
      op.kind = 1; op.idx = (int)(&r - n->res.data()); op.x0 = x0; op.C0 = C0; op.x1 = x1; op.C1 = C1; op.H = H; op.W = W; op.out = out;
      op.h1 = h1; op.st1 = st1; op.st2 = st2;
      tape->push_back(op);
    }
    const T* resid;
    if (r.skip) {  // 1x1 skip_connection over the (virtually concatenated) input
      T* sk = alloc(opx, r.Cout);
      if (!plan) {
        GemmArgs g{};
        g.a0 = x0; g.lda0 = C0; g.K0 = C0; g.a1 = x1; g.lda1 = C1; g.K1 = C1; g.w = r.sk.w; g.bias = r.sk.bias;
        g.c = sk; g.ldc = r.Cout; g.M = opx; g.N = r.Cout;
        if ((rc = launch_gemm_nt(st, n->dtype, g))) return rc;
      }
      resid = sk;
    } else {
      resid = r.updown ? xr : x0;  // (Cin == Cout: never a concatenated input)
    }
    if ((rc = conv(r.c2, a2, out, Ho, Wo, resid, out_psum))) return rc;
    ar.top = mark;
    return MAUA_OK;
  }

  // AttentionBlock, in place on x (dense [B][HW][C])
  int attention(const UAttn& at, T* x, int H, int W, T* out) {
    const long px = (long)B * H * W;
    T* qkv_keep = keep ? alloc(px, 3 * at.C) : nullptr;
    T* ao_keep = keep ? alloc(px, at.C) : nullptr;
    float* lse = keep ? (float*)ar.get((size_t)B * at.heads * H * W * 4) : nullptr;
    float* st1 = stats_alloc();
    const size_t mark = ar.top;
    T* a = alloc(px, at.C);
    int rc;
    if ((rc = gn(at.n, x, at.C, nullptr, 0, H, W, nullptr, 0, 0, a, nullptr, st1))) return rc;
    T* qkv = keep ? qkv_keep : alloc(px, 3 * at.C);
    T* ao = keep ? ao_keep : alloc(px, at.C);
    if (keep) {
      TapeOp op{};
      op.kind = 2; op.idx = (int)(&at - n->attn.data()); op.x0 = x; op.C0 = at.C; op.H = H; op.W = W; op.out = out; op.h1 = qkv; op.ao = ao;
      op.st1 = st1; op.lse = lse;
      tape->push_back(op);
    }
    if (!plan) {
      GemmArgs g{};
      g.a0 = a; g.lda0 = at.C; g.K0 = at.C; g.w = at.qkv.w; g.bias = at.qkv.bias; g.c = qkv; g.ldc = 3 * at.C; g.M = px;
      g.N = 3 * at.C;
      if ((rc = launch_gemm_nt(st, n->dtype, g))) return rc;
      AttnArgs aa{};
      aa.qkv = qkv; aa.out = ao; aa.B = B; aa.T = H * W; aa.heads = at.heads; aa.D = n->head_ch; aa.ld_qkv = 3 * at.C;
      aa.ld_out = at.C; aa.scale = 1.f / sqrtf((float)n->head_ch); aa.lse = lse;
      if ((rc = launch_attention(st, n->dtype, aa))) return rc;
      GemmArgs p{};
      p.a0 = ao; p.lda0 = at.C; p.K0 = at.C; p.w = at.proj.w; p.bias = at.proj.bias; p.res = x; p.ldr = at.C; p.c = out;
      p.ldc = at.C; p.M = px; p.N = at.C;
      if ((rc = launch_gemm_nt(st, n->dtype, p))) return rc;
    }
    ar.top = mark;
    return MAUA_OK;
  }

  // one TimestepEmbedSequential: layers applied to [x0 | x1]; returns the block's output tensor (allocated persistently)
  int block(const UBlock& b, const T* x0, int C0, const T* x1, int C1, int& H, int& W, T** outp) {
    const T* cur0 = x0; int c0 = C0; const T* cur1 = x1; int c1 = C1;
    T* out = nullptr;
    for (const ULayer& l : b.layers) {
      if (l.kind == 1) {
        const URes& r = n->res[l.idx];
        const int Ho = r.updown == 1 ? H / 2 : (r.updown == 2 ? H * 2 : H), Wo = r.updown == 1 ? W / 2 : (r.updown == 2 ? W * 2 : W);
        out = alloc((long)B * Ho * Wo, r.Cout);
        float* pso = psum_alloc(Ho, Wo, r.Cout);   // (lives as long as the tensor: later blocks' GroupNorms read it)
        if (int rc = resblock(r, cur0, c0, cur1, c1, H, W, out, pso)) return rc;
        H = Ho; W = Wo;
        cur0 = out; c0 = r.Cout; cur1 = nullptr; c1 = 0;
      } else {
        const UAttn& at = n->attn[l.idx];
        T* o2 = alloc((long)B * H * W, at.C);
        psums.erase(o2);
        if (int rc = attention(at, const_cast<T*>(cur0), H, W, o2)) return rc;
        out = o2;
        cur0 = out; c0 = at.C;
      }
    }
    *outp = out;
    return MAUA_OK;
  }

  int forward(const float* x_nchw, const float* t, int H, int W, float* out_nchw) {
    int rc;
    const int E = n->emb_dim, mc = n->mc;
    const long px = (long)B * H * W;
    // ---- timestep path (f32)
    float* e0 = (float*)ar.get((size_t)B * mc * 4);
    float* e1 = (float*)ar.get((size_t)B * E * 4);
    float* e2 = (float*)ar.get((size_t)B * E * 4);
    emb_all = (float*)ar.get((size_t)B * n->emb_total * 4);
    if (!plan && n->emb_row) {
      emb_all = const_cast<float*>(n->emb_row);   // (read-only; the samples' rows coincide: stride 0 below)
    } else if (!plan) {
      if ((rc = unet_emb_rows(n, st, t, B, e0, e1, e2, emb_all))) return rc;
    }
    // split-K workspace of the gather GEMM: sized in the planning pass, placed here in the real one
    gather_ws = (float*)ar.get(plan ? 0 : n_gather_bytes);
    if (keep) n->tape_gather_ws = gather_ws;
    // ---- input: NCHW f32 -> NHWC T, channels padded to 32
    T* xin = alloc(px, n->conv_in.Cip);
    if (!plan && (rc = launch_nchw_to_nhwc<float, T>(st, x_nchw, xin, B, n->in_ch, H * W, n->conv_in.Cip))) return rc;
    std::vector<T*> hs;
    std::vector<int> hs_c;
    T* h = alloc(px, n->conv_in.Cop);
    if ((rc = conv(n->conv_in, xin, h, H, W, nullptr))) return rc;   // (3 -> C input convolution: generic kernel, no piece sums)
    int ch = n->conv_in.Co, hh = H, ww = W;
    T* const h0_first = h;
    hs.push_back(h); hs_c.push_back(ch);
    for (size_t i = 1; i < n->input.size(); i++) {
      T* o;
      if ((rc = block(n->input[i], h, ch, nullptr, 0, hh, ww, &o))) return rc;
      h = o; ch = n->input[i].out_ch;
      hs.push_back(h); hs_c.push_back(ch);
    }
    {
      T* o;
      if ((rc = block(n->middle, h, ch, nullptr, 0, hh, ww, &o))) return rc;
      h = o;
    }
    for (size_t i = 0; i < n->output.size(); i++) {
      T* skip = hs.back(); const int sc = hs_c.back();
      hs.pop_back(); hs_c.pop_back();
      T* o;
      if ((rc = block(n->output[i], h, ch, skip, sc, hh, ww, &o))) return rc;
      h = o; ch = n->output[i].out_ch;
    }
    // ---- out: GroupNorm -> SiLU -> conv -> NCHW f32
    float* stf = stats_alloc();
    if (keep) {
      n->tape_h0 = (void*)h0_first; n->tape_hf = h; n->tape_cf = ch; n->tape_stf = stf; n->tape_emb = emb_all;
      n->tape_emb_ld = n->emb_row ? 0L : (long)n->emb_total;
    }
    T* a = alloc(px, ch);
    if ((rc = gn(n->out_norm, h, ch, nullptr, 0, hh, ww, nullptr, 1, 0, a, nullptr, stf))) return rc;
    T* y = alloc(px, n->conv_out.Cop);
    if ((rc = conv(n->conv_out, a, y, hh, ww, nullptr))) return rc;
    if (!plan && (rc = launch_nhwc_to_nchw<T, float>(st, y, out_nchw, B, n->out_ch, H * W, n->conv_out.Cop))) return rc;
    return MAUA_OK;
  }

  size_t n_gather_bytes = 0;

  // ------------------------------------------------------------------------------------------ input gradient (guided.py:250-272)
  // dx = conv3x3(dy) with the transposed, spatially flipped kernel (PlainConv.wt_t), no bias, optional residual
  int conv_t(const PlainConv& c, const T* dy, T* dx, int H, int W, const T* res) {
    return conv(ConvView{c.Cop, c.Cip, c.wt_t.get(), c.zero_bias.as<float>()}, dy, dx, H, W, res, nullptr);
  }
  // c [M][N] = a [M][K] w_t^T (+ res), w_t rows [n0, n0 + N) of a transposed linear weight [Kin][Nout]
  int gemm_t(const ULin& l, int n0, int N, const T* a, T* c, long M, const T* res) {
    if (plan) return MAUA_OK;
    GemmArgs g{};
    g.a0 = a; g.lda0 = l.N; g.K0 = l.N; g.w = (const char*)l.w_t + (size_t)n0 * l.N * sizeof(T); g.bias = nullptr;
    g.res = res; g.ldr = N; g.c = c; g.ldc = N; g.M = M; g.N = N;
    return launch_gemm_nt(st, n->dtype, g);
  }
  int gn_vjp(const UGN& g, const void* x0, int C0, const void* x1, int C1, int H, int W, const float* stats, const float* ss, int silu,
             int mode, const T* dy, const T* dres, const T* add0, const T* add1, T* dx0, T* dx1) {
    const size_t mark = ar.top;
    void* ws = ar.get(group_norm_vjp_workspace(B, C0 + C1, (long)H * W, (int)sizeof(T)));
    int rc = MAUA_OK;
    if (!plan) {
      GnVjpArgs a{};
      a.x0 = x0; a.C0 = C0; a.x1 = x1; a.C1 = C1; a.stats = stats; a.gamma = g.gamma; a.beta = g.beta; a.ss = ss; a.ss_ld = n->tape_emb_ld;
      a.silu = silu; a.mode = mode; a.dy = dy; a.dres = dres; a.add0 = add0; a.add1 = add1; a.dx0 = dx0; a.dx1 = dx1; a.B = B; a.H = H; a.W = W;
      rc = launch_group_norm_vjp(st, n->dtype, a, ws);
    }
    ar.top = mark;
    return rc;
  }
  // the gradient buffer of a forward tensor: the one already there (a second consumer adds to it) or a fresh one
  T* grad_of(const void* t, long px, int C, bool* had) {
    auto it = grads.find(t);
    *had = it != grads.end();
    if (*had) return it->second;
    T* g = alloc(px, C);
    grads[t] = g;
    return g;
  }

  int resblock_vjp(const TapeOp& op) {
    const URes& r = n->res[op.idx];
    const int H = op.H, W = op.W;
    const int Ho = r.updown == 1 ? H / 2 : (r.updown == 2 ? H * 2 : H), Wo = r.updown == 1 ? W / 2 : (r.updown == 2 ? W * 2 : W);
    const long ipx = (long)B * H * W, opx = (long)B * Ho * Wo;
    auto it = grads.find(op.out);
    if (it == grads.end()) return fail("maua_unet_vjp: a block's output has no gradient (tape out of order)");
    const T* dout = it->second;
    bool had0 = false, had1 = false;
    T* dx0 = grad_of(op.x0, ipx, op.C0, &had0);
    T* dx1 = op.x1 ? grad_of(op.x1, ipx, op.C1, &had1) : nullptr;
    const size_t mark = ar.top;
    int rc;
    T* d_a2 = alloc(opx, r.Cout);
    if ((rc = conv_t(r.c2, dout, d_a2, Ho, Wo, nullptr))) return rc;
    T* d_h1 = alloc(opx, r.Cout);
    if ((rc = gn_vjp(r.n2, op.h1, r.Cout, nullptr, 0, Ho, Wo, op.st2, n->tape_emb + r.emb_off, 1, 0, d_a2, nullptr, nullptr, nullptr, d_h1,
                     nullptr)))
      return rc;
    T* d_a1 = alloc(opx, r.Cin);
    if ((rc = conv_t(r.c1, d_h1, d_a1, Ho, Wo, nullptr))) return rc;
    if (r.skip) {
      // out = skip_connection([x0 | x1]) + ...: the 1x1 convolution's input gradients land in dx0 / dx1 first
      if ((rc = gemm_t(r.sk, 0, op.C0, dout, dx0, opx, had0 ? dx0 : nullptr))) return rc;
      if (op.x1 && (rc = gemm_t(r.sk, op.C0, op.C1, dout, dx1, opx, had1 ? dx1 : nullptr))) return rc;
      rc = gn_vjp(r.n1, op.x0, op.C0, op.x1, op.C1, H, W, op.st1, nullptr, 1, 0, d_a1, nullptr, dx0, dx1, dx0, dx1);
    } else {
      // identity (or resampled: x_upd) residual: through the same resampling's adjoint inside the pass
      rc = gn_vjp(r.n1, op.x0, op.C0, nullptr, 0, H, W, op.st1, nullptr, 1, r.updown, d_a1, dout, had0 ? dx0 : nullptr, nullptr, dx0, nullptr);
    }
    ar.top = mark;
    return rc;
  }

  int attention_vjp(const TapeOp& op) {
    const UAttn& at = n->attn[op.idx];
    const int H = op.H, W = op.W;
    const long px = (long)B * H * W;
    auto it = grads.find(op.out);
    if (it == grads.end()) return fail("maua_unet_vjp: a block's output has no gradient (tape out of order)");
    const T* dout = it->second;
    bool had = false;
    T* dx = grad_of(op.x0, px, at.C, &had);
    const size_t mark = ar.top;
    int rc;
    T* d_ao = alloc(px, at.C);
    if ((rc = gemm_t(at.proj, 0, at.C, dout, d_ao, px, nullptr))) return rc;
    T* d_qkv = alloc(px, 3 * at.C);
    float* delta = (float*)ar.get((size_t)B * at.heads * H * W * 4);
    if (!plan) {
      AttnVjpArgs a{};
      a.qkv = op.h1; a.out = op.ao; a.d_out = d_ao; a.lse = op.lse; a.d_qkv = d_qkv; a.delta = delta; a.B = B; a.T = H * W; a.heads = at.heads;
      a.D = n->head_ch; a.ld_qkv = 3 * at.C; a.ld_out = at.C; a.scale = 1.f / sqrtf((float)n->head_ch);
      if ((rc = launch_attention_vjp(st, n->dtype, a))) return rc;
    }
    T* d_a = alloc(px, at.C);
    if ((rc = gemm_t(at.qkv, 0, at.C, d_qkv, d_a, px, nullptr))) return rc;
    rc = gn_vjp(at.n, op.x0, at.C, nullptr, 0, H, W, op.st1, nullptr, 0, 0, d_a, dout, had ? dx : nullptr, nullptr, dx, nullptr);
    ar.top = mark;
    return rc;
  }

  // g_out [B][out_ch][H][W] f32 -> g_x [B][in_ch][H][W] f32; walks n->tape (or, planning, `ops`) backwards
  int backward(const std::vector<TapeOp>& ops, const float* g_out, int H, int W, float* g_x) {
    int rc;
    const long px = (long)B * H * W;
    T* dy = alloc(px, n->conv_out.Cop);
    if (!plan && (rc = launch_nchw_to_nhwc<float, T>(st, g_out, dy, B, g_channels ? g_channels : n->out_ch, H * W, n->conv_out.Cop))) return rc;
    T* d_a = alloc(px, n->tape_cf);
    if ((rc = conv_t(n->conv_out, dy, d_a, H, W, nullptr))) return rc;
    bool had = false;
    T* d_hf = grad_of(n->tape_hf, px, n->tape_cf, &had);
    if ((rc = gn_vjp(n->out_norm, n->tape_hf, n->tape_cf, nullptr, 0, H, W, n->tape_stf, nullptr, 1, 0, d_a, nullptr, nullptr, nullptr, d_hf,
                     nullptr)))
      return rc;
    for (size_t i = ops.size(); i-- > 0;) {
      const TapeOp& op = ops[i];
      if ((rc = op.kind == 1 ? resblock_vjp(op) : attention_vjp(op))) return rc;
    }
    auto it = grads.find(n->tape_h0);
    if (it == grads.end()) return fail("maua_unet_vjp: the input convolution's output has no gradient");
    T* d_xin = alloc(px, n->conv_in.Cip);
    if ((rc = conv_t(n->conv_in, it->second, d_xin, H, W, nullptr))) return rc;
    if (!plan && (rc = launch_nhwc_to_nchw<T, float>(st, d_xin, g_x, B, n->in_ch, H * W, n->conv_in.Cip))) return rc;
    return MAUA_OK;
  }
};
template <typename T>
int run_forward(maua_unet* n, const float* x, const float* t, int B, int H, int W, float* out, bool keep) {
  hipStream_t st = n->ctx->stream;
  const size_t key = shape_key(B, H, W) ^ (keep ? (size_t)1 << 62 : 0);
  n->tape_valid = false;
  if (key != n->planned_key) {
    // planning pass: the same walk with a counting arena (a kept forward: followed by the gradient's walk)
    n->arena.plan = true; n->arena.top = 0; n->arena.peak = 0;
    Runner<T> pr(n, st, B, true, keep);
    std::vector<TapeOp> ptape;
    pr.tape = &ptape;
    if (int rc = pr.forward(x, t, H, W, out)) return rc;
    if (keep)
      if (int rc = pr.backward(ptape, nullptr, H, W, nullptr)) return rc;
    const size_t need = n->arena.peak + pr.gather_ws_bytes + (1 << 20);
    if (need > n->arena.base.bytes()) {
      MAUA_HIP_CHECK(hipStreamSynchronize(st));
      drop_sampler_graphs(n);   // (their pointers are into the old arena: gone whether or not the new one can be had)
      if (int rc = n->arena.base.alloc(need)) return rc;
    }
    // a replan inside the same arena keeps the captured loops: each was captured under its own mode's plan (the graphs' keys hold
    // shape and mode), its offsets are baked in and stay inside [base, base + cap) - alternating an ordinary and a kept forward at
    // one shape no longer destroys and recaptures both
    n->gather_bytes = pr.gather_ws_bytes;
    n->planned_key = key;
  }
  if (int rc = n->ones.ensure(st, B, n->max_ch)) return rc;
  n->arena.plan = false; n->arena.top = 0;
  Runner<T> r(n, st, B, false, keep);
  r.n_gather_bytes = n->gather_bytes;
  n->tape.clear();
  r.tape = &n->tape;
  if (int rc = r.forward(x, t, H, W, out)) return rc;
  if (keep) { n->tape_valid = true; n->tape_B = B; n->tape_H = H; n->tape_W = W; n->tape_top = n->arena.top; }
  return MAUA_OK;
}

// the gradient's walk continues on the arena where the kept forward stopped (its tensors stay where they are)
// g_channels: channels of g_out actually handed in ([B][g_channels][H][W]; the remaining output channels' gradient is zero)
template <typename T>
int run_vjp(maua_unet* n, const float* g_out, float* g_x, int g_channels) {
  hipStream_t st = n->ctx->stream;
  n->arena.plan = false; n->arena.top = n->tape_top;
  Runner<T> r(n, st, n->tape_B, false, true);
  r.n_gather_bytes = n->gather_bytes;
  r.gather_ws = n->tape_gather_ws;
  r.g_channels = g_channels ? g_channels : n->out_ch;
  return r.backward(n->tape, g_out, n->tape_H, n->tape_W, g_x);
}

}  // namespace

// ---- what sampler.hip uses of the network (unet_internal.h)
int maua::unet_forward(maua_unet* n, const float* x, const float* t, int B, int H, int W, float* out, bool keep) {
  return dispatch_dtype<bf16_t, float>(n->dtype, "maua_unet", [&](auto e) { return run_forward<decltype(e)>(n, x, t, B, H, W, out, keep); });
}

int maua::unet_vjp(maua_unet* n, const float* g_out, float* g_x, int g_channels) {
  return dispatch_dtype<bf16_t, float>(n->dtype, "maua_unet", [&](auto e) { return run_vjp<decltype(e)>(n, g_out, g_x, g_channels); });
}

// the launchers of the two small f32 kernels: the network's timestep path and the operator-level entry points run through these
int maua::launch_timestep_embedding(hipStream_t st, const float* t, const float* freqs, int B, int dim, float* e) {
  const long work = (long)B * (dim / 2);
  MAUA_REQUIRE(work <= 0x7fffffffL - 256, "timestep_embedding: B * (dim / 2) does not fit the kernel's int index");
  hipLaunchKernelGGL(timestep_embedding_kernel, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, st, t, freqs, e, B, dim);
  MAUA_HIP_CHECK(hipGetLastError());
  return MAUA_OK;
}

int maua::launch_linear_rows(hipStream_t st, const float* x, const float* W, const float* bias, int B, int K, int N, int act_in, int act_out,
                             float* y) {
  hipLaunchKernelGGL(linear_rows_kernel, dim3((N + 3) / 4), dim3(256), 0, st, x, W, bias, y, B, K, N, act_in, act_out);
  MAUA_HIP_CHECK(hipGetLastError());
  return MAUA_OK;
}

int maua::unet_emb_rows(maua_unet* n, hipStream_t st, const float* t, int rows, float* e0, float* e1, float* e2, float* emb) {
  const int E = n->emb_dim, mc = n->mc;
  if (int rc = launch_timestep_embedding(st, t, n->freqs_loaded ? n->freqs : nullptr, rows, mc, e0)) return rc;
  if (int rc = launch_linear_rows(st, e0, n->te0_w, n->te0_b, rows, mc, E, 0, 1, e1)) return rc;
  if (int rc = launch_linear_rows(st, e1, n->te2_w, n->te2_b, rows, E, E, 0, 0, e2)) return rc;
  return launch_linear_rows(st, e2, n->embw, n->embb, rows, E, n->emb_total, 1, 0, emb);
}

bool maua::unet_planned(const maua_unet* n, int B, int H, int W) { return n->planned_key == shape_key(B, H, W) && B <= n->ones.b; }

extern "C" {

// nn.py timestep_embedding as an operator: t [B] -> e [B][dim] = [cos(t f_i) | sin(t f_i) | 0 if dim is odd], f_i = freqs[i] (a float32
// table of dim / 2 values) or, freqs NULL, computed on the device
int maua_timestep_embedding(maua_ctx* ctx, const float* t, const float* freqs, int B, int dim, float* e) {
  MAUA_REQUIRE(ctx, "maua_timestep_embedding: ctx is NULL");
  MAUA_REQUIRE(B >= 0, "maua_timestep_embedding: B is negative");
  MAUA_REQUIRE(dim >= 2, "maua_timestep_embedding: dim must be at least 2");
  if (B == 0) return MAUA_OK;
  MAUA_REQUIRE(t && e, "maua_timestep_embedding: NULL argument");
  return launch_timestep_embedding(ctx->stream, t, freqs, B, dim, e);
}

// y [B][N] = act_out(W [N][K] . act_in(x [B][K]) + bias [N]); act: 0 none, 1 SiLU; bias may be NULL
int maua_linear_rows(maua_ctx* ctx, const float* x, const float* W, const float* bias, int B, int K, int N, int act_in, int act_out, float* y) {
  MAUA_REQUIRE(ctx, "maua_linear_rows: ctx is NULL");
  MAUA_REQUIRE(B >= 0 && K >= 0 && N >= 0, "maua_linear_rows: B, K or N is negative");
  MAUA_REQUIRE((act_in == 0 || act_in == 1) && (act_out == 0 || act_out == 1), "maua_linear_rows: an activation is 0 (none) or 1 (SiLU)");
  if (B == 0 || N == 0) return MAUA_OK;
  MAUA_REQUIRE(y && (K == 0 || (x && W)), "maua_linear_rows: NULL argument");
  return launch_linear_rows(ctx->stream, x, W, bias, B, K, N, act_in, act_out, y);
}

int maua_unet_create(maua_ctx* ctx, int image_size, int in_channels, int model_channels, int out_channels, int num_res_blocks,
                     const float* channel_mult, int n_mult, const int* attention_ds, int n_attn, int num_head_channels,
                     int dtype, maua_unet** out) {
  MAUA_REQUIRE(ctx && out && channel_mult && n_mult > 0 && (attention_ds || n_attn == 0), "maua_unet_create: NULL argument");
  MAUA_REQUIRE(dtype == MAUA_F32 || dtype == MAUA_BF16, "maua_unet_create: dtype must be MAUA_F32 or MAUA_BF16");
  MAUA_REQUIRE(in_channels > 0 && in_channels <= 32 && out_channels > 0 && out_channels <= 32,
               "maua_unet_create: image channels must be 1..32");
  MAUA_REQUIRE(model_channels > 0 && model_channels % 32 == 0 && num_res_blocks > 0, "maua_unet_create: model_channels % 32");
  MAUA_REQUIRE(attention_supported(num_head_channels), "maua_unet_create: num_head_channels must be 32 or 64");
  for (int i = 0; i < n_mult; i++) {
    const int c = (int)(channel_mult[i] * model_channels);
    MAUA_REQUIRE(c > 0 && c % 32 == 0, "maua_unet_create: every level's channel count must be a multiple of 32 (GroupNorm32)");
    MAUA_REQUIRE(c % num_head_channels == 0, "maua_unet_create: channels must divide into heads");
  }
  maua_unet* n = new maua_unet();
  n->ctx = ctx; n->image_size = image_size; n->in_ch = in_channels; n->mc = model_channels; n->out_ch = out_channels;
  n->nrb = num_res_blocks; n->head_ch = num_head_channels; n->dtype = dtype; n->esize = elem_bytes(dtype);
  n->mult.assign(channel_mult, channel_mult + n_mult);
  n->attn_ds.assign(attention_ds, attention_ds + n_attn);
  n->emb_dim = 4 * model_channels;
  if (const char* e = getenv("MAUA_UNET_ROUTE")) n->route = atoi(e);
  if (int rc = build_structure(n)) {
    maua_unet_destroy(n);
    return rc;
  }
  *out = n;
  return MAUA_OK;
}

void maua_unet_destroy(maua_unet* n) {
  if (!n) return;
  hipStreamSynchronize(n->ctx->stream);
  n->smp.release();
  delete n;
}

// "route": 0 = per-shape routing of the 3x3 convolutions (LDS-direct kernel / split-K gather GEMM / generic kernel),
// 1 = every convolution on the generic kernel, 2 = never the gather GEMM (parity tests compare the routes)
int maua_unet_set_option(maua_unet* n, const char* key, int value) {
  MAUA_REQUIRE(n && key, "maua_unet_set_option: NULL argument");
  if (!strcmp(key, "psum_off")) {
    n->psum_off = value;
    n->planned_key = 0;   // (the arena layout changes)
    drop_sampler_graphs(n);
    return MAUA_OK;
  }
  if (!strcmp(key, "route")) {
    n->route = value;
    drop_sampler_graphs(n);
    return MAUA_OK;
  }
  if (!strcmp(key, "guided_fork")) {   // 1 (default): the guidance branch of maua_ddim_guided_loop beside the UNet forward; 0: behind it
    n->smp.gd_fork = value ? 1 : 0;
    drop_sampler_graphs(n);
    return MAUA_OK;
  }
  if (!strcmp(key, "vjp")) {   // 1: maua_unet_load also prepares the transposed weights maua_unet_vjp convolves / multiplies with
    MAUA_REQUIRE(value == 0 || value == 1, "maua_unet_set_option: vjp is 0 or 1");
    n->vjp = value;
    return MAUA_OK;
  }
  return fail(std::string("maua_unet_set_option: unknown option ") + key);
}

int maua_unet_param_count(maua_unet* n, long* count) {
  MAUA_REQUIRE(n && count, "maua_unet_param_count: NULL argument");
  *count = (long)n->params.size();
  return MAUA_OK;
}

// name: a key of guided-diffusion's UNetModel state dict; 3x3 conv weights [Co][Ci][3][3], 1x1 (conv1d / conv2d) weights
// [N][K][1(,1)], linear weights [N][K], GroupNorm weight / bias [C]; f32 on the host.
int maua_unet_load(maua_unet* n, const char* name, const float* host, size_t count) {
  MAUA_REQUIRE(n && name && host, "maua_unet_load: NULL argument");
  auto it = n->params.find(name);
  if (it == n->params.end()) return fail(std::string("maua_unet_load: unknown parameter name: ") + name);
  const PRef& p = it->second;
  hipStream_t st = n->ctx->stream;
  auto wrong = [&]() { return fail(std::string("maua_unet_load: ") + name + ": wrong size"); };
  switch (p.kind) {
    case P_GN_G: case P_GN_B: {
      UGN* g = (UGN*)p.obj;
      if (count != (size_t)g->C) return wrong();
      MAUA_HIP_CHECK(hipMemcpy(p.kind == P_GN_G ? g->gamma : g->beta, host, count * 4, hipMemcpyHostToDevice));
      return MAUA_OK;
    }
    case P_CONV_B: {
      PlainConv* c = (PlainConv*)p.obj;
      if (count != (size_t)c->Co) return wrong();
      return c->load_bias(st, host);
    }
    case P_LIN_B: {
      ULin* l = (ULin*)p.obj;
      if (count != (size_t)l->N) return wrong();
      MAUA_HIP_CHECK(hipMemcpy(l->bias, host, count * 4, hipMemcpyHostToDevice));
      return MAUA_OK;
    }
    case P_F32: {
      if (count != p.count) return wrong();
      MAUA_HIP_CHECK(hipMemcpy(p.f32, host, count * 4, hipMemcpyHostToDevice));
      if (p.f32 == n->freqs) n->freqs_loaded = 1;
      return MAUA_OK;
    }
    case P_CONV_W: {
      PlainConv* c = (PlainConv*)p.obj;
      if (count != (size_t)c->Co * c->Ci * 9) return wrong();
      return c->load_weight(st, n->dtype, host, n->vjp != 0);
    }
    case P_LIN_W: {
      ULin* l = (ULin*)p.obj;
      if (count != (size_t)l->N * l->K) return wrong();
      if (n->vjp && !l->w_t)
        if (int rc = own(n, &l->w_t, (size_t)l->N * l->K * n->esize)) return rc;
      // a k = 1 "convolution": [N][K] rows, converted to the network dtype (and [K][N] for the input-gradient GEMM)
      return load_weight(st, n->dtype, host, l->N, l->K, 1, l->N, l->K, l->w, n->vjp ? l->w_t : nullptr, false);
    }
  }
  return MAUA_ERR;
}

// x: device f32 [B][in_channels][H][W]; timesteps: device f32 [B] (what the wrapped model passes: the ORIGINAL timestep,
// rescaled to 0..1000); out: device f32 [B][out_channels][H][W].  H, W: multiples of 2^(levels - 1).
int maua_unet_forward(maua_unet* n, const float* x, const float* timesteps, int B, int H, int W, float* out) {
  MAUA_REQUIRE(n && x && timesteps && out, "maua_unet_forward: NULL argument");
  MAUA_REQUIRE(B >= 0 && H > 0 && W > 0, "maua_unet_forward: bad shape");
  const int down = 1 << (n->mult.size() - 1);
  MAUA_REQUIRE(H % down == 0 && W % down == 0, "maua_unet_forward: H and W must be multiples of 2^(levels - 1)");
  if (B == 0) return MAUA_OK;
  return unet_forward(n, x, timesteps, B, H, W, out, false);
}

// The forward again, keeping what its input gradient needs (GroupNorm inputs + statistics, qkv + the attention rows' log-sum-exp)
// on the arena; then maua_unet_vjp(g_out [B][out_channels][H][W]) -> g_x [B][in_channels][H][W] = (d out / d x)^T g_out, the
// vector-Jacobian product guided.py:258-272 asks autograd for (speed "regular": img = f(pred_xstart(UNet(x)))).  The pair must
// run back to back on one network (any other forward in between invalidates the kept tensors); option "vjp" = 1 before the
// weights are loaded.  Every 3x3 convolution's gradient is the same MFMA convolution with the transposed, flipped kernel.
int maua_unet_forward_keep(maua_unet* n, const float* x, const float* timesteps, int B, int H, int W, float* out) {
  MAUA_REQUIRE(n && x && timesteps && out, "maua_unet_forward_keep: NULL argument");
  MAUA_REQUIRE(n->vjp, "maua_unet_forward_keep: set option \"vjp\" = 1 before loading the weights");
  MAUA_REQUIRE(n->conv_in.wt_t && n->conv_out.wt_t, "maua_unet_forward_keep: the weights were loaded before option \"vjp\" was set");
  MAUA_REQUIRE(B > 0 && H > 0 && W > 0, "maua_unet_forward_keep: bad shape");
  const int down = 1 << (n->mult.size() - 1);
  MAUA_REQUIRE(H % down == 0 && W % down == 0, "maua_unet_forward_keep: H and W must be multiples of 2^(levels - 1)");
  return unet_forward(n, x, timesteps, B, H, W, out, true);
}

int maua_unet_vjp(maua_unet* n, const float* g_out, int B, int H, int W, float* g_x) {
  MAUA_REQUIRE(n && g_out && g_x, "maua_unet_vjp: NULL argument");
  MAUA_REQUIRE(n->tape_valid && n->tape_B == B && n->tape_H == H && n->tape_W == W,
               "maua_unet_vjp: no kept forward of this shape (call maua_unet_forward_keep first, nothing in between)");
  return unet_vjp(n, g_out, g_x, 0);
}

}  // extern "C"
