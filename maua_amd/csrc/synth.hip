// StyleGAN2 synthesis network object: parameters resident in HBM, one batched forward = a fixed sequence of
// launches on the ctx stream (styles -> [conv0(up2) -> conv1 -> toRGB+skip] x blocks -> optional u8 pack).
//
// Replaces (reference): inference/stylegan2.py:385-436 SynthesisNetwork, :275-382 SynthesisBlock,
// :195-251 SynthesisLayer, :254-272 ToRGBLayer; wrappers/stylegan2.py:85-102 (per-batch noise install).
// Activations are NHWC in the network dtype (bf16 or f32); the RGB skip image stays f32 planar.
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "common.h"
#include "internal.h"
#include "plain_conv.h"
#include "synth_internal.h"

using namespace maua;

static void prof_mark(maua_synth* n) {
  if (!n->profile || n->ev_used >= (1u << 16)) return;
  if (n->ev_used == n->ev.size()) {
    hipEvent_t e;
    if (hipEventCreate(&e) != hipSuccess) return;
    n->ev.push_back(e);
  }
  hipEventRecord(n->ev[n->ev_used++], n->ctx->stream);
}

static int channels_for(int res, int base, int maxc) { return std::min(base / res, maxc); }

// kernels a layer fits at its current grid (the forward's plan and the workspace sizing ask the same question)
static bool lowres_fits(const maua_synth* n, const ConvLayer& c) {
  return lowres_supported(n->dtype, c.Ci, c.Co, c.up, c.ih, c.iw);
}
static bool tconv_dma_fits(const maua_synth* n, const ConvLayer& c) {
  return c.up == 2 && tconv_dma_supported(n->dtype, c.Ci, c.Co, c.ih, c.iw);
}

// per-layer grids: native power-of-two sizes, scaled from the resized layer on
static void compute_dims(maua_synth* n) {
  int h = 4, w = 4;
  if (n->rs_layer == 0) { h = n->rs_th; w = n->rs_tw; }
  size_t li = 0;
  for (int blk = 0; blk < n->nblocks; blk++) {
    const int nconv = blk == 0 ? 1 : 2;
    for (int k = 0; k < nconv; k++, li++) {
      ConvLayer& c = n->convs[li];
      c.ih = h; c.iw = w;
      c.oh = h * c.up; c.ow = w * c.up;
      h = c.oh; w = c.ow;
      if (n->rs_layer == (int)li + 1) { h = n->rs_th; w = n->rs_tw; }
      c.fh = h; c.fw = w;
    }
    n->rgbs[blk].h = h; n->rgbs[blk].w = w;
  }
  n->out_h = h; n->out_w = w;
}

static void free_workspace(maua_synth* n) {
  n->wk = SynthWorkspace();
  for (auto& c : n->convs) { c.s.free(); c.d.free(); c.feat.free(); }
  for (auto& r : n->rgbs) { r.s.free(); r.wmod.free(); }
  n->kept_B = 0;   // (the kept features are gone)
}

static int ensure_workspace(maua_synth* n, int B) {
  SynthWorkspace& k = n->wk;
  if (B <= k.bcap) return MAUA_OK;
  MAUA_HIP_CHECK(hipStreamSynchronize(n->ctx->stream));
  free_workspace(n);
  size_t max_act = 0;
  for (auto& c : n->convs) {
    if (int rc = c.s.alloc((size_t)B * c.Ci * sizeof(float))) return rc;
    if (int rc = c.d.alloc((size_t)B * c.Co * sizeof(float))) return rc;
    size_t e = (size_t)c.fh * c.fw * c.Co;
    max_act = std::max(max_act, std::max(e, (size_t)c.oh * c.ow * c.Co));
    if (n->keep_features)
      if (int rc = c.feat.alloc((size_t)B * e * n->esize)) return rc;
  }
  for (auto& r : n->rgbs) {
    if (int rc = r.s.alloc((size_t)B * r.C * sizeof(float))) return rc;
    if (int rc = r.wmod.alloc((size_t)B * 3 * r.C * sizeof(float))) return rc;
  }
  // (a resized / warped layer goes through scratch buffers, also when every layer keeps its own)
  for (int i = 0; i < 2; i++)
    if (int rc = k.act[i].alloc((size_t)B * max_act * n->esize)) return rc;
  if (n->rs_layer == 0)
    if (int rc = k.const_rs.alloc((size_t)n->rs_th * n->rs_tw * n->convs[0].Ci * n->esize)) return rc;
  if (n->rs_layer >= 1) {
    const ConvLayer& hc = n->convs[n->rs_layer - 1];
    const size_t px = std::max((size_t)hc.oh * hc.ow, (size_t)n->rs_th * n->rs_tw);
    for (int i = 0; i < 2; i++)
      if (int rc = k.rgb_tmp[i].alloc((size_t)B * 3 * px * sizeof(float))) return rc;
  }
  size_t max_t = 0;
  for (auto& c : n->convs)
    if (c.up == 2) max_t = std::max(max_t, (size_t)(c.oh + 1) * (c.ow + 1) * c.Co);
  if (max_t)
    if (int rc = k.tbuf.alloc((size_t)B * max_t * n->esize)) return rc;
  size_t lx = 0, lw = 0;
  for (auto& c : n->convs)
    if (lowres_fits(n, c)) {
      size_t x1, w1;
      lowres_workspace(n->dtype, B, c.ih, c.iw, c.Ci, c.Co, c.up, &x1, &w1);
      lx = std::max(lx, x1); lw = std::max(lw, w1);
    }
  {
    int maxc = 0;
    size_t xm_elems = 0;
    for (auto& c : n->convs) {
      maxc = std::max(maxc, std::max(c.Ci, c.Co));
      // (only the up-layers whose producer has no fused toRGB need the copy: inputs up to 64^2 at 1024^2 networks;
      //  sized for any up-layer so that hooks / options can fall back to it)
      if (tconv_dma_fits(n, c)) xm_elems = std::max(xm_elems, (size_t)c.ih * c.iw * c.Ci);
    }
    if (int rc = k.ones.ensure(n->ctx->stream, B, maxc)) return rc;
    if (xm_elems)
      if (int rc = k.xm.alloc((size_t)B * xm_elems * n->esize)) return rc;
  }
  if (lx)
    if (int rc = k.lowres_xm.alloc(lx)) return rc;
  if (lw)
    if (int rc = k.lowres_ws.alloc(lw)) return rc;
  for (int i = 0; i < 2; i++)
    if (int rc = k.img[i].alloc((size_t)B * 3 * std::max(n->out_h * n->out_w, n->res * n->res) * sizeof(float))) return rc;
  // style table
  std::vector<StyleLayer> tab;
  for (auto& c : n->convs) {
    StyleLayer L{};
    L.affine_w = c.affine_w.as<float>(); L.affine_b = c.affine_b.as<float>(); L.wsq = c.wsq.as<float>(); L.wrgb = nullptr;
    L.s = c.s.as<float>(); L.d = c.d.as<float>(); L.wmod = nullptr; L.w_index = c.w_index;
    L.Cin = c.Ci; L.Co = c.Co; L.Cs = c.Ci; L.Cd = c.Co; L.scale = 1.f;
    tab.push_back(L);
  }
  for (auto& r : n->rgbs) {
    StyleLayer L{};
    L.affine_w = r.affine_w.as<float>(); L.affine_b = r.affine_b.as<float>(); L.wsq = nullptr; L.wrgb = r.wrgb.as<float>();
    L.s = r.s.as<float>(); L.d = nullptr; L.wmod = r.wmod.as<float>(); L.w_index = r.w_index;
    L.Cin = r.C; L.Co = 3; L.Cs = r.C; L.Cd = 0; L.scale = 1.f / std::sqrt((float)r.C);
    tab.push_back(L);
  }
  if (int rc = k.style_table.alloc(tab.size() * sizeof(StyleLayer))) return rc;
  MAUA_HIP_CHECK(hipMemcpy(k.style_table.get(), tab.data(), tab.size() * sizeof(StyleLayer), hipMemcpyHostToDevice));
  k.bcap = B;
  return MAUA_OK;
}

// ---- one forward: a plan (which kernel each layer takes; host only), then a launch loop that executes it

// up-layers from this input size up run as a transposed conv (tconv_up = 1).  Measured: pays off from 32^2 inputs up; below, the
// extra launch costs more than the MACs it saves (the phase kernels / the batch-wide low-resolution GEMM take those layers)
constexpr int TCONV_MIN = 32;

enum class Route : uint8_t {
  Lowres,     // <= 8x8 inputs: one batch-wide split-K GEMM (modconv_lowres.hip)
  Generic,    // modconv3x3 (up-layers: the four 3x3 phase kernels)
  DmaConv1,   // conv1 on input its producer already multiplied by the styles, LDS-direct loads (modconv_dma.hip)
  Hires,      // weights in registers (modconv_hires.hip; up-layers: the FIR-folded phase form)
  Upwalk,     // the 64 -> 32 channel up-layer on the half-folded row walk (modconv_upwalk.hip)
  FusedWalk,  // ... the whole last block as ONE walk: conv0 up -> conv1 -> toRGB + skip (-> u8)
  WalkDone,   // conv1 of that block: nothing to launch
  TconvFir,   // transposed conv + FIR + epilogue in one kernel, t stays in LDS (modconv_tconv_fir.hip)
  TconvDma,   // transposed conv: edge kernel + main block on LDS-direct loads, then the FIR / epilogue pass (t through HBM)
  Tconv2,     // transposed conv on the register-staged kernel, then the FIR / epilogue pass
};
// who multiplies a layer's input by its styles: its own kernel, the producing layer's epilogue, the producer's second store
// into the premod buffer (dual store), or a premod pass in front of the layer
enum class Src : uint8_t { Kernel, Producer, Xm, PremodPass };
enum class RgbRoute : uint8_t { Separate, Fused, Hook };  // a block's toRGB: own launch, in a conv epilogue, around a resize

struct Step {
  Route route = Route::Generic;
  Src src = Src::Kernel;
  bool scale_next = false;  // the epilogue stores the output multiplied by the next layer's styles ...
  bool dual = false;        // ... into the premod buffer, next to the plain output (dual store)
  bool rgb = false;         // the block's toRGB + skip ride on the epilogue
  bool rgb8 = false;        // ... and so does the u8 pack of the final frame
  bool skip_store = false;  // the features are not stored (nothing but the fused toRGB reads them)
};
struct Plan {
  std::vector<Step> conv;     // per conv layer
  std::vector<RgbRoute> rgb;  // per block
  bool pack = false;          // the u8 frame is packed by its own launch
};

// does a warp hook replace the output of layer k (1-based, as in maua_synth_set_warp)?
static bool layer_warped(const maua_synth* n, int k) {
  for (int s = 0; s < 3; s++)
    if (n->warp_layer[s] == k && n->warp_minv[s]) return true;
  return false;
}

// the route of a layer whose producer did not multiply its input by its styles
static Route base_route(const maua_synth* n, const ConvLayer& c) {
  const bool hires_ok = n->use_hires && hires_supported(n->dtype, c.Ci, c.Co, c.up, c.ih, c.iw);
  if (c.up == 2 && n->tconv_up) {
    // minimal up-layer: t = conv_transpose2d(x*s, W, stride 2) on the matrix cores, then FIR + epilogue.  tconv_up = 1: inputs
    // TCONV_MIN^2 .. 512^2, except where the register-stationary kernel exists (bf16 64 -> 32 channels, the 1024^2 layer): its
    // FIR-folded phase form beats tconv + upfir, whose t round trip is HBM-bound there (1.33 vs 1.56 ms at B = 32);
    // tconv_up = v > 1: every up-layer with inputs up to v
    const int hin = std::min(c.ih, c.iw), hmax = std::max(c.ih, c.iw);
    const bool dflt = n->tconv_up == 1;
    if (!(dflt && hires_ok) && hin >= (dflt ? TCONV_MIN : 1) && hmax <= (dflt ? 512 : n->tconv_up)) {
      if (!dflt || !n->tconv_dma || !tconv_dma_fits(n, c)) return Route::Tconv2;
      return n->tconv_fir > 0 && hin >= n->tconv_fir && tconv_fir_supported(n->dtype, c.Ci, c.Co, c.ih, c.iw) ? Route::TconvFir
                                                                                                           : Route::TconvDma;
    }
  }
  if (hires_ok) return Route::Hires;
  return n->lowres && lowres_fits(n, c) ? Route::Lowres : Route::Generic;
}
static bool reads_premod(Route r) { return r == Route::TconvFir || r == Route::TconvDma; }  // x must carry the styles

// Every launch of the next forward, decided from the net's state alone (shapes, dtype, options, hooks, feature capture, the
// premod buffer) and from whether the caller wants u8 frames.  No HIP calls.
// have_xm: the premod buffer exists (ensure_workspace allocates it when some up-layer fits the LDS-direct transposed convolution)
static Plan plan_forward(const maua_synth* n, bool want_u8, bool have_xm) {
  const size_t L = n->convs.size();
  Plan p;
  p.conv.resize(L);
  p.rgb.assign(n->nblocks, RgbRoute::Separate);
  p.pack = want_u8;
  for (size_t li = 0; li < L; li++) {
    const ConvLayer& c = n->convs[li];
    Step& s = p.conv[li];
    const int k = (int)li + 1;  // hook index of this layer's output
    const bool last = c.block == n->nblocks - 1;
    const bool hooked = n->rs_layer == k;
    const bool warped = layer_warped(n, k);  // a translate / zoom / rotate hook replaces the output before toRGB reads it
    const bool rs_block = n->rs_layer >= 1 && n->convs[n->rs_layer - 1].block == c.block;  // toRGB takes the hook path
    const bool fuse_rgb_ok = c.which == 1 && n->fuse_torgb && !rs_block && !warped;
    // only the next layer reads this output, unchanged (its input grid is then this layer's output grid)
    const bool private_out = !hooked && !warped && !n->keep_features && li + 1 < L;
    const bool next_replaced = n->rs_layer == k + 1 || layer_warped(n, k + 1);
    const ConvLayer* nx = private_out ? &n->convs[li + 1] : nullptr;
    s.route = base_route(n, c);
    if (c.up == 1 && s.src == Src::Producer) s.route = Route::DmaConv1;
    if (li > 0 && p.conv[li - 1].route == Route::FusedWalk) s.route = Route::WalkDone;  // (a Hires conv1)
    switch (s.route) {
      case Route::DmaConv1:
        s.rgb = fuse_rgb_ok && dma_rgb_fusable(c.Co) && c.ih % 2 == 0 && c.iw % 2 == 0;
        // the up-layer that follows takes pre-modulated input: with the block's toRGB fused here nothing else reads these
        // features, so they are stored already multiplied by its styles; (round 5) the 512-channel conv1 layers keep a separate
        // toRGB pass, which reads the PLAIN features: stored twice - plain to y, scaled into the premod buffer
        if (nx && reads_premod(base_route(n, *nx))) {
          if (s.rgb) {
            s.scale_next = true;
            p.conv[li + 1].src = Src::Producer;
          } else if (n->dual_store && have_xm && !next_replaced) {
            s.scale_next = s.dual = true;
            p.conv[li + 1].src = Src::Xm;
          }
        }
        break;
      case Route::Hires:
      case Route::WalkDone:
        if (fuse_rgb_ok) {  // conv1: the block's toRGB + skip ride on the epilogue tile, in the last block the u8 pack too
          s.rgb = true;
          s.rgb8 = last && want_u8;
          s.skip_store = last && !n->keep_features && !hooked;  // the last block's features have no other reader
        }
        // the 64 -> 32 up-layer: half the matrix work of the phase form; the last block as one walk when nothing else reads
        // its features (no hooks, no feature capture): they never reach HBM
        if (s.route == Route::Hires && c.up == 2 && n->upwalk && c.wt_h.get() &&
            upwalk_supported(n->dtype, c.Ci, c.Co, c.up, c.ih, c.iw)) {
          s.route = Route::Upwalk;
          if (n->upwalk >= 2 && last && nx && n->fuse_torgb && !rs_block && !next_replaced &&
              upwalk_fused_supported(n->dtype, c.Ci, c.Co, c.ih, c.iw)) {
            s.route = Route::FusedWalk;
            s.skip_store = true;
          }
        }
        break;
      case Route::Generic:
        s.rgb = fuse_rgb_ok && modconv_rgb_fusable(n->dtype, c.Ci, c.Co, c.up, c.ih, c.iw);
        [[fallthrough]];
      case Route::TconvFir:
      case Route::TconvDma:
      case Route::Tconv2:
        if (reads_premod(s.route) && s.src == Src::Kernel) s.src = Src::PremodPass;
        // an up-layer whose conv1 takes pre-modulated input (modconv_dma.hip) multiplies its output by that layer's styles
        if (c.up == 2 && n->dma_conv && nx && dma_conv_supported(n->dtype, nx->Ci, nx->Co, nx->up, nx->ih, nx->iw)) {
          s.scale_next = true;
          p.conv[li + 1].src = Src::Producer;
        }
        break;
      default:
        break;
    }
    if (s.rgb) p.rgb[c.block] = RgbRoute::Fused;
    if (rs_block) p.rgb[c.block] = RgbRoute::Hook;
    if (s.rgb8) p.pack = false;
  }
  return p;
}

// every synthesis layer's epilogue: lrelu 0.2, gain sqrt 2, clamp 256
static Epilogue lrelu_epilogue() { return Epilogue{MAUA_ACT_LRELU, 0.2f, std::sqrt(2.0f), 256.f}; }

extern "C" {

int maua_synth_create(maua_ctx* ctx, int img_resolution, int w_dim, int channel_base, int channel_max, int dtype,
                      int nv_compat, maua_synth** out) {
  MAUA_REQUIRE(ctx && out, "maua_synth_create: NULL argument");
  MAUA_REQUIRE(img_resolution >= 4 && (img_resolution & (img_resolution - 1)) == 0,
               "maua_synth_create: img_resolution must be a power of two >= 4");
  MAUA_REQUIRE(dtype == MAUA_F32 || dtype == MAUA_BF16 || dtype == MAUA_F16,
               "maua_synth_create: dtype must be MAUA_F32, MAUA_BF16 or MAUA_F16");
  MAUA_REQUIRE(w_dim > 0 && w_dim <= 4096, "maua_synth_create: bad w_dim");
  const int kc = elems_per_chunk(dtype, 64);
  maua_synth* n = new maua_synth();
  n->ctx = ctx; n->res = img_resolution; n->w_dim = w_dim; n->channel_base = channel_base;
  n->channel_max = channel_max; n->dtype = dtype; n->nv_compat = nv_compat;
  n->esize = elem_bytes(dtype);
  int nb = 0;
  for (int r = 4; r <= img_resolution; r *= 2) nb++;
  n->nblocks = nb;
  n->num_ws = 2 * nb;
  int widx = 0;
  for (int i = 0; i < nb; i++) {
    int r = 4 << i;
    int co = channels_for(r, channel_base, channel_max);
    if (co % 32 != 0 || co % kc != 0) {
      delete n;
      return fail("maua_synth_create: channel counts must be multiples of 32");
    }
    if (i > 0) {
      ConvLayer c{};
      c.block = i; c.which = 0; c.Ci = channels_for(r / 2, channel_base, channel_max); c.Co = co; c.res = r; c.up = 2;
      c.w_index = widx++;
      n->convs.push_back(std::move(c));
    }
    ConvLayer c{};
    c.block = i; c.which = 1; c.Ci = co; c.Co = co; c.res = r; c.up = 1; c.w_index = widx++;
    n->convs.push_back(std::move(c));
    RgbLayer g{};
    g.block = i; g.C = co; g.res = r; g.w_index = widx;  // toRGB shares the next block's first w (stylegan2.py:431-433)
    n->rgbs.push_back(std::move(g));
  }
  compute_dims(n);
  auto alloc_params = [&]() -> int {   // all zeroed
    for (auto& c : n->convs) {
      if (int rc = c.affine_w.alloc((size_t)c.Ci * w_dim * 4, true)) return rc;
      if (int rc = c.affine_b.alloc((size_t)c.Ci * 4, true)) return rc;
      if (int rc = c.bias.alloc((size_t)c.Co * 4, true)) return rc;
      if (int rc = c.noise_const.alloc((size_t)c.res * c.res * 4, true)) return rc;
      if (int rc = c.wt.alloc(prepped_weight_elems(3, c.up, c.Co, c.Ci) * n->esize, true)) return rc;
      if (c.up == 2)
        if (int rc = c.wt_t.alloc(prepped_weight_elems(3, c.up, c.Co, c.Ci) * n->esize, true)) return rc;
      // (the half-folded weights do not depend on the layer's size - it can change with a resize hook - only the routing does)
      if (upwalk_supported(n->dtype, c.Ci, c.Co, c.up, 64, 64))
        if (int rc = c.wt_h.alloc(upwalk_weight_elems(c.Co, c.Ci) * 2, true)) return rc;
      if (int rc = c.wsq.alloc((size_t)c.Co * c.Ci * 4, true)) return rc;
    }
    for (auto& g : n->rgbs) {
      if (int rc = g.affine_w.alloc((size_t)g.C * w_dim * 4, true)) return rc;
      if (int rc = g.affine_b.alloc((size_t)g.C * 4, true)) return rc;
      if (int rc = g.wrgb.alloc((size_t)3 * g.C * 4, true)) return rc;
      if (int rc = g.bias.alloc(3 * 4, true)) return rc;
    }
    return n->const_x.alloc((size_t)16 * n->convs[0].Ci * n->esize, true);
  };
  if (alloc_params()) {
    maua_synth_destroy(n);
    return fail_in("maua_synth_create");
  }
  upsample_fir16(n->fir);
  *out = n;
  return MAUA_OK;
}

void maua_synth_destroy(maua_synth* n) {
  if (!n) return;
  hipStreamSynchronize(n->ctx->stream);
  for (auto e : n->ev) hipEventDestroy(e);
  delete n;
}

int maua_synth_num_ws(const maua_synth* n) { return n ? n->num_ws : 0; }
int maua_synth_num_layers(const maua_synth* n) { return n ? (int)n->convs.size() : 0; }

int maua_synth_set_resize(maua_synth* n, int layer, int mode, int target_h, int target_w, int pad_left, int pad_right,
                          int pad_top, int pad_bottom, int pad_how, float pad_value, const float* fill_noise_host) {
  MAUA_REQUIRE(n, "maua_synth_set_resize: net is NULL");
  MAUA_REQUIRE(layer >= -1 && layer <= (int)n->convs.size(), "maua_synth_set_resize: no such layer");
  MAUA_HIP_CHECK(hipStreamSynchronize(n->ctx->stream));
  std::vector<int> before;   // every layer's noise grid (oh, ow) as it is now
  for (auto& c : n->convs) { before.push_back(c.oh); before.push_back(c.ow); }
  if (layer >= 0) {
    MAUA_REQUIRE(mode == 0 || mode == 1, "maua_synth_set_resize: mode must be 0 (stretch) or 1 (pad)");
    MAUA_REQUIRE(target_h >= 1 && target_w >= 1, "maua_synth_set_resize: empty target size");
    // native grid of the hooked tensor
    const int nat = layer == 0 ? 4 : n->convs[layer - 1].res;
    if (mode == 1) {
      // negative entries crop, as F.pad does.  The reference reaches them only through the pre-hook of layer 0
      // (wrappers/stylegan2.py:294); behind a later layer its toRGB inverse slices with negative bounds and the forward
      // fails (:313-323, the "TODO negative padding" at :278), so there is no behaviour to reproduce there.
      MAUA_REQUIRE(layer == 0 || (pad_left >= 0 && pad_right >= 0 && pad_top >= 0 && pad_bottom >= 0),
                   "maua_synth_set_resize: negative padding (cropping) is only defined at layer 0");
      MAUA_REQUIRE(-pad_left < nat && -pad_right < nat && -pad_top < nat && -pad_bottom < nat,
                   "maua_synth_set_resize: a crop must leave part of the layer");
      MAUA_REQUIRE(pad_how >= 0 && pad_how <= 3, "maua_synth_set_resize: unknown padding mode");
      MAUA_REQUIRE(target_h == nat + pad_top + pad_bottom && target_w == nat + pad_left + pad_right,
                   "maua_synth_set_resize: target size must equal the layer size plus the padding");
    }
    // the up-layers double the grid: every layer after the hook must stay even where toRGB upsamples the skip image
    n->rs_layer = layer; n->rs_mode = mode; n->rs_th = target_h; n->rs_tw = target_w;
    n->rs_pl = pad_left; n->rs_pr = pad_right; n->rs_pt = pad_top; n->rs_pb = pad_bottom;
    n->rs_how = pad_how; n->rs_value = pad_value;
  } else {
    n->rs_layer = -1;
  }
  n->rs_noise.free();
  if (layer >= 0 && fill_noise_host) {
    const int C = layer == 0 ? n->convs[0].Ci : n->convs[layer - 1].Co;
    const size_t cnt = (size_t)C * target_h * target_w;
    if (int rc = n->rs_noise.alloc(cnt * sizeof(float))) return rc;
    MAUA_HIP_CHECK(hipMemcpy(n->rs_noise.get(), fill_noise_host, cnt * sizeof(float), hipMemcpyHostToDevice));
  }
  compute_dims(n);
  free_workspace(n);
  n->kept_stale = true;
  // layers whose grid changed get a zeroed noise_const of the new size (the caller uploads fresh noise, :141-150)
  for (size_t i = 0; i < n->convs.size(); i++) {
    ConvLayer& c = n->convs[i];
    if (c.oh != before[2 * i] || c.ow != before[2 * i + 1])
      if (int rc = c.noise_const.alloc((size_t)c.oh * c.ow * sizeof(float), true)) return rc;
  }
  return MAUA_OK;
}

int maua_synth_set_warp(maua_synth* n, int slot, int layer, const float* inv_matrices_dev) {
  MAUA_REQUIRE(n, "maua_synth_set_warp: net is NULL");
  MAUA_REQUIRE(slot >= 0 && slot < 3, "maua_synth_set_warp: slot must be 0..2");
  MAUA_REQUIRE(layer >= 1 && layer <= (int)n->convs.size(), "maua_synth_set_warp: layer must name a synthesis layer (1-based index into layer_names)");
  n->warp_layer[slot] = inv_matrices_dev ? layer : -1;
  n->warp_minv[slot] = inv_matrices_dev;
  return MAUA_OK;
}

int maua_synth_layer_size(const maua_synth* n, int layer, int* h, int* w) {
  MAUA_REQUIRE(n && h && w, "maua_synth_layer_size: NULL argument");
  MAUA_REQUIRE(layer >= -1 && layer < (int)n->convs.size(), "maua_synth_layer_size: no such layer");
  if (layer < 0) { *h = n->out_h; *w = n->out_w; }
  else { *h = n->convs[layer].oh; *w = n->convs[layer].ow; }
  return MAUA_OK;
}

int maua_synth_set_option(maua_synth* n, const char* key, int value) {
  MAUA_REQUIRE(n && key, "maua_synth_set_option: NULL argument");
  if (!strcmp(key, "profile")) {
    n->profile = value;
    n->ev_used = 0;
    n->ev_fwd_start.clear();
    return MAUA_OK;
  }
  if (!strcmp(key, "keep_features")) {
    if (n->keep_features != value) {
      MAUA_HIP_CHECK(hipStreamSynchronize(n->ctx->stream));
      free_workspace(n);
      n->keep_features = value;
    }
    return MAUA_OK;
  }
  // kernel routing (read by the next forward's plan)
  static const std::pair<const char*, int maua_synth::*> routing[] = {
      {"lowres", &maua_synth::lowres},         {"use_hires", &maua_synth::use_hires}, {"upwalk", &maua_synth::upwalk},
      {"walk_segs", &maua_synth::walk_segs},   {"walk_narrow", &maua_synth::walk_narrow},
      {"fuse_torgb", &maua_synth::fuse_torgb}, {"tconv_up", &maua_synth::tconv_up},   {"tconv_fir", &maua_synth::tconv_fir},
      {"tconv_walk", &maua_synth::tconv_walk},
      {"tconv_dma", &maua_synth::tconv_dma},   {"dma_conv", &maua_synth::dma_conv},   {"dual_store", &maua_synth::dual_store}};
  for (const auto& o : routing)
    if (!strcmp(key, o.first)) {
      if (n->*o.second != value) n->kept_stale = true;
      n->*o.second = value;
      return MAUA_OK;
    }
  return fail(std::string("maua_synth_set_option: unknown option ") + key);
}

// where maua_synth_load's source lives: host memory (maua_synth_load) or this device (maua_synth_load_device, large tensors)
static thread_local hipMemcpyKind g_load_kind = hipMemcpyHostToDevice;

static int upload(float* dst, const float* host, size_t count, size_t expect, const char* name) {
  if (count != expect)
    return fail(std::string("maua_synth_load: ") + name + ": expected " + std::to_string(expect) + " values, got " +
                std::to_string(count));
  MAUA_HIP_CHECK(hipMemcpy(dst, host, count * sizeof(float), g_load_kind));
  return MAUA_OK;
}

int maua_synth_load(maua_synth* n, const char* name, const float* host, size_t count) {
  MAUA_REQUIRE(n && name && host, "maua_synth_load: NULL argument");
  std::string s(name);
  n->kept_stale = true;
  n->vjp.weights_ready = false;
  int blk = -1, pos = 0;
  if (sscanf(name, "bs.%d.%n", &blk, &pos) < 1 || blk < 0 || blk >= n->nblocks || pos == 0)
    return fail("maua_synth_load: unknown parameter name: " + s);
  std::string rest = s.substr(pos);
  hipStream_t st = n->ctx->stream;
  auto check_filter = [&]() -> int {
    if (count != 16) return fail("maua_synth_load: " + s + ": only the 4x4 [1,3,3,1] resample filter is supported");
    const float t[4] = {1, 3, 3, 1};
    for (int u = 0; u < 4; u++)
      for (int v = 0; v < 4; v++)
        if (std::fabs(host[u * 4 + v] - t[u] * t[v] / 64.f) > 1e-6f)
          return fail("maua_synth_load: " + s + ": only the 4x4 [1,3,3,1] resample filter is supported");
    return MAUA_OK;
  };
  if (rest == "resample_filter") return check_filter();
  if (rest == "const") {
    if (blk != 0) return fail("maua_synth_load: only block 0 has a const input");
    int C = n->convs[0].Ci;
    if (count != (size_t)C * 16) return fail("maua_synth_load: bs.0.const: wrong size");
    DevBuf tmp;
    if (int rc = stage(tmp, host, count, g_load_kind)) return rc;
    int rc = dispatch_dtype<bf16_t, f16_t, float>(n->dtype, "maua_synth_load",
                                                  [&](auto t) { return launch_nchw_to_nhwc<float, decltype(t)>(st, tmp.as<float>(), n->const_x.get(), 1, C, 16, C); });
    hipStreamSynchronize(st);
    return rc;
  }
  size_t dot = rest.find('.');
  if (dot == std::string::npos) return fail("maua_synth_load: unknown parameter name: " + s);
  std::string mod = rest.substr(0, dot), par = rest.substr(dot + 1);
  if (mod == "torgb") {
    RgbLayer& g = n->rgbs[blk];
    if (par == "weight") return upload(g.wrgb.as<float>(), host, count, (size_t)3 * g.C, name);
    if (par == "bias") return upload(g.bias.as<float>(), host, count, 3, name);
    if (par == "affine.weight") return upload(g.affine_w.as<float>(), host, count, (size_t)g.C * n->w_dim, name);
    if (par == "affine.bias") return upload(g.affine_b.as<float>(), host, count, g.C, name);
    return fail("maua_synth_load: unknown parameter name: " + s);
  }
  ConvLayer* c = nullptr;
  for (auto& cc : n->convs)
    if (cc.block == blk && ((mod == "conv0" && cc.which == 0) || (mod == "conv1" && cc.which == 1))) c = &cc;
  if (!c) return fail("maua_synth_load: unknown parameter name: " + s);
  if (par == "resample_filter") return check_filter();
  if (par == "bias") return upload(c->bias.as<float>(), host, count, c->Co, name);
  if (par == "affine.weight") return upload(c->affine_w.as<float>(), host, count, (size_t)c->Ci * n->w_dim, name);
  if (par == "affine.bias") return upload(c->affine_b.as<float>(), host, count, c->Ci, name);
  if (par == "noise_const") return upload(c->noise_const.as<float>(), host, count, (size_t)c->oh * c->ow, name);
  if (par == "noise_strength") {
    if (count != 1) return fail("maua_synth_load: noise_strength is a scalar");
    c->noise_strength = host[0];
    return MAUA_OK;
  }
  if (par == "weight") {
    size_t expect = (size_t)c->Co * c->Ci * 9;
    if (count != expect) return fail("maua_synth_load: " + s + ": wrong size");
    DevBuf tmp;
    if (int rc = stage(tmp, host, count, g_load_kind)) return rc;
    // F16 networks: the reference's FP16 pre-normalisation of the weight (ops.py:161-163; every convolution of the synthesis
    // network demodulates) - the styles' half is applied per batch (launch_styles)
    int rc = n->dtype == MAUA_F16 ? launch_f16_prenorm_weights(st, tmp.as<float>(), tmp.as<float>(), c->Co, c->Ci, 9) : MAUA_OK;
    if (!rc)
      rc = launch_prep_weights(st, n->dtype, tmp.as<float>(), c->wt.get(), c->wsq.as<float>(), c->Co, c->Ci, 3, c->up, (c->up == 2) ? (n->nv_compat & 1) : 0,
                               c->Co, c->Ci);
    if (!rc && c->up == 2)
      rc = launch_prep_tconv_weights(st, n->dtype, tmp.as<float>(), c->wt_t.get(), c->Co, c->Ci, n->nv_compat & 1);
    if (!rc && c->wt_h.get()) rc = launch_prep_upwalk_weights(st, tmp.as<float>(), c->wt_h.get(), c->Co, c->Ci, n->nv_compat & 1, n->dtype);
    hipStreamSynchronize(st);
    return rc;
  }
  return fail("maua_synth_load: unknown parameter name: " + s);
}

// The same from DEVICE memory (parameters drawn on the device: maua_philox_normal): large tensors are copied device to device,
// small ones (filters, scalars, <= 4096 values: the loader inspects them on the host) take a detour through a host buffer.
int maua_synth_load_device(maua_synth* n, const char* name, const float* dev, size_t count) {
  MAUA_REQUIRE(n && name && dev, "maua_synth_load_device: NULL argument");
  MAUA_HIP_CHECK(hipStreamSynchronize(n->ctx->stream));   // (the producer of `dev` ran on the context's stream)
  if (count <= 4096) {
    std::vector<float> h(count);
    MAUA_HIP_CHECK(hipMemcpy(h.data(), dev, count * 4, hipMemcpyDeviceToHost));
    return maua_synth_load(n, name, h.data(), count);
  }
  g_load_kind = hipMemcpyDeviceToDevice;
  const int rc = maua_synth_load(n, name, dev, count);
  g_load_kind = hipMemcpyHostToDevice;
  return rc;
}

int maua_synth_render_rgb8(maua_synth* n, const float* ws, const float* const* noise, const long* noise_bstride, int B,
                           float* img_out, uint8_t* rgb8_out) {
  MAUA_REQUIRE(n && ws, "maua_synth_forward: NULL argument");
  MAUA_REQUIRE(B >= 0, "maua_synth_forward: negative batch");
  // the per-sample noise factors (maua_synth_set_noise_scale) belong to THIS call: forgotten on every way out, so that a caller
  // cannot leak one batch's factors into a later forward
  struct ForgetScales { maua_synth* n; ~ForgetScales() { n->nz_scales = nullptr; n->nz_scale_stride = 0; } } forget{n};
  const bool scaled = n->nz_scales != nullptr;
  MAUA_REQUIRE(img_out || rgb8_out, "maua_synth_forward: no output buffer");
  if (B == 0) return MAUA_OK;
  if (int rc = ensure_workspace(n, B)) return rc;
  if (n->keep_features) n->kept_B = 0;   // (the kept features are being overwritten; set again when this forward is through)
  const Plan plan = plan_forward(n, rgb8_out != nullptr, (bool)n->wk.xm);
  hipStream_t st = n->ctx->stream;
  const int ntab = (int)(n->convs.size() + n->rgbs.size());
  int max_c = 0;
  for (auto& c : n->convs) max_c = std::max(max_c, std::max(c.Ci, c.Co));
  // events accumulate across forwards until maua_synth_get_profile() reads and resets them.  Slots: styles, one per conv layer
  // (two for the transposed-conv routes), toRGB per block, the u8 pack; a hook's launches land in the slot that follows
  if (n->profile) n->ev_fwd_start.push_back(n->ev_used);
  prof_mark(n);
  if (int rc = launch_styles(st, n->wk.style_table.as<StyleLayer>(), ntab, ws, n->num_ws, n->w_dim, B, max_c, n->dtype == MAUA_F16)) return rc;

  prof_mark(n);
  const void* x = n->const_x.get();
  long x_bstride = 0;
  int cur = 0;
  // the one feature-space resize (get_hook's resize(x, feat=True)): bicubic / pad + fill noise, NHWC
  auto resize_feat = [&](const void* src, long src_bstride, int nb, int H, int W, int C, void* dst) -> int {
    ResizeArgs r{};
    r.x = src; r.x_bstride = src_bstride; r.y = dst; r.B = nb; r.H = H; r.W = W; r.C = C; r.oh = n->rs_th; r.ow = n->rs_tw;
    r.mode = n->rs_mode; r.pl = n->rs_pl; r.pt = n->rs_pt; r.how = n->rs_how; r.value = n->rs_value; r.noise = n->rs_noise.as<float>();
    return launch_resize2d(st, n->dtype, true, r);
  };
  if (n->rs_layer == 0) {  // pre-hook on the first layer: its input (the learned const) is resized
    if (int rc = resize_feat(n->const_x.get(), 0, 1, 4, 4, n->convs[0].Ci, n->wk.const_rs.get())) return rc;
    x = n->wk.const_rs.get();
  }
  auto layer_noise = [&](size_t li) {
    const ConvLayer& c = n->convs[li];
    const bool given = noise && noise[li];
    NoiseOperands z;
    z.noise = given ? noise[li] : c.noise_const.as<float>();
    z.bstride = given ? (noise_bstride ? noise_bstride[li] : (long)c.oh * c.ow) : 0;
    z.strength = (n->nv_compat & 2) ? c.noise_strength : 1.f;
    // (un-normalised Loop maps: the factor 1 / (rms + eps) of each sample rides on the noise strength; only with caller-supplied maps)
    z.scale = (n->nz_scales && given) ? n->nz_scales + (long)li * n->nz_scale_stride : nullptr;
    return z;
  };
  auto layer_args = [&](auto a, size_t li, const void* in, void* out) {  // what every modulated 3x3 launch shares (ConvArgs / HiresArgs)
    const ConvLayer& c = n->convs[li];
    return maua::layer_args(a, LayerOperands{in, c.wt.get(), c.s.as<float>(), c.d.as<float>(), c.bias.as<float>(), out, B, c.ih, c.iw, c.Ci, c.Co, c.up}, layer_noise(li),
                            lrelu_epilogue());
  };
  auto pack_u8 = [&](HiresArgs& a) { pack_u8_args(a, rgb8_out, img_out == nullptr); };
  const float* prev_img = nullptr;
  int img_cur = 0;
  size_t li = 0;
  for (int blk = 0; blk < n->nblocks; blk++) {
    const int nconv = blk == 0 ? 1 : 2;
    const RgbLayer& g = n->rgbs[blk];
    float* rgb_out = (blk == n->nblocks - 1 && img_out) ? img_out : n->wk.img[img_cur].as<float>();
    auto fuse_torgb = [&](auto& a) {  // the block's toRGB + skip in the epilogue (ConvArgs / HiresArgs)
      fuse_torgb_args(a, g.wmod.as<float>(), g.bias.as<float>(), prev_img, rgb_out, 256.f, n->fir);
    };
    for (int k = 0; k < nconv; k++, li++) {
      const ConvLayer& c = n->convs[li];
      const Step& s = plan.conv[li];
      const bool hooked = n->rs_layer == (int)li + 1;  // this layer's output is resized before anything reads it
      void* y = n->keep_features && !hooked ? c.feat.get() : n->wk.act[cur].get();
      const float* next_s = s.scale_next ? n->convs[li + 1].s.as<float>() : nullptr;
      switch (s.route) {
        case Route::Lowres:
        case Route::Generic:
        case Route::DmaConv1: {
          ConvArgs a = layer_args(ConvArgs{}, li, x, y);
          a.x_bstride = x_bstride;
          a.out_scale = next_s;
          if (s.dual) a.y_scaled = n->wk.xm.get();
          if (s.rgb) fuse_torgb(a);
          if (s.route == Route::DmaConv1) a.s = nullptr;  // (the input carries the styles)
          if (int rc = s.route == Route::Lowres    ? launch_modconv_lowres(st, n->dtype, a, n->wk.lowres_xm.get(), n->wk.lowres_ws.as<float>())
                       : s.route == Route::Generic ? launch_modconv3x3(st, n->dtype, a)
                                                   : launch_modconv_dma(st, a, n->dtype))
            return rc;
          break;
        }
        case Route::Hires:
        case Route::Upwalk:
        case Route::FusedWalk: {
          HiresArgs a = layer_args(HiresArgs{}, li, x, s.skip_store ? nullptr : y);
          if (s.rgb) fuse_torgb(a);
          if (s.rgb8) pack_u8(a);
          if (s.route != Route::Hires) a.w = c.wt_h.get();  // (the half-folded weights)
          if (s.route != Route::FusedWalk) {
            if (int rc = s.route == Route::Hires ? launch_modconv_hires(st, a, n->dtype) : launch_upwalk(st, a, n->dtype)) return rc;
            break;
          }
          HiresArgs f = layer_args(HiresArgs{}, li + 1, nullptr, nullptr);  // the block's conv1 + toRGB (+ u8)
          fuse_torgb(f);
          if (plan.conv[li + 1].rgb8) pack_u8(f);
          if (int rc = launch_upwalk_fused(st, a, f, n->walk_segs, n->walk_narrow, n->dtype)) return rc;
          break;
        }
        case Route::WalkDone:
          break;
        case Route::TconvFir:
        case Route::TconvDma:
        case Route::Tconv2: {
          ConvArgs a = tconv_args(x, x_bstride, c.wt_t.get(), c.s.as<float>(), n->wk.tbuf.get(), B, c.ih, c.iw, c.Ci, c.Co);
          UpfirArgs u = upfir_args(y, c.d.as<float>(), c.bias.as<float>(), next_s, B, c.ih, c.iw, c.Co, layer_noise(li), lrelu_epilogue());
          if (s.src == Src::PremodPass)  // (the input is small: inputs up to 64^2 at 1024^2 networks)
            if (int rc = launch_premod_nhwc(st, x, x_bstride, c.s.as<float>(), n->wk.xm.get(), B, (long)c.ih * c.iw, c.Ci, n->dtype)) return rc;
          if (s.src == Src::PremodPass || s.src == Src::Xm) {
            a.x = n->wk.xm.get();
            a.x_bstride = (long)c.ih * c.iw * c.Ci;
          }
          if (reads_premod(s.route)) a.s = n->wk.ones.p();
          if (s.route == Route::TconvFir) {  // the whole layer in one kernel: t never leaves LDS (bit-identical output)
            if (int rc = launch_tconv_fir(st, a, u, n->dtype, n->tconv_walk, 0)) return rc;
            prof_mark(n);  // (two profile slots like the two-launch path: the second measures ~0)
            break;
          }
          if (s.route == Route::TconvDma) {
            // the thin edges first (3 of 9 weight blocks, no tile waste), the main block behind them; running the edges on a
            // side stream beside the main block measured no different: 8.06 vs 8.08 ms per forward
            if (int rc = launch_tconv_edges(st, a, n->dtype)) return rc;
            if (int rc = launch_tconv_dma(st, a, n->dtype)) return rc;
          } else if (int rc = launch_tconv2(st, n->dtype, a)) {
            return rc;
          }
          prof_mark(n);  // (profile mode: this up-layer occupies two slots)
          u.t = n->wk.tbuf.get();
          if (int rc = launch_upfir_epilogue(st, n->dtype, u)) return rc;
          break;
        }
      }
      prof_mark(n);
      x = y;
      x_bstride = (long)c.oh * c.ow * c.Co;
      cur ^= 1;
      if (hooked) {  // forward hook: resize(output, feat=True)
        void* dst = n->keep_features ? c.feat.get() : n->wk.act[cur].get();
        if (int rc = resize_feat(x, x_bstride, B, c.oh, c.ow, c.Co, dst)) return rc;
        x = dst;
        x_bstride = (long)c.fh * c.fw * c.Co;
        cur ^= 1;
      }
      for (int wsl = 0; wsl < 3; wsl++) {  // translate / zoom / rotate hooks on this layer (registered after the
        if (n->warp_layer[wsl] != (int)li + 1 || !n->warp_minv[wsl]) continue;  // resize hook, so they run after it)
        void* dst = n->wk.act[cur].get();
        if (dst == x) dst = n->wk.act[cur ^ 1].get();
        if (int rc = launch_warp_affine_nhwc(st, n->dtype, x, dst, n->warp_minv[wsl], B, c.fh, c.fw, c.Co)) return rc;
        if (n->keep_features) {  // the hook's output replaces the layer's
          MAUA_HIP_CHECK(hipMemcpyAsync(c.feat.get(), dst, (size_t)B * c.fh * c.fw * c.Co * n->esize, hipMemcpyDeviceToDevice, st));
        } else {
          x = dst;
          cur = (dst == n->wk.act[0].get()) ? 1 : 0;
        }
      }
    }
    if (plan.rgb[blk] != RgbRoute::Fused) {
      // around the resized block, the reference's rgb_hook / img_hook (get_hook :325-338): toRGB runs on the resized
      // features, its output goes back to the layer's native grid (bicubic back / crop), joins the skip image there,
      // and the block's image is resized forward again (no fill noise on images)
      const bool hook = plan.rgb[blk] == RgbRoute::Hook;
      RgbArgs r{};
      r.x = x; r.wmod = g.wmod.as<float>(); r.bias = g.bias.as<float>(); r.prev = hook ? nullptr : prev_img;
      r.out = hook ? n->wk.rgb_tmp[0].as<float>() : rgb_out; r.B = B; r.H = g.h; r.W = g.w; r.C = g.C; r.clamp = 256.f;
      memcpy(r.fir, n->fir, sizeof(r.fir));
      if (int rc = launch_torgb(st, n->dtype, r)) return rc;
      if (hook) {
        const ConvLayer& hc = n->convs[n->rs_layer - 1];
        const int nh = hc.oh, nw = hc.ow;  // native grid of the block
        ResizeArgs inv{};
        inv.x = n->wk.rgb_tmp[0].as<float>(); inv.x_bstride = 3L * g.h * g.w; inv.y = n->wk.rgb_tmp[1].as<float>(); inv.B = B; inv.H = g.h; inv.W = g.w;
        inv.C = 3; inv.oh = nh; inv.ow = nw; inv.mode = n->rs_mode; inv.pl = -n->rs_pl; inv.pt = -n->rs_pt;
        inv.how = MAUA_PAD_CONSTANT; inv.value = 0.f; inv.noise = nullptr;
        if (int rc = launch_resize2d(st, MAUA_F32, false, inv)) return rc;
        const float* native = n->wk.rgb_tmp[1].as<float>();
        if (prev_img) {
          if (int rc = launch_skip_add(st, n->wk.rgb_tmp[1].as<float>(), prev_img, n->wk.rgb_tmp[0].as<float>(), B, nh, nw, n->fir)) return rc;
          native = n->wk.rgb_tmp[0].as<float>();
        }
        ResizeArgs fwd{};
        fwd.x = native; fwd.x_bstride = 3L * nh * nw; fwd.y = rgb_out; fwd.B = B; fwd.H = nh; fwd.W = nw; fwd.C = 3;
        fwd.oh = g.h; fwd.ow = g.w; fwd.mode = n->rs_mode; fwd.pl = n->rs_pl; fwd.pt = n->rs_pt; fwd.how = n->rs_how;
        fwd.value = n->rs_value; fwd.noise = nullptr;
        if (int rc = launch_resize2d(st, MAUA_F32, false, fwd)) return rc;
      }
    }
    prof_mark(n);  // zero-length when fused into conv1
    prev_img = rgb_out;
    img_cur ^= 1;
  }
  if (rgb8_out) {
    if (plan.pack)
      if (int rc = launch_pack_rgb8(st, prev_img, rgb8_out, B, n->out_h, n->out_w)) return rc;
    prof_mark(n);  // zero-length when the last block's epilogue packed the frame
  }
  if (n->keep_features) {   // what maua_synth_vjp may differentiate
    n->kept_B = B;
    n->kept_scaled = scaled;
    n->kept_stale = false;
  }
  return MAUA_OK;
}

// the plan of the next forward as plain ints (host only, no launch): what a test pins so that a threshold edit shows up as a diff
int maua_synth_get_plan(maua_synth* n, int want_u8, int* conv_out, int capacity, int* rgb_out, int* pack, int* n_layers) {
  MAUA_REQUIRE(n && n_layers, "maua_synth_get_plan: NULL argument");
  bool have_xm = (bool)n->wk.xm;
  if (!n->wk.bcap)   // no workspace yet: what ensure_workspace will decide
    for (auto& c : n->convs) have_xm = have_xm || tconv_dma_fits(n, c);
  const Plan p = plan_forward(n, want_u8 != 0, have_xm);
  *n_layers = (int)p.conv.size();
  if (conv_out) {
    MAUA_REQUIRE(capacity >= (int)p.conv.size(), "maua_synth_get_plan: capacity too small");
    for (size_t i = 0; i < p.conv.size(); i++) {
      const Step& s = p.conv[i];
      const int v[7] = {(int)s.route, (int)s.src, s.scale_next, s.dual, s.rgb, s.rgb8, s.skip_store};
      memcpy(conv_out + 7 * i, v, sizeof(v));
    }
  }
  if (rgb_out)
    for (int b = 0; b < n->nblocks; b++) rgb_out[b] = (int)p.rgb[b];
  if (pack) *pack = p.pack;
  return MAUA_OK;
}

int maua_synth_set_noise_scale(maua_synth* n, const float* scales, long layer_stride) {
  MAUA_REQUIRE(n, "maua_synth_set_noise_scale: NULL argument");
  MAUA_REQUIRE(!scales || layer_stride > 0, "maua_synth_set_noise_scale: layer_stride must be positive");
  n->nz_scales = scales;
  n->nz_scale_stride = layer_stride;
  return MAUA_OK;
}

int maua_synth_get_profile(maua_synth* n, float* ms_out, int capacity, int* count) {
  MAUA_REQUIRE(n && count, "maua_synth_get_profile: NULL argument");
  // one duration per launch; the "begin" marker of every recorded forward is skipped
  int k = 0;
  if (n->ev_used > 0) MAUA_HIP_CHECK(hipEventSynchronize(n->ev[n->ev_used - 1]));
  for (size_t f = 0; f < n->ev_fwd_start.size(); f++) {
    size_t lo = n->ev_fwd_start[f], hi = (f + 1 < n->ev_fwd_start.size()) ? n->ev_fwd_start[f + 1] : n->ev_used;
    for (size_t i = lo; i + 1 < hi; i++, k++)
      if (ms_out && k < capacity) MAUA_HIP_CHECK(hipEventElapsedTime(&ms_out[k], n->ev[i], n->ev[i + 1]));
  }
  *count = k;
  if (ms_out) {  // reading resets the recording
    n->ev_used = 0;
    n->ev_fwd_start.clear();
  }
  return MAUA_OK;
}

int maua_synth_forward(maua_synth* n, const float* ws, const float* const* noise, const long* noise_bstride, int B,
                       float* img_out) {
  MAUA_REQUIRE(img_out, "maua_synth_forward: img_out is NULL");
  return maua_synth_render_rgb8(n, ws, noise, noise_bstride, B, img_out, nullptr);
}

int maua_synth_get_feature(maua_synth* n, int layer, int B, float* out_nchw) {
  MAUA_REQUIRE(n && out_nchw, "maua_synth_get_feature: NULL argument");
  MAUA_REQUIRE(n->keep_features, "maua_synth_get_feature: enable with maua_synth_set_option(net, \"keep_features\", 1)");
  MAUA_REQUIRE(layer >= 0 && layer < (int)n->convs.size(), "maua_synth_get_feature: no such layer");
  MAUA_REQUIRE(B <= n->wk.bcap, "maua_synth_get_feature: batch larger than the last forward");
  ConvLayer& c = n->convs[layer];
  hipStream_t st = n->ctx->stream;
  return dispatch_dtype<bf16_t, f16_t, float>(n->dtype, "maua_synth_get_feature", [&](auto t) {
    return launch_nhwc_to_nchw<decltype(t), float>(st, c.feat.get(), out_nchw, B, c.Co, c.fh * c.fw, c.Co);
  });
}

}  // extern "C"
