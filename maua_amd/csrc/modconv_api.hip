// Kernel-selection switches of the modulated 3x3 convolutions (maua_modconv_route, maua_modconv_ex, maua_torgb_ex): one layer of the
// StyleGAN2 synthesis network described the way synth.hip's forward describes it, run on the route of the caller's choice with styles
// and demodulation coefficients the caller chose.  For parity tests; no reference counterpart.
#include <algorithm>
#include <cstring>

#include "common.h"
#include "internal.h"
#include "plain_conv.h"

namespace maua {
namespace {

// synth.hip's Route enum, in its order; UPFIR: the FIR / epilogue pass of the transposed-convolution routes alone
enum { R_LOWRES = 0, R_GENERIC, R_DMA, R_HIRES, R_UPWALK, R_FUSED, R_WALKDONE, R_TFIR, R_TDMA, R_T2, R_UPFIR };

bool is_tconv(int r) { return r == R_TFIR || r == R_TDMA || r == R_T2; }
bool reads_premod(int r) { return r == R_TFIR || r == R_TDMA || r == R_DMA; }   // the route's kernel takes x * s

// the descriptor's operands in the form the shared argument helpers (internal.h) take them
LayerOperands operands(const maua_modconv_desc* d) {
  return LayerOperands{d->x, nullptr, d->s, d->d, d->bias, d->y, d->B, d->H, d->W, d->Ci, d->Co, d->up};
}
NoiseOperands noise_of(const maua_modconv_desc* d) { return NoiseOperands{d->noise, d->noise_bstride, d->noise_strength, d->noise_scale}; }
Epilogue epilogue_of(const maua_modconv_desc* d) { return Epilogue{d->act, d->alpha, d->gain, d->clamp}; }

template <typename A>
A desc_args(const maua_modconv_desc* d) {
  A a = layer_args(A{}, operands(d), noise_of(d), epilogue_of(d));
  if (d->rgb_out) {
    float fir[16];
    upsample_fir16(fir);
    fuse_torgb_args(a, d->rgb_wmod, d->rgb_bias, d->rgb_prev, d->rgb_out, d->rgb_clamp, fir);
  }
  return a;
}
ConvArgs conv_args(const maua_modconv_desc* d) {   // as the forward's Lowres / Generic / DmaConv1 case
  ConvArgs a = desc_args<ConvArgs>(d);
  a.x_bstride = d->x_bstride; a.out_scale = d->out_scale; a.y_scaled = d->y_scaled;
  return a;
}
HiresArgs hires_args(const maua_modconv_desc* d) {  // as its Hires / Upwalk / FusedWalk case
  HiresArgs a = desc_args<HiresArgs>(d);
  if (d->rgb8_out || d->rgb_skip_f32) pack_u8_args(a, d->rgb8_out, d->rgb_skip_f32 != 0);
  return a;
}
ConvArgs tconv_args(const maua_modconv_desc* d) {   // (w / t are set by the caller)
  return maua::tconv_args(d->x, d->x_bstride, nullptr, d->s, nullptr, d->B, d->H, d->W, d->Ci, d->Co);
}
UpfirArgs upfir_args(const maua_modconv_desc* d) {
  return maua::upfir_args(d->y, d->d, d->bias, d->out_scale, d->B, d->H, d->W, d->Co, noise_of(d), epilogue_of(d));
}

// Every refusal of the route's launchers, raised before anything is launched; *tile gets the launcher's own tile / slice choice.
int modconv_plan(const maua_modconv_desc* d, const maua_modconv_desc* d1, int dtype, int route, int* tile) {
  MAUA_REQUIRE(dtype == MAUA_F32 || dtype == MAUA_BF16 || dtype == MAUA_F16, "maua_modconv: unsupported dtype");
  MAUA_REQUIRE(route >= R_LOWRES && route <= R_UPFIR && route != R_WALKDONE, "maua_modconv: no such route");
  MAUA_REQUIRE(d->B >= 0 && d->H > 0 && d->W > 0 && d->Ci > 0 && d->Co > 0, "maua_modconv: bad shape");
  MAUA_REQUIRE(d->x && (d->w || route == R_UPFIR), "maua_modconv: NULL x / w");
  MAUA_REQUIRE(d->s || route == R_UPFIR, "maua_modconv: NULL styles");
  MAUA_REQUIRE(d->up == 1 || d->up == 2, "maua_modconv: up must be 1 or 2");
  MAUA_REQUIRE(d->y || ((route == R_HIRES || route == R_FUSED) && (d->rgb_out || route == R_FUSED)), "maua_modconv: NULL y");
  MAUA_REQUIRE(d->x_bstride == 0 || d->x_bstride >= (long)d->H * d->W * d->Ci || route == R_UPFIR, "maua_modconv: samples of x overlap");
  MAUA_REQUIRE(!d1 || route == R_FUSED, "maua_modconv: a second layer goes with the fused walk only");
  const bool dense = d->x_bstride == (long)d->H * d->W * d->Ci;
  *tile = 0;
  switch (route) {
    case R_LOWRES: {
      const ConvArgs a = conv_args(d);
      if (int rc = lowres_check(dtype, a)) return rc;
      *tile = lowres_ksplit(dtype, d->B, d->H, d->W, d->Ci, d->Co, d->up);
      return MAUA_OK;
    }
    case R_GENERIC: {
      const ConvArgs a = conv_args(d);
      if (int rc = modconv3x3_check(dtype, a)) return rc;
      *tile = modconv_tile(elem_bytes(dtype), a);
      return MAUA_OK;
    }
    case R_DMA: {
      ConvArgs a = conv_args(d);
      a.s = nullptr;   // (the input carries the styles)
      MAUA_REQUIRE(dtype != MAUA_F32, "modconv_dma: unsupported dtype");
      MAUA_REQUIRE(dma_conv_supported(dtype, a.Ci, a.Co, a.up, a.H, a.W), "modconv_dma: unsupported shape");
      if (int rc = dma_conv_check(dtype, a)) return rc;
      MAUA_REQUIRE(!a.rgb_out || (dma_rgb_fusable(a.Co) && a.rgb_wmod && a.rgb_bias && a.H % 2 == 0 && a.W % 2 == 0),
                   "modconv_dma: fused toRGB needs all channels in one N tile");
      MAUA_REQUIRE(d->Ci % 8 == 0, "premod: Ci must be a multiple of 8");
      *tile = dma_conv_tile(dtype, a);
      return MAUA_OK;
    }
    case R_HIRES:
    case R_UPWALK: {
      MAUA_REQUIRE(dense, "maua_modconv: this route reads a dense input");
      MAUA_REQUIRE(!d->out_scale && !d->y_scaled, "maua_modconv: this route carries no out_scale / y_scaled");
      const HiresArgs a = hires_args(d);
      return route == R_HIRES ? hires_check(a, dtype) : upwalk_check(a, dtype);
    }
    case R_FUSED: {
      MAUA_REQUIRE(d1, "maua_modconv: the fused walk needs the block's conv1");
      MAUA_REQUIRE(dense, "maua_modconv: this route reads a dense input");
      MAUA_REQUIRE(!d->out_scale && !d->y_scaled && !d1->out_scale && !d1->y_scaled && !d->rgb_out,
                   "maua_modconv: this route carries no out_scale / y_scaled");
      MAUA_REQUIRE(d1->w && d1->s && d1->B == d->B, "maua_modconv: NULL x / w");
      return upwalk_fused_check(hires_args(d), hires_args(d1), dtype);
    }
    case R_TFIR:
    case R_TDMA:
    case R_T2: {
      MAUA_REQUIRE(d->up == 2, "maua_modconv: the transposed-convolution routes are up-layers");
      MAUA_REQUIRE(!d->rgb_out && !d->y_scaled && !d->rgb8_out, "maua_modconv: the transposed-convolution routes carry no toRGB / y_scaled");
      const ConvArgs a = tconv_args(d);
      const UpfirArgs u = upfir_args(d);
      if (route == R_TFIR) return tconv_fir_check(a, u, dtype);
      if (route == R_TDMA) {
        MAUA_REQUIRE(d->Ci % 8 == 0, "premod: Ci must be a multiple of 8");
        if (int rc = tconv_edges_check(a, dtype)) return rc;
        if (int rc = tconv_dma_check(a, dtype)) return rc;
      } else if (int rc = tconv2_check(dtype, a)) {
        return rc;
      }
      return upfir_check(dtype, u);
    }
    case R_UPFIR:
      MAUA_REQUIRE(!d->rgb_out && !d->y_scaled && !d->rgb8_out, "maua_modconv: the transposed-convolution routes carry no toRGB / y_scaled");
      return upfir_check(dtype, upfir_args(d));
  }
  return MAUA_OK;
}

}  // namespace
}  // namespace maua

using namespace maua;

extern "C" int maua_modconv_route(const maua_modconv_desc* d, const maua_modconv_desc* d1, int dtype, int route, int* tile) {
  MAUA_REQUIRE(d, "maua_modconv_route: desc is NULL");
  int t = 0;
  if (int rc = modconv_plan(d, d1, dtype, route, &t)) return rc;
  if (tile) *tile = t;
  return MAUA_OK;
}

extern "C" int maua_modconv_ex(maua_ctx* ctx, const maua_modconv_desc* d, const maua_modconv_desc* d1, int dtype, int route,
                               int force_segs, int narrow_ok) {
  MAUA_REQUIRE(ctx && d, "maua_modconv_ex: NULL argument");
  int tile = 0;
  if (int rc = modconv_plan(d, d1, dtype, route, &tile)) return rc;
  if (d->B == 0) return MAUA_OK;
  const size_t es = elem_bytes(dtype);
  const size_t CoCi = (size_t)d->Co * d->Ci, px = (size_t)d->B * d->H * d->W;
  // workspaces from the context's scratch arena: prepared weights (two layers for the fused walk), unit styles, the pre-modulated
  // input, t, the split-K partial sums
  const size_t w_bytes = route == R_UPFIR ? 0
                         : route == R_UPWALK || route == R_FUSED ? upwalk_weight_elems(d->Co, d->Ci) * 2
                         : is_tconv(route)                     ? 16 * CoCi * es
                                                               : prepped_weight_elems(3, d->up, d->Co, d->Ci) * es;
  const size_t w1_bytes = route == R_FUSED ? prepped_weight_elems(3, 1, d1->Co, d1->Ci) * es : 0;
  const size_t ones_bytes = route == R_TFIR || route == R_TDMA ? (size_t)d->B * d->Ci * 4 : 0;
  size_t xm_bytes = reads_premod(route) ? px * d->Ci * es : 0, ws_bytes = 0;
  if (route == R_LOWRES) lowres_workspace(dtype, d->B, d->H, d->W, d->Ci, d->Co, d->up, &xm_bytes, &ws_bytes);
  const size_t t_bytes = (route == R_TDMA || route == R_T2) && !d->t ? (size_t)d->B * (2 * d->H + 1) * (2 * d->W + 1) * d->Co * es : 0;
  char *w, *w1, *xm, *tbuf;
  float *ones, *ws;
  if (int rc = carve_scratch(ctx, [&](Scratch& s) {
        w = s.take<char>(w_bytes); w1 = s.take<char>(w1_bytes); ones = s.take<float>(ones_bytes / 4);
        xm = s.take<char>(xm_bytes); ws = s.take<float>(ws_bytes / 4); tbuf = s.take<char>(t_bytes);
      }))
    return rc;
  hipStream_t st = ctx->stream;
  // weights as maua_synth_load prepares them for the route
  if (route == R_UPWALK || route == R_FUSED) {
    if (int rc = launch_prep_upwalk_weights(st, d->w, w, d->Co, d->Ci, d->flip, dtype)) return rc;
  } else if (is_tconv(route)) {
    if (int rc = launch_prep_tconv_weights(st, dtype, d->w, w, d->Co, d->Ci, d->flip)) return rc;
  } else if (route != R_UPFIR) {
    if (int rc = launch_prep_weights(st, dtype, d->w, w, nullptr, d->Co, d->Ci, 3, d->up, d->up == 2 ? d->flip : 0, d->Co, d->Ci))
      return rc;
  }
  if (route == R_FUSED)
    if (int rc = launch_prep_weights(st, dtype, d1->w, w1, nullptr, d1->Co, d1->Ci, 3, 1, 0, d1->Co, d1->Ci)) return rc;
  // what the plan's Src does in front of a route that reads pre-modulated input: the premod pass, unit styles for the kernel
  const void* x = d->x;
  long x_bstride = d->x_bstride;
  if (reads_premod(route)) {
    if (int rc = launch_premod_nhwc(st, d->x, d->x_bstride, d->s, xm, d->B, (long)d->H * d->W, d->Ci, dtype)) return rc;
    x = xm;
    x_bstride = (long)d->H * d->W * d->Ci;
  }
  if (ones_bytes)
    if (int rc = launch_fill_ones(st, ones, (long)d->B * d->Ci)) return rc;
  switch (route) {
    case R_LOWRES:
    case R_GENERIC:
    case R_DMA: {
      ConvArgs a = conv_args(d);
      a.x = x; a.x_bstride = x_bstride; a.w = w;
      if (route == R_DMA) a.s = nullptr;
      return route == R_LOWRES    ? launch_modconv_lowres(st, dtype, a, xm, ws)
             : route == R_GENERIC ? launch_modconv3x3(st, dtype, a)
                                  : launch_modconv_dma(st, a, dtype);
    }
    case R_HIRES:
    case R_UPWALK:
    case R_FUSED: {
      HiresArgs a = hires_args(d);
      a.w = w;
      if (route == R_HIRES) return launch_modconv_hires(st, a, dtype);
      if (route == R_UPWALK) return launch_upwalk(st, a, dtype);
      HiresArgs f = hires_args(d1);
      f.x = nullptr; f.y = nullptr; f.w = w1;
      a.y = nullptr;
      return launch_upwalk_fused(st, a, f, force_segs, narrow_ok, dtype);
    }
    case R_TFIR:
    case R_TDMA:
    case R_T2: {
      void* t = d->t ? d->t : tbuf;
      ConvArgs a = tconv_args(d);
      a.x = x; a.x_bstride = x_bstride; a.w = w; a.y = t;
      if (route != R_T2) a.s = ones;
      UpfirArgs u = upfir_args(d);
      if (route == R_TFIR) return launch_tconv_fir(st, a, u, dtype, force_segs >= 0, force_segs);   // (force_segs < 0: the tile form)
      if (route == R_TDMA) {
        if (int rc = launch_tconv_edges(st, a, dtype)) return rc;
        if (int rc = launch_tconv_dma(st, a, dtype)) return rc;
      } else if (int rc = launch_tconv2(st, dtype, a)) {
        return rc;
      }
      u.t = t;
      return launch_upfir_epilogue(st, dtype, u);
    }
    case R_UPFIR: {
      UpfirArgs u = upfir_args(d);
      u.t = d->x;
      return launch_upfir_epilogue(st, dtype, u);
    }
  }
  return MAUA_OK;
}

extern "C" int maua_torgb_ex(maua_ctx* ctx, const void* x, const float* wmod, const float* bias, const float* prev, float* out, int B,
                             int H, int W, int C, float clamp, int dtype) {
  MAUA_REQUIRE(ctx && x && wmod && bias && out, "maua_torgb_ex: NULL argument");
  MAUA_REQUIRE(B >= 0 && H > 0 && W > 0 && C > 0, "maua_torgb_ex: bad shape");
  MAUA_REQUIRE(!prev || (H % 2 == 0 && W % 2 == 0), "maua_torgb_ex: the skip image needs an even grid");
  RgbArgs r{};
  r.x = x; r.wmod = wmod; r.bias = bias; r.prev = prev; r.out = out; r.B = B; r.H = H; r.W = W; r.C = C; r.clamp = clamp;
  upsample_fir16(r.fir);
  return launch_torgb(ctx->stream, dtype, r);
}
