// Kernel-selection switches of the plain 3x3 convolutions (maua_conv3x3_route, maua_conv3x3_ex): one convolution described the way
// the networks describe theirs (ConvArgs without styles - the diffusion UNet, the secondary model, the VGG perceptors, the up-scalers),
// run on a kernel of the caller's choice.  For parity tests; no reference counterpart.
#include <algorithm>

#include "common.h"
#include "internal.h"
#include "plain_conv.h"

namespace maua {
namespace {

struct ConvPlan { int kernel, variant, ksplit; };

bool dtype_ok(int dtype) { return dtype == MAUA_F32 || dtype == MAUA_BF16 || dtype == MAUA_F16 || dtype == MAUA_F32_SPLIT; }

// the launch arguments, filled as Runner::conv (unet.hip), super.hip and perceptor.hip fill theirs (w / s are set by the caller)
ConvArgs conv_args(const maua_conv_desc* d) {
  ConvArgs a{};
  a.x = d->x; a.x_pstride = d->x_pstride; a.x_bstride = d->x_bstride; a.bias = d->bias;
  a.y = d->y; a.y_pstride = d->y_pstride; a.y_coff = d->y_coff; a.y_bstride = d->y_bstride;
  a.res = d->res; a.res_pstride = d->res_pstride; a.res_bstride = d->res_bstride;
  a.res2 = d->res2; a.res2_pstride = d->res2_pstride; a.res2_bstride = d->res2_bstride; a.res_gain = d->res_gain;
  a.B = d->B; a.H = d->H; a.W = d->W; a.Ci = d->Ci; a.Co = d->Co; a.up = 1;
  a.act = d->act; a.alpha = d->alpha; a.gain = d->gain; a.clamp = d->clamp;
  a.Ci_read = d->Ci_read; a.x_up2 = d->x_up2; a.variant = d->variant; a.psum = d->psum;
  return a;
}

// sel: 0 / 1 / 2 = the UNet's routing under that "route" option, 101 / 102 / 103 = kernel 1 / 2 / 3 whatever the routing would take.
// Every refusal of the chosen launcher is raised here, before anything is launched; *a gets the routing's own variant / psum choice.
int conv_plan(const maua_conv_desc* d, int dtype, int sel, ConvArgs* a, ConvPlan* out) {
  MAUA_REQUIRE(dtype_ok(dtype), "maua_conv3x3: unsupported dtype");
  MAUA_REQUIRE(d->B >= 0 && d->H > 0 && d->W > 0 && d->Ci > 0 && d->Co > 0, "maua_conv3x3: bad shape");
  MAUA_REQUIRE(d->x && d->w && d->y, "maua_conv3x3: NULL x / w / y");
  MAUA_REQUIRE(!d->res2 || d->res, "maua_conv3x3: res2 goes with res (no kernel applies it alone)");
  MAUA_REQUIRE(d->x_pstride >= 0 && d->y_pstride >= 0 && d->y_coff >= 0 && d->Ci_read >= 0 && d->Ci_read <= d->Ci,
               "maua_conv3x3: bad strides / Ci_read");
  MAUA_REQUIRE(sel == 0 || sel == 1 || sel == 2 || (sel >= 101 && sel <= 103), "maua_conv3x3: kernel must be 0 .. 3");
  *a = conv_args(d);
  ConvPlan p{0, 0, 0};
  if (sel < 100) {
    // (the split type is float32 storage: the network routes it as float32, i.e. to the generic kernel or never at all)
    const UnetConvRoute r = unet_conv_route(dtype, sel, d->B, d->H, d->W, d->Ci, d->Co);
    p.kernel = r.kernel;
    a->variant = r.variant;
    if (!(r.kernel == 2 && r.wide)) a->psum = nullptr;   // as in the network: only the wide LDS-direct tiles leave piece sums
  } else {
    p.kernel = sel - 100;
  }
  if (p.kernel == 1) {
    MAUA_REQUIRE(d->Ci % 32 == 0, "modconv3x3: Ci must be a multiple of 32 (pad channels)");
    MAUA_REQUIRE(d->Co % 32 == 0, "modconv3x3: Co must be a multiple of 32 (pad channels)");
    MAUA_REQUIRE(d->B <= 65535, "modconv3x3: grid too large");
    MAUA_REQUIRE(!a->x_up2 && !a->psum && (!a->Ci_read || a->Ci_read == a->Ci), "modconv3x3: no x_up2 / psum / Ci_read on the generic kernel");
    p.variant = modconv_tile(elem_bytes(dtype), *a);
  } else if (p.kernel == 2) {
    if (int rc = dma_conv_check(dtype, *a)) return rc;
    p.variant = dma_conv_tile(dtype, *a);
  } else {
    if (int rc = gather_conv_check(dtype, *a)) return rc;
    p.ksplit = gather_conv_ksplit(dtype, d->B, d->H, d->W, d->Ci, d->Co);
  }
  *out = p;
  return MAUA_OK;
}

}  // namespace
}  // namespace maua

using namespace maua;

extern "C" int maua_conv3x3_route(const maua_conv_desc* d, int dtype, int unet_route_option, int* variant, int* ksplit) {
  MAUA_REQUIRE(d, "maua_conv3x3_route: desc is NULL");
  ConvArgs a;
  ConvPlan p;
  if (int rc = conv_plan(d, dtype, unet_route_option, &a, &p)) return rc;
  if (variant) *variant = p.variant;
  if (ksplit) *ksplit = p.ksplit;
  return p.kernel;
}

extern "C" int maua_conv3x3_ex(maua_ctx* ctx, const maua_conv_desc* d, int dtype, int kernel) {
  MAUA_REQUIRE(ctx && d, "maua_conv3x3_ex: NULL argument");
  MAUA_REQUIRE(kernel >= 0 && kernel <= 3, "maua_conv3x3: kernel must be 0 .. 3");
  ConvArgs a;
  ConvPlan p;
  if (int rc = conv_plan(d, dtype, kernel ? 100 + kernel : 0, &a, &p)) return rc;
  if (d->B == 0) return MAUA_OK;
  const size_t es = elem_bytes(dtype);
  const size_t wt_bytes = prepped_weight_elems(3, 1, d->Co, d->Ci) * es;
  const size_t ones_bytes = p.kernel == 1 ? (size_t)d->B * d->Ci * 4 : 0;
  const size_t ws_bytes = p.kernel == 3 ? gather_conv_workspace(dtype, d->B, d->H, d->W, d->Ci, d->Co) : 0;
  char* w;
  float *ones, *ws;
  if (int rc = carve_scratch(ctx, [&](Scratch& s) { w = s.take<char>(wt_bytes); ones = s.take<float>(ones_bytes / 4); ws = s.take<float>(ws_bytes / 4); }))
    return rc;
  hipStream_t st = ctx->stream;
  // weights as the networks prepare theirs: [9][Co][Ci] in the storage type, the split type's float32 copy split in place
  const int store_dtype = dtype == MAUA_F32_SPLIT ? MAUA_F32 : dtype;
  if (int rc = launch_prep_weights(st, store_dtype, d->w, w, nullptr, d->Co, d->Ci, 3, 1, 0, d->Co, d->Ci)) return rc;
  if (dtype == MAUA_F32_SPLIT)
    if (int rc = launch_f32_split_inplace(st, w, (long)9 * d->Co * d->Ci)) return rc;
  a.w = w;
  if (p.kernel == 1) {   // the generic kernel multiplies its input by styles: all ones, as every plain network passes
    if (int rc = launch_fill_ones(st, ones, (long)d->B * d->Ci)) return rc;
    a.s = ones;
    return launch_modconv3x3(st, dtype, a);
  }
  if (p.kernel == 2) return launch_modconv_dma(st, a, dtype);
  return launch_conv_gather(st, dtype, a, ws);
}
