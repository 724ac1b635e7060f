// The ResNet bottleneck backbone as a library object (maua_resnet_*): the SwAV ResNet-50 feature extractor of the GAN metrics.
//
// Replaces (reference): maua/GAN/metrics/extractors/swav.py ResNet.forward_backbone (:283-301) over Bottleneck blocks (:89-139) as
// _make_layer builds them (:242-281: the stride sits on the first block's 3x3 and on its 1x1 downsample branch).  BatchNorm is folded
// into weight and bias before anything reaches this file (maua_amd/resnet.py), so a block is four launches of resnet_conv.hip's kernel:
//   t1 = relu(conv1(x));  t2 = relu(conv2(t1));  id = downsample(x) or x;  out = relu(conv3(t2) + id)
// The projection head and the prototypes are not built (forward_head with both None is the identity).
#include <algorithm>
#include <vector>

#include "common.h"
#include "internal.h"
#include "plain_conv.h"

namespace maua {
namespace {

struct RConv {
  int Ci = 0, Co = 0, k = 0, stride = 1, pad = 0;
  DevBuf wt;     // prepared weights (allocated by the first load)
  DevBuf bias;   // float [Co]
};

struct RBlock { int c1, c2, c3, ds; };   // indices into convs (ds: -1 = identity)

}  // namespace
}  // namespace maua

using namespace maua;

struct maua_resnet {
  maua_ctx* ctx = nullptr;   // NULL: a shape-only object (conv_count / conv_shape), nothing on a device
  int dtype = MAUA_F32;
  size_t esize = 4;
  int width = 64;
  std::vector<RConv> convs;
  std::vector<RBlock> blocks;
  int layer_end[4] = {0, 0, 0, 0};   // one past the last block of each layer
  // the activation workspace: one carved set, placed for (B, H, W)
  DevBuf ws;
  int B = 0, H = 0, W = 0;           // what the pieces were placed for (0: none)
  bool ran = false;                  // the taps hold a forward of that shape
  void* tap[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  int tc[6] = {0}, th[6] = {0}, tw[6] = {0};
  void *t1 = nullptr, *t2 = nullptr, *ds = nullptr, *ping = nullptr, *pong = nullptr;
};

namespace {

// stage sizes for an H x W input: stem, pool, layer1 .. layer4
void stage_shapes(maua_resnet* n, int H, int W) {
  int h = sconv_out(H, 7, 2, 3), w = sconv_out(W, 7, 2, 3);
  n->tc[0] = n->width; n->th[0] = h; n->tw[0] = w;
  h = sconv_out(h, 3, 2, 1); w = sconv_out(w, 3, 2, 1);
  n->tc[1] = n->width; n->th[1] = h; n->tw[1] = w;
  for (int l = 0; l < 4; l++) {
    if (l > 0) { h = sconv_out(h, 3, 2, 1); w = sconv_out(w, 3, 2, 1); }
    n->tc[2 + l] = (n->width << l) * 4; n->th[2 + l] = h; n->tw[2 + l] = w;
  }
}

int place(maua_resnet* n, int B, int H, int W) {
  if (n->ws && B == n->B && H == n->H && W == n->W) return MAUA_OK;
  MAUA_HIP_CHECK(hipStreamSynchronize(n->ctx->stream));   // (a forward of the old layout may still run)
  n->B = n->H = n->W = 0; n->ran = false;
  stage_shapes(n, H, W);
  // inside layer l a block reads at most [h_in][w_in][C_out] (the first block's conv1 output, before the stride) and writes [h][w][C_out]
  size_t inner = 0, outer = 0;
  for (int l = 0; l < 4; l++) {
    const size_t pin = (size_t)n->th[1 + l] * n->tw[1 + l], pout = (size_t)n->th[2 + l] * n->tw[2 + l];
    inner = std::max(inner, (size_t)B * pin * (size_t)(n->width << l));
    outer = std::max(outer, (size_t)B * pout * (size_t)n->tc[2 + l]);
  }
  const size_t es = n->esize;
  auto layout = [&](Scratch& s) {
    for (int i = 0; i < 6; i++) n->tap[i] = s.take<char>((size_t)B * n->th[i] * n->tw[i] * n->tc[i] * es);
    n->t1 = s.take<char>(inner * es);
    n->t2 = s.take<char>(inner * es);
    n->ds = s.take<char>(outer * es);
    n->ping = s.take<char>(outer * es);
    n->pong = s.take<char>(outer * es);
  };
  if (int rc = carve_into(n->ws, layout)) return rc;
  n->B = B; n->H = H; n->W = W;
  return MAUA_OK;
}

int run_conv(maua_resnet* n, int index, const void* x, int B, int H, int W, const void* res, bool relu, void* y) {
  const RConv& c = n->convs[index];
  MAUA_REQUIRE(c.wt && c.bias, "maua_resnet_forward: convolution " + std::to_string(index) + " has no weight or no bias loaded");
  SConvArgs a{};
  a.x = x; a.w = c.wt.get(); a.bias = c.bias.as<float>(); a.res = res; a.y = y;
  a.B = B; a.H = H; a.W = W; a.Ci = c.Ci; a.Co = c.Co; a.k = c.k; a.stride = c.stride; a.pad = c.pad;
  a.relu = relu; a.stem = index == 0; a.kpad = a.stem ? stem_kpad(n->dtype) : 0;
  return launch_sconv(n->ctx->stream, n->dtype, a);
}

}  // namespace

extern "C" {

int maua_resnet_create(maua_ctx* ctx, int dtype, const int* layers, int width, maua_resnet** out) {
  MAUA_REQUIRE(layers && out, "maua_resnet_create: NULL argument");
  MAUA_REQUIRE(dtype == MAUA_F32 || dtype == MAUA_BF16, "maua_resnet_create: unsupported dtype");
  MAUA_REQUIRE(width > 0 && width % 64 == 0 && width <= 1024, "maua_resnet_create: width must be a multiple of 64, at most 1024");
  for (int l = 0; l < 4; l++) MAUA_REQUIRE(layers[l] >= 1 && layers[l] <= 256, "maua_resnet_create: every layer has 1 .. 256 blocks");
  maua_resnet* n = new maua_resnet();
  n->ctx = ctx; n->dtype = dtype; n->esize = elem_bytes(dtype); n->width = width;
  auto add = [&](int ci, int co, int k, int stride, int pad) {
    RConv c; c.Ci = ci; c.Co = co; c.k = k; c.stride = stride; c.pad = pad;
    n->convs.push_back(std::move(c));
    return (int)n->convs.size() - 1;
  };
  add(3, width, 7, 2, 3);
  int inplanes = width;
  for (int l = 0; l < 4; l++) {
    const int planes = width << l, stride = l == 0 ? 1 : 2;
    for (int b = 0; b < layers[l]; b++) {
      RBlock k;
      const int st = b == 0 ? stride : 1;
      k.c1 = add(inplanes, planes, 1, 1, 0);
      k.c2 = add(planes, planes, 3, st, 1);
      k.c3 = add(planes, planes * 4, 1, 1, 0);
      k.ds = b == 0 ? add(inplanes, planes * 4, 1, st, 0) : -1;   // (swav.py:249: stride != 1 or inplanes != 4 planes - always, in a first block)
      inplanes = planes * 4;
      n->blocks.push_back(k);
    }
    n->layer_end[l] = (int)n->blocks.size();
  }
  *out = n;
  return MAUA_OK;
}

void maua_resnet_destroy(maua_resnet* n) {
  if (!n) return;
  if (n->ctx) hipStreamSynchronize(n->ctx->stream);
  delete n;
}

int maua_resnet_conv_count(maua_resnet* n) { return n ? (int)n->convs.size() : 0; }

int maua_resnet_conv_shape(maua_resnet* n, int index, int* ci, int* co, int* k, int* stride) {
  MAUA_REQUIRE(n && ci && co && k && stride && index >= 0 && index < (int)n->convs.size(), "maua_resnet_conv_shape: bad argument");
  const RConv& c = n->convs[index];
  *ci = c.Ci; *co = c.Co; *k = c.k; *stride = c.stride;
  return MAUA_OK;
}

int maua_resnet_load(maua_resnet* n, int index, int what, const float* host, size_t count) {
  MAUA_REQUIRE(n && host, "maua_resnet_load: NULL argument");
  MAUA_REQUIRE(n->ctx, "maua_resnet_load: the network was created without a context");
  MAUA_REQUIRE(index >= 0 && index < (int)n->convs.size(), "maua_resnet_load: no such convolution");
  MAUA_REQUIRE(what == 0 || what == 1, "maua_resnet_load: what must be 0 or 1");
  hipStream_t st = n->ctx->stream;
  RConv& c = n->convs[index];
  MAUA_HIP_CHECK(hipStreamSynchronize(st));   // (a forward that reads the old values may still run)
  if (what == 1) {
    MAUA_REQUIRE(count == (size_t)c.Co, "maua_resnet_load: bias: wrong size");
    if (!c.bias)
      if (c.bias.alloc((size_t)c.Co * 4)) return fail_in("maua_resnet_load");
    MAUA_HIP_CHECK(hipMemcpy(c.bias.get(), host, (size_t)c.Co * 4, hipMemcpyHostToDevice));
    return MAUA_OK;
  }
  MAUA_REQUIRE(count == (size_t)c.Co * c.Ci * c.k * c.k, "maua_resnet_load: weight: wrong size");
  const bool stem = index == 0;
  const size_t elems = stem ? (size_t)c.Co * stem_kpad(n->dtype) : prepped_weight_elems(c.k, 1, c.Co, c.Ci);
  if (!c.wt)
    if (c.wt.alloc(elems * n->esize)) return fail_in("maua_resnet_load");
  DevBuf tmp;
  if (stage(tmp, host, count)) return fail_in("maua_resnet_load");
  const int rc = stem ? launch_prep_stem_weights(st, n->dtype, tmp.as<float>(), c.wt.get(), c.Co)
                      : launch_prep_weights(st, n->dtype, tmp.as<float>(), c.wt.get(), nullptr, c.Co, c.Ci, c.k, 1, 0, c.Co, c.Ci);
  hipStreamSynchronize(st);   // (also on failure: tmp is freed behind whatever was launched)
  return rc;
}

}  // extern "C"

namespace {

// ev: NULL, or 8 events recorded on the stream before the stem and after the stem, the pool, layer1 .. layer4 and the average pool
int forward_impl(maua_resnet* n, const float* img, int B, int H, int W, float* features, hipEvent_t* ev) {
  MAUA_REQUIRE(n && img && features, "maua_resnet_forward: NULL argument");
  MAUA_REQUIRE(n->ctx, "maua_resnet_forward: the network was created without a context");
  MAUA_REQUIRE(B >= 0 && B <= 65535 && H >= 1 && W >= 1 && (long)H * W <= (1L << 26), "maua_resnet_forward: bad image shape");
  if (B == 0) return MAUA_OK;
  if (int rc = place(n, B, H, W)) return rc;
  hipStream_t st = n->ctx->stream;
  n->ran = false;
  int mark = 0;
  auto stamp = [&]() -> int {
    if (ev) MAUA_HIP_CHECK(hipEventRecord(ev[mark++], st));
    return MAUA_OK;
  };
  if (int rc = stamp()) return rc;
  if (int rc = run_conv(n, 0, img, B, H, W, nullptr, true, n->tap[0])) return rc;
  if (int rc = stamp()) return rc;
  if (int rc = launch_maxpool3x3s2(st, n->dtype, n->tap[0], n->tap[1], B, n->th[0], n->tw[0], n->width)) return rc;
  if (int rc = stamp()) return rc;
  const void* x = n->tap[1];
  int h = n->th[1], w = n->tw[1], blk = 0;
  for (int l = 0; l < 4; l++) {
    for (; blk < n->layer_end[l]; blk++) {
      const RBlock& k = n->blocks[blk];
      const int ho = n->th[2 + l], wo = n->tw[2 + l];
      void* y = blk + 1 == n->layer_end[l] ? n->tap[2 + l] : (x == n->ping ? n->pong : n->ping);
      if (int rc = run_conv(n, k.c1, x, B, h, w, nullptr, true, n->t1)) return rc;
      if (int rc = run_conv(n, k.c2, n->t1, B, h, w, nullptr, true, n->t2)) return rc;
      const void* id = x;
      if (k.ds >= 0) {
        if (int rc = run_conv(n, k.ds, x, B, h, w, nullptr, false, n->ds)) return rc;
        id = n->ds;
      }
      if (int rc = run_conv(n, k.c3, n->t2, B, ho, wo, id, true, y)) return rc;
      x = y; h = ho; w = wo;
    }
    if (int rc = stamp()) return rc;
  }
  if (int rc = launch_global_avgpool(st, n->dtype, n->tap[5], features, B, n->th[5], n->tw[5], n->tc[5])) return rc;
  if (int rc = stamp()) return rc;
  n->ran = true;
  return MAUA_OK;
}

}  // namespace

extern "C" {

int maua_resnet_forward(maua_resnet* n, const float* img, int B, int H, int W, float* features) {
  return forward_impl(n, img, B, H, W, features, nullptr);
}

int maua_resnet_forward_timed(maua_resnet* n, const float* img, int B, int H, int W, float* features, float* stage_ms) {
  MAUA_REQUIRE(stage_ms, "maua_resnet_forward_timed: NULL argument");
  MAUA_REQUIRE(B > 0, "maua_resnet_forward_timed: empty batch");
  hipEvent_t ev[8];
  int made = 0;
  int rc = MAUA_OK;
  for (; made < 8; made++)
    if (hipEventCreate(&ev[made]) != hipSuccess) { rc = fail("maua_resnet_forward_timed: hipEventCreate failed"); break; }
  if (!rc) rc = forward_impl(n, img, B, H, W, features, ev);
  if (!rc && hipEventSynchronize(ev[7]) != hipSuccess) rc = fail("maua_resnet_forward_timed: hipEventSynchronize failed");
  for (int i = 0; !rc && i < 7; i++)
    if (hipEventElapsedTime(&stage_ms[i], ev[i], ev[i + 1]) != hipSuccess) rc = fail("maua_resnet_forward_timed: hipEventElapsedTime failed");
  for (int i = 0; i < made; i++) (void)hipEventDestroy(ev[i]);
  return rc;
}

int maua_resnet_tap_shape(maua_resnet* n, int stage, int* C, int* h, int* w) {
  MAUA_REQUIRE(n && C && h && w, "maua_resnet_tap_shape: NULL argument");
  MAUA_REQUIRE(stage >= 0 && stage < 6, "maua_resnet_tap_shape: stage must be 0 .. 5");
  MAUA_REQUIRE(n->ran, "maua_resnet_tap_shape: call maua_resnet_forward first");
  *C = n->tc[stage]; *h = n->th[stage]; *w = n->tw[stage];
  return MAUA_OK;
}

int maua_resnet_tap(maua_resnet* n, int stage, float* out) {
  MAUA_REQUIRE(n && out, "maua_resnet_tap: NULL argument");
  MAUA_REQUIRE(stage >= 0 && stage < 6, "maua_resnet_tap: stage must be 0 .. 5");
  MAUA_REQUIRE(n->ran, "maua_resnet_tap: call maua_resnet_forward first");
  hipStream_t st = n->ctx->stream;
  const int C = n->tc[stage], hw = n->th[stage] * n->tw[stage];
  return dispatch_dtype<bf16_t, float>(n->dtype, "maua_resnet_tap", [&](auto t) {
    return launch_nhwc_to_nchw<decltype(t), float>(st, n->tap[stage], out, n->B, C, hw, C);
  });
}

}  // extern "C"
