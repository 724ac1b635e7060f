// The gradient of the StyleGAN2 synthesis network to its latents: maua_synth_vjp walks a forward that kept its features
// (option "keep_features" = 1: every layer's output stays in its own buffer, the styles and demodulation coefficients stay in the
// layers' s / d) from the last block to the first, g_img -> g_ws.  No reference counterpart in code: the reference differentiates
// inference/stylegan2.py:385-436 with torch.autograd (sampling/langevin.py).
//
// Per block, last to first (img_r = toRGB(x_r) + upsample2d(img_{r/2}), x_r = conv1(conv0(x_{r/2}))):
//   toRGB     g_x_r (+)= wmod^T g_img_r (+: what the next block's conv0 already left there), g_s from g_wmod
//   skip      g_img_{r/2} = upsample2d^T g_img_r
//   conv1     g_x_r -> gradient of conv0's output, g_s
//   conv0     -> g_x_{r/2}, g_s
// and every g_s goes through its affine layer into the ws row the layer read: g_ws[b][w_index] += g_s A / sqrt(w_dim) (toRGB: and
// / sqrt(C)).  A row is shared by a block's toRGB and the next block's conv0; the launches add to it in walk order.
#include <cmath>

#include "common.h"
#include "internal.h"
#include "synth_internal.h"

namespace maua {

namespace {

int synth_vjp_check(const maua_synth* n, int B) {
  MAUA_REQUIRE(n, "maua_synth_vjp: net is NULL");
  MAUA_REQUIRE(B > 0, "maua_synth_vjp: the batch must be positive");
  MAUA_REQUIRE(n->dtype != MAUA_F16, "maua_synth_vjp: an MAUA_F16 network is not differentiated (its pre-normalisation of weights and styles is not)");
  MAUA_REQUIRE(n->rs_layer < 0 && !n->warp_minv[0] && !n->warp_minv[1] && !n->warp_minv[2],
               "maua_synth_vjp: a resize or warp hook is installed (the hooks are not differentiated)");
  MAUA_REQUIRE(n->keep_features && n->kept_B > 0 && n->kept_B == B,
               "maua_synth_vjp: no kept forward of this batch size (run the forward with option keep_features = 1 first)");
  MAUA_REQUIRE(!n->kept_stale, "maua_synth_vjp: an option, a weight load or a resize came after the kept forward: run it again");
  MAUA_REQUIRE(!n->kept_scaled, "maua_synth_vjp: the kept forward ran with per-sample noise scales (RawNoise), which are not differentiated");
  return MAUA_OK;
}

int ensure_vjp(maua_synth* n, int B) {
  SynthVjpState& v = n->vjp;
  hipStream_t st = n->ctx->stream;
  if (!v.weights_ready) {   // the forward's own (rounded, flipped) weights in the gradient convolution's layout
    for (auto& c : n->convs) {
      if (!c.wg)
        if (int rc = c.wg.alloc(9 * (size_t)c.Ci * c.Co * n->esize)) return rc;
      if (int rc = launch_vjp_weights_from_prepared(st, n->dtype, (c.up == 2 ? c.wt_t : c.wt).get(), c.wg.get(), c.Co, c.Ci, c.up)) return rc;
    }
    v.weights_ready = true;
  }
  if (B <= v.bcap) return MAUA_OK;
  MAUA_HIP_CHECK(hipStreamSynchronize(st));
  v.bcap = 0;
  ModconvVjpWorkspace m{0, 0, 0, 0, 0};
  size_t feat = 0, rgb_part = 0;
  int maxc = 0;
  for (auto& c : n->convs) {
    const ModconvVjpWorkspace w = modconv_vjp_workspace(n->dtype, B, c.ih, c.iw, c.Ci, c.Co, c.up);
    m.g_u = std::max(m.g_u, w.g_u); m.g_t = std::max(m.g_t, w.g_t); m.g_xm = std::max(m.g_xm, w.g_xm);
    m.part = std::max(m.part, w.part); m.g_d = std::max(m.g_d, w.g_d);
    feat = std::max(feat, (size_t)B * c.oh * c.ow * c.Co * n->esize);
    maxc = std::max(maxc, std::max(c.Ci, c.Co));
  }
  for (auto& r : n->rgbs) rgb_part = std::max(rgb_part, torgb_vjp_part_bytes(B, r.h, r.w, r.C));
  m.part = std::max(m.part, rgb_part);
  auto layout = [&](Scratch& s) {
    for (int i = 0; i < 2; i++) {
      v.gfeat[i] = s.take<char>(feat);
      v.gimg[i] = s.take<float>((size_t)B * 3 * std::max(1, n->out_h * n->out_w / 4));
    }
    v.g_u = s.take<char>(m.g_u);
    v.g_t = m.g_t ? s.take<char>(m.g_t) : nullptr;
    v.g_xm = (float*)s.take<char>(m.g_xm);
    v.part = (float*)s.take<char>(m.part);
    v.g_d = (float*)s.take<char>(m.g_d);
    v.g_s = s.take<float>((size_t)B * maxc);
    v.g_wmod = s.take<float>((size_t)B * 3 * maxc);
  };
  if (int rc = carve_into(v.ws, layout)) return rc;
  v.bcap = B;
  return MAUA_OK;
}

// the per-group channel sums of the noise gradient: only a walk that was asked for g_noise allocates them
int ensure_noise_part(maua_synth* n, int B) {
  SynthVjpState& v = n->vjp;
  if (B <= v.npart_bcap) return MAUA_OK;
  MAUA_HIP_CHECK(hipStreamSynchronize(n->ctx->stream));
  v.npart_bcap = 0;
  size_t bytes = 0;
  for (auto& c : n->convs) bytes = std::max(bytes, modconv_vjp_noise_part_bytes(B, c.ih, c.iw, c.Co, c.up));
  if (int rc = v.npart.alloc(bytes)) return rc;
  v.npart_bcap = B;
  return MAUA_OK;
}

}  // namespace
}  // namespace maua

using namespace maua;

extern "C" int maua_synth_vjp_check(const maua_synth* net, int B) { return synth_vjp_check(net, B); }

extern "C" int maua_synth_vjp(maua_synth* n, const float* const* noise, const long* noise_bstride, int B, const float* g_img, float* g_ws) {
  return maua_synth_vjp_ex(n, noise, noise_bstride, B, g_img, g_ws, nullptr, nullptr);
}

extern "C" int maua_synth_vjp_ex(maua_synth* n, const float* const* noise, const long* noise_bstride, int B, const float* g_img, float* g_ws,
                                 float* const* g_noise, const long* g_noise_bstride) {
  if (int rc = synth_vjp_check(n, B)) return rc;
  MAUA_REQUIRE(g_img && g_ws, "maua_synth_vjp: NULL argument");
  bool want_noise = false;
  for (size_t l = 0; g_noise && l < n->convs.size(); l++) {
    if (!g_noise[l]) continue;
    want_noise = true;
    const long hw = (long)n->convs[l].oh * n->convs[l].ow;
    MAUA_REQUIRE(!g_noise_bstride || g_noise_bstride[l] == 0 || g_noise_bstride[l] >= hw, "maua_synth_vjp_ex: samples of g_noise overlap");
  }
  if (int rc = ensure_vjp(n, B)) return rc;
  if (want_noise)
    if (int rc = ensure_noise_part(n, B)) return rc;
  SynthVjpState& v = n->vjp;
  hipStream_t st = n->ctx->stream;
  MAUA_HIP_CHECK(hipMemsetAsync(g_ws, 0, (size_t)B * n->num_ws * n->w_dim * sizeof(float), st));
  const float wgain = 1.f / std::sqrt((float)n->w_dim);
  const float* gi = g_img;   // gradient of the block's image
  int img_cur = 0;
  bool have_gx = false;      // gfeat[0] already holds the next block's contribution to this block's features
  size_t li = n->convs.size();
  auto conv_vjp = [&](const ConvLayer& c, size_t l, const void* x, long x_bstride, const void* g_y, void* g_x) -> int {
    const bool given = noise && noise[l];
    ModconvVjpArgs a{};
    a.x = x; a.x_bstride = x_bstride; a.y = c.feat.get(); a.g_y = g_y; a.wg = c.wg.get(); a.wsq = c.wsq.as<float>(); a.s = c.s.as<float>(); a.d = c.d.as<float>();
    a.noise = given ? noise[l] : c.noise_const.as<float>();
    a.noise_bstride = given ? (noise_bstride ? noise_bstride[l] : (long)c.oh * c.ow) : 0;
    a.noise_strength = (n->nv_compat & 2) ? c.noise_strength : 1.f;
    a.bias = c.bias.as<float>(); a.g_x = g_x; a.accumulate = 0; a.g_s = v.g_s;
    if (g_noise && g_noise[l]) {   // (no stride array: one map per sample)
      a.g_noise = g_noise[l]; a.g_noise_bstride = g_noise_bstride ? g_noise_bstride[l] : (long)c.oh * c.ow; a.npart = v.npart.as<float>();
    }
    a.B = B; a.H = c.ih; a.W = c.iw; a.Ci = c.Ci; a.Co = c.Co; a.up = c.up;
    a.act = MAUA_ACT_LRELU; a.alpha = 0.2f; a.gain = std::sqrt(2.0f); a.clamp = 256.f;   // (synth.hip lrelu_epilogue)
    a.g_u = v.g_u; a.g_t = v.g_t; a.g_xm = v.g_xm; a.part = v.part; a.g_d = v.g_d;
    if (int rc = launch_modconv_vjp(st, n->dtype, a)) return rc;
    return launch_affine_vjp(st, v.g_s, c.Ci, c.affine_w.as<float>(), wgain, g_ws, c.w_index, n->num_ws, n->w_dim, B, c.Ci);
  };
  for (int blk = n->nblocks - 1; blk >= 0; blk--) {
    const RgbLayer& g = n->rgbs[blk];
    const ConvLayer& c1 = n->convs[li - 1];
    RgbVjpArgs r{};
    r.x = c1.feat.get(); r.wmod = g.wmod.as<float>(); r.bias = g.bias.as<float>(); r.g_img = gi; r.g_x = v.gfeat[0]; r.accumulate = have_gx; r.g_wmod = v.g_wmod;
    r.part = v.part; r.B = B; r.H = g.h; r.W = g.w; r.C = g.C; r.clamp = 256.f;
    if (int rc = launch_torgb_vjp(st, n->dtype, r)) return rc;
    if (int rc = launch_rgb_styles_vjp(st, v.g_wmod, g.wrgb.as<float>(), v.g_s, B, g.C)) return rc;
    if (int rc = launch_affine_vjp(st, v.g_s, g.C, g.affine_w.as<float>(), wgain / std::sqrt((float)g.C), g_ws, g.w_index, n->num_ws, n->w_dim, B, g.C))
      return rc;
    if (blk > 0) {
      if (int rc = launch_skip_vjp(st, gi, v.gimg[img_cur], B, g.h / 2, g.w / 2)) return rc;
      gi = v.gimg[img_cur];
      img_cur ^= 1;
    }
    if (blk == 0) {   // conv1 on the learned const input: only its styles want a gradient
      if (int rc = conv_vjp(c1, li - 1, n->const_x.get(), 0, v.gfeat[0], nullptr)) return rc;
      li -= 1;
      break;
    }
    const ConvLayer& c0 = n->convs[li - 2];
    if (int rc = conv_vjp(c1, li - 1, c0.feat.get(), (long)c0.oh * c0.ow * c0.Co, v.gfeat[0], v.gfeat[1])) return rc;
    const ConvLayer& pv = n->convs[li - 3];   // the previous block's conv1
    if (int rc = conv_vjp(c0, li - 2, pv.feat.get(), (long)pv.oh * pv.ow * pv.Co, v.gfeat[1], v.gfeat[0])) return rc;
    have_gx = true;
    li -= 2;
  }
  return MAUA_OK;
}
