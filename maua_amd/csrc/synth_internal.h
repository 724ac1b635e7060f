// The StyleGAN2 synthesis network object as its translation units see it: synth.hip (parameters, workspace, the forward) and
// synth_vjp.hip (the gradient of a kept forward to the latents).
#pragma once
#include <vector>

#include "common.h"
#include "internal.h"
#include "plain_conv.h"

namespace maua {

struct ConvLayer {
  int block, which;  // which: 0 = conv0 (up 2), 1 = conv1
  int Ci, Co, res, up, w_index;
  int ih = 0, iw = 0;   // input grid of this launch
  int oh = 0, ow = 0;   // conv output grid (= where the noise is added)
  int fh = 0, fw = 0;   // grid handed to the next layer (differs from oh x ow only on the resized layer)
  DevBuf affine_w;     // float [Ci][w_dim]
  DevBuf affine_b;     // float [Ci]
  DevBuf bias;         // float [Co]
  DevBuf noise_const;  // float [oh][ow]
  float noise_strength = 0.f;    // loaded value (used under nv_compat bit1)
  DevBuf wt;           // prepared weights (up-layers: 4 phase kernels, 9 taps each)
  DevBuf wt_t;         // up-layers: transposed-conv class weights (minimal MACs; FIR done afterwards)
  DevBuf wt_h;         // up-layers on the row-walk kernel: half-folded weights (modconv_upwalk.hip)
  DevBuf wsq;          // float [Co][Ci]
  DevBuf s;            // float [Bcap][Ci]   (s, d, feat: the forward's workspace)
  DevBuf d;            // float [Bcap][Co]
  DevBuf feat;         // keep_features buffer
  DevBuf wg;           // input-gradient weights [9][Ci][Co] (synth_vjp.hip: made from wt / wt_t on the first gradient call)
};
struct RgbLayer {
  int block, C, res, w_index;
  int h = 0, w = 0;     // grid toRGB runs on (the block's feature grid)
  DevBuf affine_w, affine_b;   // float
  DevBuf wrgb;   // float [3][C]
  DevBuf bias;   // float [3]
  DevBuf s;      // float [Bcap][C]      (s, wmod: the forward's workspace)
  DevBuf wmod;   // float [Bcap][3][C]
};

// what maua_synth_vjp keeps between calls (synth_vjp.hip); nothing of it exists on a network that only runs forwards
struct SynthVjpState {
  bool weights_ready = false;   // every ConvLayer.wg holds the weights now loaded
  DevBuf ws;                    // one set for bcap samples, carved into the pieces below (ensure_vjp)
  int bcap = 0;
  void* gfeat[2] = {nullptr, nullptr};   // gradients of two neighbouring feature tensors (network dtype)
  float* gimg[2] = {nullptr, nullptr};   // gradient of the skip image at two neighbouring resolutions
  void* g_u = nullptr;
  void* g_t = nullptr;
  float* g_xm = nullptr;
  float* part = nullptr;
  float* g_d = nullptr;
  float* g_s = nullptr;      // [B][max channels]
  float* g_wmod = nullptr;   // [B][3][max channels]
  DevBuf npart;              // maua_synth_vjp_ex with g_noise: float [B][max Co / 32 x pixels] per-group channel sums (allocated on first use)
  int npart_bcap = 0;
};

// the forward's workspace for bcap samples, beside the layers' own s / d / feat / wmod: dropped as a whole when a grid or an option changes
struct SynthWorkspace {
  int bcap = 0;
  DevBuf act[2];
  DevBuf img[2];       // float
  DevBuf rgb_tmp[2];   // float
  DevBuf style_table;  // StyleLayer []
  UnitStyles ones;     // [bcap][max channels] (kernels that take already-modulated input)
  DevBuf xm;           // [bcap] pre-modulated copy of an up-layer's input when its producer could not scale it
  DevBuf tbuf;         // [bcap] transposed-conv tensor of the largest up-layer
  DevBuf lowres_xm;    // [bcap] modconv_lowres workspaces (premodulated input, split-K partial sums: float)
  DevBuf lowres_ws;
  DevBuf const_rs;     // resized const input (rs_layer == 0)
};

}  // namespace maua

struct maua_synth {
  maua_ctx* ctx;
  int res, w_dim, channel_base, channel_max, dtype, nv_compat;
  int nblocks, num_ws;
  size_t esize;
  std::vector<maua::ConvLayer> convs;
  std::vector<maua::RgbLayer> rgbs;
  maua::DevBuf const_x;  // NHWC [4][4][C0]
  int keep_features = 0;
  int lowres = 1;      // <= 8x8 layers as one batch-wide split-K GEMM (option "lowres")
  int use_hires = 1;   // weights-in-registers kernels for the 512^2 / 1024^2 layers (bf16 / f16)
  int upwalk = 2;      // ... and their 64 -> 32 channel up-layer on the half-folded row walk (modconv_upwalk.hip);
                       // 2: the last block as one fused walk when nothing else reads its features
  int walk_segs = 0;   // fused walk: force this many row segments (0: cost model); walk_narrow: a <= 32-column last strip as two
  int walk_narrow = 1; // half-height sub-items walked at once (options "walk_segs" / "walk_narrow"; results do not depend on either)
  int fuse_torgb = 1;  // toRGB + skip fused into those conv1 epilogues
  int tconv_up = 1;    // up-layers: minimal transposed conv + separate FIR/epilogue pass (0 = 4 phase kernels)
  int tconv_fir = 256; // up-layers with inputs of at least this size: transposed conv + FIR + epilogue in ONE kernel, t stays in
                       // LDS (modconv_tconv_fir.hip); 0 = never.  Measured at B = 128 (pair -> fused): 256^2 inputs 3.61 -> 3.48 ms,
                       // 128^2 2.33 -> 2.62, 64^2 1.89 -> 2.65: the 1.42x MACs pay only where the t round trip was HBM-bound.
  int tconv_walk = 1;  // ... as a walk down 30-column strips that carries three t rows from step to step (0 = the tile form, which
                       // recomputes a one-position frame: 1.27x the steps' K-loop work); same bits (option "tconv_walk")
  const float* nz_scales = nullptr;   // [num_layers][nz_scale_stride] per-sample noise factors (maua_synth_set_noise_scale) or NULL
  long nz_scale_stride = 0;
  int dma_conv = 1;    // conv1 layers behind such an up-layer: LDS-direct-load kernel on pre-modulated input (bf16 / f16)
  int dual_store = 1;  // ... whose toRGB is a separate pass (512 channels): plain + style-scaled output in one epilogue (no premod pass)
  int tconv_dma = 1;   // the up-layers' transposed conv on LDS-direct loads (main block; pre-modulated input) + the dedicated
                       // edge kernel for the last row / column (0: the register-staged transposed conv)
  // one feature-space resize (wrappers/stylegan2.py:104-151): rs_layer = -1 none, 0 = before layer 0, L = after layer L-1
  int rs_layer = -1, rs_mode = 0, rs_th = 0, rs_tw = 0, rs_pl = 0, rs_pr = 0, rs_pt = 0, rs_pb = 0, rs_how = 3;
  float rs_value = 0.f;
  maua::DevBuf rs_noise;       // float [C][th][tw] fill noise, or empty
  int out_h = 0, out_w = 0;    // final image
  // geometric transform hooks (wrappers/stylegan2.py:153-194): up to 3 warps, applied in slot order after their layer
  int warp_layer[3] = {-1, -1, -1};
  const float* warp_minv[3] = {nullptr, nullptr, nullptr};  // device [B][6], owned by the caller
  // profile mode: HIP events recorded on the ctx stream around every launch of a forward
  int profile = 0;
  std::vector<hipEvent_t> ev;
  size_t ev_used = 0;
  std::vector<size_t> ev_fwd_start;
  maua::SynthWorkspace wk;
  float fir[16];
  // the last forward that kept its features (maua_synth_vjp differentiates exactly that one): its batch (0 = none), whether it ran
  // with per-sample noise factors, and whether an option, a weight load or a resize came after it
  int kept_B = 0;
  bool kept_scaled = false, kept_stale = false;
  maua::SynthVjpState vjp;
};
