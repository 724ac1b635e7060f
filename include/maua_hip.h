/* libmaua_hip.so — C ABI of the MI355X (gfx950) audio-reactive StyleGAN2 render path.
 *
 * This is the drop-in boundary.  The reference (maua-maua-maua/maua) has no compiled plugin
 * interface in-tree; its innermost replaceable surface is the Python operator layer
 * maua/GAN/wrappers/inference/ops.py (upstream equivalent: the CUDA plugins of
 * nv/torch_utils/ops, bound through torch_utils.custom_ops.get_plugin).  Each entry point below
 * names the reference interface it replaces (file:line relative to the reference root).
 *
 * Conventions
 *  - plain C: pointers + sizes, no C++/torch types.  All tensor pointers are DEVICE pointers in the
 *    address space of ctx's device; the caller owns every buffer it passes in, the library owns only
 *    the context workspaces and the parameters uploaded with maua_synth_load().
 *  - every call returns MAUA_OK (0) or a negative error; maua_last_error() returns a thread-local text.
 *  - launches are asynchronous on the ctx stream; the only synchronising calls are maua_ctx_sync(),
 *    maua_synth_load() (host->device upload) and the *_host helpers that say so.
 *  - a ctx is confined to one host thread at a time; different ctxs are independent.
 *  - dtype: MAUA_F32 (exact-f32 MFMA path, parity mode), MAUA_BF16 (bf16 operands, f32 accumulate: the bench dtype, every fast
 *    kernel) or MAUA_F16 (IEEE half operands, f32 accumulate - the reference's own render dtype, render/ffmpeg.py:45 and
 *    wrappers/__init__.py fp16=True; the operator layer and maua_synth_* take it on the generic MFMA kernels, with ops.py:161-165's
 *    pre-normalisation of weights and styles; the diffusion / up-scaler networks do not).
 */
#ifndef MAUA_HIP_H
#define MAUA_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MAUA_OK 0
#define MAUA_ERR (-1)

enum maua_dtype { MAUA_F32 = 0, MAUA_BF16 = 1, MAUA_F16 = 2,
                  /* float32 tensors whose products run on the bf16 matrix cores as three split products (x = hi + lo, both bf16:
                   * hi_w hi_x + lo_w hi_x + hi_w lo_x, f32 accumulate; ~2^-17 per product - between TF32's 2^-11, the CUDA default for
                   * the reference's fp32 convolutions, and exact f32).  Accepted by maua_secondary_create only. */
                  MAUA_F32_SPLIT = 3 };
/* activation ids: reference ops.py:9-19 / :44-62 */
enum maua_act {
  MAUA_ACT_LINEAR = 0, MAUA_ACT_RELU = 1, MAUA_ACT_LRELU = 2, MAUA_ACT_TANH = 3, MAUA_ACT_SIGMOID = 4,
  MAUA_ACT_ELU = 5, MAUA_ACT_SELU = 6, MAUA_ACT_SOFTPLUS = 7, MAUA_ACT_SWISH = 8
};
/* gaussian_filter padding modes: reference signal.py:108-157 (F.pad modes) */
enum maua_pad_mode { MAUA_PAD_CIRCULAR = 0, MAUA_PAD_REFLECT = 1, MAUA_PAD_REPLICATE = 2, MAUA_PAD_CONSTANT = 3 };

typedef struct maua_ctx maua_ctx;
typedef struct maua_synth maua_synth;
typedef struct maua_rrdbnet maua_rrdbnet;
typedef struct maua_unet maua_unet;
typedef struct maua_srvgg maua_srvgg;

/* ---- context (library plumbing: no reference counterpart — the reference relies on torch's current device and
 * stream; a maua_ctx carries exactly that: device ordinal, HIP stream, a scratch arena) --------------------------- */
const char* maua_version(void);
const char* maua_last_error(void);
/* stream: a hipStream_t (NULL = the device's default stream); pass torch's current stream handle. */
int maua_ctx_create(int device, void* stream, maua_ctx** out);
int maua_ctx_set_stream(maua_ctx* ctx, void* stream);
int maua_ctx_sync(maua_ctx* ctx);
/* kernel-selection switches for A/B measurements and parity tests (no reference counterpart).
 * "dma_conv" (default 1): maua_modconv2d runs eligible shapes (bf16, 3x3, up 1, Ci % 64 == 0, Co % 128 == 0,
 * H % 8 == 0, W % 32 == 0) on the LDS-direct-load kernel of the synthesis hot path. */
int maua_ctx_set_option(maua_ctx* ctx, const char* key, int value);
/* Measurement aid (bench.py `sustained_sclk_mhz`): enqueue a one-thread kernel on the ctx stream that writes two device counters
 * to stamp_dev[0..1] (device memory, 2 x u64): [0] the shader-cycle counter (ticks with the power-managed shader clock), [1] the
 * constant-rate 100 MHz counter.  Two stamps around a region: (d[0] / d[1]) x 100 MHz = the average shader clock inside it.
 * No reference counterpart (the reference publishes no throughput measurement). */
int maua_ctx_clock_stamp(maua_ctx* ctx, unsigned long long* stamp_dev);
void maua_ctx_destroy(maua_ctx* ctx);

/* ---- B1: operator layer (NCHW contiguous, like the reference tensors) --------------------------- */
/* replaces the tensor additions of SynthesisBlock.forward, inference/stylegan2.py:360 (`x = y + x`, "resnet") and :373
 * (`img = img + y`) for callers that run the network one layer at a time: out = a + b over n elements, summed in f32 and
 * rounded to dtype (F32 / BF16); out may alias a or b. */
int maua_add(maua_ctx* ctx, const void* a, const void* b, void* out, long n, int dtype);
/* replaces ops.py:65-84 bias_act (upstream plugin nv/torch_utils/ops/bias_act).
 * y = clamp(act(x + b[c]) * gain); b may be NULL; clamp < 0 disables clamping. */
int maua_bias_act(maua_ctx* ctx, const void* x, const float* b, void* y, int N, int C, int H, int W, int dtype,
                  int act, float alpha, float gain, float clamp);
/* replaces ops.py:87-114 upfirdn2d (upstream plugin nv/torch_utils/ops/upfirdn2d).
 * f: [fh,fw] f32 2-D filter (correlation, no flip); gain multiplies f (caller passes the 2-D gain,
 * i.e. reference gain**(f.ndim/2) already resolved).  Output size
 * Ho = (H*up + py0 + py1 - fh) / down + 1 (likewise Wo); y must hold [N,C,Ho,Wo]. */
int maua_upfirdn2d(maua_ctx* ctx, const void* x, const float* f, int fh, int fw, void* y, int N, int C, int H, int W,
                   int dtype, int up, int down, int px0, int px1, int py0, int py1, float gain);
/* replaces ops.py:146-186 modulated_conv2d + :189-233 conv2d_resample (+ optionally the bias_act that
 * always follows it, stylegan2.py:238-250 / :270-271), fused.
 * x [N,Ci,H,W], weight [Co,Ci,k,k] f32 (k = 1 or 3), styles [N,Ci] f32, noise [N|1,1,H*up,W*up] f32 or NULL
 * (noise_batch_stride = 0 broadcasts), bias [Co] f32 or NULL, y [N,Co,H*up,W*up].
 * up in {1,2}; for up == 2 the filter is the 4x4 [1,3,3,1] outer product /64 with gain 4 (ops.py:211-225).
 * flip_weight = 1 gives the upstream-NVIDIA kernel flip.  act/gain/clamp as maua_bias_act;
 * pass act = MAUA_ACT_LINEAR, gain = 1, clamp = -1, bias = NULL for the bare modulated_conv2d. */
int maua_modconv2d(maua_ctx* ctx, const void* x, const float* weight, const float* styles, const float* noise,
                   long noise_batch_stride, float noise_strength, const float* bias, void* y, int N, int Ci, int Co,
                   int H, int W, int k, int up, int demodulate, int flip_weight, int act, float alpha, float gain,
                   float clamp, int dtype);
/* replaces render/ffmpeg.py:72 (.add(1).div(2)) + ops/io.py:47-70 tensor2bytes:
 * u8 = round_half_even(clamp((x+1)/2, 0, 1) * 255), NCHW f32 [B,3,H,W] -> HWC u8 [B,H,W,3]. */
int maua_pack_rgb8(maua_ctx* ctx, const float* img, uint8_t* out_hwc, int B, int H, int W);
/* ops/io.py:47-70 tensor2bytes itself, any value range and channel count (ops/video.py:66 feeds every frame of a
 * VideoWriter through it): u8 = round_half_even((clamp(x, mn, mx) - mn) / (mx - mn) * 255), NCHW f32 [B,C,H,W] -> HWC u8.
 * The range is double like the Python scalars: mx - mn is formed in double and then rounded to f32, every other step is f32. */
int maua_tensor2bytes(maua_ctx* ctx, const float* img, uint8_t* out_hwc, int B, int C, int H, int W, double value_min,
                      double value_max);

/* ---- B2: synthesis network (parameters uploaded once, batched forwards) ------------------------- */
/* replaces inference/stylegan2.py:385-436 SynthesisNetwork(w_dim, img_resolution, img_channels=3,
 * channel_base, channel_max), 'skip' architecture, conv_clamp 256.
 * dtype: activation/operand type.  nv_compat: bit0 flip up-layer kernels (Q2), bit1 scale noise by
 * the loaded noise_strength instead of 1 (Q4). */
int maua_synth_create(maua_ctx* ctx, int img_resolution, int w_dim, int channel_base, int channel_max, int dtype,
                      int nv_compat, maua_synth** out);
void maua_synth_destroy(maua_synth* net);
int maua_synth_num_ws(const maua_synth* net);      /* SynthesisNetwork.num_ws, inference/stylegan2.py:409-427 */
int maua_synth_num_layers(const maua_synth* net);  /* synthesis layers in execution order (17 at 1024^2) */
/* options: "keep_features" (0/1) keeps every layer's activation for maua_synth_get_feature (parity/debug);
 * "profile" (0/1) records HIP events on the ctx stream around every launch of a forward;
 * kernel routing, for A/B comparisons and parity tests (every value computes the same network, up to rounding):
 * "tconv_up" (default 1) runs up-layers with 32^2..512^2 inputs as the minimal stride-2 transposed convolution + a
 * FIR/epilogue pass (0 = four 3x3 phase kernels everywhere, 4x the MACs; v > 1 = every up-layer with input size <= v);
 * "tconv_dma" (default 1) runs that transposed convolution on LDS-direct loads (0 = register-staged kernel);
 * "tconv_fir" (default 256) fuses it with the FIR/epilogue pass from this input size up (0 = never);
 * "tconv_walk" (default 1) lets that fused kernel walk down its column strips (0 = overlapping tiles; same bits);
 * "dma_conv" (default 1) runs the conv1 behind such an up-layer on LDS-direct loads, on pre-modulated input;
 * "dual_store" (default 1) lets a conv1 with a separate toRGB pass also store its output pre-modulated for the next up-layer;
 * "use_hires" (default 1) / "fuse_torgb" (default 1) select the register-stationary high-resolution kernels and
 * the toRGB fusion (0 = generic kernels everywhere);
 * "upwalk" (default 2) runs the 64 -> 32 channel up-layer as a row walk (1: on its own; 2: the last block as one fused
 * walk; 0 = off);
 * "walk_segs" (default 0 = cost model) / "walk_narrow" (default 1) shape that fused walk;
 * "lowres" (default 1) runs the <= 8x8 layers as one batch-wide GEMM. */
/* ---- arbitrary output sizes (maua/GAN/wrappers/stylegan2.py:104-151 change_output_resolution and
 * :216-340 get_hook).  The feature map is resized at ONE layer and every later layer runs at the scaled size.
 *  layer:  the reference's index into layer_names (0 = pre-hook on bs.0.conv1's input, L >= 1 = forward hook on
 *          the L-th entry, i.e. synthesis layer L-1 in execution order); -1 removes the resize.
 *  mode 0 "stretch": bicubic (align_corners False) to (target_h, target_w); the block's toRGB output is resized back
 *          and the block's image forward again, as the reference's rgb / img hooks do.
 *  mode 1 "pad-<how>-<where>": F.pad by (pad_left, pad_right, pad_top, pad_bottom) with pad_how (maua_pad_mode) /
 *          pad_value; inverse = crop.  Negative entries crop, as F.pad does - at layer 0 only (the pre-hook, :294): behind a
 *          later layer the reference's toRGB inverse slices with negative bounds and its forward fails (:278, :313-323).
 *  fill_noise_host: optional [C][target_h][target_w] f32 added to the resized FEATURES (the reference draws it once
 *          per hook from the per-channel mean/std of the first resized batch, :233-248; the caller owns the RNG).
 * Later layers need noise of their new size: maua_synth_layer_size reports it, maua_synth_load accepts a noise_const of
 * exactly that size. */
int maua_synth_set_resize(maua_synth* net, int layer, int mode, int target_h, int target_w, int pad_left, int pad_right,
                          int pad_top, int pad_bottom, int pad_how, float pad_value, const float* fill_noise_host);
/* geometric transform hooks (wrappers/stylegan2.py:153-194 apply_translation / apply_zoom / apply_rotation = kornia
 * translate / scale / rotate with padding_mode="reflection"): after layer `layer` (1-based index into layer_names) the
 * features are warped per sample, bilinear, reflection-padded, align_corners=True.  inv_matrices_dev [B][6] maps an
 * OUTPUT pixel (x, y) to its SOURCE pixel (row-major 2x3, device, owned by the caller and read by the next forwards);
 * NULL clears the slot.  Slots 0..2 on the same layer run in slot order (the reference registers translate, zoom,
 * rotate in that order). */
int maua_synth_set_warp(maua_synth* net, int slot, int layer, const float* inv_matrices_dev);
/* output size (h, w) of synthesis layer `layer` (execution order), or of the final image for layer == -1 */
int maua_synth_layer_size(const maua_synth* net, int layer, int* h, int* w);
/* the torch ops the hooks are made of, on NCHW tensors (dtype f32 / bf16): mode 0 = F.interpolate(x, (out_h, out_w),
 * mode="bicubic", align_corners=False); mode 1 = F.pad with left/top offsets (negative = crop), out size given;
 * mode 2 = bicubic with align_corners=True (maua/ops/image.py:240, the post-render resample).  dtype f32 / bf16 / f16.  Circular
 * padding wraps as often as it takes (torch refuses a pad larger than the input; reflect padding as large as the input is refused
 * here as there).  Checked by name: NULL or aliased x / y, any negative size, H or W of 0 with a non-empty output, mode, pad_how, dtype.
 * N, C, out_h or out_w of 0: nothing is done. */
int maua_resize2d(maua_ctx* ctx, const void* x, void* y, int N, int C, int H, int W, int out_h, int out_w, int mode,
                  int pad_left, int pad_top, int pad_how, float pad_value, int dtype);
/* depthwise 1-D correlation of planar f32 [planes][H][W] along rows (axis 0) or columns (axis 1) with reflect padding
 * `radius` (taps [2*radius+1], device): the lanczos pre-filter of maua/ops/image.py:226-236 resample.  0 <= radius < the axis's
 * length; x != y; a negative planes, H or W is refused, one of them 0 does nothing (the same for the vjp below). */
int maua_conv1d_reflect(maua_ctx* ctx, const float* x, float* y, const float* taps, int radius, int axis, long planes,
                        int H, int W);
/* the adjoints of the two steps of `resample` (maua/ops/image.py:214-240) - what autograd gives a loss taken on a resampled image
 * (LPIPSGrads, maua/grad.py:191-192): gy -> gx through the reflect-padded 1-D correlation / through the bicubic interpolation
 * (gy device f32 [N][C][out_h][out_w] -> gx [N][C][H][W]; align_corners as maua_resize2d's mode 2 / 0; gy != gx; negative sizes are
 * refused, N, C, H or W of 0 does nothing, out_h or out_w of 0 with a non-empty gx is refused) */
int maua_conv1d_reflect_vjp(maua_ctx* ctx, const float* gy, float* gx, const float* taps, int radius, int axis, long planes, int H, int W);
int maua_resize2d_bicubic_vjp(maua_ctx* ctx, const float* gy, float* gx, int N, int C, int H, int W, int out_h, int out_w, int align_corners);
int maua_synth_set_option(maua_synth* net, const char* key, int value);
/* the load_state_dict of the inference modules (inference/stylegan2.py:195-436 parameter / buffer names).
 * name: the reference state_dict key ("bs.3.conv0.weight", "bs.0.const", "bs.2.torgb.affine.bias",
 * "bs.1.conv1.noise_const", optional "bs.1.conv1.noise_strength").  host_data: HOST f32 array.
 * Synchronous.  Unknown names return MAUA_ERR ("resample_filter" buffers are accepted and checked). */
int maua_synth_load(maua_synth* net, const char* name, const float* host_data, size_t count);
/* the same with the values in DEVICE memory (e.g. drawn by maua_philox_normal): no host round trip for the large tensors */
int maua_synth_load_device(maua_synth* net, const char* name, const float* dev_values, size_t count);
/* replaces wrappers/stylegan2.py:65-102 StyleGAN2Synthesizer.forward + G_synth.forward(noise_mode="const").
 * ws [B,num_ws,w_dim] f32; noise: NULL or array of num_layers pointers, entry l = f32 [B|1, h_l, w_l] (or NULL
 * for that layer's noise_const), noise_batch_stride[l] in elements (0 = broadcast); img_out f32 [B,3,R,R]. */
int maua_synth_forward(maua_synth* net, const float* ws, const float* const* noise, const long* noise_batch_stride,
                       int B, float* img_out);
/* same, plus the u8 pack fused behind it (render/ffmpeg.py:72 + ops/io.py:47-70); img_out may be NULL. */
int maua_synth_render_rgb8(maua_synth* net, const float* ws, const float* const* noise,
                           const long* noise_batch_stride, int B, float* img_out, uint8_t* rgb8_out);
/* profile mode: per-launch durations (ms) of every forward since the last read, in launch order per forward:
 * styles, then per block [conv0 (two entries — transposed conv, FIR pass — when it runs as tconv_up),] conv1, torgb,
 * then pack_rgb8 if requested.  Synchronises on the last event;
 * a call with ms_out != NULL resets the recording (ms_out == NULL only returns the count). */
int maua_synth_get_profile(maua_synth* net, float* ms_out, int capacity, int* count);
/* Per-sample factors on the noise inputs of the NEXT maua_synth_render_rgb8 call - that one call only: it forgets them when it
 * returns (also on an error), so one batch's factors cannot leak into a later forward.  scales = device [num_layers][layer_stride >=
 * B] f32, row l for synthesis layer l (maua_noise_loop_batch_raw's output), or NULL for plain noise (x + noise * strength,
 * ops.py:184-185). */
int maua_synth_set_noise_scale(maua_synth* net, const float* scales, long layer_stride);
/* debug/parity (what a torch forward hook on SynthesisLayer would capture): copy layer l's activation (NHWC, net dtype) converted to f32 NCHW [B,C,h,w] after a forward. */
int maua_synth_get_feature(maua_synth* net, int layer, int B, float* out_nchw);
/* The gradient of the network to its latents, for the last forward that ran with option "keep_features" = 1 at this batch size
 * (that mode keeps every layer's output in its own buffer; the styles and demodulation coefficients of that forward are still in
 * the layers' buffers).  noise / noise_batch_stride: what that forward was given.  g_img: device f32 [B,3,R,R] = d loss / d img;
 * g_ws: device f32 [B,num_ws,w_dim] = d loss / d ws (overwritten).  The walk goes from the last block to the first through the
 * layer gradients below; gradients to biases and weights are not computed (to the noise inputs: maua_synth_vjp_ex).  The gradient convolutions' weights are made
 * from the loaded ones on the first call: a network that only runs forwards allocates nothing for this.  Two calls give the same
 * bits.  No reference counterpart in code (the reference uses torch.autograd, sampling/langevin.py:100-127). */
int maua_synth_vjp(maua_synth* net, const float* const* noise, const long* noise_batch_stride, int B, const float* g_img, float* g_ws);
/* The same walk, and the gradient to the noise inputs.  g_noise: NULL (then exactly maua_synth_vjp: the same kernels, the same bits), or
 * an array of num_layers device pointers, entry l = f32 gradient of layer l's noise map or NULL (not wanted: nothing is written).  With
 * the layer's v = d u + noise strength + bias: g_noise[l][b][p] = strength sum_co g_v[b][p][co].  g_noise_batch_stride[l] (NULL: h w for
 * every layer): h w = one map per sample; 0 = ONE map, the samples' gradients added in batch order (a shared input map, or the layer's
 * noise_const).  The channel sum rides in the pass that forms g_v (32 channels per workgroup, a fixed tree), the groups and the batch
 * are added in order by a second small kernel: no atomics, two calls give the same bits; g_ws has maua_synth_vjp's bits.  Refusals:
 * maua_synth_vjp_check's, and overlapping samples of a g_noise entry. */
int maua_synth_vjp_ex(maua_synth* net, const float* const* noise, const long* noise_batch_stride, int B, const float* g_img, float* g_ws,
                      float* const* g_noise, const long* g_noise_batch_stride);
/* host only: MAUA_OK if maua_synth_vjp would run; else MAUA_ERR and in maua_last_error() the cause - no kept forward of this batch
 * size; an option, a weight load or a resize after it; a resize or warp hook installed; an MAUA_F16 network; a forward that ran with
 * per-sample noise scales (maua_synth_set_noise_scale) */
int maua_synth_vjp_check(const maua_synth* net, int B);

/* ---- audio pre-pass (once per clip).  n_fft = 2048, hop = 1024, periodic Hann, centre/reflect padding ---- */
/* Spectra are FRAME-major: spec[frame][bin] complex64 (re, im interleaved), 1025 bins. */
int maua_stft_num_frames(int n_samples); /* 1 + n_samples / 1024: torch.stft centre framing, rosa/spectral.py:10-21 */
/* replaces rosa/spectral.py:10-21 stft (torch.stft).  y [n_samples] f32 -> spec [frames][1025] complex. */
int maua_stft(maua_ctx* ctx, const float* y, int n_samples, float* spec);
/* replaces rosa/spectral.py:24-32 istft (torch.istft, center=True, length=...).  -> y [length] f32. */
int maua_istft(maua_ctx* ctx, const float* spec, int n_frames, int length, float* y);
/* |spec|**power over n complex values (rosa/spectral.py:59-62 spectrogram, :113-117 magphase). */
int maua_magnitude(maua_ctx* ctx, const float* spec, long n, float power, float* mag);
/* replaces processing.py:75-85 median_filter2d as hpss calls it: window 31, reflect padding 15, along time
 * (axis 0, "harmonic") or along frequency (axis 1, "percussive") of mag [n_frames][n_bins]. */
int maua_median31(maua_ctx* ctx, const float* mag, int n_frames, int n_bins, int axis, float* out);
/* replaces rosa/spectral.py:145-161 hpss (+ :120-142 softmask): complex spec in, harmonic / percussive complex
 * spectra out (either may be NULL). */
int maua_hpss(maua_ctx* ctx, const float* spec, int n_frames, float margin, float power, float* harm_out,
              float* perc_out);
/* replaces rosa/spectral.py:65-70 melspectrogram(power=2): mel[m][f] = sum_k basis[m][k] |spec[f][k]|^2 for
 * f < n_frames_used (the reference drops the last STFT column).  basis [n_mels][1025], mel [n_mels][n_frames_used]. */
int maua_mel_power(maua_ctx* ctx, const float* spec, int n_frames_used, const float* basis, int n_mels, float* mel);
/* replaces rosa/convert.py:7-12 power_to_db (in place on mel) + rosa/beat.py:13-21: env[f] = mean_m relu(dB lag-1
 * difference), left-padded by pad_width zeros, cropped to T. */
int maua_onset_from_mel(maua_ctx* ctx, float* mel_inout, int n_mels, int T, float amin, float top_db, int pad_width,
                        int aggregate /* 0 = torch.mean (beat.py:10), 1 = torch.median(...).values (:44) */, float* env);
/* the same transforms with any power-of-two n_fft <= 2048, any hop and the caller's window (device, [n_fft]):
 * rosa/beat.py:33-39 fourier_tempogram = stft(onset_envelope, n_fft=win_length, hop_length=1) and the istft of
 * :67.  spec [1 + n_samples / hop][n_fft / 2 + 1] complex64, frame-major. */
int maua_stft_general(maua_ctx* ctx, const float* y, int n_samples, int n_fft, int hop, const float* window_dev,
                      float* out_frames_bins_complex);
int maua_istft_general(maua_ctx* ctx, const float* spec_frames_bins_complex, int n_frames, int n_fft, int hop,
                       const float* window_dev, int length, float* y);
/* rosa/beat.py:50-64 (plp steps 3-4) in place on a frame-major tempogram: zero the bins whose tempo (tempo_freq_dev
 * [n_bins], BPM) lies outside [tempo_min, tempo_max], keep only the bins at each frame's peak of log1p(1e6 |z|), divide
 * by finfo.tiny ** 0.5 + the frame's largest magnitude. */
int maua_plp_select(maua_ctx* ctx, float* tempogram_frames_bins_complex, int n_frames, int n_bins,
                    const float* tempo_freq_dev, float tempo_min, float tempo_max);
/* the autocorrelation tempogram behind selfsupervised/mir.py:27-30 (rosa.beat.tempo -> librosa.feature.tempogram,
 * un-vendored: published algorithm): ac[f][l] = sum_n (w[n] e[f+n]) (w[n+l] e[f+n+l]) for l < n_lags <= win, over the
 * n_frames hop-1 frames of env_padded [n_frames + win - 1] (the caller pads the envelope by win/2 ramp samples). */
int maua_autocorr_frames(maua_ctx* ctx, const float* env_padded, const float* window, int n_frames, int win,
                         int n_lags, float* ac_frames_lags);
/* ---- beats and Laplacian segmentation (selfsupervised/mir.py:31-41; features/rosa/segment.py) ----
 * mir.py:31 rosa.beat.beat_track(onset_envelope, trim=False, hop_length=1024, bpm=tempo): librosa is un-vendored, this is
 * its published dynamic program (librosa.beat.__beat_local_score + __beat_track_dp).  onset_norm [T] = envelope / its
 * std(ddof=1); period = round(60 * frame_rate / bpm) frames.  Outputs (device): localscore [T] f64 = the envelope
 * smoothed by exp(-0.5 (32 m / period)^2), cumscore [T] f64, backlink [T] i32 (best predecessor frame, negative = none).
 * The caller walks the links back from the last beat (host; maua_amd.segment.beats_from_links). */
int maua_beat_dp(maua_ctx* ctx, const float* onset_norm, int T, int period, double tightness, double* localscore,
                 double* cumscore, int* backlink);
/* segment.py:152-155 beat-synchronous feature: out[s][c] = lower median (mode 0, torch.median) or mean (mode 1,
 * librosa.util.sync of :241) of x[bounds[s] .. bounds[s+1])[c]; x [T][C] f32, bounds [n_segments + 1] i32 on the device */
int maua_segment_reduce(maua_ctx* ctx, const float* x, int T, int C, const int* bounds, int n_segments, int mode,
                        float* out);
/* segment.py:23-57 recurrence_matrix(data, k, width, sym=True): rec [n][n] = exp(-d / bandwidth) on the k nearest rows of
 * every column (|i - j| < width excluded), symmetrised by the minimum, bandwidth = lower median of the row maxima */
int maua_recurrence_affinity(maua_ctx* ctx, const float* data, int n, int d, int k, int width, float* rec);
/* segment.py:74-82 timelag_median_filter: median of 7 along the diagonals (time-lag domain), out != rec, 3 < n <= 16384
 * (the limit of maua_recurrence_affinity, which produces rec) */
int maua_timelag_median(maua_ctx* ctx, const float* rec, int n, float* out);
/* segment.py:60-64 median_filter1d as :193 applies it: window k (odd, <= 15) along the rows of x [n][m], reflect padding */
int maua_median_filter_rows(maua_ctx* ctx, const float* x, int n, int m, int k, float* out);
/* segment.py:106-131 differentiable_k_means on unit-norm rows data [n][k] from centres mu0 [k][k] (k <= 16): `iters`
 * updates mu = (r^T data) / sum r, r = softmax(temp * data mu^T); r_out [n][k], mu_out [k][k] */
int maua_soft_kmeans(maua_ctx* ctx, const float* data, int n, int k, const float* mu0, int iters, float temp, float* r_out,
                     float* mu_out);
/* ---- constant-Q features (rosa/constantq.py:13-115, rosa/spectral.py:164-325, rosa/pitch.py) ----
 * out[i] = scale * sum_k taps[k] x[i * stride + k - left] (zero outside the signal): one phase of torchaudio's sinc
 * resampler - what constantq.py:92 `resample(y, sr, sr / 2, "kaiser_window")` computes (torchaudio un-vendored:
 * published kernel, built by the caller). */
int maua_fir_decimate(maua_ctx* ctx, const float* x, long n, const float* taps, int ntaps, int stride, int left,
                      float scale, float* out, long n_out);
/* replaces audioreactive/audio.py:96-112 low_pass / high_pass / band_pass (scipy.signal.sosfilt over the decoded clip, float64)
 * and the lfilter under the biquads of selfsupervised/features/processing.py:142-151.  sos_host [n_sections][6] = b0 b1 b2 a0 a1 a2
 * per section (HOST array, scipy's layout), x / y [n] device float64 (y may be x); zero initial state.  Every section is scipy's
 * direct form II transposed sample for sample; the clip is cut into 128-sample chunks whose start states come from a scan. */
int maua_sosfilt(maua_ctx* ctx, const double* sos_host, int n_sections, const double* x, long n, double* y);
/* replaces processing.py:154-155 contrast_enhance (torchaudio.functional.contrast, un-vendored: the published formula)
 * y = sin(t + enhancement_amount / 750 * sin(4 t)), t = x pi / 2;  enhancement_amount in [0, 100]. */
int maua_contrast(maua_ctx* ctx, const float* x, long n, float enhancement_amount, float* y);
/* torch.istft's overlap-add (rosa/spectral.py:24-32) for already-windowed time frames [n_frames][W]: y[t] =
 * sum_f frames[f][t + start - f hop] / sum_f window[t + start - f hop]^2, t < length.  Used by the tempogram of clips
 * shorter than win_length (rosa/beat.py:48-49, 66: a non-power-of-two transform, run as a DFT GEMM). */
int maua_overlap_add(maua_ctx* ctx, const float* frames, int n_frames, int W, int hop, const float* window_dev, long start,
                     long length, float* y);
/* spectral.py:193-232 spline_eval (+ step_function when apply_step): out = step(a + f (b + f (c + f d))) with the
 * interval picked like torch.bucketize; knots [n_knots], coef [4][n_knots - 1] (a, b, c, d rows), all device f32. */
int maua_spline_step(maua_ctx* ctx, const float* x, long n, const float* knots, const float* coef, int n_knots, float h,
                     float alpha, int apply_step, float* out);
/* pitch.py:27-87 piptrack on the frame-major magnitude [n_frames][n_bins]; frame_max [n_frames] = max over bins,
 * freqs [n_bins] = the bin frequencies the band test compares (the caller's linspace), bin_hz = sr / n_fft;
 * pitch / mag [n_frames][n_bins] receive the interpolated frequency (Hz) and magnitude at accepted peaks, 0 elsewhere. */
int maua_piptrack(maua_ctx* ctx, const float* mag_frames_bins, int n_frames, int n_bins, const float* frame_max,
                  float threshold, const float* freqs, float bin_hz, float fmin, float fmax, float* pitch, float* mag);
/* replaces processing.py:53-56 normalize (eps = 1e-8) and signal.py:27-38 normalize (eps = 0):
 * y = (x - min) / ((max - min) + eps) over all n elements. */
int maua_normalize(maua_ctx* ctx, const float* x, long n, float eps, float* y);
/* replaces features/audio.py:31-37 rms: out[f] = sqrt(mean(frame_f^2)), centred reflect-padded frames. */
int maua_rms(maua_ctx* ctx, const float* y, int n_samples, int frame_length, int hop, int n_frames, float* out);
/* replaces signal.py:108-157 / processing.py:11-49 gaussian_filter: depthwise correlation along axis 0 of
 * x [T][C] with taps [2*radius+1] (built by the caller exactly as the reference builds its kernel), padding
 * min(radius,T) samples with `mode` (maua_pad_mode) and the rest by replication.  x and y must not alias. */
int maua_gaussian_filter1d(maua_ctx* ctx, const float* x, const float* taps, int radius, int T, long C, int mode,
                           float* y);
/* exact order statistics of the non-NaN (and, if mask != NULL, mask[i] != 0) elements of x[n]:
 *  mode 0: midpoint quantile with float32 q — replaces efficient_quantile.cpp:86-206 as __init__.py:6-7 calls it;
 *  mode 1: k-th smallest value, k 1-based — replaces signal.py:41-52 percentile's kthvalue;
 *  mode 2: torch.quantile(x, q) (linear interpolation, float32 rank arithmetic) — latent.py:37.
 * out3 (device) = {result, x_(lo), x_(hi)}; ranks2 (device, may be NULL) = {lo, hi} 0-based, -1 when empty. */
int maua_order_stat(maua_ctx* ctx, const float* x, const uint8_t* mask, long n, int mode, float q, long k,
                    float* out3, long long* ranks2);
/* ---- further audio features (selfsupervised/features/audio.py) ----
 * c [M][N] = a [M][K] x b [N][K]^T (f32).  Replaces rosa/spectral.py:35-56 dct (as a cosine-basis product, used by
 * audio.py:65-70 mfcc) and the phi @ chroma product of audio.py:50-62 tonnetz. */
int maua_matmul_nt(maua_ctx* ctx, const float* a, const float* b, float* c, int M, int N, int K);
/* mapping network (inference/stylegan2.py:116-192) around its matmul_nt + bias_act layers: the prologue normalize_2nd_moment
 * (ops.py:142-143: y = x / sqrt(mean(x^2, dim 1) + eps), x [P][D]) and the epilogue w.unsqueeze(1).repeat(1, n, 1)
 * (:183; out [P][n][D]) - so that the once-per-clip mapper needs no kernel outside this library. */
int maua_normalize_2nd_moment(maua_ctx* ctx, const float* x, int P, int D, float eps, float* y);
int maua_repeat_rows(maua_ctx* ctx, const float* x, int P, int D, int n, float* out);
/* replaces audio.py:118-126 spectral_flatness on the frame-major complex STFT spec [n_frames][n_bins]:
 * out[f] = exp(mean(log(max(amin, |z|^power)))) / mean(max(amin, |z|^power)). */
int maua_spectral_flatness(maua_ctx* ctx, const float* spec, int n_frames, int n_bins, float amin, float power,
                           float* out);
/* the per-band part of audio.py:76-115 spectral_contrast: for every frame sort |spec[f][lo..hi)| ascending
 * (torch.sort :107) and return the mean of the first k (valley, :109) and of the last k (peak, :110); hi - lo <= 1024.
 * The band edges / k follow the reference's float32 linspace comparisons and are computed by the caller. */
int maua_band_sorted_means(maua_ctx* ctx, const float* spec, int n_frames, int n_bins, int lo, int hi, int k,
                           float* valley, float* peak);
/* out2 (device) = {min(x), max(x)} over n elements (processing.py:134-136). */
int maua_minmax(maua_ctx* ctx, const float* x, long n, float* out2);
/* replaces processing.py:133-139 emphasize on xn = (x - min) / max(x - min) (maua_normalize with eps 0):
 * y = xn * (1 + tanh(strength * (xn - q))) * (max - min) + min; minmax_dev = {min, max} of x, q_dev = the quantile
 * of xn (maua_order_stat mode 2), both device scalars. */
int maua_emphasize(maua_ctx* ctx, const float* xn, long n, const float* minmax_dev, const float* q_dev, float strength,
                   float* y);
/* signal.py:84-105 compress / expand before their normalise: y = x * ratio where x > threshold (invert: x < threshold) */
int maua_threshold_scale(maua_ctx* ctx, const float* x, long n, float threshold, float ratio, int invert, float* y);
/* latent.py:46-51 on same-shape operands: mode 0 eerp a^(1-t) * b^t, mode 1 copeerp a^t (1 - b^t) / (1 - a^t + b^t) */
int maua_eerp(maua_ctx* ctx, const float* a, const float* b, const float* t, long n, int mode, float* y);
/* signal.py:69-76: mask[i] = x[i] > x[i+1] && x[i] > x[i-1] with neighbours clamped to the ends. */
int maua_peak_mask(maua_ctx* ctx, const float* x, int n, uint8_t* mask);
/* y = min(max(x, lo), hi + hi_add); lo = lo_dev[0] if lo_dev else lo_const; hi = hi_dev[0] (device scalars,
 * e.g. from maua_order_stat).  processing.py:59-62 standardize, signal.py:78 percentile_clip. */
int maua_clamp(maua_ctx* ctx, const float* x, const float* lo_dev, const float* hi_dev, float lo_const, float hi_add,
               long n, float* y);

/* ---- latent schedules (once per clip); tensors are [T][C] f32 with C = num_ws * w_dim ------------------- */
/* replaces latent.py:83-92 spline_loops / selfsupervised/latent.py:7-13 spline_loop_latents (the spline itself:
 * un-vendored torchcubicspline = natural cubic spline).  t_knots_host [n] and t_eval_host [T] are HOST f64 arrays
 * (strictly increasing knots); y [n][C] and out [T][C] are device f32.  Synchronises once (uploads the grids). */
int maua_spline_natural(maua_ctx* ctx, const double* t_knots_host, int n, const float* y, long C,
                        const double* t_eval_host, int T, float* out);
/* replaces latent.py:12-18 single_weighted: out[t] = a[t]*(1-env[t]) + b[t]*env[t]; a/b row strides in elements
 * (0 broadcasts one [C] row over time). */
int maua_latent_blend(maua_ctx* ctx, const float* a, long a_tstride, const float* b, long b_tstride, const float* env,
                      int T, long C, float* out);
/* replaces latent.py:21-31 multi_weighted: out[t] = sum_a (env[t][a]/sum_a' env[t][a']) * latents[a % n].
 * A <= 16384 (one row of env is staged in LDS), refused otherwise. */
int maua_weighted_sum(maua_ctx* ctx, const float* env, const float* latents, int T, int A, int n, long C, float* out);
/* latent.py:38-40: idx = int64(round_half_even(x * scale)) — the onset-bin assignment (bit-exact). */
int maua_scale_round_index(maua_ctx* ctx, const float* x, float scale, long n, long long* idx);
/* latent.py:41: out[t] = src[idx[t]] (rows of C floats); a negative index counts from the end, as numpy's does.
 * Precondition (not checked: the indices live on the device): every idx[t] lies in [-n_rows, n_rows). */
int maua_gather_rows(maua_ctx* ctx, const float* src, const long long* idx, int n_rows, int T, long C, float* out);
/* replaces signal.py:5-24 resample / F.interpolate(mode="linear", align_corners=False) along axis 0: torch's formula with every
 * operation rounded once.  A build of torch that fuses scale * (j + 0.5) - 0.5 or the final l0 x0 + l1 x1 into multiply-adds
 * (its CPU kernels do where the compiler contracts) differs from this by those roundings: an ulp of the source position. */
int maua_resample_linear(maua_ctx* ctx, const float* x, int n, long C, int size, float* out);
/* replaces latent.py:54-65 slerp: y [n_seg+1][L][D], t [k] -> out [k][n_seg][L][D] (unit-normalised, Q9). */
int maua_slerp(maua_ctx* ctx, const float* y, const float* t, int k, int n_seg, int L, int D, float* out);
/* replaces selfsupervised/latent.py:57-78: merge `sequence` into layers [l0,l1) of latents [T][L][D] in place;
 * mode 0 average, 1 modulate by mod[t], 2 overwrite. */
int maua_latent_merge(maua_ctx* ctx, float* latents, const float* sequence, const float* mod, int mode, int T, int L,
                      int D, int l0, int l1);

/* ---- per-batch noise (selfsupervised patch) ----------------------------------------------------- */
/* replaces selfsupervised/noise.py:42-53 Loop.forward(i, b): planes [3,h,w] f32 (the module's randn buffer),
 * idx [T] f32 (= linspace(0, 2*pi*n_loops, T)), frames i0..i0+B-1 ->
 * out[b] = sin(cos(idx[i0+b] + n0) / (sigma/50) + n1) * n2, divided by its per-frame RMS + eps(f32).  out [B,h,w].
 * Alignment: when h*w is a multiple of 4 the kernels move 16 bytes at a time, so `planes` and `out` must be 16-byte aligned
 * (every plane and every frame then is); any other h*w takes a scalar path and needs 4-byte alignment only.  This holds for
 * all three Loop entry points, per layer.  sigma != 0; B <= 65535 and, batched, at most 24 layers per call (refused
 * otherwise).  The sine and cosine are the library's own short forms, held to 4 x the float32 libm deviation for
 * |argument| <= 1e4 (idx + n0 and 50 / sigma + n1 stay far below that for sigma >= 0.05). */
int maua_noise_loop(maua_ctx* ctx, const float* planes, const float* idx, int i0, int B, int h, int w, float sigma,
                    float* out);
/* the same for n Loop modules (one per synthesis layer) in three launches (maua_noise_loop is its n = 1: the same bits);
 * its factor 1 / (rms + eps) comes from the same partial sums as maua_noise_loop_batch_raw's scales; host arrays of n device pointers / sizes;
 * out[l] receives [B, h[l], w[l]].  What selfsupervised/sample.py:93-95 does per batch with 17 module calls. */
int maua_noise_loop_batch(maua_ctx* ctx, int n, const float* const* planes, const float* const* idx, const int* h,
                          const int* w, const float* sigma, int i0, int B, float* const* out);
/* replaces noise.py:11-24 Blend.forward (noise2 != NULL: sum_m noise[m]*mod[b,m] + sum_m noise2[m]*(1-mod[b,m]))
 * and :27-39 Multiply.forward (noise2 == NULL).  noise/noise2 [M,h,w], mod [B,M] (rows i..i+B of the modulator).
 * M <= 16384 (one row of the modulator is staged in LDS) and B <= 65535, refused otherwise. */
/* The same maps UN-NORMALISED in one pass + the per-(layer, sample) factor 1 / (rms + eps) that noise.py:52 divides by:
 * scales [n][B] f32 (device).  Hand the maps to the synthesis call as usual and the factors through maua_synth_set_noise_scale:
 * the consuming convolution epilogues multiply them into their noise strength, so the maps are written once and sin(cos(.)) is
 * evaluated once per value (the normalised form needs two passes).  Same reference lines as maua_noise_loop_batch. */
int maua_noise_loop_batch_raw(maua_ctx* ctx, int n, const float* const* planes, const float* const* idx, const int* h,
                              const int* w, const float* sigma, int i0, int B, float* const* out, float* scales);

int maua_noise_mix(maua_ctx* ctx, const float* noise, const float* noise2, const float* mod, int M, int B, int h,
                   int w, float* out);
/* replaces noise.py:56-63 Average (mode 0: (x+y)/2), :66-75 Modulate (mode 1: x*mod[b] + y*(1-mod[b]), mod [B]),
 * :78-86 ScaleBias (mode 2: scale*x + bias).  x, y, out [B,h,w].  B <= 65535. */
int maua_noise_combine(maua_ctx* ctx, const float* x, const float* y, const float* mod, int mode, float scale,
                       float bias, int B, int h, int w, float* out);

/* ---- N4 (first slice): RealESRGAN x4 generator, the per-frame up-scaler of "StyleGAN2 render -> RealESRGAN 4x" ----
 * replaces maua/super/image/models/realesrgan.py:22-49 (basicsr RRDBNet(3, 3, num_feat, num_block, num_grow_ch, scale 4)
 * run by RealESRGANer.enhance: [0,1] image -> network -> clamp(0,1) -> round(x * 255)) and the per-frame loop of
 * maua/super/video/frame_by_frame.py:22-33.  basicsr / realesrgan are un-vendored: published architecture. */
int maua_rrdb_create(maua_ctx* ctx, int num_feat, int num_block, int num_grow_ch, int dtype, maua_rrdbnet** out);
void maua_rrdb_destroy(maua_rrdbnet* net);
/* name: a key of basicsr's RRDBNet state dict (conv_first.weight, body.3.rdb2.conv4.bias, conv_last.weight, ...);
 * weights are [Co][Ci][3][3], biases [Co], f32 on the host. */
int maua_rrdb_load(maua_rrdbnet* net, const char* name, const float* host_data, size_t count);
/* img: device f32 [B][3][H][W] in [0,1].  out_nchw: device f32 [B][3][4H][4W] clamped to [0,1] (or NULL);
 * out_rgb8: device u8 [B][4H][4W][3] = round(clamp * 255) (or NULL). */
int maua_rrdb_forward(maua_rrdbnet* net, const float* img_nchw, int B, int H, int W, float* out_nchw, uint8_t* out_rgb8);
/* the RRDB forward without the [0,1] clamp on out_nchw (RealESRGANer clamps AFTER its tile stitching / pre-pad crop; the
 * u8 output is always clamped).  clamp01 = 1 is maua_rrdb_forward. */
/* RealESRGANer.enhance (realesrgan utils; as super/video/frame_by_frame.py:22-33 applies it per frame) for a batch of device-resident
 * u8 frames [B][h][w][3] in one call: x / 255, reflect pre_pad on the right / bottom, the network, clamp, round(255 y), crop ->
 * out_rgb8 [B][4h][4w][3].  No separate convert / pad / crop passes (round 6). */
int maua_rrdb_enhance_u8(maua_rrdbnet* net, const uint8_t* frames, int B, int h, int w, int pre_pad, uint8_t* out_rgb8);
int maua_rrdb_forward_ex(maua_rrdbnet* net, const float* img_nchw, int B, int H, int W, int clamp01, float* out_nchw,
                         uint8_t* out_rgb8);

/* ---- N4: the "xsx4-animevideo" model of realesrgan.py:34-35: realesrgan's SRVGGNetCompact(3, 3, num_feat, num_conv,
 * upscale, act_type) - convolutions + PReLU, PixelShuffle, + nearest-upsampled input (un-vendored: published architecture).
 * act_type: 0 prelu, 1 relu, 2 leakyrelu(0.1).  Parameter names: body.<2k>.weight / .bias, body.<2k+1>.weight (PReLU). */
int maua_srvgg_create(maua_ctx* ctx, int num_feat, int num_conv, int upscale, int act_type, int dtype, maua_srvgg** out);
void maua_srvgg_destroy(maua_srvgg* net);
int maua_srvgg_load(maua_srvgg* net, const char* name, const float* host_data, size_t count);
/* img device f32 [B][3][H][W]; out_nchw device f32 [B][3][sH][sW] (clamped to [0,1] when clamp01) or NULL; out_rgb8 device u8
 * [B][sH][sW][3] = round(clamp * 255) or NULL */
int maua_srvgg_forward(maua_srvgg* net, const float* img_nchw, int B, int H, int W, int clamp01, float* out_nchw,
                       uint8_t* out_rgb8);

/* ---- N4 (second half): guided-diffusion UNet + DDIM, BASELINE configs[3] "guided-diffusion 256x256, 100-step DDIM" ------
 * replaces the network maua/diffusion/processors/guided.py:164-209 create_models builds (guided_diffusion.script_util.
 * create_model_and_diffusion: UNetModel with num_channels 256, num_res_blocks 2, attention_resolutions "32, 16, 8",
 * num_head_channels 64, learn_sigma, resblock_updown, use_scale_shift_norm) and, with maua_ddim_step, the
 * diffusion.ddim_sample(model, x, t, cond_fn=...) call that guided.py:277-339 GuidedDiffusion.forward loops over.  The
 * guided_diffusion submodule is EMPTY in the reference checkout: the published architecture / sampler are restated, parity
 * unpinned.  channel_mult: n_mult multipliers of model_channels per level; attention_ds: the down-sampling rates
 * (image_size // resolution) at which blocks carry attention; only the flag set of guided.py:171-190 is implemented
 * (use_scale_shift_norm, resblock_updown, legacy attention order, no class conditioning). */
int maua_unet_create(maua_ctx* ctx, int image_size, int in_channels, int model_channels, int out_channels, int num_res_blocks,
                     const float* channel_mult, int n_mult, const int* attention_ds, int n_attn, int num_head_channels,
                     int dtype, maua_unet** out);
void maua_unet_destroy(maua_unet* net);
/* number of named parameters the network expects (every key of UNetModel.state_dict() + "timestep_embedding.freqs") */
int maua_unet_param_count(maua_unet* net, long* count);
/* name: a key of guided_diffusion's UNetModel.state_dict() (input_blocks.4.0.in_layers.2.weight, middle_block.1.qkv.weight,
 * out.2.bias, time_embed.0.weight, ...), f32 on the host: 3x3 weights [Co][Ci][3][3], 1x1 weights [N][K][1(,1)], linear
 * weights [N][K], GroupNorm scale / shift [C].  Optional "timestep_embedding.freqs" [model_channels / 2]: the float32
 * frequency table of nn.py timestep_embedding as the host computes it (otherwise computed on the device). */
int maua_unet_load(maua_unet* net, const char* name, const float* host_data, size_t count);
/* "route": 0 per-shape routing of the 3x3 convolutions (default), 1 generic kernel only, 2 no split-K gather GEMM;
 * "psum_off": 1 = GroupNorm statistics always by their own pass over the tensor (default 0: where the LDS-direct convolution
 * produced the tensor, from the piece sums its epilogue left) */
int maua_unet_set_option(maua_unet* net, const char* key, int value);
/* UNetModel.forward(x, timesteps): x device f32 [B][in_channels][H][W], timesteps device f32 [B] (the value the wrapped
 * model of respace.py passes: original timestep index, rescaled to 0..1000), out device f32 [B][out_channels][H][W].
 * H, W: multiples of 2^(levels - 1). */
int maua_unet_forward(maua_unet* net, const float* x, const float* timesteps, int B, int H, int W, float* out);
/* Guidance speed "regular" (guided.py:214-218, 250-272): the loss gradient is taken THROUGH the diffusion UNet -
 * `torch.autograd.grad(img, x, img_grad)` with img a function of p_mean_variance(model, x, t)["pred_xstart"].  The library's
 * form of that autograd call: maua_unet_forward_keep = maua_unet_forward that leaves what the input gradient reads on the
 * network's arena (GroupNorm inputs and statistics, qkv, the attention rows' log-sum-exp), then
 * maua_unet_vjp: g_x [B][in_channels][H][W] = (d out / d x)^T g_out, g_out [B][out_channels][H][W] (device f32).
 * Back to back on one network, same shape; option "vjp" = 1 (maua_unet_set_option) BEFORE maua_unet_load, which then also
 * prepares every weight's transposed copy (3x3: transposed + spatially flipped - the gradient is the same MFMA convolution). */
int maua_unet_forward_keep(maua_unet* net, const float* x, const float* timesteps, int B, int H, int W, float* out);
int maua_unet_vjp(maua_unet* net, const float* g_out, int B, int H, int W, float* g_x);
/* gaussian_diffusion.py ddim_sample for an epsilon model, clip_denoised False (guided.py:303-306): x [B][C][HW], model_out
 * [B][Cm][HW] (first C channels = eps), cond_grad = cond_fn(x, t) [B][C][HW] or NULL (condition_score), noise or NULL
 * (eta 0), coef device f32 [B][8] = {sqrt_recip_alphas_cumprod, sqrt_recipm1_alphas_cumprod, sqrt(1 - alphas_cumprod),
 * sqrt(alphas_cumprod_prev), sqrt(1 - alphas_cumprod_prev - sigma^2), sigma * (t != 0), 0, 0} at each sample's t.
 * sample (may alias x) and pred_xstart (or NULL): [B][C][HW]. */
int maua_ddim_step(maua_ctx* ctx, const float* x, const float* model_out, const float* cond_grad, const float* noise,
                   const float* coef, int B, int C, int Cm, long HW, float* sample, float* pred_xstart);
/* gaussian_diffusion.py p_sample (guided.py:302-303, sampler "p"): ancestral step of an epsilon model with learned-range
 * variance (model_out [B][2 C][H][W]), clip_denoised False; cond_grad (or NULL): condition_mean.  noise [B][C][H][W].
 * coef: device f32 [B][8] = {sqrt_recip_alphas_cumprod, sqrt_recipm1_alphas_cumprod, posterior_mean_coef1,
 * posterior_mean_coef2, posterior_log_variance_clipped, log(betas), t != 0, 0}. */
int maua_p_sample_step(maua_ctx* ctx, const float* x, const float* model_out, const float* cond_grad, const float* noise,
                       const float* coef, int B, int C, long HW, float* sample, float* pred_xstart);
/* plms_sample (guided.py:308-311, sampler "plms"; the sampler of the guided-diffusion fork the reference vendors as an
 * empty submodule: published algorithm - pseudo linear multistep, Liu et al. 2022): one model evaluation -> eps (after the
 * optional condition_score), its pred_xstart, the unconditioned pred_xstart; coef = maua_ddim_step's table. */
int maua_plms_eps(maua_ctx* ctx, const float* x, const float* model_out, const float* cond_grad, const float* coef, int B,
                  int C, int Cm, long HW, float* eps, float* pred_xstart, float* pred_xstart_orig);
/* ... and the update: eps' = (sum_i weights[i] eps_list[i]) / divisor (n_eps <= 4; host arrays of device pointers / floats), pred' from
 * eps', sample = (pred' sqrt(ac_prev) + sqrt(1 - ac_prev) eps') (t != 0) + pred_xstart (t == 0).  coef: device f32 [B][8] =
 * {sqrt_recip_ac, sqrt_recipm1_ac, sqrt(ac_prev), sqrt(1 - ac_prev), t != 0, 0, 0, 0}. */
int maua_plms_update(maua_ctx* ctx, const float* x, const float* const* eps_list, const float* weights, int n_eps,
                     float divisor, const float* pred_xstart, const float* coef, int B, long chw, float* sample);
/* out[b] = ab[b][0] * x[b] + ab[b][1] * y[b] over rows of `row` floats: q_sample (guided.py:331, gaussian_diffusion.py) */
int maua_axpby_rows(maua_ctx* ctx, const float* x, const float* y, const float* ab, int B, long row, float* out);
/* 1 when the last maua_ddim_sample_loop(use_graph = 1) replayed a captured hipGraph, 0 when it ran launch by launch */
int maua_unet_graph_active(maua_unet* net, int* active);

/* ---- secondary diffusion model: the network behind the reference's DEFAULT guidance speed ("fast")
 * Replaces maua/diffusion/processors/guided.py:68-143 (SecondaryDiffusionImageNet2.forward -> DiffusionOutput(v, pred, eps)) and the
 * torch.autograd.grad(img, x, img_grad) of GradientGuidedConditioning.forward (:236-272), which differentiates through it: the library
 * has no autograd, so the vector-Jacobian product is evaluated on the transposed network (csrc/secondary.hip).
 * Convolutions are numbered 0..23 in execution order (maua_amd/diffusion.py maps the reference's state-dict keys).
 * forward: x [B][3][H][W] f32, t [B] f32 (the cosine-schedule time in [0, 1]); H, W multiples of 32; any of v / pred / eps may be NULL.
 * vjp: g_v = d loss / d v  ->  g_x = (d v / d x)^T g_v, using the activations of the LAST forward (same B, H, W).  Device pointers. */
typedef struct maua_secondary maua_secondary;
int maua_secondary_create(maua_ctx* ctx, int dtype, maua_secondary** out);
void maua_secondary_destroy(maua_secondary* net);
int maua_secondary_conv_shape(int index, int* ci, int* co);
/* what: 0 = weight [Co][Ci][3][3] (host), 1 = bias [Co], 2 = timestep_embed.weight [8] (index ignored) */
int maua_secondary_load(maua_secondary* net, int index, int what, const float* host_data, size_t count);
int maua_secondary_forward(maua_secondary* net, const float* x, const float* t, int B, int H, int W, float* v_out, float* pred_out,
                           float* eps_out);
int maua_secondary_vjp(maua_secondary* net, const float* g_v, int B, int H, int W, float* g_x);
/* operator-level forms of the small kernels that hold the guided-diffusion path together, for parity tests (no reference counterpart
 * of their own): each launches the kernel the networks run, through the launcher the networks use.  Device pointers; a size of zero
 * does nothing; refused with the entry point's name: a negative size, an unknown dtype, C that is not whole 16-byte pieces, a pixel
 * stride below C, odd H or W where a 2 x 2 window is read, dim < 2.
 * nn.py timestep_embedding: t [B] -> e [B][dim] = [cos(t f_i) | sin(t f_i)] (i < dim / 2; a zero last column when dim is odd), the
 * argument t f_i a float32 product; freqs: the float32 table f_i = exp(-ln(10000) i / (dim / 2)) [dim / 2], or NULL: computed on the
 * device. */
int maua_timestep_embedding(maua_ctx* ctx, const float* t, const float* freqs, int B, int dim, float* e);
/* the timestep MLP's and every ResBlock's emb_layers' row product, all f32: y [B][N] = act_out(W [N][K] . act_in(x [B][K]) + bias [N]);
 * act 0 = none, 1 = SiLU (v / (1 + exp(-v))); bias may be NULL */
int maua_linear_rows(maua_ctx* ctx, const float* x, const float* W, const float* bias, int B, int K, int N, int act_in, int act_out,
                     float* y);
/* the secondary model's glue (csrc/secondary.hip), NHWC tensors in dtype (MAUA_F32 or MAUA_BF16; a bf16 store is one round to nearest
 * even of the f32 value), pixel strides in elements.
 * input: x [B][3][HW] f32, t [B], wemb [8] -> out [B][HW][32] = [x | cos(2 pi t w_k) | sin(2 pi t w_k) | 13 zeros]
 * output: vn [B][HW][32] (3 real channels), x, t -> planar f32 [B][3][HW] v, pred = x cos(t pi / 2) - v sin(t pi / 2), eps = x sin + v cos;
 * any of the three may be NULL */
int maua_secondary_input(maua_ctx* ctx, const float* x, const float* t, const float* wemb, int B, long HW, int dtype, void* out);
int maua_secondary_output(maua_ctx* ctx, const void* vn, const float* x, const float* t, int B, long HW, int dtype, float* v, float* pred,
                          float* eps);
/* AvgPool2d(2): C channels at src (pixel stride src_stride) of the [B][H][W] grid -> dense dst [B][H / 2][W / 2][C]; H, W even */
int maua_avgpool2_nhwc(maua_ctx* ctx, const void* src, long src_stride, int B, int H, int W, int C, int dtype, void* dst);
/* F.interpolate(scale_factor=2, mode="bilinear", align_corners=False): dense src [B][h][w][C] -> C channels at dst (pixel stride
 * dst_stride) of the [B][2 h][2 w] grid; and its adjoint: gout (pixel stride g_stride, [2 h][2 w]) -> dense gin [B][h][w][C], zeroed
 * where the stored activation act (dense like gin; NULL: no mask) is not above 0.  Every product and sum rounds once. */
int maua_bilinear_up2_nhwc(maua_ctx* ctx, const void* src, int B, int h, int w, int C, int dtype, void* dst, long dst_stride);
int maua_bilinear_up2_nhwc_vjp(maua_ctx* ctx, const void* gout, long g_stride, const void* act, int B, int h, int w, int C, int dtype,
                               void* gin);
/* ReLU's gradient in place: dense g [n_pix][C] zeroed where act (pixel stride act_stride) is not above 0 */
int maua_relu_mask_nhwc(maua_ctx* ctx, void* g, const void* act, long act_stride, long n_pix, int C, int dtype);
/* where a skip leaves: out [B][H][W][C] (dense) = act > 0 ? gcat + 0.25 gpool[y / 2][x / 2] : 0; gcat, act: C channels at pixel stride
 * cat_stride of the [B][H][W] grid; gpool dense [B][H / 2][W / 2][C]; H, W even */
int maua_skip_grad_nhwc(maua_ctx* ctx, const void* gcat, const void* act, long cat_stride, const void* gpool, int B, int H, int W, int C,
                        int dtype, void* out);
/* the gradient's two layout kernels: to_nhwc 1: planar f32 src [B][3][HW] -> dst [B][HW][32] in dtype (channels 3.. zero); 0: src
 * [B][HW][32] in dtype -> planar f32 dst [B][3][HW] */
int maua_secondary_grad_layout(maua_ctx* ctx, const void* src, int B, long HW, int dtype, int to_nhwc, void* dst);
/* operator-level forms of the UNet's building blocks, NHWC tensors in `dtype` (guided_diffusion/unet.py, nn.py):
 * QKVAttentionLegacy.forward - qkv [B][T][3 * heads * head_ch] with channel = head * 3 ch + {q | k | v} * ch + c (what
 * `qkv.reshape(bs * n_heads, ch * 3, length).split(ch, dim=1)` sees) -> out [B][T][heads * head_ch]; head_ch 32 or 64 */
int maua_attention_legacy(maua_ctx* ctx, const void* qkv, void* out, int B, int T, int heads, int head_ch, int dtype);
/* the same with CLIP's causal mask (build_attention_mask: triu(-inf, 1) - query t attends to keys 0 .. t), the text tower's
 * attention; same layouts, head_ch 32 or 64; forward only */
int maua_attention_causal(maua_ctx* ctx, const void* qkv, void* out, int B, int T, int heads, int head_ch, int dtype);
/* its input gradient (autograd through QKVAttentionLegacy.forward): d_out [B][T][heads * head_ch] -> d_qkv like qkv */
int maua_attention_legacy_vjp(maua_ctx* ctx, const void* qkv, const void* d_out, void* d_qkv, int B, int T, int heads, int head_ch,
                              int dtype);
/* the fused attention kernels behind the three entry points above, the diffusion UNet and both CLIP towers with every launch argument
 * in the caller's hand, for parity tests (no reference counterpart).  Per (sample b, head h), rows t of qkv at (b T + t) ld_qkv + 3 h
 * head_ch + {0 | head_ch | 2 head_ch}: out[(b T + t) ld_out + h head_ch + c] = sum_j softmax_j(scale q_t . k_j) v_j[c], with causal != 0
 * over the keys j <= t only; lse (optional, float [B][heads][T]): log sum_j exp(scale q_t . k_j), what the gradient rebuilds the
 * weights from.  Strides in elements of dtype (MAUA_F32 or MAUA_BF16).  Checked: head_ch 32 or 64, T > 0, B and heads <= 65535, qkv
 * and out 16-byte aligned, ld_qkv >= 3 heads head_ch and ld_out >= heads head_ch, both whole 16-byte pieces.  B == 0: nothing is done. */
typedef struct {
  const void* qkv; void* out; float* lse;
  int B, T, heads, head_ch; long ld_qkv, ld_out;
  float scale; int causal; int dtype;
} maua_attn_desc;
/* the input gradient: d_out (laid out like out) -> d_qkv (like qkv).  out and lse are operands: the forward's result and log-sum-exp
 * rows as the caller has them; delta: float workspace [B][heads][T], left holding the rows' d_out . out.  The same checks, on every
 * pointer; causal != 0 is refused (there is no gradient of the causal forward). */
typedef struct {
  const void* qkv; const void* out; const void* d_out; const float* lse; void* d_qkv; float* delta;
  int B, T, heads, head_ch; long ld_qkv, ld_out;
  float scale; int causal; int dtype;
} maua_attn_vjp_desc;
/* host only, no device needed: MAUA_OK, or MAUA_ERR + maua_last_error() with the launcher's own message.  Pointers are only checked,
 * never dereferenced. */
int maua_attention_check(const maua_attn_desc* d);
int maua_attention_vjp_check(const maua_attn_vjp_desc* d);
/* launch on the context's stream (the gradient: its three kernels); refused, with no launch, as the check refuses */
int maua_attention_ex(maua_ctx* ctx, const maua_attn_desc* d);
int maua_attention_vjp_ex(maua_ctx* ctx, const maua_attn_vjp_desc* d);
/* conv_nd(1, K, N, 1) / a linear layer over rows (AttentionBlock.qkv / proj_out + residual, ResBlock.skip_connection):
 * c[M][N] = a[M][K] x w[N][K]^T + bias[N] (+ res[M][N]); K % 32 (bf16) / 16 (f32) == 0, N % 32 == 0 */
int maua_linear_nt(maua_ctx* ctx, const void* a, const void* w, const float* bias, const void* res, void* c, long M, int N,
                   int K, int dtype);
/* kernel-selection switches of the GEMM behind maua_linear_nt and the UNet / CLIP / perceptor layers, for parity tests (no
 * reference counterpart).  c[m][n] = sum_k A[m][k] w[n][k] (+ bias[n]) (+ res[m][n]), A's columns [0, K0) from a0 (row stride lda0)
 * and [K0, K0 + K1) from a1 (lda1); w [N][K0 + K1] dense; res [M][ldr]; c [M][ldc]; strides in elements of dtype (MAUA_BF16 or
 * MAUA_F32).  epi (bf16, kernels 3 and 4 only): 1 = c2[m][n] <- QuickGELU(c[m][n]) as well (row stride ldc2); 2 = c <- c *
 * QuickGELU'(aux[m][n]) (ldaux).  batch > 1: that many products of one A source, no bias, no residual, a0 / w / c of product b
 * at + b * a_bstride / w_bstride / c_bstride elements (batch <= 65535, strides whole 16-byte pieces).  Always checked: K0, K1
 * whole 64-byte chunks, N % 32 == 0, lda0 / lda1 whole 16-byte pieces, ldc % 4 == 0, a0, a1, w, bias, c, res, c2, aux 16-byte aligned.
 * Kernels: 1 = 64 x 128 register-staged (any such shape, f32 or bf16, epi 0); 2 = 128 x 128 register-staged (K parts whole
 * 128-byte chunks, ldc / ldr 16-byte pieces, epi 0); 3 = 256 x 128 LDS-direct (bf16, batch 1, K parts whole 64-channel chunks,
 * N % 128 == 0, ldc / ldr / ldc2 / ldaux % 8 == 0, M lda0 2, M lda1 2 and N (K0 + K1) 2 below 2^32 bytes); 4 = 256 x 256
 * LDS-direct (as 3, plus K1 == 0 and N % 256 == 0).  Production routing adds thresholds that are about occupancy only, never
 * about correctness: kernel 2 needs M >= 128; kernels 3 / 4 need prefer_dma, M >= 256 and at least 256 tiles of 256 x 128 (3) /
 * 256 x 256 (4) - and take 4 over 3 unless the environment sets MAUA_GEMM_DMA_128.  A forced kernel drops exactly these. */
typedef struct {
  const void* a0; long lda0; int K0;   const void* a1; long lda1; int K1;
  const void* w;  const float* bias;   const void* res; long ldr;
  void* c; long ldc; long M; int N;
  int epi; void* c2; long ldc2; const void* aux; long ldaux;
  int batch; long a_bstride, w_bstride, c_bstride;
} maua_gemm_desc;
/* host only, no device needed: the kernel (1 .. 4) the launch would run (force 0: production routing, prefer_dma as the ctx
 * option "linear_dma" / the CLIP tower set it), *remap_out its XCD remap (kernel 2: the number of N tiles whose M tile is kept on
 * one XCD, 0 = none; may be NULL); MAUA_ERR + maua_last_error() if refused.  Pointers are only checked, never dereferenced. */
int maua_gemm_nt_route(const maua_gemm_desc* d, int dtype, int prefer_dma, int* remap_out);
/* launch: force 0 = production routing, 1 .. 4 = that kernel, refused (no launch) when it cannot take the shape */
int maua_gemm_nt_ex(maua_ctx* ctx, const maua_gemm_desc* d, int dtype, int prefer_dma, int force);
/* kernel-selection switches of the plain 3x3 convolutions (padding 1) behind the diffusion UNet, the secondary model, the VGG
 * perceptors and the up-scalers, for parity tests (no reference counterpart).  One convolution, described as those networks describe
 * theirs; every tensor NHWC in `dtype` (MAUA_F32_SPLIT: float32 tensors), strides in elements, 0 = dense:
 *   v = clamp(act(sum_{tap, ci < Ci} w[co][ci][tap] x[b][p + tap][ci] + bias[co]) * gain)     (clamp < 0: none)
 *   y[b][p][y_coff + co] = v                                              without res
 *                        = T(v) + res[b][p][co]                           with res: the value as it would have been stored, plus res
 *                        = res_gain * T(T(v) + res) + res2[b][p][co]      with res2 as well (res2 needs res)
 * T = rounding to the 16-bit storage type (the identity for the float32 types); the result is rounded once more when it is stored.
 * x: x_pstride elements per pixel (>= Ci, 0 = Ci), x_bstride per sample; with x_up2 the tensor is [B][H / 2][W / 2] and the layer
 * sees it up-sampled x2 by pixel repetition.  w: DEVICE float32 [Co][Ci][3][3], bias DEVICE float32 [Co] or NULL; both are prepared
 * into the context's scratch arena on every call.  Ci_read (0 = Ci): input channels that are fetched at all - the weights of the
 * others must be zero (LDS-direct kernel: rounded up to whole 32-channel chunks, at least two).  psum (optional, LDS-direct wide tiles):
 * float [B][(H / 8) * (W / 32)][Co / 8][16] - per 8 x 32-pixel tile and 8-channel piece the 8 sums, then the 8 sums of squares, of
 * the values stored.  variant: 128 = the LDS-direct kernel's 128-channel tile although 256 would divide.  Ci, Co multiples of 32.
 * Kernels: 1 = generic (any such shape, every dtype; no x_up2 / psum / Ci_read); 2 = LDS-direct (MAUA_BF16: Ci % 64 == 0, Co % 128
 * == 0, H % 8 == 0, W % 32 == 0 - the wide tiles - or Co of 32 / 64, H >= 8, W >= 32, Ci % 64 == 0 or Co == 32 and Ci % 32 == 0, Ci >= 96 -
 * the narrow tiles, no psum; MAUA_F16: wide tiles only, no psum, no x_up2); 3 = split-K gather GEMM (MAUA_BF16 / MAUA_F32, H W <= 1024,
 * Ci a multiple of 128 bytes, Co % 128 == 0, dense x, one residual, none of x_up2 / psum / Ci_read). */
typedef struct {
  const void* x; int x_pstride; long x_bstride;
  const float* w; const float* bias;
  void* y; int y_pstride, y_coff; long y_bstride;
  const void* res; int res_pstride; long res_bstride;
  const void* res2; int res2_pstride; long res2_bstride; float res_gain;
  int B, H, W, Ci, Co;
  int act; float alpha, gain, clamp;
  int Ci_read, x_up2, variant;
  float* psum;
} maua_conv_desc;
/* host only, no device needed: the kernel (1 .. 3) the diffusion UNet runs this convolution on under its option "route" =
 * unet_route_option (0 per-shape routing, 1 always the generic kernel, 2 never the gather GEMM) - or, with unet_route_option = 100 +
 * k, kernel k as maua_conv3x3_ex forces it.  *variant (may be NULL): kernel 1 - which of its tile rules fires, 1 .. 9 in the order of
 * launch_modconv3x3's source (1 and 9: 256 pixels x 32 channels; 2 and 4: 256 x 128, 128-byte K chunks; 3: 256 x 128, 64-byte chunks;
 * 5 / 6: 128 x 128 with 128 / 64-byte chunks; 7: 256 x 64, 3-tap stages; 8: 256 x 64, 9-tap stages); kernel 2 - output channels per
 * workgroup, 256 / 128 / 64 / 32, + 1 for the 32-channel tile's odd-chunk form, + 2 for the piece-sum instantiations; kernel 3 - 0.
 * *ksplit (may be NULL): kernel 3's K slices, else 0.  MAUA_ERR + maua_last_error() (the launcher's own message) if the kernel refuses
 * the shape or the arguments.  Pointers are only checked, never dereferenced. */
int maua_conv3x3_route(const maua_conv_desc* d, int dtype, int unet_route_option, int* variant, int* ksplit);
/* launch on the context's stream: kernel 0 = the UNet's production routing (piece sums only where it takes the wide LDS-direct
 * tiles, its own choice of `variant`), 1 .. 3 = that kernel, refused (no launch, no fall-back) when it cannot take the shape or the
 * arguments */
int maua_conv3x3_ex(maua_ctx* ctx, const maua_conv_desc* d, int dtype, int kernel);
/* One operation of the ResNet backbone (csrc/resnet_conv.hip) with every argument in the caller's hand, for parity tests (no reference
 * counterpart).  Tensors dense NHWC in `dtype` (MAUA_F32: exact f32 products, or MAUA_BF16; any other dtype is refused):
 *   y[b][oh][ow][co] = act(sum_{r, s, ci} w[co][ci][r][s] x[b][oh stride - pad + r][ow stride - pad + s][ci] + bias[co] (+ res[b][oh][ow][co]))
 * pixels outside the image count as zero; act = ReLU (relu != 0) or none, applied AFTER the residual; the residual is read in `dtype`, the
 * sum is float32 and rounded once when stored.  Output size (H + 2 pad - k) / stride + 1.  (k, stride, pad) is one of (1, 1, 0),
 * (1, 2, 0), (3, 1, 1), (3, 2, 1) with Ci and Co multiples of 64 - or (7, 2, 3) with Ci = 3, the stem: x is then the PLANAR float32 image
 * [B][3][H][W] (no residual).  w: DEVICE float32 [Co][Ci][k][k], bias: DEVICE float32 [Co] or NULL; w is prepared into the context's
 * scratch arena on every call.  The summation order is a function of the shape alone.  Anything else is refused: MAUA_ERR +
 * maua_last_error(), no launch, no fall-back. */
typedef struct maua_sconv_desc {
  const void* x; const float* w; const float* bias; const void* res; void* y;
  int B, H, W, Ci, Co, k, stride, pad, relu;
} maua_sconv_desc;
int maua_conv_strided_ex(maua_ctx* ctx, const maua_sconv_desc* d, int dtype);
/* MaxPool2d(3, stride 2, padding 1) of NHWC x [B][H][W][C] -> y [B][(H - 1) / 2 + 1][(W - 1) / 2 + 1][C]: taps outside the image are
 * excluded (not zeros).  C % 8 == 0. */
int maua_maxpool3x3s2(maua_ctx* ctx, const void* x, void* y, int B, int H, int W, int C, int dtype);
/* AdaptiveAvgPool2d((1, 1)) + flatten of NHWC x -> out float32 [B][C]: the pixels summed in float32 in index order, then one multiply by
 * 1 / (H W).  C % 8 == 0. */
int maua_global_avgpool(maua_ctx* ctx, const void* x, float* out, int B, int H, int W, int C, int dtype);
/* kernel-selection switches of the MODULATED 3x3 convolutions of the StyleGAN2 synthesis network, for parity tests (no reference
 * counterpart).  One layer as the network's forward describes it, on the route of the caller's choice:
 *   v = clamp(act(d[b][co] * conv(x[b] * s[b], w)[co] + noise[b][p] * noise_strength * noise_scale[b] + bias[co]) * gain)
 * conv: up == 1 a 3x3 correlation with padding 1; up == 2 conv_transpose2d(stride 2) + the [1, 3, 3, 1] FIR with gain 4 (flip: the
 * weights are flipped first, the upstream behaviour).  y = T(v), or what the route makes of out_scale (the next layer's styles,
 * [B][Co]) and y_scaled (the dual store: y plain, y_scaled scaled).  x NHWC [B][H][W][Ci] in `dtype`, x_bstride elements between
 * samples (0: one sample for all); w DEVICE float32 [Co][Ci][3][3]; s [B][Ci], d [B][Co] or NULL: DEVICE float32, chosen by the caller;
 * noise float32 [B | 1][H up][W up] or NULL; y NHWC [B][H up][W up][Co].  Optional fused toRGB + skip (rgb_out != NULL):
 * rgb_out[b][c][p] = clamp(sum_co T(v)[co] rgb_wmod[b][c][co] + rgb_bias[c], rgb_clamp) + upsample2d(rgb_prev)[b][c][p], planar
 * float32; rgb8_out: the same image as u8 HWC; rgb_skip_f32: only the u8 frame; y == NULL: the features are not stored.
 * t (optional): where the transposed-convolution routes leave their intermediate [B][2H + 1][2W + 1][Co] (else scratch).
 * Routes (synth.hip's Route enum): 0 Lowres, 1 Generic, 2 DmaConv1, 3 Hires, 4 Upwalk, 5 FusedWalk (d1 = the block's conv1 with
 * its toRGB), 7 TconvFir, 8 TconvDma (edges + main + FIR / epilogue pass), 9 Tconv2 (+ FIR / epilogue pass), 10 the FIR / epilogue
 * pass alone (x = t).  Weights are prepared, and the input pre-multiplied where the route reads it so, exactly as the network does,
 * in the context's scratch arena on every call. */
typedef struct {
  const void* x; long x_bstride;
  const float* w; int flip;
  const float* s; const float* d;
  const float* noise; long noise_bstride; float noise_strength; const float* noise_scale;
  const float* bias;
  void* y;
  int B, H, W, Ci, Co, up;
  int act; float alpha, gain, clamp;
  const float* out_scale; void* y_scaled;
  const float* rgb_wmod; const float* rgb_bias; const float* rgb_prev; float* rgb_out; float rgb_clamp;
  unsigned char* rgb8_out; int rgb_skip_f32;
  void* t;
} maua_modconv_desc;
/* host only, no device needed: MAUA_OK if `route` can compute the layer - its *_supported predicate and every refusal of its
 * launchers, with the launcher's own message in maua_last_error() otherwise.  *tile (may be NULL): Generic - the tile rule, 1 .. 9;
 * DmaConv1 - output channels per workgroup; Lowres - its K slices; else 0.  Pointers are only checked, never dereferenced.
 * Not predicted here: the halo-register and LDS budgets that launch_modconv3x3 and launch_tconv2 check once their tile is laid out
 * (no shape with Ci, Co multiples of 32 exceeds them today); maua_modconv_ex meets those after the weights were prepared. */
int maua_modconv_route(const maua_modconv_desc* d, const maua_modconv_desc* d1, int dtype, int route, int* tile);
/* launch on the context's stream; refused (no launch, no fall-back) when the route cannot take the layer.  force_segs / narrow_ok:
 * the fused walk's row segments and narrow last strip (launch_upwalk_fused); on the tconv_fir route force_segs > 0 forces the row
 * segments of its strip walk and force_segs < 0 selects its tile form (synth option "tconv_walk" = 0); ignored elsewhere */
int maua_modconv_ex(maua_ctx* ctx, const maua_modconv_desc* d, const maua_modconv_desc* d1, int dtype, int route, int force_segs,
                    int narrow_ok);
/* the separate toRGB launch: out[b][c][p] = clamp(sum_ch x[b][p][ch] wmod[b][c][ch] + bias[c], clamp) + upsample2d(prev)[b][c][p];
 * x NHWC [B][H][W][C] in dtype, wmod [B][3][C], bias [3], prev [B][3][H / 2][W / 2] or NULL, out [B][3][H][W] float32 */
int maua_torgb_ex(maua_ctx* ctx, const void* x, const float* wmod, const float* bias, const float* prev, float* out, int B, int H,
                  int W, int C, float clamp, int dtype);
/* The gradient of one such layer to its input and its styles.  fwd: the layer exactly as maua_modconv_ex took it, with y = the output
 * that call left (the activation mask and the convolution result are recovered from it; the latter is not kept); act linear or
 * lrelu, no noise_scale / out_scale / y_scaled / fused toRGB.  g_y: d loss / d y, NHWC in `dtype` like y; g_x: d loss / d x
 * [B][H][W][Ci] in `dtype` (may be NULL); g_s: d loss / d s, DEVICE float32 [B][Ci], through the modulation and through d as the
 * demodulation coefficients of s (d[b][co] = rsqrt(sum_ci s^2 sum_taps W^2 + 1e-8); d == NULL: no such term).  The input-gradient
 * convolution runs on the matrix cores (bf16, or exact float32), up == 2 as a stride-2 implicit GEMM over the FIR adjoint of g_y.
 * Reductions run in a fixed order.  dtype: MAUA_F32 or MAUA_BF16 (MAUA_F16 is refused: its pre-normalisation is not differentiated). */
int maua_modconv_vjp_ex(maua_ctx* ctx, const maua_modconv_desc* fwd, const void* g_y, void* g_x, float* g_s, int dtype);
/* host only, no device needed: every refusal of maua_modconv_vjp_ex, with the same message.  Pointers are only checked. */
int maua_modconv_vjp_check(const maua_modconv_desc* fwd, const void* g_y, float* g_s, int dtype);
/* the gradient of maua_torgb_ex's y = clamp(x . wmod + bias, clamp) (recomputed for the clamp's mask; the skip image passes g_img
 * on unchanged): g_x [B][H][W][C] in `dtype` = (accumulate ? g_x : 0) + sum_c wmod[b][c][.] g_img[b][c][p] where |y| < clamp,
 * g_wmod DEVICE float32 [B][3][C] = sum_p x[b][p][.] g_img[b][c][p]; g_img DEVICE float32 [B][3][H][W]; C a multiple of 32 */
int maua_torgb_vjp_ex(maua_ctx* ctx, const void* x, const float* wmod, const float* bias, const float* g_img, void* g_x, float* g_wmod,
                      int B, int H, int W, int C, float clamp, int accumulate, int dtype);
int maua_torgb_vjp_check(const void* x, const float* wmod, const float* bias, const float* g_img, void* g_x, float* g_wmod, int B, int H,
                         int W, int C, int dtype);
/* the plan of the next forward (host only, no launch): per conv layer 7 ints {route, src (0 Kernel, 1 Producer, 2 Xm, 3 PremodPass),
 * scale_next, dual, rgb, rgb8, skip_store} into conv_out [capacity][7], per block its toRGB route (0 Separate, 1 Fused, 2 Hook) into
 * rgb_out [blocks]; *pack: the u8 frame is packed by its own launch.  Returns the number of conv layers through *n_layers. */
int maua_synth_get_plan(maua_synth* net, int want_u8, int* conv_out, int capacity, int* rgb_out, int* pack, int* n_layers);
/* GroupNorm32(32, C)(x) [* (1 + scale) + shift with scale_shift [B][2C] (ResBlock use_scale_shift_norm)] [-> SiLU];
 * statistics in float64, eps 1e-5.  x, y [B][H][W][C] */
int maua_group_norm_nhwc(maua_ctx* ctx, const void* x, const float* gamma, const float* beta, const float* scale_shift,
                         int silu, int B, int H, int W, int C, int dtype, void* y);
/* its input gradient, with the ResBlocks' resampling behind the activation (resample 0 none, 1 avg_pool2d 2, 2 nearest x2:
 * h_upd(in_rest(x)), unet.py ResBlock._forward): dy [B][Ho][Wo][C] -> dx [B][H][W][C]; dres (optional, shaped like dy): the
 * gradient of x_upd(x), the same resampling of the raw input, added */
int maua_group_norm_nhwc_vjp(maua_ctx* ctx, const void* x, const float* gamma, const float* beta, const float* scale_shift, int silu,
                             int resample, const void* dy, const void* dres, int B, int H, int W, int C, int dtype, void* dx);
/* the fused GroupNorm pass behind the two entry points above and every norm of the diffusion UNet, and its input gradient, with
 * every launch argument in the caller's hand, for parity tests (no reference counterpart).  Tensors NHWC in dtype (MAUA_F32 or
 * MAUA_BF16), 16 bytes = EPC elements (4 / 8) a piece.  The input is the virtual concatenation [x0 | x1] of [B][H][W][C0] and
 * [B][H][W][C1] (x1 NULL, C1 0: one source; the boundary may fall inside a group), C = C0 + C1:
 *   u = (x - mean) * rstd * gamma + beta;  ss != NULL: u = u * (1 + ss[b ss_ld + c]) + ss[b ss_ld + C + c];  silu: u = u sigmoid(u)
 *   y [B][Ho][Wo][C] = R(u): mode 0 the identity, 1 the 2x2 average (Ho = H / 2, Wo = W / 2, floored like avg_pool2d), 2 nearest x2;
 *   xr (optional, like y) = R(x), the ResBlock's x_upd.  Statistics per (sample, group of C / 32 channels) in float64, eps 1e-5.
 * ss_ld: floats between the samples' scale-shift rows - 0 (one row for all) or >= 2 C.  ps0 / ps1 (optional, bf16 only): the piece
 * sums maua_conv_desc.psum describes, float [B][rows][C_i / 8][16], left by the convolution that produced that source; the statistics
 * are taken from them when the group kernels run and every source has them, else from a pass over the tensor.  stats_out
 * (optional): float [B][32][2], left holding (mean, rstd).  force_route: 0 = as the network routes, 1 = the per-channel kernels.
 * Routes: 0 = group kernels (C / 32 a multiple of EPC and B * Ho <= 65535), 1 = per-channel kernels; both read the tensor in
 * chunks of ppc pixels, nchunk <= 128 per sample, RY = max(1, 512 / (C / EPC)) pixel rows per workgroup.
 * Checked: dtype; x0, gamma, beta, y non-NULL; B >= 0, H, W, C0 > 0; C % 32 == 0, C / EPC <= 1024, C0 % EPC == 0; x1 non-NULL when
 * C1 > 0; mode 0 .. 2, mode 1 needs H, W >= 2; ss_ld; every pointer and ss_ld whole 16-byte pieces; B <= 65535 and fewer than 2^31
 * pixels per sample; piece sums: bf16, H % 8 == 0, W % 32 == 0, C_i % 128 == 0, rows_i == (H / 8) * (W / 32).  B == 0: nothing is done. */
typedef struct {
  const void* x0; int C0; const void* x1; int C1; int B, H, W;
  const float* gamma; const float* beta; const float* ss; long ss_ld;
  int silu, mode; void* y; void* xr;
  const float* ps0; int rows0; const float* ps1; int rows1;
  float* stats_out; int force_route; int dtype;
} maua_gn_desc;
/* the input gradient: dy, dres (optional; the gradient of xr or of an identity skip) [B][Ho][Wo][C] -> dx0 [B][H][W][C0], dx1
 * [B][H][W][C1]; add0 / add1 (optional, may alias dx0 / dx1): gradients already known for x0 / x1, added.  stats: the forward's
 * [B][32][2] (mean, rstd), an operand.  The same checks, on every pointer, plus: dx1 non-NULL when C1 > 0; mode 1 needs even H and
 * W; H <= 65535.  The partial sums run RY = max(1, 256 / (C / EPC)) pixel rows per workgroup; the last kernel runs once per range of
 * 65535 / H samples. */
typedef struct {
  const void* x0; int C0; const void* x1; int C1;
  const float* stats; const float* gamma; const float* beta; const float* ss; long ss_ld;
  int silu, mode; const void* dy; const void* dres; const void* add0; const void* add1; void* dx0; void* dx1;
  int B, H, W; int dtype;
} maua_gn_vjp_desc;
/* host only, no device needed: MAUA_OK, or MAUA_ERR + maua_last_error() with the launcher's own message.  Pointers are only checked,
 * never dereferenced. */
int maua_group_norm_check(const maua_gn_desc* d);
int maua_group_norm_vjp_check(const maua_gn_vjp_desc* d);
/* host only: what the launch would run (any output pointer may be NULL); refused as the check refuses.  stats_source: 0 = a pass
 * over the tensor, 1 = the piece sums.  ranges: launches of the gradient's last kernel. */
int maua_group_norm_plan(const maua_gn_desc* d, int* route, int* RY, int* ppc, int* nchunk, int* stats_source);
int maua_group_norm_vjp_plan(const maua_gn_vjp_desc* d, int* RY, int* ppc, int* nchunk, int* ranges);
/* launch on the context's stream (workspaces from its scratch arena); refused, with no launch, as the check refuses */
int maua_group_norm_ex(maua_ctx* ctx, const maua_gn_desc* d);
int maua_group_norm_vjp_ex(maua_ctx* ctx, const maua_gn_vjp_desc* d);
/* the unconditioned sampling loop of guided.py:333-337 inside the library: n_steps x (forward + DDIM update) on x in place;
 * model_t host f32 [n_steps], coef host f32 [n_steps][8]; use_graph: capture the loop in one hipGraph and replay it. */
int maua_ddim_sample_loop(maua_unet* net, float* x, int B, int H, int W, const float* model_t, const float* coef, int n_steps,
                          int use_graph, float* pred_xstart);
/* the GUIDED sampling loop - configs[3] as BASELINE states it - inside the library, one hipGraph per shape.  Replaces the per-step
 * Python of maua/diffusion/processors/guided.py:302-311, 333-337 (diffusion.ddim_sample(..., cond_fn=self.conditioning)) with
 * cond_fn = GradientGuidedConditioning.forward at the reference's default speed "fast" (:236-272: secondary model forward, img =
 * pred * sigma + x * (1 - sigma), the grad modules' d loss / d img, torch.autograd.grad back through the secondary model) and an
 * image-MSE grad module (d loss / d img = (img - target) * mse_k; a result holding a NaN counts as zeros, :262-265).  Per step:
 * out = unet(x, t); pred = secondary(x, cos_t).pred; img; g; grad = c0 g + c1 (dv/dx)^T g; x, pred_xstart = ddim_step(x, out, grad).
 * model_t / coef as maua_ddim_sample_loop; guide: host f32 [n_steps][5] = {cos_t, sigma, 1 - sigma, -(sigma a_c + 1 - sigma),
 * sigma s_c} (the host evaluates them like :249-252, :266-268 do); target: device f32 [B][3][H][W] (target_bstride = 3 H W) or one
 * image for every sample (target_bstride = 0).  Both networks must have been created on the same context.
 * sec == NULL: speed "regular" (guided.py:214-218, 250-252) - img is built from THIS network's pred_xstart and the gradient goes back
 * through it: per step out = forward_keep(x, t); pred = ra x - rm eps (eps = the first in_channels of out); img; g; grad = c0 g +
 * c1 (d eps / d x)^T g (maua_unet_vjp); DDIM update.  guide[s] = {-, sigma, 1 - sigma, -(sigma ra + 1 - sigma), sigma rm}; option
 * "vjp" = 1 before the weights are loaded.  One hipGraph as well. */
int maua_ddim_guided_loop(maua_unet* net, maua_secondary* sec, float* x, int B, int H, int W, const float* model_t, const float* coef,
                          const float* guide, int n_steps, const float* target, long target_bstride, float mse_k, int use_graph,
                          float* pred_xstart);
/* 1 when the last maua_ddim_guided_loop(use_graph = 1) replayed a captured hipGraph, 0 when it ran launch by launch */
int maua_unet_guided_graph_active(maua_unet* net, int* active);
/* that grad module as an operator: out = (img - target) * k over B rows of `row` floats, zeros if the result holds a NaN
 * (guided.py:256-265 with an image-MSE loss); target_bstride = row or 0 */
int maua_mse_guide_grad(maua_ctx* ctx, const float* img, const float* target, long target_bstride, float k, int B, long row,
                        float* out);

/* ---- text-prompt guidance: CLIPGrads (configs[3]: "audio-onset-switched text prompts") ------------------------------------
 * Replaces maua/grad.py:96-165: per sampler step, `cutout_batches` x { MauaCutouts of the image estimate (maua/ops/cutouts.py:8-50),
 * Normalize, clip_model.encode_image (OpenAI CLIP VisionTransformer: un-vendored pip dependency, published architecture restated,
 * parity unpinned), spherical_dist_loss to the target embeddings (maua/loss.py:22-25), weights, mean over cutouts,
 * torch.autograd.grad(loss.sum() * scale, img) / cutout_batches }, clamp_gradient.  The gradient is evaluated on the transposed
 * network inside the library (csrc/clip.hip, clip_guide.hip, transformer.hip, cutouts.hip, gemm_dma.hip).  Target embeddings are handed in (set_targets :117-143,
 * computed once, off the loop): text prompts through the text tower below (maua_clip_text_*), image (style) targets with
 * maua_clip_encode_image.  dtype: MAUA_BF16 (the reference runs the perceptor in fp16) or MAUA_F32 (exact products, parity mode).
 * Parameter names: CLIP's state-dict keys below "visual." (conv1.weight, class_embedding, positional_embedding, ln_pre.*,
 * transformer.resblocks.<i>.{attn.in_proj_weight, attn.in_proj_bias, attn.out_proj.*, ln_1.*, mlp.c_fc.*, mlp.c_proj.*, ln_2.*},
 * ln_post.*, proj), host float32 in the checkpoint's layout. */
typedef struct maua_clip maua_clip;
int maua_clip_create(maua_ctx* ctx, int input_resolution, int patch_size, int width, int layers, int heads, int output_dim, int dtype,
                     maua_clip** out);
void maua_clip_destroy(maua_clip* net);
int maua_clip_load(maua_clip* net, const char* name, const float* host_data, size_t count);
/* Any patch size that divides the input: a patch row of 3 * patch_size^2 values is held at a stride rounded up to a multiple of 64
 * (ViT-L/14: 588 -> 640; 16 / 32-pixel patches: unchanged), zero-padded, so the patch embedding and its transpose stay plain GEMMs.
 * The cutouts of a guidance call go through the tower in groups: as many cutouts per pass as the kernels' index ranges and a byte
 * budget allow - kept activations + workspace per image (10 x [tokens][width] per layer: ViT-L/14 ~137 MB, @336px ~307 MB in bf16)
 * plus the cutouts' scratch.  bytes = 0 (default): the device's free memory when a guidance call (or the guided loop) first sees a
 * batch shape, plus what the tower already holds, less a reserve of 1/8 (at least 2 GiB); bytes > 0: that budget.  The group size
 * stays fixed for a batch shape / cutn until the limit changes; the gradient is the sum over groups in a fixed order.  One cutout
 * (B images) is never split: a budget below it is refused, with the bytes it needs in the message. */
int maua_clip_set_workspace_limit(maua_clip* net, size_t bytes);
/* VisionTransformer.forward (clip/model.py): images device f32 [N][3][R][R], already normalised -> embeds device f32 [N][E];
 * keep != 0 keeps the activations for maua_clip_encode_image_vjp: d_embeds [N][E] -> d_images [N][3][R][R] */
int maua_clip_encode_image(maua_clip* net, const float* images, int N, int keep, float* embeds);
int maua_clip_encode_image_vjp(maua_clip* net, const float* d_embeds, int N, float* d_images);
/* the buffers CLIPGrads.set_targets registers (:134-143): S sets of P target embeddings [S][P][E] (host or device; normalised here
 * as spherical_dist_loss does) with prompt weights [S][P] (already divided by |sum|, :139-143); sel: host [B] - the set each sample
 * of a batch is guided towards (prompts switched per frame by the clip's onsets) - or NULL: set 0 for every sample */
int maua_clip_set_targets(maua_clip* net, const float* targets, const float* weights, int S, int P, const int* sel, int B);
/* CLIPGrads.forward (:145-159): img device f32 [B][3][H][W] in [-1, 1]; rects HOST int [batches][cutn][3] = (size, top, left) of
 * every cutout of every cutout batch (the host draws them like MauaCutouts.forward does); grad device f32 [B][3][H][W];
 * clamp_gradient <= 0: none; a result holding a NaN is returned as zeros (guided.py:262-265).
 * mult: NULL, or HOST float [batches][cutn] - cutout i stands for mult[i] IDENTICAL cutouts of the reference's list (its first
 * cutn // 4 cutouts of a square image are the same rectangle, cutouts.py:16-27): one pass through the tower carries their weight; the
 * mean over cutouts then divides by the sum of a batch's multiplicities.  Same gradient, fewer images. */
int maua_clip_guide_grad(maua_clip* net, const float* img, int B, int H, int W, const int* rects, const float* mult, int cutn, int batches,
                         float scale, float clamp_gradient, float* grad);
/* maua_clip_guide_grad with augmented cutouts (no multiplicities: augmented cutouts all differ): augs HOST float [batches][cutn][17]
 * ("normal", per_call 0: rects of the padded image, no flags) or [batches][17] ("dango", per_call 1), keys HOST [batches] - one noise
 * key per cutout batch (maua_cutouts_aug's layout) */
int maua_clip_guide_grad_aug(maua_clip* net, const float* img, int B, int H, int W, const int* rects, int cutn, int batches, const float* augs,
                             const unsigned long long* keys, int per_call, float scale, float clamp_gradient, float* grad);
/* sum_p w_p dist_p of the first `count` cutout images of the last pass through the tower (cutout-major; device f32 [count]) */
int maua_clip_last_image_losses(maua_clip* net, int count, float* out);
/* CLIP's text tower (clip/model.py CLIP.encode_text: token_embedding + positional_embedding, `layers` pre-LN residual blocks with
 * the causal mask, ln_final of the EOT row = argmax of the row's token ids, @ text_projection); published architecture restated,
 * parity unpinned.  Forward only: prompts are constants of the guided loop.  dtype MAUA_BF16 or MAUA_F32 (exact products).
 * Parameter names: CLIP's top-level text keys (token_embedding.weight [vocab][w], positional_embedding [ctx][w],
 * transformer.resblocks.<i>.{attn.in_proj_weight, attn.in_proj_bias, attn.out_proj.*, ln_1.*, mlp.c_fc.*, mlp.c_proj.*, ln_2.*},
 * ln_final.*, text_projection [w][E]), host float32 in the checkpoint's layout.  Workspaces grow on demand. */
typedef struct maua_clip_text maua_clip_text;
int maua_clip_text_create(maua_ctx* ctx, int context_length, int vocab_size, int width, int layers, int heads, int embed_dim, int dtype,
                          maua_clip_text** out);
void maua_clip_text_destroy(maua_clip_text* net);
int maua_clip_text_load(maua_clip_text* net, const char* name, const float* host_data, size_t count);
/* tokens device int32 [N][context_length] (clip.tokenize's ids; every id must lie in [0, vocab_size) - an id outside is clamped,
 * never read outside the table) -> embeds device f32 [N][embed_dim] */
int maua_clip_text_encode(maua_clip_text* net, const int* tokens, int N, float* embeds);
/* the guided loop with THIS grad module: the following maua_ddim_guided_loop calls on `net` (speed "fast": a secondary model, or
 * "regular") evaluate CLIPGrads on the image estimate instead of the image-MSE module (their target / mse_k arguments are ignored);
 * rects: HOST int [n_steps][batches][cutn][3], one draw per step and cutout batch (mult: NULL or [n_steps][batches][cutn], as above),
 * read at every call of the loop.  clip == NULL:
 * back to the image-MSE module.  The whole step - UNet, secondary model, cutouts, image tower forward and backward, DDIM update -
 * stays one hipGraph. */
int maua_unet_set_clip_guide(maua_unet* net, maua_clip* clip, const int* rects, const float* mult, int n_steps, int cutn, int batches,
                             float scale, float clamp_gradient);
/* operator-level pieces.  maua_cutouts: random_cutouts (cutouts.py:8-38) on HOST rectangles [n_cut][3] applied to img * mul + add,
 * resized to cut_size^2 by the `resize_right` algorithm (cubic, antialiased, zero padding), Normalize(mean3, std3) -> out device f32
 * [n_cut * B][3][cut_size][cut_size] (cutout-major, like torch.cat); maua_cutouts_vjp: d_out -> d_img [B][3][H][W].  A rectangle is
 * (size | flags, top, left): flags MAUA's grey (1 << 30) and mirror (1 << 29) bits of DangoCutouts, no others.  Checked by name before
 * anything is carved, copied or launched: NULL or aliased pointers, n_cut and cut_size >= 1, H and W >= 1, n_cut * B <= 65535 (the
 * gradient also 3 * B and H <= 65535), min(H, W) <= 4 * cut_size - 1 (16 filter taps), every rectangle's size >= 1 and the rectangle
 * inside the image.  B == 0: nothing is done. */
int maua_cutouts(maua_ctx* ctx, const float* img, int B, int H, int W, const int* rects, int n_cut, int cut_size, float mul, float add,
                 const float* mean3, const float* std3, float* out);
int maua_cutouts_vjp(maua_ctx* ctx, const float* d_out, int B, int H, int W, const int* rects, int n_cut, int cut_size, float mul,
                     const float* std3, float* d_img);
/* The cutouts with the torchvision augmentation pipeline of "normal" / "dango" cutouts (cutouts.py:59-71 / 133-146, skip_augs=False;
 * csrc/cutout_augs.hip): flip, noise, nearest RandomAffine, noise, bilinear RandomPerspective, noise, grey, noise.
 * augs: HOST float records of MAUA_AUG_REC values in the draw order {flip, affine[6] (torchvision's inverse affine matrix), persp_on,
 * persp[8] (its perspective coefficients; ignored when off), grey} - flags 0 / 1, finite, invertible: anything else is refused.
 * per_call 0 ("normal"): augs [n_cut], record n augments crop n (no flags in its rectangle) at its own size before the resize;
 * per_call 1 ("dango"): augs [1] augments every resized cutout.  The noise is the library's Philox normals x 0.01 under `key`, stream
 * 4 j + stage (stage 0..3 in pipeline order), offset = the row-major element index: "normal": j = n, tensor [B][3][s][s]; "dango":
 * j = 0, tensor [n_cut * B][3][cut_size][cut_size].  The warps fill 0 in the space img * mul + add.  out as maua_cutouts;
 * maua_cutouts_aug_vjp: d_out -> d_img (the noise drops out; deterministic: no float atomics). */
#define MAUA_AUG_REC 17
int maua_cutouts_aug(maua_ctx* ctx, const float* img, int B, int H, int W, const int* rects, int n_cut, int cut_size, float mul, float add,
                     const float* mean3, const float* std3, const float* augs, unsigned long long key, int per_call, float* out);
int maua_cutouts_aug_vjp(maua_ctx* ctx, const float* d_out, int B, int H, int W, const int* rects, int n_cut, int cut_size, float mul,
                         const float* std3, const float* augs, int per_call, float* d_img);
/* nn.LayerNorm over the last dimension of x [rows][C] in dtype (float32 statistics, eps 1e-5; clip/model.py LayerNorm); stats:
 * optional device f32 [rows][2] = (mean, rstd), what maua_layer_norm_vjp needs: dx = d LayerNorm / d x applied to dy (+ add) */
int maua_layer_norm(maua_ctx* ctx, const void* x, const float* gamma, const float* beta, long rows, int C, int dtype, void* y, float* stats);
int maua_layer_norm_vjp(maua_ctx* ctx, const void* x, const float* stats, const float* gamma, const void* dy, const void* add, long rows,
                        int C, int dtype, void* dx);

/* ---- image-prompt grad modules: ColorMatchGrads, VGGGrads, LPIPSGrads (the other members of get_diffusion_model's list,
 * maua/diffusion/image.py:92-97) ------------------------------------------------------------------------------------------
 * ColorMatchGrads (maua/grad.py:27-70): hue histogram of clamp((img + 1) / 2) under kornia's rgb_to_hsv (restated; radians clamped
 * to [0, 1] as the reference does), weighted by sqrt(sat * val), normalised to sum 1 - differentiable_histogram's 255 masked passes
 * as one pass with 64-bit fixed-point sums (bit-identical from run to run).  img device f32 [B][3][H][W] in [-1, 1].
 *   maua_colormatch_hist : hist device f32 [B][nbins]                                   (histogram(), set_targets :65-69)
 *   maua_colormatch_grad : grad = d (scale * mse_loss(hist, target)) / d img in closed form (forward :67-70); target device f32
 *                          [nbins] (target_per_sample == 0) or [B][nbins]; loss: optional device f32 [B], the samples' shares of the
 *                          loss (their sum is the reference's scalar)
 * Checked by name: NULL pointers, grad aliasing img, 2 <= nbins <= 1024, H and W >= 1, 0 <= B <= 65535 (B == 0: nothing is done) and
 * H * W <= 2^23 (nbins - 1): a pixel adds less than 2^41 / (nbins - 1) to a 64-bit sum, beyond that the sums could pass 2^64.  An image
 * whose weights are all zero (all grey, with saturation weighting) gives 0 / 0: a NaN histogram, as the reference does, and a gradient
 * holding NaN, which maua_grad_accumulate drops. */
int maua_colormatch_hist(maua_ctx* ctx, const float* img, int B, int H, int W, int nbins, int sat_weighting, float* hist);
int maua_colormatch_grad(maua_ctx* ctx, const float* img, int B, int H, int W, int nbins, int sat_weighting, const float* target,
                         int target_per_sample, float scale, float* grad, float* loss);
/* the conditioning's sum over its grad modules (guided.py:258-266 `if torch.isnan(sub).any(): sub = zeros; img_grad += sub`) without
 * the host round trip: acc = (first ? 0 : acc) + (sub holds a NaN ? 0 : sub) over n device floats */
int maua_grad_accumulate(maua_ctx* ctx, const float* sub, float* acc, long n, int first);
/* VGG perceptors (csrc/perceptor.hip).  plan: n_ops entries, > 0 = Conv2d(3x3, pad 1) to that many channels (multiples of 64) + ReLU,
 * 0 = MaxPool2d(2) - torchvision's vgg19 / vgg16 `features` cut after the last tap; replicate_first: the first convolution pads by
 * replication (vgg_kbc.py:40); the network sees ((img * in_mul + in_add) - mean) / std (VGGGrads: img.add(1).div(2) + ImageNet
 * Normalize, vgg_kbc.py:33; LPIPS: its ScalingLayer).  dtype MAUA_F32 (exact products, parity mode) or MAUA_BF16.  Weights: torch
 * layout [Co][Ci][3][3] / [Co] per convolution, in plan order (torchvision keys "<features index>.weight / .bias"); the published
 * networks are un-vendored (torchvision, lpips: parity unpinned), random-init in tests and bench. */
typedef struct maua_vgg maua_vgg;
int maua_vgg_create(maua_ctx* ctx, int dtype, const int* plan, int n_ops, int replicate_first, float in_mul, float in_add,
                    const float* mean3, const float* std3, maua_vgg** out);
void maua_vgg_destroy(maua_vgg* net);
int maua_vgg_conv_count(maua_vgg* net);
int maua_vgg_conv_shape(maua_vgg* net, int index, int* ci, int* co);
int maua_vgg_load(maua_vgg* net, int conv_index, int what /* 0 weight, 1 bias */, const float* host_data, size_t count);
/* forward of img device f32 [B][3][H][W]; every activation is kept for the calls below (plan entry index `op`):
 * maua_vgg_features -> planar f32 [B][C][h][w]; maua_vgg_gram -> Gram matrices [B][C][C] (loss.py:57-80 gram_matrix per image:
 * Perceptor.get_target_embeddings, perceptors/__init__.py:44-76); maua_vgg_lpips_features -> unit-normalised features [B][h w][C] */
int maua_vgg_forward(maua_vgg* net, const float* img, int B, int H, int W);
int maua_vgg_features(maua_vgg* net, int op, float* out);
int maua_vgg_gram(maua_vgg* net, int op, float* out);
int maua_vgg_lpips_features(maua_vgg* net, int op, float* out);
/* VGGGrads.forward (maua/grad.py:90-93): grad = d sum_taps strength * feature_loss(gram(tap), target) / d img, per image
 * (feature_loss = scaled_mse_loss / numel, loss.py:33-54); taps HOST int [n_taps] (plan entries), targets HOST array of n_taps DEVICE
 * pointers to f32 [C][C] (target_bstride NULL / 0) or [B][C][C] (target_bstride[k] = C * C); loss optional device f32 [B] */
int maua_vgg_style_grad(maua_vgg* net, const float* img, int B, int H, int W, const int* taps, int n_taps, const float* const* targets,
                        const long* target_bstride, float strength, float* grad, float* loss);
/* The NCA style loss (maua/nca/train.py:122-142, 228-229): G_b = F_b^T F_b / (h w) per tap, L = sum_taps mean((mean_b G_b - T)^2);
 * grad = dL / d img [B][3][H][W], loss one optional device f32.  taps / targets as above, every target one f32 [C][C] in the same
 * normalisation (maua_vgg_gram's output divided by h w) */
int maua_vgg_gram_mean_grad(maua_vgg* net, const float* img, int B, int H, int W, const int* taps, int n_taps, const float* const* targets,
                            float* grad, float* loss);
/* LPIPSGrads.forward (maua/grad.py:189-193) at the network's own size: grad = d (scale * sum_b lpips(img_b, target)) / d img;
 * targets: HOST array of DEVICE pointers to the target's unit-normalised tap features (maua_vgg_lpips_features: [hw][C], shared, or
 * [B][hw][C] with target_bstride[k] = hw * C), lins: DEVICE pointers to the lin layers' weights [C]; dist optional device f32 [B] */
int maua_vgg_lpips_grad(maua_vgg* net, const float* img, int B, int H, int W, const int* taps, int n_taps, const float* const* targets,
                        const long* target_bstride, const float* const* lins, float scale, float* grad, float* dist);

/* ResNet bottleneck backbone (csrc/resnet.hip): the feature extractor of the GAN metrics' "SwAV" option
 * (maua/GAN/metrics/extractors/swav.py ResNet(Bottleneck, layers): ConstantPad2d(1) + 7x7 stride-2 stem, MaxPool2d(3, 2, 1), four
 * layers of bottleneck blocks - the stride on each block's 3x3 - global average pool; forward_backbone, no head).  BatchNorm never
 * reaches the library: the caller folds it into each convolution's weight and bias.  layers: HOST int [4] blocks per layer (>= 1 each);
 * width (a multiple of 64; 64 for ResNet-50): the stem's channels, the features are 32 * width wide.  dtype MAUA_F32 (exact products)
 * or MAUA_BF16.  Convolutions are indexed in the state dict's order: conv1 (the stem), then per block conv1, conv2, conv3 and - in the
 * first block of a layer - downsample.0.  maua_resnet_conv_shape reports Ci, Co, kernel size and stride of one (no device needed).
 * maua_resnet_load: what 0 = weight, HOST float32 [Co][Ci][k][k], prepared once into the kernels' layout; 1 = bias, HOST float32 [Co].
 * maua_resnet_forward: img device planar f32 [B][3][H][W] -> features device f32 [B][32 * width]; the activation workspace is laid out
 * for (B, H, W) and laid out again when they change.  Every stage's output of the last forward is kept: maua_resnet_tap writes stage
 * 0 stem, 1 max-pool, 2 .. 5 layer1 .. layer4 as planar float32 [B][C][h][w] (device), maua_resnet_tap_shape reports C, h, w. */
typedef struct maua_resnet maua_resnet;
int maua_resnet_create(maua_ctx* ctx, int dtype, const int* layers, int width, maua_resnet** out);
void maua_resnet_destroy(maua_resnet* net);
int maua_resnet_conv_count(maua_resnet* net);
int maua_resnet_conv_shape(maua_resnet* net, int index, int* ci, int* co, int* k, int* stride);
int maua_resnet_load(maua_resnet* net, int conv_index, int what /* 0 weight, 1 bias */, const float* host_data, size_t count);
int maua_resnet_forward(maua_resnet* net, const float* img, int B, int H, int W, float* features);
/* the same forward with HIP events between its stages; synchronises and writes HOST float [7] milliseconds: stem, max-pool,
 * layer1 .. layer4, average pool (scripts/bench_swav.py) */
int maua_resnet_forward_timed(maua_resnet* net, const float* img, int B, int H, int W, float* features, float* stage_ms);
int maua_resnet_tap_shape(maua_resnet* net, int stage, int* C, int* h, int* w);
int maua_resnet_tap(maua_resnet* net, int stage, float* out);

/* grad modules as library objects, so that the guided loop can evaluate a LIST of them per step (guided.py:258-266 sums the modules'
 * gradients; get_diffusion_model hands the sampler up to four, maua/diffusion/image.py:92-97).  kind: MAUA_GUIDE_STYLE = VGGGrads
 * (arguments of maua_vgg_style_grad: net, taps, targets = Gram matrices, target_bstride, scale = strength), MAUA_GUIDE_LPIPS =
 * LPIPSGrads (arguments of maua_vgg_lpips_grad, lins), MAUA_GUIDE_COLORMATCH = ColorMatchGrads (targets[0] = the target histogram
 * [nbins] - target_bstride[0] == nbins: one per sample -, nbins, sat_weighting, scale; net / taps / lins unused).  The target tensors
 * stay the caller's: device pointers that must outlive the guide; updating them IN PLACE re-targets the guide, also inside an already
 * captured loop.  maua_guide_grad: the module as an operator, grad = d loss / d img of img device f32 [B][3][H][W]. */
#define MAUA_GUIDE_STYLE 0
#define MAUA_GUIDE_LPIPS 1
#define MAUA_GUIDE_COLORMATCH 2
typedef struct maua_guide maua_guide;
int maua_guide_create(maua_ctx* ctx, int kind, maua_vgg* net, const int* taps, int n_taps, const float* const* targets,
                      const long* target_bstride, const float* const* lins, float scale, int nbins, int sat_weighting, maua_guide** out);
void maua_guide_destroy(maua_guide* guide);
int maua_guide_grad(maua_guide* guide, const float* img, int B, int H, int W, float* grad);
/* the guided loop with THESE grad modules: the following maua_ddim_guided_loop calls on `net` evaluate every guide of the list on the
 * step's image estimate and sum the results (a module whose gradient holds a NaN is skipped, guided.py:262-265) - after CLIPGrads when
 * maua_unet_set_clip_guide is active as well, instead of the image-MSE module otherwise (its target / mse_k arguments are then
 * ignored).  n_guides == 0: back to the default.  The whole step stays inside the one captured hipGraph. */
int maua_unet_set_guides(maua_unet* net, maua_guide* const* guides, int n_guides);

/* ---- image operators of the multi-resolution pipeline (maua/diffusion/image.py:132-214: what runs between two scales; csrc/image_ops.hip).
 * Planar device f32 images [B][3][H][W]; every operator is a gather with a fixed summation order (bit-identical from run to run).
 *
 * maua_image_resize: resize_right.resize(img, out_shape=(Ho, Wo), interp_method=...) (diffusion/image.py:66-71 cubic, :180 lanczos3) on
 * `planes` = B * C planes.  The per-axis tap tables come from the caller (maua_amd/image.py resize_tables: the published float32
 * arithmetic - kernel stretched by 1 / scale when shrinking, weights normalised per output sample): left_* DEVICE int [out], w_* DEVICE
 * f32 [out][taps]; source indices outside the image contribute zero (zero padding).  left_y == NULL keeps the rows (H == Ho), left_x
 * == NULL the columns.  Rows first, then columns.  dst = resized + add, or (dst + resized) + add when accumulate != 0 (the perlin init's
 * `resize(a) + resize(b) - 1`, :65-69). */
int maua_image_resize(maua_ctx* ctx, const float* src, int planes, int H, int W, float* dst, int Ho, int Wo, const int* left_y,
                      const float* w_y, int taps_y, const int* left_x, const float* w_x, int taps_x, int accumulate, float add);
/* destitch (maua/ops/image.py:15-23): out [(n_rows * n_cols) * B][3][T][T], tile (r, c) of image b at index (r * n_cols + c) * B + b;
 * ys / xs HOST int arrays: the tile origins (the reference's linspace(0, H - T, n).round(), evaluated by the caller). */
int maua_image_destitch(maua_ctx* ctx, const float* img, int B, int H, int W, int tile_size, const int* ys, int n_rows, const int* xs,
                        int n_cols, float* out);
/* restitch (maua/ops/image.py:26-62): tiles [n_rows * n_cols][3][T][T] -> out [1][3][H][W] = sum tile * wy * wx / sum wy * wx, in the
 * reference's tile order; wy DEVICE f32 [n_rows][T], wx DEVICE f32 [n_cols][T]: blend_weight1d per tile row / column (smoothstep fades,
 * none at the image's edges), built by the caller. */
int maua_image_restitch(maua_ctx* ctx, const float* tiles, int tile_size, const int* ys, int n_rows, const int* xs, int n_cols,
                        const float* wy, const float* wx, float* out, int H, int W);
/* sharpen (maua/ops/image.py:70-71: torchvision adjust_sharpness of (img + 1) / 2, back to [-1, 1]): 3x3 blur [[1,1,1],[1,5,1],[1,1,1]] / 13
 * on interior pixels, border pixels kept, strength * img + (1 - strength) * blurred, clamp to [0, 1]. */
int maua_image_sharpen(maua_ctx* ctx, const float* img, int B, int H, int W, float strength, float* out);
/* match_histogram mode "avg" (maua/ops/image.py:105-173) in two steps around a float64 host step (the symmetric square roots of the two
 * 3x3 covariances and the inverse: maua_amd/image.py).  maua_image_moments: per frame f the 11 partial sums (3 sums, products 00 01 02 11
 * 12 22, min, max) of every slice of 4096 pixels of value = mean of images f * navg .. + navg - 1 (source.mean(0), :134) + noise_scale *
 * noise[f] (:141-144; noise optional DEVICE f32 [frames][3][HW]); min / max are of the images alone (:171-173).  partial DEVICE f32
 * [frames][maua_image_moments_slices(HW)][11].  maua_image_match_apply, one frame [3][HW]: out = scale * (m (img + noise_scale * noise -
 * mu_t) + mu_s) (+ out when accumulate: a list of sources, :130, :166), clamped to [lo, hi] when clamp; m / mu_t / mu_s HOST f32. */
int maua_image_moments_slices(long HW);
int maua_image_moments(maua_ctx* ctx, const float* img, int frames, int navg, long HW, const float* noise, float noise_scale,
                       float* partial);
int maua_image_match_apply(maua_ctx* ctx, const float* img, const float* noise, float noise_scale, long HW, const float* m,
                           const float* mu_t, const float* mu_s, float scale, int accumulate, int clamp, float lo, float hi, float* out);
/* create_perlin_noise (maua/ops/noise.py:90-132) from given gradient vectors: grads DEVICE f32, per (channel, octave) gx [(w + 1)][(h + 1)]
 * then gy (torch.randn(2, w + 1, h + 1, 1, 1), :96, with w / h doubling per octave) at element offsets[channel * n_octaves + octave]
 * (HOST long); octaves HOST f32 [n_octaves]; 1 channel when grayscale, else 3.  The octave sum, clamp(0, 1), to_pil_image's bytes,
 * ImageOps.autocontrast and to_tensor -> out [3][width << n_octaves][height << n_octaves]; raw (optional): perlin_ms's sum before the
 * clamp, [channels][..][..].  Uses the context's scratch arena. */
int maua_image_perlin(maua_ctx* ctx, const float* grads, const long* offsets, const float* octaves, int n_octaves, int width, int height,
                      int grayscale, float* raw, float* out);

/* ---- optical-flow operators of the video pipeline (maua/diffusion/video.py:125-301 and what it uses of maua/flow/; csrc/flow.hip).
 * Planar device f32 images [B][3][H][W]; flows [B][H][W][2] in (x, y) order, as the reference holds them.  Gathers only, fixed summation
 * order, no atomics: a rerun is bit-identical.  No entry point allocates (maua_farneback_create plans the estimator's workspace).
 *
 * maua_flow_warp: warp(x, flow_warp_map(flow * exaggeration)) (flow/lib.py:51-63 with diffusion/video.py:161-162) in one launch, the grid
 * not materialised: pixel (x, y) samples at linspace(-1, 1, W)[x] + exaggeration flow_x / W, linspace(-1, 1, H)[y] + exaggeration flow_y / H
 * (the reference's normalisation as written: by W and H) with grid_sample(bilinear, padding_mode="reflection", align_corners=False).
 * img / out [B][C][H][W]. */
int maua_flow_warp(maua_ctx* ctx, const float* img, const float* flow, float exaggeration, int B, int C, int H, int W, float* out);
/* check_consistency (flow/consistency.py:78-127; get_consistency_map's "full" mode, flow/lib.py:66-80) per sample: central differences of
 * the backward flow (zero "same" padding, both channels summed), the forward flow sampled at p + backward (bilinear, align_corners=True,
 * zero padding), motion_boundary -> 0, missed -> -0.75, overshoot -> 0 in that order, then torchvision's gaussian_blur(kernel_size=3)
 * (sigma 0.8, reflect padding) and clip(0, 1).  Two launches: classes [B][H][W] (scratch of the caller's) then out [B][H][W].  Flow values
 * are clamped to +-clamp as they are read (diffusion/video.py:148-149; INFINITY: none). */
int maua_flow_consistency(maua_ctx* ctx, const float* forward, const float* backward, int B, int H, int W, float clamp, float* classes,
                          float* out);
/* F.interpolate(mode="bilinear", align_corners=False) of a channels-last tensor [B][H][W][C] -> [B][out_h][out_w][C] (diffusion/video.py:153-157:
 * flows, C = 2, and consistency maps, C = 1): dst = interpolate(clamp(src, +-clamp)) * multiplier (:149, :156). */
int maua_flow_resize_bilinear(maua_ctx* ctx, const float* src, int B, int H, int W, int C, float* dst, int out_h, int out_w, float multiplier,
                              float clamp);
/* The frame composition of diffusion/video.py:248-277 in one launch: mask = (consistency trust + 1 - trust) blend (consistency NULL: blend),
 * init = (frame + mask warp(prev)) / (1 + mask) (prev NULL: frame); cached != NULL: fade init + (1 - fade) cached (:268-269); noise_scale != 0:
 * + noise_scale z, z = element i of maua_philox_normal(seed, stream 0) for element i of [B][3][H][W] (:277; torch's randn_like values are
 * not reproduced).  With prev and cached NULL this is the noise step alone (after pre_hook / hist_persist). */
int maua_flow_compose(maua_ctx* ctx, const float* frame, const float* prev, const float* flow, const float* consistency, const float* cached,
                      int B, int H, int W, float exaggeration, float trust, float blend, float fade, float noise_scale, unsigned long long seed,
                      float* out);
/* One turbo in-between frame (diffusion/video.py:221-238): prev_out = warp(prev) (prev may be NULL), next_out = warp(next) when warp_next
 * (the t != 0 and f_n < N + wrap_around rule is the caller's), img = prev_out (1 - blend_t) + next' blend_t with next' the warped or the
 * given next; without prev, img = next'.  One launch. */
int maua_flow_turbo(maua_ctx* ctx, const float* prev, const float* next, const float* flow, int B, int H, int W, float exaggeration, int warp_next,
                    float blend_t, float* prev_out, float* next_out, float* img);
/* Farneback's dense flow (flow/__init__.py:35-55: cv2.calcOpticalFlowFarneback(pyr_scale=0.8, levels=15, winsize=15, iterations=15, poly_n=7,
 * poly_sigma=1.5, flags=10) of luminance(im).mul(255).byte(), on the host there) restated from the published algorithm: box window, zero
 * initial flow.  The handle owns a workspace planned for max_h x max_w.  maua_farneback_pair: im_a / im_b [3][H][W] in [0, 1] ->
 * flow_ab = flow(prev = a, next = b) and flow_ba = flow(b, a), [H][W][2] each, both directions in one batched launch per stage.
 * maua_farneback_levels: the number of pyramid levels an H x W pair is processed at (host only). */
typedef struct maua_farneback maua_farneback;
int maua_farneback_levels(int H, int W);
int maua_farneback_create(maua_ctx* ctx, int max_h, int max_w, maua_farneback** out);
int maua_farneback_destroy(maua_farneback* handle);
int maua_farneback_pair(maua_farneback* handle, maua_ctx* ctx, const float* im_a, const float* im_b, int H, int W, float* flow_ab,
                        float* flow_ba);
/* the estimator with its stages in the caller's hand, for parity tests (no reference counterpart).  maua_farneback_pair is this launch
 * with level_hi = level_lo = -1, iterations 0, no initial flow and no dumps.
 *   level_hi, level_lo: the pyramid levels level_hi .. level_lo are processed, downwards (-1, -1: the top level, maua_farneback_levels - 1,
 *     down to 0).  flow_ab / flow_ba have level_lo's size [h][w][2] (maua_farneback_level_size).
 *   iterations: 1 .. 15 per level; 0 means 15.
 *   init_ab / init_ba (both or neither): the flows entering level_hi, [h][w][2] at that level's size; NULL: zero.
 *   dumps (each optional), device-to-device copies out of the workspace behind the stage that filled it, all of level_lo:
 *     gray [2][H][W] the 8-bit luminance of (a, b); blur [2][H][W] the level's Gaussian blur of it; level [2][h][w] its resize;
 *     coef [2][5][h][w] the polynomial expansion's coefficients of x, y, x^2, y^2, xy; flow_in [2][h][w][2] the flow entering the level
 *     (direction a -> b, then b -> a); mat [2][5][h][w] the update matrices before the first iteration.
 * Refused, in front of the first launch: NULL or aliased arguments, an image below 15 x 15, above 2^26 pixels or above the handle's pixel
 * count, a handle of another device, a level range out of order or above the top level, iterations outside 0 .. 15, one initial flow
 * without the other, a pyramid blur wider than the image. */
typedef struct {
  const float* im_a; const float* im_b; int H, W;
  float* flow_ab; float* flow_ba;
  int level_hi, level_lo, iterations;
  const float* init_ab; const float* init_ba;
  float* gray; float* blur; float* level; float* coef; float* flow_in; float* mat;
} maua_farneback_desc;
/* host only: the size of pyramid level `level` (0 .. maua_farneback_levels - 1) of an H x W pair: round(W 0.8^level) by round(H 0.8^level),
 * half to even, as the launcher computes it */
int maua_farneback_level_size(int H, int W, int level, int* h, int* w);
/* host only, no device needed: MAUA_OK, or MAUA_ERR + maua_last_error() with the launcher's own message.  Pointers are only checked, never
 * dereferenced.  handle may be NULL (there is none without a device): the descriptor alone is checked. */
int maua_farneback_check(const maua_farneback* handle, const maua_farneback_desc* d);
int maua_farneback_pair_ex(maua_farneback* handle, maua_ctx* ctx, const maua_farneback_desc* d);

/* ---- audio-reactivity instruments: per-frame visual features and matrix correlations (csrc/video_features.hip) ---------------
 * Per-frame features of maua/audiovisual/audioreactive/selfsupervised/features/video.py:12-75, taken while the frames are on the device:
 *   the histograms of R, G, B (video.py:12-31) and of H, S, V (:35-57; kornia.color.rgb_to_hsv restated from its published form: v = max,
 *     s = (max - min) / (max + 1e-8), the hue of the first maximal channel, h = 2 pi ((h_k / deltac / 6) % 1) with torch's remainder):
 *     torch.histc(frame, bins) with the frame-channel's own minimum and maximum as the range ([v - 1, v + 1] when they coincide), bin
 *     int((x - min) * bins / (max - min)) in float32 with the right edge folded into the last bin, each histogram divided by its largest bin;
 *   visual_variance (:61-62): the unbiased variance over N = 3 H W;
 *   absdiff (:66-75): sum |frame_b - frame_{b-1}|; the handle carries a device copy of the last frame of the previous push, so a stream
 *     may be pushed in batches of any size (the reference's 64-frame chunking changes nothing in the result and is not reproduced).
 * frames: `B` dense frames in one of three layouts; a uint8 value k means k / 255 by a correctly rounded division (decord ... .div(255),
 * video.py:208).  Outputs (device): hist [B][6][bins] float32 in the order R, G, B, H, S, V; counts [B][6][bins] int32, optional (NULL), the
 * raw bin counts; variance [B]; diff [B], against the carried frame for b = 0 and 0 for the very first frame of a stream.  The reference's
 * absdiff is cat(diff[1:], diff[-1:]) over the stream.
 * Counts and the uint8 sums are integers throughout and every float operation is correctly rounded and uncontracted: counts and hist agree
 * with a float32 host restatement to the bit, a rerun is bit-identical.  float32 frames: the sums are accumulated in float64.
 * No entry point allocates: maua_vfeat_create plans the workspace for max_batch frames of H x W.  Refused, in front of the first launch: a
 * layout outside 0 .. 2, bins outside 1 .. 256, B above max_batch, a frame size other than the handle's (or above 2^24 pixels, where a float32
 * bin count stops being exact), a handle of another device, NULL outputs, a layout that changes inside a stream.  maua_vfeat_reset forgets
 * the carried frame: the next push starts a stream. */
enum { MAUA_VFEAT_U8_HWC = 0, MAUA_VFEAT_U8_CHW = 1, MAUA_VFEAT_F32_CHW = 2 };
typedef struct maua_vfeat maua_vfeat;
int maua_vfeat_create(maua_ctx* ctx, int H, int W, int bins, int max_batch, maua_vfeat** out);
int maua_vfeat_destroy(maua_vfeat* handle);
int maua_vfeat_reset(maua_vfeat* handle);
/* host only, no device needed: MAUA_OK, or MAUA_ERR + maua_last_error() with maua_vfeat_push's own message.  Pointers are only checked, never
 * dereferenced.  handle may be NULL (there is none without a device): then H, W, bins and max_batch describe the plan; with a handle, bins
 * and max_batch are the handle's. */
int maua_vfeat_check(const maua_vfeat* handle, int H, int W, int bins, int max_batch, const void* frames, int layout, int B, const float* hist,
                     const int* counts, const float* variance, const float* diff);
int maua_vfeat_push(maua_vfeat* handle, maua_ctx* ctx, const void* frames, int layout, int B, int H, int W, float* hist, int* counts,
                    float* variance, float* diff);
/* Matrix correlations between x [T][Fx] and y [T][Fy] (device float32, rows = time), correlation.py:353-382 with :14-56, :72-121, :278-282:
 * pearson and concordance (torch.median's lower median over the column pairs), autocorrcorr, rv, rv2 (the modified RV) and r1.  No T x T
 * matrix is formed: trace(XX^T YY^T) = |X^T Y|_F^2, the modified RV subtracts sum_t |x_t|^2 |y_t|^2, and autocorrcorr's five sums over the
 * pairs i < j follow from |sum_t x^_t|^2, |X^^T X^|_F^2, |X^^T Y^|_F^2 and the unit diagonals.  Column means, row norms and one
 * [Fx + Fy] x T x [Fx + Fy] product in float64, summed over T in slabs of 64 rows in a fixed order, no atomics; a finishing kernel writes the
 * metric to out [1] (device float32).  ws: maua_correlation_workspace() bytes of device memory, 256-byte aligned (nothing is allocated).
 * Refused, in front of the first launch: an unknown metric, Fx != Fy for pearson / concordance / r1, Fx + Fy above 1024, T below 2 (3 for
 * autocorrcorr), NULL arguments, a short workspace.  maua_correlation_check: host only, the same refusals. */
enum { MAUA_CORR_PEARSON = 0, MAUA_CORR_CONCORDANCE = 1, MAUA_CORR_AUTOCORRCORR = 2, MAUA_CORR_RV = 3, MAUA_CORR_RV2 = 4, MAUA_CORR_R1 = 5 };
long maua_correlation_workspace(int T, int Fx, int Fy);
int maua_correlation_check(const float* x, const float* y, int T, int Fx, int Fy, int metric, const void* ws, long ws_bytes, const float* out);
int maua_correlation(maua_ctx* ctx, const float* x, const float* y, int T, int Fx, int Fy, int metric, void* ws, long ws_bytes, float* out);

/* ---- GAN evaluation metrics on a float64 matrix-core GEMM (maua/GAN/metrics/{frechet,kernel,prdc}.py; csrc/gemm_f64.hip) ------------
 * Everything here is float64 on v_mfma_f64_16x16x4_f64.  Feature matrices are device memory, row-major [rows][d], float32 (f64 = 0, widened
 * on load) or float64 (f64 = 1).  Workspaces are device memory, 256-byte aligned, sized by the _workspace call beside each entry point
 * (nothing is allocated).  Sums are trees of a fixed shape and counts are integer atomics: a rerun is bit-identical.
 *
 * maua_gemm_f64: row-major C = alpha op(A) op(B) + beta C, op(A) [M][K], op(B) [K][N]; transa / transb != 0: the operand is stored
 * transposed ([K][M] / [N][K]).  Any M, N, K >= 1, leading dimensions at least a stored row; beta == 0 never reads C. */
int maua_gemm_f64(maua_ctx* ctx, int transa, int transb, int M, int N, int K, double alpha, const double* a, long lda, const double* b, long ldb,
                  double beta, double* c, long ldc);
/* frechet.py:73-74: mean [d] = torch.mean(feats, axis=0) and cov [d][d] = torch.cov(feats.T): centred before the product, denominator N - 1
 * (N >= 2). */
long maua_metrics_moments_workspace(int N, int d);
int maua_metrics_moments(maua_ctx* ctx, const void* feats, int f64, int N, int d, void* ws, long ws_bytes, double* mean, double* cov);
/* frechet.py:4-46, the Newton-Schulz square root of m [d][d]: Y = m / |m|_F, Z = I; T = (3 I - Z Y) / 2, Y <- Y T, Z <- T Z;
 * s = Y sqrt(|m|_F), error = |m - s s|_F / |m|_F; stops once error <= 1e-5 or error > the previous one, and s [d][d] (device) is the S of
 * the iteration that stopped, the diverged one included, as the reference returns it.  errors [num_iters] and iters [1] are HOST memory
 * (either may be NULL): the error of every iteration run and their number.  Synchronises the stream once per iteration. */
long maua_sqrtm_workspace(int d);
int maua_sqrtm_newton_schulz(maua_ctx* ctx, const double* m, int d, int num_iters, void* ws, long ws_bytes, double* s, double* errors, int* iters);
/* frechet.py:61-94: |mu1 - mu2|^2 + tr sigma1 + tr sigma2 - 2 tr sqrtm(sigma1 sigma2); on a non-finite root the one retry with eps on both
 * diagonals (:82-85).  distance [1], errors [num_iters], iters [1], retried [1]: HOST memory (the last three may be NULL). */
long maua_frechet_workspace(int N1, int N2, int d);
int maua_frechet_distance(maua_ctx* ctx, const void* feats1, int N1, const void* feats2, int N2, int d, int f64, double eps, int num_iters,
                          void* ws, long ws_bytes, double* distance, double* errors, int* iters, int* retried);
/* kernel.py:4-18 with n = d.  idx [S][2][m] (device): for subset s the rows of feats2 that make x, then the rows of feats1 that make y,
 * drawn by the host in that order (an index outside its set yields NaN, never a read).  raw [S][3][2] (device): sum and trace of
 * (x x^T / n + 1)^3, (y y^T / n + 1)^3, (x y^T / n + 1)^3; sums [S][3] (device): sum a, tr a, sum b of :14-15; kid [1] (device): :16-17.
 * 2 <= m <= min(N1, N2). */
long maua_kernel_distance_workspace(int m, int d);
int maua_kernel_distance(maua_ctx* ctx, const void* feats1, int N1, const void* feats2, int N2, int d, int f64, const long* idx, int S, int m,
                         void* ws, long ws_bytes, double* kid, double* sums, double* raw);
/* prdc.py:10-24: dist [N][M] (device) = max(|x_i|^2 + |y_j|^2 - 2 x_i . y_j, 0), NaN -> 0.  The one call that writes the matrix. */
long maua_prdc_workspace(int N, int M, int d);
int maua_pairwise_distances(maua_ctx* ctx, const void* x, int N, const void* y, int M, int d, int f64, void* ws, long ws_bytes, double* dist);
/* prdc.py:27-37: radii [N] (device) = the (nearest_k + 1)-th smallest distance of every row to its own set, the self distance included.
 * nearest_k in 1 .. 15, N >= nearest_k + 1; ws: maua_prdc_workspace(N, 1, d) bytes. */
int maua_knn_radii(maua_ctx* ctx, const void* feats, int N, int d, int f64, int nearest_k, void* ws, long ws_bytes, double* radii);
/* prdc.py:40-61 as integers: counts [4] (device) = fakes inside some real ball, reals inside some fake ball, sum over the fakes of the real
 * balls they lie in, reals whose nearest fake lies inside their own ball; r_real [N], r_fake [M] (device): the two radius vectors.
 * precision = counts[0] / M, recall = counts[1] / N, density = counts[2] / (nearest_k M), coverage = counts[3] / N. */
int maua_prdc(maua_ctx* ctx, const void* real, int N, const void* fake, int M, int d, int f64, int nearest_k, void* ws, long ws_bytes,
              unsigned long long* counts, double* r_real, double* r_fake);

/* ---- dense float64 SVD and symmetric eigendecomposition: one-sided Jacobi (csrc/svd_f64.hip) -----------------------------------------
 * Serves maua/GAN/decomposition/sefa.py:7,25 (`torch.svd(weight).V` of the stacked style-affine weights) and GANSpace's PCA.  Hestenes'
 * method in float64: pairs of columns of A are rotated until they are orthogonal; the rotations accumulate in V.  No vendor solver.
 *   Order: the round-robin tournament on N = n rounded up to even.  A sweep is N - 1 rounds of N / 2 disjoint pairs; position 0 keeps
 *   player 0, position k >= 1 of round r holds player 1 + (k - 1 + r) mod (N - 1), pair i is (position i, position N - 1 - i); a pair with
 *   the padding index N - 1 of an odd n is skipped.  maua_jacobi_schedule (host only, no device): the pairs of one round in that order,
 *   pairs [2 n_pairs] = p0, q0, p1, q1, ...
 *   Pair (p, q): alpha = |a_p|^2, beta = |a_q|^2, gamma = a_p . a_q; left alone when alpha = 0, beta = 0 or |gamma| <= sqrt(m) eps
 *   sqrt(alpha) sqrt(beta), eps = 2^-52 (LAPACK dgesvj's rule); else zeta = (beta - alpha) / (2 gamma), t = sign(zeta) / (|zeta| +
 *   sqrt(1 + zeta^2)) (sign(0) = 1), c = 1 / sqrt(1 + t^2), s = c t; a_p <- c a_p - s a_q, a_q <- s a_p + c a_q, the same on v_p, v_q.
 *   Stop: after the first sweep that rotated nothing - the host reads one integer per sweep; at most max_sweeps (1 .. 30, 0 = 30) sweeps.
 *   When they run out the call returns MAUA_ERR AFTER writing the outputs of the last iterate, and sweeps / last_rotations say how far it got.
 *   Finish: sigma_i = |a_i|, sorted descending (stable: ties keep the lower column first), u_i = a_i / sigma_i - a column with sigma_i = 0
 *   gets u_i = 0, so U has orthonormal columns only over the nonzero singular values - and every (u_i, v_i) is flipped so that v_i's
 *   largest-magnitude component (the lowest index on a tie) is positive: the output is a function of A alone.
 *   Paths: 1 = one workgroup runs every round and sweep with A^T and V resident in LDS ((m + n) n doubles + 128 bytes within 159 KiB);
 *   2 = one launch per round, one workgroup per pair, each column read from memory once per round (staged in LDS while 2 m doubles fit
 *   128 KiB); 0 = path 1 where it fits, else 2.  All three dot products come from one function with one summation order, so both paths
 *   and every rerun return the same bits.
 * a [m][lda] row-major device f64, m >= n >= 1, n <= 4096, m <= 1048576; s [n], u [m][n] (want_u != 0; else not touched, may be NULL),
 * v [n][n] row-major device f64 with A = u diag(s) v^T; sweeps, last_rotations: HOST ints (either may be NULL).  ws: *_workspace_bytes() bytes of
 * device memory, 256-byte aligned (nothing is allocated).  Accuracy is norm-wise: |s - s_exact| = O(max(m, n) eps |A|), no relative
 * claim for small singular values.  The *_check entries are host only, need no device, never dereference a pointer and state every refusal:
 * n < 1, m < n, the size limits, lda < n, an unknown path, path 1 on a matrix beyond its limit, max_sweeps outside 0 .. 30, NULL arguments,
 * a short or misaligned workspace. */
int maua_jacobi_schedule(int n, int round, int* pairs, int* n_pairs);
long maua_svd_f64_workspace_bytes(int m, int n);
int maua_svd_f64_check(const double* a, int m, int n, long lda, int want_u, int path, int max_sweeps, const void* ws, long ws_bytes, const double* s,
                       const double* u, const double* v);
int maua_svd_f64(maua_ctx* ctx, const double* a, int m, int n, long lda, int want_u, int path, int max_sweeps, void* ws, long ws_bytes, double* s,
                 double* u, double* v, int* sweeps, int* last_rotations);
/* Symmetric S [n][lds] (only assumed, not checked): w [n] ascending and q [n][n] row-major, column i the eigenvector of w[i], as
 * torch.linalg.eigh orders them, signs by the rule above.  The Jacobi above runs on S + c I, c = max_i sum_j |S_ij| (Gershgorin), which is
 * positive semidefinite: its right singular vectors are S's eigenvectors and w = sigma - c.  (Without the shift a pair +lambda, -lambda
 * of an indefinite S shares one singular value and the SVD mixes its two vectors.)  Eigenvalue accuracy is ABSOLUTE, O(n eps (|S| + c)),
 * not relative: an eigenvalue far below |S| keeps few digits. */
long maua_eigh_f64_workspace_bytes(int n);
int maua_eigh_f64_check(const double* s, int n, long lds, int path, int max_sweeps, const void* ws, long ws_bytes, const double* w, const double* q);
int maua_eigh_f64(maua_ctx* ctx, const double* s, int n, long lds, int path, int max_sweeps, void* ws, long ws_bytes, double* w, double* q, int* sweeps,
                  int* last_rotations);

/* ---- build-owned counter RNG: Philox4x32-10, identical on every device / rank and in the oracle twin (oracle/rng.py,
 * pinned to the published known-answer vectors).  No reference counterpart: the reference's random-init generator and noise planes
 * come from torch's host generator (inference/stylegan2.py:216-227, selfsupervised/noise.py:42-53); the benchmark's synthetic
 * network and planes are drawn on the device instead (a clip's set-up then costs kernels, not 32 M host draws + their upload).
 * Element i of (seed, stream): counter {i / 4, stream}, key seed, word i % 4; offset = index of out[0] in the stream (any value:
 * a tensor may be filled in pieces).  normal: Box-Muller on word pairs, u = ((x >> 9) + 0.5) 2^-23; out = mean + stdev z. */
int maua_philox_u32(maua_ctx* ctx, unsigned long long seed, unsigned long long stream, unsigned long long offset, uint32_t* out, long n);
int maua_philox_normal(maua_ctx* ctx, unsigned long long seed, unsigned long long stream, unsigned long long offset, float* out, long n,
                       float mean, float stdev);
/* The benchmark clip's waveform on the device (0.3 sin(2 pi 220 t) + 0.2 (u - 0.5) [(2t mod 1) < 0.05] + 0.01 n; u / n =
 * streams 0 / 1 of `seed`): out device f32 [n].  No reference counterpart (synthetic input); host twin oracle/rng.py clip_audio. */
int maua_philox_clip_audio(maua_ctx* ctx, unsigned long long seed, long n, double sample_rate, float* out);

/* ---- latent-space projection (project.hip; maua_amd/projection.py drives it).  Restated from the published algorithm (Karras et al. 2020,
 * "Analyzing and Improving the Image Quality of StyleGAN", appendix D): the reference's maua/parameterizations/stylegan.py is an empty file
 * and the published projector.py is not among its files, so parity with that code is unpinned.  Every operation is rounded on its own (no
 * fused multiply-add, IEEE division and square root) and every sum runs in ONE order: a range is cut into chunks of 4096 elements; in a
 * chunk, thread t of 256 adds elements t, t + 256, ... in that order, the 256 sums fold as a[t] += a[t + s], s = 128, 64 .. 1, and the
 * chunks are added in chunk order.  Reruns give the same bits; tests/projection_ref.py restates every entry in float32 to the bit.  All
 * tensors device f32.  Every *_check is host only, needs no device and only checks pointers; ws: *_workspace_bytes() bytes, 256-byte aligned.
 *
 * maua_noise_reg: the noise regulariser of maps n [B][R][R], R a power of two in 4 .. 16384 (anything else is refused).  Per sample, n_0 = n;
 * level k adds mean(n_k roll(n_k, 1, x))^2 + mean(n_k roll(n_k, 1, y))^2; after the level whose side is <= 8 it stops, else n_{k+1} =
 * the 2 x 2 average of n_k ((a + b) + (c + d)) / 4 (maua_noise_reg_levels(R): 1 for 4 and 8, 2 for 16, 8 for 1024).  loss [B] (or NULL) =
 * the levels in order, x then y.  grad [B][R][R] (or NULL): weight d loss / d n, written (accumulate 0) or added to what is there - the
 * network's g_noise.  Closed form: level k gives 2 m_x / R_k^2 (left + right neighbour) + the same in y, plus a quarter of the coarser
 * level's gradient at [i / 2][j / 2] (the pooling's adjoint), from the coarsest level down. */
long maua_noise_reg_workspace_bytes(int B, int R);
int maua_noise_reg_levels(int R);
int maua_noise_reg_check(const float* n, int B, int R, const float* loss, const float* grad, const void* ws, long ws_bytes);
int maua_noise_reg(maua_ctx* ctx, const float* n, int B, int R, float weight, float* loss, float* grad, int accumulate, void* ws,
                   long ws_bytes);
/* One Adam update (torch.optim.Adam without amsgrad or weight decay) of param [n] from grad [n] with the moments m, v [n]:
 *   m = m + (1 - beta1) (g - m);  v = beta2 v + ((1 - beta2) g) g;  param = param - (step m) / (sqrt(v) inv_sqrt_bc2 + eps)
 * step = lr / (1 - beta1^t) and inv_sqrt_bc2 = 1 / sqrt(1 - beta2^t) are the caller's, computed in double on the host. */
int maua_adam_step_check(const float* param, const float* grad, const float* m, const float* v, long n, float beta1, float beta2, float eps);
int maua_adam_step(maua_ctx* ctx, float* param, const float* grad, float* m, float* v, long n, float beta1, float beta2, float eps,
                   float step, float inv_sqrt_bc2);
/* n [maps][N] in place, per map: n -= mean(n); n *= 1 / sqrt(mean(n^2)).  A constant map becomes 0 x inf = NaN, as the published
 * `buf -= buf.mean(); buf *= buf.square().mean().rsqrt()` makes it: not special-cased. */
long maua_noise_renorm_workspace_bytes(int maps, long N);
int maua_noise_renorm_check(const float* n, int maps, long N, const void* ws, long ws_bytes);
int maua_noise_renorm(maua_ctx* ctx, float* n, int maps, long N, void* ws, long ws_bytes);
/* ws [B][num_ws][w_dim] = w[b][r_in] + scale eps[b][r_in] (product, then sum); w and eps [B][w_rows][w_dim], w_rows = 1 (space w: r_in = 0)
 * or num_ws (space w+: r_in = r); eps may be NULL (ws = w).  maua_latent_reduce: the adjoint for space w, g_w [B][w_dim] = sum_r
 * g_ws[b][r], rows in order. */
int maua_latent_expand_check(const float* w, int w_rows, const float* eps, const float* ws, int B, int num_ws, int w_dim);
int maua_latent_expand(maua_ctx* ctx, const float* w, int w_rows, const float* eps, float scale, float* ws, int B, int num_ws, int w_dim);
int maua_latent_reduce_check(const float* g_ws, const float* g_w, int B, int num_ws, int w_dim);
int maua_latent_reduce(maua_ctx* ctx, const float* g_ws, float* g_w, int B, int num_ws, int w_dim);
/* Latent directions (csrc/latent.hip; the edit that follows sefa.py:7,25's factorisation): ws, out [T][num_ws][C], dirs [k][C], coeffs [T][k],
 * device f32.  Rows ws_lo <= l < ws_hi: out[t][l] = ws[t][l] + sum_j coeffs[t][j] dirs[j], j ascending, every term one fmaf(coeff, dir, acc)
 * starting from ws; every other row is copied.  An empty range or k = 0 copies ws.  out may not alias ws. */
int maua_latent_add_directions_check(const float* ws, const float* dirs, const float* coeffs, int T, int num_ws, int C, int k, int ws_lo, int ws_hi,
                                     const float* out);
int maua_latent_add_directions(maua_ctx* ctx, const float* ws, const float* dirs, const float* coeffs, int T, int num_ws, int C, int k, int ws_lo,
                               int ws_hi, float* out);

/* ---- neural cellular automaton (maua/nca/train.py:152-193, after znah's gitart_kunstformen_ca) ------------------------------------
 * One update of the f32 state x [B][chn][H][W]:  x += w2 . relu(w1 . perception(x) + b1) . mask
 *   perception: per channel, the circular 3 x 3 stencils {identity, sobel_x, sobel_x^T, laplacian} with the reference's un-normalised
 *               integer taps (train.py:153-169); feature 4 c + f (channel-major, what its reshape(b, -1, h, w) produces)
 *   mask:       floorf(u + rate) per pixel, shared by the channels; rate a scalar, or rate_map [H][W] (generate.py:57) when not NULL
 *   u:          the caller's device tensor u [n_steps][B][H][W], or (u == NULL) unit23 of word ((t B + b) H + y) W + x of the Philox
 *               stream (seed, stream) in maua_philox_u32's addressing, t = step0 + the step's index in this call: a run split into
 *               several calls, or into windows, draws the same masks.  oracle/rng.py u32 is the host twin.
 * One launch per step (steps_per_launch = 2, 4: per that many steps, on a halo advanced inside the workgroup, same bits) does perception, both products, bias, ReLU, mask and residual; nothing between them goes to memory.  Neighbours
 * read the old state, so the steps alternate between x and a buffer the handle owns and the result ends in x.  The parameters are read at
 * every call from the caller's device f32 tensors w1 [hidden][4 chn], b1 [hidden], w2 [chn][hidden] and staged into the operand layout
 * by the step kernel itself.  dtype selects the PRODUCTS, not the state: MAUA_F32 = exact v_mfma_f32_32x32x2_f32 (an f32 fma chain, the
 * parity mode), MAUA_F32_SPLIT = hi/lo bf16 operands and three products per k-step (lo x lo, <= 2^-16 of a product, is dropped).
 * Limits: chn a multiple of 4 up to 16, hidden a multiple of 32 up to 128; H, W >= 3; steps_per_launch 1, 2 or 4.
 * Window mode (W_sub > 0; generate.py:25-36's checkpoint grid): columns [col0, col0 + W_sub) of every row are a torus of width W_sub, and
 * only window columns [margin, W_sub - margin) are written back; W stays the row length of x, of rate_map and of u, and the Philox word
 * is addressed with the column in the whole row, so overlapping windows see one mask per pixel and step. */
/* perception alone (train.py:167-169), for callers that want the features: x [B][C][H][W] f32 -> out [B][4 C][H][W]; any C; H, W >= 3 */
int maua_nca_perception(maua_ctx* ctx, const float* x, int B, int C, int H, int W, float* out);
typedef struct maua_nca maua_nca;
typedef struct {
  float* x; int B, H, W;
  const float *w1, *b1, *w2;
  int n_steps;
  float rate; const float* rate_map;
  const float* u;
  unsigned long long seed, stream, step0;
  int col0, W_sub, margin;   /* W_sub = 0: the whole grid */
  int steps_per_launch;      /* 0 = 1; 2, 4: that many steps per launch (same bits; not in window mode or forward_keep) */
} maua_nca_desc;
int maua_nca_create(maua_ctx* ctx, int chn, int hidden, int dtype, maua_nca** out);
int maua_nca_destroy(maua_nca* handle);
/* host only, no device needed (handle may be NULL: then chn, hidden and dtype describe it): MAUA_OK, or MAUA_ERR + maua_last_error() with
 * maua_nca_step's own refusal.  Pointers are only checked, never dereferenced. */
int maua_nca_check(const maua_nca* handle, int chn, int hidden, int dtype, const maua_nca_desc* d);
/* n_steps updates of d->x in place, on the context's stream */
int maua_nca_step(maua_nca* handle, const maua_nca_desc* d);
/* the same steps from d->x (left as it is), every state kept: states [n_steps + 1][B][chn][H][W], states[0] = x.  No window mode. */
int maua_nca_forward_keep(maua_nca* handle, const maua_nca_desc* d, float* states);
/* The gradient of those n_steps updates: from the kept states and g_last = dL/dx_N [B][chn][H][W] to g_first = dL/dx_0 and the parameter
 * gradients dw1 [hidden][4 chn], db1 [hidden], dw2 [chn][hidden] (all written, not added to), walking the steps backwards.  d gives the
 * parameters, the rate and the masks' source exactly as it did to maua_nca_forward_keep (d->x is not read); no window mode.  Per step the
 * hidden layer is recomputed from the stored state with the forward's own summation (ReLU's mask is the forward's), g is masked,
 * dW2 += gy h^T, gh = (w2^T gy) [h > 0], dW1 += gh p^T, db1 += sum gh, g += perception^T(w1^T gh) (the circular stencils with flipped
 * taps).  Sums over pixels and steps run in a fixed order - per-workgroup partials carried across the steps, then one ordered reduce - so
 * two runs give identical bits.  Products are exact f32 whatever the handle's dtype.  g_first may not alias g_last. */
int maua_nca_vjp(maua_nca* handle, const maua_nca_desc* d, const float* states, const float* g_last, float* g_first, float* dw1, float* db1,
                 float* dw2);

/* ---- multi-GPU: the one exchange step of the frame-sharded render ------------------------------------
 * One process per GPU; frames are sharded by contiguous range (no data-path collective).  maua_gather_frames moves every
 * rank's packed u8 shard to `root`, ordered by rank, as grouped RCCL point-to-point transfers on the context's stream
 * (replaces the single-process frame list of maua/audiovisual/generate.py:57-98; process layout as
 * maua/super/image/bulk.py:31-109).  Bootstrap: rank 0 calls maua_comm_unique_id and hands the 128 bytes to the other
 * ranks out of band (torch.distributed broadcast, a file, MPI ...); every rank then calls maua_comm_init.  RCCL is bound
 * at first use (dlopen): single-GPU hosts never load it. */
typedef struct { char internal[128]; } maua_comm_id;   /* = ncclUniqueId */
typedef struct maua_comm maua_comm;
int maua_comm_unique_id(maua_comm_id* id);
int maua_comm_init(maua_ctx* ctx, const maua_comm_id* id, int rank, int world, maua_comm** out);
/* bytes_per_rank [world]: shard sizes (host array); send: this rank's shard (device); recv: root only, sum of the sizes. */
int maua_gather_frames(maua_comm* comm, const uint8_t* send, const long* bytes_per_rank, uint8_t* recv, int root);
/* one round of the STREAMED gather: rank r's piece (bytes_per_rank[r] bytes; 0 = not in this round) lands at byte
 * offsets_per_rank[r] of the root's clip buffer recv_base - the k-th finished chunk of every rank, sent on a side stream
 * while chunk k + 1 renders, so the root's ingress hides behind the render.  The root's own piece is not moved. */
int maua_gather_frames_at(maua_comm* comm, const uint8_t* send, const long* bytes_per_rank, uint8_t* recv_base,
                          const long* offsets_per_rank, int root);
/* the stream this communicator's transfers are enqueued on (default: the context's stream).  The streamed gather gives it a
 * side stream that waits on an event of the render stream, so that a round travels while the next chunk renders
 * (use_ctx_stream != 0: back to the context's stream). */
int maua_comm_set_stream(maua_comm* comm, void* stream, int use_ctx_stream);
/* the communicator's own rank count / rank (ncclCommCount, ncclCommUserRank): what a result line quotes as its RCCL world */
int maua_comm_count(maua_comm* comm, int* nranks, int* rank);
int maua_comm_destroy(maua_comm* comm);

#ifdef __cplusplus
}
#endif
#endif /* MAUA_HIP_H */
