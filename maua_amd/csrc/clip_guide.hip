// CLIPGrads around the image tower (clip.hip): per sampler step, `cutout_batches` times, cutouts of the current image estimate
// (cutouts.hip, cutout_augs.hip) go through the tower, the loss head and the way back, in groups that fit the workspace budget; the
// groups' gradients are summed in a fixed order, clamped and scaled.  Reference: maua/grad.py:96-165.
#include <cmath>

#include "clip_internal.h"

using namespace maua;

namespace maua {
namespace {

constexpr int NPARTS = 1024;

// clamp_gradient (grad.py:156-158): magnitude = sqrt(mean(grad^2)); grad *= min(magnitude, clamp) / magnitude - two launches, fixed
// partial layout
__global__ __launch_bounds__(256) void sq_partial_kernel(const float* __restrict__ g, long n, double* __restrict__ part) {
  __shared__ double red[256];
  double s = 0.0;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) s += (double)g[i] * g[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}
__global__ __launch_bounds__(256) void clamp_scale_kernel(float* __restrict__ g, long n, const double* __restrict__ part, int nparts, float clamp,
                                                          float scale) {
  // the partial sums once per workgroup, in a fixed order (every thread used to walk all 1024 of them: 0.86 ms for a 6 M-value gradient)
  __shared__ double red[256];
  double acc = 0.0;
  for (int i = threadIdx.x; i < nparts; i += 256) acc += part[i];
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  const double s = red[0];
  float f = scale;
  if (clamp > 0.f) {
    const float mag = sqrtf((float)(s / (double)n)) * fabsf(scale);
    if (mag > clamp) f *= clamp / mag;
  }
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) g[i] = (s != s) ? 0.f : g[i] * f;   // (a gradient holding a NaN counts as zeros: guided.py:262-265)
}

}  // namespace

void clip_stamp(maua_clip* n, unsigned long long* uid, unsigned long long* epoch) {
  *uid = n ? n->uid : 0;
  *epoch = n ? n->epoch : 0;
}
maua_ctx* clip_ctx(maua_clip* n) { return n ? n->ctx : nullptr; }

const float CLIP_MEAN[3] = {0.48145466f, 0.4578275f, 0.40821073f}, CLIP_STD[3] = {0.26862954f, 0.26130258f, 0.27577711f};   // grad.py:110

// one pass of N images (patch rows in n->patches) through the tower and back (their gradient in n->dwide's patch-row layout)
static int tower_pass(maua_clip* n, long N, int B, float coef, const float* mult_dev) {
  if (int rc = run_forward(n, N, true)) return rc;
  if (int rc = zero_dx(n, N)) return rc;
  if (int rc = run_head(n, N, true, nullptr, B, coef, true, mult_dev)) return rc;
  return run_backward(n, N);
}

// One cutout batch group of CLIPGrads.forward on device rectangles: cutouts of img -> tower -> loss head -> back to d img, added into
// (or written to) grad.  rects_dev: [n_cut][3].  coef: the head's factor (scale excluded: applied at the end with the clamp).
static int clip_grad_group(maua_clip* n, const float* img, int B, int H, int W, const int* rects_dev, const float* mult_dev, int n_cut,
                           float coef, float* grad, int accumulate) {
  hipStream_t st = n->ctx->stream;
  CutoutPlan p{};
  p.img = img; p.rects = rects_dev; p.B = B; p.H = H; p.W = W; p.n_cut = n_cut; p.cs = n->res; p.mul = 0.5f; p.add = 0.5f;
  for (int c = 0; c < 3; c++) { p.mean[c] = CLIP_MEAN[c]; p.std[c] = CLIP_STD[c]; }
  p.patch = n->patch; p.patch_ld = n->kpp;
  if (int rc = launch_cutout_tables(st, p, n->cut_tables)) return rc;
  if (int rc = launch_cutouts_forward(st, n->dtype, p, n->cut_tables, n->patches)) return rc;
  if (int rc = tower_pass(n, (long)n_cut * B, B, coef, mult_dev)) return rc;
  return launch_cutouts_vjp(st, n->dtype, p, n->cut_tables, n->dwide, n->cut_th, grad, accumulate);
}

// Cutouts per pass through the tower.  Shape bounds: 32-bit byte offsets inside the GEMM operands, <= 65535 images.  Byte budget:
// one pass keeps ws_bytes_per_image() of activations and workspace per image, plus the cutouts' own scratch (tables, the horizontal
// adjoint's rows, the augmented cutouts' two f32 buffers); the group is capped so that one pass fits in
//   * ws_limit, when maua_clip_set_workspace_limit set one, else
//   * the device's free memory now + what this tower's workspaces already hold, less a reserve of 1/8 of that and at least 2 GiB
//     (the networks beside the tower plan their own workspaces after this call; fragmentation).
// A cutout is B images and cannot be split: below that the call is refused with the bytes one cutout needs.
static size_t cutout_bytes(const maua_clip* n, int B, int H, int W, int aug_side) {   // of ONE cutout of the batch
  const size_t per_image = ws_bytes_per_image(n) + (size_t)3 * n->res * std::min(H, W) * 4 + (size_t)2 * 3 * aug_side * aug_side * 4;
  return per_image * (size_t)B + (size_t)n->res * (4 + 4 * 16) + 4;
}
static int group_size(maua_clip* n, int B, int H, int W, int cutn, int aug_side, int* out) {
  const long max_images = std::min<long>(65535, ((1L << 32) - 1) / ((long)n->Tk * 4 * n->width * (long)n->esize));
  long grp = std::max<long>(1, std::min<long>(cutn, max_images / std::max(B, 1)));
  const size_t one = cutout_bytes(n, B, H, W, aug_side);
  size_t budget = n->ws_limit;
  if (!budget) {
    size_t free_b = 0, total_b = 0;
    MAUA_HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
    const size_t avail = free_b + (size_t)n->cap * ws_bytes_per_image(n) * (n->keep ? 1 : 0);
    const size_t reserve = std::max<size_t>(avail / 8, (size_t)2 << 30);
    budget = avail > reserve ? avail - reserve : 0;
  }
  if (budget / one < (size_t)grp) grp = (long)(budget / one);
  if (grp < 1)
    return fail("maua_clip: one cutout of this batch (" + std::to_string(B) + " images) needs " + std::to_string(one) +
                " bytes of tower workspace, the budget is " + std::to_string(budget) +
                (n->ws_limit ? " (maua_clip_set_workspace_limit)" : " (free device memory less the reserve)"));
  *out = (int)grp;
  return MAUA_OK;
}

// workspaces of a guidance call (all allocations happen here, none inside clip_grad_group: a captured loop calls this first), and
// the group size its passes run with: fixed here, and kept while the batch shape, cutn and the limit stay the same - a captured loop
// replays it, and a call's float32 sum over groups keeps its order from call to call
int clip_prepare_guide(maua_clip* n, int B, int H, int W, int cutn, int aug_side) {
  MAUA_REQUIRE(n->tgt && n->P > 0, "maua_clip: no targets (maua_clip_set_targets)");
  if (!(n->grp > 0 && n->grp_B == B && n->grp_H == H && n->grp_W == W && n->grp_cutn == cutn && n->grp_aug == aug_side)) {
    int grp = 0;
    if (int rc = group_size(n, B, H, W, cutn, aug_side, &grp)) return rc;
    if (grp != n->grp) n->epoch++;   // (a captured loop holds the old split)
    n->grp = grp; n->grp_B = B; n->grp_H = H; n->grp_W = W; n->grp_cutn = cutn; n->grp_aug = aug_side;
  }
  const int n_cut_group = n->grp;
  if (int rc = ensure_ws(n, (long)n_cut_group * B, 1)) return rc;
  const size_t tb = cutouts_table_bytes(n_cut_group, n->res), thb = cutouts_th_bytes(n_cut_group, B, n->res, std::min(H, W));
  if (tb > n->cut_tables_bytes || thb > n->cut_th_bytes || !n->parts) {
    MAUA_HIP_CHECK(hipStreamSynchronize(n->ctx->stream));
    const size_t ntb = std::max(tb, n->cut_tables_bytes), nthb = std::max(thb, n->cut_th_bytes);
    n->cut_tables_bytes = n->cut_th_bytes = 0;
    n->epoch++;   // (the pieces move)
    auto layout = [&](Scratch& s) {
      n->cut_tables = s.take<char>(ntb); n->cut_th = (float*)s.take<char>(nthb); n->parts = s.take<double>(NPARTS);
    };
    if (int rc = carve_into(n->cut_ws, layout)) return rc;
    n->cut_tables_bytes = ntb; n->cut_th_bytes = nthb;
  }
  return MAUA_OK;
}

// The groups of a guidance call in their fixed order - body(k, c0, nc, accumulate): cutouts c0 .. c0 + nc of cutout batch k, written
// to (the first) or added into grad - then clamp_gradient and the scale
template <class Body>
static int guide_groups(maua_clip* n, int B, int H, int W, int cutn, int batches, float scale, float clamp_gradient, float* grad, Body body) {
  const int grp = n->grp;   // fixed by clip_prepare_guide; the gradient is the sum over groups in this fixed order
  bool first = true;
  for (int k = 0; k < batches; k++)
    for (int c0 = 0; c0 < cutn; c0 += grp) {
      if (int rc = body(k, c0, std::min(grp, cutn - c0), first ? 0 : 1)) return rc;
      first = false;
    }
  const long cnt = (long)B * 3 * H * W;
  hipStream_t st = n->ctx->stream;
  hipLaunchKernelGGL(sq_partial_kernel, dim3(NPARTS), dim3(256), 0, st, grad, cnt, n->parts);
  hipLaunchKernelGGL(clamp_scale_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, st, grad, cnt, n->parts, NPARTS, clamp_gradient,
                     scale);
  MAUA_HIP_CHECK(hipGetLastError());
  return MAUA_OK;
}

// the whole of CLIPGrads.forward (:145-159) on device rectangles [batches][cutn][3].  mult_dev: NULL, or [batches][cutn] multiplicities -
// cutout n stands for mult identical cutouts of the reference's list (on a square image its first cutn // 4 cutouts are the same
// rectangle, cutouts.py:16-27: one pass through the tower carries their weight) and cutn_total = what the multiplicities of a batch sum to
int clip_guide_grad(maua_clip* n, const float* img, int B, int H, int W, const int* rects_dev, const float* mult_dev, int cutn, int cutn_total,
                    int batches, float scale, float clamp_gradient, float* grad) {
  MAUA_REQUIRE(n->grp > 0 && n->grp_B == B && n->grp_cutn == cutn, "maua_clip: clip_prepare_guide was not called for this batch / cutn");
  const float coef = 1.f / ((float)cutn_total * (float)batches);
  return guide_groups(n, B, H, W, cutn, batches, scale, clamp_gradient, grad, [&](int k, int c0, int nc, int accumulate) {
    const long i0 = (long)k * cutn + c0;
    return clip_grad_group(n, img, B, H, W, rects_dev + i0 * 3, mult_dev ? mult_dev + i0 : nullptr, nc, coef, grad, accumulate);
  });
}

// One cutout group of CLIPGrads.forward with augmented cutouts (cutout_augs.hip).  "normal" (per_call 0): the group's n_cut records
// augment their crops of img into per-cutout slots (aug_x2), the resize reads slot n for cutout n (slot_rects: (size, 0, 0)); back:
// resize VJP per slot -> augmentation adjoint -> the crops' gradients summed into grad in cutout order.  "dango" (per_call 1): the
// resize writes planar [n_cut B][3][cs][cs] (aug_x2), the call's one record augments it into the tower's patch rows; back: patch-row
// gradient -> adjoint -> the existing cutouts VJP.  noise_i0: the group's first image in the call's [N B] noise layout ("dango").
static int clip_grad_group_aug(maua_clip* n, const float* img, int B, int H, int W, const int* rects_dev, const int* slot_rects_dev,
                               const void* recs, int n_cut, int per_call, int noise_i0, float coef, float* grad, int accumulate) {
  hipStream_t st = n->ctx->stream;
  const long N = (long)n_cut * B;
  const float zero3[3] = {0.f, 0.f, 0.f}, one3[3] = {1.f, 1.f, 1.f};
  CutoutPlan p{};
  p.B = B; p.n_cut = n_cut; p.cs = n->res;
  if (!per_call) {
    const int S = std::min(H, W);
    if (int rc = aug_forward_src(st, recs, n_cut, B, S, 0, img, H, W, 0.5f, 0.5f, n->aug_x1.as<float>())) return rc;
    if (int rc = aug_forward_out(st, MAUA_F32, recs, n_cut, B, S, 0, n->aug_x1.as<float>(), n->aug_x2.as<float>(), 0, zero3, one3)) return rc;
    p.img = n->aug_x2.as<float>(); p.rects = slot_rects_dev; p.H = S; p.W = S; p.mul = 1.f; p.add = 0.f; p.img_stride = (long)B * 3 * S * S;
    for (int c = 0; c < 3; c++) { p.mean[c] = CLIP_MEAN[c]; p.std[c] = CLIP_STD[c]; }
    p.patch = n->patch; p.patch_ld = n->kpp;
    if (int rc = launch_cutout_tables(st, p, n->cut_tables)) return rc;
    if (int rc = launch_cutouts_forward(st, n->dtype, p, n->cut_tables, n->patches)) return rc;
    if (int rc = tower_pass(n, N, B, coef, nullptr)) return rc;
    if (int rc = launch_cutouts_vjp(st, n->dtype, p, n->cut_tables, n->dwide, n->cut_th, n->aug_x2.as<float>(), 0)) return rc;
    if (int rc = aug_adjoint_out(st, MAUA_F32, recs, n_cut, B, S, n->aug_x2.as<float>(), 0, one3, n->aug_x1.as<float>())) return rc;
    return aug_adjoint_src(st, recs, n_cut, B, S, n->aug_x1.as<float>(), H, W, 0.5f, grad, accumulate);
  }
  const int cs = n->res;
  p.img = img; p.rects = rects_dev; p.H = H; p.W = W; p.mul = 0.5f; p.add = 0.5f;
  for (int c = 0; c < 3; c++) { p.mean[c] = 0.f; p.std[c] = 1.f; }
  if (int rc = launch_cutout_tables(st, p, n->cut_tables)) return rc;
  if (int rc = launch_cutouts_forward(st, MAUA_F32, p, n->cut_tables, n->aug_x2.as<float>())) return rc;
  if (int rc = aug_forward_src(st, recs, 1, (int)N, cs, noise_i0, n->aug_x2.as<float>(), cs, cs, 1.f, 0.f, n->aug_x1.as<float>())) return rc;
  if (int rc = aug_forward_out(st, n->dtype, recs, 1, (int)N, cs, noise_i0, n->aug_x1.as<float>(), n->patches, n->patch, CLIP_MEAN, CLIP_STD, n->kpp)) return rc;
  if (int rc = tower_pass(n, N, B, coef, nullptr)) return rc;
  if (int rc = aug_adjoint_out(st, n->dtype, recs, 1, (int)N, cs, n->dwide, n->patch, CLIP_STD, n->aug_x2.as<float>(), n->kpp)) return rc;
  if (int rc = aug_adjoint_src(st, recs, 1, (int)N, cs, n->aug_x2.as<float>(), cs, cs, 1.f, n->aug_x1.as<float>(), 0)) return rc;
  return launch_cutouts_vjp(st, MAUA_F32, p, n->cut_tables, n->aug_x1.as<float>(), n->cut_th, grad, accumulate);
}

// every rectangle (size | flags, top, left) lies inside the image; flags: the grey / mirror bits are allowed
static int check_rects(const std::string& who, const int* rects, long count, int H, int W, bool flags) {
  for (long i = 0; i < count; i++) {
    const int s = rects[3 * i] & CUT_SIZE_MASK, oy = rects[3 * i + 1], ox = rects[3 * i + 2];
    MAUA_REQUIRE(s > 0 && oy >= 0 && ox >= 0 && oy + s <= H && ox + s <= W, who + ": a cutout leaves the image");
    MAUA_REQUIRE(flags || (rects[3 * i] & ~CUT_SIZE_MASK) == 0, who + ": \"normal\" cutouts carry no grey / flip flags");
  }
  return MAUA_OK;
}

}  // namespace maua

extern "C" {

// CLIPGrads.set_targets' result (:117-143): S sets of P target embeddings [S][P][E] (host or device floats are both copied with
// hipMemcpyDefault; normalised here like spherical_dist_loss does) and prompt weights [S][P] (already divided by |sum|).  sel: per
// sample of a batch the set it is guided towards ([B] host ints, audio-switched prompts) or NULL (set 0 for everybody)
int maua_clip_set_targets(maua_clip* n, const float* targets, const float* weights, int S, int P, const int* sel, int B) {
  MAUA_REQUIRE(n && targets && weights && S > 0 && P > 0, "maua_clip_set_targets: bad arguments");
  MAUA_HIP_CHECK(hipStreamSynchronize(n->ctx->stream));
  std::vector<float> t((size_t)S * P * n->E), wv((size_t)S * P);
  MAUA_HIP_CHECK(hipMemcpy(t.data(), targets, t.size() * 4, hipMemcpyDefault));
  MAUA_HIP_CHECK(hipMemcpy(wv.data(), weights, wv.size() * 4, hipMemcpyDefault));
  for (long r = 0; r < (long)S * P; r++) {
    double ss = 0;
    for (int j = 0; j < n->E; j++) ss += (double)t[r * n->E + j] * t[r * n->E + j];
    const float nn = std::max((float)std::sqrt(ss), 1e-12f);
    for (int j = 0; j < n->E; j++) t[r * n->E + j] /= nn;
  }
  if (t.size() * 4 != n->tgt.bytes() || wv.size() * 4 != n->twt.bytes()) {
    n->epoch++;
    if (int rc = n->tgt.alloc(t.size() * 4)) return rc;
    if (int rc = n->twt.alloc(wv.size() * 4)) return rc;
  }
  MAUA_HIP_CHECK(hipMemcpy(n->tgt.as<float>(), t.data(), t.size() * 4, hipMemcpyHostToDevice));
  MAUA_HIP_CHECK(hipMemcpy(n->twt.as<float>(), wv.data(), wv.size() * 4, hipMemcpyHostToDevice));
  n->S = S; n->P = P;
  n->sel_B = 0;
  if (sel) {
    MAUA_REQUIRE(B > 0, "maua_clip_set_targets: sel needs the batch size");
    for (int b = 0; b < B; b++) MAUA_REQUIRE(sel[b] >= 0 && sel[b] < S, "maua_clip_set_targets: sel out of range");
    if ((size_t)B * 4 > n->sel.bytes()) {
      n->epoch++;
      if (int rc = n->sel.alloc((size_t)B * 4)) return rc;
    }
    MAUA_HIP_CHECK(hipMemcpy(n->sel.as<int>(), sel, (size_t)B * 4, hipMemcpyHostToDevice));
    n->sel_B = B;
  }
  return MAUA_OK;
}

// CLIPGrads.forward (:145-159): img [B][3][H][W] f32 in [-1, 1] (device), rects: HOST ints [batches][cutn][3] = (size, top, left) of
// every cutout of every cutout batch (what MauaCutouts draws), -> grad [B][3][H][W] f32 = d (scale * sum_b loss_b) / d img, averaged
// over the cutout batches, with clamp_gradient (<= 0: none) applied
int maua_clip_guide_grad(maua_clip* n, const float* img, int B, int H, int W, const int* rects, const float* mult, int cutn, int batches,
                         float scale, float clamp_gradient, float* grad) {
  MAUA_REQUIRE(n && img && rects && grad, "maua_clip_guide_grad: NULL argument");
  MAUA_REQUIRE(B >= 0 && cutn > 0 && batches > 0, "maua_clip_guide_grad: bad sizes");
  if (int rc = clip_loaded(n)) return rc;
  if (B == 0) return MAUA_OK;
  MAUA_REQUIRE(n->sel_B == 0 || n->sel_B == B, "maua_clip_guide_grad: the per-sample target selection was set for another batch size");
  if (int rc = check_rects("maua_clip_guide_grad", rects, (long)batches * cutn, H, W, true)) return rc;
  int cutn_total = cutn;
  if (mult) {
    double tot = 0;
    for (int i = 0; i < cutn; i++) tot += mult[i];
    cutn_total = (int)(tot + 0.5);
    for (int k = 1; k < batches; k++) {
      double t = 0;
      for (int i = 0; i < cutn; i++) t += mult[(long)k * cutn + i];
      MAUA_REQUIRE((int)(t + 0.5) == cutn_total, "maua_clip_guide_grad: every cutout batch must stand for the same number of cutouts");
    }
    MAUA_REQUIRE(cutn_total >= cutn, "maua_clip_guide_grad: multiplicities are >= 1");
  }
  const size_t cnt = (size_t)batches * cutn * 4;   // 3 ints + 1 float per cutout
  if (cnt * 4 > n->rects_dev.bytes()) {
    MAUA_HIP_CHECK(hipStreamSynchronize(n->ctx->stream));
    if (int rc = n->rects_dev.alloc(cnt * 4)) return rc;
  }
  float* mult_dev = mult ? (float*)(n->rects_dev.as<int>() + (size_t)batches * cutn * 3) : nullptr;
  MAUA_HIP_CHECK(hipMemcpyAsync(n->rects_dev.as<int>(), rects, (size_t)batches * cutn * 12, hipMemcpyHostToDevice, n->ctx->stream));
  if (mult) MAUA_HIP_CHECK(hipMemcpyAsync(mult_dev, mult, (size_t)batches * cutn * 4, hipMemcpyHostToDevice, n->ctx->stream));
  MAUA_HIP_CHECK(hipStreamSynchronize(n->ctx->stream));   // (the caller's arrays may be temporaries)
  if (int rc = clip_prepare_guide(n, B, H, W, cutn)) return rc;
  return clip_guide_grad(n, img, B, H, W, n->rects_dev.as<int>(), mult_dev, cutn, cutn_total, batches, scale, clamp_gradient, grad);
}

// CLIPGrads.forward with augmented "normal" (per_call 0) / "dango" (per_call 1) cutouts: maua_clip_guide_grad with, per cutout batch,
// the augmentation records (HOST float [batches][cutn][17] / [batches][17]) and the noise key (HOST [batches])
int maua_clip_guide_grad_aug(maua_clip* n, const float* img, int B, int H, int W, const int* rects, int cutn, int batches, const float* augs,
                             const unsigned long long* keys, int per_call, float scale, float clamp_gradient, float* grad) {
  MAUA_REQUIRE(n && img && rects && augs && keys && grad, "maua_clip_guide_grad_aug: NULL argument");
  MAUA_REQUIRE(B >= 0 && cutn > 0 && batches > 0, "maua_clip_guide_grad_aug: bad sizes");
  MAUA_REQUIRE(per_call == 0 || per_call == 1, "maua_clip_guide_grad_aug: per_call is 0 (\"normal\") or 1 (\"dango\")");
  if (int rc = clip_loaded(n)) return rc;
  if (B == 0) return MAUA_OK;
  MAUA_REQUIRE(n->sel_B == 0 || n->sel_B == B, "maua_clip_guide_grad_aug: the per-sample target selection was set for another batch size");
  const long total = (long)batches * cutn;
  if (int rc = check_rects("maua_clip_guide_grad_aug", rects, total, H, W, per_call != 0)) return rc;
  MAUA_REQUIRE(per_call || H == W, "maua_clip_guide_grad_aug: \"normal\" cutouts need a square image");
  const int n_rec = per_call ? batches : (int)total;
  std::vector<char> recs((size_t)n_rec * aug_record_bytes());
  if (int rc = aug_records(augs, n_rec, per_call ? nullptr : rects, n->res, keys, per_call ? 1 : cutn, recs.data())) return rc;
  hipStream_t st = n->ctx->stream;
  const int S = per_call ? n->res : std::min(H, W);
  if (int rc = clip_prepare_guide(n, B, H, W, cutn, S)) return rc;
  const size_t xb = (size_t)n->grp * B * 3 * S * S * 4;
  if ((size_t)total * 24 > n->aug_rects.bytes() || recs.size() > n->aug_recs.bytes() || xb > n->aug_x1.bytes() || xb > n->aug_x2.bytes()) {
    MAUA_HIP_CHECK(hipStreamSynchronize(st));
    n->epoch++;
    if (int rc = n->aug_rects.reserve((size_t)total * 24)) return rc;
    if (int rc = n->aug_recs.reserve(recs.size())) return rc;
    if (int rc = n->aug_x1.reserve(xb)) return rc;
    if (int rc = n->aug_x2.reserve(xb)) return rc;
  }
  std::vector<int> slot((size_t)total * 3);
  for (long i = 0; i < total; i++) { slot[3 * i] = rects[3 * i] & CUT_SIZE_MASK; slot[3 * i + 1] = 0; slot[3 * i + 2] = 0; }
  MAUA_HIP_CHECK(hipMemcpyAsync(n->aug_rects.as<int>(), rects, (size_t)total * 12, hipMemcpyHostToDevice, st));
  MAUA_HIP_CHECK(hipMemcpyAsync(n->aug_rects.as<int>() + 3 * total, slot.data(), (size_t)total * 12, hipMemcpyHostToDevice, st));
  MAUA_HIP_CHECK(hipMemcpyAsync(n->aug_recs.get(), recs.data(), recs.size(), hipMemcpyHostToDevice, st));
  MAUA_HIP_CHECK(hipStreamSynchronize(st));   // (the host vectors die with this call)
  const float coef = 1.f / ((float)cutn * (float)batches);
  const size_t rb = aug_record_bytes();
  return guide_groups(n, B, H, W, cutn, batches, scale, clamp_gradient, grad, [&](int k, int c0, int nc, int accumulate) {
    const long i0 = (long)k * cutn + c0;
    const void* rp = (const char*)n->aug_recs.get() + (per_call ? (size_t)k : (size_t)i0) * rb;
    return clip_grad_group_aug(n, img, B, H, W, n->aug_rects.as<int>() + 3 * i0, n->aug_rects.as<int>() + 3 * (total + i0), rp, nc, per_call, c0 * B, coef, grad,
                               accumulate);
  });
}

// sum_p w_p dist_p of each cutout image of the LAST pass through the tower ([n] floats, device; n <= cutn * B: cutout-major, what
// `dists.view(-1, B, P).mul(weights).sum(2)` holds in grad.py:153)
int maua_clip_last_image_losses(maua_clip* n, int count, float* out) {
  MAUA_REQUIRE(n && out && count >= 0 && count <= n->kept_N, "maua_clip_last_image_losses: more values asked for than the last pass had images");
  MAUA_HIP_CHECK(hipMemcpyAsync(out, n->loss, (size_t)count * 4, hipMemcpyDeviceToDevice, n->ctx->stream));
  return MAUA_OK;
}

}  // extern "C"
