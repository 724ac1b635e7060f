// The secondary diffusion model of the reference's DEFAULT guidance speed ("fast") - forward AND the vector-Jacobian product with
// respect to its input, evaluated by hand on the transposed network (the library has no autograd).
//
// Replaces (reference): maua/diffusion/processors/guided.py:68-143 (SecondaryDiffusionImageNet2: FourierFeatures timestep planes,
// 24 3x3 convolutions + ReLU, five AvgPool2d(2) / bilinear-x2 levels, skip concatenations; forward -> v, pred = x alpha - v sigma,
// eps = x sigma + v alpha) and the torch.autograd.grad(img, x, img_grad) of :236-272 that back-propagates through it.
//
//   forward :  h = [x | emb(t)] -> c0 -> c1 = s0 | down -> c2 -> c3 = s1 | down -> c4 -> c5 = s2 | down -> c6 -> c7 = s3 | down -> c8 -> c9 = s4
//              | down -> c10 .. c13 -> up -> [. | s4] -> c14 -> c15 -> up -> [. | s3] -> c16 -> c17 -> up -> [. | s2] -> c18 -> c19 -> up -> [. | s1]
//              -> c20 -> c21 -> up -> [. | s0] -> c22 -> c23 = v                                        (channels 64 128 128 256 256 512)
//   vjp     :  the same graph backwards: a 3x3 convolution's input gradient is the 3x3 convolution with the transposed, flipped
//              kernel (prepared at load time: the caller hands both layouts), ReLU's is the mask of the STORED forward activation,
//              AvgPool2d's is a quarter of the gradient at each of the four pixels, the bilinear up-sampling's is its adjoint
//              (gathered per input pixel from the <= 4 x 4 output pixels it touches, same clamped-source rule), a concatenation's
//              is the split; where a skip leaves (s_k feeds both the pool and the concatenation) the two gradients add.
//
// MI355X design: everything NHWC in the network dtype, concatenations are channel slices of one buffer (the convolutions write
// slices, the pool reads them: no copies), all 48 convolutions run on the MFMA implicit-GEMM kernel of modconv.hip (a plain
// convolution = unit styles, no demodulation; ReLU = leaky ReLU with slope 0 on its fast epilogue), the element-wise steps are
// 16-byte streaming kernels with the mask / add / pool-gradient fused.  Forward keeps every activation (13.9 M parameters, about 1 GB
// of activations per 16 samples at 256^2 in bf16); vjp() consumes the state of the LAST forward of the same shape.
#include <atomic>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "common.h"
#include "internal.h"
#include "plain_conv.h"

using namespace maua;

namespace {

constexpr int NCONV = 24;
constexpr int CS[6] = {64, 128, 128, 256, 256, 512};

__device__ __forceinline__ void bil_src(int o, int n, int& i0, int& i1, float& f) {
#pragma clang fp contract(off)
  // F.interpolate(scale_factor=2, mode="bilinear", align_corners=False): src = (o + 0.5) / 2 - 0.5, clamped at 0
  float s = fmaxf((o + 0.5f) * 0.5f - 0.5f, 0.f);
  i0 = (int)s;
  i1 = min(i0 + 1, n - 1);
  f = s - (float)i0;
}

// in0[p][0..2] = x, [3..18] = cos / sin(2 pi t w_k) (FourierFeatures :57-66), [19..31] = 0
template <typename T>
__global__ __launch_bounds__(256) void sec_input_kernel(const float* __restrict__ x, const float* __restrict__ t,
                                                        const float* __restrict__ wemb, T* __restrict__ out, int B, long HW) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)B * HW) return;
  const long b = idx / HW, p = idx - b * HW;
  const float tb = t[b];
  T* o = out + idx * 32;
#pragma unroll
  for (int c = 0; c < 3; c++) Elem<T>::store(o + c, x[(b * 3 + c) * HW + p]);
#pragma unroll
  for (int k = 0; k < 8; k++) {
    const float f = 2.f * 3.14159265358979323846f * tb * wemb[k];
    Elem<T>::store(o + 3 + k, cosf(f));
    Elem<T>::store(o + 11 + k, sinf(f));
  }
#pragma unroll
  for (int c = 19; c < 32; c++) Elem<T>::store(o + c, 0.f);
}

// AvgPool2d(2): src = C channels at src (pixel stride sps), H x W -> dense [H/2][W/2][C]
template <typename T>
__global__ __launch_bounds__(256) void avgpool2_kernel(const T* __restrict__ src, int sps, T* __restrict__ dst, int B, int H, int W,
                                                       int C) {
  constexpr int E = 16 / (int)sizeof(T);
  const int ppp = C / E, h2 = H / 2, w2 = W / 2;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)B * h2 * w2 * ppp) return;
  const int pc = (int)(idx % ppp);
  long p = idx / ppp;
  const int x = (int)(p % w2); p /= w2;
  const int y = (int)(p % h2);
  const int b = (int)(p / h2);
  float v[E];
#pragma unroll
  for (int e = 0; e < E; e++) v[e] = 0.f;
#pragma unroll
  for (int dy = 0; dy < 2; dy++)
#pragma unroll
    for (int dx = 0; dx < 2; dx++) {
      const T* s = src + (((long)b * H + 2 * y + dy) * W + 2 * x + dx) * sps + pc * E;
#pragma unroll
      for (int e = 0; e < E; e++) v[e] += Elem<T>::load(s + e);
    }
  T* d = dst + (((long)b * h2 + y) * w2 + x) * C + pc * E;
#pragma unroll
  for (int e = 0; e < E; e++) Elem<T>::store(d + e, v[e] * 0.25f);
}

// bilinear x2: dense [h][w][C] -> C channels at dst (pixel stride dps) of the [2h][2w] grid.  The order is pinned: every product and
// sum of the expression below rounds once (plain operators, contraction off in this body - the pragma is lexical), so the map and its
// adjoint are the same float32 numbers on every build; tests/diffusion_ref.py restates both.
template <typename T>
__global__ __launch_bounds__(256) void bilinear_up2_kernel(const T* __restrict__ src, T* __restrict__ dst, int dps, int B, int h, int w,
                                                           int C) {
#pragma clang fp contract(off)
  constexpr int E = 16 / (int)sizeof(T);
  const int ppp = C / E;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)B * 4 * h * w * ppp) return;
  const int pc = (int)(idx % ppp);
  long p = idx / ppp;
  const int ox = (int)(p % (2 * w)); p /= 2 * w;
  const int oy = (int)(p % (2 * h));
  const int b = (int)(p / (2 * h));
  int y0, y1, x0, x1;
  float fy, fx;
  bil_src(oy, h, y0, y1, fy);
  bil_src(ox, w, x0, x1, fx);
  const T* s = src + (long)b * h * w * C + pc * E;
  float v[E];
#pragma unroll
  for (int e = 0; e < E; e++) {
    const float a = Elem<T>::load(s + ((long)y0 * w + x0) * C + e), bq = Elem<T>::load(s + ((long)y0 * w + x1) * C + e);
    const float c = Elem<T>::load(s + ((long)y1 * w + x0) * C + e), d = Elem<T>::load(s + ((long)y1 * w + x1) * C + e);
    v[e] = (1.f - fy) * ((1.f - fx) * a + fx * bq) + fy * ((1.f - fx) * c + fx * d);
  }
  T* o = dst + (((long)b * 2 * h + oy) * 2 * w + ox) * dps + pc * E;
#pragma unroll
  for (int e = 0; e < E; e++) Elem<T>::store(o + e, v[e]);
}

// the adjoint of bilinear_up2: g_in[y][x] = sum over the output pixels that read (y, x) of their weight x g_out, rows then columns
// ascending, each term (wy wx) g rounded at the product of the weights, at the product with g and at the sum; then the ReLU
// mask of the stored activation `act` (dense [h][w][C]; NULL: none).  gout: C channels at pixel stride gps of the [2h][2w] grid.
template <typename T>
__global__ __launch_bounds__(256) void bilinear_up2_adjoint_kernel(const T* __restrict__ gout, int gps, const T* __restrict__ act,
                                                                   T* __restrict__ gin, int B, int h, int w, int C) {
#pragma clang fp contract(off)
  constexpr int E = 16 / (int)sizeof(T);
  const int ppp = C / E;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)B * h * w * ppp) return;
  const int pc = (int)(idx % ppp);
  long p = idx / ppp;
  const int x = (int)(p % w); p /= w;
  const int y = (int)(p % h);
  const int b = (int)(p / h);
  float v[E];
#pragma unroll
  for (int e = 0; e < E; e++) v[e] = 0.f;
  for (int oy = max(2 * y - 1, 0); oy <= min(2 * y + 2, 2 * h - 1); oy++) {
    int y0, y1;
    float fy;
    bil_src(oy, h, y0, y1, fy);
    const float wy = (y0 == y ? 1.f - fy : 0.f) + (y1 == y ? fy : 0.f);
    if (wy == 0.f) continue;
    for (int ox = max(2 * x - 1, 0); ox <= min(2 * x + 2, 2 * w - 1); ox++) {
      int x0, x1;
      float fx;
      bil_src(ox, w, x0, x1, fx);
      const float wx = (x0 == x ? 1.f - fx : 0.f) + (x1 == x ? fx : 0.f);
      if (wx == 0.f) continue;
      const T* g = gout + (((long)b * 2 * h + oy) * 2 * w + ox) * gps + pc * E;
#pragma unroll
      for (int e = 0; e < E; e++) v[e] += wy * wx * Elem<T>::load(g + e);
    }
  }
  const long o = (((long)b * h + y) * w + x) * C + pc * E;
#pragma unroll
  for (int e = 0; e < E; e++) {
    const bool on = !act || Elem<T>::load(act + o + e) > 0.f;
    Elem<T>::store(gin + o + e, on ? v[e] : 0.f);
  }
}

// g[p][c] *= (act[p][c] > 0): dense g, act with pixel stride aps
template <typename T>
__global__ __launch_bounds__(256) void relu_mask_kernel(T* __restrict__ g, const T* __restrict__ act, int aps, long n_pix, int C) {
  constexpr int E = 16 / (int)sizeof(T);
  const int ppp = C / E;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n_pix * ppp) return;
  const long p = idx / ppp;
  const int c = (int)(idx - p * ppp) * E;
#pragma unroll
  for (int e = 0; e < E; e++)
    if (!(Elem<T>::load(act + p * aps + c + e) > 0.f)) Elem<T>::store(g + p * C + c + e, 0.f);
}

// where a skip leaves: g_skip[p][c] = (act > 0) ? gcat[p][c] + 0.25 * gpool[p / 2][c] : 0
// (gcat / act: C channels at pixel stride cps of the H x W grid; gpool dense [H/2][W/2][C]; out dense [H][W][C])
template <typename T>
__global__ __launch_bounds__(256) void skip_grad_kernel(const T* __restrict__ gcat, const T* __restrict__ act, int cps,
                                                        const T* __restrict__ gpool, T* __restrict__ out, int B, int H, int W, int C) {
  constexpr int E = 16 / (int)sizeof(T);
  const int ppp = C / E;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)B * H * W * ppp) return;
  const int pc = (int)(idx % ppp);
  long p = idx / ppp;
  const int x = (int)(p % W); p /= W;
  const int y = (int)(p % H);
  const int b = (int)(p / H);
  const long pi = ((long)b * H + y) * W + x;
  const long pp = (((long)b * (H / 2) + (y >> 1)) * (W / 2) + (x >> 1)) * C + pc * E;
#pragma unroll
  for (int e = 0; e < E; e++) {
    const float a = Elem<T>::load(act + pi * cps + pc * E + e);
    const float v = Elem<T>::load(gcat + pi * cps + pc * E + e) + 0.25f * Elem<T>::load(gpool + pp + e);
    Elem<T>::store(out + pi * C + pc * E + e, a > 0.f ? v : 0.f);
  }
}

// v (first 3 of 32 channels, NHWC) -> v / pred / eps as planar f32 (any NULL skipped): pred = x alpha - v sigma, eps = x sigma + v alpha
template <typename T>
__global__ __launch_bounds__(256) void sec_output_kernel(const T* __restrict__ vn, const float* __restrict__ x, const float* __restrict__ t,
                                                         float* __restrict__ v_out, float* __restrict__ pred, float* __restrict__ eps,
                                                         int B, long HW) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)B * HW) return;
  const long b = idx / HW, p = idx - b * HW;
  const float ang = t[b] * 1.57079632679489661923f;
  const float al = cosf(ang), si = sinf(ang);
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const float v = Elem<T>::load(vn + idx * 32 + c);
    const long o = (b * 3 + c) * HW + p;
    const float xv = x[o];
    if (v_out) v_out[o] = v;
    if (pred) pred[o] = xv * al - v * si;
    if (eps) eps[o] = xv * si + v * al;
  }
}

// planar f32 [B][3][HW] -> NHWC T [.][32] (channels 3.. zero)
template <typename T>
__global__ __launch_bounds__(256) void sec_grad_in_kernel(const float* __restrict__ g, T* __restrict__ out, int B, long HW) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)B * HW) return;
  const long b = idx / HW, p = idx - b * HW;
#pragma unroll
  for (int c = 0; c < 32; c++) Elem<T>::store(out + idx * 32 + c, c < 3 ? g[(b * 3 + c) * HW + p] : 0.f);
}

// NHWC T [.][32] -> planar f32 [B][3][HW]
template <typename T>
__global__ __launch_bounds__(256) void sec_grad_out_kernel(const T* __restrict__ g, float* __restrict__ out, int B, long HW) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)B * HW) return;
  const long b = idx / HW, p = idx - b * HW;
#pragma unroll
  for (int c = 0; c < 3; c++) out[(b * 3 + c) * HW + p] = Elem<T>::load(g + idx * 32 + c);
}

}  // namespace

struct maua_secondary {
  maua_ctx* ctx;
  // identity of this model and of its device buffers: a captured graph that holds pointers into them (sampler.hip's guided loop) is valid
  // for one (uid, epoch) only.  uid is never reused (an allocator may hand a later model the freed one's address); epoch moves whenever
  // a workspace or table is freed or reallocated.
  unsigned long long uid = 0, epoch = 0;
  int dtype;
  int conv_dtype;
  size_t esize;
  PlainConv conv[NCONV];   // padded to 32 channels, each with its transposed copy
  DevBuf wemb;             // float [8] FourierFeatures weight
  UnitStyles ones;         // [bcap][512]
  // activations of the last forward and the gradient workspaces: one set carved from ws (grow-only); see forward_t for the layout
  DevBuf ws;
  size_t cap_px = 0;       // B * H * W the pieces were placed for
  int B = 0, H = 0, W = 0; // shape of the last forward (0: none)
  void* in0 = nullptr;
  void* a[5] = {};         // first conv of each level: a[0] = c0 out, a[k] = c(2k) out
  void* cat[5] = {};       // [up(main) | skip] per level
  void* pool[5] = {};      // pool[k] = down(skip k-1) (k = 1..5; index k-1)
  void* bott[4] = {};      // c10 .. c13 outputs
  void* dec[9] = {};       // c14 .. c22 outputs
  void* vbuf = nullptr;    // c23 output (32 channels, 3 real)
  // gradient workspaces (vjp)
  void *ga = nullptr, *gb = nullptr, *gcat = nullptr, *gpool = nullptr;
};

namespace {

int level_ch_main(int k) { return k == 0 ? CS[0] : k == 1 ? CS[1] : k == 2 ? CS[2] : k == 3 ? CS[3] : CS[4]; }   // channels of up(main) at level k
int level_ch_skip(int k) { return CS[k]; }                                                                      // ... of the skip s_k

// the 24 convolutions in execution order: channels in / out (guided.py:77-134)
void conv_plan(int (&ci)[NCONV], int (&co)[NCONV]) {
  const int c0 = CS[0], c1 = CS[1], c2 = CS[2], c3 = CS[3], c4 = CS[4], c5 = CS[5];
  const int I[NCONV] = {19, c0, c0, c1, c1, c2, c2, c3, c3, c4, c4, c5, c5, c5, 2 * c4, c4, 2 * c3, c3, 2 * c2, c2, 2 * c1, c1, 2 * c0, c0};
  const int O[NCONV] = {c0, c0, c1, c1, c2, c2, c3, c3, c4, c4, c5, c5, c5, c4, c4, c3, c3, c2, c2, c1, c1, c0, c0, 3};
  for (int i = 0; i < NCONV; i++) { ci[i] = I[i]; co[i] = O[i]; }
}

template <typename T>
int ensure_ws(maua_secondary* n, int B, int H, int W) {
  hipStream_t st = n->ctx->stream;
  const size_t px = (size_t)B * H * W, es = n->esize;
  if (px > n->cap_px) {
    MAUA_HIP_CHECK(hipStreamSynchronize(st));
    n->cap_px = 0;
    n->B = n->H = n->W = 0;
    n->epoch++;
    auto layout = [&](Scratch& s) {
      auto take = [&](size_t elems) -> void* { return s.take<char>(elems * es); };
      n->in0 = take(px * 32);
      n->vbuf = take(px * 32);
      for (int k = 0; k < 5; k++) {
        const size_t lp = px >> (2 * k);
        n->a[k] = take(lp * CS[k]);
        n->cat[k] = take(lp * (level_ch_main(k) + level_ch_skip(k)));
        n->pool[k] = take((lp >> 2) * CS[k]);
      }
      const size_t l5 = px >> 10;
      const int bc[4] = {CS[5], CS[5], CS[5], CS[4]};
      for (int i = 0; i < 4; i++) n->bott[i] = take(l5 * bc[i]);
      // decoder outputs: c14, c15 at level 4; c16, c17 at 3; c18, c19 at 2; c20, c21 at 1; c22 at 0
      const int dc[9] = {CS[4], CS[3], CS[3], CS[2], CS[2], CS[1], CS[1], CS[0], CS[0]};
      const int dl[9] = {4, 4, 3, 3, 2, 2, 1, 1, 0};
      for (int i = 0; i < 9; i++) n->dec[i] = take((px >> (2 * dl[i])) * dc[i]);
      // gradient workspaces: the widest tensors of the backward pass are the level-0 ones (128 channels)
      n->ga = take(px * 128);
      n->gb = take(px * 128);
      n->gcat = take(px * 224);   // the concatenations' gradients of all five levels, back to back: 128 + 64 + 16 + 8 + 2 per level-0 pixel
      n->gpool = take(px * 128 / 4);
    };
    if (int rc = carve_into(n->ws, layout)) return rc;
    n->cap_px = px;
  }
  bool moved = false;
  const int rc = n->ones.ensure(st, B, 512, &moved);
  if (moved) n->epoch++;
  return rc;
}

// y slice = act(conv3x3(x) + bias): x = all Cip channels of a buffer with xps channels per pixel, y = Cop channels at offset ycoff of
// a buffer with yps per pixel.  transposed: the input-gradient convolution of the same layer (Cop -> Cip, no bias, no activation)
int run_conv(maua_secondary* n, const PlainConv& c, bool transposed, const void* x, int xps, void* y, int yps, int ycoff, int B, int h, int w,
             bool relu) {
  ConvArgs a{};
  const int Ci = transposed ? c.Cop : c.Cip, Co = transposed ? c.Cip : c.Cop;
  a.x = x; a.x_bstride = (long)h * w * xps; a.x_pstride = xps; a.w = transposed ? c.wt_t.get() : c.wt.get(); a.s = n->ones.p(); a.d = nullptr;
  a.noise = nullptr; a.bias = (transposed ? c.zero_bias : c.bias).as<float>(); a.y = y; a.y_pstride = yps; a.y_coff = ycoff; a.y_bstride = (long)h * w * yps;
  a.B = B; a.H = h; a.W = w; a.Ci = Ci; a.Co = Co; a.up = 1;
  a.act = relu ? MAUA_ACT_LRELU : MAUA_ACT_LINEAR; a.alpha = relu ? 0.f : 1.f; a.gain = 1.f; a.clamp = -1.f;
  return launch_modconv3x3(n->ctx->stream, n->conv_dtype, a);
}

#define SEC_LAUNCH(KERNEL, TOTAL, ...)                                                                         \
  do {                                                                                                         \
    const long total_ = (TOTAL);                                                                               \
    if (total_ > 0) hipLaunchKernelGGL(KERNEL, dim3((unsigned)((total_ + 255) / 256)), dim3(256), 0, st, __VA_ARGS__); \
    MAUA_HIP_CHECK(hipGetLastError());                                                                         \
  } while (0)

// one launcher per glue kernel: the network (forward_t, vjp_t) and the operator-level entry points at the end of this file run through these
template <typename T>
int launch_sec_input(hipStream_t st, const float* x, const float* t, const float* wemb, int B, long HW, T* out) {
  SEC_LAUNCH(sec_input_kernel<T>, (long)B * HW, x, t, wemb, out, B, HW);
  return MAUA_OK;
}
template <typename T>
int launch_sec_output(hipStream_t st, const T* vn, const float* x, const float* t, int B, long HW, float* v, float* pred, float* eps) {
  SEC_LAUNCH(sec_output_kernel<T>, (long)B * HW, vn, x, t, v, pred, eps, B, HW);
  return MAUA_OK;
}
template <typename T>
int launch_avgpool2(hipStream_t st, const T* src, int sps, int B, int H, int W, int C, T* dst) {
  constexpr int E = 16 / (int)sizeof(T);
  SEC_LAUNCH(avgpool2_kernel<T>, (long)B * (H / 2) * (W / 2) * (C / E), src, sps, dst, B, H, W, C);
  return MAUA_OK;
}
template <typename T>
int launch_bilinear_up2(hipStream_t st, const T* src, int B, int h, int w, int C, T* dst, int dps) {
  constexpr int E = 16 / (int)sizeof(T);
  SEC_LAUNCH(bilinear_up2_kernel<T>, (long)B * 4 * h * w * (C / E), src, dst, dps, B, h, w, C);
  return MAUA_OK;
}
template <typename T>
int launch_bilinear_up2_adjoint(hipStream_t st, const T* gout, int gps, const T* act, int B, int h, int w, int C, T* gin) {
  constexpr int E = 16 / (int)sizeof(T);
  SEC_LAUNCH(bilinear_up2_adjoint_kernel<T>, (long)B * h * w * (C / E), gout, gps, act, gin, B, h, w, C);
  return MAUA_OK;
}
template <typename T>
int launch_relu_mask(hipStream_t st, T* g, const T* act, int aps, long n_pix, int C) {
  constexpr int E = 16 / (int)sizeof(T);
  SEC_LAUNCH(relu_mask_kernel<T>, n_pix * (C / E), g, act, aps, n_pix, C);
  return MAUA_OK;
}
template <typename T>
int launch_skip_grad(hipStream_t st, const T* gcat, const T* act, int cps, const T* gpool, int B, int H, int W, int C, T* out) {
  constexpr int E = 16 / (int)sizeof(T);
  SEC_LAUNCH(skip_grad_kernel<T>, (long)B * H * W * (C / E), gcat, act, cps, gpool, out, B, H, W, C);
  return MAUA_OK;
}
template <typename T>
int launch_sec_grad_in(hipStream_t st, const float* g, int B, long HW, T* out) {
  SEC_LAUNCH(sec_grad_in_kernel<T>, (long)B * HW, g, out, B, HW);
  return MAUA_OK;
}
template <typename T>
int launch_sec_grad_out(hipStream_t st, const T* g, int B, long HW, float* out) {
  SEC_LAUNCH(sec_grad_out_kernel<T>, (long)B * HW, g, out, B, HW);
  return MAUA_OK;
}

template <typename T>
int forward_t(maua_secondary* n, const float* x, const float* t, int B, int H, int W, float* v_out, float* pred, float* eps) {
  hipStream_t st = n->ctx->stream;
  if (int rc = ensure_ws<T>(n, B, H, W)) return rc;
  const long HW = (long)H * W;
  int rc;
  if ((rc = launch_sec_input<T>(st, x, t, n->wemb.as<float>(), B, HW, (T*)n->in0))) return rc;
  // encoder: level k's skip s_k lands in the upper channel slice of cat[k]
  const void* cur = n->in0;
  int cur_ps = 32;
  for (int k = 0; k < 5; k++) {
    const int h = H >> k, w = W >> k, cm = level_ch_main(k), csk = level_ch_skip(k), cps = cm + csk;
    if ((rc = run_conv(n, n->conv[2 * k], false, cur, cur_ps, n->a[k], CS[k], 0, B, h, w, true))) return rc;
    if ((rc = run_conv(n, n->conv[2 * k + 1], false, n->a[k], CS[k], n->cat[k], cps, cm, B, h, w, true))) return rc;
    if ((rc = launch_avgpool2<T>(st, (const T*)n->cat[k] + cm, cps, B, h, w, csk, (T*)n->pool[k]))) return rc;
    cur = n->pool[k];
    cur_ps = csk;
  }
  // bottleneck at level 5: c10 .. c13
  {
    const int h = H >> 5, w = W >> 5;
    const int bc[4] = {CS[5], CS[5], CS[5], CS[4]};
    for (int i = 0; i < 4; i++) {
      if ((rc = run_conv(n, n->conv[10 + i], false, cur, cur_ps, n->bott[i], bc[i], 0, B, h, w, true))) return rc;
      cur = n->bott[i];
      cur_ps = bc[i];
    }
  }
  // decoder: up into the lower slice of cat[k], two convolutions, k = 4 .. 1; then level 0
  for (int k = 4; k >= 0; k--) {
    const int h = H >> k, w = W >> k, cm = level_ch_main(k), cps = cm + level_ch_skip(k);
    if ((rc = launch_bilinear_up2<T>(st, (const T*)cur, B, h / 2, w / 2, cm, (T*)n->cat[k], cps))) return rc;
    if (k > 0) {
      const int i0 = 14 + 2 * (4 - k);
      const int c_mid = n->conv[i0].Cop, c_out = n->conv[i0 + 1].Cop;
      if ((rc = run_conv(n, n->conv[i0], false, n->cat[k], cps, n->dec[2 * (4 - k)], c_mid, 0, B, h, w, true))) return rc;
      if ((rc = run_conv(n, n->conv[i0 + 1], false, n->dec[2 * (4 - k)], c_mid, n->dec[2 * (4 - k) + 1], c_out, 0, B, h, w, true))) return rc;
      cur = n->dec[2 * (4 - k) + 1];
    } else {
      if ((rc = run_conv(n, n->conv[22], false, n->cat[0], cps, n->dec[8], CS[0], 0, B, h, w, true))) return rc;
      if ((rc = run_conv(n, n->conv[23], false, n->dec[8], CS[0], n->vbuf, 32, 0, B, h, w, false))) return rc;
    }
  }
  if ((rc = launch_sec_output<T>(st, (const T*)n->vbuf, x, t, B, HW, v_out, pred, eps))) return rc;
  n->B = B; n->H = H; n->W = W;
  return MAUA_OK;
}

template <typename T>
int vjp_t(maua_secondary* n, const float* g_v, float* g_x) {
  hipStream_t st = n->ctx->stream;
  const int B = n->B, H = n->H, W = n->W;
  const long HW = (long)H * W;
  int rc;
  T *ga = (T*)n->ga, *gb = (T*)n->gb, *gcat = (T*)n->gcat, *gpool = (T*)n->gpool;
  // v = c23(d22): no ReLU on v
  if ((rc = launch_sec_grad_in<T>(st, g_v, B, HW, ga))) return rc;
  if ((rc = run_conv(n, n->conv[23], true, ga, 32, gb, CS[0], 0, B, H, W, false))) return rc;       // G(d22) before its mask
  if ((rc = launch_relu_mask<T>(st, gb, (const T*)n->dec[8], CS[0], (long)B * HW, CS[0]))) return rc;
  // decoder backwards, level 0 .. 4: G(cat[k]) = convT(first decoder conv of the level); its lower slice goes down through the
  // up-sampling's adjoint, its upper slice waits in gcat_k for the encoder's way back.  The cat gradients of all levels are kept
  // (they are needed again on the way up): level k's lives in its own buffer - reuse the forward's bott / pool scratch? no: allocate
  // from the gradient arena below.
  // (sizes: G(cat[k]) has (cm + cs) channels at level k: 128 px-channels at level 0, 64 at level 1, 16, 8, 2: all fit gcat back to back)
  T* gcat_k[5];
  {
    size_t off = 0;
    for (int k = 0; k < 5; k++) {
      gcat_k[k] = gcat + off;
      off += ((size_t)B * HW >> (2 * k)) * (level_ch_main(k) + level_ch_skip(k));
    }
  }
  T* gcur = gb;      // G(output of the second decoder conv of the level above), masked; at level 0: G(d22)
  T* gother = ga;
  for (int k = 0; k <= 4; k++) {
    const int h = H >> k, w = W >> k, cm = level_ch_main(k), cps = cm + level_ch_skip(k);
    const long lp = (long)B * h * w;
    const int i_first = k == 0 ? 22 : 14 + 2 * (4 - k);
    if (k > 0) {
      // gcur = G(second conv's output) -> through the second conv -> mask of the first conv's output
      const int c_mid = n->conv[i_first].Cop;
      if ((rc = run_conv(n, n->conv[i_first + 1], true, gcur, n->conv[i_first + 1].Cop, gother, c_mid, 0, B, h, w, false))) return rc;
      if ((rc = launch_relu_mask<T>(st, gother, (const T*)n->dec[2 * (4 - k)], c_mid, lp, c_mid))) return rc;
      std::swap(gcur, gother);
    }
    if ((rc = run_conv(n, n->conv[i_first], true, gcur, n->conv[i_first].Cop, gcat_k[k], cps, 0, B, h, w, false))) return rc;
    // lower slice -> adjoint of the up-sampling -> G(source), masked by the source's stored activation
    const void* src_act = k == 4 ? n->bott[3] : n->dec[2 * (4 - (k + 1)) + 1];
    if ((rc = launch_bilinear_up2_adjoint<T>(st, (const T*)gcat_k[k], cps, (const T*)src_act, B, h / 2, w / 2, cm, gother))) return rc;
    std::swap(gcur, gother);
  }
  // bottleneck backwards: gcur = G(c13 out), masked
  {
    const int h = H >> 5, w = W >> 5;
    const long lp = (long)B * h * w;
    for (int i = 3; i >= 1; i--) {
      const int c_prev = n->conv[10 + i].Cip;
      if ((rc = run_conv(n, n->conv[10 + i], true, gcur, n->conv[10 + i].Cop, gother, c_prev, 0, B, h, w, false))) return rc;
      if ((rc = launch_relu_mask<T>(st, gother, (const T*)n->bott[i - 1], c_prev, lp, c_prev))) return rc;
      std::swap(gcur, gother);
    }
    if ((rc = run_conv(n, n->conv[10], true, gcur, n->conv[10].Cop, gpool, CS[4], 0, B, h, w, false))) return rc;   // G(pool[4])
  }
  // encoder backwards, level 4 .. 0: G(s_k) = G(cat[k])[skip slice] + pool gradient, masked; through c(2k+1), mask, through c(2k)
  for (int k = 4; k >= 0; k--) {
    const int h = H >> k, w = W >> k, cm = level_ch_main(k), csk = level_ch_skip(k), cps = cm + csk;
    const long lp = (long)B * h * w;
    if ((rc = launch_skip_grad<T>(st, (const T*)gcat_k[k] + cm, (const T*)n->cat[k] + cm, cps, (const T*)gpool, B, h, w, csk, gcur))) return rc;
    if ((rc = run_conv(n, n->conv[2 * k + 1], true, gcur, csk, gother, CS[k], 0, B, h, w, false))) return rc;
    if ((rc = launch_relu_mask<T>(st, gother, (const T*)n->a[k], CS[k], lp, CS[k]))) return rc;
    // through the level's first conv: into the pool gradient of the level above (k > 0) or the network input (k = 0)
    const int cin = n->conv[2 * k].Cip;
    if ((rc = run_conv(n, n->conv[2 * k], true, gother, CS[k], k > 0 ? (void*)gpool : (void*)gcur, cin, 0, B, h, w, false))) return rc;
  }
  if ((rc = launch_sec_grad_out<T>(st, (const T*)gcur, B, HW, g_x))) return rc;
  return MAUA_OK;
}

}  // namespace

namespace maua {
maua_ctx* secondary_ctx(maua_secondary* n) { return n ? n->ctx : nullptr; }
void secondary_stamp(maua_secondary* n, unsigned long long* uid, unsigned long long* epoch) {
  *uid = n ? n->uid : 0;
  *epoch = n ? n->epoch : 0;
}
}

extern "C" {

int maua_secondary_create(maua_ctx* ctx, int dtype, maua_secondary** out) {
  MAUA_REQUIRE(ctx && out, "maua_secondary_create: NULL argument");
  MAUA_REQUIRE(dtype == MAUA_F32 || dtype == MAUA_BF16 || dtype == MAUA_F32_SPLIT,
               "maua_secondary_create: dtype must be MAUA_F32, MAUA_F32_SPLIT or MAUA_BF16");
  maua_secondary* n = new maua_secondary();
  static std::atomic<unsigned long long> next_uid{1};
  n->uid = next_uid.fetch_add(1);
  // MAUA_F32_SPLIT: float32 tensors everywhere (dtype below), only the convolutions' products differ (conv_dtype)
  n->ctx = ctx; n->conv_dtype = dtype; n->dtype = dtype == MAUA_F32_SPLIT ? MAUA_F32 : dtype; n->esize = elem_bytes(n->dtype);
  int ci[NCONV], co[NCONV];
  conv_plan(ci, co);
  for (int i = 0; i < NCONV; i++)
    if (n->conv[i].alloc(ci[i], co[i], (ci[i] + 31) / 32 * 32, (co[i] + 31) / 32 * 32, n->esize, true)) {
      maua_secondary_destroy(n);
      return fail("maua_secondary_create: out of device memory");
    }
  if (n->wemb.alloc(32, true)) {
    maua_secondary_destroy(n);
    return fail("maua_secondary_create: out of device memory");
  }
  *out = n;
  return MAUA_OK;
}

void maua_secondary_destroy(maua_secondary* n) {
  if (!n) return;
  hipStreamSynchronize(n->ctx->stream);
  delete n;
}

int maua_secondary_conv_shape(int index, int* ci, int* co) {
  MAUA_REQUIRE(index >= 0 && index < NCONV && ci && co, "maua_secondary_conv_shape: bad argument");
  int I[NCONV], O[NCONV];
  conv_plan(I, O);
  *ci = I[index];
  *co = O[index];
  return MAUA_OK;
}

// what: 0 = convolution weight [Co][Ci][3][3] (the transposed network's layout is derived here), 1 = bias [Co],
// 2 = timestep_embed.weight [8] (index ignored)
int maua_secondary_load(maua_secondary* n, int index, int what, const float* host, size_t count) {
  MAUA_REQUIRE(n && host, "maua_secondary_load: NULL argument");
  hipStream_t st = n->ctx->stream;
  if (what == 2) {
    MAUA_REQUIRE(count == 8, "maua_secondary_load: timestep_embed.weight has 8 values");
    MAUA_HIP_CHECK(hipMemcpy(n->wemb.get(), host, 32, hipMemcpyHostToDevice));
    return MAUA_OK;
  }
  MAUA_REQUIRE(index >= 0 && index < NCONV, "maua_secondary_load: no such convolution");
  PlainConv& c = n->conv[index];
  if (what == 1) {
    MAUA_REQUIRE(count == (size_t)c.Co, "maua_secondary_load: bias: wrong size");
    return c.load_bias(st, host);
  }
  MAUA_REQUIRE(what == 0, "maua_secondary_load: what must be 0, 1 or 2");
  MAUA_REQUIRE(count == (size_t)c.Co * c.Ci * 9, "maua_secondary_load: weight: wrong size");
  return c.load_weight(st, n->dtype, host, true, n->conv_dtype == MAUA_F32_SPLIT);
}

int maua_secondary_forward(maua_secondary* n, const float* x, const float* t, int B, int H, int W, float* v_out, float* pred_out,
                           float* eps_out) {
  MAUA_REQUIRE(n && x && t, "maua_secondary_forward: NULL argument");
  MAUA_REQUIRE(B >= 0 && H > 0 && W > 0 && H % 32 == 0 && W % 32 == 0, "maua_secondary_forward: H and W must be positive multiples of 32");
  if (B == 0) return MAUA_OK;
  return dispatch_dtype<bf16_t, float>(n->dtype, "maua_secondary_forward",
                                       [&](auto e) { return forward_t<decltype(e)>(n, x, t, B, H, W, v_out, pred_out, eps_out); });
}

int maua_secondary_vjp(maua_secondary* n, const float* g_v, int B, int H, int W, float* g_x) {
  MAUA_REQUIRE(n && g_v && g_x, "maua_secondary_vjp: NULL argument");
  MAUA_REQUIRE(n->B > 0 && B == n->B && H == n->H && W == n->W, "maua_secondary_vjp: call maua_secondary_forward with the same shape first");
  return dispatch_dtype<bf16_t, float>(n->dtype, "maua_secondary_vjp", [&](auto e) { return vjp_t<decltype(e)>(n, g_v, g_x); });
}

// ---- the glue kernels above as operators (include/maua_hip.h): each runs the network's own launcher
namespace {
// what every NHWC form checks in front of its launch: the dtype, the sizes' signs, whole 16-byte pieces per pixel, pixel strides
int glue_check(const char* who, int dtype, int B, int H, int W, int C, long stride0, long stride1, bool even) {
  const std::string w(who);
  if (dtype != MAUA_F32 && dtype != MAUA_BF16) return fail(w + ": dtype must be MAUA_F32 or MAUA_BF16");
  if (B < 0 || H < 0 || W < 0 || C < 0) return fail(w + ": a negative size");
  if (C % elems_per_piece(dtype)) return fail(w + ": C must be whole 16-byte pieces");
  if (even && ((H | W) & 1)) return fail(w + ": H and W must be even");
  if (stride0 < C || stride1 < C) return fail(w + ": a pixel stride below C");
  if (stride0 > 0x7fffffffL || stride1 > 0x7fffffffL) return fail(w + ": a pixel stride beyond int");
  return MAUA_OK;
}
}  // namespace

int maua_secondary_input(maua_ctx* ctx, const float* x, const float* t, const float* wemb, int B, long HW, int dtype, void* out) {
  MAUA_REQUIRE(ctx, "maua_secondary_input: ctx is NULL");
  MAUA_REQUIRE(dtype == MAUA_F32 || dtype == MAUA_BF16, "maua_secondary_input: dtype must be MAUA_F32 or MAUA_BF16");
  MAUA_REQUIRE(B >= 0 && HW >= 0, "maua_secondary_input: a negative size");
  if (B == 0 || HW == 0) return MAUA_OK;
  MAUA_REQUIRE(x && t && wemb && out, "maua_secondary_input: NULL argument");
  return dispatch_dtype<bf16_t, float>(dtype, "maua_secondary_input",
                                       [&](auto e) { return launch_sec_input<decltype(e)>(ctx->stream, x, t, wemb, B, HW, (decltype(e)*)out); });
}

int maua_secondary_output(maua_ctx* ctx, const void* vn, const float* x, const float* t, int B, long HW, int dtype, float* v, float* pred,
                          float* eps) {
  MAUA_REQUIRE(ctx, "maua_secondary_output: ctx is NULL");
  MAUA_REQUIRE(dtype == MAUA_F32 || dtype == MAUA_BF16, "maua_secondary_output: dtype must be MAUA_F32 or MAUA_BF16");
  MAUA_REQUIRE(B >= 0 && HW >= 0, "maua_secondary_output: a negative size");
  if (B == 0 || HW == 0) return MAUA_OK;
  MAUA_REQUIRE(vn && x && t, "maua_secondary_output: NULL argument");
  return dispatch_dtype<bf16_t, float>(dtype, "maua_secondary_output", [&](auto e) {
    return launch_sec_output<decltype(e)>(ctx->stream, (const decltype(e)*)vn, x, t, B, HW, v, pred, eps);
  });
}

int maua_avgpool2_nhwc(maua_ctx* ctx, const void* src, long src_stride, int B, int H, int W, int C, int dtype, void* dst) {
  MAUA_REQUIRE(ctx, "maua_avgpool2_nhwc: ctx is NULL");
  if (int rc = glue_check("maua_avgpool2_nhwc", dtype, B, H, W, C, src_stride, C, true)) return rc;
  if (B == 0 || H == 0 || W == 0 || C == 0) return MAUA_OK;
  MAUA_REQUIRE(src && dst, "maua_avgpool2_nhwc: NULL argument");
  return dispatch_dtype<bf16_t, float>(dtype, "maua_avgpool2_nhwc", [&](auto e) {
    return launch_avgpool2<decltype(e)>(ctx->stream, (const decltype(e)*)src, (int)src_stride, B, H, W, C, (decltype(e)*)dst);
  });
}

int maua_bilinear_up2_nhwc(maua_ctx* ctx, const void* src, int B, int h, int w, int C, int dtype, void* dst, long dst_stride) {
  MAUA_REQUIRE(ctx, "maua_bilinear_up2_nhwc: ctx is NULL");
  if (int rc = glue_check("maua_bilinear_up2_nhwc", dtype, B, h, w, C, dst_stride, C, false)) return rc;
  if (B == 0 || h == 0 || w == 0 || C == 0) return MAUA_OK;
  MAUA_REQUIRE(src && dst, "maua_bilinear_up2_nhwc: NULL argument");
  return dispatch_dtype<bf16_t, float>(dtype, "maua_bilinear_up2_nhwc", [&](auto e) {
    return launch_bilinear_up2<decltype(e)>(ctx->stream, (const decltype(e)*)src, B, h, w, C, (decltype(e)*)dst, (int)dst_stride);
  });
}

int maua_bilinear_up2_nhwc_vjp(maua_ctx* ctx, const void* gout, long g_stride, const void* act, int B, int h, int w, int C, int dtype,
                               void* gin) {
  MAUA_REQUIRE(ctx, "maua_bilinear_up2_nhwc_vjp: ctx is NULL");
  if (int rc = glue_check("maua_bilinear_up2_nhwc_vjp", dtype, B, h, w, C, g_stride, C, false)) return rc;
  if (B == 0 || h == 0 || w == 0 || C == 0) return MAUA_OK;
  MAUA_REQUIRE(gout && gin, "maua_bilinear_up2_nhwc_vjp: NULL argument");
  return dispatch_dtype<bf16_t, float>(dtype, "maua_bilinear_up2_nhwc_vjp", [&](auto e) {
    return launch_bilinear_up2_adjoint<decltype(e)>(ctx->stream, (const decltype(e)*)gout, (int)g_stride, (const decltype(e)*)act, B, h, w, C,
                                                    (decltype(e)*)gin);
  });
}

int maua_relu_mask_nhwc(maua_ctx* ctx, void* g, const void* act, long act_stride, long n_pix, int C, int dtype) {
  MAUA_REQUIRE(ctx, "maua_relu_mask_nhwc: ctx is NULL");
  MAUA_REQUIRE(n_pix >= 0, "maua_relu_mask_nhwc: a negative size");
  if (int rc = glue_check("maua_relu_mask_nhwc", dtype, 0, 0, 0, C, act_stride, C, false)) return rc;
  if (n_pix == 0 || C == 0) return MAUA_OK;
  MAUA_REQUIRE(g && act, "maua_relu_mask_nhwc: NULL argument");
  return dispatch_dtype<bf16_t, float>(dtype, "maua_relu_mask_nhwc", [&](auto e) {
    return launch_relu_mask<decltype(e)>(ctx->stream, (decltype(e)*)g, (const decltype(e)*)act, (int)act_stride, n_pix, C);
  });
}

int maua_skip_grad_nhwc(maua_ctx* ctx, const void* gcat, const void* act, long cat_stride, const void* gpool, int B, int H, int W, int C,
                        int dtype, void* out) {
  MAUA_REQUIRE(ctx, "maua_skip_grad_nhwc: ctx is NULL");
  if (int rc = glue_check("maua_skip_grad_nhwc", dtype, B, H, W, C, cat_stride, C, true)) return rc;
  if (B == 0 || H == 0 || W == 0 || C == 0) return MAUA_OK;
  MAUA_REQUIRE(gcat && act && gpool && out, "maua_skip_grad_nhwc: NULL argument");
  return dispatch_dtype<bf16_t, float>(dtype, "maua_skip_grad_nhwc", [&](auto e) {
    return launch_skip_grad<decltype(e)>(ctx->stream, (const decltype(e)*)gcat, (const decltype(e)*)act, (int)cat_stride,
                                         (const decltype(e)*)gpool, B, H, W, C, (decltype(e)*)out);
  });
}

int maua_secondary_grad_layout(maua_ctx* ctx, const void* src, int B, long HW, int dtype, int to_nhwc, void* dst) {
  MAUA_REQUIRE(ctx, "maua_secondary_grad_layout: ctx is NULL");
  MAUA_REQUIRE(dtype == MAUA_F32 || dtype == MAUA_BF16, "maua_secondary_grad_layout: dtype must be MAUA_F32 or MAUA_BF16");
  MAUA_REQUIRE(B >= 0 && HW >= 0, "maua_secondary_grad_layout: a negative size");
  MAUA_REQUIRE(to_nhwc == 0 || to_nhwc == 1, "maua_secondary_grad_layout: to_nhwc is 0 or 1");
  if (B == 0 || HW == 0) return MAUA_OK;
  MAUA_REQUIRE(src && dst, "maua_secondary_grad_layout: NULL argument");
  return dispatch_dtype<bf16_t, float>(dtype, "maua_secondary_grad_layout", [&](auto e) {
    using T = decltype(e);
    return to_nhwc ? launch_sec_grad_in<T>(ctx->stream, (const float*)src, B, HW, (T*)dst)
                   : launch_sec_grad_out<T>(ctx->stream, (const T*)src, B, HW, (float*)dst);
  });
}

}  // extern "C"
