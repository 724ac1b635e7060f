// The neural cellular automaton's step (maua/nca/train.py:152-193): one launch per update,
//     x += w2 . relu(w1 . perception(x) + b1) . floor(u + rate)
// with the state [B][chn][H][W] f32 in memory and nothing in between leaving the workgroup.
//
// A workgroup (4 waves) owns a 4 x 32 pixel tile.  It stages the tile with a one-pixel circular halo (wrapped when it is staged, so a
// grid smaller than the tile wraps onto itself) and the parameters in LDS.  A wave then takes one 32-pixel row segment at a time:
//   1. its lanes evaluate the four stencils of their channels from LDS straight into the operand fragment (lane = pixel, lane half =
//      which channels of the k-step: no perception tile is ever written);
//   2. H^T [hidden][pixel] = w1 P^T + b1: the WEIGHTS are the M side and the pixels the N side, so the accumulator has the pixel on the
//      lane and the hidden units in its registers, the accumulator starts from the bias;
//   3. Y^T [chn -> 32][pixel] = w2 relu(H^T) sums over the first product's ROW index, so relu(H^T)'s registers are the B operand as they
//      are: no LDS round trip between the products.  chn is padded to the instruction's 32 rows here (a quarter of the work);
//   4. rows c < chn of Y^T: x_new = x_old + y * mask, stored along the row (lane = consecutive x).
// MAUA_F32: Mma<float> (v_mfma_f32_32x32x2_f32), an f32 fma chain per output whose k order within an 8-group is {4 h + e} as mma.h states.
// MAUA_F32_SPLIT: every operand as hi + lo bf16 (mma.h), three v_mfma_f32_32x32x16_bf16 per 16 k; the weights are split when staged, the
// perception and relu(H^T) in registers.
// Several steps per launch (K = 2, 4; temporal blocking): the tile is staged with a K-pixel halo and advanced K times inside LDS, the updated
// region shrinking by one ring per sub-step; the halo pixels a neighbouring workgroup computes too get the same mask (it is addressed
// by step and pixel), so the result has K = 1's bits.  Not in window mode, whose margin columns are not updated between steps.
// The kernel is instantiated for (chn, hidden) <= (12, 96), the reference's sizes, and <= (16, 128); smaller sizes run the next
// instantiation on zero-padded parameters (the added products are exact zeros).
#include "nca_internal.h"

namespace maua {

namespace {

struct StepArgs {
  const float* src; float* dst;
  const float *w1, *b1, *w2;
  int chn, hidden, B, H, Wt, ld, col0, wlo, whi;
  float rate; const float* rate_map; const float* u;
  uint32_t s0, s1, t0, t1;
  unsigned long long t;
};

// K steps per launch: the tile is staged with a K-pixel halo, RH x RW positions, and for K > 1 in two copies that the sub-steps alternate
// between (a neighbour reads the old state)
template <int K>
struct Halo {
  static constexpr int RH = TH + 2 * K, RW = TW + 2 * K, LD = RW + 2, NBUF = K > 1 ? 2 : 1;
};
template <typename T, int CQ, int NB, int K>
struct Smem;
template <int CQ, int NB, int K>
struct Smem<float, CQ, NB, K> {
  static constexpr int K1 = 16 * CQ, NH = 32 * NB, L1 = K1 + 4, L2 = NH + 4;
  float xs[Halo<K>::NBUF][4 * CQ][Halo<K>::RH][Halo<K>::LD];
  float b1[NH];
  float w1[NH][L1];
  float w2[16][L2];
};
template <int CQ, int NB, int K>
struct Smem<f32s_t, CQ, NB, K> {
  static constexpr int K1 = 16 * CQ, NH = 32 * NB, L1 = K1 + 8, L2 = NH + 8;
  float xs[Halo<K>::NBUF][4 * CQ][Halo<K>::RH][Halo<K>::LD];
  float b1[NH];
  uint16_t w1h[NH][L1], w1l[NH][L1];
  uint16_t w2h[16][L2], w2l[16][L2];   // column 32 nb + 16 s + 8 h + j holds hidden unit 32 nb + 16 s + 8 (j >> 2) + 4 h + (j & 3)
};

__device__ __forceinline__ void split1(float v, uint16_t& hi, uint16_t& lo) {
  hi = f2bf(v);
  lo = f2bf(v - bf2f(hi));
}

template <typename T, int CQ, int NB, int K>
__global__ __launch_bounds__(256) void nca_step_kernel(const StepArgs a) {
  using S = Smem<T, CQ, NB, K>;
  constexpr int RH = Halo<K>::RH, RW = Halo<K>::RW, LD = Halo<K>::LD;
  constexpr bool kSplit = IsSplit<T>::value;
  __shared__ __attribute__((aligned(16))) S sm;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
  const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH, b = blockIdx.z;
  const long plane = (long)a.H * a.ld;

  // ---- stage the tile + halo (circular: the wrapped row and column of every halo position first, one division each) and the
  // parameters (zero-padded to the instantiation's sizes)
  __shared__ int xi[RW], yi[RH];
  if (tid < RW) xi[tid] = wrap(x0 + tid - K, a.Wt);
  else if (tid < RW + RH) yi[tid - RW] = wrap(y0 + tid - RW - K, a.H);
  __syncthreads();
  for (int i = tid; i < 4 * CQ * RH * RW; i += 256) {
    const int c = i / (RH * RW), rem = i - c * (RH * RW), yy = rem / RW, xx = rem - yy * RW;
    float v = 0.f;
    if (c < a.chn) v = a.src[((long)b * a.chn + c) * plane + (long)yi[yy] * a.ld + a.col0 + xi[xx]];
    sm.xs[0][c][yy][xx] = v;
  }
  for (int i = tid; i < S::NH; i += 256) sm.b1[i] = i < a.hidden ? a.b1[i] : 0.f;
  for (int i = tid; i < S::NH * S::K1; i += 256) {
    const int n = i / S::K1, k = i - n * S::K1;
    const float v = (n < a.hidden && k < 4 * a.chn) ? a.w1[n * 4 * a.chn + k] : 0.f;
    if constexpr (kSplit) split1(v, sm.w1h[n][k], sm.w1l[n][k]);
    else sm.w1[n][k] = v;
  }
  for (int i = tid; i < 16 * S::NH; i += 256) {
    const int c = i / S::NH, n = i - c * S::NH;
    const float v = (c < a.chn && n < a.hidden) ? a.w2[c * a.hidden + n] : 0.f;
    if constexpr (kSplit) {
      const int w = n & 15, col = (n & ~15) + 8 * ((w >> 2) & 1) + 4 * (w >> 3) + (w & 3);   // unit 8 q + 4 h + e of a 16-group -> column 8 h + 4 q + e
      split1(v, sm.w2h[c][col], sm.w2l[c][col]);
    } else {
      sm.w2[c][n] = v;
    }
  }
  __syncthreads();

  // sub-step s updates the tile grown by e = K - 1 - s rings (what the later sub-steps' stencils reach), as 32-pixel row segments dealt
  // to the waves in turn; position (row, col) of the tile is xs[.][.][K + row][K + col], the state of pixel (yi, xi) of the grid, so a
  // position that wraps onto another one holds the same value as that one at every sub-step: the mask is addressed by the grid's pixel
#pragma unroll 1
  for (int sub = 0; sub < K; sub++) {
  const int e = K - 1 - sub, nseg = (TW + 2 * e + 31) / 32, cur = sub & (Halo<K>::NBUF - 1);
  const bool last = sub == K - 1;
  for (int it = wave; it < (TH + 2 * e) * nseg; it += 4) {
    const int seg = it % nseg, ly = it / nseg - e, col = 32 * seg - e + r;
    const bool active = col < TW + e;
    const int lc = active ? col : TW + e - 1;       // (an idle lane recomputes the segment's last pixel)
    const int gy = y0 + ly, gx = x0 + lc;
    f32x16 acc[NB];
#pragma unroll
    for (int nb = 0; nb < NB; nb++)
#pragma unroll
      for (int g = 0; g < 16; g++) acc[nb][g] = sm.b1[32 * nb + (g & 3) + 8 * (g >> 2) + 4 * h];

    if constexpr (!kSplit) {
      // k = 8 j + 4 h + e: filter e of channel 2 j + h
#pragma unroll
      for (int j = 0; j < 2 * CQ; j++) {
        const u32x4 p = __builtin_bit_cast(u32x4, stencils_ld<LD>(&sm.xs[cur][2 * j + h][K + ly - 1][K + lc - 1]));
#pragma unroll
        for (int nb = 0; nb < NB; nb++)
          Mma<float>::step(acc[nb], *reinterpret_cast<const u32x4*>(&sm.w1[32 * nb + r][8 * j + 4 * h]), p);
      }
    } else {
      // k = 16 s + 8 h + j: filters of channels 4 s + 2 h, 4 s + 2 h + 1
#pragma unroll
      for (int s = 0; s < CQ; s++) {
        const u32x4 p0 = f32_split4(stencils_ld<LD>(&sm.xs[cur][4 * s + 2 * h][K + ly - 1][K + lc - 1])), p1 = f32_split4(stencils_ld<LD>(&sm.xs[cur][4 * s + 2 * h + 1][K + ly - 1][K + lc - 1]));
        const u32x4 ph = {p0[0], p0[1], p1[0], p1[1]}, pl = {p0[2], p0[3], p1[2], p1[3]};
#pragma unroll
        for (int nb = 0; nb < NB; nb++) {
          const u32x4 wh = *reinterpret_cast<const u32x4*>(&sm.w1h[32 * nb + r][16 * s + 8 * h]);
          const u32x4 wl = *reinterpret_cast<const u32x4*>(&sm.w1l[32 * nb + r][16 * s + 8 * h]);
          Mma<f32s_t>::step(acc[nb], wh, ph);
          Mma<f32s_t>::step(acc[nb], wh, pl);
          Mma<f32s_t>::step(acc[nb], wl, ph);
        }
      }
    }

    f32x16 y;
#pragma unroll
    for (int g = 0; g < 16; g++) y[g] = 0.f;
    const int rc = r & 15;                 // rows 16 .. 31 of the padded w2 are zero
    const bool real = r < 16;
#pragma unroll
    for (int nb = 0; nb < NB; nb++) {
#pragma unroll
      for (int g = 0; g < 16; g++) acc[nb][g] = fmaxf(acc[nb][g], 0.f);
      if constexpr (!kSplit) {
#pragma unroll
        for (int q = 0; q < 4; q++) {
          u32x4 w = *reinterpret_cast<const u32x4*>(&sm.w2[rc][32 * nb + 8 * q + 4 * h]);
          if (!real) w = u32x4{0u, 0u, 0u, 0u};
          const f32x4 hv = {acc[nb][4 * q], acc[nb][4 * q + 1], acc[nb][4 * q + 2], acc[nb][4 * q + 3]};
          Mma<float>::step(y, w, __builtin_bit_cast(u32x4, hv));
        }
      } else {
#pragma unroll
        for (int s = 0; s < 2; s++) {
          const f32x4 v0 = {acc[nb][8 * s], acc[nb][8 * s + 1], acc[nb][8 * s + 2], acc[nb][8 * s + 3]};
          const f32x4 v1 = {acc[nb][8 * s + 4], acc[nb][8 * s + 5], acc[nb][8 * s + 6], acc[nb][8 * s + 7]};
          const u32x4 q0 = f32_split4(v0), q1 = f32_split4(v1);
          const u32x4 hh = {q0[0], q0[1], q1[0], q1[1]}, hl = {q0[2], q0[3], q1[2], q1[3]};
          u32x4 wh = *reinterpret_cast<const u32x4*>(&sm.w2h[rc][32 * nb + 16 * s + 8 * h]);
          u32x4 wl = *reinterpret_cast<const u32x4*>(&sm.w2l[rc][32 * nb + 16 * s + 8 * h]);
          if (!real) { wh = u32x4{0u, 0u, 0u, 0u}; wl = wh; }
          Mma<f32s_t>::step(y, wh, hh);
          Mma<f32s_t>::step(y, wh, hl);
          Mma<f32s_t>::step(y, wl, hh);
        }
      }
    }

    // ---- mask and residual: register g < 8 is channel (g & 3) + 8 (g >> 2) + 4 h of pixel r
    const long pix = (long)yi[K + ly] * a.ld + a.col0 + xi[K + lc];
    const float* us = a.u ? a.u + (long)sub * a.B * plane : nullptr;
    if (last) {
      if (active && gy < a.H && gx >= a.wlo && gx < a.whi) {
        const float mask = nca_mask(us, a.rate_map, a.rate, a.t + sub, a.B, b, plane, pix, a.s0, a.s1, a.t0, a.t1);
#pragma unroll
        for (int g = 0; g < 8; g++) {
          const int c = (g & 3) + 8 * (g >> 2) + 4 * h;
          if (c < a.chn) a.dst[((long)b * a.chn + c) * plane + pix] = sm.xs[cur][c][K + ly][K + lc] + y[g] * mask;
        }
      }
    } else if (active) {
      const float mask = nca_mask(us, a.rate_map, a.rate, a.t + sub, a.B, b, plane, pix, a.s0, a.s1, a.t0, a.t1);
#pragma unroll
      for (int g = 0; g < 8; g++) {
        const int c = (g & 3) + 8 * (g >> 2) + 4 * h;       // (a padded channel: 0 + 0 * mask)
        if (c < 4 * CQ) sm.xs[cur ^ (Halo<K>::NBUF - 1)][c][K + ly][K + lc] = sm.xs[cur][c][K + ly][K + lc] + y[g] * mask;
      }
    }
  }
  if (!last) __syncthreads();
  }
}

// perception as an operator of its own (train.py:167-169): out [B][4 C][H][W], feature 4 c + f; the step kernel never calls this
__global__ __launch_bounds__(256) void nca_perception_kernel(const float* __restrict__ x, float* __restrict__ out, long BC, int H, int W) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const long plane = (long)H * W;
  if (i >= BC * plane) return;
  const long bc = i / plane;
  const int rem = (int)(i - bc * plane), y = rem / W, xx = rem - y * W;
  const int ym = y == 0 ? H - 1 : y - 1, yp = y == H - 1 ? 0 : y + 1, xm = xx == 0 ? W - 1 : xx - 1, xp = xx == W - 1 ? 0 : xx + 1;
  const float* p = x + bc * plane;
  const float a = p[(long)ym * W + xm], b = p[(long)ym * W + xx], c = p[(long)ym * W + xp], d = p[(long)y * W + xm], e = p[(long)y * W + xx],
              f = p[(long)y * W + xp], g = p[(long)yp * W + xm], h = p[(long)yp * W + xx], k = p[(long)yp * W + xp];
  float* o = out + bc * 4 * plane + rem;
  o[0] = e;
  o[plane] = ((c - a) + 2.f * (f - d)) + (k - g);
  o[2 * plane] = ((g - a) + 2.f * (h - b)) + (k - c);
  o[3 * plane] = (((a + c) + (g + k)) + 2.f * ((b + h) + (d + f))) - 12.f * e;
}

// window mode: the columns a step wrote, from the handle's buffer back into the state
__global__ __launch_bounds__(256) void nca_copy_cols_kernel(const float* __restrict__ src, float* __restrict__ dst, long rows, int ld, int c0,
                                                            int n) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * n) return;
  const long row = i / n;
  const long o = row * ld + c0 + (i - row * n);
  dst[o] = src[o];
}

template <typename T, int K>
void launch_step_k(hipStream_t stream, const StepArgs& a) {
  const dim3 grid(cdiv(a.Wt, TW), cdiv(a.H, TH), a.B);
  if (a.chn <= 12 && a.hidden <= 96) hipLaunchKernelGGL((nca_step_kernel<T, 3, 3, K>), grid, dim3(256), 0, stream, a);
  else hipLaunchKernelGGL((nca_step_kernel<T, 4, 4, K>), grid, dim3(256), 0, stream, a);
}

template <typename T>
void launch_step(hipStream_t stream, const StepArgs& a, int k) {
  if (k == 4) launch_step_k<T, 4>(stream, a);
  else if (k == 2) launch_step_k<T, 2>(stream, a);
  else launch_step_k<T, 1>(stream, a);
}

}  // namespace

}  // namespace maua

using namespace maua;


namespace {

int check_desc(const char* who, int chn, int hidden, int dtype, const maua_nca_desc* d, bool keep) {
  const std::string p = std::string(who) + ": ";
  MAUA_REQUIRE(nca_sizes_ok(chn, hidden), p + "chn must be a multiple of 4 up to 16 and hidden a multiple of 32 up to 128");
  MAUA_REQUIRE(dtype == MAUA_F32 || dtype == MAUA_F32_SPLIT, p + "dtype must be MAUA_F32 or MAUA_F32_SPLIT (it selects the products; the state is float32)");
  MAUA_REQUIRE(d, p + "desc is NULL");
  MAUA_REQUIRE(d->x && d->w1 && d->b1 && d->w2, p + "x, w1, b1 and w2 must not be NULL");
  MAUA_REQUIRE(d->B >= 1 && d->B <= 65535, p + "B must be in 1 .. 65535");
  MAUA_REQUIRE(d->H >= 3 && d->W >= 3, p + "H and W must be at least 3");
  MAUA_REQUIRE(d->H <= 65535 * TH, p + "H too large");
  MAUA_REQUIRE(d->n_steps >= 0, p + "n_steps is negative");
  MAUA_REQUIRE(d->steps_per_launch == 0 || d->steps_per_launch == 1 || d->steps_per_launch == 2 || d->steps_per_launch == 4,
               p + "steps_per_launch must be 1, 2 or 4");
  MAUA_REQUIRE(d->steps_per_launch <= 1 || (!keep && d->W_sub == 0),
               p + "steps_per_launch above 1 neither keeps the states between its steps nor runs in window mode");
  MAUA_REQUIRE((long)d->B * chn * d->H * d->W < (1l << 40), p + "state too large");
  if (d->W_sub != 0) {
    MAUA_REQUIRE(!keep, p + "no window mode");
    MAUA_REQUIRE(d->W_sub >= 3 && d->col0 >= 0 && d->col0 + (long)d->W_sub <= d->W, p + "the window must lie inside the row and be at least 3 wide");
    MAUA_REQUIRE(d->margin >= 0 && 2 * d->margin < d->W_sub, p + "margin must leave a column to write");
  } else {
    MAUA_REQUIRE(d->col0 == 0 && d->margin == 0, p + "col0 and margin need W_sub");
  }
  return MAUA_OK;
}

StepArgs make_args(const maua_nca* h, const maua_nca_desc* d) {
  StepArgs a{};
  a.w1 = d->w1; a.b1 = d->b1; a.w2 = d->w2;
  a.chn = h->chn; a.hidden = h->hidden; a.B = d->B; a.H = d->H; a.ld = d->W;
  a.Wt = d->W_sub ? d->W_sub : d->W; a.col0 = d->col0; a.wlo = d->margin; a.whi = a.Wt - d->margin;
  a.rate = d->rate; a.rate_map = d->rate_map;
  a.s0 = (uint32_t)d->seed; a.s1 = (uint32_t)(d->seed >> 32); a.t0 = (uint32_t)d->stream; a.t1 = (uint32_t)(d->stream >> 32);
  return a;
}

void launch(const maua_nca* h, const StepArgs& a, int k = 1) {
  dispatch_dtype<float, f32s_t>(h->dtype, "maua_nca", [&](auto t) { launch_step<decltype(t)>(h->ctx->stream, a, k); });
}

}  // namespace

extern "C" {

int maua_nca_create(maua_ctx* ctx, int chn, int hidden, int dtype, maua_nca** out) {
  MAUA_REQUIRE(ctx && out, "maua_nca_create: ctx or out is NULL");
  MAUA_REQUIRE(nca_sizes_ok(chn, hidden), "maua_nca_create: chn must be a multiple of 4 up to 16 and hidden a multiple of 32 up to 128");
  MAUA_REQUIRE(dtype == MAUA_F32 || dtype == MAUA_F32_SPLIT,
               "maua_nca_create: dtype must be MAUA_F32 or MAUA_F32_SPLIT (it selects the products; the state is float32)");
  maua_nca* h = new maua_nca();
  h->ctx = ctx; h->chn = chn; h->hidden = hidden; h->dtype = dtype;
  *out = h;
  return MAUA_OK;
}

int maua_nca_destroy(maua_nca* h) {
  if (!h) return MAUA_OK;
  if (h->tmp) hipStreamSynchronize(h->ctx->stream);
  delete h;
  return MAUA_OK;
}

int maua_nca_perception(maua_ctx* ctx, const float* x, int B, int C, int H, int W, float* out) {
  MAUA_REQUIRE(ctx && x && out, "maua_nca_perception: a pointer is NULL");
  MAUA_REQUIRE(B >= 1 && C >= 1 && H >= 3 && W >= 3, "maua_nca_perception: B and C must be positive, H and W at least 3");
  const long n = (long)B * C * H * W;
  MAUA_REQUIRE(n < (1l << 38), "maua_nca_perception: tensor too large");
  hipLaunchKernelGGL(nca_perception_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, x, out, (long)B * C, H, W);
  MAUA_HIP_CHECK(hipGetLastError());
  return MAUA_OK;
}

int maua_nca_check(const maua_nca* h, int chn, int hidden, int dtype, const maua_nca_desc* d) {
  if (h) { chn = h->chn; hidden = h->hidden; dtype = h->dtype; }
  return check_desc("maua_nca_step", chn, hidden, dtype, d, false);
}

int maua_nca_step(maua_nca* h, const maua_nca_desc* d) {
  MAUA_REQUIRE(h, "maua_nca_step: handle is NULL");
  if (int rc = check_desc("maua_nca_step", h->chn, h->hidden, h->dtype, d, false)) return rc;
  if (d->n_steps == 0) return MAUA_OK;
  const long plane = (long)d->H * d->W, n = (long)d->B * h->chn * plane;
  if (int rc = nca_reserve(h, (size_t)n * sizeof(float))) return rc;
  StepArgs a = make_args(h, d);
  hipStream_t st = h->ctx->stream;
  if (d->W_sub) {
    const long rows = (long)d->B * h->chn * d->H;
    const int ncols = a.whi - a.wlo;
    for (int s = 0; s < d->n_steps; s++) {
      a.src = d->x; a.dst = h->tmp.as<float>(); a.t = d->step0 + (unsigned long long)s;
      a.u = d->u ? d->u + (long)s * d->B * plane : nullptr;
      launch(h, a);
      hipLaunchKernelGGL(nca_copy_cols_kernel, dim3((unsigned)((rows * ncols + 255) / 256)), dim3(256), 0, st, h->tmp.as<float>(), d->x, rows, d->W,
                         d->col0 + a.wlo, ncols);
    }
  } else {
    // launches of k steps, the remainder as launches of 2 and 1; an odd number of launches starts from a copy in the buffer, so that
    // the last one writes x
    const int k = d->steps_per_launch > 1 ? d->steps_per_launch : 1;
    auto width = [&](int left) { return left >= k ? k : left >= 2 && k >= 2 ? 2 : 1; };
    int launches = 0;
    for (int s = 0; s < d->n_steps; s += width(d->n_steps - s)) launches++;
    float* cur = d->x;
    float* other = h->tmp.as<float>();
    if (launches & 1) {
      MAUA_HIP_CHECK(hipMemcpyAsync(h->tmp.as<float>(), d->x, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, st));
      cur = h->tmp.as<float>(); other = d->x;
    }
    for (int s = 0; s < d->n_steps;) {
      const int w = width(d->n_steps - s);
      a.src = cur; a.dst = other; a.t = d->step0 + (unsigned long long)s;
      a.u = d->u ? d->u + (long)s * d->B * plane : nullptr;
      launch(h, a, w);
      float* t = cur; cur = other; other = t;
      s += w;
    }
  }
  MAUA_HIP_CHECK(hipGetLastError());
  return MAUA_OK;
}

int maua_nca_forward_keep(maua_nca* h, const maua_nca_desc* d, float* states) {
  MAUA_REQUIRE(h, "maua_nca_forward_keep: handle is NULL");
  if (int rc = check_desc("maua_nca_forward_keep", h->chn, h->hidden, h->dtype, d, true)) return rc;
  MAUA_REQUIRE(states, "maua_nca_forward_keep: states is NULL");
  const long plane = (long)d->H * d->W, n = (long)d->B * h->chn * plane;
  hipStream_t st = h->ctx->stream;
  MAUA_HIP_CHECK(hipMemcpyAsync(states, d->x, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, st));
  StepArgs a = make_args(h, d);
  for (int s = 0; s < d->n_steps; s++) {
    a.src = states + (long)s * n; a.dst = states + (long)(s + 1) * n; a.t = d->step0 + (unsigned long long)s;
    a.u = d->u ? d->u + (long)s * d->B * plane : nullptr;
    launch(h, a);
  }
  MAUA_HIP_CHECK(hipGetLastError());
  return MAUA_OK;
}

}  // extern "C"
