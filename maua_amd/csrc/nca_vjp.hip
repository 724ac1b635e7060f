// The gradient of the cellular automaton's steps (nca.hip), walked backwards over the states maua_nca_forward_keep stored.  Per step, with
// g = dL/dx_{s+1}, p = perception(x_s), h = relu(w1 p + b1), gy = mask . g:
//     dW2 += gy h^T      gh = (w2^T gy) . [h > 0]      dW1 += gh p^T      db1 += sum gh      g <- g + perception^T(w1^T gh)
// Two launches per step.
//   nca_vjp_pixel_kernel: per 32-pixel row segment, everything that stays at the pixel.  The forward's two products are recomputed in the
//     forward's orientation (weights M, pixels N: hidden units in the registers, the pixel on the lane); gh^T = w2^T gy has the same
//     accumulator layout, so ReLU's mask is register against register, and gp^T = w1^T gh sums over gh^T's row index, which takes the
//     registers as they are.  The parameter gradients sum over PIXELS, the lane index of all of these, so h (then gh), p and gy go once
//     through the wave's LDS slab as [unit][pixel] and come back with the unit on the lane: dW2 = gy h^T and dW1 = gh p^T are MFMA
//     products with K = 32 pixels, accumulated in registers over the wave's segments.  A row of ones under p (row 16 CQ) makes db1 a column of dW1.
//     The workgroup's waves add their accumulators in wave order through LDS, and the sum goes to the workgroup's slot of a partials
//     buffer, added to what the steps walked before left there: every sum in a fixed order, no atomics.
//   nca_vjp_stencil_kernel: g_new = g + the circular stencils with flipped taps applied to gp (the neighbours' gp: a second launch).
// nca_vjp_reduce_kernel then adds the slots in index order and writes dW1, db1, dW2 in the parameters' layouts.
// All products are exact f32 (v_mfma_f32_32x32x2_f32) whatever the handle's dtype.
#include "nca_internal.h"

namespace maua {

namespace {

constexpr int PS = 36;   // row stride of the per-wave [unit][pixel] slabs: 32 pixels + 4 (16-byte rows, conflict-free quads)

struct VjpArgs {
  const float* x;        // this step's input state
  const float* g;        // dL/d(next state)
  float* gp;             // [B][4 chn][H][W]
  float* partial;        // [blocks][slots of 1024]
  const float *w1, *b1, *w2;
  int chn, hidden, B, H, W, accumulate;
  float rate; const float* rate_map; const float* u;
  uint32_t s0, s1, t0, t1;
  unsigned long long t;
};

template <int CQ, int NB, int NW>
struct VjpSmem {
  static constexpr int K1 = 16 * CQ, NH = 32 * NB, KP = (K1 + 31) / 32, KB = (K1 + 1 + 31) / 32, LW = NH + 4;
  static constexpr int ACCS = NB * KB + NB;   // dW1 blocks (nb, kb), then dW2 blocks nb
  float xs[4 * CQ][TH + 2][SW];
  float b1[NH];
  float w1t[32 * KP][LW];   // [k][n]
  float w2[16][LW];         // [c][n]
  float t1[NW][NH][PS];     // h, then gh, as [n][pixel]
  float pk[NW][32 * KB][PS];   // p as [k][pixel]; row K1 = 1
  float gy[NW][16][PS];     // gy as [c][pixel]
};

template <int CQ, int NB, int NW>
__global__ __launch_bounds__(64 * NW) void nca_vjp_pixel_kernel(const VjpArgs a) {
  using S = VjpSmem<CQ, NB, NW>;
  static_assert(sizeof(float) * S::ACCS * 1024 <= sizeof(S::t1) + sizeof(S::pk) + sizeof(S::gy), "the wave reduction reuses the slabs");
  __shared__ __attribute__((aligned(16))) S sm;
  constexpr int NT = 64 * NW;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
  const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH, b = blockIdx.z;
  const long plane = (long)a.H * a.W;

  __shared__ int xi[TW + 2], yi[TH + 2];
  if (tid < TW + 2) xi[tid] = wrap(x0 + tid - 1, a.W);
  else if (tid < TW + 2 + TH + 2) yi[tid - (TW + 2)] = wrap(y0 + tid - (TW + 2) - 1, a.H);
  __syncthreads();
  for (int i = tid; i < 4 * CQ * (TH + 2) * (TW + 2); i += NT) {
    const int c = i / ((TH + 2) * (TW + 2)), rem = i - c * ((TH + 2) * (TW + 2)), yy = rem / (TW + 2), xx = rem - yy * (TW + 2);
    float v = 0.f;
    if (c < a.chn) v = a.x[((long)b * a.chn + c) * plane + (long)yi[yy] * a.W + xi[xx]];
    sm.xs[c][yy][xx] = v;
  }
  for (int i = tid; i < S::NH; i += NT) sm.b1[i] = i < a.hidden ? a.b1[i] : 0.f;
  for (int i = tid; i < 32 * S::KP * S::NH; i += NT) {
    const int k = i / S::NH, n = i - k * S::NH;
    sm.w1t[k][n] = (n < a.hidden && k < 4 * a.chn) ? a.w1[n * 4 * a.chn + k] : 0.f;
  }
  for (int i = tid; i < 16 * S::NH; i += NT) {
    const int c = i / S::NH, n = i - c * S::NH;
    sm.w2[c][n] = (c < a.chn && n < a.hidden) ? a.w2[c * a.hidden + n] : 0.f;
  }
  for (int i = lane; i < 32 * S::KB * PS; i += 64) {
    const int k = i / PS;
    sm.pk[wave][k][i - k * PS] = k == S::K1 ? 1.f : 0.f;   // rows < K1 are rewritten per segment
  }
  __syncthreads();

  f32x16 dw1[NB][S::KB], dw2[NB];
#pragma unroll
  for (int nb = 0; nb < NB; nb++) {
#pragma unroll
    for (int g = 0; g < 16; g++) {
      dw2[nb][g] = 0.f;
#pragma unroll
      for (int kb = 0; kb < S::KB; kb++) dw1[nb][kb][g] = 0.f;
    }
  }
  const int rc = r & 15;
  const bool real = r < 16;

  for (int ly = wave; ly < TH; ly += NW) {
    const int gyy = y0 + ly, gx = x0 + r;
    const bool valid = gyy < a.H && gx < a.W;
    const long pix = (long)gyy * a.W + gx;

    // ---- the forward's hidden layer, p into the slab on the way
    f32x16 acc[NB];
#pragma unroll
    for (int nb = 0; nb < NB; nb++)
#pragma unroll
      for (int g = 0; g < 16; g++) acc[nb][g] = sm.b1[32 * nb + (g & 3) + 8 * (g >> 2) + 4 * h];
#pragma unroll
    for (int j = 0; j < 2 * CQ; j++) {
      const f32x4 p = stencils(&sm.xs[2 * j + h][ly][r]);
#pragma unroll
      for (int e = 0; e < 4; e++) sm.pk[wave][8 * j + 4 * h + e][r] = valid ? p[e] : 0.f;
#pragma unroll
      for (int nb = 0; nb < NB; nb++) {
        const int k = 8 * j + 4 * h, n = 32 * nb + r;
        const f32x4 w = {sm.w1t[k][n], sm.w1t[k + 1][n], sm.w1t[k + 2][n], sm.w1t[k + 3][n]};
        Mma<float>::step(acc[nb], __builtin_bit_cast(u32x4, w), __builtin_bit_cast(u32x4, p));
      }
    }
#pragma unroll
    for (int nb = 0; nb < NB; nb++)
#pragma unroll
      for (int g = 0; g < 16; g++) sm.t1[wave][32 * nb + (g & 3) + 8 * (g >> 2) + 4 * h][r] = fmaxf(acc[nb][g], 0.f);

    // ---- gy = mask . g (zero outside the grid), as the B operand of w2^T gy (k = 8 j + 4 h + e = channel) and into the slab
    float mask = 0.f;
    if (valid) mask = nca_mask(a.u, a.rate_map, a.rate, a.t, a.B, b, plane, pix, a.s0, a.s1, a.t0, a.t1);
    f32x16 gh[NB];
#pragma unroll
    for (int nb = 0; nb < NB; nb++)
#pragma unroll
      for (int g = 0; g < 16; g++) gh[nb][g] = 0.f;
#pragma unroll
    for (int j = 0; j < 2; j++) {
      f32x4 gv;
#pragma unroll
      for (int e = 0; e < 4; e++) {
        const int c = 8 * j + 4 * h + e;
        gv[e] = (valid && c < a.chn) ? a.g[((long)b * a.chn + c) * plane + pix] * mask : 0.f;
        sm.gy[wave][c][r] = gv[e];
      }
#pragma unroll
      for (int nb = 0; nb < NB; nb++) {
        const int c = 8 * j + 4 * h, n = 32 * nb + r;
        const f32x4 w = {sm.w2[c][n], sm.w2[c + 1][n], sm.w2[c + 2][n], sm.w2[c + 3][n]};
        Mma<float>::step(gh[nb], __builtin_bit_cast(u32x4, w), __builtin_bit_cast(u32x4, gv));
      }
    }
#pragma unroll
    for (int nb = 0; nb < NB; nb++)
#pragma unroll
      for (int g = 0; g < 16; g++) gh[nb][g] = acc[nb][g] > 0.f ? gh[nb][g] : 0.f;
    __syncthreads();   // the slabs are written (each wave reads its own; the loop is uniform over the workgroup)

    // ---- dW2 += gy h^T: A = gy [c -> 32][pixel], B = h^T [pixel][n]; k = 8 j + 4 h + e = pixel
#pragma unroll
    for (int j = 0; j < 4; j++) {
      u32x4 ga = *reinterpret_cast<const u32x4*>(&sm.gy[wave][rc][8 * j + 4 * h]);
      if (!real) ga = u32x4{0u, 0u, 0u, 0u};
#pragma unroll
      for (int nb = 0; nb < NB; nb++) Mma<float>::step(dw2[nb], ga, *reinterpret_cast<const u32x4*>(&sm.t1[wave][32 * nb + r][8 * j + 4 * h]));
    }
    __syncthreads();
#pragma unroll
    for (int nb = 0; nb < NB; nb++)
#pragma unroll
      for (int g = 0; g < 16; g++) sm.t1[wave][32 * nb + (g & 3) + 8 * (g >> 2) + 4 * h][r] = gh[nb][g];
    __syncthreads();

    // ---- dW1 += gh p^T (column 4 chn: db1): A = gh [n][pixel], B = p^T [pixel][k]
#pragma unroll
    for (int j = 0; j < 4; j++) {
#pragma unroll
      for (int kb = 0; kb < S::KB; kb++) {
        const u32x4 pb = *reinterpret_cast<const u32x4*>(&sm.pk[wave][32 * kb + r][8 * j + 4 * h]);
#pragma unroll
        for (int nb = 0; nb < NB; nb++) Mma<float>::step(dw1[nb][kb], *reinterpret_cast<const u32x4*>(&sm.t1[wave][32 * nb + r][8 * j + 4 * h]), pb);
      }
    }

    // ---- gp^T = w1^T gh: A = w1^T [k][n], B = gh^T's registers (unit 32 nb + 8 q + 4 h + e in register 4 q + e)
#pragma unroll
    for (int kb = 0; kb < S::KP; kb++) {
      f32x16 gp;
#pragma unroll
      for (int g = 0; g < 16; g++) gp[g] = 0.f;
#pragma unroll
      for (int nb = 0; nb < NB; nb++)
#pragma unroll
        for (int q = 0; q < 4; q++) {
          const f32x4 hv = {gh[nb][4 * q], gh[nb][4 * q + 1], gh[nb][4 * q + 2], gh[nb][4 * q + 3]};
          Mma<float>::step(gp, *reinterpret_cast<const u32x4*>(&sm.w1t[32 * kb + r][32 * nb + 8 * q + 4 * h]), __builtin_bit_cast(u32x4, hv));
        }
      if (valid) {
#pragma unroll
        for (int g = 0; g < 16; g++) {
          const int k = 32 * kb + (g & 3) + 8 * (g >> 2) + 4 * h;
          if (k < 4 * a.chn) a.gp[((long)b * 4 * a.chn + k) * plane + pix] = gp[g];
        }
      }
    }
    __syncthreads();   // the slabs are free for the next segment
  }

  // ---- the waves' accumulators, added in wave order; the last wave adds the slot's earlier steps and stores
  float* red = &sm.t1[0][0][0];
  float* slot = a.partial + ((long)(blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * (S::ACCS * 1024);
  for (int w = 0; w < NW; w++) {
    if (wave == w) {
#pragma unroll
      for (int ai = 0; ai < S::ACCS; ai++) {
#pragma unroll
        for (int g = 0; g < 16; g++) {
          const int nb = ai < NB * S::KB ? ai / S::KB : ai - NB * S::KB;
          float v = ai < NB * S::KB ? dw1[nb][ai - nb * S::KB][g] : dw2[nb][g];
          const int o = (ai * 16 + g) * 64 + lane;
          if (w > 0) v = red[o] + v;
          if (w == NW - 1) slot[o] = a.accumulate ? slot[o] + v : v;
          else red[o] = v;
        }
      }
    }
    __syncthreads();
  }
}

// g_new [b][c] = g + sum_f sum_taps F_f[dy][dx] gp[4 c + f][y - dy][x - dx]: the circular stencils with flipped taps
__global__ __launch_bounds__(256) void nca_vjp_stencil_kernel(const float* __restrict__ g, const float* __restrict__ gp, float* __restrict__ out,
                                                              int BC, int H, int W) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const long plane = (long)H * W;
  if (i >= BC * plane) return;
  const long bc = i / plane;
  const int rem = (int)(i - bc * plane), y = rem / W, x = rem - y * W;
  const int ym = y == 0 ? H - 1 : y - 1, yp = y == H - 1 ? 0 : y + 1, xm = x == 0 ? W - 1 : x - 1, xp = x == W - 1 ? 0 : x + 1;
  const float* q = gp + bc * 4 * plane;
  const float* sx = q + plane;
  const float* sy = q + 2 * plane;
  const float* lp = q + 3 * plane;
#define AT(p, yy, xx) p[(long)(yy) * W + (xx)]
  // the tap F[dy][dx] meets gp at (y - dy, x - dx): sobel_x's +1 column (dx = +1) reads x - 1
  const float vx = ((AT(sx, ym, xm) - AT(sx, ym, xp)) + 2.f * (AT(sx, y, xm) - AT(sx, y, xp))) + (AT(sx, yp, xm) - AT(sx, yp, xp));
  const float vy = ((AT(sy, ym, xm) - AT(sy, yp, xm)) + 2.f * (AT(sy, ym, x) - AT(sy, yp, x))) + (AT(sy, ym, xp) - AT(sy, yp, xp));
  const float vl = (((AT(lp, ym, xm) + AT(lp, ym, xp)) + (AT(lp, yp, xm) + AT(lp, yp, xp))) +
                    2.f * ((AT(lp, ym, x) + AT(lp, yp, x)) + (AT(lp, y, xm) + AT(lp, y, xp)))) - 12.f * AT(lp, y, x);
#undef AT
  out[i] = g[i] + ((q[rem] + vx) + (vy + vl));
}

// the workgroups' slots added in index order; element (block ai, register g, lane) -> its place in dW1 / db1 / dW2
__global__ __launch_bounds__(256) void nca_vjp_reduce_kernel(const float* __restrict__ partial, int slots, int accs, int nbk, int kb_n, int k_ones, int chn,
                                                             int hidden, float* __restrict__ dw1, float* __restrict__ db1, float* __restrict__ dw2) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= accs * 1024) return;
  float s = 0.f;
  for (int k = 0; k < slots; k++) s += partial[(long)k * accs * 1024 + i];
  const int ai = i >> 10, g = (i >> 6) & 15, lane = i & 63, r = lane & 31, h = lane >> 5, row = (g & 3) + 8 * (g >> 2) + 4 * h;
  if (ai < nbk) {
    const int nb = ai / kb_n, kb = ai - nb * kb_n, n = 32 * nb + row, k = 32 * kb + r;
    if (n < hidden && k < 4 * chn) dw1[n * 4 * chn + k] = s;
    if (n < hidden && k == k_ones) db1[n] = s;
  } else {
    const int n = 32 * (ai - nbk) + r, c = row;
    if (c < chn && n < hidden) dw2[c * hidden + n] = s;
  }
}

}  // namespace

}  // namespace maua

using namespace maua;

extern "C" {

int maua_nca_vjp(maua_nca* h, const maua_nca_desc* d, const float* states, const float* g_last, float* g_first, float* dw1, float* db1,
                 float* dw2) {
  MAUA_REQUIRE(h && d, "maua_nca_vjp: handle or desc is NULL");
  MAUA_REQUIRE(states && g_last && g_first && dw1 && db1 && dw2 && d->w1 && d->b1 && d->w2, "maua_nca_vjp: a pointer is NULL");
  MAUA_REQUIRE(d->B >= 1 && d->B <= 65535 && d->H >= 3 && d->W >= 3 && d->H <= 65535 * TH, "maua_nca_vjp: B must be in 1 .. 65535, H and W at least 3");
  MAUA_REQUIRE(d->n_steps >= 0, "maua_nca_vjp: n_steps is negative");
  MAUA_REQUIRE(g_first != g_last, "maua_nca_vjp: g_first may not alias g_last (the walk reads one while it writes the other)");
  MAUA_REQUIRE(d->W_sub == 0 && d->col0 == 0 && d->margin == 0, "maua_nca_vjp: no window mode");
  MAUA_REQUIRE((long)d->B * 4 * h->chn * d->H * d->W < (1l << 40), "maua_nca_vjp: state too large");
  const int chn = h->chn, hidden = h->hidden;
  const long plane = (long)d->H * d->W, n = (long)d->B * chn * plane;
  hipStream_t st = h->ctx->stream;
  const bool small = chn <= 12 && hidden <= 96;
  const int kb_n = small ? 2 : 3, nb_n = small ? 3 : 4, accs = nb_n * kb_n + nb_n;
  const dim3 grid(cdiv(d->W, TW), cdiv(d->H, TH), d->B);
  const long slots = (long)grid.x * grid.y * grid.z;
  // workspace: the second gradient buffer, gp, the partials
  const size_t g_bytes = (size_t)n * sizeof(float), gp_bytes = 4 * g_bytes, part_bytes = (size_t)slots * accs * 1024 * sizeof(float);
  if (d->n_steps == 0) {                       // (no workspace needed)
    MAUA_HIP_CHECK(hipMemcpyAsync(g_first, g_last, g_bytes, hipMemcpyDeviceToDevice, st));
    MAUA_HIP_CHECK(hipMemsetAsync(dw1, 0, (size_t)hidden * 4 * chn * sizeof(float), st));
    MAUA_HIP_CHECK(hipMemsetAsync(db1, 0, (size_t)hidden * sizeof(float), st));
    MAUA_HIP_CHECK(hipMemsetAsync(dw2, 0, (size_t)chn * hidden * sizeof(float), st));
    return MAUA_OK;
  }
  if (int rc = nca_reserve(h, g_bytes + gp_bytes + part_bytes)) return rc;
  float* g_tmp = h->tmp.as<float>();
  float* gp = g_tmp + n;
  float* partial = gp + 4 * n;
  VjpArgs a{};
  a.gp = gp; a.partial = partial; a.w1 = d->w1; a.b1 = d->b1; a.w2 = d->w2;
  a.chn = chn; a.hidden = hidden; a.B = d->B; a.H = d->H; a.W = d->W;
  a.rate = d->rate; a.rate_map = d->rate_map;
  a.s0 = (uint32_t)d->seed; a.s1 = (uint32_t)(d->seed >> 32); a.t0 = (uint32_t)d->stream; a.t1 = (uint32_t)(d->stream >> 32);
  const float* cur = g_last;
  for (int s = d->n_steps - 1; s >= 0; s--) {
    float* nxt = (s & 1) ? g_tmp : g_first;   // step 0 writes g_first
    a.x = states + (long)s * n; a.g = cur; a.accumulate = s != d->n_steps - 1;
    a.t = d->step0 + (unsigned long long)s;
    a.u = d->u ? d->u + (long)s * d->B * plane : nullptr;
    if (small) hipLaunchKernelGGL((nca_vjp_pixel_kernel<3, 3, 4>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((nca_vjp_pixel_kernel<4, 4, 2>), grid, dim3(128), 0, st, a);
    hipLaunchKernelGGL(nca_vjp_stencil_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, cur, gp, nxt, d->B * chn, d->H, d->W);
    cur = nxt;
  }
  hipLaunchKernelGGL(nca_vjp_reduce_kernel, dim3((accs * 1024 + 255) / 256), dim3(256), 0, st, partial, (int)slots, accs, nb_n * kb_n, kb_n, small ? 48 : 64, chn,
                     hidden, dw1, db1, dw2);
  MAUA_HIP_CHECK(hipGetLastError());
  return MAUA_OK;
}

}  // extern "C"
