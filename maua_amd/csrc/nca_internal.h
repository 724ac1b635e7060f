// What the cellular automaton's step (nca.hip) and its gradient (nca_vjp.hip) share: the tile, the stencils, the update mask, the handle.
#pragma once
#include "common.h"
#include "internal.h"
#include "mma.h"
#include "philox.h"

struct maua_nca {
  maua_ctx* ctx;
  int chn, hidden, dtype;
  maua::DevBuf tmp;   // float, grow-only: the step's second state buffer / the gradient's workspace
};

namespace maua {

// tile: 4 rows (one 32-pixel segment per wave) measured 17-18 % faster than 8 and 80 % faster than 16 on the 256 x 256 render (the
// step is bound by latency, and two workgroups per CU overlap one's staging with the other's products); SW: LDS row stride (34 used)
constexpr int TH = 4, TW = 32, SW = TW + 4;

__device__ __forceinline__ int wrap(int v, int n) { v %= n; return v < 0 ? v + n : v; }

// the four stencils of one channel at tile position (row ly, column r) of plane p with LDS row stride SW (taps as train.py:153-155,
// summed row by row)
template <int SW>
__device__ __forceinline__ f32x4 stencils_ld(const float* p) {
  const float a = p[0], b = p[1], c = p[2], d = p[SW], e = p[SW + 1], f = p[SW + 2], g = p[2 * SW], h = p[2 * SW + 1], i = p[2 * SW + 2];
  f32x4 o;
  o[0] = e;
  o[1] = ((c - a) + 2.f * (f - d)) + (i - g);
  o[2] = ((g - a) + 2.f * (h - b)) + (i - c);
  o[3] = __builtin_fmaf(-12.f, e, ((a + c) + (g + i)) + 2.f * ((b + h) + (d + f)));   // the one inexact product: fused by name, so that
                                                                                        // every instantiation rounds it the same way
  return o;
}
__device__ __forceinline__ f32x4 stencils(const float* p) { return stencils_ld<SW>(p); }

// floorf(u + rate) of pixel `pix` (= y * row length + x) of image b at step t: the caller's uniforms (u: this step's [B][H][W]) or
// unit23 of word (t B + b) plane + pix of the Philox stream (key s0 s1, stream t0 t1) in rng.hip's addressing
__device__ __forceinline__ float nca_mask(const float* u, const float* rate_map, float rate, unsigned long long t, int B, int b, long plane,
                                          long pix, uint32_t s0, uint32_t s1, uint32_t t0, uint32_t t1) {
  float uv;
  if (u) {
    uv = u[(long)b * plane + pix];
  } else {
    const unsigned long long idx = (t * (unsigned long long)B + (unsigned long long)b) * (unsigned long long)plane + (unsigned long long)pix;
    const unsigned long long ctr = idx >> 2;
    const U4 v = philox4x32_10((uint32_t)ctr, (uint32_t)(ctr >> 32), t0, t1, s0, s1);
    const uint32_t wsel = (uint32_t)(idx & 3);
    uv = unit23(wsel == 0 ? v.x : wsel == 1 ? v.y : wsel == 2 ? v.z : v.w);
  }
  return floorf(uv + (rate_map ? rate_map[pix] : rate));
}

static inline bool nca_sizes_ok(int chn, int hidden) {
  return chn >= 4 && chn <= 16 && chn % 4 == 0 && hidden >= 32 && hidden <= 128 && hidden % 32 == 0;
}

static inline int nca_reserve(maua_nca* h, size_t bytes) {
  if (bytes <= h->tmp.bytes()) return MAUA_OK;
  if (h->tmp) MAUA_HIP_CHECK(hipStreamSynchronize(h->ctx->stream));
  return h->tmp.alloc(bytes);
}

}  // namespace maua
