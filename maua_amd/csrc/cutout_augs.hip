// The torchvision augmentation pipeline of "normal" and "dango" cutouts, and its adjoint.
//
// Replaces (reference): maua/ops/cutouts.py:59-71 / 133-146 - `self.augs`, the "Video Input" pipeline both classes default to
// (skip_augs=False):
//   RandomHorizontalFlip(0.5), +N(0,1) 0.01, RandomAffine(15, translate=(0.1, 0.1)) [NEAREST, fill 0], +noise,
//   RandomPerspective(0.4, p=0.7) [BILINEAR, fill 0], +noise, RandomGrayscale(0.15), +noise
// and the part of `torch.autograd.grad(loss, img)` (grad.py:155) that runs back through it.  torchvision is absent from the reference
// tree and the image: its tensor path (>= 0.12) is restated (parity unpinned; tests/torchvision_augs_ref.py is the CPU statement).
//   "normal" (Cutouts): one record per cutout, applied to the crop at the crop's own size s before the resize; the B images of a
//            cutout share it.  The augmented crops go to per-cutout slots [n_cut][B][3][S][S] (S = the padded side) which the
//            existing resize reads through CutoutPlan::img_stride.
//   "dango"  (DangoCutouts): one record per call, applied to the whole resized batch [N B][3][cs][cs] (cutout-major).
//
// Records (host, float [AUG_REC = 17], the draw order): flip, affine[6] (torchvision's inverse affine matrix as float32), persp_on,
// persp[8] (float32 perspective coefficients, ignored when off), grey.  aug_records() checks them and adds what the kernels need:
// the grid coefficients rescaled like torchvision's (theta^T / (0.5 w, 0.5 h), float32) and, in double, the inverse of each warp's
// pixel map (sample coordinate -> output pixel), which bounds the adjoint's candidate windows.
//
// Noise (the `x + torch.randn_like(x) * 0.01` Lambdas): the library's Philox4x32-10 normals (rng.hip, CPU twin oracle/rng.py), key =
// one 64-bit value per cutout call (drawn by the host from torch's device generator), stream = 4 j + stage (stage 0..3 in pipeline
// order), offset = the row-major element index of the tensor the stage sees: "normal": j = the cutout's index in its call, the tensor
// [B][3][s][s]; "dango": j = 0, the tensor [N B][3][cs][cs].  The adjoint does not see it (every stage is affine in the image).
//
// Fill: the warps fill with 0 in the [0, 1] space (after (img + 1) / 2): the "normal" padding (-1 in the sampler's range) is 0 there.
//
// Grids (torchvision's expression order, float32, no contraction):
//   affine       xb = x - s/2 + 0.5; gx = xb a0 + yb a1 + a2 (a = theta / (0.5 s)); ix = ((gx + 1) s - 1) / 2; nearest = rint (half to
//                even), 0 outside.  The appended-ones mask of _apply_grid_transform is 1 or 0 under nearest: the plain zero-padded sample.
//   perspective  xb = x + 0.5; gx = (xb p0 + yb p1 + p2) / (xb p6 + yb p7 + 1) - 1 (p0..5 / (0.5 s)); bilinear taps nw, ne, sw, se;
//                mask m = the in-bounds weights' sum; out = sample * m + (1 - m) * 0 - near the border the value is scaled by the
//                coverage twice, as torchvision does.
//   grey         0.2989 r + 0.587 g + 0.114 b into all three planes.
//
// MI355X design: HBM bound and small beside the perceptor.  Four passes, 64 lanes along x (coalesced rows), 4 rows per workgroup,
// one record per grid z slice (its parameters are wave-uniform: scalar loads from a small device table).
//   forward  (1) src -> A: flip, noise 0, nearest affine, noise 1 (the affine's gather reads the source directly: the flipped, noised
//                stage-1 image is never stored); (2) A -> out: bilinear perspective + mask, noise 2, grey, noise 3, then Normalize and
//                the store (planar f32 slots, or the perceptor's patch rows).
//   adjoint  deterministic gathers, no float atomics (reruns give identical bits, like cutouts.hip):
//            (1) out -> dA: per A pixel, the output pixels whose bilinear footprint touches it - candidates from the inverse
//                perspective map of the pixel's [-1, 1]^2 sample square (bounding box + 1 px), each checked with the SAME float
//                expressions as the forward; the grey adjoint and 1 / std folded in;
//            (2) dA -> d src: per source pixel, the output pixels whose nearest sample it is (inverse affine map of its [-0.5, 0.5]^2
//                square, checked the same way), the flip's mirror, the affine (img + 1) / 2's 1 / 2, and for "normal" the sum over
//                the cutouts covering the pixel in a fixed cutout order.
#include <cmath>
#include <cstring>

#include "common.h"
#include "internal.h"

namespace maua {

namespace {

struct AugRec {
  float aff[6];               // rescaled affine grid coefficients
  float per[8];               // rescaled perspective coefficients
  double ia[9];               // inverse pixel map of the affine (sample coordinate -> output pixel), 3 x 3
  double ip[9];               // the same for the perspective
  unsigned long long key;     // noise key
  int flip, persp, grey, s;   // s: side of the images the record applies to
  int oy, ox;                 // crop origin in the source ("normal"), else 0
  int j, full;                // noise stream base 4 j; full: the perspective's inverse is not usable (scan every pixel)
};

constexpr int AUG_TX = 64, AUG_TY = 4;

struct U4 { uint32_t x, y, z, w; };

// Philox4x32-10 and the Box-Muller pairs exactly as rng.hip's philox_kernel draws them (element i: counter i / 4, word pair i % 4 / 2)
__device__ __forceinline__ U4 philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; r++) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
    c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return U4{c0, c1, c2, c3};
}

__device__ __forceinline__ float unit23(uint32_t x) { return ((float)(x >> 9) + 0.5f) * 1.1920928955078125e-07f; }

// x + randn * 0.01 for element i of stream `stream`
__device__ __forceinline__ float add_noise(float x, unsigned long long key, uint32_t stream, unsigned long long i) {
  const unsigned long long c = i >> 2;
  const U4 v = philox((uint32_t)c, (uint32_t)(c >> 32), stream, 0u, (uint32_t)key, (uint32_t)(key >> 32));
  const int w = (int)(i & 3);
  const uint32_t a = w < 2 ? v.x : v.z, b = w < 2 ? v.y : v.w;
  const float r = sqrtf(-2.0f * logf(unit23(a)));
  const float th = 6.283185307179586f * unit23(b);
  const float z = (w & 1) ? r * sinf(th) : r * cosf(th);
  return __fadd_rn(x, __fmul_rn(z, 0.01f));
}

__device__ __forceinline__ unsigned long long elem(long img, int c, int y, int x, int s) {
  return (((unsigned long long)img * 3 + c) * s + y) * s + x;
}

// grid_sampler_unnormalize (align_corners=False): ((g + 1) s - 1) / 2
__device__ __forceinline__ float unnorm(float g, int s) { return __fmul_rn(__fsub_rn(__fmul_rn(__fadd_rn(g, 1.f), (float)s), 1.f), 0.5f); }

// the nearest affine sample of output pixel (x, y): source (nx, ny), false outside
__device__ __forceinline__ bool affine_at(const AugRec& R, int x, int y, int& nx, int& ny) {
  const float c0 = 0.5f - 0.5f * (float)R.s;
  const float xb = __fadd_rn((float)x, c0), yb = __fadd_rn((float)y, c0);
  const float gx = __fadd_rn(__fadd_rn(__fmul_rn(xb, R.aff[0]), __fmul_rn(yb, R.aff[1])), R.aff[2]);
  const float gy = __fadd_rn(__fadd_rn(__fmul_rn(xb, R.aff[3]), __fmul_rn(yb, R.aff[4])), R.aff[5]);
  nx = (int)rintf(unnorm(gx, R.s));
  ny = (int)rintf(unnorm(gy, R.s));
  return nx >= 0 && nx < R.s && ny >= 0 && ny < R.s;
}

// the perspective's bilinear footprint of output pixel (x, y): top-left tap (x0, y0), the four weights (nw, ne, sw, se), the mask m
__device__ __forceinline__ void persp_at(const AugRec& R, int x, int y, int& x0, int& y0, float w[4], float& m) {
  const float xb = __fadd_rn((float)x, 0.5f), yb = __fadd_rn((float)y, 0.5f);
  const float g1x = __fadd_rn(__fadd_rn(__fmul_rn(xb, R.per[0]), __fmul_rn(yb, R.per[1])), R.per[2]);
  const float g1y = __fadd_rn(__fadd_rn(__fmul_rn(xb, R.per[3]), __fmul_rn(yb, R.per[4])), R.per[5]);
  const float g2 = __fadd_rn(__fadd_rn(__fmul_rn(xb, R.per[6]), __fmul_rn(yb, R.per[7])), 1.f);
  const float ix = unnorm(__fsub_rn(__fdiv_rn(g1x, g2), 1.f), R.s), iy = unnorm(__fsub_rn(__fdiv_rn(g1y, g2), 1.f), R.s);
  const float fx = floorf(ix), fy = floorf(iy);
  const float ex = __fsub_rn(__fadd_rn(fx, 1.f), ix), ey = __fsub_rn(__fadd_rn(fy, 1.f), iy);
  const float dx = __fsub_rn(ix, fx), dy = __fsub_rn(iy, fy);
  w[0] = __fmul_rn(ex, ey); w[1] = __fmul_rn(dx, ey); w[2] = __fmul_rn(ex, dy); w[3] = __fmul_rn(dx, dy);
  // (a sample far outside: the taps stay out of bounds; clamp before the int conversion)
  x0 = (int)fmaxf(fminf(fx, 1e6f), -1e6f);
  y0 = (int)fmaxf(fminf(fy, 1e6f), -1e6f);
  m = 0.f;
#pragma unroll
  for (int t = 0; t < 4; t++) {
    const int xx = x0 + (t & 1), yy = y0 + (t >> 1);
    if (xx >= 0 && xx < R.s && yy >= 0 && yy < R.s) m = __fadd_rn(m, w[t]);
  }
}

// the output pixels whose sample can land in the sample-space square [u - r, u + r] x [v - r, v + r] under the map whose inverse is
// `inv`: the bounding box of the corners' images + 1 px, clipped to the image; the whole image if a corner has no finite image
__device__ __forceinline__ void window(const double* inv, bool full, double u, double v, double r, int s, int& xa, int& xb, int& ya, int& yb) {
  xa = 0; ya = 0; xb = s - 1; yb = s - 1;
  if (full) return;
  double lx = 1e300, hx = -1e300, ly = 1e300, hy = -1e300;
  for (int k = 0; k < 4; k++) {
    const double cu = u + ((k & 1) ? r : -r), cv = v + ((k & 2) ? r : -r);
    const double hw = inv[6] * cu + inv[7] * cv + inv[8];
    if (!(hw > 1e-12)) return;
    const double px = (inv[0] * cu + inv[1] * cv + inv[2]) / hw, py = (inv[3] * cu + inv[4] * cv + inv[5]) / hw;
    lx = fmin(lx, px); hx = fmax(hx, px); ly = fmin(ly, py); hy = fmax(hy, py);
  }
  xa = (int)fmax(floor(lx) - 1.0, 0.0); xb = (int)fmin(ceil(hx) + 1.0, (double)(s - 1));
  ya = (int)fmax(floor(ly) - 1.0, 0.0); yb = (int)fmin(ceil(hy) + 1.0, (double)(s - 1));
}

struct AugArgs {
  const AugRec* rec;
  int n_rec, nimg, S, noise_i0;
  const float* src;      // forward (1): [nimg][3][H][W] (crop at the record's (oy, ox)), read as src * mul + add
  int H, W;
  float mul, add;
  const float* a;        // A: [n_rec * nimg][3][S][S]
  float* a_out;
  void* out;             // forward (2): planar f32 [n_rec * nimg][3][S][S] or patch rows (T) of S x S images
  const void* d_out;     // adjoint (1): the same layouts
  int patch, patch_ld;   // patch_ld: elements between patch rows (>= 3 p p; the columns past 3 p p are neither written nor read)
  float mean[3], inv_std[3];
  float* dst;            // adjoint (2): [nimg][3][H][W]
  int accumulate;
};

// grid (ceil(S / 64), ceil(S / 4), n_rec * nimg), block (64, 4)
__global__ __launch_bounds__(256) void aug_fwd_src_kernel(AugArgs a) {
  const int x = blockIdx.x * AUG_TX + threadIdx.x, y = blockIdx.y * AUG_TY + threadIdx.y;
  const long i = blockIdx.z;
  const int r = (int)(i / a.nimg), b = (int)(i - (long)r * a.nimg);
  const AugRec& R = a.rec[r];
  if (x >= R.s || y >= R.s) return;
  const long nb = b + a.noise_i0;
  int nx, ny;
  const bool in = affine_at(R, x, y, nx, ny);
  const long plane = (long)a.H * a.W;
  const int sx = R.flip ? R.s - 1 - nx : nx;
  const uint32_t st0 = 4u * R.j, st1 = st0 + 1u;
#pragma unroll
  for (int c = 0; c < 3; c++) {
    float v = 0.f;
    if (in) {
      v = fmaf(a.src[((long)b * 3 + c) * plane + (long)(R.oy + ny) * a.W + R.ox + sx], a.mul, a.add);
      v = add_noise(v, R.key, st0, elem(nb, c, ny, nx, R.s));
    }
    v = add_noise(v, R.key, st1, elem(nb, c, y, x, R.s));
    a.a_out[((i * 3 + c) * a.S + y) * a.S + x] = v;
  }
}

template <typename T>
__device__ __forceinline__ long patch_index(const AugArgs& a, long img, int c, int y, int x) {
  const int p = a.patch, g = a.S / p;
  return (img * g * g + (long)(y / p) * g + x / p) * a.patch_ld + c * p * p + (y % p) * p + x % p;
}

template <typename T>
__global__ __launch_bounds__(256) void aug_fwd_out_kernel(AugArgs a) {
  const int x = blockIdx.x * AUG_TX + threadIdx.x, y = blockIdx.y * AUG_TY + threadIdx.y;
  const long i = blockIdx.z;
  const int r = (int)(i / a.nimg), b = (int)(i - (long)r * a.nimg);
  const AugRec& R = a.rec[r];
  if (x >= R.s || y >= R.s) return;
  const long nb = b + a.noise_i0;
  const long plane = (long)a.S * a.S;
  const float* A = a.a + i * 3 * plane;
  float v[3];
  if (R.persp) {
    int x0, y0;
    float w[4], m;
    persp_at(R, x, y, x0, y0, w, m);
#pragma unroll
    for (int c = 0; c < 3; c++) {
      float acc = 0.f;
#pragma unroll
      for (int t = 0; t < 4; t++) {
        const int xx = x0 + (t & 1), yy = y0 + (t >> 1);
        const float sv = (xx >= 0 && xx < R.s && yy >= 0 && yy < R.s) ? A[c * plane + (long)yy * a.S + xx] : 0.f;
        acc = __fadd_rn(acc, __fmul_rn(sv, w[t]));
      }
      v[c] = __fmul_rn(acc, m);
    }
  } else {
#pragma unroll
    for (int c = 0; c < 3; c++) v[c] = A[c * plane + (long)y * a.S + x];
  }
  const uint32_t st2 = 4u * R.j + 2u, st3 = st2 + 1u;
#pragma unroll
  for (int c = 0; c < 3; c++) v[c] = add_noise(v[c], R.key, st2, elem(nb, c, y, x, R.s));
  if (R.grey) {
    const float l = __fadd_rn(__fadd_rn(__fmul_rn(0.2989f, v[0]), __fmul_rn(0.587f, v[1])), __fmul_rn(0.114f, v[2]));
    v[0] = v[1] = v[2] = l;
  }
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const float o = (add_noise(v[c], R.key, st3, elem(nb, c, y, x, R.s)) - a.mean[c]) * a.inv_std[c];
    if (a.patch == 0) reinterpret_cast<float*>(a.out)[(i * 3 + c) * plane + (long)y * a.S + x] = o;
    else Elem<T>::store(reinterpret_cast<T*>(a.out) + patch_index<T>(a, i, c, y, x), o);
  }
}

// the upstream gradient of output pixel (x, y) of image i, through Normalize and the grey stage's adjoint
template <typename T>
__device__ __forceinline__ void grad_at(const AugArgs& a, const AugRec& R, long i, int x, int y, float g[3]) {
  const long plane = (long)a.S * a.S;
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const float d = a.patch == 0 ? reinterpret_cast<const float*>(a.d_out)[(i * 3 + c) * plane + (long)y * a.S + x]
                                 : Elem<T>::load(reinterpret_cast<const T*>(a.d_out) + patch_index<T>(a, i, c, y, x));
    g[c] = d * a.inv_std[c];
  }
  if (R.grey) {
    const float t = g[0] + g[1] + g[2];
    g[0] = 0.2989f * t; g[1] = 0.587f * t; g[2] = 0.114f * t;
  }
}

// adjoint (1): out -> dA.  grid (ceil(S / 64), ceil(S / 4), n_rec * nimg)
template <typename T>
__global__ __launch_bounds__(256) void aug_adj_out_kernel(AugArgs a) {
  const int x = blockIdx.x * AUG_TX + threadIdx.x, y = blockIdx.y * AUG_TY + threadIdx.y;
  const long i = blockIdx.z;
  const int r = (int)(i / a.nimg);
  const AugRec& R = a.rec[r];
  if (x >= R.s || y >= R.s) return;
  float acc[3] = {0.f, 0.f, 0.f};
  if (!R.persp) {
    grad_at<T>(a, R, i, x, y, acc);
  } else {
    int xa, xb, ya, yb;
    window(R.ip, R.full != 0, (double)x, (double)y, 1.0, R.s, xa, xb, ya, yb);
    for (int oy = ya; oy <= yb; oy++)
      for (int ox = xa; ox <= xb; ox++) {
        int x0, y0;
        float w[4], m;
        persp_at(R, ox, oy, x0, y0, w, m);
        const int tx = x - x0, ty = y - y0;
        if (tx < 0 || tx > 1 || ty < 0 || ty > 1) continue;
        const float wt = w[ty * 2 + tx] * m;
        float g[3];
        grad_at<T>(a, R, i, ox, oy, g);
#pragma unroll
        for (int c = 0; c < 3; c++) acc[c] = fmaf(wt, g[c], acc[c]);
      }
  }
  const long plane = (long)a.S * a.S;
#pragma unroll
  for (int c = 0; c < 3; c++) a.a_out[(i * 3 + c) * plane + (long)y * a.S + x] = acc[c];
}

// adjoint (2): dA -> d src, summed over the records covering the pixel.  grid (ceil(W / 64), ceil(H / 4), nimg)
__global__ __launch_bounds__(256) void aug_adj_src_kernel(AugArgs a) {
  const int X = blockIdx.x * AUG_TX + threadIdx.x, Y = blockIdx.y * AUG_TY + threadIdx.y;
  const int b = blockIdx.z;
  if (X >= a.W || Y >= a.H) return;
  const long plane = (long)a.S * a.S;
  float acc[3] = {0.f, 0.f, 0.f};
  for (int r = 0; r < a.n_rec; r++) {
    const AugRec& R = a.rec[r];
    const int y1 = Y - R.oy, xs = X - R.ox;
    if (y1 < 0 || y1 >= R.s || xs < 0 || xs >= R.s) continue;
    const int x1 = R.flip ? R.s - 1 - xs : xs;
    const float* dA = a.a + ((long)r * a.nimg + b) * 3 * plane;
    int xa, xb, ya, yb;
    window(R.ia, false, (double)x1, (double)y1, 0.5, R.s, xa, xb, ya, yb);
    for (int oy = ya; oy <= yb; oy++)
      for (int ox = xa; ox <= xb; ox++) {
        int nx, ny;
        if (!affine_at(R, ox, oy, nx, ny) || nx != x1 || ny != y1) continue;
#pragma unroll
        for (int c = 0; c < 3; c++) acc[c] += dA[c * plane + (long)oy * a.S + ox];
      }
  }
  const long dplane = (long)a.H * a.W;
#pragma unroll
  for (int c = 0; c < 3; c++) {
    float* d = a.dst + ((long)b * 3 + c) * dplane + (long)Y * a.W + X;
    *d = a.accumulate ? *d + acc[c] * a.mul : acc[c] * a.mul;
  }
}

// ------------------------------------------------------------------------------------------------ host side
void mat3_mul(const double* a, const double* b, double* o) {
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) o[3 * i + j] = a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j] + a[3 * i + 2] * b[6 + j];
}

bool mat3_inv(const double* m, double* o) {
  const double det = m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
  if (!std::isfinite(det) || std::fabs(det) < 1e-12) return false;
  o[0] = (m[4] * m[8] - m[5] * m[7]) / det; o[1] = (m[2] * m[7] - m[1] * m[8]) / det; o[2] = (m[1] * m[5] - m[2] * m[4]) / det;
  o[3] = (m[5] * m[6] - m[3] * m[8]) / det; o[4] = (m[0] * m[8] - m[2] * m[6]) / det; o[5] = (m[2] * m[3] - m[0] * m[5]) / det;
  o[6] = (m[3] * m[7] - m[4] * m[6]) / det; o[7] = (m[1] * m[6] - m[0] * m[7]) / det; o[8] = (m[0] * m[4] - m[1] * m[3]) / det;
  for (int k = 0; k < 9; k++)
    if (!std::isfinite(o[k])) return false;
  return true;
}

bool is_bit(float v) { return v == 0.f || v == 1.f; }

}  // namespace

size_t aug_record_bytes() { return sizeof(AugRec); }

// augs: [n_rec][AUG_REC]; rects: host [n_rec][3] (size, top, left) for "normal", NULL for "dango" (side `side`, origin 0); record r
// takes keys[r / recs_per_key] and noise j = r % recs_per_key ("dango": recs_per_key 1, j = 0)
int aug_records(const float* augs, int n_rec, const int* rects, int side, const unsigned long long* keys, int recs_per_key, void* host_out) {
  MAUA_REQUIRE(augs && keys && host_out && n_rec > 0 && recs_per_key > 0, "cutout augmentations: bad arguments");
  AugRec* out = (AugRec*)host_out;
  for (int r = 0; r < n_rec; r++) {
    const float* f = augs + (long)r * AUG_REC;
    AugRec R;
    std::memset(&R, 0, sizeof(R));
    const std::string at = "cutout augmentations: record " + std::to_string(r) + ": ";
    if (!is_bit(f[0]) || !is_bit(f[7]) || !is_bit(f[16])) return fail(at + "the flip / perspective / grey entries must be 0 or 1");
    for (int k = 1; k < 7; k++)
      if (!std::isfinite(f[k])) return fail(at + "the affine matrix is not finite");
    if (f[7] != 0.f)
      for (int k = 8; k < 16; k++)
        if (!std::isfinite(f[k])) return fail(at + "the perspective coefficients are not finite");
    R.flip = f[0] != 0.f; R.persp = f[7] != 0.f; R.grey = f[16] != 0.f;
    R.s = rects ? (rects[3 * r] & CUT_SIZE_MASK) : side;
    R.oy = rects ? rects[3 * r + 1] : 0;
    R.ox = rects ? rects[3 * r + 2] : 0;
    MAUA_REQUIRE(R.s > 0, "cutout augmentations: empty image");
    R.key = keys[r / recs_per_key];
    R.j = r % recs_per_key;
    const float hs = 0.5f * (float)R.s;   // torch.tensor([0.5 w, 0.5 h]) (float32; exact)
    for (int k = 0; k < 6; k++) R.aff[k] = f[1 + k] / hs;
    // the affine's pixel map: ix = a0 xb + a1 yb + a2 + (s - 1) / 2, xb = x + 0.5 - s / 2
    const double s = R.s, cx = 0.5 - 0.5 * s, h = (s - 1) / 2;
    const double ma[9] = {f[1], f[2], f[1] * cx + f[2] * cx + f[3] + h, f[4], f[5], f[4] * cx + f[5] * cx + f[6] + h, 0, 0, 1};
    if (!mat3_inv(ma, R.ia)) return fail(at + "the affine matrix is singular");
    if (R.persp) {
      for (int k = 0; k < 6; k++) R.per[k] = f[8 + k] / hs;
      R.per[6] = f[14]; R.per[7] = f[15];
      // the perspective's pixel map: (ix + 0.5, iy + 0.5) = H (x + 0.5, y + 0.5)
      const double hc[9] = {f[8], f[9], f[10], f[11], f[12], f[13], f[14], f[15], 1.0};
      const double tin[9] = {1, 0, 0.5, 0, 1, 0.5, 0, 0, 1}, tout[9] = {1, 0, -0.5, 0, 1, -0.5, 0, 0, 1};
      double t1[9], mp[9];
      mat3_mul(hc, tin, t1);
      mat3_mul(tout, t1, mp);
      if (!mat3_inv(mp, R.ip)) return fail(at + "the perspective transform is singular");
      // the windows need a positive denominator over the whole output image (it is affine in x, y: the corners decide)
      for (int k = 0; k < 4; k++) {
        const double xb = (k & 1) ? s : 0.0, yb = (k & 2) ? s : 0.0;
        if (!(f[14] * xb + f[15] * yb + 1.0 > 1e-6)) R.full = 1;
      }
      if (!R.full) {   // scale the inverse so that its third component is positive where the forward's denominator is
        const double u = mp[0] * 0.0 + mp[1] * 0.0 + mp[2], v = mp[3] * 0.0 + mp[4] * 0.0 + mp[5], w = mp[8];
        const double hw = R.ip[6] * (u / w) + R.ip[7] * (v / w) + R.ip[8];
        if (hw < 0)
          for (int k = 0; k < 9; k++) R.ip[k] = -R.ip[k];
      }
    }
    out[r] = R;
  }
  return MAUA_OK;
}

static AugArgs args(const void* recs, int n_rec, int nimg, int S, int noise_i0) {
  AugArgs a{};
  a.rec = (const AugRec*)recs; a.n_rec = n_rec; a.nimg = nimg; a.S = S; a.noise_i0 = noise_i0;
  for (int c = 0; c < 3; c++) { a.mean[c] = 0.f; a.inv_std[c] = 1.f; }
  return a;
}

static int check_grid(int n_rec, int nimg, int S) {
  MAUA_REQUIRE(n_rec > 0 && nimg > 0 && S > 0 && (long)n_rec * nimg <= 65535, "cutout augmentations: at most 65535 images per launch");
  return MAUA_OK;
}

int aug_forward_src(hipStream_t st, const void* recs, int n_rec, int nimg, int S, int noise_i0, const float* src, int H, int W, float mul,
                    float add, float* x1) {
  if (int rc = check_grid(n_rec, nimg, S)) return rc;
  AugArgs a = args(recs, n_rec, nimg, S, noise_i0);
  a.src = src; a.H = H; a.W = W; a.mul = mul; a.add = add; a.a_out = x1;
  hipLaunchKernelGGL(aug_fwd_src_kernel, dim3((unsigned)cdiv(S, AUG_TX), (unsigned)cdiv(S, AUG_TY), (unsigned)(n_rec * nimg)),
                     dim3(AUG_TX, AUG_TY), 0, st, a);
  MAUA_HIP_CHECK(hipGetLastError());
  return MAUA_OK;
}

int aug_forward_out(hipStream_t st, int dtype, const void* recs, int n_rec, int nimg, int S, int noise_i0, const float* x1, void* out,
                    int patch, const float* mean3, const float* std3, int patch_ld) {
  if (int rc = check_grid(n_rec, nimg, S)) return rc;
  MAUA_REQUIRE(patch == 0 || S % patch == 0, "cutout augmentations: the side must be a whole number of patches");
  MAUA_REQUIRE(patch_ld == 0 || (patch > 0 && patch_ld >= 3 * patch * patch), "cutout augmentations: the patch-row stride is below 3 * patch^2");
  AugArgs a = args(recs, n_rec, nimg, S, noise_i0);
  a.a = x1; a.out = out; a.patch = patch; a.patch_ld = patch_ld ? patch_ld : 3 * patch * patch;
  for (int c = 0; c < 3; c++) { a.mean[c] = mean3[c]; a.inv_std[c] = 1.f / std3[c]; }
  const dim3 grid((unsigned)cdiv(S, AUG_TX), (unsigned)cdiv(S, AUG_TY), (unsigned)(n_rec * nimg)), block(AUG_TX, AUG_TY);
  auto launch = [&](auto t) { hipLaunchKernelGGL(aug_fwd_out_kernel<decltype(t)>, grid, block, 0, st, a); };
  if (int rc = dispatch_dtype<bf16_t, float>(dtype, "cutout augmentations", launch)) return rc;
  MAUA_HIP_CHECK(hipGetLastError());
  return MAUA_OK;
}

int aug_adjoint_out(hipStream_t st, int dtype, const void* recs, int n_rec, int nimg, int S, const void* d_out, int patch,
                    const float* std3, float* d_a, int patch_ld) {
  if (int rc = check_grid(n_rec, nimg, S)) return rc;
  MAUA_REQUIRE(patch == 0 || S % patch == 0, "cutout augmentations: the side must be a whole number of patches");
  MAUA_REQUIRE(patch_ld == 0 || (patch > 0 && patch_ld >= 3 * patch * patch), "cutout augmentations: the patch-row stride is below 3 * patch^2");
  AugArgs a = args(recs, n_rec, nimg, S, 0);
  a.d_out = d_out; a.patch = patch; a.patch_ld = patch_ld ? patch_ld : 3 * patch * patch; a.a_out = d_a;
  for (int c = 0; c < 3; c++) a.inv_std[c] = 1.f / std3[c];
  const dim3 grid((unsigned)cdiv(S, AUG_TX), (unsigned)cdiv(S, AUG_TY), (unsigned)(n_rec * nimg)), block(AUG_TX, AUG_TY);
  auto launch = [&](auto t) { hipLaunchKernelGGL(aug_adj_out_kernel<decltype(t)>, grid, block, 0, st, a); };
  if (int rc = dispatch_dtype<bf16_t, float>(dtype, "cutout augmentations", launch)) return rc;
  MAUA_HIP_CHECK(hipGetLastError());
  return MAUA_OK;
}

int aug_adjoint_src(hipStream_t st, const void* recs, int n_rec, int nimg, int S, const float* d_a, int H, int W, float mul, float* dst,
                    int accumulate) {
  if (int rc = check_grid(n_rec, nimg, S)) return rc;
  MAUA_REQUIRE(H <= 4 * 65535, "cutout augmentations: image too tall for one launch");
  AugArgs a = args(recs, n_rec, nimg, S, 0);
  a.a = d_a; a.H = H; a.W = W; a.mul = mul; a.dst = dst; a.accumulate = accumulate;
  hipLaunchKernelGGL(aug_adj_src_kernel, dim3((unsigned)cdiv(W, AUG_TX), (unsigned)cdiv(H, AUG_TY), (unsigned)nimg), dim3(AUG_TX, AUG_TY),
                     0, st, a);
  MAUA_HIP_CHECK(hipGetLastError());
  return MAUA_OK;
}

}  // namespace maua

using namespace maua;

extern "C" {

// see include/maua_hip.h.  Workspace (the context's scratch): tables | rects | records | A | B
static int cutouts_aug_common(maua_ctx* ctx, const char* who, int B, int H, int W, const int* rects, int n_cut, int cut_size,
                              const float* augs, unsigned long long key, int per_call, std::vector<char>& recs, int& n_rec, int& S) {
  MAUA_REQUIRE(B > 0 && n_cut > 0 && cut_size > 0 && H > 0 && W > 0, std::string(who) + ": bad sizes");
  MAUA_REQUIRE(per_call == 0 || per_call == 1, std::string(who) + ": per_call is 0 (\"normal\") or 1 (\"dango\")");
  for (int i = 0; i < n_cut; i++) {
    const int s = rects[3 * i] & CUT_SIZE_MASK, oy = rects[3 * i + 1], ox = rects[3 * i + 2];
    MAUA_REQUIRE(s > 0 && oy >= 0 && ox >= 0 && oy + s <= H && ox + s <= W, std::string(who) + ": a cutout leaves the image");
    MAUA_REQUIRE(per_call || (rects[3 * i] & ~CUT_SIZE_MASK) == 0, std::string(who) + ": \"normal\" cutouts carry no grey / flip flags");
  }
  n_rec = per_call ? 1 : n_cut;
  S = per_call ? cut_size : std::min(H, W);
  recs.resize((size_t)n_rec * aug_record_bytes());
  if (int rc = aug_records(augs, n_rec, per_call ? nullptr : rects, cut_size, &key, per_call ? 1 : n_cut, recs.data())) return rc;
  MAUA_REQUIRE(ctx, std::string(who) + ": ctx is NULL");
  return MAUA_OK;
}

int maua_cutouts_aug(maua_ctx* ctx, const float* img, int B, int H, int W, const int* rects, int n_cut, int cut_size, float mul, float add,
                     const float* mean3, const float* std3, const float* augs, unsigned long long key, int per_call, float* out) {
  MAUA_REQUIRE(img && rects && out && mean3 && std3 && augs, "maua_cutouts_aug: NULL argument");
  std::vector<char> recs;
  int n_rec = 0, S = 0;
  if (int rc = cutouts_aug_common(ctx, "maua_cutouts_aug", B, H, W, rects, n_cut, cut_size, augs, key, per_call, recs, n_rec, S)) return rc;
  char *base, *recd;   // base: the resize tables
  int* rd;
  float *x1, *x2;
  if (int rc = carve_scratch(ctx, [&](Scratch& s) {
        base = s.take<char>(cutouts_table_bytes(n_cut, cut_size)); rd = s.take<int>((size_t)n_cut * 6); recd = s.take<char>(recs.size());
        x1 = s.take<float>((size_t)n_cut * B * 3 * S * S); x2 = s.take<float>((size_t)n_cut * B * 3 * S * S);
      }))
    return rc;
  std::vector<int> slot((size_t)n_cut * 3);
  for (int i = 0; i < n_cut; i++) { slot[3 * i] = rects[3 * i] & CUT_SIZE_MASK; slot[3 * i + 1] = 0; slot[3 * i + 2] = 0; }
  MAUA_HIP_CHECK(hipMemcpyAsync(rd, rects, (size_t)n_cut * 12, hipMemcpyHostToDevice, ctx->stream));
  MAUA_HIP_CHECK(hipMemcpyAsync(rd + 3 * n_cut, slot.data(), (size_t)n_cut * 12, hipMemcpyHostToDevice, ctx->stream));
  MAUA_HIP_CHECK(hipMemcpyAsync(recd, recs.data(), recs.size(), hipMemcpyHostToDevice, ctx->stream));
  MAUA_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  const float zero3[3] = {0.f, 0.f, 0.f}, one3[3] = {1.f, 1.f, 1.f};
  CutoutPlan p{};
  p.B = B; p.n_cut = n_cut; p.cs = cut_size;
  if (!per_call) {   // crops -> augmented slots -> resize (Normalize at the end)
    if (int rc = aug_forward_src(ctx->stream, recd, n_rec, B, S, 0, img, H, W, mul, add, x1)) return rc;
    if (int rc = aug_forward_out(ctx->stream, MAUA_F32, recd, n_rec, B, S, 0, x1, x2, 0, zero3, one3)) return rc;
    p.img = x2; p.rects = rd + 3 * n_cut; p.H = S; p.W = S; p.mul = 1.f; p.add = 0.f; p.img_stride = (long)B * 3 * S * S;
    for (int c = 0; c < 3; c++) { p.mean[c] = mean3[c]; p.std[c] = std3[c]; }
    if (int rc = launch_cutout_tables(ctx->stream, p, base)) return rc;
    return launch_cutouts_forward(ctx->stream, MAUA_F32, p, base, out);
  }
  // resize -> one record over the whole batch (Normalize at the end)
  p.img = img; p.rects = rd; p.H = H; p.W = W; p.mul = mul; p.add = add;
  for (int c = 0; c < 3; c++) { p.mean[c] = 0.f; p.std[c] = 1.f; }
  if (int rc = launch_cutout_tables(ctx->stream, p, base)) return rc;
  if (int rc = launch_cutouts_forward(ctx->stream, MAUA_F32, p, base, x2)) return rc;
  if (int rc = aug_forward_src(ctx->stream, recd, 1, n_cut * B, S, 0, x2, S, S, 1.f, 0.f, x1)) return rc;
  return aug_forward_out(ctx->stream, MAUA_F32, recd, 1, n_cut * B, S, 0, x1, out, 0, mean3, std3);
}

int maua_cutouts_aug_vjp(maua_ctx* ctx, const float* d_out, int B, int H, int W, const int* rects, int n_cut, int cut_size, float mul,
                         const float* std3, const float* augs, int per_call, float* d_img) {
  MAUA_REQUIRE(d_out && rects && d_img && std3 && augs, "maua_cutouts_aug_vjp: NULL argument");
  std::vector<char> recs;
  int n_rec = 0, S = 0;
  if (int rc = cutouts_aug_common(ctx, "maua_cutouts_aug_vjp", B, H, W, rects, n_cut, cut_size, augs, 0ull, per_call, recs, n_rec, S)) return rc;
  char *base, *recd;   // base: the resize tables
  int* rd;
  float *x1, *x2, *th;
  if (int rc = carve_scratch(ctx, [&](Scratch& s) {
        base = s.take<char>(cutouts_table_bytes(n_cut, cut_size)); rd = s.take<int>((size_t)n_cut * 6); recd = s.take<char>(recs.size());
        x1 = s.take<float>((size_t)n_cut * B * 3 * S * S); x2 = s.take<float>((size_t)n_cut * B * 3 * S * S);
        th = (float*)s.take<char>(cutouts_th_bytes(n_cut, B, cut_size, per_call ? std::min(H, W) : S));
      }))
    return rc;
  std::vector<int> slot((size_t)n_cut * 3);
  for (int i = 0; i < n_cut; i++) { slot[3 * i] = rects[3 * i] & CUT_SIZE_MASK; slot[3 * i + 1] = 0; slot[3 * i + 2] = 0; }
  MAUA_HIP_CHECK(hipMemcpyAsync(rd, rects, (size_t)n_cut * 12, hipMemcpyHostToDevice, ctx->stream));
  MAUA_HIP_CHECK(hipMemcpyAsync(rd + 3 * n_cut, slot.data(), (size_t)n_cut * 12, hipMemcpyHostToDevice, ctx->stream));
  MAUA_HIP_CHECK(hipMemcpyAsync(recd, recs.data(), recs.size(), hipMemcpyHostToDevice, ctx->stream));
  MAUA_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  const float one3[3] = {1.f, 1.f, 1.f};
  CutoutPlan p{};
  p.B = B; p.n_cut = n_cut; p.cs = cut_size;
  if (!per_call) {   // resize VJP per slot -> augmentation adjoint -> sum over the cutouts into d_img
    p.rects = rd + 3 * n_cut; p.H = S; p.W = S; p.mul = 1.f; p.img_stride = (long)B * 3 * S * S;
    for (int c = 0; c < 3; c++) { p.mean[c] = 0.f; p.std[c] = std3[c]; }
    if (int rc = launch_cutout_tables(ctx->stream, p, base)) return rc;
    if (int rc = launch_cutouts_vjp(ctx->stream, MAUA_F32, p, base, d_out, th, x2, 0)) return rc;
    if (int rc = aug_adjoint_out(ctx->stream, MAUA_F32, recd, n_rec, B, S, x2, 0, one3, x1)) return rc;
    return aug_adjoint_src(ctx->stream, recd, n_rec, B, S, x1, H, W, mul, d_img, 0);
  }
  if (int rc = aug_adjoint_out(ctx->stream, MAUA_F32, recd, 1, n_cut * B, S, d_out, 0, std3, x2)) return rc;
  if (int rc = aug_adjoint_src(ctx->stream, recd, 1, n_cut * B, S, x2, S, S, 1.f, x1, 0)) return rc;
  p.rects = rd; p.H = H; p.W = W; p.mul = mul;
  for (int c = 0; c < 3; c++) { p.mean[c] = 0.f; p.std[c] = 1.f; }
  if (int rc = launch_cutout_tables(ctx->stream, p, base)) return rc;
  return launch_cutouts_vjp(ctx->stream, MAUA_F32, p, base, x1, th, d_img, 0);
}

}  // extern "C"
