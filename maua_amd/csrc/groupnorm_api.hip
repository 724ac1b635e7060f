// Descriptor entry points of the fused GroupNorm pass and its input gradient (maua_group_norm_check / _plan / _ex,
// maua_group_norm_vjp_check / _plan / _ex): one call of groupnorm.hip's launch_group_norm or groupnorm_vjp.hip's launch_group_norm_vjp
// - the launchers the diffusion UNet and the operator entry points go through - with every argument in the caller's hand: both
// sources of the virtual concatenation, the resampling mode and the raw second output, the scale-shift row stride, the producing
// convolution's piece sums, the kernel route, and for the gradient the forward's statistics as an operand.  For parity tests; no
// reference counterpart.
#include "common.h"
#include "internal.h"

namespace maua {
namespace {

GnArgs gn_args(const maua_gn_desc* d) {
  GnArgs a{};
  a.x0 = d->x0; a.C0 = d->C0; a.x1 = d->x1; a.C1 = d->C1; a.B = d->B; a.H = d->H; a.W = d->W; a.gamma = d->gamma; a.beta = d->beta;
  a.ss = d->ss; a.ss_ld = d->ss_ld; a.silu = d->silu; a.mode = d->mode; a.y = d->y; a.xr = d->xr;
  a.ps0 = d->ps0; a.rows0 = d->rows0; a.ps1 = d->ps1; a.rows1 = d->rows1; a.force_route = d->force_route;
  return a;
}

int gn_check(const maua_gn_desc* d, const GnArgs& a) {
  if (int rc = group_norm_check(d->dtype, a)) return rc;
  MAUA_REQUIRE(d->force_route == 0 || d->force_route == 1, "group_norm: force_route is 0 (as routed) or 1 (per-channel kernels)");
  MAUA_REQUIRE(((size_t)d->stats_out & 15) == 0, "group_norm: pointers and ss_ld must be whole 16-byte pieces");
  return MAUA_OK;
}

GnVjpArgs gn_vjp_args(const maua_gn_vjp_desc* d) {
  GnVjpArgs a{};
  a.x0 = d->x0; a.C0 = d->C0; a.x1 = d->x1; a.C1 = d->C1; a.stats = d->stats; a.gamma = d->gamma; a.beta = d->beta; a.ss = d->ss;
  a.ss_ld = d->ss_ld; a.silu = d->silu; a.mode = d->mode; a.dy = d->dy; a.dres = d->dres; a.add0 = d->add0; a.add1 = d->add1;
  a.dx0 = d->dx0; a.dx1 = d->dx1; a.B = d->B; a.H = d->H; a.W = d->W;
  return a;
}

}  // namespace
}  // namespace maua

using namespace maua;

extern "C" int maua_group_norm_check(const maua_gn_desc* d) {
  MAUA_REQUIRE(d, "maua_group_norm_check: desc is NULL");
  return gn_check(d, gn_args(d));
}

extern "C" int maua_group_norm_plan(const maua_gn_desc* d, int* route, int* RY, int* ppc, int* nchunk, int* stats_source) {
  MAUA_REQUIRE(d, "maua_group_norm_plan: desc is NULL");
  const GnArgs a = gn_args(d);
  if (int rc = gn_check(d, a)) return rc;
  const GnPlanInfo p = group_norm_plan(d->dtype, a);
  if (route) *route = p.route;
  if (RY) *RY = p.RY;
  if (ppc) *ppc = p.ppc;
  if (nchunk) *nchunk = p.nchunk;
  if (stats_source) *stats_source = p.stats_source;
  return MAUA_OK;
}

extern "C" int maua_group_norm_ex(maua_ctx* ctx, const maua_gn_desc* d) {
  MAUA_REQUIRE(ctx && d, "maua_group_norm_ex: NULL argument");
  const GnArgs a = gn_args(d);
  if (int rc = gn_check(d, a)) return rc;
  if (d->B == 0) return MAUA_OK;
  const size_t part_bytes = group_norm_workspace(d->B, d->C0 + d->C1, (long)d->H * d->W, elem_bytes(d->dtype));
  double* part;
  float* stats;
  if (int rc = carve_scratch(ctx, [&](Scratch& s) { part = (double*)s.take<char>(part_bytes); stats = s.take<float>((size_t)d->B * 64); })) return rc;
  return launch_group_norm(ctx->stream, d->dtype, a, part, d->stats_out ? d->stats_out : stats);
}

extern "C" int maua_group_norm_vjp_check(const maua_gn_vjp_desc* d) {
  MAUA_REQUIRE(d, "maua_group_norm_vjp_check: desc is NULL");
  return group_norm_vjp_check(d->dtype, gn_vjp_args(d));
}

extern "C" int maua_group_norm_vjp_plan(const maua_gn_vjp_desc* d, int* RY, int* ppc, int* nchunk, int* ranges) {
  MAUA_REQUIRE(d, "maua_group_norm_vjp_plan: desc is NULL");
  const GnVjpArgs a = gn_vjp_args(d);
  if (int rc = group_norm_vjp_check(d->dtype, a)) return rc;
  const GnVjpPlanInfo p = group_norm_vjp_plan(d->dtype, a);
  if (RY) *RY = p.RY;
  if (ppc) *ppc = p.ppc;
  if (nchunk) *nchunk = p.nchunk;
  if (ranges) *ranges = p.ranges;
  return MAUA_OK;
}

extern "C" int maua_group_norm_vjp_ex(maua_ctx* ctx, const maua_gn_vjp_desc* d) {
  MAUA_REQUIRE(ctx && d, "maua_group_norm_vjp_ex: NULL argument");
  const GnVjpArgs a = gn_vjp_args(d);
  if (int rc = group_norm_vjp_check(d->dtype, a)) return rc;
  if (d->B == 0) return MAUA_OK;
  const size_t ws_bytes = group_norm_vjp_workspace(d->B, d->C0 + d->C1, (long)d->H * d->W, elem_bytes(d->dtype));
  void* ws;
  if (int rc = carve_scratch(ctx, [&](Scratch& s) { ws = s.take<char>(ws_bytes); })) return rc;
  return launch_group_norm_vjp(ctx->stream, d->dtype, a, ws);
}

// ---- operator-level entry points (NHWC tensors in the network dtype) -----------------------------------------------------------
extern "C" {

// GroupNorm32(32, C) (+ optional per-sample scale-shift [B][2C]: y * (1 + scale) + shift) (+ SiLU) on NHWC x -> y
int maua_group_norm_nhwc(maua_ctx* ctx, const void* x, const float* gamma, const float* beta, const float* scale_shift,
                         int silu, int B, int H, int W, int C, int dtype, void* y) {
  MAUA_REQUIRE(ctx && x && gamma && beta && y, "maua_group_norm_nhwc: NULL argument");
  MAUA_REQUIRE(C % 32 == 0 && (dtype == MAUA_F32 || dtype == MAUA_BF16), "maua_group_norm_nhwc: C % 32, f32 / bf16");
  if (B == 0) return MAUA_OK;
  const size_t part_bytes = group_norm_workspace(B, C, (long)H * W, elem_bytes(dtype));
  double* part;
  float* stats;
  if (int rc = carve_scratch(ctx, [&](Scratch& s) { part = (double*)s.take<char>(part_bytes); stats = s.take<float>((size_t)B * 64); })) return rc;
  GnArgs a{};
  a.x0 = x; a.C0 = C; a.B = B; a.H = H; a.W = W; a.gamma = gamma; a.beta = beta; a.ss = scale_shift; a.ss_ld = 2L * C; a.silu = silu;
  a.y = y;
  return launch_group_norm(ctx->stream, dtype, a, part, stats);
}

// GroupNorm32 (+ scale-shift) (+ SiLU) (+ resample: 0 none, 1 2x2 average, 2 nearest x2 - behind the activation, as the
// ResBlocks' h_upd): dy [B][Ho][Wo][C] -> dx [B][H][W][C]; dres (optional, like dy): the gradient of the resampled raw x, added.
int maua_group_norm_nhwc_vjp(maua_ctx* ctx, const void* x, const float* gamma, const float* beta, const float* scale_shift, int silu,
                             int resample, const void* dy, const void* dres, int B, int H, int W, int C, int dtype, void* dx) {
  MAUA_REQUIRE(ctx && x && gamma && beta && dy && dx, "maua_group_norm_nhwc_vjp: NULL argument");
  MAUA_REQUIRE(C % 32 == 0 && (dtype == MAUA_F32 || dtype == MAUA_BF16), "maua_group_norm_nhwc_vjp: C % 32, f32 / bf16");
  if (B == 0) return MAUA_OK;
  const size_t part_bytes = group_norm_workspace(B, C, (long)H * W, elem_bytes(dtype));
  const size_t vjp_bytes = group_norm_vjp_workspace(B, C, (long)H * W, elem_bytes(dtype));
  double* part;
  float* stats;
  void* ws;
  if (int rc = carve_scratch(ctx, [&](Scratch& s) {
        part = (double*)s.take<char>(part_bytes); stats = s.take<float>((size_t)B * 64); ws = s.take<char>(vjp_bytes);
      }))
    return rc;
  // the forward's statistics (its output goes nowhere: the statistics passes only)
  if (int rc = launch_group_norm_stats(ctx->stream, dtype, x, C, B, H, W, part, stats)) return rc;
  GnVjpArgs a{};
  a.x0 = x; a.C0 = C; a.stats = stats; a.gamma = gamma; a.beta = beta; a.ss = scale_shift; a.ss_ld = 2L * C; a.silu = silu; a.mode = resample;
  a.dy = dy; a.dres = dres; a.dx0 = dx; a.B = B; a.H = H; a.W = W;
  return launch_group_norm_vjp(ctx->stream, dtype, a, ws);
}

}  // extern "C"
