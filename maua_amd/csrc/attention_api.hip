// Descriptor entry points of the fused attention kernels (maua_attention_check / _ex, maua_attention_vjp_check / _ex): one launch of
// attention.hip or attention_vjp.hip with every argument of the launcher in the caller's hand - row strides, the softmax scale, the
// causal flag, the log-sum-exp rows, and for the gradient the forward's result and log-sum-exp as operands (so a test can hand it the
// kernel's own or a reference's).  For parity tests; no reference counterpart.  The networks and the operator entry points at the end
// of this file fill AttnArgs / AttnVjpArgs themselves.
#include <cmath>

#include "common.h"
#include "internal.h"

namespace maua {
namespace {

AttnArgs attn_args(const maua_attn_desc* d) {
  AttnArgs a{};
  a.qkv = d->qkv; a.out = d->out; a.lse = d->lse; a.B = d->B; a.T = d->T; a.heads = d->heads; a.D = d->head_ch;
  a.ld_qkv = d->ld_qkv; a.ld_out = d->ld_out; a.scale = d->scale; a.causal = d->causal;
  return a;
}

AttnVjpArgs attn_vjp_args(const maua_attn_vjp_desc* d) {
  AttnVjpArgs a{};
  a.qkv = d->qkv; a.out = d->out; a.d_out = d->d_out; a.lse = d->lse; a.d_qkv = d->d_qkv; a.delta = d->delta;
  a.B = d->B; a.T = d->T; a.heads = d->heads; a.D = d->head_ch; a.ld_qkv = d->ld_qkv; a.ld_out = d->ld_out; a.scale = d->scale;
  a.causal = d->causal;
  return a;
}

}  // namespace
}  // namespace maua

using namespace maua;

extern "C" int maua_attention_check(const maua_attn_desc* d) {
  MAUA_REQUIRE(d, "maua_attention_check: desc is NULL");
  return attention_check(d->dtype, attn_args(d));
}

extern "C" int maua_attention_ex(maua_ctx* ctx, const maua_attn_desc* d) {
  MAUA_REQUIRE(ctx && d, "maua_attention_ex: NULL argument");
  return launch_attention(ctx->stream, d->dtype, attn_args(d));
}

extern "C" int maua_attention_vjp_check(const maua_attn_vjp_desc* d) {
  MAUA_REQUIRE(d, "maua_attention_vjp_check: desc is NULL");
  return attention_vjp_check(d->dtype, attn_vjp_args(d));
}

extern "C" int maua_attention_vjp_ex(maua_ctx* ctx, const maua_attn_vjp_desc* d) {
  MAUA_REQUIRE(ctx && d, "maua_attention_vjp_ex: NULL argument");
  return launch_attention_vjp(ctx->stream, d->dtype, attn_vjp_args(d));
}

// ---- operator-level entry points (NHWC tensors in the network dtype) -----------------------------------------------------------
extern "C" {

// QKVAttentionLegacy.forward: qkv [B][T][3 * heads * head_ch] (channel = head * 3 ch + {q, k, v} * ch + c) -> out [B][T][heads * ch]
int maua_attention_legacy(maua_ctx* ctx, const void* qkv, void* out, int B, int T, int heads, int head_ch, int dtype) {
  MAUA_REQUIRE(ctx, "maua_attention_legacy: ctx is NULL");
  AttnArgs a{};
  a.qkv = qkv; a.out = out; a.B = B; a.T = T; a.heads = heads; a.D = head_ch; a.ld_qkv = 3L * heads * head_ch;
  a.ld_out = (long)heads * head_ch; a.scale = 1.f / sqrtf((float)head_ch);
  return launch_attention(ctx->stream, dtype, a);
}

// the same with CLIP's causal mask (text tower): query t attends to keys 0 .. t
int maua_attention_causal(maua_ctx* ctx, const void* qkv, void* out, int B, int T, int heads, int head_ch, int dtype) {
  MAUA_REQUIRE(ctx, "maua_attention_causal: ctx is NULL");
  AttnArgs a{};
  a.qkv = qkv; a.out = out; a.B = B; a.T = T; a.heads = heads; a.D = head_ch; a.ld_qkv = 3L * heads * head_ch;
  a.ld_out = (long)heads * head_ch; a.scale = 1.f / sqrtf((float)head_ch); a.causal = 1;
  return launch_attention(ctx->stream, dtype, a);
}

// Input gradient of maua_attention_legacy (what maua_unet_vjp walks a network with): qkv as the forward's, d_out [B][T][C] -> d_qkv
// [B][T][3C] (the forward is re-run here for the rows' log-sum-exp and the result).
int maua_attention_legacy_vjp(maua_ctx* ctx, const void* qkv, const void* d_out, void* d_qkv, int B, int T, int heads, int head_ch,
                              int dtype) {
  MAUA_REQUIRE(ctx && qkv && d_out && d_qkv, "maua_attention_legacy_vjp: NULL argument");
  MAUA_REQUIRE(dtype == MAUA_F32 || dtype == MAUA_BF16, "maua_attention_legacy_vjp: f32 / bf16");
  if (B == 0) return MAUA_OK;
  char* ws;
  float *lse, *delta;
  if (int rc = carve_scratch(ctx, [&](Scratch& s) {
        ws = s.take<char>((size_t)B * T * heads * head_ch * elem_bytes(dtype));
        lse = s.take<float>((size_t)B * heads * T); delta = s.take<float>((size_t)B * heads * T);
      }))
    return rc;
  AttnArgs f{};
  f.qkv = qkv; f.out = ws; f.B = B; f.T = T; f.heads = heads; f.D = head_ch; f.ld_qkv = 3L * heads * head_ch;
  f.ld_out = (long)heads * head_ch; f.scale = 1.f / sqrtf((float)head_ch); f.lse = lse;
  if (int rc = launch_attention(ctx->stream, dtype, f)) return rc;
  AttnVjpArgs a{};
  a.qkv = qkv; a.out = ws; a.d_out = d_out; a.lse = f.lse; a.d_qkv = d_qkv; a.delta = delta; a.B = B; a.T = T;
  a.heads = heads; a.D = head_ch; a.ld_qkv = f.ld_qkv; a.ld_out = f.ld_out; a.scale = f.scale;
  return launch_attention_vjp(ctx->stream, dtype, a);
}

}  // extern "C"
