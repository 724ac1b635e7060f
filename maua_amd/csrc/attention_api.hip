// Descriptor entry points of the fused attention kernels (maua_attention_check / _ex, maua_attention_vjp_check / _ex): one launch of
// attention.hip or attention_vjp.hip with every argument of the launcher in the caller's hand - row strides, the softmax scale, the
// causal flag, the log-sum-exp rows, and for the gradient the forward's result and log-sum-exp as operands (so a test can hand it the
// kernel's own or a reference's).  For parity tests; no reference counterpart.  The networks and the operator entry points of unet.hip
// fill AttnArgs / AttnVjpArgs themselves.
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
