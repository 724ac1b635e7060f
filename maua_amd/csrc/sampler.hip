// The samplers around the guided-diffusion UNet (unet.hip): the per-step arithmetic of DDIM / p_sample / PLMS as operators, and the
// two in-library DDIM loops (maua_ddim_sample_loop, maua_ddim_guided_loop) with their hipGraph capture.
//
// Replaces (reference): `diffusion.ddim_sample` / `p_sample` / `plms_sample` (gaussian_diffusion.py of the guided-diffusion submodule)
// as maua/diffusion/processors/guided.py:277-339 `GuidedDiffusion.forward` loops over them, with `cond_fn` =
// GradientGuidedConditioning (guided.py:236-272).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "common.h"
#include "internal.h"
#include "unet_internal.h"

using namespace maua;

namespace {

// ------------------------------------------------------------------------------------------------------ DDIM step
// The step kernels below evaluate the reference's float32 tensor expressions in its order, every product, sum and quotient rounded
// once: plain operators with contraction switched off in each body (the pragma is lexical).  __fmul_rn / __fadd_rn would not do: they
// are inline operators to this compiler and the back end fuses them (latent.hip found the same); (k0 x - pred) / k1 cancels, so one
// fused rounding is not small against the result.  expf in p_sample_step_kernel is the device library's: that sample is bounded, not exact.
//
// gaussian_diffusion.py ddim_sample for an epsilon-predicting model (clip_denoised False), in the reference's float32
// operation order; coefficients per sample: cf[b] = {sqrt_recip_ac, sqrt_recipm1_ac, sqrt(1 - ac), sqrt(ac_prev),
// sqrt(1 - ac_prev - sigma^2), sigma * nonzero_mask, 0, 0}.  model_out [B][Cm][HW] (eps = first C channels), x [B][C][HW].
__global__ __launch_bounds__(256) void ddim_step_kernel(const float* __restrict__ x, const float* __restrict__ model_out,
                                                        const float* __restrict__ grad, const float* __restrict__ noise,
                                                        const float* __restrict__ cf, int C, int Cm, long HW, long total,
                                                        float* __restrict__ sample, float* __restrict__ pred_out) {
#pragma clang fp contract(off)
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const long chw = (long)C * HW;
  const int b = (int)(idx / chw);
  const long rem = idx - (long)b * chw;
  const float* k = cf + b * 8;
  const float xv = x[idx];
  const float eps_m = model_out[(long)b * Cm * HW + rem];
  float pred = k[0] * xv - k[1] * eps_m;           // _predict_xstart_from_eps
  if (grad) {                                      // condition_score
    float eps = (k[0] * xv - pred) / k[1];
    eps = eps - k[2] * grad[idx];
    pred = k[0] * xv - k[1] * eps;
  }
  const float eps = (k[0] * xv - pred) / k[1];     // _predict_eps_from_xstart
  float s = pred * k[3] + k[4] * eps;
  if (noise) s += k[5] * noise[idx];
  sample[idx] = s;
  if (pred_out) pred_out[idx] = pred;
}

// gaussian_diffusion.py p_sample (ancestral step) for an epsilon model with learned-range variance (learn_sigma: the second half
// of the model's channels interpolates between the posterior and the beta log-variance), clip_denoised False, optional
// condition_mean.  cf[b] = {sqrt_recip_ac, sqrt_recipm1_ac, posterior_mean_coef1, posterior_mean_coef2,
// posterior_log_variance_clipped, log(beta), nonzero_mask, 0}.
__global__ __launch_bounds__(256) void p_sample_step_kernel(const float* __restrict__ x, const float* __restrict__ model_out,
                                                            const float* __restrict__ grad, const float* __restrict__ noise,
                                                            const float* __restrict__ cf, int C, long HW, long total,
                                                            float* __restrict__ sample, float* __restrict__ pred_out) {
#pragma clang fp contract(off)
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const long chw = (long)C * HW;
  const int b = (int)(idx / chw);
  const long rem = idx - (long)b * chw;
  const float* k = cf + b * 8;
  const float xv = x[idx];
  const float* mo = model_out + (long)b * 2 * chw;
  const float eps = mo[rem], vv = mo[chw + rem];
  const float frac = (vv + 1.f) / 2.f;
  const float logvar = frac * k[5] + (1.f - frac) * k[4];
  const float pred = k[0] * xv - k[1] * eps;                 // _predict_xstart_from_eps
  float mean = k[2] * pred + k[3] * xv;                      // q_posterior_mean_variance
  if (grad) mean = mean + expf(logvar) * grad[idx];          // condition_mean: mean + variance * gradient
  sample[idx] = mean + k[6] * expf(0.5f * logvar) * noise[idx];
  if (pred_out) pred_out[idx] = pred;
}

// One model evaluation of plms_sample (the pseudo linear multistep sampler of the guided-diffusion fork the reference
// vendors as a submodule): pred_orig = x0 from the network's epsilon; with a condition gradient the score is conditioned
// (condition_score) -> pred; eps = _predict_eps_from_xstart(x, t, pred).  cf[b] = maua_ddim_step's coefficients.
__global__ __launch_bounds__(256) void plms_eps_kernel(const float* __restrict__ x, const float* __restrict__ model_out,
                                                       const float* __restrict__ grad, const float* __restrict__ cf, int C,
                                                       int Cm, long HW, long total, float* __restrict__ eps_out,
                                                       float* __restrict__ pred_out, float* __restrict__ pred_orig_out) {
#pragma clang fp contract(off)
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const long chw = (long)C * HW;
  const int b = (int)(idx / chw);
  const long rem = idx - (long)b * chw;
  const float* k = cf + b * 8;
  const float xv = x[idx];
  const float eps_m = model_out[(long)b * Cm * HW + rem];
  const float pred_orig = k[0] * xv - k[1] * eps_m;
  float pred = pred_orig;
  if (grad) {
    float e = (k[0] * xv - pred) / k[1];
    e = e - k[2] * grad[idx];
    pred = k[0] * xv - k[1] * e;
  }
  eps_out[idx] = (k[0] * xv - pred) / k[1];
  if (pred_out) pred_out[idx] = pred;
  if (pred_orig_out) pred_orig_out[idx] = pred_orig;
}

// The multistep update: eps' = (sum_i w[i] * eps_i) / div (i < n: Adams-Bashforth weights, or (1, 1) / 2 for the improved-Euler start),
// pred' = _predict_xstart_from_eps(x, t, eps'), mean = pred' sqrt(ac_prev) + sqrt(1 - ac_prev) eps',
// sample = mean * nonzero + pred * (1 - nonzero).  cf[b] = {sqrt_recip_ac, sqrt_recipm1_ac, sqrt(ac_prev), sqrt(1 - ac_prev),
// nonzero_mask, 0, 0, 0}
struct PlmsEps { const float* e[4]; float w[4]; float div; int n; };
__global__ __launch_bounds__(256) void plms_update_kernel(const float* __restrict__ x, PlmsEps pe, const float* __restrict__ pred,
                                                          const float* __restrict__ cf, long chw, long total,
                                                          float* __restrict__ sample) {
#pragma clang fp contract(off)
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int b = (int)(idx / chw);
  const float* k = cf + b * 8;
  // (separately rounded products and sums, left to right, then the division: the order of the reference's expression - contraction is off)
  float ep = pe.w[0] * pe.e[0][idx];
  for (int i = 1; i < pe.n; i++) ep = ep + pe.w[i] * pe.e[i][idx];
  ep = ep / pe.div;
  const float pp = k[0] * x[idx] - k[1] * ep;
  const float mean = pp * k[2] + k[3] * ep;
  sample[idx] = mean * k[4] + pred[idx] * (1.f - k[4]);
}

// out = a[b] * x + c[b] * y (q_sample: sqrt(ac) * x_start + sqrt(1 - ac) * noise), per-sample coefficients
__global__ __launch_bounds__(256) void axpby_rows_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                         const float* __restrict__ ab, long row, long total,
                                                         float* __restrict__ out) {
#pragma clang fp contract(off)
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int b = (int)(idx / row);
  out[idx] = ab[2 * b] * x[idx] + ab[2 * b + 1] * y[idx];
}

// the image-MSE grad module of the guided sampler: g = (img - target) * k[b] (k = 2 scale / numel, one per sample; read from device
// memory so that a captured loop serves every scale), one target per sample or one for all (tstride 0); any NaN raises *flag
__global__ __launch_bounds__(256) void mse_guide_grad_kernel(const float* __restrict__ img, const float* __restrict__ target,
                                                             long tstride, const float* __restrict__ kdev, long row, long total,
                                                             float* __restrict__ out, int* __restrict__ flag) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  bool bad = false;
  if (idx < total) {
    const long b = idx / row, i = idx - b * row;
    const float v = (img[idx] - target[b * tstride + i]) * kdev[b];
    out[idx] = v;
    bad = v != v;
  }
  if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
}
// GradientGuidedConditioning.forward (guided.py:262-265): a grad module whose output holds a NaN contributes zeros
// eps = the first C channels of a model output [B][Cm][HW], made contiguous (speed "regular": pred_xstart is built from it with
// axpby_rows_kernel, exactly as the step-by-step path does - same kernel, same bits)
__global__ __launch_bounds__(256) void eps_rows_kernel(const float* __restrict__ model_out, long chw, long cmhw, long total,
                                                       float* __restrict__ eps) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const long b = i / chw;
  eps[i] = model_out[b * cmhw + (i - b * chw)];
}

__global__ __launch_bounds__(256) void zero_if_flag_kernel(float* __restrict__ g, long total, const int* __restrict__ flag) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  // (an agent-scope load: served by L2, where the previous launch's atomicOr landed - not by the scalar / vector L1)
  if (idx < total && __hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) g[idx] = 0.f;
}

// Captures n_steps calls of step(s, main, side) -> int into one executable: main is the private capture stream, side the stream of a
// parallel branch (NULL: none, the step gets main twice).  The step sets the context's stream itself (every launcher reads it); it is
// back on the caller's stream on every path out of here.  The caller has run its own eager warm-up: nothing that plans, allocates or
// sets a kernel attribute may happen in a captured step.  A capture or instantiation that fails leaves *exec NULL and raises *failed
// (the loop runs eagerly from then on, the capture is never tried again); only what fails before the capture begins is an error.
template <typename Step>
int capture_steps(maua_unet* n, const char* who, int n_steps, hipStream_t side, Step step, hipGraphExec_t* exec, int* failed) {
  hipStream_t st = n->ctx->stream;
  hipStream_t& cap = n->smp.cap_stream;
  if (*exec) { hipGraphExecDestroy(*exec); *exec = nullptr; }
  if (!cap) MAUA_HIP_CHECK(hipStreamCreateWithFlags(&cap, hipStreamNonBlocking));
  MAUA_HIP_CHECK(hipStreamSynchronize(st));
  hipGraph_t graph = nullptr;
  hipError_t e = hipStreamBeginCapture(cap, hipStreamCaptureModeThreadLocal);
  int rc = MAUA_OK;
  if (e == hipSuccess) {
    for (int s = 0; s < n_steps && !rc; s++) rc = step(s, cap, side ? side : cap);
    n->ctx->stream = st;
    e = hipStreamEndCapture(cap, &graph);
  }
  if (!rc && e == hipSuccess) e = hipGraphInstantiate(exec, graph, nullptr, nullptr, 0);
  if (graph) hipGraphDestroy(graph);
  if (rc || e != hipSuccess) {
    (void)hipGetLastError();  // clear the sticky error; run eagerly from now on
    *exec = nullptr;
    *failed = 1;
    if (getenv("MAUA_VERBOSE"))
      fprintf(stderr, "[maua] %s: graph capture unavailable (%s), running eagerly\n", who, rc ? maua_last_error() : hipGetErrorString(e));
  }
  return MAUA_OK;
}

}  // namespace

size_t maua::shape_key(int B, int H, int W) { return ((size_t)B << 40) ^ ((size_t)H << 20) ^ (size_t)W; }

// the captured sampler loops hold pointers into the arena / the per-step tables: whatever moves those drops both executables
void maua::drop_sampler_graphs(maua_unet* n) {
  maua_unet::SamplerState& sm = n->smp;
  if (sm.graph_exec) { hipGraphExecDestroy(sm.graph_exec); sm.graph_exec = nullptr; sm.graph_key = 0; }
  if (sm.gd_exec) { hipGraphExecDestroy(sm.gd_exec); sm.gd_exec = nullptr; sm.gd_key = 0; }
}

void maua_unet::SamplerState::release() {
  if (graph_exec) hipGraphExecDestroy(graph_exec);
  if (gd_exec) hipGraphExecDestroy(gd_exec);
  for (hipStream_t s : {cap_stream, side_stream, cap_side})
    if (s) hipStreamDestroy(s);
  for (hipEvent_t e : {ev_fork, ev_join})
    if (e) hipEventDestroy(e);
  *this = SamplerState();
}

extern "C" {

// 1 when the last maua_ddim_sample_loop(use_graph = 1) replayed a captured hipGraph, 0 when it ran eagerly
int maua_unet_graph_active(maua_unet* n, int* active) {
  MAUA_REQUIRE(n && active, "maua_unet_graph_active: NULL argument");
  *active = n->smp.graph_exec && !n->smp.graph_failed ? 1 : 0;
  return MAUA_OK;
}

// One DDIM update (gaussian_diffusion.py ddim_sample, epsilon model, clip_denoised False).  x [B][C][H][W], model_out
// [B][Cm][H][W] (Cm >= C: the learned-variance channels are not used by DDIM), cond_grad = cond_fn(x, t) or NULL, noise or
// NULL (eta = 0), coef: device f32 [B][8] = {sqrt_recip_alphas_cumprod, sqrt_recipm1_alphas_cumprod,
// sqrt(1 - alphas_cumprod), sqrt(alphas_cumprod_prev), sqrt(1 - alphas_cumprod_prev - sigma^2), sigma * (t != 0), 0, 0}.
int maua_ddim_step(maua_ctx* ctx, const float* x, const float* model_out, const float* cond_grad, const float* noise,
                   const float* coef, int B, int C, int Cm, long HW, float* sample, float* pred_xstart) {
  MAUA_REQUIRE(ctx, "maua_ddim_step: ctx is NULL");
  MAUA_REQUIRE(B >= 0 && HW >= 0, "maua_ddim_step: a negative size");
  if (B == 0 || HW == 0) return MAUA_OK;
  MAUA_REQUIRE(x && model_out && coef && sample && C > 0 && Cm >= C, "maua_ddim_step: NULL argument");
  const long total = (long)B * C * HW;
  hipLaunchKernelGGL(ddim_step_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, x, model_out,
                     cond_grad, noise, coef, C, Cm, HW, total, sample, pred_xstart);
  MAUA_HIP_CHECK(hipGetLastError());
  return MAUA_OK;
}

// One p_sample update (gaussian_diffusion.py p_sample + p_mean_variance with learned-range variance, epsilon model,
// clip_denoised False; cond_grad = cond_fn(x, t) or NULL: condition_mean).  model_out [B][2 C][H][W]; noise [B][C][H][W];
// coef: device f32 [B][8] = {sqrt_recip_alphas_cumprod, sqrt_recipm1_alphas_cumprod, posterior_mean_coef1, posterior_mean_coef2,
// posterior_log_variance_clipped, log(betas), t != 0, 0}.
int maua_p_sample_step(maua_ctx* ctx, const float* x, const float* model_out, const float* cond_grad, const float* noise,
                       const float* coef, int B, int C, long HW, float* sample, float* pred_xstart) {
  MAUA_REQUIRE(ctx, "maua_p_sample_step: ctx is NULL");
  MAUA_REQUIRE(B >= 0 && HW >= 0, "maua_p_sample_step: a negative size");
  if (B == 0 || HW == 0) return MAUA_OK;
  MAUA_REQUIRE(x && model_out && noise && coef && sample && C > 0, "maua_p_sample_step: NULL argument");
  const long total = (long)B * C * HW;
  hipLaunchKernelGGL(p_sample_step_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, x, model_out,
                     cond_grad, noise, coef, C, HW, total, sample, pred_xstart);
  MAUA_HIP_CHECK(hipGetLastError());
  return MAUA_OK;
}

// plms_sample's get_model_output: eps (after the optional condition_score), its pred_xstart and the unconditioned one.
// coef: maua_ddim_step's table.
int maua_plms_eps(maua_ctx* ctx, const float* x, const float* model_out, const float* cond_grad, const float* coef, int B,
                  int C, int Cm, long HW, float* eps, float* pred_xstart, float* pred_xstart_orig) {
  MAUA_REQUIRE(ctx, "maua_plms_eps: ctx is NULL");
  MAUA_REQUIRE(B >= 0 && HW >= 0, "maua_plms_eps: a negative size");
  if (B == 0 || HW == 0) return MAUA_OK;
  MAUA_REQUIRE(x && model_out && coef && eps && C > 0 && Cm >= C, "maua_plms_eps: NULL argument");
  const long total = (long)B * C * HW;
  hipLaunchKernelGGL(plms_eps_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, x, model_out,
                     cond_grad, coef, C, Cm, HW, total, eps, pred_xstart, pred_xstart_orig);
  MAUA_HIP_CHECK(hipGetLastError());
  return MAUA_OK;
}

// plms_sample's update from n_eps (1..4) epsilon tensors: eps' = (sum_i weights[i] eps_list[i]) / divisor, accumulated left to
// right like the reference's expressions ((3 e1 - e2) / 2, (23 e1 - 16 e2 + 5 e3) / 12, ...); coef: device f32 [B][8] = {sqrt_recip_ac, sqrt_recipm1_ac, sqrt(ac_prev),
// sqrt(1 - ac_prev), t != 0, 0, 0, 0}.
int maua_plms_update(maua_ctx* ctx, const float* x, const float* const* eps_list, const float* weights, int n_eps,
                     float divisor, const float* pred_xstart, const float* coef, int B, long chw, float* sample) {
  MAUA_REQUIRE(ctx, "maua_plms_update: ctx is NULL");
  MAUA_REQUIRE(B >= 0 && chw >= 0, "maua_plms_update: a negative size");
  if (B == 0 || chw == 0) return MAUA_OK;
  MAUA_REQUIRE(x && eps_list && weights && pred_xstart && coef && sample && n_eps >= 1 && n_eps <= 4, "maua_plms_update: bad argument");
  MAUA_REQUIRE(divisor != 0.f, "maua_plms_update: divisor is zero");
  PlmsEps pe{};
  pe.n = n_eps; pe.div = divisor;
  for (int i = 0; i < n_eps; i++) {
    MAUA_REQUIRE(eps_list[i], "maua_plms_update: NULL epsilon tensor");
    pe.e[i] = eps_list[i]; pe.w[i] = weights[i];
  }
  const long total = (long)B * chw;
  hipLaunchKernelGGL(plms_update_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, x, pe, pred_xstart,
                     coef, chw, total, sample);
  MAUA_HIP_CHECK(hipGetLastError());
  return MAUA_OK;
}

// out[b] = ab[b][0] * x[b] + ab[b][1] * y[b] over rows of `row` elements (q_sample, gaussian_diffusion.py)
int maua_axpby_rows(maua_ctx* ctx, const float* x, const float* y, const float* ab, int B, long row, float* out) {
  MAUA_REQUIRE(ctx, "maua_axpby_rows: ctx is NULL");
  MAUA_REQUIRE(B >= 0 && row >= 0, "maua_axpby_rows: a negative size");
  if (B == 0 || row == 0) return MAUA_OK;
  MAUA_REQUIRE(x && y && ab && out, "maua_axpby_rows: NULL argument");
  const long total = (long)B * row;
  hipLaunchKernelGGL(axpby_rows_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, x, y, ab, row,
                     total, out);
  MAUA_HIP_CHECK(hipGetLastError());
  return MAUA_OK;
}

// what both sampler loops need on the device before their first step: the timesteps [n_steps][B], the DDIM coefficients
// [n_steps][B][8], the model-output / pred_xstart buffers and every step's timestep projections (emb_table)
static int prepare_sampler(maua_unet* n, int B, int H, int W, const float* model_t, const float* coef, int n_steps) {
  hipStream_t st = n->ctx->stream;
  const long chw = (long)n->in_ch * H * W;
  // per-step constants on the device: timesteps [n_steps][B], coefficients [n_steps][B][8]
  if (n->smp.g_steps < n_steps * B || !n->smp.g_t) {
    MAUA_HIP_CHECK(hipStreamSynchronize(st));
    n->smp.g_steps = 0;
    drop_sampler_graphs(n);
    if (int rc = n->smp.g_t.alloc((size_t)n_steps * B * 4)) return rc;
    if (int rc = n->smp.g_cf.alloc((size_t)n_steps * B * 8 * 4)) return rc;
    n->smp.g_steps = n_steps * B;
  }
  {
    std::vector<float> ht((size_t)n_steps * B), hc((size_t)n_steps * B * 8);
    for (int s = 0; s < n_steps; s++)
      for (int b = 0; b < B; b++) {
        ht[(size_t)s * B + b] = model_t[s];
        memcpy(&hc[((size_t)s * B + b) * 8], coef + (size_t)s * 8, 32);
      }
    MAUA_HIP_CHECK(hipMemcpyAsync(n->smp.g_t.as<float>(), ht.data(), ht.size() * 4, hipMemcpyHostToDevice, st));
    MAUA_HIP_CHECK(hipMemcpyAsync(n->smp.g_cf.as<float>(), hc.data(), hc.size() * 4, hipMemcpyHostToDevice, st));
    MAUA_HIP_CHECK(hipStreamSynchronize(st));
  }
  const size_t out_bytes = (size_t)B * n->out_ch * H * W * 4, pred_bytes = (size_t)B * chw * 4;
  if (!n->smp.g_out || !n->smp.g_pred || n->smp.g_out.bytes() + n->smp.g_pred.bytes() < out_bytes + pred_bytes) {
    MAUA_HIP_CHECK(hipStreamSynchronize(st));
    drop_sampler_graphs(n);
    if (int rc = n->smp.g_out.alloc(out_bytes)) return rc;
    if (int rc = n->smp.g_pred.alloc(pred_bytes)) return rc;
  }
  // every step's timestep projections at once: the timesteps are known up front and shared by the samples, so the stacked
  // emb_layers GEMV (51 k x 1024 f32 weights at the 256^2 configuration) runs once per loop with n_steps rows instead of
  // once per step with B rows
  if (n->smp.emb_table_rows < (size_t)n_steps) {
    MAUA_HIP_CHECK(hipStreamSynchronize(st));
    n->smp.emb_table_rows = 0;
    drop_sampler_graphs(n);
    if (int rc = n->smp.emb_table.alloc((size_t)n_steps * n->emb_total * 4)) return rc;
    n->smp.emb_table_rows = n_steps;
  }
  {
    const int E = n->emb_dim, mc = n->mc;
    DevBuf tmp;
    if (int rc = tmp.alloc((size_t)n_steps * (1 + mc + 2 * E) * 4)) return rc;
    float *tt = tmp.as<float>(), *e0, *e1, *e2;
    e0 = tt + n_steps; e1 = e0 + (size_t)n_steps * mc; e2 = e1 + (size_t)n_steps * E;
    MAUA_HIP_CHECK(hipMemcpyAsync(tt, model_t, (size_t)n_steps * 4, hipMemcpyHostToDevice, st));
    if (int rc = unet_emb_rows(n, st, tt, n_steps, e0, e1, e2, n->smp.emb_table.as<float>())) return rc;
    MAUA_HIP_CHECK(hipStreamSynchronize(st));
  }
  return MAUA_OK;
}

// The unconditioned sampler loop inside the library: n_steps x (UNet forward + DDIM update), x updated in place.
// model_t: host f32 [n_steps] (the timestep the network sees at each step, same for every sample); coef: host f32
// [n_steps][8] (maua_ddim_step's coefficients).  use_graph: capture the whole loop in ONE hipGraph on first use for a
// (B, H, W, n_steps) and replay it afterwards (a forward is ~400 short launches: the graph removes the launch gaps).
// pred_xstart (optional) receives the last step's prediction.
int maua_ddim_sample_loop(maua_unet* n, float* x, int B, int H, int W, const float* model_t, const float* coef, int n_steps,
                          int use_graph, float* pred_xstart) {
  MAUA_REQUIRE(n && x && model_t && coef && n_steps > 0, "maua_ddim_sample_loop: NULL argument");
  if (B == 0) return MAUA_OK;
  hipStream_t st = n->ctx->stream;
  const long chw = (long)n->in_ch * H * W;
  const size_t key = shape_key(B, H, W) ^ ((size_t)n_steps << 52);
  if (int rc = prepare_sampler(n, B, H, W, model_t, coef, n_steps)) return rc;
  const size_t pred_bytes = (size_t)B * chw * 4;
  auto body = [&](int s) -> int {
    n->emb_row = n->smp.emb_table.as<float>() + (size_t)s * n->emb_total;
    int rc = maua_unet_forward(n, x, n->smp.g_t.as<float>() + (size_t)s * B, B, H, W, n->smp.g_out.as<float>());
    n->emb_row = nullptr;
    if (rc) return rc;
    return maua_ddim_step(n->ctx, x, n->smp.g_out.as<float>(), nullptr, nullptr, n->smp.g_cf.as<float>() + (size_t)s * B * 8, B, n->in_ch, n->out_ch,
                          (long)H * W, x, n->smp.g_pred.as<float>());
  };
  if (use_graph && !n->smp.graph_failed) {
    if (!n->smp.graph_exec || n->smp.graph_key != key || n->smp.g_x != x) {
      // one eager forward first: plans the arena, sets the kernels' attributes (nothing of that is capturable)
      // - on a scratch copy so that x is not advanced
      if (!unet_planned(n, B, H, W)) {
        DevBuf tmp;
        if (int rc = tmp.alloc(pred_bytes)) return rc;
        MAUA_HIP_CHECK(hipMemcpyAsync(tmp.get(), x, pred_bytes, hipMemcpyDeviceToDevice, st));
        int rc = maua_unet_forward(n, tmp.as<float>(), n->smp.g_t.as<float>(), B, H, W, n->smp.g_out.as<float>());
        hipStreamSynchronize(st);
        if (rc) return rc;
      }
      auto step = [&](int s, hipStream_t main, hipStream_t) -> int {
        n->ctx->stream = main;   // the launchers read the context's stream
        return body(s);
      };
      if (int rc = capture_steps(n, "ddim_sample_loop", n_steps, nullptr, step, &n->smp.graph_exec, &n->smp.graph_failed)) return rc;
      if (n->smp.graph_exec) {
        n->smp.graph_key = key;
        n->smp.g_x = x;
      }
    }
  }
  if (use_graph && n->smp.graph_exec && !n->smp.graph_failed) {
    MAUA_HIP_CHECK(hipGraphLaunch(n->smp.graph_exec, st));
  } else {
    for (int s = 0; s < n_steps; s++)
      if (int rc = body(s)) return rc;
  }
  if (pred_xstart) MAUA_HIP_CHECK(hipMemcpyAsync(pred_xstart, n->smp.g_pred.as<float>(), pred_bytes, hipMemcpyDeviceToDevice, st));
  return MAUA_OK;
}

// g = (img - target) * k over rows, zeros when any element is NaN (MSEGuide + the NaN rule of guided.py:262-265); k: device scalar
// (reset_flag = false: *flag was zeroed by the caller - the captured sampler loop keeps memset nodes out of its graph: replays of a
//  graph holding a 4-byte memset node were seen reading a non-zero flag after an eager run of the same calls, on ROCm 7.0.2)
static int mse_guide_grad(maua_ctx* ctx, const float* img, const float* target, long tstride, const float* kdev, int B, long row,
                          float* out, int* flag, bool reset_flag = true) {
  const long total = (long)B * row;
  if (reset_flag) MAUA_HIP_CHECK(hipMemsetAsync(flag, 0, 4, ctx->stream));
  hipLaunchKernelGGL(mse_guide_grad_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, img, target, tstride,
                     kdev, row, total, out, flag);
  hipLaunchKernelGGL(zero_if_flag_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, out, total, flag);
  MAUA_HIP_CHECK(hipGetLastError());
  return MAUA_OK;
}

// The image-MSE grad module as an operator: out = (img - target) * k, zeros if that holds a NaN.  img, out [B][row]; target [B][row]
// (target_bstride = row) or one row for all samples (0).
int maua_mse_guide_grad(maua_ctx* ctx, const float* img, const float* target, long target_bstride, float k, int B, long row, float* out) {
  MAUA_REQUIRE(ctx, "maua_mse_guide_grad: ctx is NULL");
  MAUA_REQUIRE(B >= 0 && row >= 0, "maua_mse_guide_grad: a negative size");
  if (B == 0 || row == 0) return MAUA_OK;
  MAUA_REQUIRE(img && target && out, "maua_mse_guide_grad: NULL argument");
  int* flag;
  float* kd;
  if (int rc = carve_scratch(ctx, [&](Scratch& s) { flag = s.take<int>(1); kd = s.take<float>(B); })) return rc;
  std::vector<float> hk((size_t)B, k);
  MAUA_HIP_CHECK(hipMemcpyAsync(kd, hk.data(), (size_t)B * 4, hipMemcpyHostToDevice, ctx->stream));
  MAUA_HIP_CHECK(hipStreamSynchronize(ctx->stream));   // (hk lives on this call's stack)
  return mse_guide_grad(ctx, img, target, target_bstride, kd, B, row, out, flag);
}

// configs[3] as BASELINE states it: the GUIDED DDIM loop inside the library, one hipGraph per shape.  Per step s (guided.py:302-311,
// 333-337 with cond_fn = GradientGuidedConditioning, speed "fast", :236-272, and the image-MSE grad module):
//   out  = unet(x, t_s)                                      pred = secondary(x, cos_t_s).pred          (:252-253)
//   img  = sigma_s pred + (1 - sigma_s) x                    g    = (img - target) k, zeros if NaN      (:254, :256-265)
//   grad = c0_s g + c1_s (dv/dx)^T g                         x, pred_xstart = ddim_step(x, out, grad)   (:266-268, ddim_sample)
// guide: host f32 [n_steps][5] = {cos_t, sigma, 1 - sigma, -(sigma a_c + 1 - sigma), sigma s_c} as GradientGuidedConditioning.forward
// evaluates them.  target: device [B][C][H][W] (target_bstride = C H W) or one image for all samples (0).  x is updated in place.
// sec == NULL: speed "regular" - out = forward_keep(x, t_s); eps = out[:, :C]; pred = ra x - rm eps; img, g as above;
// grad = c0_s g + c1_s (d eps / d x)^T g from maua_unet_vjp's walk; guide[s] = {-, sigma, 1 - sigma, -(sigma ra + 1 - sigma), sigma rm}.
int maua_ddim_guided_loop(maua_unet* n, maua_secondary* sec, float* x, int B, int H, int W, const float* model_t, const float* coef,
                          const float* guide, int n_steps, const float* target, long target_bstride, float mse_k, int use_graph,
                          float* pred_xstart) {
  MAUA_REQUIRE(n && x && model_t && coef && guide && n_steps > 0, "maua_ddim_guided_loop: NULL argument");
  // sec == NULL: speed "regular" (guided.py:214-218, 250-252) - the gradient goes through THIS network: a kept forward + its input
  // gradient per step, no secondary model
  const bool regular = sec == nullptr;
  if (regular) {
    MAUA_REQUIRE(n->vjp && n->conv_in.wt_t && n->conv_out.wt_t, "maua_ddim_guided_loop: speed \"regular\" needs option \"vjp\" = 1 before the weights are loaded");
    MAUA_REQUIRE(n->out_ch >= n->in_ch, "maua_ddim_guided_loop: the model output must hold an epsilon per image channel");
  } else {
    MAUA_REQUIRE(n->in_ch == 3, "maua_ddim_guided_loop: the secondary model guides 3-channel images");
    MAUA_REQUIRE(secondary_ctx(sec) == n->ctx, "maua_ddim_guided_loop: both networks must live on one context (one stream)");
  }
  const long chw = (long)n->in_ch * H * W;
  MAUA_REQUIRE(target_bstride == 0 || target_bstride == chw, "maua_ddim_guided_loop: target_bstride is 0 or C * H * W");
  if (B == 0) return MAUA_OK;
  hipStream_t st = n->ctx->stream;
  const size_t key = shape_key(B, H, W) ^ ((size_t)n_steps << 52) ^ ((size_t)(uintptr_t)sec << 1) ^ (target_bstride ? 1u : 0u) ^ (regular ? 2u : 0u);
  maua_clip* const clip = n->smp.gd_clip;
  if (clip) {
    MAUA_REQUIRE(clip_ctx(clip) == n->ctx, "maua_ddim_guided_loop: the image tower must live on the networks' context");
    MAUA_REQUIRE(n->smp.gd_rect_steps == n_steps, "maua_ddim_guided_loop: maua_unet_set_clip_guide was given another number of steps");
    MAUA_REQUIRE(n->in_ch == 3, "maua_ddim_guided_loop: CLIP guides 3-channel images");
    for (size_t i = 0; i < n->smp.gd_rects_host.size(); i += 3)
      MAUA_REQUIRE((n->smp.gd_rects_host[i] & CUT_SIZE_MASK) > 0 && n->smp.gd_rects_host[i + 1] >= 0 && n->smp.gd_rects_host[i + 2] >= 0 &&
                       n->smp.gd_rects_host[i + 1] + (n->smp.gd_rects_host[i] & CUT_SIZE_MASK) <= H &&
                       n->smp.gd_rects_host[i + 2] + (n->smp.gd_rects_host[i] & CUT_SIZE_MASK) <= W,
                   "maua_ddim_guided_loop: a cutout leaves the image");
    if (int rc = clip_prepare_guide(clip, B, H, W, n->smp.gd_cutn)) return rc;
  } else if (n->smp.gd_guides.empty()) {
    MAUA_REQUIRE(target, "maua_ddim_guided_loop: target is NULL");
  }
  const bool guides = !n->smp.gd_guides.empty();
  if (guides) {
    MAUA_REQUIRE(n->in_ch == 3, "maua_ddim_guided_loop: the grad modules guide 3-channel images");
    for (maua_guide* g : n->smp.gd_guides) {
      MAUA_REQUIRE(guide_ctx(g) == n->ctx, "maua_ddim_guided_loop: a grad module lives on another context");
      if (int rc = guide_prepare(g, B, H, W)) return rc;
    }
  }
  if (int rc = prepare_sampler(n, B, H, W, model_t, coef, n_steps)) return rc;
  const size_t tb = (size_t)B * chw, tab = (size_t)n_steps * B * 7 + B;
  if (n->smp.gd_cap < 10 * tb || n->smp.gd_tab_cap < tab || !n->smp.gd_flag || n->smp.gd_flags < n_steps) {
    MAUA_HIP_CHECK(hipStreamSynchronize(st));
    n->smp.gd_cap = n->smp.gd_tab_cap = 0; n->smp.gd_flags = 0;
    drop_sampler_graphs(n);
    auto layout = [&](Scratch& s) {
      n->smp.gd_buf = s.take<float>(10 * tb); n->smp.gd_tab = s.take<float>(tab); n->smp.gd_flag = s.take<int>((size_t)n_steps);
    };
    if (int rc = carve_into(n->smp.gd_ws, layout)) return rc;
    n->smp.gd_cap = 10 * tb; n->smp.gd_tab_cap = tab; n->smp.gd_flags = n_steps;
  }
  float *bx = n->smp.gd_buf, *bv = bx + tb, *bp = bv + tb, *be = bp + tb, *bimg = be + tb, *bg = bimg + tb, *bjv = bg + tb,
        *bgrad = bjv + tb, *btgt = bgrad + tb, *bsub = btgt + tb;
  float *t_ct = n->smp.gd_tab, *t_img = t_ct + (size_t)n_steps * B, *t_grad = t_img + (size_t)n_steps * B * 2,
        *t_pred = t_grad + (size_t)n_steps * B * 2, *t_k = t_pred + (size_t)n_steps * B * 2;
  {
    std::vector<float> h(tab);
    for (int s = 0; s < n_steps; s++)
      for (int b = 0; b < B; b++) {
        const float* gs = guide + (size_t)s * 5;
        h[(size_t)s * B + b] = gs[0];
        h[(size_t)n_steps * B + ((size_t)s * B + b) * 2] = gs[1];
        h[(size_t)n_steps * B + ((size_t)s * B + b) * 2 + 1] = gs[2];
        h[(size_t)n_steps * B * 3 + ((size_t)s * B + b) * 2] = gs[3];
        h[(size_t)n_steps * B * 3 + ((size_t)s * B + b) * 2 + 1] = gs[4];
        h[(size_t)n_steps * B * 5 + ((size_t)s * B + b) * 2] = coef[(size_t)s * 8];        // (ra, -rm): pred_xstart from eps (regular)
        h[(size_t)n_steps * B * 5 + ((size_t)s * B + b) * 2 + 1] = -coef[(size_t)s * 8 + 1];
      }
    for (int b = 0; b < B; b++) h[(size_t)n_steps * B * 7 + b] = mse_k;
    MAUA_HIP_CHECK(hipMemcpyAsync(n->smp.gd_tab, h.data(), tab * 4, hipMemcpyHostToDevice, st));
    MAUA_HIP_CHECK(hipStreamSynchronize(st));
  }
  MAUA_HIP_CHECK(hipMemsetAsync(n->smp.gd_flag, 0, (size_t)n_steps * 4, st));
  MAUA_HIP_CHECK(hipMemcpyAsync(bx, x, tb * 4, hipMemcpyDeviceToDevice, st));
  if (!clip && !guides) MAUA_HIP_CHECK(hipMemcpyAsync(btgt, target, (target_bstride ? tb : (size_t)chw) * 4, hipMemcpyDeviceToDevice, st));
  // the grad module(s) of step s on the context's current stream: bimg -> bg
  auto guide_grad = [&](int s) -> int {
    int rc = MAUA_OK;
    if (clip)
      rc = clip_guide_grad(clip, bimg, B, H, W, n->smp.gd_rects.as<int>() + (size_t)s * n->smp.gd_batches * n->smp.gd_cutn * 3,
                           n->smp.gd_mult ? n->smp.gd_mult + (size_t)s * n->smp.gd_batches * n->smp.gd_cutn : nullptr, n->smp.gd_cutn, n->smp.gd_cutn_total,
                           n->smp.gd_batches, n->smp.gd_clip_scale, n->smp.gd_clip_clamp, bg);
    else if (!guides)
      return mse_guide_grad(n->ctx, bimg, btgt, target_bstride ? chw : 0, t_k, B, chw, bg, n->smp.gd_flag + s, false);
    // guided.py:258-266: img_grad += sub_grad per module, a module whose gradient holds a NaN skipped
    for (size_t k = 0; k < n->smp.gd_guides.size() && !rc; k++) {
      rc = guide_eval(n->smp.gd_guides[k], bimg, B, H, W, bsub);
      if (!rc) rc = screened_accumulate(n->ctx->stream, bsub, bg, (long)tb, !clip && k == 0, n->smp.gd_gflag.as<int>());
    }
    return rc;
  };
  if (n->smp.gd_fork && !n->smp.ev_fork) {
    MAUA_HIP_CHECK(hipEventCreateWithFlags(&n->smp.ev_fork, hipEventDisableTiming));
    MAUA_HIP_CHECK(hipEventCreateWithFlags(&n->smp.ev_join, hipEventDisableTiming));
    MAUA_HIP_CHECK(hipStreamCreateWithFlags(&n->smp.side_stream, hipStreamNonBlocking));
    MAUA_HIP_CHECK(hipStreamCreateWithFlags(&n->smp.cap_side, hipStreamNonBlocking));
  }
  // one step on (main, side): the UNet forward on main; the guidance branch - it reads x and nothing the forward writes - on side
  // (main itself when the fork is off); the DDIM update on main behind both.  Every launcher reads the context's stream.
  // speed "regular": no parallel branch (the gradient needs the forward it differentiates); everything on `main`
  auto step_regular = [&](int s, hipStream_t main) -> int {
    n->ctx->stream = main;
    n->emb_row = n->smp.emb_table.as<float>() + (size_t)s * n->emb_total;
    int rc = unet_forward(n, bx, n->smp.g_t.as<float>() + (size_t)s * B, B, H, W, n->smp.g_out.as<float>(), true);
    if (!rc) {
      // pred_xstart = ra x - rm eps (gaussian_diffusion.py _predict_xstart_from_eps), img = sigma pred + (1 - sigma) x (:252)
      const long total = (long)B * chw;
      hipLaunchKernelGGL(eps_rows_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, main, n->smp.g_out.as<float>(), chw, (long)n->out_ch * H * W,
                         total, be);
      if (hipGetLastError() != hipSuccess) rc = fail("maua_ddim_guided_loop: launch failed");
      if (!rc) rc = maua_axpby_rows(n->ctx, bx, be, t_pred + (size_t)s * B * 2, B, chw, bp);
      if (!rc) rc = maua_axpby_rows(n->ctx, bp, bx, t_img + (size_t)s * B * 2, B, chw, bimg);
    }
    if (!rc) rc = guide_grad(s);
    if (!rc) rc = unet_vjp(n, bg, bjv, n->in_ch);
    n->emb_row = nullptr;
    if (!rc) rc = maua_axpby_rows(n->ctx, bg, bjv, t_grad + (size_t)s * B * 2, B, chw, bgrad);
    if (rc) return rc;
    return maua_ddim_step(n->ctx, bx, n->smp.g_out.as<float>(), bgrad, nullptr, n->smp.g_cf.as<float>() + (size_t)s * B * 8, B, n->in_ch, n->out_ch, (long)H * W, bx,
                          n->smp.g_pred.as<float>());
  };
  auto step_on = [&](int s, hipStream_t main, hipStream_t side) -> int {
    if (regular) return step_regular(s, main);
    const bool fork = side != main;
    if (fork) {
      MAUA_HIP_CHECK(hipEventRecord(n->smp.ev_fork, main));
      MAUA_HIP_CHECK(hipStreamWaitEvent(side, n->smp.ev_fork, 0));
    }
    n->ctx->stream = main;
    n->emb_row = n->smp.emb_table.as<float>() + (size_t)s * n->emb_total;
    int rc = maua_unet_forward(n, bx, n->smp.g_t.as<float>() + (size_t)s * B, B, H, W, n->smp.g_out.as<float>());
    n->emb_row = nullptr;
    if (!rc) {
      n->ctx->stream = side;
      rc = maua_secondary_forward(sec, bx, t_ct + (size_t)s * B, B, H, W, bv, bp, be);
      if (!rc) rc = maua_axpby_rows(n->ctx, bp, bx, t_img + (size_t)s * B * 2, B, chw, bimg);
      if (!rc) rc = guide_grad(s);
      if (!rc) rc = maua_secondary_vjp(sec, bg, B, H, W, bjv);
      if (!rc) rc = maua_axpby_rows(n->ctx, bg, bjv, t_grad + (size_t)s * B * 2, B, chw, bgrad);
    }
    n->ctx->stream = main;
    if (fork) {   // (joined whatever happened: a capture must not end with an unjoined stream)
      hipError_t e1 = hipEventRecord(n->smp.ev_join, side), e2 = hipStreamWaitEvent(main, n->smp.ev_join, 0);
      if (!rc && (e1 != hipSuccess || e2 != hipSuccess)) rc = fail("maua_ddim_guided_loop: joining the guidance branch failed");
    }
    if (rc) return rc;
    return maua_ddim_step(n->ctx, bx, n->smp.g_out.as<float>(), bgrad, nullptr, n->smp.g_cf.as<float>() + (size_t)s * B * 8, B, n->in_ch, n->out_ch, (long)H * W, bx,
                          n->smp.g_pred.as<float>());
  };
  auto body = [&](int s) -> int {   // eager: on the caller's stream (+ the side stream)
    int rc = step_on(s, st, n->smp.gd_fork ? n->smp.side_stream : st);
    n->ctx->stream = st;
    return rc;
  };
  // the captured graph holds raw pointers into the secondary model's weights and workspaces: it is this model's, at this generation
  // of its buffers, or it is recaptured (the address alone does not identify a model: a freed one's can be handed out again)
  unsigned long long sec_uid = 0, sec_epoch = 0;
  unsigned long long clip_uid = 0, clip_ep = 0;
  auto sec_matches = [&]() {
    secondary_stamp(sec, &sec_uid, &sec_epoch);
    clip_stamp(clip, &clip_uid, &clip_ep);
    bool guides_same = n->smp.gd_guide_epochs.size() == n->smp.gd_guides.size();
    for (size_t k = 0; guides_same && k < n->smp.gd_guides.size(); k++) guides_same = guide_epoch(n->smp.gd_guides[k]) == n->smp.gd_guide_epochs[k];
    return sec_uid == n->smp.gd_sec_uid && sec_epoch == n->smp.gd_sec_epoch && clip_uid == n->smp.gd_clip_uid && clip_ep == n->smp.gd_clip_epoch &&
           n->smp.gd_guide_gen == n->smp.gd_guide_gen_seen && guides_same;
  };
  if (use_graph && !n->smp.gd_failed) {
    if (!n->smp.gd_exec || n->smp.gd_key != key || !sec_matches()) {
      // one eager step on scratch copies first: it plans both networks' workspaces and sets the kernels' attributes (none of that
      // can be captured); bx is restored afterwards
      {
        int rc = body(0);
        if (rc) return rc;
        MAUA_HIP_CHECK(hipMemcpyAsync(bx, x, tb * 4, hipMemcpyDeviceToDevice, st));
        MAUA_HIP_CHECK(hipMemsetAsync(n->smp.gd_flag, 0, (size_t)n_steps * 4, st));
      }
      if (int rc = capture_steps(n, "ddim_guided_loop", n_steps, n->smp.gd_fork ? n->smp.cap_side : nullptr, step_on, &n->smp.gd_exec,
                                 &n->smp.gd_failed))
        return rc;
      if (n->smp.gd_exec) {
        n->smp.gd_key = key;
        secondary_stamp(sec, &n->smp.gd_sec_uid, &n->smp.gd_sec_epoch);   // (after the eager step: that is what sized the workspaces)
        clip_stamp(clip, &n->smp.gd_clip_uid, &n->smp.gd_clip_epoch);
        n->smp.gd_guide_gen_seen = n->smp.gd_guide_gen;
        n->smp.gd_guide_epochs.clear();
        for (maua_guide* g : n->smp.gd_guides) n->smp.gd_guide_epochs.push_back(guide_epoch(g));
      }
    }
  }
  if (use_graph && n->smp.gd_exec && !n->smp.gd_failed) {
    // (the copies / memset above are stream-ordered before the graph anyway; one host wait per 100-step loop costs nothing and keeps
    //  the replay independent of how the runtime orders copy engines against graph launches)
    MAUA_HIP_CHECK(hipStreamSynchronize(st));
    MAUA_HIP_CHECK(hipGraphLaunch(n->smp.gd_exec, st));
    n->smp.gd_last_graph = 1;
  } else {
    n->smp.gd_last_graph = 0;
    for (int s = 0; s < n_steps; s++)
      if (int rc = body(s)) return rc;
  }
  MAUA_HIP_CHECK(hipMemcpyAsync(x, bx, tb * 4, hipMemcpyDeviceToDevice, st));
  if (pred_xstart) MAUA_HIP_CHECK(hipMemcpyAsync(pred_xstart, n->smp.g_pred.as<float>(), tb * 4, hipMemcpyDeviceToDevice, st));
  return MAUA_OK;
}

// CLIPGrads as the guided loop's grad module (maua/grad.py:96-165 in place of the image-MSE module); rects: host [n_steps][batches][cutn][3]
int maua_unet_set_clip_guide(maua_unet* n, maua_clip* clip, const int* rects, const float* mult, int n_steps, int cutn, int batches,
                             float scale, float clamp_gradient) {
  MAUA_REQUIRE(n, "maua_unet_set_clip_guide: net is NULL");
  if (!clip) {
    if (n->smp.gd_clip) n->smp.gd_guide_gen++;
    n->smp.gd_clip = nullptr;
    return MAUA_OK;
  }
  MAUA_REQUIRE(rects && n_steps > 0 && cutn > 0 && batches > 0, "maua_unet_set_clip_guide: bad arguments");
  hipStream_t st = n->ctx->stream;
  const size_t per = (size_t)n_steps * batches * cutn, cnt = per * 4;   // 3 ints + 1 float per cutout
  int cutn_total = cutn;
  if (mult) {
    for (size_t b = 0; b < (size_t)n_steps * batches; b++) {
      double t = 0;
      for (int i = 0; i < cutn; i++) t += mult[b * cutn + i];
      if (b == 0) cutn_total = (int)(t + 0.5);
      MAUA_REQUIRE((int)(t + 0.5) == cutn_total && cutn_total >= cutn,
                   "maua_unet_set_clip_guide: every cutout batch must stand for the same number (>= cutn) of cutouts");
    }
  }
  if (cnt * 4 > n->smp.gd_rects.bytes()) {
    MAUA_HIP_CHECK(hipStreamSynchronize(st));
    n->smp.gd_guide_gen++;
    if (int rc = n->smp.gd_rects.alloc(cnt * 4)) return rc;
  }
  float* mult_dev = mult ? (float*)(n->smp.gd_rects.as<int>() + per * 3) : nullptr;
  // (everything a captured loop bakes into its launches moves the generation; the rectangles themselves are data it reads)
  if (n->smp.gd_clip != clip || n->smp.gd_rect_steps != n_steps || n->smp.gd_cutn != cutn || n->smp.gd_batches != batches || n->smp.gd_clip_scale != scale ||
      n->smp.gd_clip_clamp != clamp_gradient || n->smp.gd_mult != mult_dev || n->smp.gd_cutn_total != cutn_total)
    n->smp.gd_guide_gen++;
  n->smp.gd_rects_host.assign(rects, rects + per * 3);
  MAUA_HIP_CHECK(hipMemcpyAsync(n->smp.gd_rects.as<int>(), n->smp.gd_rects_host.data(), per * 12, hipMemcpyHostToDevice, st));
  if (mult) MAUA_HIP_CHECK(hipMemcpyAsync(mult_dev, mult, per * 4, hipMemcpyHostToDevice, st));
  MAUA_HIP_CHECK(hipStreamSynchronize(st));
  n->smp.gd_clip = clip; n->smp.gd_rect_steps = n_steps; n->smp.gd_cutn = cutn; n->smp.gd_batches = batches; n->smp.gd_clip_scale = scale;
  n->smp.gd_clip_clamp = clamp_gradient; n->smp.gd_mult = mult_dev; n->smp.gd_cutn_total = cutn_total;
  return MAUA_OK;
}

// a list of grad modules (guides.hip) as the guided loop's conditioning: evaluated after CLIPGrads (if set) and summed
int maua_unet_set_guides(maua_unet* n, maua_guide* const* guides, int n_guides) {
  MAUA_REQUIRE(n && n_guides >= 0 && (n_guides == 0 || guides), "maua_unet_set_guides: bad arguments");
  std::vector<unsigned long long> uids;
  for (int k = 0; k < n_guides; k++) {
    MAUA_REQUIRE(guides[k], "maua_unet_set_guides: NULL guide");
    uids.push_back(guide_uid(guides[k]));
  }
  if (uids != n->smp.gd_guide_uids) n->smp.gd_guide_gen++;   // (a captured loop bakes the list into its launches)
  n->smp.gd_guide_uids = uids;
  n->smp.gd_guides.assign(guides, guides + n_guides);
  if (n_guides && !n->smp.gd_gflag)
    if (int rc = n->smp.gd_gflag.alloc(256)) return rc;
  return MAUA_OK;
}

// 1 when the last maua_ddim_guided_loop(use_graph = 1) replayed a captured hipGraph
int maua_unet_guided_graph_active(maua_unet* n, int* active) {
  MAUA_REQUIRE(n && active, "maua_unet_guided_graph_active: NULL argument");
  *active = n->smp.gd_exec && !n->smp.gd_failed && n->smp.gd_last_graph ? 1 : 0;
  return MAUA_OK;
}

}  // extern "C"
