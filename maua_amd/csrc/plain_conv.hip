// Host-side plumbing of the plain-convolution networks (plain_conv.h): weight staging and preparation, the per-layer record, the
// unit styles.  Nothing here knows which network calls it: padding rules, parameter names and size checks stay with the callers.
#include <algorithm>

#include "internal.h"
#include "plain_conv.h"

namespace maua {

int stage(DevBuf& tmp, const float* src, size_t count, hipMemcpyKind kind) {
  if (int rc = tmp.alloc(count * 4)) return rc;
  MAUA_HIP_CHECK(hipMemcpy(tmp.get(), src, count * 4, kind));
  return MAUA_OK;
}

int load_weight(hipStream_t st, int dtype, const float* host, int Co, int Ci, int k, int Cop, int Cip, void* wt, void* wt_t, bool split) {
  const size_t count = (size_t)Co * Ci * k * k;
  const size_t elems = prepped_weight_elems(k, 1, Cop, Cip), bytes = elems * elem_bytes(dtype);
  DevBuf w, w_t;
  if (int rc = stage(w, host, count)) return rc;
  auto prep = [&]() -> int {
    MAUA_HIP_CHECK(hipMemsetAsync(wt, 0, bytes, st));   // (padded channels stay zero)
    if (int rc = launch_prep_weights(st, dtype, w.as<float>(), wt, nullptr, Co, Ci, k, 1, 0, Cop, Cip)) return rc;
    if (wt_t) {
      if (int rc = w_t.alloc(count * 4)) return rc;
      if (int rc = launch_transpose_flip(st, w.as<float>(), w_t.as<float>(), Co, Ci, k * k)) return rc;
      MAUA_HIP_CHECK(hipMemsetAsync(wt_t, 0, bytes, st));
      if (int rc = launch_prep_weights(st, dtype, w_t.as<float>(), wt_t, nullptr, Ci, Co, k, 1, 0, Cip, Cop)) return rc;
    }
    if (split) {   // both copies in the form the matrix cores read
      if (int rc = launch_f32_split_inplace(st, wt, (long)elems)) return rc;
      if (wt_t)
        if (int rc = launch_f32_split_inplace(st, wt_t, (long)elems)) return rc;
    }
    return MAUA_OK;
  };
  const int rc = prep();
  hipStreamSynchronize(st);   // (also on failure: the staging buffers are freed behind whatever was launched)
  return rc;
}

int PlainConv::alloc(int ci, int co, int cip, int cop, size_t es, bool transposed) {
  Ci = ci; Co = co; Cip = cip; Cop = cop; esize = es;
  if (int rc = wt.alloc((size_t)9 * Cop * Cip * esize, true)) return rc;
  if (int rc = bias.alloc((size_t)Cop * 4, true)) return rc;
  return transposed ? alloc_transposed() : MAUA_OK;
}

int PlainConv::alloc_transposed() {
  if (!wt_t)
    if (int rc = wt_t.alloc((size_t)9 * Cop * Cip * esize, true)) return rc;
  if (!zero_bias)
    if (int rc = zero_bias.alloc((size_t)std::max(Cip, Cop) * 4, true)) return rc;
  return MAUA_OK;
}

int PlainConv::load_bias(hipStream_t st, const float* host) {
  MAUA_HIP_CHECK(hipStreamSynchronize(st));   // (a forward that reads the old values may still run)
  MAUA_HIP_CHECK(hipMemcpy(bias.get(), host, (size_t)Co * 4, hipMemcpyHostToDevice));
  return MAUA_OK;
}

int PlainConv::load_weight(hipStream_t st, int dtype, const float* host, bool transposed, bool split) {
  if (transposed)
    if (int rc = alloc_transposed()) return rc;
  return maua::load_weight(st, dtype, host, Co, Ci, 3, Cop, Cip, wt.get(), transposed ? wt_t.get() : nullptr, split);
}

namespace {
__global__ __launch_bounds__(256) void fill_ones_kernel(float* __restrict__ p, long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = 1.f;
}
}  // namespace

int launch_fill_ones(hipStream_t st, float* p, long n) {
  if (n <= 0) return MAUA_OK;
  hipLaunchKernelGGL(fill_ones_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, p, n);
  MAUA_HIP_CHECK(hipGetLastError());
  return MAUA_OK;
}

int UnitStyles::ensure(hipStream_t st, int B, int C, bool* moved) {
  if (B <= b && C <= c) return MAUA_OK;
  MAUA_HIP_CHECK(hipStreamSynchronize(st));
  const int nb = std::max(B, b), nc = std::max(C, c);
  if (moved) *moved = true;
  b = c = 0;
  if (int rc = buf.alloc((size_t)nb * nc * 4)) return rc;
  if (int rc = launch_fill_ones(st, p(), (long)nb * nc)) return rc;
  MAUA_HIP_CHECK(hipStreamSynchronize(st));
  b = nb; c = nc;
  return MAUA_OK;
}

}  // namespace maua
