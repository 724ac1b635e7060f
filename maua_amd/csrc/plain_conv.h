// What every network that runs plain 3x3 convolutions through the modulated-conv launchers keeps on the host side (super.hip,
// secondary.hip, perceptor.hip, unet.hip, synth.hip): the staging buffer of a weight load, the per-layer record with its prepared
// weights, and the unit styles the generic kernel multiplies its input by.  Defined in plain_conv.hip.
#pragma once
#include "common.h"

namespace maua {

// A float32 device temporary of one load: freed on every way out of its scope.  Not an allocator - the networks' long-lived
// buffers stay raw pointers with their own free lists.
struct DevTemp {
  float* p = nullptr;
  DevTemp() = default;
  DevTemp(const DevTemp&) = delete;
  DevTemp& operator=(const DevTemp&) = delete;
  DevTemp(DevTemp&& o) noexcept : p(o.p) { o.p = nullptr; }
  DevTemp& operator=(DevTemp&& o) noexcept {
    if (this != &o) { hipFree(p); p = o.p; o.p = nullptr; }
    return *this;
  }
  ~DevTemp() { hipFree(p); }   // (hipFree(NULL) is a no-op)
  int alloc(size_t count);     // `count` floats, uninitialised
  int stage(const float* src, size_t count, hipMemcpyKind kind = hipMemcpyHostToDevice);   // alloc + a synchronous copy of src
};

// f32 [Co][Ci][k][k] on the host (k = 3: a convolution, k = 1: a linear layer) -> wt [k*k][Cop][Cip] in `dtype`, zero padded, and
// (wt_t != NULL) the layer's input gradient wt_t [k*k][Cip][Cop] from Wt[ci][co][t] = W[co][ci][k*k - 1 - t]; split: both float32
// buffers in the MAUA_F32_SPLIT form.  Writes into the buffers handed in and returns with the stream idle.
int load_weight(hipStream_t st, int dtype, const float* host, int Co, int Ci, int k, int Cop, int Cip, void* wt, void* wt_t, bool split);

struct PlainConv {
  int Ci = 0, Co = 0, Cip = 0, Cop = 0;   // real / padded channel counts (the padding rule is the network's)
  void* wt = nullptr;                      // prepared [9][Cop][Cip]
  void* wt_t = nullptr;                    // the input-gradient convolution's [9][Cip][Cop], where the network has one
  float* bias = nullptr;                   // [Cop], zero padded
  float* zero_bias = nullptr;              // [max(Cip, Cop)] zeros, with wt_t: the gradient convolution has no bias
  size_t esize = 0;

  // everything allocated is zeroed; the pointers never change afterwards (captured graphs hold them)
  int alloc(int Ci, int Co, int Cip, int Cop, size_t esize, bool transposed);
  int alloc_transposed();   // wt_t + zero_bias, unless they exist
  void free();
  int load_bias(hipStream_t st, const float* host);   // Co values
  // Co * Ci * 9 values; transposed: wt_t too (allocated here on a first load)
  int load_weight(hipStream_t st, int dtype, const float* host, bool transposed, bool split = false);
};

// [b][c] floats of 1: the styles of a plain convolution on the generic kernel.  ensure() grows it for B samples of C channels
// (synchronising; the stream is idle again on return) and sets *moved when the old buffer was freed - whoever caches the pointer
// (a captured graph) has to know.
struct UnitStyles {
  float* p = nullptr;
  int b = 0, c = 0;
  int ensure(hipStream_t st, int B, int C, bool* moved = nullptr);
  void free();
};
int launch_fill_ones(hipStream_t st, float* p, long n);

}  // namespace maua
