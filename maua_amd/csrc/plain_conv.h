// What every network that runs plain 3x3 convolutions through the modulated-conv launchers keeps on the host side (super.hip,
// secondary.hip, perceptor.hip, unet.hip, synth.hip): the staging buffer of a weight load, the per-layer record with its prepared
// weights, and the unit styles the generic kernel multiplies its input by.  Defined in plain_conv.hip.
#pragma once
#include "common.h"

namespace maua {

// a device temporary of one load: `count` floats copied synchronously from src; freed on every way out of the DevBuf's scope
int stage(DevBuf& tmp, const float* src, size_t count, hipMemcpyKind kind = hipMemcpyHostToDevice);

// f32 [Co][Ci][k][k] on the host (k = 3: a convolution, k = 1: a linear layer) -> wt [k*k][Cop][Cip] in `dtype`, zero padded, and
// (wt_t != NULL) the layer's input gradient wt_t [k*k][Cip][Cop] from Wt[ci][co][t] = W[co][ci][k*k - 1 - t]; split: both float32
// buffers in the MAUA_F32_SPLIT form.  Writes into the buffers handed in and returns with the stream idle.
int load_weight(hipStream_t st, int dtype, const float* host, int Co, int Ci, int k, int Cop, int Cip, void* wt, void* wt_t, bool split);

struct PlainConv {
  int Ci = 0, Co = 0, Cip = 0, Cop = 0;   // real / padded channel counts (the padding rule is the network's)
  DevBuf wt;                               // prepared [9][Cop][Cip]
  DevBuf wt_t;                             // the input-gradient convolution's [9][Cip][Cop], where the network has one
  DevBuf bias;                             // float [Cop], zero padded
  DevBuf zero_bias;                        // float [max(Cip, Cop)] zeros, with wt_t: the gradient convolution has no bias
  size_t esize = 0;

  // everything allocated is zeroed; the pointers never change afterwards (captured graphs hold them)
  int alloc(int Ci, int Co, int Cip, int Cop, size_t esize, bool transposed);
  int alloc_transposed();   // wt_t + zero_bias, unless they exist
  int load_bias(hipStream_t st, const float* host);   // Co values
  // Co * Ci * 9 values; transposed: wt_t too (allocated here on a first load)
  int load_weight(hipStream_t st, int dtype, const float* host, bool transposed, bool split = false);
};

// [b][c] floats of 1: the styles of a plain convolution on the generic kernel.  ensure() grows it for B samples of C channels
// (synchronising; the stream is idle again on return) and sets *moved when the old buffer was freed - whoever caches the pointer
// (a captured graph) has to know.
struct UnitStyles {
  DevBuf buf;
  int b = 0, c = 0;   // what buf holds (set after it is filled)
  float* p() const { return buf.as<float>(); }
  int ensure(hipStream_t st, int B, int C, bool* moved = nullptr);
};
int launch_fill_ones(hipStream_t st, float* p, long n);

}  // namespace maua
