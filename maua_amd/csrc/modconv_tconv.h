// What the three transposed-convolution units (modconv_tconv.hip, modconv_tconv_dma.hip, modconv_tconv_fir.hip) share: the order of
// a K chunk's nine weight blocks and the LDS piece swizzle of their 64-byte rows.  Included by those three only.
#pragma once

namespace maua {

// weight block k of a stage: (shift slot, class).  slot s: (p,q) = (1,1), (1,0), (0,1), (0,0); class = 2a' + b'.
// (__constant__ tables in memory: the kernels index them with a per-lane block number, the row a lane's LDS-direct load fills)
__device__ __constant__ const int kTconvSlot[9] = {0, 1, 1, 2, 2, 3, 3, 3, 3};
__device__ __constant__ const int kTconvCls[9] = {0, 0, 1, 0, 2, 0, 1, 2, 3};

// the 16-byte piece p of the 64-byte LDS row n (weights and halo alike) sits at piece p ^ tconv_swz(n): a quarter-wave's
// ds_read_b128 then hits 16 distinct bank groups (an LDS-direct load fills linearly, so padding cannot do it); applied to the
// SOURCE address of the load and to the fragment read
__device__ __forceinline__ int tconv_swz(int n) { return (n >> 2) & 3; }

}  // namespace maua
