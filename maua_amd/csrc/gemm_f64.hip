// Float64 GEMM on v_mfma_f64_16x16x4_f64 and the GAN evaluation metrics built on it (maua/GAN/metrics/{frechet,kernel,prdc}.py).
//
// One main loop, gemm_f64_mainloop<BM, BN>: row-major C += op(A) op(B) for one BM x BN tile, 256 threads = 2 x 2 waves of (BM/2) x (BN/2),
// K in steps of 16 through two LDS stages (the next slab travels global -> registers while this one is multiplied, one barrier per step).
// Every element is loaded under a predicate (zero outside M, N, K), so any M, N, K >= 1 and any leading dimensions run unpadded.
// Operands lie in LDS in the layout their source makes cheap to write: [r][17] when K is contiguous in memory, [k][BR + 16] when the
// row / column index is; both let the 16 lanes of a fragment column and its neighbouring k read 8 bytes each without sharing a bank.
//
// Three epilogues consume the accumulators (functors over the same loop):
//   StoreEpi   c = alpha acc + beta c                                     covariances, Newton-Schulz products, the residual M - S S
//   PolyEpi    per-block partial sums of (g / n + 1)^3 and of its diagonal  KID; a second kernel adds the partials in a fixed order
//   DistEpi    d = max(|x|^2 + |y|^2 - 2 g, 0), NaN -> 0, staged in LDS     PRDC; the N x M matrix is never written (mode STORE excepted)
// No floating-point atomics anywhere: sums are trees of a fixed shape, counts are integer atomics, so reruns are bit-identical.
#include <math.h>

#include <utility>

#include "mma_f64.h"

namespace maua {
namespace {

constexpr int kThreads = 256;
constexpr int kBK = 16;
constexpr int kTopK = 16;   // values kept per row: nearest_k + 1 <= 16

template <int BM, int BN> struct TileF64 {
  static constexpr int WM = BM / 2, WN = BN / 2, FM = WM / 16, FN = WN / 16;
  static constexpr int kAStage = (BM * 17 > kBK * (BM + 16)) ? BM * 17 : kBK * (BM + 16);   // doubles per stage
  static constexpr int kBStage = (BN * 17 > kBK * (BN + 16)) ? BN * 17 : kBK * (BN + 16);
  static constexpr int kStageDoubles = 2 * (kAStage + kBStage);
  static constexpr int kDistLd = BN + 1;
  static constexpr int kDistDoubles = BM * kDistLd + BM + BN;   // the distance tile + the two radius slices
  static constexpr size_t kSmemBytes = sizeof(double) * (kStageDoubles > kDistDoubles ? kStageDoubles : kDistDoubles);
};

// op(A)(m, k) = a[m * a_rs + k * a_cs], op(B)(k, n) = b[k * b_rs + n * b_cs]; *_kcontig: K is the unit-stride index of that operand
struct OperandsF64 {
  const double* a; long a_rs, a_cs; int a_kcontig;
  const double* b; long b_rs, b_cs; int b_kcontig;
  int M, N, K;
};

inline OperandsF64 make_operands(int transa, int transb, int M, int N, int K, const double* a, long lda, const double* b,
                                                     long ldb) {
  OperandsF64 o;
  o.a = a; o.a_rs = transa ? 1 : lda; o.a_cs = transa ? lda : 1; o.a_kcontig = !transa;
  o.b = b; o.b_rs = transb ? 1 : ldb; o.b_cs = transb ? ldb : 1; o.b_kcontig = transb ? 1 : 0;
  o.M = M; o.N = N; o.K = K;
  return o;
}

// one BR x 16 slab: element (r, k) of the tile <- p[(r0 + r) * rs + (k0 + k) * ks], zero outside R x K
template <int BR>
__device__ __forceinline__ void slab_load(double (&reg)[BR / 16], const double* __restrict__ p, long rs, long ks, int kcontig, int r0, int k0,
                                          int R, int K, int tid) {
#pragma unroll
  for (int i = 0; i < BR / 16; i++) {
    const int r = kcontig ? (tid >> 4) + 16 * i : tid % BR;
    const int k = kcontig ? (tid & 15) : tid / BR + (kThreads / BR) * i;
    const int gr = r0 + r, gk = k0 + k;
    reg[i] = (gr < R && gk < K) ? p[(long)gr * rs + (long)gk * ks] : 0.0;
  }
}
template <int BR>
__device__ __forceinline__ void slab_store(const double (&reg)[BR / 16], double* lds, int kcontig, int tid) {
  const int lr = kcontig ? 17 : 1, lk = kcontig ? 1 : BR + 16;
#pragma unroll
  for (int i = 0; i < BR / 16; i++) {
    const int r = kcontig ? (tid >> 4) + 16 * i : tid % BR;
    const int k = kcontig ? (tid & 15) : tid / BR + (kThreads / BR) * i;
    lds[r * lr + k * lk] = reg[i];
  }
}

// acc[fm][fn] += the (row0, col0) tile of op(A) op(B).  smem: TileF64::kStageDoubles doubles.  Ends behind a barrier: smem is free again.
template <int BM, int BN>
__device__ __forceinline__ void gemm_f64_mainloop(f64x4 (&acc)[BM / 32][BN / 32], const OperandsF64& o, int row0, int col0, double* smem) {
  typedef TileF64<BM, BN> T;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
  double* As[2] = {smem, smem + T::kAStage};
  double* Bs[2] = {smem + 2 * T::kAStage, smem + 2 * T::kAStage + T::kBStage};
  const int alr = o.a_kcontig ? 17 : 1, alk = o.a_kcontig ? 1 : BM + 16;
  const int blr = o.b_kcontig ? 17 : 1, blk = o.b_kcontig ? 1 : BN + 16;
  double ra[BM / 16], rb[BN / 16];
  const int nk = (o.K + kBK - 1) / kBK;
  slab_load<BM>(ra, o.a, o.a_rs, o.a_cs, o.a_kcontig, row0, 0, o.M, o.K, tid);
  slab_load<BN>(rb, o.b, o.b_cs, o.b_rs, o.b_kcontig, col0, 0, o.N, o.K, tid);
  slab_store<BM>(ra, As[0], o.a_kcontig, tid);
  slab_store<BN>(rb, Bs[0], o.b_kcontig, tid);
  __syncthreads();
  const int a_off = (wm * T::WM + MmaF64::a_row(lane)) * alr + MmaF64::k_of(lane) * alk;
  const int b_off = (wn * T::WN + MmaF64::b_col(lane)) * blr + MmaF64::k_of(lane) * blk;
  for (int t = 0; t < nk; t++) {
    const bool more = t + 1 < nk;
    if (more) {
      slab_load<BM>(ra, o.a, o.a_rs, o.a_cs, o.a_kcontig, row0, (t + 1) * kBK, o.M, o.K, tid);
      slab_load<BN>(rb, o.b, o.b_cs, o.b_rs, o.b_kcontig, col0, (t + 1) * kBK, o.N, o.K, tid);
    }
    const double* A = As[t & 1] + a_off;
    const double* B = Bs[t & 1] + b_off;
#pragma unroll
    for (int kk = 0; kk < kBK / 4; kk++) {
      double af[T::FM], bf[T::FN];
#pragma unroll
      for (int fm = 0; fm < T::FM; fm++) af[fm] = A[fm * 16 * alr + kk * 4 * alk];
#pragma unroll
      for (int fn = 0; fn < T::FN; fn++) bf[fn] = B[fn * 16 * blr + kk * 4 * blk];
#pragma unroll
      for (int fm = 0; fm < T::FM; fm++)
#pragma unroll
        for (int fn = 0; fn < T::FN; fn++) MmaF64::step(acc[fm][fn], af[fm], bf[fn]);
    }
    if (more) {
      slab_store<BM>(ra, As[(t + 1) & 1], o.a_kcontig, tid);
      slab_store<BN>(rb, Bs[(t + 1) & 1], o.b_kcontig, tid);
    }
    __syncthreads();
  }
}

template <int BM, int BN>
__device__ __forceinline__ void acc_zero(f64x4 (&acc)[BM / 32][BN / 32]) {
#pragma unroll
  for (int fm = 0; fm < BM / 32; fm++)
#pragma unroll
    for (int fn = 0; fn < BN / 32; fn++) acc[fm][fn] = f64x4{0.0, 0.0, 0.0, 0.0};
}

// visit(value, tile row, tile col) for every accumulator element of this lane
template <int BM, int BN, typename F>
__device__ __forceinline__ void acc_visit(const f64x4 (&acc)[BM / 32][BN / 32], F&& visit) {
  typedef TileF64<BM, BN> T;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wm = wave >> 1, wn = wave & 1;
#pragma unroll
  for (int fm = 0; fm < T::FM; fm++)
#pragma unroll
    for (int fn = 0; fn < T::FN; fn++)
#pragma unroll
      for (int r = 0; r < 4; r++)
        visit(acc[fm][fn][r], wm * T::WM + fm * 16 + MmaF64::d_row(lane, r), wn * T::WN + fn * 16 + MmaF64::d_col(lane));
}

// fixed-shape tree over the block's 256 values (red: 256 doubles of LDS); the sum is in every thread's return value
__device__ __forceinline__ double block_sum(double v, double* red) {
  const int tid = threadIdx.x;
  __syncthreads();
  red[tid] = v;
  __syncthreads();
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  return red[0];
}

// ---- epilogues -------------------------------------------------------------------------------------------------------------------------
struct StoreEpi {
  double alpha, beta;
  double* c; long ldc;
  template <int BM, int BN>
  __device__ __forceinline__ void operator()(const f64x4 (&acc)[BM / 32][BN / 32], const OperandsF64& o, int row0, int col0, double*) const {
    acc_visit<BM, BN>(acc, [&](double v, int r, int cc) {
      const int row = row0 + r, col = col0 + cc;
      if (row < o.M && col < o.N) {
        double* p = c + (long)row * ldc + col;
        *p = beta == 0.0 ? alpha * v : alpha * v + beta * *p;
      }
    });
  }
};

struct PolyEpi {
  double n;          // kernel.py:14-15: (g / n + 1) ** 3
  double* partial;   // [blocks][2]: the whole sum, the diagonal's
  template <int BM, int BN>
  __device__ __forceinline__ void operator()(const f64x4 (&acc)[BM / 32][BN / 32], const OperandsF64& o, int row0, int col0, double* smem) const {
    double sum = 0.0, diag = 0.0;
    acc_visit<BM, BN>(acc, [&](double v, int r, int cc) {
      const int row = row0 + r, col = col0 + cc;
      if (row < o.M && col < o.N) {
        const double u = v / n + 1.0, p = u * u * u;
        sum += p;
        if (row == col) diag += p;
      }
    });
    sum = block_sum(sum, smem);
    diag = block_sum(diag, smem);
    if (threadIdx.x == 0) {
      const long blk = (long)blockIdx.y * gridDim.x + blockIdx.x;
      partial[2 * blk] = sum;
      partial[2 * blk + 1] = diag;
    }
  }
};

template <int BM, int BN, typename Epi>
__global__ __launch_bounds__(kThreads) void gemm_f64_kernel(OperandsF64 o, Epi epi) {
  extern __shared__ double smem[];
  f64x4 acc[BM / 32][BN / 32];
  acc_zero<BM, BN>(acc);
  const int row0 = blockIdx.y * BM, col0 = blockIdx.x * BN;
  gemm_f64_mainloop<BM, BN>(acc, o, row0, col0, smem);
  epi.template operator()<BM, BN>(acc, o, row0, col0, smem);
}

// ---- distance-select (prdc.py:10-24, :27-37, :52-59) -------------------------------------------------------------------------------------
enum { DIST_STORE = 0, DIST_RADII = 1, DIST_COUNT = 2 };

// keep the kTopK smallest, ascending; compile-time indices only, so the list stays in registers
__device__ __forceinline__ void topk_insert(double (&best)[kTopK], double v) {
  if (!(v < best[kTopK - 1])) return;
#pragma unroll
  for (int j = 0; j < kTopK; j++) {
    const double lo = fmin(best[j], v), hi = fmax(best[j], v);
    best[j] = lo;
    v = hi;
  }
}

struct DistArgs {
  const double* xn;      // [M] |x_i|^2
  const double* yn;      // [N] |y_j|^2
  int mode, tiles_per_block;
  double* dist; long ldd;            // STORE
  double* lists;                     // RADII: [M][gridDim.x][kTopK]
  const double* r_row;               // COUNT: radius of row i (a real sample), [M]
  const double* r_col;               //        radius of column j (a fake sample), [N]
  int* col_count;                    //        [N] sum_i (d < r_row_i)
  int* row_any;                      //        [M] any_j (d < r_col_j)
  unsigned long long* row_min;       //        [M] bits of min_j d (d >= 0: the order of the bit patterns is the order of the values)
};

template <int BM, int BN>
__global__ __launch_bounds__(kThreads) void dist_f64_kernel(OperandsF64 o, DistArgs g) {
  typedef TileF64<BM, BN> T;
  extern __shared__ double smem[];
  double* D = smem;
  double* rr = smem + BM * T::kDistLd;
  double* rc = rr + BM;
  const int tid = threadIdx.x, row0 = blockIdx.y * BM;
  const int ntiles = (o.N + BN - 1) / BN;
  const int tile_lo = blockIdx.x * g.tiles_per_block;
  const int tile_hi = tile_lo + g.tiles_per_block < ntiles ? tile_lo + g.tiles_per_block : ntiles;
  double best[kTopK];
#pragma unroll
  for (int j = 0; j < kTopK; j++) best[j] = INFINITY;
  bool any = false;
  double dmin = INFINITY;
  for (int tile = tile_lo; tile < tile_hi; tile++) {
    const int col0 = tile * BN;
    f64x4 acc[BM / 32][BN / 32];
    acc_zero<BM, BN>(acc);
    gemm_f64_mainloop<BM, BN>(acc, o, row0, col0, smem);      // ends behind a barrier: the stages may now hold the distance tile
    acc_visit<BM, BN>(acc, [&](double v, int r, int cc) {
      const int row = row0 + r, col = col0 + cc;
      double d = 0.0;
      if (row < o.M && col < o.N) {
        d = (g.xn[row] + g.yn[col]) - 2.0 * v;
        if (d != d) d = 0.0;
        d = fmax(d, 0.0);
        if (g.mode == DIST_STORE) g.dist[(long)row * g.ldd + col] = d;
      }
      D[r * T::kDistLd + cc] = d;
    });
    if (g.mode == DIST_COUNT) {
      if (tid < BM) rr[tid] = row0 + tid < o.M ? g.r_row[row0 + tid] : 0.0;
      else if (tid < BM + BN) rc[tid - BM] = col0 + tid - BM < o.N ? g.r_col[col0 + tid - BM] : 0.0;
    }
    __syncthreads();
    const int ncols = o.N - col0 < BN ? o.N - col0 : BN, nrows = o.M - row0 < BM ? o.M - row0 : BM;
    if (g.mode == DIST_RADII) {
      if (tid < nrows)
        for (int j = 0; j < ncols; j++) topk_insert(best, D[tid * T::kDistLd + j]);
    } else if (g.mode == DIST_COUNT) {
      if (tid < nrows) {
        for (int j = 0; j < ncols; j++) {
          const double d = D[tid * T::kDistLd + j];
          any = any || d < rc[j];
          dmin = fmin(dmin, d);
        }
      } else if (tid >= BM && tid - BM < ncols) {
        const int j = tid - BM;
        int cnt = 0;
        for (int i = 0; i < nrows; i++) cnt += D[i * T::kDistLd + j] < rr[i] ? 1 : 0;
        if (cnt) atomicAdd(g.col_count + col0 + j, cnt);
      }
    }
    __syncthreads();      // the tile is consumed before the next main loop stages over it
  }
  if (tid < BM && row0 + tid < o.M) {
    const int row = row0 + tid;
    if (g.mode == DIST_RADII) {
      double* out = g.lists + ((long)row * gridDim.x + blockIdx.x) * kTopK;
#pragma unroll
      for (int j = 0; j < kTopK; j++) out[j] = best[j];
    } else if (g.mode == DIST_COUNT && tile_lo < tile_hi) {
      if (any) atomicOr(g.row_any + row, 1);
      atomicMin(g.row_min + row, (unsigned long long)__double_as_longlong(dmin));
    }
  }
}

// radii[i] = the (k + 1)-th smallest of row i's lists: topk(k + 1, largest=False).max, the self distance included (prdc.py:35-36)
__global__ void radii_merge_kernel(const double* __restrict__ lists, int rows, int nlists, int k, double* __restrict__ radii) {
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= rows) return;
  double best[kTopK];
#pragma unroll
  for (int j = 0; j < kTopK; j++) best[j] = INFINITY;
  const double* p = lists + (long)row * nlists * kTopK;
  for (int i = 0; i < nlists * kTopK; i++) topk_insert(best, p[i]);
  double r = 0.0;
#pragma unroll
  for (int j = 0; j < kTopK; j++)
    if (j == k) r = best[j];
  radii[row] = r;
}

__global__ void fill_u64_kernel(unsigned long long* p, long n, unsigned long long v) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}

// counts[0..3] += precise fakes, recalled reals, sum of the density counts, covered reals (prdc.py:56-59 as integers)
__global__ void prdc_finish_kernel(const int* __restrict__ col_count, int ncol, const int* __restrict__ row_any,
                                   const unsigned long long* __restrict__ row_min, const double* __restrict__ r_row, int nrow,
                                   unsigned long long* counts) {
  unsigned long long precise = 0, recalled = 0, density = 0, covered = 0;
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < ncol; j += gridDim.x * blockDim.x) {
    precise += col_count[j] > 0;
    density += (unsigned long long)col_count[j];
  }
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nrow; i += gridDim.x * blockDim.x) {
    recalled += row_any[i] != 0;
    covered += __longlong_as_double((long long)row_min[i]) < r_row[i];
  }
  if (precise) atomicAdd(counts + 0, precise);
  if (recalled) atomicAdd(counts + 1, recalled);
  if (density) atomicAdd(counts + 2, density);
  if (covered) atomicAdd(counts + 3, covered);
}

// ---- small f64 kernels ---------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ void widen_norm_kernel(const T* __restrict__ x, int rows, int d, double* __restrict__ out, double* __restrict__ norm) {
  // one wave per row: out[row][:] = (double)x[row][:], norm[row] = sum of squares, lanes strided and then a fixed xor tree
  const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;
  double s = 0.0;
  for (int c = lane; c < d; c += 64) {
    const double v = (double)x[(long)row * d + c];
    if (out) out[(long)row * d + c] = v;
    s += v * v;
  }
  for (int m = 32; m > 0; m >>= 1) s += __shfl_xor(s, m);
  if (lane == 0 && norm) norm[row] = s;
}

// rows of out <- rows idx[] of x, widened; an index outside [0, rows) writes NaN instead of reading
template <typename T>
__global__ void gather_rows_kernel(const T* __restrict__ x, int rows, int d, const long* __restrict__ idx, int m, double* __restrict__ out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)m * d) return;
  const long r = idx[i / d];
  out[i] = (r >= 0 && r < rows) ? (double)x[r * d + i % d] : NAN;
}

template <typename T>
__global__ void col_mean_kernel(const T* __restrict__ x, int rows, int d, double* __restrict__ mean) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= d) return;
  double s = 0.0;
  for (int r = 0; r < rows; r++) s += (double)x[(long)r * d + c];
  mean[c] = s / rows;
}
template <typename T>
__global__ void centre_kernel(const T* __restrict__ x, int rows, int d, const double* __restrict__ mean, double* __restrict__ out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < (long)rows * d) out[i] = (double)x[i] - mean[i % d];
}

// out = s * in, + diag on the diagonal of a [d][d] matrix (in may be NULL: zero)
__global__ void scale_diag_kernel(const double* __restrict__ in, double s, double diag, int d, double* __restrict__ out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)d * d) return;
  double v = in ? s * in[i] : 0.0;
  if (i / d == i % d) v += diag;
  out[i] = v;
}

enum { RED_SUMSQ = 0, RED_TRACE = 1, RED_DIFFSQ = 2, RED_NONFINITE = 3 };
constexpr int kRedBlocks = 128;
// stage 1: block b sums its contiguous share; stage 2 (blocks == 1, mode < 0): the partials.  Shapes depend on n alone.
__global__ __launch_bounds__(kThreads) void reduce_kernel(const double* __restrict__ x, const double* __restrict__ y, long n, long stride, int mode,
                                                          double* __restrict__ out) {
  __shared__ double red[kThreads];
  const long per = (n + gridDim.x - 1) / gridDim.x, lo = blockIdx.x * per, hi = lo + per < n ? lo + per : n;
  double s = 0.0;
  for (long i = lo + threadIdx.x; i < hi; i += kThreads) {
    const double v = x[i * stride];
    if (mode == RED_SUMSQ) s += v * v;
    else if (mode == RED_DIFFSQ) s += (v - y[i]) * (v - y[i]);
    else if (mode == RED_NONFINITE) s += isfinite(v) ? 0.0 : 1.0;
    else s += v;
  }
  s = block_sum(s, red);
  if (threadIdx.x == 0) out[blockIdx.x] = s;
}

// kid and the per-subset sums from raw [S][3][2] = {sum, diag} of (x x^T), (y y^T), (x y^T)   (kernel.py:14-17)
__global__ void kid_finish_kernel(const double* __restrict__ raw, int S, int m, double* __restrict__ sums, double* __restrict__ kid) {
  if (blockIdx.x || threadIdx.x) return;
  double t = 0.0;
  for (int s = 0; s < S; s++) {
    const double* r = raw + 6 * s;
    const double a = r[0] + r[2], tra = r[1] + r[3], b = r[4];
    sums[3 * s] = a; sums[3 * s + 1] = tra; sums[3 * s + 2] = b;
    t += (a - tra) / (m - 1) - b * 2 / m;
  }
  *kid = t / S / m;
}

// ---- launches ------------------------------------------------------------------------------------------------------------------------
template <typename K> int allow_smem(K kern, size_t bytes) {
  MAUA_HIP_CHECK(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  return MAUA_OK;
}

template <int BM, int BN, typename Epi> int launch_gemm(hipStream_t st, const OperandsF64& o, const Epi& epi) {
  auto kern = gemm_f64_kernel<BM, BN, Epi>;
  const size_t smem = TileF64<BM, BN>::kSmemBytes;
  if (allow_smem(kern, smem) != MAUA_OK) return MAUA_ERR;
  hipLaunchKernelGGL(kern, dim3(cdiv(o.N, BN), cdiv(o.M, BM)), dim3(kThreads), smem, st, o, epi);
  return MAUA_OK;
}

// the 128 x 128 tile once both sides fill at least two of them; the 64 x 64 tile below (more blocks, less edge waste)
inline bool big_tile(int M, int N) { return M > 128 && N > 128; }

int gemm_f64(hipStream_t st, int transa, int transb, int M, int N, int K, double alpha, const double* a, long lda, const double* b, long ldb,
             double beta, double* c, long ldc) {
  const OperandsF64 o = make_operands(transa, transb, M, N, K, a, lda, b, ldb);
  const StoreEpi epi{alpha, beta, c, ldc};
  return big_tile(M, N) ? launch_gemm<128, 128>(st, o, epi) : launch_gemm<64, 64>(st, o, epi);
}

int gemm_check(const char* who, int transa, int transb, int M, int N, int K, const void* a, long lda, const void* b, long ldb, const void* c,
               long ldc) {
  const std::string w(who);
  MAUA_REQUIRE(M >= 1 && N >= 1 && K >= 1, w + ": M, N and K must be at least 1");
  MAUA_REQUIRE(a && b && c, w + ": NULL argument");
  MAUA_REQUIRE(lda >= (transa ? M : K) && ldb >= (transb ? K : N) && ldc >= N, w + ": a leading dimension is shorter than its row");
  return MAUA_OK;
}

// out[0] <- the reduction of x (tmp: kRedBlocks doubles)
void reduce(hipStream_t st, const double* x, const double* y, long n, long stride, int mode, double* tmp, double* out) {
  hipLaunchKernelGGL(reduce_kernel, dim3(kRedBlocks), dim3(kThreads), 0, st, x, y, n, stride, mode, tmp);
  hipLaunchKernelGGL(reduce_kernel, dim3(1), dim3(kThreads), 0, st, (const double*)tmp, (const double*)nullptr, (long)kRedBlocks, 1L, -1, out);
}

template <typename T> void centre(hipStream_t st, const T* x, int N, int d, double* xc, double* mean) {
  hipLaunchKernelGGL(col_mean_kernel<T>, dim3(cdiv(d, 64)), dim3(64), 0, st, x, N, d, mean);
  const long n = (long)N * d;
  hipLaunchKernelGGL(centre_kernel<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, x, N, d, (const double*)mean, xc);
}

int moments(hipStream_t st, const void* x, int f64, int N, int d, double* xc, double* mean, double* cov) {
  if (f64) centre(st, (const double*)x, N, d, xc, mean);
  else centre(st, (const float*)x, N, d, xc, mean);
  return gemm_f64(st, 1, 0, d, d, N, 1.0 / (N - 1), xc, d, xc, d, 0.0, cov, d);     // torch.cov: centred, N - 1
}

// the workspace layouts: each one function of a Scratch, measured by the *_workspace call and placed by the entry point beside it
double* moments_ws(Scratch& s, int N, int d) { return s.take<double>((size_t)N * d); }

struct SqrtmWs { double *Y, *Z, *T, *Y2, *Z2, *R, *tmp, *scal; };
SqrtmWs sqrtm_ws(Scratch& s, int d) {
  auto mat = [&] { return s.take<double>((size_t)d * d); };
  return SqrtmWs{mat(), mat(), mat(), mat(), mat(), mat(), s.take<double>(kRedBlocks), s.take<double>(8)};
}

// frechet.py:4-46.  errors [num_iters] and iters are host memory; s [d][d] is device memory.
int sqrtm_ns(hipStream_t st, const double* m, int d, int num_iters, const SqrtmWs& w, double* s, double* errors, int* iters) {
  const long dd = (long)d * d;
  const unsigned eb = (unsigned)((dd + 255) / 256);
  double ss_m = 0.0;
  reduce(st, m, nullptr, dd, 1, RED_SUMSQ, w.tmp, w.scal);
  MAUA_HIP_CHECK(hipMemcpyAsync(&ss_m, w.scal, sizeof(double), hipMemcpyDeviceToHost, st));
  MAUA_HIP_CHECK(hipStreamSynchronize(st));
  const double norm = sqrt(ss_m), root = sqrt(norm);
  hipLaunchKernelGGL(scale_diag_kernel, dim3(eb), dim3(256), 0, st, m, 1.0 / norm, 0.0, d, w.Y);     // Y = M / |M|
  hipLaunchKernelGGL(scale_diag_kernel, dim3(eb), dim3(256), 0, st, (const double*)nullptr, 0.0, 1.0, d, w.Z);
  double *Y = w.Y, *Z = w.Z, *Y2 = w.Y2, *Z2 = w.Z2;
  double prev = 1000000.0;
  int it = 0;
  for (; it < num_iters;) {
    hipLaunchKernelGGL(scale_diag_kernel, dim3(eb), dim3(256), 0, st, (const double*)nullptr, 0.0, 1.0, d, w.T);
    if (gemm_f64(st, 0, 0, d, d, d, -0.5, Z, d, Y, d, 1.5, w.T, d) != MAUA_OK) return MAUA_ERR;     // T = (3 I - Z Y) / 2
    if (gemm_f64(st, 0, 0, d, d, d, 1.0, Y, d, w.T, d, 0.0, Y2, d) != MAUA_OK) return MAUA_ERR;     // Y <- Y T
    if (gemm_f64(st, 0, 0, d, d, d, 1.0, w.T, d, Z, d, 0.0, Z2, d) != MAUA_OK) return MAUA_ERR;     // Z <- T Z
    std::swap(Y, Y2);
    std::swap(Z, Z2);
    hipLaunchKernelGGL(scale_diag_kernel, dim3(eb), dim3(256), 0, st, (const double*)Y, root, 0.0, d, s);      // S = Y sqrt(|M|)
    MAUA_HIP_CHECK(hipMemcpyAsync(w.R, m, dd * sizeof(double), hipMemcpyDeviceToDevice, st));
    if (gemm_f64(st, 0, 0, d, d, d, -1.0, s, d, s, d, 1.0, w.R, d) != MAUA_OK) return MAUA_ERR;     // R = M - S S
    reduce(st, w.R, nullptr, dd, 1, RED_SUMSQ, w.tmp, w.scal);
    double ss_r = 0.0;
    MAUA_HIP_CHECK(hipMemcpyAsync(&ss_r, w.scal, sizeof(double), hipMemcpyDeviceToHost, st));
    MAUA_HIP_CHECK(hipStreamSynchronize(st));
    const double error = sqrt(ss_r) / norm;
    if (errors) errors[it] = error;
    it++;
    if (fabs(error) <= 1e-5 || error > prev) break;      // torch.isclose(error, 0, atol=1e-5), or the divergence guard
    prev = error;
  }
  if (iters) *iters = it;
  MAUA_HIP_CHECK(hipGetLastError());
  return MAUA_OK;
}

struct FrechetWs { double *xc, *mu1, *mu2, *s1, *s2, *P, *S, *scal; SqrtmWs sq; };
FrechetWs frechet_ws(Scratch& s, int N1, int N2, int d) {
  auto mat = [&] { return s.take<double>((size_t)d * d); };
  return FrechetWs{s.take<double>((size_t)(N1 > N2 ? N1 : N2) * d), s.take<double>(d), s.take<double>(d), mat(), mat(), mat(), mat(),
                   s.take<double>(8), sqrtm_ws(s, d)};
}

struct KidWs { double *x, *y, *partial; };
KidWs kid_ws(Scratch& s, int m, int d) {
  return KidWs{s.take<double>((size_t)m * d), s.take<double>((size_t)m * d), s.take<double>((size_t)cdiv(m, 64) * cdiv(m, 64) * 2)};
}

struct PrdcWs { double *x, *y, *xn, *yn, *lists; int *col_count, *row_any; unsigned long long* row_min; };
int dist_splits(int rows, int cols) {      // column blocks per row tile: enough blocks to fill the device, lists that stay small
  const int row_tiles = cdiv(rows, 64), col_tiles = cdiv(cols, 64);
  int splits = cdiv(1024, row_tiles);
  if (splits > col_tiles) splits = col_tiles;
  if (splits > 64) splits = 64;
  return splits < 1 ? 1 : splits;
}
PrdcWs prdc_ws(Scratch& s, int N, int M, int d) {
  const size_t ln = (size_t)N * dist_splits(N, N), lm = (size_t)M * dist_splits(M, M);
  return PrdcWs{s.take<double>((size_t)N * d), s.take<double>((size_t)M * d), s.take<double>(N), s.take<double>(M),
                s.take<double>((ln > lm ? ln : lm) * kTopK), s.take<int>(M), s.take<int>(N), s.take<unsigned long long>(N)};
}

int launch_dist(hipStream_t st, const OperandsF64& o, DistArgs g, int splits) {
  auto kern = dist_f64_kernel<64, 64>;
  const size_t smem = TileF64<64, 64>::kSmemBytes;
  if (allow_smem(kern, smem) != MAUA_OK) return MAUA_ERR;
  g.tiles_per_block = cdiv(cdiv(o.N, 64), splits);
  hipLaunchKernelGGL(kern, dim3(splits, cdiv(o.M, 64)), dim3(kThreads), smem, st, o, g);
  return MAUA_OK;
}

void widen(hipStream_t st, const void* x, int f64, int rows, int d, double* out, double* norm) {
  if (f64) hipLaunchKernelGGL(widen_norm_kernel<double>, dim3(cdiv(rows, 4)), dim3(256), 0, st, (const double*)x, rows, d, out, norm);
  else hipLaunchKernelGGL(widen_norm_kernel<float>, dim3(cdiv(rows, 4)), dim3(256), 0, st, (const float*)x, rows, d, out, norm);
}

// radii of the rows of x [rows][d] (f64, norms xn) among themselves
int knn_radii(hipStream_t st, const double* x, const double* xn, int rows, int d, int k, double* lists, double* radii) {
  const OperandsF64 o = make_operands(0, 1, rows, rows, d, x, d, x, d);
  DistArgs g{};
  g.xn = xn; g.yn = xn; g.mode = DIST_RADII; g.lists = lists;
  const int splits = dist_splits(rows, rows);
  if (launch_dist(st, o, g, splits) != MAUA_OK) return MAUA_ERR;
  hipLaunchKernelGGL(radii_merge_kernel, dim3(cdiv(rows, 64)), dim3(64), 0, st, (const double*)lists, rows, splits, k, radii);
  return MAUA_OK;
}

int k_check(const char* who, int nearest_k, int rows) {
  const std::string w(who);
  MAUA_REQUIRE(nearest_k >= 1 && nearest_k <= kTopK - 1, w + ": nearest_k must be 1 .. 15");
  MAUA_REQUIRE(rows >= nearest_k + 1, w + ": a set needs at least nearest_k + 1 rows (topk of nearest_k + 1 distances, prdc.py:36)");
  return MAUA_OK;
}

}  // namespace
}  // namespace maua

using namespace maua;

extern "C" {

int maua_gemm_f64(maua_ctx* ctx, int transa, int transb, int M, int N, int K, double alpha, const double* a, long lda, const double* b, long ldb,
                  double beta, double* c, long ldc) {
  MAUA_REQUIRE(ctx, "maua_gemm_f64: ctx is NULL");
  if (gemm_check("maua_gemm_f64", transa, transb, M, N, K, a, lda, b, ldb, c, ldc) != MAUA_OK) return MAUA_ERR;
  if (gemm_f64(ctx->stream, transa, transb, M, N, K, alpha, a, lda, b, ldb, beta, c, ldc) != MAUA_OK) return MAUA_ERR;
  MAUA_HIP_CHECK(hipGetLastError());
  return MAUA_OK;
}

long maua_metrics_moments_workspace(int N, int d) {
  if (N < 2 || d < 1) return 0;
  return (long)scratch_bytes(moments_ws, N, d);
}

int maua_metrics_moments(maua_ctx* ctx, const void* feats, int f64, int N, int d, void* ws, long ws_bytes, double* mean, double* cov) {
  MAUA_REQUIRE(ctx, "maua_metrics_moments: ctx is NULL");
  MAUA_REQUIRE(N >= 2 && d >= 1, "maua_metrics_moments: N must be at least 2 (the covariance divides by N - 1) and d at least 1");
  MAUA_REQUIRE(feats && ws && mean && cov, "maua_metrics_moments: NULL argument");
  MAUA_REQUIRE(((size_t)ws & 255) == 0 && ws_bytes >= maua_metrics_moments_workspace(N, d),
               "maua_metrics_moments: the workspace must be 256-byte aligned and hold maua_metrics_moments_workspace() bytes");
  Scratch s(ws);
  if (moments(ctx->stream, feats, f64, N, d, moments_ws(s, N, d), mean, cov) != MAUA_OK) return MAUA_ERR;
  MAUA_HIP_CHECK(hipGetLastError());
  return MAUA_OK;
}

long maua_sqrtm_workspace(int d) { return d < 1 ? 0 : (long)scratch_bytes(sqrtm_ws, d); }

int maua_sqrtm_newton_schulz(maua_ctx* ctx, const double* m, int d, int num_iters, void* ws, long ws_bytes, double* s, double* errors, int* iters) {
  MAUA_REQUIRE(ctx, "maua_sqrtm_newton_schulz: ctx is NULL");
  MAUA_REQUIRE(d >= 1, "maua_sqrtm_newton_schulz: d must be at least 1");
  MAUA_REQUIRE(num_iters > 0, "maua_sqrtm_newton_schulz: num_iters must be greater than 0");
  MAUA_REQUIRE(m && ws && s, "maua_sqrtm_newton_schulz: NULL argument");
  MAUA_REQUIRE(((size_t)ws & 255) == 0 && ws_bytes >= maua_sqrtm_workspace(d),
               "maua_sqrtm_newton_schulz: the workspace must be 256-byte aligned and hold maua_sqrtm_workspace() bytes");
  Scratch place(ws);
  return sqrtm_ns(ctx->stream, m, d, num_iters, sqrtm_ws(place, d), s, errors, iters);
}

long maua_frechet_workspace(int N1, int N2, int d) {
  if (N1 < 2 || N2 < 2 || d < 1) return 0;
  return (long)scratch_bytes(frechet_ws, N1, N2, d);
}

int maua_frechet_distance(maua_ctx* ctx, const void* feats1, int N1, const void* feats2, int N2, int d, int f64, double eps, int num_iters,
                          void* ws, long ws_bytes, double* distance, double* errors, int* iters, int* retried) {
  MAUA_REQUIRE(ctx, "maua_frechet_distance: ctx is NULL");
  MAUA_REQUIRE(N1 >= 2 && N2 >= 2 && d >= 1, "maua_frechet_distance: both sets need at least 2 rows and d at least 1");
  MAUA_REQUIRE(num_iters > 0, "maua_frechet_distance: num_iters must be greater than 0");
  MAUA_REQUIRE(feats1 && feats2 && ws && distance, "maua_frechet_distance: NULL argument");
  MAUA_REQUIRE(((size_t)ws & 255) == 0 && ws_bytes >= maua_frechet_workspace(N1, N2, d),
               "maua_frechet_distance: the workspace must be 256-byte aligned and hold maua_frechet_workspace() bytes");
  hipStream_t st = ctx->stream;
  Scratch place(ws);
  const FrechetWs w = frechet_ws(place, N1, N2, d);
  const SqrtmWs& q = w.sq;
  if (moments(st, feats1, f64, N1, d, w.xc, w.mu1, w.s1) != MAUA_OK) return MAUA_ERR;
  if (moments(st, feats2, f64, N2, d, w.xc, w.mu2, w.s2) != MAUA_OK) return MAUA_ERR;
  const long dd = (long)d * d;
  const unsigned eb = (unsigned)((dd + 255) / 256);
  double host[5];
  if (retried) *retried = 0;
  if (gemm_f64(st, 0, 0, d, d, d, 1.0, w.s1, d, w.s2, d, 0.0, w.P, d) != MAUA_OK) return MAUA_ERR;
  if (sqrtm_ns(st, w.P, d, num_iters, w.sq, w.S, errors, iters) != MAUA_OK) return MAUA_ERR;
  reduce(st, w.S, nullptr, dd, 1, RED_NONFINITE, q.tmp, w.scal + 4);
  MAUA_HIP_CHECK(hipMemcpyAsync(host + 4, w.scal + 4, sizeof(double), hipMemcpyDeviceToHost, st));
  MAUA_HIP_CHECK(hipStreamSynchronize(st));
  if (host[4] != 0.0) {
    // frechet.py:82-85: the product might be almost singular; eps on both diagonals for the product alone (the traces below stay those of
    // the covariances without it).  The offset copies borrow two of the iteration's buffers, which it overwrites afterwards.
    hipLaunchKernelGGL(scale_diag_kernel, dim3(eb), dim3(256), 0, st, (const double*)w.s1, 1.0, eps, d, q.R);
    hipLaunchKernelGGL(scale_diag_kernel, dim3(eb), dim3(256), 0, st, (const double*)w.s2, 1.0, eps, d, q.T);
    if (gemm_f64(st, 0, 0, d, d, d, 1.0, q.R, d, q.T, d, 0.0, w.P, d) != MAUA_OK) return MAUA_ERR;
    if (sqrtm_ns(st, w.P, d, num_iters, w.sq, w.S, errors, iters) != MAUA_OK) return MAUA_ERR;
    if (retried) *retried = 1;
  }
  reduce(st, w.mu1, w.mu2, d, 1, RED_DIFFSQ, q.tmp, w.scal + 0);
  reduce(st, w.s1, nullptr, d, (long)d + 1, RED_TRACE, q.tmp, w.scal + 1);
  reduce(st, w.s2, nullptr, d, (long)d + 1, RED_TRACE, q.tmp, w.scal + 2);
  reduce(st, w.S, nullptr, d, (long)d + 1, RED_TRACE, q.tmp, w.scal + 3);
  MAUA_HIP_CHECK(hipMemcpyAsync(host, w.scal, 4 * sizeof(double), hipMemcpyDeviceToHost, st));
  MAUA_HIP_CHECK(hipStreamSynchronize(st));
  *distance = host[0] + host[1] + host[2] - 2 * host[3];      // frechet.py:93
  MAUA_HIP_CHECK(hipGetLastError());
  return MAUA_OK;
}

long maua_kernel_distance_workspace(int m, int d) {
  if (m < 2 || d < 1) return 0;
  return (long)scratch_bytes(kid_ws, m, d);
}

int maua_kernel_distance(maua_ctx* ctx, const void* feats1, int N1, const void* feats2, int N2, int d, int f64, const long* idx, int S, int m,
                         void* ws, long ws_bytes, double* kid, double* sums, double* raw) {
  MAUA_REQUIRE(ctx, "maua_kernel_distance: ctx is NULL");
  MAUA_REQUIRE(N1 >= 1 && N2 >= 1 && d >= 1 && S >= 1, "maua_kernel_distance: N1, N2, d and the subset count must be at least 1");
  MAUA_REQUIRE(m >= 2 && m <= N1 && m <= N2, "maua_kernel_distance: the subset size must be 2 .. min(N1, N2) (kernel.py:16 divides by m - 1)");
  MAUA_REQUIRE(feats1 && feats2 && idx && ws && kid && sums && raw, "maua_kernel_distance: NULL argument");
  MAUA_REQUIRE(((size_t)ws & 255) == 0 && ws_bytes >= maua_kernel_distance_workspace(m, d),
               "maua_kernel_distance: the workspace must be 256-byte aligned and hold maua_kernel_distance_workspace() bytes");
  hipStream_t st = ctx->stream;
  Scratch place(ws);
  const KidWs w = kid_ws(place, m, d);
  double *x = w.x, *y = w.y, *partial = w.partial;
  const int blocks = cdiv(m, 64) * cdiv(m, 64);
  const unsigned gb = (unsigned)(((long)m * d + 255) / 256);
  for (int s = 0; s < S; s++) {
    const long* ix = idx + (long)s * 2 * m;      // kernel.py:12-13: x from feats2, y from feats1
    if (f64) {
      hipLaunchKernelGGL(gather_rows_kernel<double>, dim3(gb), dim3(256), 0, st, (const double*)feats2, N2, d, ix, m, x);
      hipLaunchKernelGGL(gather_rows_kernel<double>, dim3(gb), dim3(256), 0, st, (const double*)feats1, N1, d, ix + m, m, y);
    } else {
      hipLaunchKernelGGL(gather_rows_kernel<float>, dim3(gb), dim3(256), 0, st, (const float*)feats2, N2, d, ix, m, x);
      hipLaunchKernelGGL(gather_rows_kernel<float>, dim3(gb), dim3(256), 0, st, (const float*)feats1, N1, d, ix + m, m, y);
    }
    const double* lhs[3] = {x, y, x};
    const double* rhs[3] = {x, y, y};
    for (int p = 0; p < 3; p++) {
      const OperandsF64 o = make_operands(0, 1, m, m, d, lhs[p], d, rhs[p], d);
      if (launch_gemm<64, 64>(st, o, PolyEpi{(double)d, partial}) != MAUA_OK) return MAUA_ERR;
      double* out = raw + 6 * s + 2 * p;
      hipLaunchKernelGGL(reduce_kernel, dim3(1), dim3(kThreads), 0, st, (const double*)partial, (const double*)nullptr, (long)blocks, 2L, -1, out);
      hipLaunchKernelGGL(reduce_kernel, dim3(1), dim3(kThreads), 0, st, (const double*)partial + 1, (const double*)nullptr, (long)blocks, 2L, -1,
                         out + 1);
    }
  }
  hipLaunchKernelGGL(kid_finish_kernel, dim3(1), dim3(64), 0, st, (const double*)raw, S, m, sums, kid);
  MAUA_HIP_CHECK(hipGetLastError());
  return MAUA_OK;
}

long maua_prdc_workspace(int N, int M, int d) {
  if (N < 1 || M < 1 || d < 1) return 0;
  return (long)scratch_bytes(prdc_ws, N, M, d);
}

int maua_knn_radii(maua_ctx* ctx, const void* feats, int N, int d, int f64, int nearest_k, void* ws, long ws_bytes, double* radii) {
  MAUA_REQUIRE(ctx, "maua_knn_radii: ctx is NULL");
  MAUA_REQUIRE(N >= 1 && d >= 1, "maua_knn_radii: N and d must be at least 1");
  if (k_check("maua_knn_radii", nearest_k, N) != MAUA_OK) return MAUA_ERR;
  MAUA_REQUIRE(feats && ws && radii, "maua_knn_radii: NULL argument");
  MAUA_REQUIRE(((size_t)ws & 255) == 0 && ws_bytes >= maua_prdc_workspace(N, 1, d),
               "maua_knn_radii: the workspace must be 256-byte aligned and hold maua_prdc_workspace(N, 1, d) bytes");
  Scratch place(ws);
  const PrdcWs w = prdc_ws(place, N, 1, d);
  widen(ctx->stream, feats, f64, N, d, w.x, w.xn);
  if (knn_radii(ctx->stream, w.x, w.xn, N, d, nearest_k, w.lists, radii) != MAUA_OK) return MAUA_ERR;
  MAUA_HIP_CHECK(hipGetLastError());
  return MAUA_OK;
}

int maua_pairwise_distances(maua_ctx* ctx, const void* x, int N, const void* y, int M, int d, int f64, void* ws, long ws_bytes, double* dist) {
  MAUA_REQUIRE(ctx, "maua_pairwise_distances: ctx is NULL");
  MAUA_REQUIRE(N >= 1 && M >= 1 && d >= 1, "maua_pairwise_distances: N, M and d must be at least 1");
  MAUA_REQUIRE(x && y && ws && dist, "maua_pairwise_distances: NULL argument");
  MAUA_REQUIRE(((size_t)ws & 255) == 0 && ws_bytes >= maua_prdc_workspace(N, M, d),
               "maua_pairwise_distances: the workspace must be 256-byte aligned and hold maua_prdc_workspace() bytes");
  Scratch place(ws);
  const PrdcWs w = prdc_ws(place, N, M, d);
  widen(ctx->stream, x, f64, N, d, w.x, w.xn);
  widen(ctx->stream, y, f64, M, d, w.y, w.yn);
  const OperandsF64 o = make_operands(0, 1, N, M, d, w.x, d, w.y, d);
  DistArgs g{};
  g.xn = w.xn; g.yn = w.yn; g.mode = DIST_STORE; g.dist = dist; g.ldd = M;
  if (launch_dist(ctx->stream, o, g, cdiv(M, 64)) != MAUA_OK) return MAUA_ERR;
  MAUA_HIP_CHECK(hipGetLastError());
  return MAUA_OK;
}

int maua_prdc(maua_ctx* ctx, const void* real, int N, const void* fake, int M, int d, int f64, int nearest_k, void* ws, long ws_bytes,
              unsigned long long* counts, double* r_real, double* r_fake) {
  MAUA_REQUIRE(ctx, "maua_prdc: ctx is NULL");
  MAUA_REQUIRE(N >= 1 && M >= 1 && d >= 1, "maua_prdc: N, M and d must be at least 1");
  if (k_check("maua_prdc", nearest_k, N < M ? N : M) != MAUA_OK) return MAUA_ERR;
  MAUA_REQUIRE(real && fake && ws && counts && r_real && r_fake, "maua_prdc: NULL argument");
  MAUA_REQUIRE(((size_t)ws & 255) == 0 && ws_bytes >= maua_prdc_workspace(N, M, d),
               "maua_prdc: the workspace must be 256-byte aligned and hold maua_prdc_workspace() bytes");
  hipStream_t st = ctx->stream;
  Scratch place(ws);
  const PrdcWs w = prdc_ws(place, N, M, d);
  widen(st, real, f64, N, d, w.x, w.xn);
  widen(st, fake, f64, M, d, w.y, w.yn);
  if (knn_radii(st, w.x, w.xn, N, d, nearest_k, w.lists, r_real) != MAUA_OK) return MAUA_ERR;
  if (knn_radii(st, w.y, w.yn, M, d, nearest_k, w.lists, r_fake) != MAUA_OK) return MAUA_ERR;
  MAUA_HIP_CHECK(hipMemsetAsync(w.col_count, 0, (size_t)M * 4, st));
  MAUA_HIP_CHECK(hipMemsetAsync(w.row_any, 0, (size_t)N * 4, st));
  MAUA_HIP_CHECK(hipMemsetAsync(counts, 0, 4 * sizeof(unsigned long long), st));
  hipLaunchKernelGGL(fill_u64_kernel, dim3(cdiv(N, 256)), dim3(256), 0, st, w.row_min, (long)N, 0x7ff0000000000000ull);     // +inf
  const OperandsF64 o = make_operands(0, 1, N, M, d, w.x, d, w.y, d);
  DistArgs g{};
  g.xn = w.xn; g.yn = w.yn; g.mode = DIST_COUNT;
  g.r_row = r_real; g.r_col = r_fake; g.col_count = w.col_count; g.row_any = w.row_any; g.row_min = w.row_min;
  if (launch_dist(st, o, g, dist_splits(N, M)) != MAUA_OK) return MAUA_ERR;
  hipLaunchKernelGGL(prdc_finish_kernel, dim3(64), dim3(256), 0, st, (const int*)w.col_count, M, (const int*)w.row_any,
                     (const unsigned long long*)w.row_min, (const double*)r_real, N, counts);
  MAUA_HIP_CHECK(hipGetLastError());
  return MAUA_OK;
}

}  // extern "C"
