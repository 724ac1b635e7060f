// Dense float64 singular value decomposition and symmetric eigendecomposition: one-sided Jacobi (Hestenes).
//
// Serves (reference): maua/GAN/decomposition/sefa.py:7,25 - `torch.svd(weight).V` of the stacked style-affine weights.
// No rocSOLVER, hipSOLVER or torch.linalg: the rotations below are the whole solver.
//
// Storage: the workspace holds At [n][mp] (column j of A is row j, contiguous; mp = m rounded up to even, the pad is zero and stays zero
// under a rotation) and Vt [n][np] (row j = v_j, V starts as I).  A pair (p, q) of columns is orthogonalised by the plane rotation that
// zeroes a_p . a_q; the same rotation goes to v_p, v_q.  The pairs of a sweep follow the round-robin tournament (jacobi_pair): N - 1
// rounds of N / 2 disjoint pairs, so a round's pairs run side by side and rounds are separated by a launch boundary (path 2) or a
// workgroup barrier (path 1).  No grid-wide barrier, no float atomics.
//
// Same bits everywhere: alpha = |a_p|^2, beta = |a_q|^2, gamma = a_p . a_q come from ONE function, dot3, run by ONE wave: lane l adds
// elements 2l, 2l + 1, 2l + 128, 2l + 129, ... in that order with fma, then the 64 partial sums fold as v += shfl_xor(v, o), o = 32 .. 1
// (a + b is commutative, so every lane holds the same bits).  The rotation's scalars and the element update (rot2) are written without
// contraction.  Path 1 (one workgroup, everything resident in LDS) and path 2 (one launch per round, one workgroup per pair) call
// the same functions on the same values in the same pair order and therefore return the same bits; so does a rerun.
#include <algorithm>
#include <cmath>
#include <numeric>
#include <vector>

#include "common.h"
#include "internal.h"

namespace maua {
namespace {

constexpr int kSvdMaxN = 4096;            // the chosen upper limits: n columns, m rows
constexpr int kSvdMaxM = 1 << 20;
constexpr int kSvdMaxSweeps = 30;
constexpr long kLdsBudget = 159 * 1024;   // path 1: At, Vt and the reduction scratch of one workgroup (160 KiB per CU, 1 KiB spare)
constexpr int kLdsScratch = 128;          // path 1: 16 per-wave rotation counts + the total
constexpr long kStageBudget = 128 * 1024; // path 2: both columns of a pair staged in LDS between the dot products and the update
constexpr int kPairThreads = 256;
constexpr int kResidentThreads = 1024;
constexpr double kEps = 2.220446049250313e-16;   // 2^-52

inline int even_up(int x) { return (x + 1) & ~1; }
inline long resident_bytes(int m, int n) { return ((long)even_up(m) + even_up(n)) * n * 8 + kLdsScratch; }

// Pair i (0 <= i < N / 2) of round r (0 <= r < N - 1) of the tournament on N (even) players: position 0 holds player 0 for good, position
// k >= 1 holds player 1 + (k - 1 + r) mod (N - 1); the pair is (position i, position N - 1 - i).
__host__ __device__ inline void jacobi_pair(int N, int r, int i, int* p, int* q) {
  const int k = N - 1 - i;
  *p = i == 0 ? 0 : 1 + (i - 1 + r) % (N - 1);
  *q = 1 + (k - 1 + r) % (N - 1);
}

typedef double d2 __attribute__((ext_vector_type(2)));

// The one dot-product function (see the head of the file).  x, y: mp doubles, 16-byte aligned, mp even.  Every lane of the wave returns
// the same three sums.
__device__ __forceinline__ void dot3(const double* x, const double* y, int mp, int lane, double* alpha, double* beta, double* gamma) {
  double a = 0.0, b = 0.0, g = 0.0;
  for (int k = 2 * lane; k < mp; k += 128) {
    const d2 u = *(const d2*)(x + k), v = *(const d2*)(y + k);
    a = fma(u.x, u.x, a); a = fma(u.y, u.y, a);
    b = fma(v.x, v.x, b); b = fma(v.y, v.y, b);
    g = fma(u.x, v.x, g); g = fma(u.y, v.y, g);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    a += __shfl_xor(a, o);
    b += __shfl_xor(b, o);
    g += __shfl_xor(g, o);
  }
  *alpha = a; *beta = b; *gamma = g;
}

// c = 1 / sqrt(1 + t^2), |t| <= 1, rounded once.  The plain expression is biased: for a small t the root of 1 + k eps (k odd) lies just
// below a rounding tie and always rounds down, so c^2 + s^2 exceeds 1 by 0.24 eps on average, every column's norm creeps up by a
// quarter eps per rotation (+23 eps over the ~600 rotations of a 64-column run) and sum(sigma) drifts off the trace.  Here the
// residuals of 1 + t^2, of the root and of the reciprocal are carried (exact by fma) and folded into one correction: c is the
// correctly rounded value in all but 4 of 10^4 cases and c^2 + s^2 - 1 averages below 0.01 eps.
__device__ __forceinline__ double cosine_of_tangent(double t) {
#pragma clang fp contract(off)
  const double p = t * t, pe = fma(t, t, -p);
  const double w = 1.0 + p, e = ((1.0 - w) + p) + pe;     // 1 + t^2 = w + e
  const double r = sqrt(w), rho = fma(-r, r, w);          // w = r^2 + rho
  const double d = (rho + e) / (2.0 * r);                 // sqrt(w + e) = r + d
  const double c0 = 1.0 / r, q = fma(-c0, r, 1.0);        // 1 = c0 r + q
  return fma(c0, q - d * c0, c0);                         // 1 / (r + d) = c0 (1 + q - d c0)
}

// LAPACK dgesvj's stop rule and the rotation that zeroes gamma: false = the pair is left as it is.
__device__ __forceinline__ bool rotation(double alpha, double beta, double gamma, double tol, double* c, double* s) {
#pragma clang fp contract(off)
  if (alpha == 0.0 || beta == 0.0 || !(fabs(gamma) > tol * (sqrt(alpha) * sqrt(beta)))) return false;
  const double zeta = (beta - alpha) / (2.0 * gamma);
  const double t = (zeta < 0.0 ? -1.0 : 1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
  *c = cosine_of_tangent(t);
  *s = *c * t;
  return true;
}

// x <- c x - s y, y <- s x + c y on `len` (even) doubles: thread `tid` of `nthreads` takes the 16-byte pieces tid, tid + nthreads, ...
// Each product and each sum is rounded on its own, so who runs an element does not change it.
__device__ __forceinline__ void rot2(const double* xi, const double* yi, double* xo, double* yo, int len, double c, double s, int tid, int nthreads) {
#pragma clang fp contract(off)
  for (int k = 2 * tid; k < len; k += 2 * nthreads) {
    const d2 u = *(const d2*)(xi + k), v = *(const d2*)(yi + k);
    d2 nu, nv;
    nu.x = c * u.x - s * v.x; nu.y = c * u.y - s * v.y;
    nv.x = s * u.x + c * v.x; nv.y = s * u.y + c * v.y;
    *(d2*)(xo + k) = nu;
    *(d2*)(yo + k) = nv;
  }
}

// ---- set-up: At = (A + shift I)^T with a zero pad, Vt = I ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void jacobi_load_kernel(const double* __restrict__ A, long lda, int m, int n, int mp, int np,
                                                          const double* __restrict__ shift, double* __restrict__ At, double* __restrict__ Vt) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long na = (long)n * mp, nv = (long)n * np;
  if (idx < na) {
    const int j = (int)(idx / mp), r = (int)(idx % mp);
    double v = 0.0;
    if (r < m) {
      v = A[(long)r * lda + j];
      if (shift && r == j) v += *shift;
    }
    At[idx] = v;
  } else if (idx < na + nv) {
    const long k = idx - na;
    Vt[k] = (k / np == k % np) ? 1.0 : 0.0;
  }
}

// ---- path 2: one launch per round, one workgroup per pair ----------------------------------------------------------------------------
// staged != 0: the two columns go to LDS once (dynamic, 2 mp doubles), the dot products and the update read them there and each column is
// read from memory once per round; staged == 0 (columns beyond the LDS budget): both read memory.  Wave 0 runs dot3; everybody updates.
// rotated [N / 2]: slot i counts pair i's rotations over the rounds of a sweep - one workgroup per slot per launch, launches in order,
// so a plain load and store.
__global__ __launch_bounds__(kPairThreads) void jacobi_pair_kernel(double* __restrict__ At, double* __restrict__ Vt, int m, int n, int mp, int np,
                                                                   int N, int round, int staged, double tol, int* __restrict__ rotated) {
  extern __shared__ __attribute__((aligned(16))) double cols[];
  __shared__ double cs[2];
  __shared__ int flag;
  int p, q;
  jacobi_pair(N, round, blockIdx.x, &p, &q);
  if (p >= n || q >= n) return;    // the padding index of an odd n (uniform over the workgroup)
  double* ap = At + (long)p * mp;
  double* aq = At + (long)q * mp;
  const int tid = threadIdx.x;
  const double *xp = ap, *xq = aq;
  if (staged) {
    for (int k = 2 * tid; k < mp; k += 2 * kPairThreads) {
      *(d2*)(cols + k) = *(const d2*)(ap + k);
      *(d2*)(cols + mp + k) = *(const d2*)(aq + k);
    }
    xp = cols;
    xq = cols + mp;
    __syncthreads();
  }
  if (tid < 64) {
    double alpha, beta, gamma, c = 1.0, s = 0.0;
    dot3(xp, xq, mp, tid, &alpha, &beta, &gamma);
    const bool rot = rotation(alpha, beta, gamma, tol, &c, &s);
    if (tid == 0) {
      cs[0] = c; cs[1] = s; flag = rot ? 1 : 0;
      rotated[blockIdx.x] += rot ? 1 : 0;
    }
  }
  __syncthreads();
  if (!flag) return;
  const double c = cs[0], s = cs[1];
  rot2(xp, xq, ap, aq, mp, c, s, tid, kPairThreads);
  double* vp = Vt + (long)p * np;
  double* vq = Vt + (long)q * np;
  rot2(vp, vq, vp, vq, np, c, s, tid, kPairThreads);
}

// sum of rotated [count] -> total [0], and the slots back to zero for the next sweep (integers: the order does not matter)
__global__ __launch_bounds__(256) void jacobi_count_kernel(int* __restrict__ rotated, int count, int* __restrict__ total) {
  __shared__ int part[256];
  int v = 0;
  for (int i = threadIdx.x; i < count; i += 256) {
    v += rotated[i];
    rotated[i] = 0;
  }
  part[threadIdx.x] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) part[threadIdx.x] += part[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) total[0] = part[0];
}

// ---- path 1: one workgroup, At and Vt resident in LDS, every round and sweep in one launch ------------------------------------------------
// 16 waves; wave w takes pairs w, w + 16, ... of a round (dot3, rotation and rot2 by that wave alone), a barrier ends the round.
// info [0] = sweeps run, info [1] = rotations of the last sweep.
__global__ __launch_bounds__(kResidentThreads) void jacobi_resident_kernel(double* __restrict__ At, double* __restrict__ Vt, int m, int n, int mp, int np,
                                                                           int max_sweeps, double tol, int* __restrict__ info) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  double* a = sm;
  double* v = sm + (long)n * mp;
  int* counts = (int*)(v + (long)n * np);   // [16] per wave, [16] the total
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, waves = kResidentThreads / 64;
  const int na = n * mp, nv = n * np;       // both even
  for (int k = 2 * tid; k < na; k += 2 * kResidentThreads) *(d2*)(a + k) = *(const d2*)(At + k);
  for (int k = 2 * tid; k < nv; k += 2 * kResidentThreads) *(d2*)(v + k) = *(const d2*)(Vt + k);
  __syncthreads();
  const int N = n + (n & 1);
  int sweeps = 0, total = 0;
  for (int sweep = 0; sweep < max_sweeps; sweep++) {
    int rot_count = 0;
    for (int r = 0; r < N - 1; r++) {
      for (int i = wave; i < N / 2; i += waves) {
        int p, q;
        jacobi_pair(N, r, i, &p, &q);
        if (p >= n || q >= n) continue;
        double* ap = a + p * mp;
        double* aq = a + q * mp;
        double alpha, beta, gamma, c = 1.0, s = 0.0;
        dot3(ap, aq, mp, lane, &alpha, &beta, &gamma);
        if (rotation(alpha, beta, gamma, tol, &c, &s)) {   // uniform over the wave: every lane holds the same sums
          rot_count++;
          rot2(ap, aq, ap, aq, mp, c, s, lane, 64);
          rot2(v + p * np, v + q * np, v + p * np, v + q * np, np, c, s, lane, 64);
        }
      }
      __syncthreads();
    }
    if (lane == 0) counts[wave] = rot_count;
    __syncthreads();
    if (tid == 0) {
      int t = 0;
      for (int w = 0; w < waves; w++) t += counts[w];
      counts[16] = t;
    }
    __syncthreads();
    total = counts[16];
    sweeps = sweep + 1;
    __syncthreads();
    if (total == 0) break;     // uniform: everybody read the same word
  }
  for (int k = 2 * tid; k < na; k += 2 * kResidentThreads) *(d2*)(At + k) = *(const d2*)(a + k);
  for (int k = 2 * tid; k < nv; k += 2 * kResidentThreads) *(d2*)(Vt + k) = *(const d2*)(v + k);
  if (tid == 0) {
    info[0] = sweeps;
    info[1] = total;
  }
}

// ---- finish --------------------------------------------------------------------------------------------------------------------------
// one wave per column j: sigma_j = sqrt(dot3's |a_j|^2); sign_j = -1 where v_j's largest-magnitude component (lowest index on a tie) is
// negative, else +1
__global__ __launch_bounds__(64) void jacobi_column_kernel(const double* __restrict__ At, const double* __restrict__ Vt, int n, int mp, int np,
                                                           double* __restrict__ sigma, double* __restrict__ sign) {
  const int j = blockIdx.x, lane = threadIdx.x;
  const double* a = At + (long)j * mp;
  double alpha, beta, gamma;
  dot3(a, a, mp, lane, &alpha, &beta, &gamma);
  const double* v = Vt + (long)j * np;
  double best = -1.0, val = 0.0;
  int at = 0x7fffffff;
  for (int k = lane; k < n; k += 64) {
    const double x = v[k], ax = fabs(x);
    if (ax > best) { best = ax; val = x; at = k; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ob = __shfl_xor(best, o), ov = __shfl_xor(val, o);
    const int oa = __shfl_xor(at, o);
    if (ob > best || (ob == best && oa < at)) { best = ob; val = ov; at = oa; }
  }
  if (lane == 0) {
    sigma[j] = sqrt(alpha);
    sign[j] = val < 0.0 ? -1.0 : 1.0;
  }
}

// out column i = Jacobi column order[i]: S[i] = sigma - shift, V[k][i] = sign v[k], U[r][i] = sign a[r] / sigma (0 where sigma = 0)
__global__ __launch_bounds__(256) void jacobi_emit_kernel(const double* __restrict__ At, const double* __restrict__ Vt, int m, int n, int mp, int np,
                                                          const double* __restrict__ sigma, const double* __restrict__ sign,
                                                          const int* __restrict__ order, const double* __restrict__ shift,
                                                          double* __restrict__ S, double* __restrict__ U, double* __restrict__ V) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)m * n) return;          // m >= n
  const int r = (int)(idx / n), i = (int)(idx % n);
  const int j = order[i];
  const double sg = sigma[j], sn = sign[j];
  if (r == 0) S[i] = shift ? sg - *shift : sg;
  if (r < n) V[(long)r * n + i] = sn * Vt[(long)j * np + r];
  if (U) U[(long)r * n + i] = sg > 0.0 ? sn * At[(long)j * mp + r] / sg : 0.0;
}

// ---- eigh's shift: the Gershgorin bound c = max_i sum_j |S_ij| ------------------------------------------------------------------------
__global__ __launch_bounds__(64) void gershgorin_rows_kernel(const double* __restrict__ S, long lds, int n, double* __restrict__ rows) {
  const int i = blockIdx.x, lane = threadIdx.x;
  double a = 0.0;
  for (int k = lane; k < n; k += 64) a += fabs(S[(long)i * lds + k]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
  if (lane == 0) rows[i] = a;
}
__global__ __launch_bounds__(64) void gershgorin_max_kernel(const double* __restrict__ rows, int n, double* __restrict__ shift) {
  const int lane = threadIdx.x;
  double a = 0.0;
  for (int k = lane; k < n; k += 64) a = fmax(a, rows[k]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) a = fmax(a, __shfl_xor(a, o));
  if (lane == 0) shift[0] = a;
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------
struct SvdWs { double *At, *Vt, *sigma, *sign, *shift, *rows; int *order, *rotated, *info; };
SvdWs svd_ws(Scratch& s, int m, int n) {
  const int mp = even_up(m), np = even_up(n), N = n + (n & 1);
  SvdWs w;
  w.At = s.take<double>((size_t)n * mp);
  w.Vt = s.take<double>((size_t)n * np);
  w.sigma = s.take<double>(n);
  w.sign = s.take<double>(n);
  w.shift = s.take<double>(1);
  w.rows = s.take<double>(n);
  w.order = s.take<int>(n);
  w.rotated = s.take<int>(N / 2);
  w.info = s.take<int>(2);
  return w;
}

int svd_check(const char* who, const void* a, int m, int n, long lda, int path, int max_sweeps, const void* ws, long ws_bytes, const void* s,
              const void* v) {
  const std::string w(who);
  MAUA_REQUIRE(n >= 1, w + ": n must be at least 1");
  MAUA_REQUIRE(m >= n, w + ": m must be at least n (decompose the transpose: the Python layer does)");
  MAUA_REQUIRE(n <= kSvdMaxN && m <= kSvdMaxM, w + ": at most 4096 columns and 1048576 rows");
  MAUA_REQUIRE(lda >= n, w + ": the leading dimension must be at least n");
  MAUA_REQUIRE(path >= 0 && path <= 2, w + ": path must be 0 (auto), 1 (one workgroup, LDS resident) or 2 (one launch per round)");
  MAUA_REQUIRE(max_sweeps >= 0 && max_sweeps <= kSvdMaxSweeps, w + ": max_sweeps must be 1 .. 30 (0 = 30)");
  MAUA_REQUIRE(path != 1 || resident_bytes(m, n) <= kLdsBudget,
               w + ": path 1 keeps (m + n) n doubles in the LDS of one workgroup (159 KiB); this matrix does not fit");
  MAUA_REQUIRE(a && ws && s && v, w + ": NULL argument");
  MAUA_REQUIRE(((size_t)ws & 255) == 0 && ws_bytes >= (long)scratch_bytes(svd_ws, m, n),
               w + ": the workspace must be 256-byte aligned and hold " + (w == "maua_eigh_f64" ? "maua_eigh_f64_workspace_bytes" : "maua_svd_f64_workspace_bytes") +
                   "() bytes");
  return MAUA_OK;
}

// the Jacobi iteration and the finish on a loaded workspace.  reverse: ascending output (eigh).  MAUA_ERR after the outputs are written
// when max_sweeps sweeps did not reach a sweep without rotations.
int jacobi_run(hipStream_t st, const SvdWs& w, int m, int n, int path, int max_sweeps, bool use_shift, bool reverse, double* S, double* U,
               double* V, int* sweeps_out, int* rotations_out, const char* who) {
  const int mp = even_up(m), np = even_up(n), N = n + (n & 1);
  const double tol = std::sqrt((double)m) * kEps;
  if (max_sweeps == 0) max_sweeps = kSvdMaxSweeps;
  if (path == 0) path = resident_bytes(m, n) <= kLdsBudget ? 1 : 2;
  int info[2] = {0, 0};
  if (path == 1) {
    const size_t smem = (size_t)resident_bytes(m, n);
    MAUA_HIP_CHECK(hipFuncSetAttribute((const void*)jacobi_resident_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
    hipLaunchKernelGGL(jacobi_resident_kernel, dim3(1), dim3(kResidentThreads), smem, st, w.At, w.Vt, m, n, mp, np, max_sweeps, tol, w.info);
    MAUA_HIP_CHECK(hipGetLastError());
    MAUA_HIP_CHECK(hipMemcpyAsync(info, w.info, sizeof(info), hipMemcpyDeviceToHost, st));
    MAUA_HIP_CHECK(hipStreamSynchronize(st));
  } else {
    const int staged = (long)2 * mp * 8 <= kStageBudget;
    const size_t smem = staged ? (size_t)2 * mp * 8 : 0;
    if (smem > 48 * 1024)
      MAUA_HIP_CHECK(hipFuncSetAttribute((const void*)jacobi_pair_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
    MAUA_HIP_CHECK(hipMemsetAsync(w.rotated, 0, sizeof(int) * (N / 2), st));
    for (int sweep = 0; sweep < max_sweeps; sweep++) {
      for (int r = 0; r < N - 1; r++)
        hipLaunchKernelGGL(jacobi_pair_kernel, dim3(N / 2), dim3(kPairThreads), smem, st, w.At, w.Vt, m, n, mp, np, N, r, staged, tol, w.rotated);
      hipLaunchKernelGGL(jacobi_count_kernel, dim3(1), dim3(256), 0, st, w.rotated, N / 2, w.info);
      MAUA_HIP_CHECK(hipGetLastError());
      MAUA_HIP_CHECK(hipMemcpyAsync(&info[1], w.info, sizeof(int), hipMemcpyDeviceToHost, st));
      MAUA_HIP_CHECK(hipStreamSynchronize(st));
      info[0] = sweep + 1;
      if (info[1] == 0) break;
    }
  }
  if (sweeps_out) *sweeps_out = info[0];
  if (rotations_out) *rotations_out = info[1];
  // sigma and the signs per column; the order on the host: descending, stable (ties: the lower column first); eigh reads it backwards
  hipLaunchKernelGGL(jacobi_column_kernel, dim3(n), dim3(64), 0, st, (const double*)w.At, (const double*)w.Vt, n, mp, np, w.sigma, w.sign);
  MAUA_HIP_CHECK(hipGetLastError());
  std::vector<double> sigma(n);
  MAUA_HIP_CHECK(hipMemcpyAsync(sigma.data(), w.sigma, sizeof(double) * n, hipMemcpyDeviceToHost, st));
  MAUA_HIP_CHECK(hipStreamSynchronize(st));
  std::vector<int> order(n);
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return sigma[x] > sigma[y]; });
  if (reverse) std::reverse(order.begin(), order.end());
  MAUA_HIP_CHECK(hipMemcpyAsync(w.order, order.data(), sizeof(int) * n, hipMemcpyHostToDevice, st));
  const long elems = (long)m * n;
  hipLaunchKernelGGL(jacobi_emit_kernel, dim3((unsigned)((elems + 255) / 256)), dim3(256), 0, st, (const double*)w.At, (const double*)w.Vt, m, n, mp,
                     np, (const double*)w.sigma, (const double*)w.sign, (const int*)w.order, use_shift ? (const double*)w.shift : nullptr, S, U, V);
  MAUA_HIP_CHECK(hipGetLastError());
  MAUA_HIP_CHECK(hipStreamSynchronize(st));    // `order` leaves scope
  if (info[1] != 0)
    return fail(std::string(who) + ": no sweep without rotations within " + std::to_string(max_sweeps) + " sweeps (the last one rotated " +
                std::to_string(info[1]) + " pairs); the outputs hold the last iterate");
  return MAUA_OK;
}

void jacobi_load(hipStream_t st, const SvdWs& w, const double* a, long lda, int m, int n, bool use_shift) {
  const int mp = even_up(m), np = even_up(n);
  const long elems = (long)n * mp + (long)n * np;
  hipLaunchKernelGGL(jacobi_load_kernel, dim3((unsigned)((elems + 255) / 256)), dim3(256), 0, st, a, lda, m, n, mp, np,
                     use_shift ? (const double*)w.shift : nullptr, w.At, w.Vt);
}

}  // namespace
}  // namespace maua

using namespace maua;

extern "C" {

int maua_jacobi_schedule(int n, int round, int* pairs, int* n_pairs) {
  MAUA_REQUIRE(n >= 1 && n <= kSvdMaxN, "maua_jacobi_schedule: n must be 1 .. 4096");
  const int N = n + (n & 1);
  MAUA_REQUIRE(round >= 0 && round < N - 1, "maua_jacobi_schedule: a sweep of n columns has N - 1 rounds, N = n rounded up to even");
  MAUA_REQUIRE(pairs && n_pairs, "maua_jacobi_schedule: NULL argument");
  int count = 0;
  for (int i = 0; i < N / 2; i++) {
    int p, q;
    jacobi_pair(N, round, i, &p, &q);
    if (p >= n || q >= n) continue;
    pairs[2 * count] = p;
    pairs[2 * count + 1] = q;
    count++;
  }
  *n_pairs = count;
  return MAUA_OK;
}

long maua_svd_f64_workspace_bytes(int m, int n) {
  if (n < 1 || m < n || n > kSvdMaxN || m > kSvdMaxM) return 0;
  return (long)scratch_bytes(svd_ws, m, n);
}

int maua_svd_f64_check(const double* a, int m, int n, long lda, int want_u, int path, int max_sweeps, const void* ws, long ws_bytes, const double* s,
                       const double* u, const double* v) {
  if (svd_check("maua_svd_f64", a, m, n, lda, path, max_sweeps, ws, ws_bytes, s, v) != MAUA_OK) return MAUA_ERR;
  MAUA_REQUIRE(!want_u || u, "maua_svd_f64: want_u needs u");
  return MAUA_OK;
}

int maua_svd_f64(maua_ctx* ctx, const double* a, int m, int n, long lda, int want_u, int path, int max_sweeps, void* ws, long ws_bytes, double* s,
                 double* u, double* v, int* sweeps, int* last_rotations) {
  MAUA_REQUIRE(ctx, "maua_svd_f64: ctx is NULL");
  if (maua_svd_f64_check(a, m, n, lda, want_u, path, max_sweeps, ws, ws_bytes, s, u, v) != MAUA_OK) return MAUA_ERR;
  Scratch place(ws);
  const SvdWs w = svd_ws(place, m, n);
  jacobi_load(ctx->stream, w, a, lda, m, n, false);
  MAUA_HIP_CHECK(hipGetLastError());
  return jacobi_run(ctx->stream, w, m, n, path, max_sweeps, false, false, s, want_u ? u : nullptr, v, sweeps, last_rotations, "maua_svd_f64");
}

long maua_eigh_f64_workspace_bytes(int n) { return maua_svd_f64_workspace_bytes(n, n); }

int maua_eigh_f64_check(const double* s, int n, long lds, int path, int max_sweeps, const void* ws, long ws_bytes, const double* w, const double* q) {
  return svd_check("maua_eigh_f64", s, n, n, lds, path, max_sweeps, ws, ws_bytes, w, q);
}

int maua_eigh_f64(maua_ctx* ctx, const double* s, int n, long lds, int path, int max_sweeps, void* ws, long ws_bytes, double* w, double* q, int* sweeps,
                  int* last_rotations) {
  MAUA_REQUIRE(ctx, "maua_eigh_f64: ctx is NULL");
  if (maua_eigh_f64_check(s, n, lds, path, max_sweeps, ws, ws_bytes, w, q) != MAUA_OK) return MAUA_ERR;
  Scratch place(ws);
  const SvdWs k = svd_ws(place, n, n);
  hipStream_t st = ctx->stream;
  hipLaunchKernelGGL(gershgorin_rows_kernel, dim3(n), dim3(64), 0, st, s, lds, n, k.rows);
  hipLaunchKernelGGL(gershgorin_max_kernel, dim3(1), dim3(64), 0, st, (const double*)k.rows, n, k.shift);
  jacobi_load(st, k, s, lds, n, n, true);
  MAUA_HIP_CHECK(hipGetLastError());
  return jacobi_run(st, k, n, n, path, max_sweeps, true, true, w, nullptr, q, sweeps, last_rotations, "maua_eigh_f64");
}

}  // extern "C"
