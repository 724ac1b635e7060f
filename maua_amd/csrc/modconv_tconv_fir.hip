// Minimal-MAC up-layer in ONE kernel: t = conv_transpose2d(x * s, W, stride 2) on the matrix cores, the 4 x 4 FIR and the
// layer epilogue straight from the workgroup's LDS tile of t - the (2H+1) x (2W+1) tensor never reaches HBM.
//
// Replaces (reference): ops.py:211-225 (conv2d_resample, up = 2: conv_transpose2d, then upfirdn2d pad 1 gain 4) + :184-185
// noise + :65-84 bias_act, i.e. what modconv_tconv_dma.hip + upfir.hip do in two launches with t written and re-read
// (round 2: the pair ran at 2.6x its algorithmic bytes; the 256^2 -> 512^2 layer alone was 12 % of the step).
//
// A workgroup computes t for 8 x 32 positions x 32 channels exactly like tconv_dma_kernel (same K loop, same LDS-direct
// pipeline, same accumulation order: t is bit-identical), leaves the tile in LDS as bf16 - the rounding the HBM tensor had -
// and evaluates the FIR + epilogue with upfir_epilogue_kernel's arithmetic (same operation order: the layer output is
// bit-identical to the two-launch path).  An output pixel needs t rows Y-1 .. Y+2 and columns X-1 .. X+2.  Zero halo pixels on
// every side make positions outside the image (and the thin last row / column of positions, which the two-launch path needs an
// extra kernel for) come out right by themselves.  Two forms share every line of the K loop, the tile write and the FIR:
//
// Tile form (WALK = false).  One workgroup, one tile: 16 x 64 t values yield 12 x 60 outputs, so tiles advance by 6 x 30 positions
// and overlap by a one-position frame that is recomputed, not exchanged: 8 / 6 x 32 / 30 = 1.42x the transposed convolution's MACs,
// and the LDS-direct weight / halo pieces and the halo re-fetch with them.
//
// Walk form (WALK = true, the default: synth option "tconv_walk").  A workgroup keeps its 30-column strip and walks down it in steps
// of 8 NEW position rows: 32 / 30 of the MACs.  A step runs the unchanged K loop, writes its 16 x 64 t tile, and evaluates the 16
// output rows 2 P0 - 2 .. 2 P0 + 13 (P0 = its first position row), which read the t rows 2 P0 - 3 .. 2 P0 + 15: the tile and the
// last three t rows of the step above.  Those are carried as the bf16 t VALUES (what the two-launch path keeps in HBM: nothing new is
// rounded) - 3 x 64 x 32 x 2 B = 12 KB per workgroup = three 16-byte pieces per thread, read from the tile behind the FIR phase, held
// in 12 VGPRs across the next K loop (when LDS is full of K buffers, 73 KB) and written back in front of the next tile as its position
// rows -2, -1 (when the K buffers are dead): 64 + 16 = 80 KB, two workgroups per CU as before.  The carry is zero above the image.
// A strip is cut into row segments (host: tconv_walk_plan); a lower segment starts with one warm-up step - the step above its first,
// outputs masked - that builds its carry.  Per step, not per workgroup: the halo sources and the zeroing of out-of-image halo pixels
// (the t tile overwrites the K buffers), the noise values and the per-channel vectors (24 registers held across the K loop would
// spill; they are L2 hits requested ahead like the noise).  Every step drains its K loop, so each starts on buffer 0 and an odd
// Ci / 32 needs no parity.  The step loop would let the compiler keep ~50 per-thread addresses (tile write, FIR columns, halo
// sources) as loop invariants in registers across the K loop (measured: 196 .. 236 bytes / lane of scratch); an opaque copy of the
// thread index per step keeps them local (256 VGPRs, no scratch).  Measured at B = 128 on the 256^2 -> 512^2 layer (two segments:
// 34 steps per strip where the tile form runs 43 tile rows, 0.79x the MFMAs and 0.79x the fetched bytes by the counters):
// 3.31 -> 3.11 ms, the step 27.64 -> 27.39 ms.  History: a round-3 walk that carried the rows as f32 horizontal sums (48 VGPRs)
// spilled 228 bytes / lane and measured 4.20 vs 3.48 ms; 16-row tiles (one workgroup per CU) 3.78 vs 3.50 ms.
#include "common.h"
#include "internal.h"
#include "mma.h"
#include "modconv_tconv.h"

namespace maua {

namespace {

constexpr int PTW = 32;                            // position columns per workgroup (rows: template parameter, 8 or 16)
constexpr int HW1 = PTW + 1;                       // halo columns
constexpr int KB = 64;                             // bytes of K per LDS row (32 bf16 channels = one chunk)
constexpr int WROWS = 9 * 32;
constexpr int WBUF = WROWS * KB;
constexpr int OFF_H = 2 * WBUF;
constexpr int ES = 128 * 2;                        // t tile: [position][class * 32 + ch] bf16, row stride (unpadded: XOR-swizzled)

// The t tile, [position p = (tr >> 1) * 32 + (tc >> 1)][class (tr & 1) * 2 + (tc & 1)][32 channels] bf16, rows of 256 bytes
// swizzled on two levels (round 5; the padded 272-byte rows of rounds 3-4 had 35 % of this kernel's LDS cycles in conflicts):
//   the 64-byte class block sits at slot  cls ^ (p & 3)        - the four 2-column strips of a ds_read_b128 lane group differ in p & 3
//   its 16-byte piece pc at               pc ^ ((p >> 2) & 3)  - 16 consecutive positions of a ds_write_b64 lane group take the 16
//                                                                 (slot, piece) combinations: both sides conflict-free
// column part of the byte offset of piece pc of t[.][tc]; the row part is (tr >> 1) * 32 * ES and XOR ((tr & 1) << 7)
__device__ __forceinline__ int t_col(int tc, int pc) {
  const int p = tc >> 1;
  return p * ES + ((((tc & 1) ^ (p & 3)) << 6) | ((pc ^ ((p >> 2) & 3)) << 4));
}

// the two horizontal [1,3,3,1] sums of one t row for the output columns xl, xl + 1 (upfir_hrow's arithmetic); tcol[rx] =
// t_col(xl - 1 + rx, pc)
template <typename F>
__device__ __forceinline__ void fir_hrow(const char* tile, int tr, const int (&tcol)[5], f32x2_t (&h)[2][4]) {
  f32x2_t c[5][4];
  const int rowb = (tr >> 1) * (PTW * ES), rsw = (tr & 1) << 7;
#pragma unroll
  for (int rx = 0; rx < 5; rx++) {
    const u32x4 v = *reinterpret_cast<const u32x4*>(tile + rowb + (tcol[rx] ^ rsw));
#pragma unroll
    for (int k = 0; k < 4; k++) c[rx][k] = f32x2_t{Fmt16<F>::lo(v[k]), Fmt16<F>::hi(v[k])};
  }
#pragma unroll
  for (int e = 0; e < 4; e++) {
    h[0][e] = (c[0][e] + c[3][e]) + 3.f * (c[1][e] + c[2][e]);
    h[1][e] = (c[1][e] + c[4][e]) + 3.f * (c[2][e] + c[3][e]);
  }
}

}  // namespace

// PTH_ = 8: 4 waves, 73 KB of LDS (walk: 80), two workgroups per CU; tile form: 6 x 30 useful positions of 8 x 32 (1.42x MACs), walk: 8 x 30.
// The tile form is written for any even PTH_; PTH_ = 16 (8 waves, 136 KB, ONE workgroup per CU, 14 x 30 of 16 x 32 = 1.22x MACs) measured
// 3.78 vs 3.50 ms on the 256^2 -> 512^2 layer at B = 128 - two workgroups out of phase are worth more than the saved rows.
template <int PTH_, typename F, bool WALK>
__global__ __launch_bounds__(PTH_ * 32, PTH_ == 8 ? 2 : 1) void tconv_fir_kernel(ConvArgs a, UpfirArgs u, int nseg, int seg_steps) {
  constexpr int PTH = PTH_, UPR = PTH - 2;           // position rows computed / useful (tile form)
  static_assert(!WALK || PTH_ == 8, "the walk carries three t rows of a 16-row tile");
  constexpr int HPX = (PTH + 1) * HW1, HBUF = HPX * KB;
  constexpr int NW = PTH / 2, NT = NW * 64;
  constexpr int WJ = (WBUF / 1024 + NW - 1) / NW, HJ = (HPX * 4 + NT - 1) / NT;
  constexpr int FG = NT / 128, FROWS = (WALK ? 2 * PTH : 2 * UPR) / FG;  // FIR thread groups of 120, output rows per group (6 or 7; walk: 8)
  static_assert(FG * FROWS == (WALK ? 2 * PTH : 2 * UPR), "output rows must split evenly over the FIR groups");
  constexpr int OFF_T = WALK ? 2 * PTW * ES : 0;     // the t tile; the walk keeps position rows -2, -1 (the carried t rows -3 .. -1) in front of it
  extern __shared__ __attribute__((aligned(1024))) char smem[];
  const unsigned lds0 = __builtin_amdgcn_readfirstlane(lds_off(smem));
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, h = lane >> 5;
  // Workgroup order (1-D grid): the dispatcher places block L on XCD L % 8, each XCD has its own L2.  The channel
  // blocks of one (tile, sample) read the same input halo, so they run back to back ON ONE XCD (cb fastest inside an
  // XCD, in groups of <= 8 blocks = <= 2.4 MB of weights, which stay L2-resident next to the halos): x is fetched from
  // HBM once per group instead of once per channel block.  Placement is a speed matter only.
  const int tiles_x = (a.W + 29) / 30, tiles = tiles_x * (WALK ? nseg : (a.H + UPR - 1) / UPR), CB = a.Co >> 5;
  const int cbg = CB < 8 ? CB : 8, n_ts = tiles * a.B, per_group = ((n_ts + 7) >> 3) * 8 * cbg;
  const int L = blockIdx.x, grp = L / per_group, Lg = L - grp * per_group;
  const int xcd = Lg & 7, idx = Lg >> 3;
  const int cb = grp * cbg + idx % cbg, ts = (idx / cbg) * 8 + xcd;
  if (ts >= n_ts) return;
  const int b = ts / tiles, tile = ts - b * tiles;
  const int tyi = tile / tiles_x, txi = tile - tyi * tiles_x;
  const int tx0 = txi * 30 - 1;   // first position column of the tile (a one-position frame around 30)
  // walk: segment tyi of the strip.  The strip has n_steps steps of 8 position rows; segment 0 takes the first seg_steps of them, every
  // later one seg_steps - 1 behind a warm-up step (the step above its first, outputs masked) that builds its carry: seg_steps each.
  // The segment owns the output rows [y_lo, y_hi): a step at position row P0 yields the rows 2 P0 - 2 .. 2 P0 + 13.
  int step = 0, step_end = 1, y_lo = 0, y_hi = 2 * a.H;
  if (WALK) {
    const int n_steps = (a.H >> 3) + 1, s0 = tyi ? seg_steps + (tyi - 1) * (seg_steps - 1) : 0;
    step_end = min(n_steps, tyi ? s0 + seg_steps - 1 : seg_steps);
    step = tyi ? s0 - 1 : 0;
    y_lo = tyi ? 16 * s0 - 2 : 0;
    if (step_end < n_steps) y_hi = 16 * step_end - 2;
  }
  const char* xb = reinterpret_cast<const char*>(a.x) + (long)b * a.x_bstride * 2;
  const char* wp = reinterpret_cast<const char*>(a.w);

  // weight sources: LDS row R = 32 k + n of the chunk's [288][64 B] image <- global row of block k, channel n
  unsigned woff[WJ];
#pragma unroll
  for (int j = 0; j < WJ; j++) {
    const int ii = wave + NW * j;
    const int R = min(16 * ii + (lane >> 2), WROWS - 1);
    const int k = R >> 5, n = R & 31;
    const int q = (lane & 3) ^ tconv_swz(R);
    woff[j] = (unsigned)((((((kTconvSlot[k] * CB + cb) * 4 + kTconvCls[k]) * 32 + n) * a.Ci) + q * 8) * 2);
  }
#define TD_ISSUE(C_, BUF_)                                                                               \
  {                                                                                                      \
    const char* ws_ = wp + (long)(C_) * KB;                                                              \
    _Pragma("unroll") for (int j = 0; j < WJ; j++)                                                      \
      if (wave + NW * j < WBUF / 1024) dma16_s(ws_, woff[j], lds0 + (BUF_) * WBUF + (wave + NW * j) * 1024); \
    const char* xs_ = xb + (long)(C_) * KB;                                                              \
    _Pragma("unroll") for (int j = 0; j < HJ; j++)                                                      \
      if (hoff[j] != 0xffffffffu) dma16_s(xs_, hoff[j], lds0 + OFF_H + (BUF_) * HBUF + (wave + NW * j) * 1024); \
  }

  // fragment addresses.  A: halo pixel of (local row 2 wave + R, column r) under shift (p, q) = row + 1 - p, r + 1 - q
  const int hp00 = (2 * wave) * HW1 + r;   // halo row 2 wave, halo column r  (= shift (1,1) of the wave's first row)
  const unsigned b0 = (unsigned)(r * KB + ((tconv_swz(r) ^ h) << 4));
#define TD_A(HR_, Q1_, KS_, BUF_)                                                                                              \
  ({                                                                                                                           \
    const int hp_ = hpv + (HR_) * HW1 + (Q1_);                                                                                 \
    *reinterpret_cast<const u32x4*>(smem + ((OFF_H + (BUF_) * HBUF + hp_ * KB + ((tconv_swz(hp_) ^ h) << 4)) ^ ((KS_) << 5))); \
  })
#define TD_B(K_, KS_, BUF_) (*reinterpret_cast<const u32x4*>(smem + (BUF_) * WBUF + (K_) * 32 * KB + (b0 ^ ((KS_) << 5))))

  // walk: the t rows 13 .. 15 of a step's tile are the rows -3 .. -1 of the next: 12 KB per workgroup, three 16-byte pieces per thread
  // (pieces 0, 1: position row 7 = t rows 14, 15; piece 2: the t row 13 half of position row 6, which the class swizzle puts into the
  // upper 128 bytes of a position whose p & 2 is clear and into the lower 128 of the others).  Zero above the image and above a warm-up step.
  u32x4 carry[3] = {u32x4{0u, 0u, 0u, 0u}, u32x4{0u, 0u, 0u, 0u}, u32x4{0u, 0u, 0u, 0u}};
  const int n_chunks = a.Ci >> 5;
  do {
  // (the step loop must not turn the per-thread addresses of the halo sources, the tile write and the FIR into loop invariants that
  // stay in registers across the K loop: each of the three starts from a thread index the compiler cannot see through)
  int tidh = tid;
  if (WALK) asm volatile("" : "+v"(tidh));
  const int ty0 = WALK ? 8 * step : tyi * UPR - 1;   // first position row of the tile (tile form: a one-position frame around UPR)
  // halo sources (pixels outside the image are never loaded: zeroed; per step, because the t tile overwrites the buffers)
  unsigned hoff[HJ];
#pragma unroll
  for (int j = 0; j < HJ; j++) {
    const int P = (wave + NW * j) * 64 + (tidh & 63);
    const int hp = P >> 2, q = (P & 3) ^ tconv_swz(hp);
    const int py = (hp * 1986) >> 16;  // hp / 33 for hp < 561
    const int px = hp - py * HW1;
    const int gy = ty0 - 1 + py, gx = tx0 - 1 + px;
    hoff[j] = 0xffffffffu;
    if (P < HPX * 4) {
      if (gy >= 0 && gx >= 0 && gy < a.H && gx < a.W) {
        hoff[j] = (unsigned)(((gy * a.W + gx) * a.Ci + q * 8) * 2);
      } else {
        *reinterpret_cast<u32x4*>(smem + OFF_H + P * 16) = u32x4{0u, 0u, 0u, 0u};
        *reinterpret_cast<u32x4*>(smem + OFF_H + HBUF + P * 16) = u32x4{0u, 0u, 0u, 0u};
      }
    }
  }
  f32x16 acc[2][4];
#pragma unroll
  for (int R = 0; R < 2; R++)
#pragma unroll
    for (int c = 0; c < 4; c++)
#pragma unroll
      for (int e = 0; e < 16; e++) acc[R][c][e] = 0.f;

  // (every step drains its K loop, so every step starts on buffer 0 whatever the parity of Ci / 32)
  TD_ISSUE(0, 0)
  if (n_chunks > 1) TD_ISSUE(1, 1)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  int hpv = hp00;
  // one k-step: 6 halo fragments (rows 2w .. 2w+2 of the halo x column shifts q = 1, 0), 9 weight fragments, 18 MFMAs;
  // per class the taps accumulate in the order of tconv2_kernel (shift slots 0, 1, 2, 3)
#define TD_STEP(KS_, BUF_)                                                                                            \
  {                                                                                                                   \
    u32x4 A00 = TD_A(0, 0, KS_, BUF_), A01 = TD_A(0, 1, KS_, BUF_);   /* halo row 2w:   q = 1, q = 0 */               \
    u32x4 A10 = TD_A(1, 0, KS_, BUF_), A11 = TD_A(1, 1, KS_, BUF_);   /* halo row 2w+1 */                             \
    u32x4 A20 = TD_A(2, 0, KS_, BUF_), A21 = TD_A(2, 1, KS_, BUF_);   /* halo row 2w+2 */                             \
    {                                                                                                                 \
      const u32x4 B0 = TD_B(0, KS_, BUF_), B1 = TD_B(1, KS_, BUF_), B2 = TD_B(2, KS_, BUF_);                          \
      Mma<F>::step(acc[0][0], B0, A00); Mma<F>::step(acc[1][0], B0, A10);   /* shift (1,1) */                         \
      Mma<F>::step(acc[0][1], B2, A01); Mma<F>::step(acc[1][1], B2, A11);   /* shift (1,0), class 1 */                \
      Mma<F>::step(acc[0][0], B1, A01); Mma<F>::step(acc[1][0], B1, A11);   /* shift (1,0), class 0 */                \
    }                                                                                                                 \
    {                                                                                                                 \
      const u32x4 B3 = TD_B(3, KS_, BUF_), B4 = TD_B(4, KS_, BUF_);                                                   \
      Mma<F>::step(acc[0][2], B4, A10); Mma<F>::step(acc[1][2], B4, A20);   /* shift (0,1), class 2 */                \
      Mma<F>::step(acc[0][0], B3, A10); Mma<F>::step(acc[1][0], B3, A20);   /* shift (0,1), class 0 */                \
    }                                                                                                                 \
    {                                                                                                                 \
      const u32x4 B5 = TD_B(5, KS_, BUF_), B6 = TD_B(6, KS_, BUF_), B7 = TD_B(7, KS_, BUF_), B8 = TD_B(8, KS_, BUF_); \
      Mma<F>::step(acc[0][3], B8, A11); Mma<F>::step(acc[1][3], B8, A21);   /* shift (0,0) */                         \
      Mma<F>::step(acc[0][1], B6, A11); Mma<F>::step(acc[1][1], B6, A21);                                             \
      Mma<F>::step(acc[0][2], B7, A11); Mma<F>::step(acc[1][2], B7, A21);                                             \
      Mma<F>::step(acc[0][0], B5, A11); Mma<F>::step(acc[1][0], B5, A21);                                             \
    }                                                                                                                 \
  }
  for (int c = 0; c < n_chunks; c++) {
    const int buf = c & 1;
    asm volatile("" : "+v"(hpv));  // (keeps the fragment addresses out of loop-invariant registers)
    TD_STEP(0, buf)
    // the chunk's last fragment reads are issued inside the next step; the barrier that frees the buffers comes after
    // they have returned, so it splits that step by hand: loads, wait, barrier, refill, MFMAs
    {
      u32x4 A00 = TD_A(0, 0, 1, buf), A01 = TD_A(0, 1, 1, buf), A10 = TD_A(1, 0, 1, buf), A11 = TD_A(1, 1, 1, buf);
      u32x4 A20 = TD_A(2, 0, 1, buf), A21 = TD_A(2, 1, 1, buf);
      const u32x4 B0 = TD_B(0, 1, buf), B1 = TD_B(1, 1, buf), B2 = TD_B(2, 1, buf), B3 = TD_B(3, 1, buf), B4 = TD_B(4, 1, buf);
      const u32x4 B5 = TD_B(5, 1, buf), B6 = TD_B(6, 1, buf), B7 = TD_B(7, 1, buf), B8 = TD_B(8, 1, buf);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // chunk c+1 (issued one chunk ago) has landed
      __syncthreads();                                  // ... for everybody; chunk c's buffers are free
      if (c + 2 < n_chunks) TD_ISSUE(c + 2, buf)
      Mma<F>::step(acc[0][0], B0, A00); Mma<F>::step(acc[1][0], B0, A10);
      Mma<F>::step(acc[0][1], B2, A01); Mma<F>::step(acc[1][1], B2, A11);
      Mma<F>::step(acc[0][0], B1, A01); Mma<F>::step(acc[1][0], B1, A11);
      Mma<F>::step(acc[0][2], B4, A10); Mma<F>::step(acc[1][2], B4, A20);
      Mma<F>::step(acc[0][0], B3, A10); Mma<F>::step(acc[1][0], B3, A20);
      Mma<F>::step(acc[0][3], B8, A11); Mma<F>::step(acc[1][3], B8, A21);
      Mma<F>::step(acc[0][1], B6, A11); Mma<F>::step(acc[1][1], B6, A21);
      Mma<F>::step(acc[0][2], B7, A11); Mma<F>::step(acc[1][2], B7, A21);
      Mma<F>::step(acc[0][0], B5, A11); Mma<F>::step(acc[1][0], B5, A21);
    }
  }
  // ---- the epilogue's global operands are requested BEFORE the tile is written: per-channel vectors (every step: 24 registers
  // held across the K loop would spill) and the thread's noise values (one float2 per output row) are in flight across the two barriers and the first three
  // FIR rows instead of being waited for row by row (every wait would also have drained the row's stores: 6 exposed round trips per
  // thread, 1.88 of the kernel's 3.5 ms).
  int tidf = tid;
  if (WALK) asm volatile("" : "+v"(tidf));
  // FIR + epilogue threads: a thread owns a 2-column strip x one 16-byte channel piece and walks FROWS output rows: 30 strips x 4
  // pieces x 2 row halves.  Local t row / column 0 = global t row 2 ty0 / column 2 tx0; local output (yl, xl) = global (2 ty0 + yl,
  // 2 tx0 + xl) reads local t rows yl-1 .. yl+2.  Tile form: yl in [2, 14); walk: yl in [-2, 14), rows -3 .. -1 are the carry.
  const int fhalf = tidf / 120, fw = tidf - fhalf * 120;
  const int strip = fw >> 2, pc = fw & 3;
  const int xl = 2 + 2 * strip, yl0 = (WALK ? -2 : 2) + FROWS * fhalf;
  const int X = 2 * tx0 + xl, Wo = 2 * a.W;
  const int cho = cb * 32 + pc * 8;
  const bool fir_on = tidf < 120 * FG && X < Wo;
  f32x2_t dv[4], bv[4], sv[4];
  auto load_channel_vectors = [&]() {
#pragma unroll
    for (int e4 = 0; e4 < 8; e4 += 4) {
      const float4 s4 = u.out_scale ? *reinterpret_cast<const float4*>(u.out_scale + (long)b * a.Co + cho + e4)
                                    : make_float4(1.f, 1.f, 1.f, 1.f);
      sv[e4 / 2] = f32x2_t{s4.x, s4.y}; sv[e4 / 2 + 1] = f32x2_t{s4.z, s4.w};
      const float4 d4 = u.d ? *reinterpret_cast<const float4*>(u.d + (long)b * a.Co + cho + e4) : make_float4(1.f, 1.f, 1.f, 1.f);
      const float4 b4 = u.bias ? *reinterpret_cast<const float4*>(u.bias + cho + e4) : make_float4(0.f, 0.f, 0.f, 0.f);
      dv[e4 / 2] = f32x2_t{d4.x, d4.y}; dv[e4 / 2 + 1] = f32x2_t{d4.z, d4.w};
      bv[e4 / 2] = f32x2_t{b4.x, b4.y}; bv[e4 / 2 + 1] = f32x2_t{b4.z, b4.w};
    }
  };
  const int coff2 = (tidf >> 3) * ES + (((tidf >> 3) & 2) ? 0 : 128) + (tidf & 7) * 16;
  const bool fir_step = !WALK || 16 * step + 14 > y_lo;   // (a warm-up step owns none of its output rows)
  float2 nzv[FROWS];
#pragma unroll
  for (int k = 0; k < FROWS; k++) nzv[k] = make_float2(0.f, 0.f);
  if (fir_on && fir_step) {
    load_channel_vectors();
    if (u.noise) {
      const float* nb = u.noise + (long)b * u.noise_bstride;
#pragma unroll
      for (int k = 0; k < FROWS; k++) {
        const int Y = 2 * ty0 + yl0 + k;
        if (Y >= y_lo && Y < y_hi) nzv[k] = *reinterpret_cast<const float2*>(nb + (long)Y * Wo + X);
      }
    }
  }
  // ---- t tile -> LDS [position][class * 32 + ch] as bf16 (the rounding of the two-launch path's HBM tensor)
  __syncthreads();
  char* tt = smem + OFF_T;
  const int rt = tidf & 31, ht = (tidf >> 5) & 1;
#pragma unroll
  for (int R = 0; R < 2; R++) {
    const int m = (2 * wave + R) * 32 + rt;   // (m & 3 = r & 3, (m >> 2) & 3 = (r >> 2) & 3: the swizzle terms are per-lane constants)
#pragma unroll
    for (int c = 0; c < 4; c++)
#pragma unroll
      for (int qd = 0; qd < 4; qd++)
        *reinterpret_cast<uint2*>(tt + m * ES + (((c ^ (rt & 3)) << 6) | ((qd ^ ((rt >> 2) & 3)) << 4) | (ht << 3))) =
            make_uint2(Fmt16<F>::pack2(acc[R][c][qd * 4 + 0], acc[R][c][qd * 4 + 1]), Fmt16<F>::pack2(acc[R][c][qd * 4 + 2], acc[R][c][qd * 4 + 3]));
  }
  if (WALK) {   // the carried rows, in front of the tile
    *reinterpret_cast<u32x4*>(smem + PTW * ES + tidf * 16) = carry[0];
    *reinterpret_cast<u32x4*>(smem + PTW * ES + 4096 + tidf * 16) = carry[1];
    *reinterpret_cast<u32x4*>(smem + coff2) = carry[2];
  }
  __syncthreads();
  // ---- FIR + epilogue (upfir_epilogue_kernel's arithmetic)
  {
    if (fir_on && fir_step) {
#pragma unroll
      for (int e = 0; e < 4; e++) { dv[e] *= 0.0625f * u.gain; bv[e] *= u.gain; }
      const float nzs = u.noise_strength * u.gain * (u.noise_scale ? u.noise_scale[b] : 1.f);
      const float cl = u.clamp >= 0.f ? u.clamp : 3.0e38f;
      char* yb = reinterpret_cast<char*>(u.y) + (long)b * (2 * a.H) * Wo * a.Co * 2;
      int tcol[5];
#pragma unroll
      for (int rx = 0; rx < 5; rx++) tcol[rx] = t_col(xl - 1 + rx, pc);
      f32x2_t hr[4][2][4];
      fir_hrow<F>(tt, yl0 - 1, tcol, hr[0]);
      fir_hrow<F>(tt, yl0, tcol, hr[1]);
      fir_hrow<F>(tt, yl0 + 1, tcol, hr[2]);
#pragma unroll
      for (int k = 0; k < FROWS; k++) {
        fir_hrow<F>(tt, yl0 + k + 2, tcol, hr[(k + 3) & 3]);
        const int Y = 2 * ty0 + yl0 + k;
        if (Y >= y_lo && Y < y_hi) {
          const float nz[2] = {nzv[k].x * nzs, nzv[k].y * nzs};
#pragma unroll
          for (int j = 0; j < 2; j++) {
            f32x2_t o[4];
#pragma unroll
            for (int e = 0; e < 4; e++) {
              const f32x2_t accv = (hr[k & 3][j][e] + hr[(k + 3) & 3][j][e]) + 3.f * (hr[(k + 1) & 3][j][e] + hr[(k + 2) & 3][j][e]);
              f32x2_t t = accv * dv[e] + (bv[e] + nz[j]);
              const f32x2_t ta = t * u.alpha;
              t = f32x2_t{fmaxf(t[0], ta[0]), fmaxf(t[1], ta[1])};
              o[e] = f32x2_t{__builtin_amdgcn_fmed3f(t[0], -cl, cl), __builtin_amdgcn_fmed3f(t[1], -cl, cl)} * sv[e];
            }
            *reinterpret_cast<u32x4*>(yb + (((long)Y * Wo + X + j) * a.Co + cho) * 2) =
                u32x4{Fmt16<F>::pack2(o[0][0], o[0][1]), Fmt16<F>::pack2(o[1][0], o[1][1]), Fmt16<F>::pack2(o[2][0], o[2][1]), Fmt16<F>::pack2(o[3][0], o[3][1])};
          }
        }
      }
    }
  }
  if (!WALK || ++step >= step_end) break;
  // the last three t rows of this tile are the first three of the next; the barrier frees the tile for the next step's K buffers
  carry[0] = *reinterpret_cast<const u32x4*>(tt + 7 * PTW * ES + tidf * 16);
  carry[1] = *reinterpret_cast<const u32x4*>(tt + 7 * PTW * ES + 4096 + tidf * 16);
  carry[2] = *reinterpret_cast<const u32x4*>(tt + 6 * PTW * ES + coff2);
  __syncthreads();
  } while (true);
#undef TD_ISSUE
#undef TD_A
#undef TD_B
#undef TD_STEP
}

bool tconv_fir_supported(int dtype, int Ci, int Co, int H, int W) {
  return (dtype == MAUA_BF16 || dtype == MAUA_F16) && Ci % 32 == 0 && Co % 32 == 0 && H >= 16 && W >= 32 && (long)H * W * Ci * 2 < (1L << 32) &&
         16L * Co * Ci * 2 < (1L << 32);
}

// what launch_tconv_fir checks before it launches (host only)
int tconv_fir_check(const ConvArgs& a, const UpfirArgs& u, int dtype) {
  MAUA_REQUIRE(tconv_fir_supported(dtype, a.Ci, a.Co, a.H, a.W), "tconv_fir: unsupported shape");
  MAUA_REQUIRE(u.act == MAUA_ACT_LRELU && u.alpha >= 0.f && u.alpha <= 1.f && u.gain > 0.f, "tconv_fir: lrelu epilogue only");
  MAUA_REQUIRE(!u.noise || (((uintptr_t)u.noise % 8) == 0 && u.noise_bstride % 2 == 0), "tconv_fir: noise must be 8-byte aligned");
  const int pth = 8, upr = pth - 2;
  const int tiles = ((a.H + upr - 1) / upr) * ((a.W + 29) / 30), CB = a.Co / 32, cbg = CB < 8 ? CB : 8;
  MAUA_REQUIRE(CB % cbg == 0, "tconv_fir: channel blocks must split into groups of 8");
  const long n_ts = (long)tiles * a.B, grid = ((n_ts + 7) / 8) * 8 * cbg * (CB / cbg);
  MAUA_REQUIRE(grid < (1L << 31), "tconv_fir: grid too large");
  return MAUA_OK;
}

// the walk's row segments: the count that minimises the worst workgroup's step count over the resident slots (two workgroups per CU),
// and the steps per segment.  A strip has n_steps = H / 8 + 1 steps; with seg_steps = ceil((n_steps + segs - 1) / segs) the first segment
// takes seg_steps of them and every later one seg_steps - 1 behind its warm-up step.  force_segs > 0: that many (at most n_steps / 2).
static void tconv_walk_plan(const ConvArgs& a, int slots, int force_segs, int* nseg, int* seg_steps) {
  const int n_steps = a.H / 8 + 1, max_segs = std::max(1, n_steps / 2);
  const long per_seg = (long)a.B * (a.Co / 32) * ((a.W + 29) / 30);
  long best = -1;
  for (int cand = 1; cand <= max_segs; cand++) {
    if (force_segs > 0 && cand != std::min(force_segs, max_segs)) continue;
    const int steps = (n_steps + cand - 1 + cand - 1) / cand;
    const int segs = n_steps > steps ? 1 + (n_steps - steps + steps - 2) / (steps - 1) : 1;   // (none of them empty)
    const long cost = ((per_seg * segs + slots - 1) / slots) * steps;
    if (best < 0 || cost < best) { best = cost; *nseg = segs; *seg_steps = steps; }
  }
}

// the whole up-layer: a = the transposed convolution's arguments (x already multiplied by the styles, w from
// launch_prep_tconv_weights; y unused), u = the FIR / epilogue arguments (t unused; lrelu with 0 <= alpha <= 1, gain > 0).
// walk = 1: the strips are walked downwards (force_segs > 0: in that many row segments); 0: the tile form.  Same bits either way.
int launch_tconv_fir(hipStream_t stream, const ConvArgs& a, const UpfirArgs& u, int dtype, int walk, int force_segs) {
  if (int rc = tconv_fir_check(a, u, dtype)) return rc;
  if (a.B == 0) return MAUA_OK;
  const int pth = 8, upr = pth - 2;
  const int CB = a.Co / 32, cbg = CB < 8 ? CB : 8;
  int nseg = 1, seg_steps = 1;
  if (walk) {
    int dev = 0, cus = 256;
    MAUA_HIP_CHECK(hipGetDevice(&dev));
    MAUA_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    tconv_walk_plan(a, 2 * cus, force_segs, &nseg, &seg_steps);
  }
  const int tiles = (walk ? nseg : (a.H + upr - 1) / upr) * ((a.W + 29) / 30);
  const long n_ts = (long)tiles * a.B, grid = ((n_ts + 7) / 8) * 8 * cbg * (CB / cbg);
  const size_t kbuf = (size_t)2 * WBUF + 2 * (pth + 1) * HW1 * KB;   // the K loop's buffers; then the t tile (walk: + two carried position rows)
  const size_t smem = std::max<size_t>(kbuf, (size_t)(pth + (walk ? 2 : 0)) * PTW * ES);
  auto kern = dtype == MAUA_F16 ? (walk ? tconv_fir_kernel<8, f16_t, true> : tconv_fir_kernel<8, f16_t, false>)
                                : (walk ? tconv_fir_kernel<8, bf16_t, true> : tconv_fir_kernel<8, bf16_t, false>);
  MAUA_HIP_CHECK(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
  hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(256), smem, stream, a, u, nseg, seg_steps);
  MAUA_HIP_CHECK(hipGetLastError());
  return MAUA_OK;
}

}  // namespace maua
