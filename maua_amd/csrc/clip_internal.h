// What the CLIP units pass between them: the piece helpers of their kernels, the residual block both towers run (transformer.hip),
// the image tower's state and passes (clip.hip) as CLIPGrads drives them (clip_guide.hip), and the text tower's state (clip_text.hip).
#pragma once
#include <algorithm>
#include <string>
#include <vector>

#include "common.h"
#include "internal.h"

namespace maua {

// ------------------------------------------------------------------------------------------------ device helpers
template <typename T> struct Pc;   // a 16-byte piece <-> floats
template <> struct Pc<bf16_t> {
  static constexpr int N = 8;
  __device__ static __forceinline__ void load(const bf16_t* p, float* v) {
    const u32x4 u = *reinterpret_cast<const u32x4*>(p);
#pragma unroll
    for (int k = 0; k < 4; k++) { v[2 * k] = bf2f((bf16_t)(u[k] & 0xffffu)); v[2 * k + 1] = __uint_as_float(u[k] & 0xffff0000u); }
  }
  __device__ static __forceinline__ void store(bf16_t* p, const float* v) {
    u32x4 u;
#pragma unroll
    for (int k = 0; k < 4; k++) u[k] = pack2bf(v[2 * k], v[2 * k + 1]);
    *reinterpret_cast<u32x4*>(p) = u;
  }
};
template <> struct Pc<float> {
  static constexpr int N = 4;
  __device__ static __forceinline__ void load(const float* p, float* v) {
    const float4 u = *reinterpret_cast<const float4*>(p);
    v[0] = u.x; v[1] = u.y; v[2] = u.z; v[3] = u.w;
  }
  __device__ static __forceinline__ void store(float* p, const float* v) { *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]); }
};

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ float block_sum(float v, float* red) {   // 256 threads; red: 4 floats of LDS
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

constexpr int LN_MAXP = 8;   // LayerNorm's 16-byte pieces per lane: C <= 64 * 8 * (16 / sizeof(T))

// ------------------------------------------------------------------------------------------------ the residual block (transformer.hip)
struct BlockWeights {   // *_t: the transposes, the image tower's way back (the text tower has none)
  DevBuf w_qkv, w_qkv_t, w_out, w_out_t, w_fc, w_fc_t, w_pr, w_pr_t;        // tower dtype
  DevBuf b_qkv, b_out, b_fc, b_pr, ln1_g, ln1_b, ln2_g, ln2_b;               // float
};
// what a block's forward writes on its way: kept per layer for the way back (image tower), or one set shared by the layers.  x is
// the block's input as the way back reads it (the forward takes its input as an argument); st1 / st2 / lse may be NULL (not kept)
struct BlockActs {
  void *x = nullptr, *qkv = nullptr, *ao = nullptr, *xm = nullptr, *h = nullptr;
  float *st1 = nullptr, *st2 = nullptr, *lse = nullptr;
};
struct BlockRun {
  hipStream_t st;
  int dtype, width, heads;
  long N;             // images / sequences
  int Tk;             // tokens of each
  long rows;          // rows the row-wise kernels (LayerNorm, QuickGELU) cover: N * Tk
  long gemm_rows;     // rows the GEMMs cover (>= rows; the text tower's floor)
  int prefer_dma;     // GemmArgs.prefer_dma; QuickGELU rides on a GEMM's epilogue only with this set, where gemm_dma.hip takes the shape
  int causal;         // AttnArgs.causal
};

void launch_layer_norm(hipStream_t st, int dtype, const void* x, const float* g, const float* b, void* y, float* stats, long rows, int C);
void launch_layer_norm_vjp(hipStream_t st, int dtype, const void* x, const float* stats, const float* g, const void* dy, const void* add,
                           void* dx, long rows, int C, int drop_T);
void launch_quick_gelu(hipStream_t st, int dtype, const void* h, void* a, long count);                       // count: elements
void launch_quick_gelu_vjp(hipStream_t st, int dtype, const void* h, const void* da, void* dh, long count);   // (dh may be da)
// c [M][N] = a [M][K] w^T (+ bias) (+ res) on the run's GEMM route; epi: GemmArgs.epi, asked for only where that route fuses it
int block_gemm(const BlockRun& r, const void* a, long M, int K, const void* w, int N, const float* bias, const void* res, void* c, int epi = 0,
               void* c2 = nullptr, const void* aux = nullptr);
// x -> xn through one block; lno [gemm_rows][w], act [gemm_rows][4 w]: scratch.  The launches report through hipGetLastError
int block_forward(const BlockRun& r, const BlockWeights& l, const void* x, const BlockActs& k, void* lno, void* act, void* xn);
// dx (gradient of the block's output) -> dx (of its input), in place; other, dtmp [rows][w], dqkv [rows][3 w], dwide [rows][4 w], delta: scratch
int block_backward(const BlockRun& r, const BlockWeights& l, const BlockActs& k, void* dx, void* other, void* dqkv, void* dwide, void* dtmp,
                   float* delta);
// host float matrix [R][C] -> device [R][C] in dtype (and optionally its transpose [C][R]); rows permuted by `perm` when given
// (both allocate an empty `dev` and write into a held one)
int upload_matrix(int dtype, size_t esize, const float* h, int R, int C, const int* perm, DevBuf* dev, DevBuf* dev_t);
int upload_vec(const float* h, size_t count, const int* perm, DevBuf* dev);
bool is_block_key(const std::string& s);   // "transformer.resblocks.<i>.<par>"
int load_block(std::vector<BlockWeights>& L, int dtype, size_t esize, int width, int heads, const char* who, const std::string& s,
               const float* host, size_t count, bool with_t);
bool blocks_loaded(const std::vector<BlockWeights>& L);

}  // namespace maua

struct maua_clip {
  maua_ctx* ctx;
  int dtype;
  size_t esize;
  int res, patch, width, layers, heads, E, G, Tk, kp;   // G = res / patch, Tk = G * G + 1 tokens, kp = 3 * patch^2
  // kpp: elements between patch rows = kp rounded up to a multiple of 64 (one rule for both dtypes: the GEMMs take K in 64-byte
  // chunks, the LDS-direct kernel in 64 elements).  p = 16 / 32: kpp == kp (768 / 3072); p = 14: 588 -> 640.  The pad columns of
  // `patches` are zeroed by a kernel when the buffer is (re)allocated and no writer touches them afterwards; conv1.weight's pad
  // columns (and its transpose's pad rows) are zeros, so the backward GEMM writes zeros there and the readers stop at kp.
  int kpp;
  maua::DevBuf w_conv, w_conv_t;                               // [w][kpp], [kpp][w]
  maua::DevBuf cls, pos, lnpre_g, lnpre_b, lnpost_g, lnpost_b, proj;   // float
  std::vector<maua::BlockWeights> L;
  std::vector<maua::BlockActs> K;   // kept by the forward for the way back: per layer (keep), else K[0] serves every layer
  // workspaces for `cap` images: one set carved from ws by ensure_ws - the pieces below and every piece of K
  maua::DevBuf ws;
  long cap = 0;            // (cap, keep: what the set is placed for; set after it)
  int keep = 0;            // sized with the kept activations of a gradient pass
  void *patches = nullptr, *pe = nullptr, *tok = nullptr, *x_last = nullptr, *lno = nullptr, *act = nullptr;
  void *dxa = nullptr, *dxb = nullptr, *dqkv = nullptr, *dwide = nullptr, *dtmp = nullptr;
  float *st_pre = nullptr, *delta = nullptr, *embed = nullptr, *loss = nullptr;
  long kept_N = 0;         // images of the last kept forward (0: none)
  // cutouts per pass through the tower, fixed by clip_prepare_guide for (grp_B, grp_H, grp_W, grp_cutn, grp_aug) until one of them or
  // the limit changes (0: not fixed yet).  ws_limit: bytes one pass may take (maua_clip_set_workspace_limit; 0 = from free memory)
  int grp = 0, grp_B = 0, grp_H = 0, grp_W = 0, grp_cutn = 0, grp_aug = 0;
  size_t ws_limit = 0;
  // targets
  maua::DevBuf tgt, twt;         // float [S][P][E], [S][P]
  int S = 0, P = 0;
  maua::DevBuf sel;              // int: the target set of each sample
  int sel_B = 0;           // samples it is set for (0: set 0 for everybody)
  // cutout scratch: one set carved from cut_ws by clip_prepare_guide
  maua::DevBuf cut_ws;
  void* cut_tables = nullptr; size_t cut_tables_bytes = 0;   // (the sizes the pieces are placed for; set after the set)
  float* cut_th = nullptr; size_t cut_th_bytes = 0;
  double* parts = nullptr;
  maua::DevBuf rects_dev;        // int: rectangles + the multiplicities behind them (floats)
  // augmented cutouts (cutout_augs.hip): rectangles + slot rectangles, records, and the two [group][B][3][S][S] buffers
  maua::DevBuf aug_rects;        // int
  maua::DevBuf aug_recs;
  maua::DevBuf aug_x1, aug_x2;   // float
  unsigned long long uid = 0, epoch = 0;   // identity of this tower / generation of its buffers (a captured graph holds pointers into
};                                          // them: sampler.hip compares both before a replay)

// CLIP's text tower (CLIP.encode_text): forward only - prompts are constants of the guided loop
struct maua_clip_text {
  maua_ctx* ctx;
  int dtype;
  size_t esize;
  int ctx_len, vocab, width, layers, heads, E;
  maua::DevBuf tok_emb, pos, lnf_g, lnf_b, proj;   // f32 [vocab][w], [ctx][w], [w], [w], [w][E]
  std::vector<maua::BlockWeights> L;   // (no transposes: no way back)
  // workspaces for `cap` sequences (at least TEXT_MIN_ROWS rows), shared by the layers: one set carved from ws
  maua::DevBuf ws;
  long cap = 0;            // (set after the set is placed)
  void *xa = nullptr, *xb = nullptr, *lno = nullptr, *act = nullptr;
  maua::BlockActs k;   // qkv, ao, xm, h (no input kept, no statistics)
};

namespace maua {

// ---- clip.hip, for clip_guide.hip
int clip_loaded(maua_clip* n);   // every parameter of the tower, or the error
// workspaces for N images; keep: every layer's activations stay (a gradient pass follows), otherwise the layers share one set
int ensure_ws(maua_clip* n, long N, int keep);
size_t ws_bytes_per_image(const maua_clip* n);   // what ensure_ws(N, keep = 1) allocates per image
// patch rows in n->patches -> n->x_last; the head on it: embeddings, losses, and (with_grad) the class tokens' gradient into the zeroed
// n->dxa; d x_last in n->dxa -> d patches in n->dwide
int run_forward(maua_clip* n, long N, bool keep);
int zero_dx(maua_clip* n, long N);
int run_head(maua_clip* n, long N, bool with_grad, const float* d_embed, int B, float coef, bool write_loss, const float* mult = nullptr);
int run_backward(maua_clip* n, long N);

}  // namespace maua
