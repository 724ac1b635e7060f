// The guided-diffusion UNet's state (unet.hip) and the narrow interface the in-library sampler loops (sampler.hip) use on it.
#pragma once
#include <string>
#include <unordered_map>
#include <vector>

#include "common.h"
#include "internal.h"
#include "plain_conv.h"

namespace maua {

// ----------------------------------------------------------------------------------------------------- parameters
struct UGN { int C = 0; float* gamma = nullptr; float* beta = nullptr; };
// (the 3x3 convolutions are PlainConv, padded to 32 channels; wt_t exists once a weight was loaded under option "vjp")
struct ULin{ int K = 0, N = 0; void* w = nullptr; float* bias = nullptr; void* w_t = nullptr; };   // w_t [K][N]: the input-gradient GEMM
struct URes { int Cin, Cout, updown; UGN n1; PlainConv c1; int emb_off; UGN n2; PlainConv c2; bool skip; ULin sk; };
struct UAttn { int C, heads; UGN n; ULin qkv, proj; };
struct ULayer { int kind; int idx; };  // 0 conv_in, 1 res, 2 attn
struct UBlock { std::vector<ULayer> layers; int out_ch = 0; };

enum PKind { P_GN_G, P_GN_B, P_CONV_W, P_CONV_B, P_LIN_W, P_LIN_B, P_F32 };
struct PRef { PKind kind; void* obj; float* f32 = nullptr; size_t count = 0; };

// What a kept forward (maua_unet_forward_keep) leaves for maua_unet_vjp: per layer, the tensors its input gradient reads
struct TapeOp {
  int kind, idx;                  // 1 ResBlock, 2 AttentionBlock (index into res / attn)
  const void* x0; int C0;         // the layer's input (virtually concatenated [x0 | x1])
  const void* x1; int C1;
  int H, W;                       // input size
  void* out;                      // its output
  void* h1;                       // ResBlock: conv1's output (the second GroupNorm's input); Attention: qkv
  void* ao;                       // Attention: the attention result (proj_out's input)
  float* st1;                     // statistics of the first / only GroupNorm
  float* st2;                     // ... of the ResBlock's second
  float* lse;                     // Attention: log-sum-exp rows
};

struct Arena {
  DevBuf base;
  size_t top = 0, peak = 0;
  bool plan = true;
  void* get(size_t bytes) {
    const size_t o = (top + 255) & ~(size_t)255;
    top = o + bytes;
    if (top > peak) peak = top;
    return plan ? (void*)(uintptr_t)(o + 256) : (void*)(base.as<char>() + o);  // (planning: a non-NULL token, never dereferenced)
  }
};

}  // namespace maua

struct maua_unet {
  maua_ctx* ctx;
  int image_size, in_ch, mc, out_ch, nrb, head_ch, dtype;
  size_t esize;
  std::vector<float> mult;
  std::vector<int> attn_ds;
  int emb_dim;
  maua::PlainConv conv_in, conv_out;
  maua::UGN out_norm;
  std::vector<maua::URes> res;
  std::vector<maua::UAttn> attn;
  std::vector<maua::UBlock> input, output;
  maua::UBlock middle;
  int final_ch = 0;
  // f32 timestep path: time_embed.{0,2}, all emb_layers stacked [emb_total][emb_dim]
  float *te0_w = nullptr, *te0_b = nullptr, *te2_w = nullptr, *te2_b = nullptr, *embw = nullptr, *embb = nullptr;
  float* freqs = nullptr;  // [mc / 2] timestep-embedding frequencies (optional upload: "timestep_embedding.freqs")
  int freqs_loaded = 0;
  int emb_total = 0;
  std::unordered_map<std::string, maua::PRef> params;
  std::vector<maua::DevBuf> owned;   // the parameters behind the pointers of the records above
  maua::UnitStyles ones;   // [bcap][max_ch]
  int max_ch = 0;
  maua::Arena arena;
  size_t planned_key = 0;  // B, H, W the arena was planned for
  size_t gather_bytes = 0; // split-K workspace of the gather GEMM at that shape
  int route = 0;           // debugging / ablation: 1 = every 3x3 convolution on the generic kernel
  int psum_off = 0;        // 1: GroupNorm statistics always by their own pass (A/B of the convolution epilogues' piece sums)
  const float* emb_row = nullptr;    // non-NULL during a sampler-loop forward: this step's row (all samples share the timestep)
  // input gradient (maua_unet_forward_keep + maua_unet_vjp; option "vjp" = 1 before the weights are loaded)
  int vjp = 0;
  std::vector<maua::TapeOp> tape;
  bool tape_valid = false;           // the arena still holds the kept forward the tape describes
  int tape_B = 0, tape_H = 0, tape_W = 0;
  void* tape_h0 = nullptr;           // conv_in's output
  void* tape_hf = nullptr;           // the last block's output (out_norm's input)
  int tape_cf = 0;
  float* tape_stf = nullptr;         // out_norm's statistics
  float* tape_emb = nullptr;         // the emb_layers outputs of that forward
  long tape_emb_ld = 0;
  size_t tape_top = 0;               // arena top behind the kept forward
  float* tape_gather_ws = nullptr;   // the split-K workspace of that forward (the gradient convolutions share it)

  // What the in-library sampler loops (sampler.hip) keep on a network; the forward reads none of it
  struct SamplerState {
    // sampler graph (maua_ddim_sample_loop)
    hipGraphExec_t graph_exec = nullptr;
    size_t graph_key = 0;
    maua::DevBuf emb_table;            // float [n_steps][emb_total]: every step's emb_layers outputs, computed once per sampler loop
    size_t emb_table_rows = 0;         // (rows it holds; set after it)
    hipStream_t cap_stream = nullptr;  // capture happens on a private stream (the caller's may be the legacy NULL stream)
    int graph_failed = 0;              // capture / instantiation failed once: the loop runs eagerly from then on
    float* g_x = nullptr;              // the caller's tensor the graph was captured on
    maua::DevBuf g_out, g_pred;        // float: the model's output, pred_xstart
    maua::DevBuf g_t, g_cf;            // float [g_steps], [g_steps][8]: timesteps and DDIM coefficients per step and sample
    int g_steps = 0;                   // (set after them)
    // guided sampler graph (maua_ddim_guided_loop): its own executable; the sample, the target and every per-step constant live in
    // library buffers, so one capture serves every call of a shape
    hipGraphExec_t gd_exec = nullptr;
    size_t gd_key = 0;
    unsigned long long gd_sec_uid = 0, gd_sec_epoch = 0;   // the secondary model (and its buffers' generation) gd_exec points into
    // text-prompt guidance (maua_unet_set_clip_guide): CLIPGrads instead of the image-MSE module in the guided loop
    std::vector<maua_guide*> gd_guides;   // maua_unet_set_guides: grad modules evaluated (after CLIPGrads, if set) and summed per step
    std::vector<unsigned long long> gd_guide_uids, gd_guide_epochs;   // (epochs: as of the capture)
    maua::DevBuf gd_gflag;             // int: the NaN screen's flag of the guides' sum
    maua_clip* gd_clip = nullptr;
    maua::DevBuf gd_rects;             // int [n_steps][batches][cutn][3] (+ [n_steps][batches][cutn] float multiplicities behind them)
    float* gd_mult = nullptr;          // those multiplicities (into gd_rects), or NULL: every cutout counts once
    int gd_last_graph = 0;             // the LAST guided loop replayed a captured graph (maua_unet_guided_graph_active)
    int gd_cutn_total = 0;
    std::vector<int> gd_rects_host;
    int gd_rect_steps = 0, gd_cutn = 0, gd_batches = 0;
    float gd_clip_scale = 1.f, gd_clip_clamp = 0.f;
    unsigned long long gd_clip_uid = 0, gd_clip_epoch = 0, gd_guide_gen = 0, gd_guide_gen_seen = 0;
    int gd_failed = 0;
    maua::DevBuf gd_ws;                // one set, carved into the three pieces below; their counts are set after it is placed
    float* gd_buf = nullptr;           // x | v | pred | eps | img | g | jv | grad | target, B * C * H * W floats each
    size_t gd_cap = 0;                 // floats
    float* gd_tab = nullptr;           // cos_t [S][B] | (sigma, 1 - sigma) [S][B][2] | grad coefficients [S][B][2] | k [B]
    size_t gd_tab_cap = 0;             // floats
    int* gd_flag = nullptr;            // [gd_flags] one NaN flag per step, zeroed before every loop (outside the graph)
    int gd_flags = 0;
    // the guidance branch of a step (secondary forward, grad module, secondary VJP) depends on x only: it runs BESIDE the UNet forward
    // on a side stream (a parallel branch of the captured graph) and joins at the DDIM update; option "guided_fork" = 0: one stream
    int gd_fork = 1;
    hipStream_t side_stream = nullptr, cap_side = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    void release();                    // both executables, the streams and the events; the buffers free themselves
  } smp;
};

namespace maua {

// ---- unet.hip, for sampler.hip
// the forward on the context's stream (x, t, out as maua_unet_forward's); keep: as maua_unet_forward_keep, leaving the tape for unet_vjp
int unet_forward(maua_unet* n, const float* x, const float* t, int B, int H, int W, float* out, bool keep);
// the kept forward's input gradient; g_channels: channels of g_out actually handed in ([B][g_channels][H][W]; the remaining output
// channels' gradient is zero), 0: all of them
int unet_vjp(maua_unet* n, const float* g_out, float* g_x, int g_channels);
// the timestep path: t [rows] (device) -> emb [rows][emb_total], every ResBlock's emb_layers output; e0 [rows][mc], e1 and e2
// [rows][emb_dim]: scratch
int unet_emb_rows(maua_unet* n, hipStream_t st, const float* t, int rows, float* e0, float* e1, float* e2, float* emb);
// the two small f32 kernels at the top of unet.hip on a stream: e [B][dim] = timestep_embedding(t) (freqs: a float32 table or NULL);
// y [B][N] = act_out(W [N][K] . act_in(x) + bias) (act: 0 none, 1 SiLU; bias or NULL).  Sizes are the caller's to check.
int launch_timestep_embedding(hipStream_t st, const float* t, const float* freqs, int B, int dim, float* e);
int launch_linear_rows(hipStream_t st, const float* x, const float* W, const float* bias, int B, int K, int N, int act_in, int act_out, float* y);
// the arena is planned for an ordinary forward of this shape and `ones` covers B: such a forward allocates nothing (capturable)
bool unet_planned(const maua_unet* n, int B, int H, int W);

// ---- sampler.hip, for unet.hip
size_t shape_key(int B, int H, int W);
// the captured sampler loops hold pointers into the arena / the per-step tables: whatever moves those drops both executables
void drop_sampler_graphs(maua_unet* n);

}  // namespace maua
