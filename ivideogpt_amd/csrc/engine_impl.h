// Per-call execution context shared by tokenizer.cpp / transformer.cpp / api.cpp.
#pragma once
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "engine.h"

namespace ivg {

#define IVG_TRY(x) do { int _r = (x); if (_r != 0) return _r; } while (0)

// GroupNorm statistics of an activation tensor that its PRODUCER (a conv3x3 epilogue) already reduced: [N][chunks][groups] double2
struct GnStats { void* part = nullptr; int chunks = 0; };

// One prompt pass over ids (or embeds) [B][L]: appends K / V of positions [0, L) to the cache and writes whichever outputs are set
struct PrefillReq {
  const int64_t* ids = nullptr; int64_t ids_stride = 0; int B = 0, L = 0;
  const void* act_emb = nullptr; int act_T = 0, ctx = 1; bool all_slots = false;   // embedded action table [B][act_T][H], added on the first sdf slot, or on all
  float* logits_all = nullptr;      // [B][L][V]
  float* logits_last = nullptr; void* hidden_last = nullptr;   // [B][V], and the residual rows [B][H] of the last position they come from
  const void* embeds = nullptr;     // [B][L][H] llm dtype: used instead of the embedding of ids
  void* hidden_all = nullptr;       // [B][L][H] llm dtype: post-final-norm hidden states (eval heads)
  const int64_t* labels = nullptr; float* token_nll = nullptr;   // [B][L]: shifted cross-entropy per position
  // ivg_kv_extend's chunk pass: the L rows are positions [pos0, pos0 + L) appended to the kept cache (`ids` points at column pos0);
  // next_ids (stride ids_stride, pointing at column pos0 + 1): the given next tokens token_nll [B][L] is taken against, instead of labels
  bool append = false; int pos0 = 0; const int64_t* next_ids = nullptr;
  // ivg_kv_extend_scored's chunk pass: token_scores [B][L][3] against next_ids, columns c >= ts_first_forced with (c - ts_first_forced) %
  // ts_period == 0 forced (three zeros); frame_rew [B][fr_F] / frame_hid [B][fr_F][H] from residual rows b * L + fr_row0 + 17 k
  float* token_scores = nullptr; int ts_first_forced = 0, ts_period = 0;
  float* frame_rew = nullptr; void* frame_hid = nullptr; int fr_row0 = 0, fr_F = 0;
};

// ivg_kv_extend: positions [keep_len, L0 - 1) of `prompt` teacher-forced onto the kept cache (arguments already checked and verified)
struct ExtendReq {
  const int64_t* prompt = nullptr; int64_t prompt_stride = 0; int B = 0, keep_len = 0, L0 = 0;
  const float* actions = nullptr; int act_T = 0, ctx = 1;
  float* token_nll = nullptr;       // [B][L0 - 1 - keep_len] or null
  // ivg_kv_extend_scored: [B][T][3], [B][F_out], [B][F_out][H] or null; the frames are i_first .. i_first + F_out - 1 (kv_extend_frames)
  float* token_scores = nullptr; float* frame_rewards = nullptr; void* frame_hidden = nullptr;
  bool chunk = false;               // route: one chunk pass (native bf16 cache, head_dim 64) or decode steps with given inputs
};

// One rollout of n_new tokens after a prompt of L0, for B trajectories
struct GenerateReq {
  const int64_t* prompt = nullptr; int64_t prompt_stride = 0; int B = 0, L0 = 0, n_new = 0;
  const float* actions = nullptr; int act_T = 0, ctx = 1;
  const float* uniforms = nullptr; int top_k = 0;
  int64_t* ids_out = nullptr; float* reward_out = nullptr;
  bool reuse_kv = false;            // the cache already holds positions [0, L0 - 1) of this prompt
  // embeds != null: llm.generate(inputs_embeds=...) -- the prompt is given as input embeddings, only the n_new tokens are
  // returned (new_ids_out [B][n_new]); hidden_out [B][H]: post-norm hidden state of the last forward pass
  const void* embeds = nullptr; int64_t* new_ids_out = nullptr; void* hidden_out = nullptr;
  bool force_sdf = false;           // every 17th new token is the forced sdf even without actions (generate_without_action)
  bool fanout = false;              // ivg_generate_fanout: a shared-context rollout whose prefix [0, L0 - 1) IS the kept cache (no prompt pass)
  int group = 1;                    // > 1: shared-context rollout, `prompt` holds one row per group of `group` consecutive trajectories
  // ivg_generate_frames: reward / post-norm hidden state of every frame whose 16th token is fed, [B][n_new / 17] and [B][n_new / 17][H]
  float* frame_rewards_out = nullptr; void* frame_hidden_out = nullptr;
  // ivg_generate_scored / ivg_generate_embeds_scored: [B][n_new][3] = logprob, entropy, max logprob of every decided new token
  float* token_scores_out = nullptr;
  // ivg_generate_filtered and its siblings: [B][n_new][4] = filtered logprob, filtered entropy, kept log-mass, support of every decided new token
  float* filtered_scores_out = nullptr;
};

struct Run {
  ivg_engine* e;
  hipStream_t st;
  bool planning;  // true: only walk the allocation plan (no launches) to size the workspace
  bool x3 = false;   // the entry point running now computes its fp32 matrix products in split-bf16 arithmetic (IVG_F32X3 path)
  unsigned int* kv_amax = nullptr;   // prefill: after each layer's rope_kv, fold max |K|, |V| per head into kv_amax[layer][2][heads] (ivg_kv_calibrate)
  int kv_group = 1;  // decoder_trunk: trajectories per shared context (cross-attention K / V projected once per group; detokenize sets it)

  // ---- primitives (tokenizer.cpp)
  int conv(DType dt, const void* X, int N, int H, int W, const ConvW& c, void* Y, int stride, int ups, const void* Rres, int flags,
           int out_f32, GnStats* out_stats = nullptr /* in: .part = buffer; out: .chunks (0: the statistics were not produced) */,
           const void* in_coef = nullptr /* GroupNorm + SiLU of X applied inside the conv3x3 staging; returns -100 when not covered */);
  // conv(silu(GroupNorm(x))) with the normalisation fused into the convolution's input staging where the 3x3 kernel covers the
  // shape (the normalised tensor never reaches HBM); otherwise GroupNorm into `scratch`, then the convolution
  int norm_conv(DType dt, const void* x, int N, int H, int W, const NormW& n, float eps, const GnStats* x_stats, const ConvW& c, void* Y,
                const void* Rres, void* scratch, GnStats* out_stats);
  int gemm(DType dt, const IgemmArgs& a, double flops, double bytes);
  int linear(DType dt, const void* X, long rows, const ConvW& c, void* Y, const void* Rres, int flags, int out_f32);
  int gnorm(DType dt, const void* X, void* Y, int N, int P, int C, const NormW& n, float eps, int silu, const float* pos,
            const GnStats* stats = nullptr /* statistics of X from its producer: skips the statistics pass */);
  int resnet(DType dt, const void* x, int N, int H, int W, const ResnetW& r, void* out, const GnStats* x_stats = nullptr,
             GnStats* out_stats = nullptr);
  size_t gn_stats_bytes(int N, int H, int W, int C) const;
  int self_attention(DType dt, const void* x, int N, int P, int C, const AttnW& a, void* out);
  int xatt_project_kv(DType dt, const void* feat, int B, const XAttW& x, void* Kp, void* VpT);
  int cross_attention(DType dt, const void* z, int B, int F, const XAttW& x, const void* Kp, const void* VpT, void* out);
  int encoder_trunk(const TrunkW& w, const void* pixels, DType pix_dt, int B, int per, int T_total, int t0,
                    std::vector<Feature>* keep, const std::vector<Feature>* cond, void* latent,
                    const ivg_enc_cache* kept = nullptr /* conditional encoder on kept K / V projections (cond is not read) */);
  int decoder_trunk(const TrunkW& w, const void* z, int B, int per, int T_total, int t0, std::vector<Feature>* keep,
                    const std::vector<Feature>* cond, void* out_pixels, DType out_dt);
  int tokenize(const void* pixels, DType pix_dt, int B, int T, int64_t* ids, int64_t ids_stride, int64_t* labels, bool ctx_only,
               ivg_enc_cache* fill = nullptr /* context-only call: also project the context features into this cache */);
  int tokenize_frames(const void* frames, DType pix_dt, int B, int n, const ivg_enc_cache* cache, int64_t* ids, int64_t ids_stride);
  int detokenize(const int64_t* ids, int B, int F, void* out_pixels, DType out_dt, ivg_cache* cache, int cache_mode,
                 int group = 1 /* > 1: consecutive rows share their context (decoded / projected once per group) */);

  // ---- transformer (transformer.cpp)
  int prefill(const PrefillReq& q);
  int generate(const GenerateReq& q);
  int extend(const ExtendReq& q);

  // ---- measurement
  void prof_begin(DType dt, double flops, double bytes, int base = 0);   // base 0: igemm classes, 2: conv3x3 classes
  void prof_end(DType dt, int base = 0);
  void prof_cancel(DType dt, int base = 0);
};

size_t dtype_size(DType d);
long long enc_counter(int which);   // 0: images through the plain encoder trunk, 1: through the conditional one, 2: xatt_project_kv calls for an encoder
int build_tokenizer(ivg_engine* e);
int build_transformer(ivg_engine* e);
size_t gen_buffer_bytes(const ivg_engine* e);
// device-side verification (one stream synchronisation) that the kept KV cache was built from this very prefix
// (positions [0, len) of B kept trajectories, 1 <= len <= the kept length; ids_only: the action rows of the cached slots are not compared)
int kv_prefix_matches_ids(ivg_engine* e, const int64_t* prompt, int64_t prompt_stride, int B, int len, const float* actions, int act_T,
                          int ctx, hipStream_t st, bool* ok, bool ids_only = false);
// frames whose 16th token, position q_i = 257 ctx + 17 i + 15, lies in [keep_len, L0 - 2]: *i_first the first one; -> their number
int kv_extend_frames(int keep_len, int L0, int ctx, int* i_first);
bool kv_extend_chunk_covers(const ivg_engine* e);   // ivg_kv_extend takes the chunk pass on this engine (format, element type, head dim, switch)
int kv_prefix_matches_embeds(ivg_engine* e, const void* embeds, int B, int L0, hipStream_t st, bool* ok);
int need_kept_cache(ivg_engine* e, const char* entry);   // 0, or the refusal of an entry that works on a kept cache where the engine holds none
// ivg_kv_select: the kept cache's rows, and everything the verification above compares them with, gathered by `parents`
int kv_select(ivg_engine* e, const int32_t* parents, int n, hipStream_t st);
// ivg_kv_snapshot_create / _restore: everything kv_select gathers, copied out into a device allocation of the caller's and back in
// (arguments other than the engine and the snapshot pointers are checked here)
int kv_snapshot_create(ivg_engine* e, ivg_kv_snapshot** out, hipStream_t st);
int kv_snapshot_restore(ivg_engine* e, const ivg_kv_snapshot* s, const int32_t* parents, int n, hipStream_t st);
size_t kv_select_scratch_bytes(const ivg_engine* e);   // workspace that stages one slab of any buffer ivg_kv_select gathers, all rows staged

}  // namespace ivg
