// Llama-style autoregressive transformer over video tokens on the hand-written kernels.
//
// Replaces (structure only; arithmetic is in the .hip kernels):
//   HF LlamaForCausalLM.forward / GenerationMixin._sample          
//   HeadModelWithAction.generate / .forward                        ivideogpt/transformer/action_model.py:56-121,154-205
// MI355X-first differences from the reference's op sequence (token-identical):
//   * ONE prefill + KV-cached single-token steps even in the action-conditioned mode (the reference
//     re-prefills the whole prefix for every future frame, action_model.py:101-110);
//   * a decode step is a fixed sequence of 62 kernels (sampler, 12 x [QKV GEMM with the input RMSNorm folded in, attention,
//     o-proj + residual, gate/up GEMM with the post-attention norm + SiLU(gate)*up, down-proj + residual], lm_head with the
//     final norm) whose step-dependent scalars live in device memory, captured once into a hipGraph and replayed for every
//     generated token -- no host sync, no per-step Python;
//   * decode GEMMs stream each weight matrix once; their K reduction happens inside the workgroup in a fixed order
//     (deterministic, no partials in HBM);
//   * the prompt pass uses the 256 x 256-tile GEMM (gemm256.hip), a vectorised RoPE + cache append and, in bf16, a one-pass
//     causal attention kernel; step-wise callers (MBRL) keep the KV cache across calls (ivg_generate_continue).
#include <cstring>
#include "engine_impl.h"
#include "switches.h"

namespace ivg {

#define CK(x) do { int _e = (x); if (_e != 0) return e->fail(IVG_ERR_HIP, std::string(#x) + " failed: hip error " + std::to_string(_e)); } while (0)

static size_t esz(DType d) { return d == BF16 ? 2 : 4; }
static size_t rup(size_t v, size_t a) { return (v + a - 1) / a * a; }

struct GenBuf {  // persistent decode-step buffers (fixed addresses so the captured step graph can be replayed)
  StepState* state;
  char* x; char* qkv; char* attn; char* act; float* logits;
  int64_t* ids; float* uni; char* act_emb; int Bc, ids_ld;
  float* last_act;   // [Bc][max_frames][action_dim]: the action table of the call that built the kept KV cache
  int* flag;         // mismatch counter of the prefix verification
  // per-frame heads (ivg_generate_frames): [Bc][F_max] rewards and [Bc][F_max][H] post-norm hidden rows, written by frame_heads_kernel
  // inside the steps and copied to the caller per chunk, like ids
  float* frame_rew; char* frame_hid; int F_max;
  // token scores (ivg_generate_scored): [Bc][ids_ld][3] floats, column j - 1 written by token_scores_kernel right after the sampler
  // decided new token j; copied to the caller per chunk
  float* tok_scores;
  // filtered scores (ivg_generate_filtered): [Bc][ids_ld][4] floats, column j - 1 written by filtered_scores_kernel in the same slot
  float* filt_scores;
};

// What the decode steps of one chunk of a call do beyond the fixed sequence (step_key names every field)
struct StepOpts {
  // shared-context rollout (ivg_generate_shared, ivg_generate_fanout): rows of the chunk in groups of sh_G sharing the cache rows
  // [0, sh_P) of their prompt -- see decode_attn_kernel SHARED.  sh_P = 0: off
  int sh_P = 0, sh_G = 1, sh_row0 = 0;
  bool fr_rew = false, fr_hid = false;   // the steps carry frame_heads_kernel, writing GenBuf::frame_rew / frame_hid
  bool scored = false;                   // the steps carry token_scores_kernel
  bool filtered = false;                 // the steps carry filtered_scores_kernel
};

static size_t gen_layout(const ivg_engine* e, GenBuf& g, char* base) {   // base = null: only the size
  const ivg_config& c = e->cfg;
  const DType dt = e->llm_dt;
  const int Bc = e->kvc.chunk, H = c.hidden_size, I = c.intermediate_size, V = c.vocab_size;
  g.Bc = Bc;
  g.ids_ld = e->Lmax;
  size_t off = 0;
  auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off = rup(off + bytes, 256); return p; };
  g.state = (StepState*)take(256);
  g.x = take((size_t)Bc * H * esz(dt));
  g.qkv = take((size_t)Bc * 3 * H * esz(dt));
  g.attn = take((size_t)Bc * H * esz(dt));
  g.act = take((size_t)Bc * I * esz(dt));
  g.logits = (float*)take((size_t)Bc * V * 4);
  g.ids = (int64_t*)take((size_t)Bc * g.ids_ld * 8);
  g.uni = (float*)take((size_t)Bc * g.ids_ld * 4);
  g.act_emb = take((size_t)Bc * std::max(1, c.max_frames) * H * esz(dt));
  g.last_act = (float*)take((size_t)Bc * std::max(1, c.max_frames) * std::max(1, c.action_dim) * 4);
  g.flag = (int*)take(256);
  g.F_max = std::max(1, e->Lmax / 17);   // a frame needs 17 new tokens
  g.frame_rew = (float*)take((size_t)Bc * g.F_max * 4);
  g.frame_hid = take((size_t)Bc * g.F_max * H * esz(dt));
  g.tok_scores = (float*)take((size_t)Bc * g.ids_ld * 3 * 4);
  g.filt_scores = (float*)take((size_t)Bc * g.ids_ld * 4 * 4);
  return off;
}

size_t gen_buffer_bytes(const ivg_engine* e) {
  GenBuf g;
  return gen_layout(e, g, nullptr);
}

static GenBuf gen_buf(const ivg_engine* e) {   // the layout over the engine's buffer
  GenBuf g;
  gen_layout(e, g, e->gen_buf);
  return g;
}

// -------------------------------------------------------------------------------------------- prefill
static bool flash_prefill_covers(DType dt, int hd) {
  return sw().flash_prefill && dt == BF16 && hd == 64;   // IVG_FLASH_PREFILL=0: score GEMM + softmax + P.V GEMM (A/B tests)
}

int Run::prefill(const PrefillReq& q) {
  const ivg_config& c = e->cfg;
  const KvCache& kvc = e->kvc;
  const int B = q.B, L = q.L;
  const DType dt = e->llm_dt;
  x3 = e->llm_x3;
  const int H = c.hidden_size, I = c.intermediate_size, V = c.vocab_size, heads = e->heads, hd = e->hd, Lmax = e->Lmax;
  const long M = (long)B * L;
  const int Lp = (int)rup(L, 64);
  const size_t m = e->ws.mark();
  char* x = (char*)e->ws.alloc((size_t)M * H * esz(dt));
  char* xn = (char*)e->ws.alloc((size_t)M * H * esz(dt));
  char* qkv = (char*)e->ws.alloc((size_t)M * 3 * H * esz(dt));
  char* attn = (char*)e->ws.alloc((size_t)M * H * esz(dt));
  char* act = (char*)e->ws.alloc((size_t)M * I * esz(dt));
  // q.append: the rows are positions [pos0, pos0 + L) appended to the kept cache (ivg_kv_extend's chunk pass: a native bf16 cache at
  // head_dim 64) -- RoPE at pos0, chunk_attn_kernel against cache rows [0, pos0 + l], and the kept state is the caller's to update
  const bool append = q.append;
  const bool flash = append || flash_prefill_covers(dt, hd);   // one-pass causal attention: no score matrix in HBM
  float* S = flash ? nullptr : (float*)e->ws.alloc((size_t)B * heads * L * Lp * 4);
  // a cache that is not in the engine's element type (24-bit planes, FP8): the pass itself is untouched -- RoPE writes one layer's K / V
  // rows here (the score GEMM reads K as a matrix) and the cache packs them into its own rows
  char* stage_k = kvc.staged() ? (char*)e->ws.alloc(kvc.stage_bytes(B)) : nullptr;
  char* stage_v = kvc.staged() ? (char*)e->ws.alloc(kvc.stage_bytes(B)) : nullptr;
  char* Pm = flash ? nullptr : (char*)e->ws.alloc((size_t)B * heads * L * Lp * esz(dt));
  if (!planning) {
    if (!append) e->kvc.forget_kept();   // the cache rows are about to be overwritten (ivg_generate re-validates them at its end)
    if (q.embeds) CK((int)hipMemcpyAsync(x, q.embeds, (size_t)M * H * esz(dt), hipMemcpyDeviceToDevice, st));
    else CK(launch_embed(q.ids, q.ids_stride, e->embed, x, dt, B, L, H, V, st));
    if (q.act_emb) {  // action embedding on the sdf slot(s): slot i (position 257*ctx - 1 + 17*i) gets action i + ctx - 1
      for (int i = 0;; ++i) {
        const int pos = 257 * q.ctx - 1 + 17 * i - q.pos0;   // (row of the pass)
        if (pos >= L || i + q.ctx - 1 >= q.act_T) break;
        if (pos < 0) continue;
        CK(launch_add_rows(x + (size_t)pos * H * esz(dt), (long)L * H, (const char*)q.act_emb + (size_t)(i + q.ctx - 1) * H * esz(dt),
                           (long)q.act_T * H, B, H, dt, st));
        if (!q.all_slots) break;
      }
    }
  }
  for (int l = 0; l < c.num_layers; ++l) {
    const LayerW& w = e->layers[l];
    if (!planning) CK(launch_add_rmsnorm(x, H, e->ones, xn, (int)M, H, c.rms_norm_eps, dt, st));
    ConvW wq; wq.w = w.wqkv; wq.cin = H; wq.cout = 3 * H;
    IVG_TRY(linear(dt, xn, M, wq, qkv, nullptr, 0, 0));
    char* kl = stage_k ? stage_k : kvc.ptr(l, 0);   // where this layer's roped K / V rows are in the engine's element type
    char* vl = stage_v ? stage_v : kvc.ptr(l, 1);
    if (append) {   // (no V^T image: chunk_attn_kernel reads V from the cache rows)
      if (!planning) CK(launch_rope_kv(qkv, kl, vl, nullptr, 0, e->rope_cos, e->rope_sin, B, L, heads, hd, Lmax, nullptr, q.pos0, dt, st));
    } else if (!planning) {
      CK(launch_rope_kv(qkv, kl, vl, e->vt, Lp, e->rope_cos, e->rope_sin, B, L, heads, hd, Lmax, nullptr, 0, dt, st));
      if (kv_amax) CK(launch_kv_absmax(kl, vl, B, heads, L, Lmax, kv_amax + (size_t)l * 2 * heads, st));
      CK(kvc.store_staged(l, stage_k, stage_v, B, L, st));
    }
    if (append) {
      if (!planning) CK(launch_chunk_attn(qkv, kl, vl, attn, B, L, heads, hd, Lmax, q.pos0, dt, st));
    } else if (flash) {
      if (!planning) CK(launch_flash_prefill(qkv, kl, e->vt, attn, B, L, Lp, heads, hd, Lmax, dt, st));
    } else {
    {  // S[b][h] = Q K^T / sqrt(hd)
      IgemmArgs g;
      g.X = qkv; g.W = kl; g.Y = S;
      g.Nimg = 1; g.Hin = 1; g.Win = L; g.Cin = hd; g.ldx = 3 * H; g.Hout = 1; g.Wout = L;
      g.N = L; g.ldw = hd; g.c_pix = Lp; g.c_ch = 1; g.flags = IG_OUT_F32; g.alpha = 1.0f / sqrtf((float)hd);
      g.nb0 = B; g.nb1 = heads;
      g.sa[0] = (long)L * 3 * H; g.sa[1] = hd;
      g.sw[0] = (long)heads * Lmax * hd; g.sw[1] = (long)Lmax * hd;
      g.sy[0] = (long)heads * L * Lp; g.sy[1] = (long)L * Lp;
      IVG_TRY(gemm(dt, g, 2.0 * B * heads * (double)L * L * hd, (double)esz(dt) * 2.0 * M * H + 4.0 * B * heads * L * Lp));
    }
    if (!planning) CK(launch_softmax(S, Pm, (long)B * heads * L, L, L, Lp, Lp, 1, dt, st));
    {  // attn[b][:, h*hd..] = P V
      IgemmArgs g;
      g.X = Pm; g.W = e->vt; g.Y = attn;
      g.Nimg = 1; g.Hin = 1; g.Win = L; g.Cin = Lp; g.ldx = Lp; g.Hout = 1; g.Wout = L;
      g.N = hd; g.ldw = Lp; g.c_pix = H; g.c_ch = 1;
      g.nb0 = B; g.nb1 = heads;
      g.sa[0] = (long)heads * L * Lp; g.sa[1] = (long)L * Lp;
      g.sw[0] = (long)heads * hd * Lp; g.sw[1] = (long)hd * Lp;
      g.sy[0] = (long)L * H; g.sy[1] = hd;
      IVG_TRY(gemm(dt, g, 2.0 * B * heads * (double)L * Lp * hd, (double)esz(dt) * ((double)B * heads * L * Lp + 2.0 * M * H)));
    }
    }
    ConvW wo; wo.w = w.wo; wo.cin = H; wo.cout = H;
    IVG_TRY(linear(dt, attn, M, wo, x, x, 0, 0));  // in-place residual
    if (!planning) CK(launch_add_rmsnorm(x, H, e->ones, xn, (int)M, H, c.rms_norm_eps, dt, st));
    {  // act = silu(gate) * up   (weights packed [16 gate | 16 up] per 32 rows)
      IgemmArgs g;
      g.X = xn; g.W = w.wgu; g.Y = act;
      g.Nimg = 1; g.Hin = 1; g.Win = (int)M; g.Cin = H; g.ldx = H; g.Hout = 1; g.Wout = (int)M;
      g.N = 2 * I; g.ldw = H; g.c_pix = I; g.c_ch = 1; g.flags = IG_GLU;
      IVG_TRY(gemm(dt, g, 2.0 * M * (double)H * 2 * I, (double)esz(dt) * ((double)M * H + 2.0 * I * H + (double)M * I)));
    }
    ConvW wd; wd.w = w.wdown; wd.cin = I; wd.cout = H;
    IVG_TRY(linear(dt, act, M, wd, x, x, 0, 0));
  }
  if (q.hidden_all && !planning) {
    if (!e->final_norm) return e->fail(IVG_ERR_MISSING, "hidden states requested but 'llm.norm' is not in the weight table");
    CK(launch_final_hidden(x, e->final_norm, q.hidden_all, (int)M, H, c.rms_norm_eps, dt, st));
  }
  // frame heads of an append pass: only the fr_F residual rows per trajectory that fed a frame's 16th token (not a norm over all M rows)
  if ((q.frame_rew || q.frame_hid) && q.fr_F > 0 && !planning)
    CK(launch_frame_rows_heads(x, q.fr_row0, L, 17, e->rew_w, e->rew_b, e->final_norm, q.frame_rew, q.frame_hid, B, H, q.fr_F, 0, q.fr_F,
                               c.rms_norm_eps, dt, st));
  if (q.logits_all) {
    if (!planning) CK(launch_add_rmsnorm(x, H, e->ones, xn, (int)M, H, c.rms_norm_eps, dt, st));
    ConvW wl; wl.w = e->lm_head; wl.cin = H; wl.cout = V;
    IVG_TRY(linear(dt, xn, M, wl, q.logits_all, nullptr, 0, 1));
  }
  if (q.token_nll || q.token_scores) {
    // loss without the [B][L][V] fp32 logits tensor (3.1 GB at B = 64, L = 751): lm_head over chunks of rows, each chunk reduced
    // to its per-position cross-entropy before the next one overwrites it
    const long Rc = std::min<long>(M, 4096);
    float* chunk = (float*)e->ws.alloc((size_t)Rc * V * 4);
    if (!planning && !q.logits_all) CK(launch_add_rmsnorm(x, H, e->ones, xn, (int)M, H, c.rms_norm_eps, dt, st));
    ConvW wl; wl.w = e->lm_head; wl.cin = H; wl.cout = V;
    for (long r0 = 0; r0 < M; r0 += Rc) {
      const long rows = std::min(Rc, M - r0);
      IVG_TRY(linear(dt, xn + (size_t)r0 * H * esz(dt), rows, wl, chunk, nullptr, 0, 1));
      if (planning) continue;
      if (q.token_nll) {
        if (q.next_ids) CK(launch_token_nll(chunk, q.next_ids, q.ids_stride, r0, (int)rows, L, V, q.token_nll, L, st));
        else CK(launch_ce_rows(chunk, q.labels, r0, (int)rows, L, V, q.token_nll, st));
      }
      if (q.token_scores)
        CK(launch_token_scores_rows(chunk, q.next_ids, q.ids_stride, r0, (int)rows, L, V, q.ts_first_forced, q.ts_period, q.token_scores, L, st));
    }
  }
  if (q.logits_last && !planning) {
    // last position of every sequence -> residual rows hidden_last [B][H]; final RMSNorm is fused into the lm_head GEMM
    CK((int)hipMemcpy2DAsync(q.hidden_last, (size_t)H * esz(dt), x + (size_t)(L - 1) * H * esz(dt), (size_t)L * H * esz(dt),
                             (size_t)H * esz(dt), B, hipMemcpyDeviceToDevice, st));
    SkinnyArgs s;
    s.X = q.hidden_last; s.W = e->lm_head; s.Y = q.logits_last; s.M = B; s.N = V; s.K = H; s.ldx = H; s.ldw = H; s.ldy = V;
    s.flags = IG_OUT_F32 | SK_NORM; s.eps = c.rms_norm_eps; s.lds_kb = e->decode_lds_kb;
    s.w_shared = e->in_flight();   // (the same policy as the steps' lm_head: one copy of the weights under several engines)
    CK(launch_skinny(s, dt, st));
  }
  e->ws.reset(m);
  return 0;
}

// -------------------------------------------------------------------------------------------- one decode step
// decide token j (sample / forced), embed it, run it through the layers against the KV cache, produce the
// logits for token j+1, advance the device-side state.
// (Splitting the rows into several concurrent chains on side streams was measured twice -- rounds 2 and 3, also on CU-masked
// streams -- without gain: every launch is bound by what one CU ingests, half-batch GEMMs cost what full-batch ones do.  Removed.)
static int step_body(ivg_engine* e, hipStream_t st, const GenBuf& g, const StepOpts& o, int B, const SampleArgs& sa, bool forward, bool skip_sample = false) {
  const ivg_config& c = e->cfg;
  const DType dt = e->llm_dt;
  const int H = c.hidden_size, I = c.intermediate_size, V = c.vocab_size;
  const size_t es = esz(dt);
  StepState* state = g.state;
  char* x = g.x; char* qkv = g.qkv; char* attn = g.attn; char* act = g.act; float* logits = g.logits;
  if (!skip_sample) CK(launch_sample_embed(sa, B, dt, st));   // skip: x already holds the input row (embeds path, kept KV cache)
  // token scores: the row the sampler just read is still whole (this step's lm_head overwrites it), the id it stored is in the id row
  if (!skip_sample && o.scored)
    CK(launch_token_scores(sa.logits, V, state, sa.ids_out, sa.ids_stride, sa.L0, sa.forced_period, g.tok_scores, g.ids_ld, B, st));
  // filtered scores: the same row and id under the sampler's own temperature, top-k and top-p (greedy: none of them)
  if (!skip_sample && o.filtered)
    CK(launch_filtered_scores(sa.logits, V, state, sa.ids_out, sa.ids_stride, sa.L0, sa.forced_period, sa.top_k, sa.temperature, sa.top_p,
                              sa.uniforms == nullptr, g.filt_scores, g.ids_ld, B, st));
  if (!forward) return 0;
  // 5 launches per layer: RMSNorms are fused into the consuming GEMMs (weights pre-multiplied by the norm weight,
  // row scale computed from the activations the GEMM streams anyway), residual adds into the producing GEMMs.
  const size_t gp_ld = (size_t)IVG_GEMM_PROF_SLOTS * 2 * e->Lmax;
  auto gprof = [&](SkinnyArgs& a, int idx) {
    if (!e->gemm_prof_on || !e->gemm_prof) return;
    a.prof = e->gemm_prof + (size_t)idx * gp_ld; a.pos = (const int*)state; a.prof_ld = e->Lmax;
  };
  // The batches-in-flight profile of an engine (an LDS budget below a whole CU, set per engine -- ivg_config.decode_lds_kb -- or process-wide
  // -- IVG_DECODE_LDS_KB: it shares the GPU -- and ONE copy of the weights -- with other engines, bench.py --lanes): beside the LDS budget, (1) the weight requests of the decode GEMMs use the default cache policy
  // instead of non-temporal ones -- the other engines ask for the same lines within microseconds (+1.7 %) -- and (2) no launch warms
  // the next launch's weights: with (1) the other lanes' launches already do, and the extra requests only compete with three attention
  // streams (+2.0 % on top; profiles/r05_lanes_policy.txt).  One batch alone keeps non-temporal weights + warm-up (rounds 2 / 3: each
  // byte is read once per token, the warm-up hides its first touch).
  const bool in_flight = e->in_flight();
  const bool w_shared = in_flight;
  const bool warm = !in_flight;
  // every launch also pulls the weight tiles of the NEXT launch of the chain toward the CUs that will consume them (dgemm3.hip): the
  // dependent GEMM then starts on (Infinity-)cache hits instead of a cold HBM stream
  // Conditional per shape (round 6, profiles/r06_warmup_by_kind.txt): the gate/up matrix -- half of a layer's weight bytes -- is NOT warmed:
  // requesting its 9.4 MB under o-proj lengthens o-proj by what it then saves gate/up (3.36 / 4.91 us warmed vs 2.9 / 5.35 cold), and
  // those requests were most of the class's counted traffic (2.4 x the algorithmic bytes; Infinity-Cache re-reads).  q/k/v, o-proj, down
  // and lm_head keep their warm-up (0.4 - 1.8 us per launch each).
  auto link_next = [&](SkinnyArgs& cur, const SkinnyArgs& nxt) {
    if (!warm) return;
    if (nxt.flags & IG_GLU) return;
    int rows = dgemm3_w_rows_per_block(nxt, dt);
    if (rows <= 0) rows = dgemm_w_rows_per_block(nxt, dt);   // the next launch runs on the second-generation kernel
    if (rows <= 0 || nxt.ldw != nxt.K) return;
    cur.next_W = nxt.W; cur.next_tile_bytes = (long)rows * nxt.K * (long)es; cur.next_tiles = nxt.N / rows;
  };
  auto layer_args = [&](int l, SkinnyArgs* g) {
    const LayerW& w = e->layers[l];
    for (int k = 0; k < 4; ++k) { g[k].x3 = e->llm_x3 && sw().x3; g[k].lds_kb = e->decode_lds_kb; g[k].w_shared = w_shared; g[k].kind = k; }
    SkinnyArgs& s = g[0];
    s.X = x; s.W = w.wqkv; s.Y = qkv; s.M = B; s.N = 3 * H; s.K = H; s.ldx = H; s.ldw = H; s.ldy = 3 * H;
    s.flags = SK_NORM; s.eps = c.rms_norm_eps;
    SkinnyArgs& o = g[1];
    o.X = attn; o.W = w.wo; o.Y = x; o.M = B; o.N = H; o.K = H; o.ldx = H; o.ldw = H; o.ldy = H; o.flags = IG_RESIDUAL;
    SkinnyArgs& u = g[2];
    u.X = x; u.W = w.wgu; u.Y = act; u.M = B; u.N = 2 * I; u.K = H; u.ldx = H; u.ldw = H; u.ldy = I;
    u.flags = IG_GLU | SK_NORM; u.eps = c.rms_norm_eps;
    SkinnyArgs& d = g[3];
    d.X = act; d.W = w.wdown; d.Y = x; d.M = B; d.N = H; d.K = I; d.ldx = I; d.ldw = I; d.ldy = H; d.flags = IG_RESIDUAL;
  };
  SkinnyArgs lm;
  lm.X = x; lm.W = e->lm_head; lm.Y = logits; lm.M = B; lm.N = V; lm.K = H; lm.ldx = H; lm.ldw = H; lm.ldy = V;
  lm.flags = IG_OUT_F32 | SK_NORM; lm.eps = c.rms_norm_eps; lm.lds_kb = e->decode_lds_kb; lm.w_shared = w_shared; lm.kind = 4;
  lm.bump = (int*)state;  // pos += 1, j += 1 once the last reader of this chain's state (its last attention) is done
  SkinnyArgs cur[4], nxt[4];
  layer_args(0, cur);
  for (int l = 0; l < c.num_layers; ++l) {
    const bool last = l + 1 == c.num_layers;
    if (!last) layer_args(l + 1, nxt);
    link_next(cur[0], cur[1]); link_next(cur[1], cur[2]); link_next(cur[2], cur[3]); link_next(cur[3], last ? lm : nxt[0]);
    gprof(cur[0], 4 * l + 0);
    CK(launch_skinny(cur[0], dt, st));
    unsigned long long* aprof = e->attn_prof_on ? e->attn_prof + (size_t)l * IVG_ATTN_PROF_SLOTS * 2 * e->Lmax : nullptr;
    CK(e->kvc.decode_attn(l, qkv, attn, e->rope_cos, e->rope_sin, B, state, aprof, st, o.sh_P, o.sh_G, o.sh_row0));
    gprof(cur[1], 4 * l + 1);
    CK(launch_skinny(cur[1], dt, st));
    gprof(cur[2], 4 * l + 2);
    CK(launch_skinny(cur[2], dt, st));
    gprof(cur[3], 4 * l + 3);
    CK(launch_skinny(cur[3], dt, st));
    if (!last) for (int k = 0; k < 4; ++k) cur[k] = nxt[k];
  }
  {   // the first GEMM of the next step's chain: q/k/v of layer 0
    SkinnyArgs first[4];
    layer_args(0, first);
    link_next(lm, first[0]);
  }
  // per-frame heads: x is final here (the last down-projection is done, the next sampler has not run) and the state still names the
  // token this step fed (lm_head advances it)
  if (o.fr_rew || o.fr_hid)
    CK(launch_frame_heads(x, state, e->rew_w, e->rew_b, e->final_norm, o.fr_rew ? g.frame_rew : nullptr, o.fr_hid ? g.frame_hid : nullptr, B, H,
                          g.F_max, c.rms_norm_eps, dt, st));
  gprof(lm, 4 * c.num_layers);
  CK(launch_skinny(lm, dt, st));
  return 0;
}

// The key of a captured step graph: everything step_body bakes into the launches of a step, so that a replay is the step the call would
// have launched.  A step feature that changes what step_body launches or passes by value adds its component HERE.
static std::string step_key(const ivg_engine* e, const StepOpts& o, const SampleArgs& sa, int B) {
  uint32_t t_bits; memcpy(&t_bits, &sa.temperature, 4);   // (by their BIT PATTERNS: to_string keeps six decimals)
  uint32_t p_bits; memcpy(&p_bits, &sa.top_p, 4);
  std::string k = std::to_string(B);                        // the rows of every launch
  k += ":" + std::to_string(t_bits);                        // sampler: logits / temperature
  k += ":" + std::to_string(p_bits);                        // sampler: nucleus filter
  k += ":" + std::to_string(e->decode_lds_kb);              // decode GEMMs: the LDS budget picks kernel generation and tiling
  k += ":" + std::to_string(switches_generation());         // every launcher: the kernel-selection switches a replay would keep ignoring
  k += sa.uniforms ? ":s" : ":g";                           // sampler: draws from the uniforms buffer, or greedy
  k += ":" + std::to_string(sa.top_k);                      // sampler: top-k filter
  k += ":" + std::to_string(sa.forced_period);              // sampler: the forced-sdf schedule
  k += ":" + std::to_string(sa.ctx);                        // sampler: action row of a forced slot (with slot0 = (L0 - 257 ctx) / 17)
  k += ":" + std::to_string(sa.act_T);                      // sampler: row stride of the embedded action table
  k += ":" + std::to_string(sa.L0);                         // sampler: column of new token j; shared: the prefix length sh_P = L0 - 1
  if (e->attn_prof_on) k += ":p";                           // decode attention: launch-window stamps
  if (e->gemm_prof_on) k += ":q";                           // decode GEMMs: launch-window stamps
  if (o.sh_P > 0) k += ":sh" + std::to_string(o.sh_G) + ":" + std::to_string(o.sh_row0);   // decode attention: the groups' shared rows
  if (o.fr_rew || o.fr_hid) k += std::string(":f") + (o.fr_rew ? "r" : "") + (o.fr_hid ? "h" : "");   // frame_heads_kernel and its outputs
  if (o.scored) k += ":ts";                                 // token_scores_kernel after the sampler
  if (o.filtered) k += ":fs";                               // filtered_scores_kernel after it
  return k + e->kvc.graph_key();                            // decode attention: the cache format and its scales
}

// ---------------------------------------------------------------------------------------- captured step graphs (ivg_engine::graphs)
// every exec is destroyed only once nothing queued on the stream can still be replaying it
static int drop_graphs(ivg_engine* e, hipStream_t st) {
  CK((int)hipStreamSynchronize(st));
  for (auto& kv : e->graphs) (void)hipGraphExecDestroy(kv.second);
  e->graphs.clear();
  return 0;
}

// the graph of n_steps consecutive steps under `key`, captured on first use.  *out = null: no graph (IVG_GRAPH off, the null stream, or
// the capture failed) -- the caller launches eagerly
static int step_graph(ivg_engine* e, hipStream_t st, const std::string& key, int n_steps, const GenBuf& g, const StepOpts& o, int Bc, const SampleArgs& sa,
                      hipGraphExec_t* out) {
  *out = nullptr;
  if (!(e->use_graph && st != nullptr)) return 0;
  if (e->graphs_gen != switches_generation()) {   // the switch table changed: no captured step of the old table can be replayed again
    if (!e->graphs.empty()) IVG_TRY(drop_graphs(e, st));
    e->graphs_gen = switches_generation();
  }
  const std::string k = key + (n_steps > 1 ? ":x" + std::to_string(n_steps) : "");
  auto it = e->graphs.find(k);
  if (it != e->graphs.end()) { *out = it->second; return 0; }
  hipGraph_t graph = nullptr;
  hipGraphExec_t ex = nullptr;
  if (hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal) == hipSuccess) {
    int rc = 0;
    for (int i = 0; i < n_steps && rc == 0; ++i) rc = step_body(e, st, g, o, Bc, sa, true);
    const hipError_t ce = hipStreamEndCapture(st, &graph);
    if (rc == 0 && ce == hipSuccess && graph && hipGraphInstantiate(&ex, graph, nullptr, nullptr, 0) == hipSuccess) {
      if (e->graphs.size() >= 64) IVG_TRY(drop_graphs(e, st));   // bound the cache (a server fed ever new prompt lengths): drop all, recapture on demand
      e->graphs[k] = ex;
      *out = ex;
    } else {
      (void)hipGetLastError();
    }
    if (graph) (void)hipGraphDestroy(graph);
  } else {
    (void)hipGetLastError();
  }
  return 0;
}

struct Chunk { int b0, Bc; StepOpts o; };   // rows [b0, b0 + Bc) of a call, and what their steps carry

// The chunk's inputs into the step buffers, and the cache rows of its prompt: id rows (shared: expanded per group, and the groups' prompt
// pass), uniforms, the embedded action table, the prompt pass, the embeddings snapshot
static int stage_chunk(Run& r, const GenerateReq& q, const GenBuf& g, const Chunk& k) {
  ivg_engine* e = r.e; hipStream_t st = r.st;
  const ivg_config& c = e->cfg;
  const DType dt = e->llm_dt;
  const int b0 = k.b0, Bc = k.Bc, L0 = q.L0, n_new = q.n_new, act_T = q.act_T, group = q.group, H = c.hidden_size;
  const size_t es = esz(dt);
  const bool shared = k.o.sh_P > 0;
  if (e->gemm_prof_on && e->gemm_prof) {
    CK((int)hipMemsetAsync(e->gemm_prof, 0, (size_t)(4 * c.num_layers + 1) * IVG_GEMM_PROF_SLOTS * 2 * e->Lmax * 8, st));
    e->gemm_prof_B = Bc;
  }
  if (e->attn_prof_on) {  // fresh launch windows for this call: every stamp slot back to 0 (= not stamped)
    CK((int)hipMemsetAsync(e->attn_prof, 0, (size_t)c.num_layers * IVG_ATTN_PROF_SLOTS * 2 * e->Lmax * 8, st));
    e->attn_prof_B = Bc; e->kvc.prof_eb = (int)e->kvc.elem_bytes();
  }
  if (shared) {   // every trajectory starts from a copy of its group's prompt; groups g_lo .. g_hi have rows in this chunk
    const int g_lo = b0 / group, g_hi = (b0 + Bc - 1) / group;
    // (attending the prompt rows once per 16 trajectories on the matrix cores -- tools/ubench/prefix_attn_mfma.hip -- shortens the
    // attention launch but needs a launch of its own per layer: every call measured slower, profiles/r06_shared_prefix_mfma_ab.txt)
    CK(launch_expand_prompt_rows(q.prompt, q.prompt_stride, g.ids, g.ids_ld, Bc, L0, group, b0, st));
    if (!q.fanout) {
      PrefillReq p; p.ids = q.prompt + (long)g_lo * q.prompt_stride; p.ids_stride = q.prompt_stride; p.B = g_hi - g_lo + 1; p.L = L0 - 1; p.ctx = q.ctx;
      IVG_TRY(r.prefill(p));
    }
  } else if (!q.embeds)
    CK((int)hipMemcpy2DAsync(g.ids, (size_t)g.ids_ld * 8, q.prompt + (long)b0 * q.prompt_stride, (size_t)q.prompt_stride * 8, (size_t)L0 * 8, Bc,
                             hipMemcpyDeviceToDevice, st));
  if (q.uniforms)
    CK((int)hipMemcpy2DAsync(g.uni, (size_t)g.ids_ld * 4, q.uniforms + (long)b0 * n_new, (size_t)n_new * 4, (size_t)n_new * 4, Bc,
                             hipMemcpyDeviceToDevice, st));
  if (q.actions) {
    CK(launch_action_embed(q.actions + (long)b0 * act_T * c.action_dim, e->act_w, e->act_b, g.act_emb, dt, Bc * act_T, c.action_dim, H, st));
    if (q.B <= g.Bc && !q.fanout) CK((int)hipMemcpyAsync(g.last_act, q.actions, (size_t)q.B * act_T * c.action_dim * 4, hipMemcpyDeviceToDevice, st));
  }
  if (!q.reuse_kv && !shared) {
    PrefillReq p; p.ids = g.ids; p.ids_stride = g.ids_ld; p.B = Bc; p.L = L0; p.act_emb = q.actions ? g.act_emb : nullptr; p.act_T = act_T; p.ctx = q.ctx;
    p.all_slots = true; p.logits_last = g.logits; p.hidden_last = g.x; p.embeds = q.embeds;
    IVG_TRY(r.prefill(p));
  }
  if (q.embeds) {   // keep what the cache is (being) built from: the whole prompt after a prefill, its last row on the kept-cache path
    const int p0 = q.reuse_kv ? L0 - 1 : 0;
    CK((int)hipMemcpy2DAsync(e->emb_snap + (size_t)p0 * H * es, (size_t)e->Lmax * H * es, (const char*)q.embeds + (size_t)p0 * H * es,
                             (size_t)L0 * H * es, (size_t)(L0 - p0) * H * es, Bc, hipMemcpyDeviceToDevice, st));
    if (q.reuse_kv)   // the input row of the first forward pass comes straight from the caller
      CK((int)hipMemcpy2DAsync(g.x, (size_t)H * es, (const char*)q.embeds + (size_t)(L0 - 1) * H * es, (size_t)L0 * H * es, (size_t)H * es, Bc,
                               hipMemcpyDeviceToDevice, st));
  }
  return 0;
}

// The chunk's n_new decisions: the first step(s) eagerly, the rest as replays of the captured step graphs; the heads that read the last
// forward pass (reward_out, hidden_out) before the final decide-only step
static int run_steps(Run& r, const GenerateReq& q, const GenBuf& g, const Chunk& k) {
  ivg_engine* e = r.e; hipStream_t st = r.st;
  const ivg_config& c = e->cfg;
  const DType dt = e->llm_dt;
  const int b0 = k.b0, Bc = k.Bc, L0 = q.L0, n_new = q.n_new, H = c.hidden_size, V = c.vocab_size;
  const StepOpts& o = k.o;
  // reuse_kv: the cache already holds positions [0, L0 - 1); the step counter starts at j = 0, whose "decision" is the
  // forced sdf the prompt ends with (0 % 17 == 0): the sampler re-embeds it with the new action and the forward pass of
  // that step appends position L0 - 1 and yields the logits of new token 1 -- exactly what the prefill would have left
  const bool feed_last = q.reuse_kv || o.sh_P > 0;   // the cache holds [0, L0 - 1): step j = 0 feeds the prompt's last token
  CK(launch_state_set(g.state, feed_last ? L0 - 1 : L0, feed_last ? 0 : 1, st));
  SampleArgs sa{};
  sa.logits = g.logits; sa.V = V;
  sa.uniforms = q.uniforms ? g.uni : nullptr; sa.n_uni = g.ids_ld;
  sa.top_k = q.top_k;
  sa.ids_out = g.ids; sa.ids_stride = g.ids_ld; sa.L0 = L0;
  sa.forced_period = (q.actions || q.force_sdf) ? 17 : 0; sa.forced_token = V - 1;   // (no action embedding is added without actions: sa.act == null)
  sa.E = e->embed; sa.x = g.x; sa.H = H;
  sa.act = q.actions ? g.act_emb : nullptr; sa.act_T = q.act_T; sa.ctx = q.ctx;
  sa.slot0 = q.actions ? (L0 - 257 * q.ctx) / 17 : 0;  // a prompt that already holds t generated frames (MBRL step-wise rollout)
  sa.state = g.state;
  sa.temperature = e->temperature;
  sa.top_p = e->top_p;
  // reward head: reads the residual stream left by the LAST forward pass, i.e. before the final decide-only step
  // overwrites it with the embedding of the last token (mbrl/video_predictor.py:311-313: hidden state of the last step)
  auto reward = [&]() -> int {
    if (q.hidden_out) {   // hidden_states[-1][-1] of HF generate: the last forward pass, after the final norm
      if (!e->final_norm) return e->fail(IVG_ERR_MISSING, "generate: hidden state requested but 'llm.norm' is not in the weight table");
      CK(launch_final_hidden(g.x, e->final_norm, (char*)q.hidden_out + (size_t)b0 * H * esz(dt), Bc, H, c.rms_norm_eps, dt, st));
    }
    if (!q.reward_out) return 0;
    if (!e->rew_w) return e->fail(IVG_ERR_MISSING, "generate: reward requested but reward_linear is not loaded");
    CK(launch_rowdot(g.x, e->rew_w, e->rew_b, q.reward_out + b0, Bc, H, c.rms_norm_eps, dt, st));
    return 0;
  };
  // steps of this call that feed new tokens [j0, j0 + n) and carry frame_heads_kernel: those that hit a frame (test hook)
  auto note_frames = [&](int j0, int n) {
    if (!(o.fr_rew || o.fr_hid)) return;
    int hits = 0;
    for (int t = j0; t < j0 + n; ++t) hits += t % 17 == 16 && t / 17 < g.F_max;
    frame_heads_note(hits);
  };
  // steps of this call that ran the sampler, and token_scores_kernel after it (test hook)
  auto note_scores = [&](int n) { if (o.scored) token_scores_note(n); if (o.filtered) filtered_scores_note(n); };
  int j = 1;
  // step 1 eagerly (also performs every kernel's one-time attribute setup), then replay a captured step graph
  if (feed_last) { IVG_TRY(step_body(e, st, g, o, Bc, sa, true, q.embeds != nullptr)); if (!q.embeds) note_scores(1); }   // j = 0: feed the prompt's last token
  if (n_new == 1) IVG_TRY(reward());
  if (n_new >= 1) { IVG_TRY(step_body(e, st, g, o, Bc, sa, j < n_new)); note_scores(1); if (j < n_new) note_frames(j, 1); ++j; }
  // the step sequence is position-independent (all step-dependent scalars live in StepState): it is captured once as a graph of
  // ONE step and once as a graph of `multi` consecutive steps -- the long rollouts replay the multi-step graph (a graph launch
  // costs the host ~10-16 us and leaves a bubble on the device; 8 steps per launch amortise it), the tail the single-step one
  // (the same step graph serves both entry modes)
  constexpr int multi = 8;
  hipGraphExec_t exec = nullptr, exec_multi = nullptr;
  const std::string key = j < n_new ? step_key(e, o, sa, Bc) : std::string();
  if (j < n_new) IVG_TRY(step_graph(e, st, key, 1, g, o, Bc, sa, &exec));
  if (exec && multi > 1 && n_new - j >= 2 * multi) IVG_TRY(step_graph(e, st, key, multi, g, o, Bc, sa, &exec_multi));
  while (j < n_new) {
    if (exec_multi && n_new - j >= multi) { CK((int)hipGraphLaunch(exec_multi, st)); note_frames(j, multi); note_scores(multi); j += multi; }
    else if (exec) { CK((int)hipGraphLaunch(exec, st)); note_frames(j, 1); note_scores(1); ++j; }
    else { IVG_TRY(step_body(e, st, g, o, Bc, sa, true)); note_frames(j, 1); note_scores(1); ++j; }
  }
  if (j == n_new && n_new > 1) {
    IVG_TRY(reward());
    IVG_TRY(step_body(e, st, g, o, Bc, sa, false));  // decide the last token (no forward)
    note_scores(1);
  }
  return 0;
}

// The chunk's rows of every output the call asked for, out of the step buffers
static int copy_chunk_out(Run& r, const GenerateReq& q, const GenBuf& g, const Chunk& k) {
  ivg_engine* e = r.e; hipStream_t st = r.st;
  const DType dt = e->llm_dt;
  const int b0 = k.b0, Bc = k.Bc, L0 = q.L0, n_new = q.n_new, H = e->cfg.hidden_size;
  const size_t es = esz(dt);
  const long Ltot = (long)L0 + n_new;
  const int F_out = n_new / 17;   // frames whose 16th token, new token 17 i + 16, is fed (<= n_new - 1)
  if (q.embeds) {
    CK((int)hipMemcpy2DAsync(q.new_ids_out + (long)b0 * n_new, (size_t)n_new * 8, g.ids + L0, (size_t)g.ids_ld * 8, (size_t)n_new * 8, Bc,
                             hipMemcpyDeviceToDevice, st));
    if (n_new > 1)   // inputs of the positions the steps appended: the embeddings of the fed new tokens
      CK(launch_embed(g.ids + L0, g.ids_ld, e->embed, e->emb_snap + (size_t)L0 * H * es, dt, Bc, n_new - 1, H, e->cfg.vocab_size, st, (long)e->Lmax * H));
  } else {
    CK((int)hipMemcpy2DAsync(q.ids_out + (long)b0 * Ltot, (size_t)Ltot * 8, g.ids, (size_t)g.ids_ld * 8, (size_t)Ltot * 8, Bc,
                             hipMemcpyDeviceToDevice, st));
  }
  if (k.o.fr_rew)
    CK((int)hipMemcpy2DAsync(q.frame_rewards_out + (long)b0 * F_out, (size_t)F_out * 4, g.frame_rew, (size_t)g.F_max * 4, (size_t)F_out * 4, Bc,
                             hipMemcpyDeviceToDevice, st));
  if (k.o.scored)
    CK((int)hipMemcpy2DAsync(q.token_scores_out + (long)b0 * n_new * 3, (size_t)n_new * 12, g.tok_scores, (size_t)g.ids_ld * 12, (size_t)n_new * 12, Bc,
                             hipMemcpyDeviceToDevice, st));
  if (k.o.filtered)
    CK((int)hipMemcpy2DAsync(q.filtered_scores_out + (long)b0 * n_new * 4, (size_t)n_new * 16, g.filt_scores, (size_t)g.ids_ld * 16, (size_t)n_new * 16, Bc,
                             hipMemcpyDeviceToDevice, st));
  if (k.o.fr_hid)
    CK((int)hipMemcpy2DAsync((char*)q.frame_hidden_out + (size_t)b0 * F_out * H * es, (size_t)F_out * H * es, g.frame_hid, (size_t)g.F_max * H * es,
                             (size_t)F_out * H * es, Bc, hipMemcpyDeviceToDevice, st));
  return 0;
}

// group > 1 (ivg_generate_shared): `prompt` holds one row per GROUP of `group` consecutive trajectories (B = groups x group rows of
// actions / uniforms / ids_out).  Per chunk: the prompts of the groups the chunk's rows belong to are prefilled ONCE each -- positions
// [0, L0 - 1), into cache rows 0 .. n_groups-1 -- and every trajectory then feeds the prompt's last token itself (step j = 0, exactly the
// kept-cache entry of the step-wise callers: that slot carries the row's own action), appending from position L0 - 1 on in its own
// cache row; the decode attention reads key rows < L0 - 1 from the group's row (decode_attn_kernel SHARED).
int Run::generate(const GenerateReq& q) {
  const int B = q.B, L0 = q.L0, group = q.group;
  const GenBuf g = gen_buf(e);
  // fanout (ivg_generate_fanout): the shared branch with the kept cache as the groups' prefix -- one chunk (the entry checks it), group
  // s's prefix already in cache row s, no prompt pass; the kept state is put back at the end exactly as it was
  const bool fanout = q.fanout;
  const bool shared = group > 1 || fanout;
  const int kept_act_T = e->kvc.last_act_T, kept_ctx = e->kvc.last_ctx;   // (what the fan-out restores)
  if (planning) {   // the prompt pass of the largest chunk (shared: of the most groups a chunk's rows can belong to)
    PrefillReq p; p.ctx = q.ctx; p.L = shared ? L0 - 1 : L0;
    p.B = shared ? std::min((std::min(B, g.Bc) + group - 1) / group + 1, std::min(B, g.Bc)) : std::min(B, g.Bc);
    return (q.reuse_kv && !shared) || fanout ? 0 : prefill(p);
  }
  e->kvc.forget_kept();   // kept again once every launch of this call is queued
  if (q.embeds && B > g.Bc) return e->fail(IVG_ERR_CAPACITY, "generate (inputs_embeds): batch exceeds the KV-cache chunk");
  if (q.embeds && !e->emb_snap) {   // one-time: copy of the inputs the cache is built from (verifies later "same prefix" claims)
    if (hipMalloc((void**)&e->emb_snap, (size_t)g.Bc * e->Lmax * e->cfg.hidden_size * esz(e->llm_dt)) != hipSuccess)
      return e->fail(IVG_ERR_HIP, "hipMalloc of the embeddings snapshot failed");
  }
  for (int b0 = 0; b0 < B; b0 += g.Bc) {
    Chunk k{b0, std::min(g.Bc, B - b0), StepOpts()};
    if (shared) { k.o.sh_P = L0 - 1; k.o.sh_G = group; k.o.sh_row0 = b0 / group * group - b0; }
    k.o.fr_rew = q.frame_rewards_out != nullptr; k.o.fr_hid = q.frame_hidden_out != nullptr; k.o.scored = q.token_scores_out != nullptr;
    k.o.filtered = q.filtered_scores_out != nullptr;
    IVG_TRY(stage_chunk(*this, q, g, k));
    IVG_TRY(run_steps(*this, q, g, k));
    IVG_TRY(copy_chunk_out(*this, q, g, k));
  }
  // the last new token is decided but never fed (a shared-context cache is not a per-trajectory cache: never kept)
  if (B <= g.Bc && !shared) e->kvc.keep(L0 + q.n_new - 1, B, q.embeds != nullptr, q.actions ? q.act_T : 0, q.ctx);
  if (fanout) {
    // the candidates' own rows lie at positions >= L0 - 1, outside the kept state; the id rows of the kept trajectories were overwritten
    // by the expanded prompts (rows [0, B / group) of candidates), the action table was never touched
    const int n_groups = B / group;
    CK((int)hipMemcpy2DAsync(g.ids, (size_t)g.ids_ld * 8, q.prompt, (size_t)q.prompt_stride * 8, (size_t)L0 * 8, n_groups, hipMemcpyDeviceToDevice, st));
    e->kvc.keep(L0 - 1, n_groups, false, kept_act_T, kept_ctx);
  }
  return 0;
}

// ---------------------------------------------------------------------------------------- kept-cache verification
static int read_flag(ivg_engine* e, const GenBuf& g, hipStream_t st, bool* ok) {
  if (!e->h_flag && hipHostMalloc((void**)&e->h_flag, sizeof(int), hipHostMallocDefault) != hipSuccess) return e->fail(IVG_ERR_HIP, "hipHostMalloc failed");
  CK((int)hipMemcpyAsync(e->h_flag, g.flag, sizeof(int), hipMemcpyDeviceToHost, st));
  CK((int)hipStreamSynchronize(st));
  *ok = *e->h_flag == 0;
  return 0;
}

// positions [0, len) of the B kept trajectories against prompt[:, :len] and the action rows of the sdf slots among them
// (ivg_generate_continue: len = the kept length; ivg_kv_extend: any prefix of it; ids_only, ivg_generate_fanout: the kept action table
// defined the cache rows and the candidates' rows for those slots are not looked at)
int kv_prefix_matches_ids(ivg_engine* e, const int64_t* prompt, int64_t prompt_stride, int B, int len, const float* actions, int act_T,
                          int ctx, hipStream_t st, bool* ok, bool ids_only) {
  *ok = false;
  const GenBuf g = gen_buf(e);
  if (!e->kvc.ids_valid || e->kvc.B != B || len < 1 || len > e->kvc.len || B > g.Bc) return 0;
  // the cache must have been built the same way: with / without actions, the same context length, the same action-table shape;
  // whatever cannot be compared row for row is a mismatch, never a silent "ok"
  if ((actions != nullptr) != (e->kvc.last_act_T > 0)) return 0;
  if (ctx != e->kvc.last_ctx) return 0;
  if (actions && !ids_only && (e->kvc.last_act_T != act_T)) return 0;
  CK((int)hipMemsetAsync(g.flag, 0, sizeof(int), st));
  CK(launch_compare_rows(prompt, prompt_stride * 8, g.ids, (long)g.ids_ld * 8, B, (long)len * 8, g.flag, st));
  if (actions && !ids_only) {   // the action rows already baked into the cached sdf slots: slot i (position 257*ctx - 1 + 17*i < kv_len) used row i + ctx - 1
    const int A = e->cfg.action_dim;
    const int slots = std::max(0, (len - (257 * ctx - 1) + 16) / 17);
    if (slots > 0 && ctx - 1 + slots > act_T) return 0;   // the cached slots used action rows the presented table does not have
    if (slots > 0)
      CK(launch_compare_rows(actions + (long)(ctx - 1) * A, (long)act_T * A * 4, g.last_act + (long)(ctx - 1) * A, (long)act_T * A * 4, B,
                             (long)slots * A * 4, g.flag, st));
  }
  return read_flag(e, g, st, ok);
}

int kv_prefix_matches_embeds(ivg_engine* e, const void* embeds, int B, int L0, hipStream_t st, bool* ok) {
  *ok = false;
  const GenBuf g = gen_buf(e);
  if (!e->kvc.snap_valid || !e->emb_snap || !e->kvc.holds(B, L0 - 1) || B > g.Bc) return 0;
  const size_t es = esz(e->llm_dt);
  const long H = e->cfg.hidden_size;
  CK((int)hipMemsetAsync(g.flag, 0, sizeof(int), st));
  CK(launch_compare_rows(embeds, (long)L0 * H * es, e->emb_snap, (long)e->Lmax * H * es, B, (long)(L0 - 1) * H * es, g.flag, st));
  return read_flag(e, g, st, ok);
}

// ---------------------------------------------------------------------------------------- kept-cache extension (ivg_kv_extend)
bool kv_extend_chunk_covers(const ivg_engine* e) {
  return sw().kv_extend_chunk && e->kvc.format == KvFormat::Native && e->llm_dt == BF16 && e->hd == 64;   // IVG_KV_EXTEND_CHUNK=0: decode steps (A/B tests)
}

int kv_extend_frames(int keep_len, int L0, int ctx, int* i_first) {
  const int q0 = 257 * ctx + 15;
  const int first = keep_len <= q0 ? 0 : (keep_len - q0 + 16) / 17;
  if (i_first) *i_first = first;
  if (L0 - 2 < q0) return 0;
  return std::max(0, (L0 - 2 - q0) / 17 - first + 1);
}

// Teacher-forces positions [keep_len, L0 - 1) onto the kept cache.  chunk: one pass over the B * T rows through Run::prefill's layers
// (append mode: RoPE at keep_len, chunk_attn_kernel).  Otherwise T eager decode steps whose input rows are given instead of sampled --
// exactly the launches generate's own steps make after the sampler, so the appended rows are bit for bit what a rollout that had
// sampled these tokens would have appended, in every cache format.  Neither touches a captured step graph.
int Run::extend(const ExtendReq& q) {
  const ivg_config& c = e->cfg;
  const DType dt = e->llm_dt;
  const int H = c.hidden_size, V = c.vocab_size, B = q.B, T = q.L0 - 1 - q.keep_len, A = c.action_dim;
  const size_t es = esz(dt);
  const GenBuf g = gen_buf(e);
  // ivg_kv_extend_scored: frames i_first .. i_first + F_out - 1 have their 16th token among the fed positions; score column c has its
  // target at position keep_len + c + 1, forced (under the forced schedule: actions given) when that is an sdf slot
  int i_first = 0;
  const bool want_frames = q.frame_rewards || q.frame_hidden;
  const int F_out = want_frames ? kv_extend_frames(q.keep_len, q.L0, q.ctx, &i_first) : 0;
  const int q_first = 257 * q.ctx + 17 * i_first + 15;
  const int slot_d = q.keep_len + 1 - (257 * q.ctx - 1);   // (target of column 0) - (first sdf slot)
  const int first_forced = slot_d <= 0 ? -slot_d : (17 - slot_d % 17) % 17, period = q.actions ? 17 : 0;
  if (!planning) e->kvc.forget_kept();   // rows from keep_len on are about to be overwritten; kept again once every launch is queued
  if (!planning && q.actions) CK(launch_action_embed(q.actions, e->act_w, e->act_b, g.act_emb, dt, B * q.act_T, A, H, st));
  if (q.chunk) {
    PrefillReq p; p.ids = q.prompt + q.keep_len; p.ids_stride = q.prompt_stride; p.B = B; p.L = T; p.ctx = q.ctx;
    p.act_emb = q.actions ? g.act_emb : nullptr; p.act_T = q.act_T; p.all_slots = true;
    p.append = true; p.pos0 = q.keep_len;
    if (q.token_nll || q.token_scores) p.next_ids = q.prompt + q.keep_len + 1;
    p.token_nll = q.token_nll;
    p.token_scores = q.token_scores; p.ts_first_forced = first_forced; p.ts_period = period;
    if (F_out > 0) { p.frame_rew = q.frame_rewards; p.frame_hid = q.frame_hidden; p.fr_row0 = q_first - q.keep_len; p.fr_F = F_out; }
    IVG_TRY(prefill(p));
  } else if (!planning) {
    CK(launch_state_set(g.state, q.keep_len, 0, st));   // (every step's lm_head advances the position)
    const SampleArgs none{};                            // the sampler never runs
    const StepOpts plain;                               // per-trajectory rows, no frame heads, no token scores
    for (int t = 0; t < T; ++t) {
      const int pos = q.keep_len + t;
      CK(launch_embed(q.prompt + pos, q.prompt_stride, e->embed, g.x, dt, B, 1, H, V, st));
      const int slot = pos - (257 * q.ctx - 1);
      if (q.actions && slot >= 0 && slot % 17 == 0)   // sdf slot i = slot / 17 carries action row i + ctx - 1
        CK(launch_add_rows(g.x, H, g.act_emb + (size_t)(slot / 17 + q.ctx - 1) * H * es, (long)q.act_T * H, B, H, dt, st));
      IVG_TRY(step_body(e, st, g, plain, B, none, true, true));
      if (q.token_nll) CK(launch_token_nll(g.logits, q.prompt + pos + 1, q.prompt_stride, 0, B, 1, V, q.token_nll + t, T, st));
      // the heads of ivg_kv_extend_scored, launched by the host (these steps are eager): g.x is the residual row this step left (lm_head
      // only reads it), g.logits the row the next decision would read -- what the rollout's own steps hand frame_heads_kernel and
      // token_scores_kernel
      if (F_out > 0 && pos >= q_first && (pos - q_first) % 17 == 0 && (pos - q_first) / 17 < F_out)
        CK(launch_frame_rows_heads(g.x, 0, 1, 0, e->rew_w, e->rew_b, e->final_norm, q.frame_rewards, q.frame_hidden, B, H, 1, (pos - q_first) / 17, F_out,
                                   c.rms_norm_eps, dt, st));
      if (q.token_scores) {
        const bool forced = period > 0 && t >= first_forced && (t - first_forced) % period == 0;
        CK(launch_token_scores_rows(g.logits, q.prompt + pos + 1, q.prompt_stride, 0, B, 1, V, 0, forced ? 1 : 0, q.token_scores + (size_t)t * 3, T, st));
      }
    }
  }
  if (planning) return 0;
  // the kept state: id columns [keep_len, L0 - 1] and the action table are the caller's
  // (column L0 - 1, the token given but not yet fed, has no place in a cache extended to its last position)
  CK((int)hipMemcpy2DAsync(g.ids + q.keep_len, (size_t)g.ids_ld * 8, q.prompt + q.keep_len, (size_t)q.prompt_stride * 8,
                           (size_t)(std::min(q.L0, g.ids_ld) - q.keep_len) * 8, B, hipMemcpyDeviceToDevice, st));
  if (q.actions) CK((int)hipMemcpyAsync(g.last_act, q.actions, (size_t)B * q.act_T * A * 4, hipMemcpyDeviceToDevice, st));
  e->kvc.keep(q.L0 - 1, B, false, q.actions ? q.act_T : 0, q.ctx);
  kv_extend_note(q.chunk ? B * T : 0, q.chunk ? 0 : B * T);
  kv_extend_heads_note(B * F_out, q.token_scores ? B * T : 0);
  return 0;
}

// ---------------------------------------------------------------------------------------- kept-cache row selection (ivg_kv_select)
// the buffers whose rows belong to the kept trajectories: the K / V slabs in the cache's own format, and what the verification above
// compares a caller's "same prefix" claim with -- the id rows, the action table, the embeddings snapshot
struct KeptBufs { KvSelectBuf kv, ids, act, emb; };   // act / emb: bytes_a == 0 where the kept state has no action table / no embeddings snapshot

// ... of a kept state given by value: `len` positions, an action table of act_T rows, with or without the embeddings snapshot
// (ivg_kv_snapshot_restore describes the state it is about to install; everyone else the one the engine holds)
static KeptBufs kept_bufs(const ivg_engine* e, const GenBuf& g, int len, int act_T, bool snap) {
  const KvCache& k = e->kvc;
  const long eb = (long)k.elem_bytes(), blk = (long)k.Lmax * k.hd * eb;
  KeptBufs r;
  KvSelectBuf& c = r.kv;
  c.base = k.base; c.slabs = k.layers * 2; c.row_stride = (long)k.heads * blk; c.slab_stride = (long)k.chunk * c.row_stride;
  c.heads = k.heads; c.head_stride = blk;
  if (k.format == KvFormat::Planes24) { c.bytes_a = (long)len * k.hd * 2; c.bytes_b = (long)len * k.hd; c.plane_b = (long)k.Lmax * k.hd * 2; }
  else c.bytes_a = (long)len * k.hd * eb;
  KvSelectBuf& ids = r.ids;
  ids.base = (char*)g.ids; ids.row_stride = (long)g.ids_ld * 8; ids.bytes_a = (long)std::min(len + 1, g.ids_ld) * 8; ids.vec = 4;   // (column len: decided, not yet fed)
  if (act_T > 0) {
    KvSelectBuf& a = r.act;
    a.base = (char*)g.last_act; a.row_stride = (long)act_T * e->cfg.action_dim * 4; a.bytes_a = a.row_stride; a.vec = 4;
  }
  if (snap) {
    const long rowb = (long)e->cfg.hidden_size * (long)esz(e->llm_dt);
    KvSelectBuf& s = r.emb;
    s.base = e->emb_snap; s.row_stride = (long)e->Lmax * rowb; s.bytes_a = (long)len * rowb;
  }
  return r;
}

static void kv_select_bufs(const ivg_engine* e, const GenBuf& g, std::vector<KvSelectBuf>& out) {
  const KvCache& k = e->kvc;
  const KeptBufs r = kept_bufs(e, g, k.len, k.last_act_T, k.snap_valid && e->emb_snap);
  out.push_back(r.kv);
  out.push_back(r.ids);
  if (r.act.bytes_a > 0) out.push_back(r.act);
  if (r.emb.bytes_a > 0) out.push_back(r.emb);
}

size_t kv_select_scratch_bytes(const ivg_engine* e) {   // (a native K / V slab and the embeddings snapshot are the same size; the id rows the rest)
  return (size_t)e->kvc.chunk * e->Lmax * std::max<size_t>((size_t)e->cfg.hidden_size * esz(e->llm_dt), 8);
}

int need_kept_cache(ivg_engine* e, const char* entry) {
  const KvCache& k = e->kvc;
  if (k.len > 0 && k.B > 0 && (k.ids_valid || k.snap_valid)) return 0;
  return e->fail(IVG_ERR_INVALID, std::string(entry) + ": the engine holds no kept cache (the last call was not a per-trajectory generate within the cache chunk, or the format or scales changed since)");
}

int kv_select(ivg_engine* e, const int32_t* parents, int n, hipStream_t st) {
  KvCache& k = e->kvc;
  IVG_TRY(need_kept_cache(e, "kv_select"));
  if (!parents || n <= 0) return e->fail(IVG_ERR_INVALID, "kv_select: parents must hold at least one row");
  KvSelectPlan plan;
  const int prc = kv_select_plan(parents, n, k.B, k.chunk, &plan);
  if (prc == KV_PLAN_CAPACITY) return e->fail(IVG_ERR_CAPACITY, "kv_select: " + std::to_string(n) + " rows exceed the KV-cache chunk (" + std::to_string(k.chunk) + ")");
  if (prc != KV_PLAN_OK) return e->fail(IVG_ERR_INVALID, "kv_select: every parent must be a row of the kept cache, [0, " + std::to_string(k.B) + ")");
  if (plan.n_direct + plan.n_staged > 0) {
    std::vector<KvSelectBuf> bufs;
    kv_select_bufs(e, gen_buf(e), bufs);
    for (const KvSelectBuf& b : bufs)   // refused before the first launch: a select never leaves the buffers half gathered
      if (plan.n_staged > 0 && (!e->ws.base || b.staged_bytes_per_slab(plan.n_staged) > e->ws.cap))
        return e->fail(IVG_ERR_CAPACITY, "kv_select: the workspace does not hold one slab's staged rows");
    for (const KvSelectBuf& b : bufs) CK(launch_kv_select(b, plan, e->ws.base, e->ws.cap, st));
    kv_select_note(plan.n_direct, plan.n_staged);
  }
  k.B = n;
  return 0;
}

// ---------------------------------------------------------------------------------------- kept-cache snapshots (ivg_kv_snapshot_*)
static size_t part_bytes(const ivg_kv_snapshot::Part& p, int rows) { return (size_t)p.slabs * rows * p.heads * (size_t)(p.bytes_a + p.bytes_b); }

int kv_snapshot_create(ivg_engine* e, ivg_kv_snapshot** out, hipStream_t st) {
  IVG_TRY(need_kept_cache(e, "kv_snapshot_create"));
  const KvCache& k = e->kvc;
  const GenBuf g = gen_buf(e);
  const KeptBufs kb = kept_bufs(e, g, k.len, k.last_act_T, k.snap_valid && e->emb_snap);
  ivg_kv_snapshot s;
  s.device = e->device;
  s.len = k.len; s.B = k.B; s.ids_valid = k.ids_valid; s.snap_valid = k.snap_valid; s.act_T = k.last_act_T; s.ctx = k.last_ctx;
  s.id_cols = (int)(kb.ids.bytes_a / 8);
  s.layers = k.layers; s.heads = k.heads; s.hd = k.hd; s.hidden = e->cfg.hidden_size; s.action_dim = e->cfg.action_dim;
  s.dt = e->llm_dt; s.x3 = e->llm_x3; s.format = k.format;
  s.table = k.table; s.k_scale = k.k_scale; s.v_scale = k.v_scale; s.scales = k.scales;
  s.embed = e->embed; s.lm_head = e->lm_head;
  // the 16-byte parts first: every part then starts at a multiple of its own vector with no padding in between
  const KvSelectBuf* bufs[4] = {&kb.kv, &kb.emb, &kb.ids, &kb.act};
  ivg_kv_snapshot::Part* parts[4] = {&s.kv, &s.emb, &s.ids, &s.act};
  for (int i = 0; i < 4; ++i) {
    ivg_kv_snapshot::Part& p = *parts[i];
    p.off = s.bytes; p.slabs = bufs[i]->slabs; p.heads = bufs[i]->heads; p.bytes_a = bufs[i]->bytes_a; p.bytes_b = bufs[i]->bytes_b; p.vec = bufs[i]->vec;
    s.bytes += part_bytes(p, s.B);
  }
  if (hipMalloc((void**)&s.mem, s.bytes) != hipSuccess) {
    (void)hipGetLastError();
    return e->fail(IVG_ERR_HIP, "kv_snapshot_create: hipMalloc of " + std::to_string(s.bytes) + " bytes failed");
  }
  for (int i = 0; i < 4; ++i)
    if (const int rc = launch_kv_snapshot(*bufs[i], s.mem + parts[i]->off, s.B, nullptr, s.B, false, st)) {
      (void)hipDeviceSynchronize();   // (launches already queued write the allocation)
      (void)hipFree(s.mem);
      return e->fail(IVG_ERR_HIP, "kv_snapshot_create: launch failed: hip error " + std::to_string(rc));
    }
  kv_snapshot_note(s.B, 0);
  *out = new ivg_kv_snapshot(std::move(s));
  return 0;
}

int kv_snapshot_restore(ivg_engine* e, const ivg_kv_snapshot* s, const int32_t* parents, int n, hipStream_t st) {
  KvCache& k = e->kvc;
  auto no = [&](const std::string& what) { return e->fail(IVG_ERR_INVALID, "kv_snapshot_restore: " + what); };
  if (parents && n <= 0) return no("parents must hold at least one row");
  if (!parents) n = s->B;
  if (s->device != e->device) return no("the snapshot lives on device " + std::to_string(s->device) + ", the engine on " + std::to_string(e->device));
  if (s->layers != k.layers || s->heads != k.heads || s->hd != k.hd || s->hidden != e->cfg.hidden_size || s->action_dim != e->cfg.action_dim)
    return no("the snapshot was taken from a transformer of another geometry (layers, heads, head_dim, hidden size or action_dim differ)");
  if (s->dt != e->llm_dt || s->x3 != e->llm_x3 || s->format != k.format)
    return no("the snapshot's element type or K/V format is not this engine's");
  if (k.format == KvFormat::Fp8) {
    const bool same = s->table == k.table &&
                      (k.table ? s->scales.size() == k.scales.size() && !memcmp(s->scales.data(), k.scales.data(), k.scales.size() * 4)
                               : !memcmp(&s->k_scale, &k.k_scale, 4) && !memcmp(&s->v_scale, &k.v_scale, 4));
    if (!same) return no("the FP8 scales in force differ from the ones the snapshot's bytes were written with");
  }
  if (s->embed != e->embed || s->lm_head != e->lm_head) return no("the snapshot was taken over other weights");
  if (parents)
    for (int i = 0; i < n; ++i)
      if (parents[i] < 0 || parents[i] >= s->B) return no("every parent must be a row of the snapshot, [0, " + std::to_string(s->B) + ")");
  const GenBuf g = gen_buf(e);
  if (n > k.chunk) return e->fail(IVG_ERR_CAPACITY, "kv_snapshot_restore: " + std::to_string(n) + " rows exceed the KV-cache chunk (" + std::to_string(k.chunk) + ")");
  if (s->len > k.Lmax || s->id_cols > g.ids_ld)
    return e->fail(IVG_ERR_CAPACITY, "kv_snapshot_restore: " + std::to_string(s->len) + " kept positions exceed the KV cache (" + std::to_string(k.Lmax) + ")");
  if (s->act_T > e->cfg.max_frames)
    return e->fail(IVG_ERR_CAPACITY, "kv_snapshot_restore: an action table of " + std::to_string(s->act_T) + " rows exceeds max_frames (" + std::to_string(e->cfg.max_frames) + ")");
  const bool emb = s->emb.bytes_a > 0;
  if (emb && !e->emb_snap && hipMalloc((void**)&e->emb_snap, (size_t)g.Bc * e->Lmax * e->cfg.hidden_size * esz(e->llm_dt)) != hipSuccess) {
    (void)hipGetLastError(); e->emb_snap = nullptr;
    return e->fail(IVG_ERR_HIP, "hipMalloc of the embeddings snapshot failed");
  }
  KeptBufs kb = kept_bufs(e, g, s->len, s->act_T, emb);
  kb.ids.bytes_a = (long)s->id_cols * 8;   // (a snapshot of a full cache has no column len; it fits, checked above)
  const KvSelectBuf* bufs[4] = {&kb.kv, &kb.emb, &kb.ids, &kb.act};
  const ivg_kv_snapshot::Part* parts[4] = {&s->kv, &s->emb, &s->ids, &s->act};
  for (int i = 0; i < 4; ++i)   // the engine's description of the state must be the snapshot's, byte count for byte count
    if (bufs[i]->slabs != parts[i]->slabs || bufs[i]->heads != parts[i]->heads || bufs[i]->bytes_a != parts[i]->bytes_a ||
        bufs[i]->bytes_b != parts[i]->bytes_b || bufs[i]->vec != parts[i]->vec)
      return no("internal: the engine lays the kept state out differently from the snapshot");
  std::vector<int32_t> ident;
  if (!parents) { ident.resize(n); for (int i = 0; i < n; ++i) ident[i] = i; parents = ident.data(); }
  k.forget_kept();   // kept again once every launch is queued
  for (int i = 0; i < 4; ++i) CK(launch_kv_snapshot(*bufs[i], s->mem + parts[i]->off, s->B, parents, n, true, st));
  k.len = s->len; k.B = n; k.ids_valid = s->ids_valid; k.snap_valid = s->snap_valid; k.last_act_T = s->act_T; k.last_ctx = s->ctx;
  kv_snapshot_note(0, n);
  return 0;
}

}  // namespace ivg
