// Engine: owns the workspace arena, KV cache and the layer graphs of the tokenizer and transformer.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/ivg.h"
#include "ops.h"

namespace ivg {

struct Arena {
  char* base = nullptr;
  size_t cap = 0, off = 0, high = 0;
  bool planning = true;  // planning pass: no memory, only the high-water mark
  bool overflow = false;
  void* alloc(size_t bytes) {
    off = (off + 255) & ~(size_t)255;
    void* p = planning ? (void*)(uintptr_t)(0x1000 + off) : (void*)(base + off);
    off += bytes;
    if (off > high) high = off;
    if (!planning && off > cap) { overflow = true; return base; }  // never hand out memory past the arena (callers plan first)
    return p;
  }
  size_t mark() const { return off; }
  void reset(size_t m) { off = m; }
};

struct ConvW { const void* w = nullptr; const float* b = nullptr; int cin = 0, cout = 0, k = 1;
               const void* w3 = nullptr; /* fp32 3x3 convs of the "x3" decode mode: weights pre-split into bf16 (hi, lo) pairs */
               const void* wsub = nullptr; const void* wsub3 = nullptr; /* upsampler convs: pre-summed sub-pixel phase weights (+ x3 split) */ };
struct NormW { const float* g = nullptr; const float* b = nullptr; };
struct ResnetW { NormW n1, n2; ConvW c1, c2, sc; bool has_sc = false; int cin = 0, cout = 0; };
struct AttnW { NormW gn; ConvW q, k, v, o; };
struct XAttW { NormW kvn, qn; const float* kv_pos = nullptr; const float* q_pos = nullptr; int kv_rows = 0;
               ConvW q, k, v, o; int C = 0, side = 0; };
struct TrunkW {  // encoder or decoder
  const float* conv_in_raw_w = nullptr;  // encoders: fp32 [C0][3][3][3]
  ConvW conv_in;                          // decoders: packed (latent -> C)
  std::vector<std::vector<ResnetW>> blocks;
  std::vector<ConvW> resample;            // down/up-sampler conv of each level (cin = 0: none)
  ResnetW mid0, mid1;
  bool has_attn = false;
  AttnW attn;
  NormW norm_out;
  ConvW conv_out;
  std::vector<XAttW> xatt;
};
struct LayerW { const void* wqkv; const void* wo; const void* wgu; const void* wdown; };  // RMSNorm weights are folded into wqkv / wgu

struct Feature { void* p = nullptr; int side = 0, C = 0; };

// ---- the transformer's K / V cache and the one owner of its format: what an element is, where a layer's rows are, how the prompt pass and
// the decode step write and read them, and which prefix the rows kept from the last generate call belong to
// Native: the engine's own element type (bf16 / fp32).  Planes24: x3 rollout, head_dim 64 -- 24 of the 32 bits in two planes (llama_ops.hip:
// decode_attn24_kernel), latched at create.  Fp8: ivg_set_kv_format(IVG_KV_FP8_E4M3) -- a bf16 rollout's K / V as one e4m3 byte per element
// (decode_attn8_kernel), dense from the start of the native cache's allocation (which keeps its size).
enum class KvFormat { Native, Planes24, Fp8 };

#define KV_HIP(x) do { hipError_t _e = (x); if (_e != hipSuccess) { err = std::string(#x) + ": " + hipGetErrorString(_e); return IVG_ERR_HIP; } } while (0)

struct KvCache {
  KvFormat format = KvFormat::Native;
  DType dt = F32;            // the engine's element type: Native elements, and what the prompt pass stages for the other two formats
  int layers = 0, heads = 0, hd = 0, Lmax = 0;
  int chunk = 0;             // min(max_batch, 128): trajectories the cache holds = rows of one rollout / prompt-pass chunk
  char* base = nullptr;      // [layers][2][chunk][heads][Lmax][hd]  (Planes24: [layers][2][chunk][heads]{[Lmax][hd] u16 | [Lmax][hd] u8})
  float k_scale = 1.0f, v_scale = 1.0f;   // Fp8: byte = e4m3(x / scale)
  // ivg_set_kv_scales: per (layer, k|v, head) scales [layers][2][heads] used instead of the two scalars while `table` is set (the device
  // buffer is rewritten only after a device synchronisation); gen counts every change of format or scales and is part of the step-graph key
  float* scales_dev = nullptr;
  std::vector<float> scales;
  bool table = false;
  unsigned gen = 0;
  unsigned int* amax = nullptr;             // what ivg_kv_calibrate observed, [layers][2][heads] fp32 bit patterns
  hipStream_t calib_stream = nullptr;       // stream of the last ivg_kv_calibrate (calibrated_scales synchronises it)
  bool calib_pending = false;
  // the cache holds positions [0, len) of B trajectories (last generate call), and what they were built from, kept so that a step-wise
  // caller's "same prefix" claim can be VERIFIED on the device: the ids in the persistent id buffer + the action table of the call
  // (ids_valid), or the input embeddings fed so far in the engine's snapshot (snap_valid)
  int len = 0, B = 0;
  bool snap_valid = false, ids_valid = false;
  int last_act_T = 0;        // rows per trajectory of the kept action table (0: the cache was built without actions)
  int last_ctx = 0;          // context length of the call that built the kept cache (action slot positions depend on it)
  int prof_eb = 0;           // elem_bytes() of the call the decode-attention profile's stamps belong to (0: none yet)

  static constexpr const char* kFp8Needs = "the FP8 K/V cache needs a transformer with llm_dtype IVG_BF16 and head_dim 64";
  bool fp8_eligible() const { return scales_dev && amax; }   // create() gave the engine the FP8 cache's tables: a bf16 (not x3) transformer, head_dim 64
  size_t native_bytes() const { return dt == BF16 ? 2 : 4; }
  size_t elem_bytes() const {
    switch (format) {
      case KvFormat::Fp8: return 1;
      case KvFormat::Planes24: return 3;
      default: return native_bytes();
    }
  }
  size_t profiled_elem_bytes() const { return prof_eb > 0 ? (size_t)prof_eb : elem_bytes(); }
  size_t table_n() const { return (size_t)layers * 2 * heads; }
  char* ptr(int layer, int which) const { return base + ((size_t)layer * 2 + which) * chunk * heads * Lmax * hd * elem_bytes(); }   // which: 0 K, 1 V
  const float* tab(int layer, int which) const { return table ? scales_dev + ((size_t)layer * 2 + which) * heads : nullptr; }
  // "layer L, k|v, head H" of a flat index into a [layers][2][heads] table
  std::string name(size_t i) const { return "layer " + std::to_string(i / (2 * heads)) + ", " + ((i / heads) % 2 ? "v" : "k") + ", head " + std::to_string(i % heads); }

  // sized for the create-time format; engines the FP8 cache is for also get its scale table and the calibration's observations
  bool create(int layers_, int heads_, int hd_, int Lmax_, int max_batch, DType dt_, bool x3, bool planes24) {
    layers = layers_; heads = heads_; hd = hd_; Lmax = Lmax_; chunk = std::min(max_batch, 128); dt = dt_;
    format = planes24 ? KvFormat::Planes24 : KvFormat::Native;
    if (hipMalloc((void**)&base, (size_t)layers * 2 * chunk * heads * Lmax * hd * elem_bytes()) != hipSuccess) return false;
    if (layers <= 0 || x3 || dt != BF16 || hd != 64) return true;
    if (hipMalloc((void**)&scales_dev, table_n() * 4) != hipSuccess || hipMalloc((void**)&amax, table_n() * 4) != hipSuccess) return false;
    (void)hipMemset(scales_dev, 0, table_n() * 4); (void)hipMemset(amax, 0, table_n() * 4);
    return true;
  }
  void destroy() { (void)hipFree(base); (void)hipFree(scales_dev); (void)hipFree(amax); }   // (hipFree(null) is a no-op)

  void forget_kept() { len = 0; B = 0; snap_valid = false; ids_valid = false; }
  void keep(int len_, int B_, bool from_embeds, int act_T, int ctx) { len = len_; B = B_; snap_valid = from_embeds; ids_valid = !from_embeds; last_act_T = act_T; last_ctx = ctx; }
  bool holds(int B_, int len_) const { return B == B_ && len == len_; }

  // ---- prompt pass.  Native: RoPE appends to the cache itself.  Otherwise it writes (and the pass's attention reads) one layer's K / V
  // rows in the engine's element type in a staging pair of stage_bytes(B) each -- never packed in place: an FP8 byte row t overlaps
  // bf16 row t / 2 -- and store_staged moves them into the layer's cache rows
  bool staged() const { return format != KvFormat::Native; }
  size_t stage_bytes(int B_) const { return (size_t)B_ * heads * Lmax * hd * native_bytes(); }
  int store_staged(int l, const void* sk, const void* sv, int B_, int L, hipStream_t st) const {
    switch (format) {
      case KvFormat::Planes24: return launch_kv24_pack(sk, sv, ptr(l, 0), ptr(l, 1), B_ * heads, L, Lmax, st);
      case KvFormat::Fp8: return launch_kv8_pack(sk, sv, ptr(l, 0), ptr(l, 1), B_ * heads, L, Lmax, k_scale, v_scale, st, heads, tab(l, 0), tab(l, 1));
      default: return 0;
    }
  }
  // ---- decode step: the attention launch of layer l over this cache (sh_*: shared-context rollout, decode_attn_kernel SHARED)
  int decode_attn(int l, const void* qkv, void* out, const float* cosT, const float* sinT, int B_, const StepState* state, unsigned long long* prof,
                  hipStream_t st, int sh_P, int sh_G, int sh_row0) const {
    switch (format) {
      case KvFormat::Fp8: return launch_decode_attn8(qkv, ptr(l, 0), ptr(l, 1), out, cosT, sinT, B_, heads, Lmax, state, prof, k_scale, v_scale, st, sh_P, sh_G, sh_row0,
                                                     tab(l, 0), tab(l, 1));
      case KvFormat::Planes24: return launch_decode_attn24(qkv, ptr(l, 0), ptr(l, 1), out, cosT, sinT, B_, heads, Lmax, state, prof, st, sh_P, sh_G, sh_row0);
      default: return launch_decode_attn(qkv, ptr(l, 0), ptr(l, 1), out, cosT, sinT, B_, heads, hd, Lmax, state, prof, dt, st, sh_P, sh_G, sh_row0);
    }
  }
  // what a captured step bakes in of the cache: kernel and arguments (the scales by their bit patterns; gen: scalars or which table)
  std::string graph_key() const {
    uint32_t ks_bits; memcpy(&ks_bits, &k_scale, 4);
    uint32_t vs_bits; memcpy(&vs_bits, &v_scale, 4);
    return format != KvFormat::Fp8 ? "" : ":kv8:" + std::to_string(ks_bits) + ":" + std::to_string(vs_bits) + ":" + std::to_string(gen);
  }

  // ---- format and scales (arguments already checked).  Whatever the cache holds was written in the previous format or with other
  // scales: a kept-cache caller starts over
  void set_format(bool fp8, float ks, float vs) {
    if (fp8) format = KvFormat::Fp8;
    else if (format == KvFormat::Fp8) format = KvFormat::Native;   // (a Planes24 engine is never FP8-eligible: it stays Planes24)
    k_scale = ks; v_scale = vs;
    table = false; ++gen;   // uniform scales: a table of ivg_set_kv_scales is dropped
    forget_kept();
  }
  int set_scales(const float* s, std::string& err) {
    // launches of an earlier call may still read the table: the device is idle before it is rewritten (this call synchronises)
    KV_HIP(hipDeviceSynchronize());
    KV_HIP(hipMemcpy(scales_dev, s, table_n() * 4, hipMemcpyHostToDevice));
    scales.assign(s, s + table_n());
    table = true; ++gen;
    forget_kept();
    return 0;
  }
  void get_scales(float* out) const { for (size_t i = 0; i < table_n(); ++i) out[i] = table ? scales[i] : ((i / heads) % 2 ? v_scale : k_scale); }

  // ---- calibration
  int reset_amax(std::string& err) {
    KV_HIP(hipDeviceSynchronize());   // (a calibration pass still running would race with the memset)
    KV_HIP(hipMemset(amax, 0, table_n() * 4));
    KV_HIP(hipDeviceSynchronize());
    calib_pending = false;
    return 0;
  }
  // the observations (once the last calibration pass has finished) and the scales they imply; *bad: index of an entry that saw Inf / NaN
  int calibrated_scales(int headroom_log2, std::vector<uint32_t>& bits, std::vector<float>& sc, long* bad, std::string& err) {
    if (calib_pending) { KV_HIP(hipStreamSynchronize(calib_stream)); calib_pending = false; }
    bits.resize(table_n()); sc.resize(table_n());
    KV_HIP(hipMemcpy(bits.data(), amax, table_n() * 4, hipMemcpyDeviceToHost));
    *bad = -1;
    for (size_t i = 0; i < table_n(); ++i) {
      float a; memcpy(&a, &bits[i], 4);
      if (bits[i] >= 0x7f800000u) { *bad = (long)i; return 0; }
      // the smallest power of two s with amax / s <= 448 (= 0.875 * 2^9), times 2^headroom; exact, in integers
      int ex = 0, p = 0;
      if (a > 0.f) { const float mant = frexpf(a, &ex); p = (mant <= 0.875f ? ex - 9 : ex - 8) + headroom_log2; }
      sc[i] = ldexpf(1.0f, std::min(126, std::max(-126, p)));
    }
    return 0;
  }
};

#undef KV_HIP

struct ProfSlot { hipEvent_t a, b; double flops, bytes; };
struct ProfClass { bool enabled = false; std::vector<ProfSlot> used; std::vector<ProfSlot> pool; };

}  // namespace ivg

struct ivg_cache {
  int B = 0;
  float* ctx_pixels = nullptr;             // [B][ctx][3][H][W] (sized for float32; holds pix_dt elements)
  int pix_dt = 0;                           // element type of the kept context pixels (the output type of the call that filled the cache)
  std::vector<void*> feat;                  // un-repeated per-trajectory context decoder features (NHWC)
  bool filled = false;
  bool clamped = false;                     // the kept context pixels were written with the output clamp on (ivg_set_output_clamp at fill time)
  int ctx = 0;                              // context length in force at fill time: rows of ctx_pixels / feat[] hold that many frames (ivg_cache_select)
};

// The conditional encoder's context, kept per trajectory: what Run::xatt_project_kv makes of the plain encoder's features at every
// cross-attention site (order of TrunkW::xatt).  Buffers are sized for the pretrained context length; rows are dense in the context
// length in force at fill time
struct ivg_enc_cache {
  const ivg_engine* owner = nullptr;
  int B = 0;
  std::vector<void*> Kp, VpT;               // per site: [B][kv][C] and [B][C][kv], kv = ctx * side * side, encode dtype
  bool filled = false;
  int ctx = 0;                              // context length in force at fill time
};

// A copy of the transformer's kept cache (ivg_kv_snapshot_create), owned by the caller: one device allocation holding the compact image
// of every buffer ivg_kv_select gathers, the kept host state, and what makes the bytes meaningful to an engine that restores them
struct ivg_kv_snapshot {
  struct Part { size_t off = 0; int slabs = 1, heads = 1; long bytes_a = 0, bytes_b = 0; int vec = 16; };   // [slabs][B][heads]{bytes_a | bytes_b} at off
  char* mem = nullptr;
  size_t bytes = 0;
  int device = 0;
  // the kept state (KvCache::keep's arguments)
  int len = 0, B = 0;
  bool ids_valid = false, snap_valid = false;
  int act_T = 0, ctx = 0;
  int id_cols = 0;                          // columns [0, id_cols) of the id rows: len + 1 where the rows are that long
  Part kv, ids, act, emb;                   // (act / emb: bytes_a == 0 when the kept cache has none)
  // what the bytes mean
  int layers = 0, heads = 0, hd = 0, hidden = 0, action_dim = 0;
  ivg::DType dt = ivg::F32;
  bool x3 = false;
  ivg::KvFormat format = ivg::KvFormat::Native;
  bool table = false;
  float k_scale = 1.0f, v_scale = 1.0f;
  std::vector<float> scales;
  const void* embed = nullptr; const void* lm_head = nullptr;   // the weights tag
};

struct ivg_engine {
  ivg_config cfg;
  int device = 0;
  std::string err;
  std::unordered_map<std::string, ivg_tensor> wmap;
  ivg::Arena ws;
  int ctx = 1;  // current context length (set_context_length)
  bool clamp_out = false;   // detokenize writes clamp(frames, 0, 1) (conv_out epilogue) instead of the raw decoder output (ivg_set_output_clamp)
  ivg::DType enc_dt, dec_dt, llm_dt;   // element types in HBM
  bool dec_x3 = false, llm_x3 = false;  // IVG_F32X3: fp32 tensors, split-bf16 matrix arithmetic on that path
  ivg::KvCache kvc;          // the transformer's K / V cache: format, layout, scales, and what the kept rows were built from
  // tokenizer
  ivg::TrunkW enc, cenc, dec, cdec;
  ivg::ConvW quant_conv, post_quant_conv, quant_linear, post_quant_linear;
  const float* cb_c = nullptr; const float* cb_d = nullptr;
  float* ee_c = nullptr; float* ee_d = nullptr;
  // transformer
  std::vector<ivg::LayerW> layers;
  const void* embed = nullptr; const void* lm_head = nullptr;  // final norm weight folded into lm_head
  float* ones = nullptr;     // [hidden] of 1.0f: the prefill's stand-alone RMSNorm has no weight left to apply
  const float* rope_cos = nullptr; const float* rope_sin = nullptr;
  const float* act_w = nullptr; const float* act_b = nullptr; const float* rew_w = nullptr; const float* rew_b = nullptr;
  int heads = 0, hd = 0, Lmax = 0;
  char* vt = nullptr;        // [Bmax][heads][hd][Lmax] transposed V scratch for the prefill
  char* gen_buf = nullptr;   // persistent decode-step buffers (fixed addresses -> graph replay)
  size_t gen_bytes = 0;
  std::unordered_map<std::string, hipGraphExec_t> graphs;
  bool use_graph = false;     // IVG_GRAPH=1 at ivg_create (switches.h)
  unsigned graphs_gen = 0;    // switches_generation() the captured graphs belong to (a changed table drops them all)
  int decode_lds_kb = 0;      // LDS budget of this engine's decode GEMMs (ivg_config.decode_lds_kb / ivg_set_decode_lds_kb; 0: process default)
  // the budget in force (this engine's, else the process default IVG_DECODE_LDS_KB) and what it implies: below a whole CU's 160 KiB the
  // engine runs the BATCHES-IN-FLIGHT profile (shared-weight cache policy, no warm-up of the next launch) -- the same whichever of
  // the two routes set the budget, and an explicit 160 is the one-batch profile like 0 (advice, round 5)
  int effective_lds_kb() const;
  bool in_flight() const { return effective_lds_kb() < 160; }
  float temperature = 1.0f;   // sampling temperature of the rollout (ivg_set_temperature; HF TemperatureLogitsWarper semantics)
  float top_p = 1.0f;         // nucleus filter of the rollout (ivg_set_top_p; HF TopPLogitsWarper up to the documented boundaries)
  ivg::ProfClass prof[IVG_K_COUNT];
  unsigned long long* attn_prof = nullptr;  // [layers][IVG_ATTN_PROF_SLOTS][2][Lmax] wall-clock stamps of the decode attention
  bool attn_prof_on = false;                // ivg_profile_enable(IVG_K_DECODE_ATTN): part of the step-graph key
  unsigned long long* gemm_prof = nullptr;  // [layers * 4 + 1][IVG_GEMM_PROF_SLOTS][2][Lmax] stamps of the decode-step GEMMs (allocated on first use)
  bool gemm_prof_on = false;                // ivg_profile_enable(IVG_K_DECODE_GEMM): part of the step-graph key
  int gemm_prof_B = 0;
  double gemm_kind_ms[5] = {0, 0, 0, 0, 0};   // last ivg_profile_read(IVG_K_DECODE_GEMM) by kind: q/k/v, o-proj, gate/up, down, lm_head
  long long gemm_kind_n[5] = {0, 0, 0, 0, 0};
  const float* final_norm = nullptr;        // model.norm.weight (fp32), for the hidden state handed to the caller
  const float* rew_w_raw = nullptr;         // reward_linear.weight as stored (applies to the post-norm hidden state)
  const float* ar_w = nullptr; const float* ar_b = nullptr;   // action_recon_linear (optional, eval loss term only)
  char* emb_snap = nullptr;                 // [Bc][Lmax][H] llm dtype, allocated on the first embeds call: the inputs of the kept cache rows (kvc.snap_valid)
  int* h_flag = nullptr;                    // pinned host word for the verification result
  int attn_prof_B = 0;
  double attn_fit_fixed_us = 0, attn_fit_gbps = 0;   // line fit of the last ivg_profile_read(IVG_K_DECODE_ATTN)

  int fail(int code, const std::string& msg) { err = msg; return code; }
};
