// C ABI of libivg (include/ivg.h): engine construction from a named weight table, workspace planning,
// the tokenize / generate / detokenize entry points and the op-level hooks used by the parity tests.
#include <cstdlib>
#include <cstring>

#include <cstdio>
#include "engine_impl.h"
#include "switches.h"

using namespace ivg;

static thread_local std::string g_create_err;

namespace ivg {

void set_create_error(const std::string& s) { g_create_err = s; }

size_t dtype_size(DType d) { return d == BF16 ? 2 : 4; }

struct Lookup {
  ivg_engine* e;
  bool ok = true;
  const ivg_tensor* find(const std::string& name, int dtype, int64_t numel) {
    auto it = e->wmap.find(name);
    if (it == e->wmap.end()) { if (ok) e->err = "missing weight tensor '" + name + "'"; ok = false; return nullptr; }
    const ivg_tensor& t = it->second;
    int64_t n = 1;
    for (int i = 0; i < t.ndim; ++i) n *= t.shape[i];
    if (t.dtype != dtype || n != numel) {
      if (ok) e->err = "weight tensor '" + name + "' has dtype " + std::to_string(t.dtype) + " / " + std::to_string(n) +
                       " elements, expected dtype " + std::to_string(dtype) + " / " + std::to_string(numel);
      ok = false;
      return nullptr;
    }
    return &t;
  }
  const void* data(const std::string& name, int dtype, int64_t numel) {
    const ivg_tensor* t = find(name, dtype, numel);
    return t ? t->data : nullptr;
  }
  const float* f32(const std::string& name, int64_t numel) { return (const float*)data(name, IVG_F32, numel); }
  ConvW conv(const std::string& n, int cin, int cout, int k, DType dt) {
    ConvW c; c.cin = cin; c.cout = cout; c.k = k;
    c.w = data(n + ".weight", (int)dt, (int64_t)cout * k * k * cin);
    c.b = f32(n + ".bias", cout);
    // optional: the same matrix pre-split into bf16 (hi, lo) pairs for the split-bf16 3x3 kernel (packing.py: pack_x3)
    if (dt == F32 && k == 3 && e->wmap.count(n + ".weight.x3")) c.w3 = data(n + ".weight.x3", IVG_BF16, (int64_t)2 * cout * k * k * cin);
    // optional (upsampler convs): the sub-pixel phase weights [4][cout][4 * cin] (packing.py: pack_subpixel), and their x3 split
    if (k == 3 && e->wmap.count(n + ".weight.subpix")) c.wsub = data(n + ".weight.subpix", (int)dt, (int64_t)16 * cout * cin);
    if (dt == F32 && k == 3 && e->wmap.count(n + ".weight.subpix.x3")) c.wsub3 = data(n + ".weight.subpix.x3", IVG_BF16, (int64_t)32 * cout * cin);
    return c;
  }
  NormW norm(const std::string& n, int C) { NormW r; r.g = f32(n + ".weight", C); r.b = f32(n + ".bias", C); return r; }
  ResnetW resnet(const std::string& n, int cin, int cout, DType dt) {
    ResnetW r; r.cin = cin; r.cout = cout;
    r.n1 = norm(n + ".norm1", cin); r.c1 = conv(n + ".conv1", cin, cout, 3, dt);
    r.n2 = norm(n + ".norm2", cout); r.c2 = conv(n + ".conv2", cout, cout, 3, dt);
    r.has_sc = cin != cout;
    if (r.has_sc) r.sc = conv(n + ".conv_shortcut", cin, cout, 1, dt);
    return r;
  }
  AttnW attn(const std::string& n, int C, DType dt) {
    AttnW a; a.gn = norm(n + ".group_norm", C);
    a.q = conv(n + ".to_q", C, C, 1, dt); a.k = conv(n + ".to_k", C, C, 1, dt);
    a.v = conv(n + ".to_v", C, C, 1, dt); a.o = conv(n + ".to_out.0", C, C, 1, dt);
    return a;
  }
  XAttW xatt(const std::string& n, int C, int side, int ctx0, DType dt) {
    XAttW x; x.C = C; x.side = side; x.kv_rows = ctx0 * side * side;
    x.kvn = norm(n + ".kv_norm", C); x.qn = norm(n + ".q_norm", C);
    x.kv_pos = f32(n + ".kv_pos_emb", (int64_t)x.kv_rows * C);
    x.q_pos = f32(n + ".q_pos_emb", (int64_t)side * side * C);
    const char* w = (const char*)data(n + ".att.in_proj_weight", (int)dt, (int64_t)3 * C * C);
    const float* b = f32(n + ".att.in_proj_bias", 3 * C);
    auto part = [&](int i) { ConvW c; c.cin = C; c.cout = C; c.k = 1; c.w = w ? w + (size_t)i * C * C * dtype_size(dt) : nullptr; c.b = b ? b + i * C : nullptr; return c; };
    x.q = part(0); x.k = part(1); x.v = part(2);
    x.o = conv(n + ".att.out_proj", C, C, 1, dt);
    return x;
  }
};

int build_tokenizer(ivg_engine* e) {
  const ivg_config& c = e->cfg;
  const int nl = c.n_levels, lpb = c.layers_per_block, lat = c.latent_channels, dim = c.vq_embed_dim, p = c.patch_size;
  const int* ch = c.block_out_channels;
  Lookup L{e};
  auto encoder = [&](const std::string& n, bool attn, bool cond, TrunkW& t) {
    const DType dt = e->enc_dt;
    t.conv_in_raw_w = L.f32(n + ".conv_in.weight", (int64_t)ch[0] * 27);
    t.conv_in.b = L.f32(n + ".conv_in.bias", ch[0]);
    int prev = ch[0], res = c.resolution;
    for (int i = 0; i < nl; ++i) {
      std::vector<ResnetW> blk;
      for (int j = 0; j < lpb; ++j) blk.push_back(L.resnet(n + ".down_blocks." + std::to_string(i) + ".resnets." + std::to_string(j), j == 0 ? prev : ch[i], ch[i], dt));
      t.blocks.push_back(blk);
      ConvW ds;
      if (i != nl - 1) { ds = L.conv(n + ".down_blocks." + std::to_string(i) + ".downsamplers.0.conv", ch[i], ch[i], 3, dt); res /= 2; }
      t.resample.push_back(ds);
      if (cond && res <= c.max_att_resolution)
        t.xatt.push_back(L.xatt(n + ".cross_att_blocks." + std::to_string(t.xatt.size()), ch[i], res, c.context_length, dt));
      prev = ch[i];
    }
    t.mid0 = L.resnet(n + ".mid_block.resnets.0", ch[nl - 1], ch[nl - 1], dt);
    t.mid1 = L.resnet(n + ".mid_block.resnets.1", ch[nl - 1], ch[nl - 1], dt);
    t.has_attn = attn;
    if (attn) t.attn = L.attn(n + ".mid_block.attentions.0", ch[nl - 1], dt);
    t.norm_out = L.norm(n + ".conv_norm_out", ch[nl - 1]);
    t.conv_out = L.conv(n + ".conv_out", ch[nl - 1], lat, 3, dt);
  };
  auto decoder = [&](const std::string& n, bool attn, bool cond, TrunkW& t) {
    const DType dt = e->dec_dt;
    const int top = ch[nl - 1];
    t.conv_in = L.conv(n + ".conv_in", lat, top, 3, dt);
    t.mid0 = L.resnet(n + ".mid_block.resnets.0", top, top, dt);
    t.mid1 = L.resnet(n + ".mid_block.resnets.1", top, top, dt);
    t.has_attn = attn;
    if (attn) t.attn = L.attn(n + ".mid_block.attentions.0", top, dt);
    int prev = top, res = 16;
    if (cond) t.xatt.push_back(L.xatt(n + ".cross_att_blocks.0", top, 16, c.context_length, dt));
    for (int i = 0; i < nl; ++i) {
      const int co = ch[nl - 1 - i];
      std::vector<ResnetW> blk;
      for (int j = 0; j < lpb + 1; ++j) blk.push_back(L.resnet(n + ".up_blocks." + std::to_string(i) + ".resnets." + std::to_string(j), j == 0 ? prev : co, co, dt));
      t.blocks.push_back(blk);
      ConvW us;
      if (i != nl - 1) { us = L.conv(n + ".up_blocks." + std::to_string(i) + ".upsamplers.0.conv", co, co, 3, dt); res *= 2; }
      t.resample.push_back(us);
      if (cond && res <= c.max_att_resolution)
        t.xatt.push_back(L.xatt(n + ".cross_att_blocks." + std::to_string(t.xatt.size()), co, res, c.context_length, dt));
      prev = co;
    }
    t.norm_out = L.norm(n + ".conv_norm_out", ch[0]);
    t.conv_out = L.conv(n + ".conv_out", ch[0], 3, 3, dt);
  };
  encoder("encoder", c.mid_block_add_attention != 0, false, e->enc);
  encoder("cond_encoder", true, true, e->cenc);
  decoder("decoder", c.mid_block_add_attention != 0, false, e->dec);
  decoder("cond_decoder", true, true, e->cdec);
  e->quant_conv = L.conv("quant_conv", lat, dim, 1, e->enc_dt);
  e->quant_linear = L.conv("quant_linear", lat, dim, p, e->enc_dt);  // [dim][p*p*lat] with (ph, pw, c) feature order
  e->post_quant_conv = L.conv("post_quant_conv", dim, lat, 1, e->dec_dt);
  e->post_quant_linear = L.conv("post_quant_linear", dim, lat * p * p, 1, e->dec_dt);
  e->cb_c = L.f32("quantize.embedding.weight", (int64_t)c.num_vq_embeddings * dim);
  e->cb_d = L.f32("dynamics_quantize.embedding.weight", (int64_t)c.num_dyn_embeddings * dim);
  return L.ok ? 0 : IVG_ERR_MISSING;
}

int build_transformer(ivg_engine* e) {
  const ivg_config& c = e->cfg;
  const DType dt = e->llm_dt;
  const int H = c.hidden_size, I = c.intermediate_size, V = c.vocab_size;
  Lookup L{e};
  e->heads = c.num_heads; e->hd = H / c.num_heads;
  e->Lmax = c.max_seq > 0 ? c.max_seq : c.max_position_embeddings;
  e->layers.clear();
  for (int l = 0; l < c.num_layers; ++l) {
    const std::string b = "llm.layers." + std::to_string(l) + ".";
    LayerW w;
    w.wqkv = L.data(b + "wqkv", (int)dt, (int64_t)3 * H * H);
    w.wo = L.data(b + "wo", (int)dt, (int64_t)H * H);
    w.wgu = L.data(b + "wgu", (int)dt, (int64_t)2 * I * H);
    w.wdown = L.data(b + "wdown", (int)dt, (int64_t)H * I);
    e->layers.push_back(w);
  }
  e->embed = L.data("llm.embed", (int)dt, (int64_t)V * H);
  e->lm_head = L.data("llm.lm_head", (int)dt, (int64_t)V * H);
  e->rope_cos = L.f32("llm.rope_cos", (int64_t)c.max_position_embeddings * (e->hd / 2));
  e->rope_sin = L.f32("llm.rope_sin", (int64_t)c.max_position_embeddings * (e->hd / 2));
  if (c.action_dim > 0) {
    e->act_w = L.f32("llm.action_linear.weight", (int64_t)H * c.action_dim);
    e->act_b = L.f32("llm.action_linear.bias", H);
  }
  if (c.reward_head) {
    e->rew_w = L.f32("llm.reward_linear.weight", H);
    e->rew_b = L.f32("llm.reward_linear.bias", 1);
    if (e->wmap.count("llm.reward_linear.raw")) e->rew_w_raw = L.f32("llm.reward_linear.raw", H);
  }
  if (e->wmap.count("llm.norm")) e->final_norm = L.f32("llm.norm", H);   // optional: only the hidden-state outputs need it
  if (c.action_dim > 0 && e->wmap.count("llm.action_recon_linear.weight")) {
    e->ar_w = L.f32("llm.action_recon_linear.weight", (int64_t)c.action_dim * H);
    e->ar_b = L.f32("llm.action_recon_linear.bias", c.action_dim);
  }
  return L.ok ? 0 : IVG_ERR_MISSING;
}

// ---- measurement hooks
void Run::prof_begin(DType dt, double flops, double bytes, int base) {
  ProfClass& pc = e->prof[base + (dt == BF16 ? 0 : 1)];
  if (!pc.enabled) return;
  ProfSlot s;
  if (!pc.pool.empty()) { s = pc.pool.back(); pc.pool.pop_back(); }
  else { if (hipEventCreate(&s.a) != hipSuccess || hipEventCreate(&s.b) != hipSuccess) return; }
  s.flops = flops; s.bytes = bytes;
  (void)hipEventRecord(s.a, st);
  pc.used.push_back(s);
}
void Run::prof_end(DType dt, int base) {
  ProfClass& pc = e->prof[base + (dt == BF16 ? 0 : 1)];
  if (!pc.enabled || pc.used.empty()) return;
  (void)hipEventRecord(pc.used.back().b, st);
}
void Run::prof_cancel(DType dt, int base) {
  ProfClass& pc = e->prof[base + (dt == BF16 ? 0 : 1)];
  if (!pc.enabled || pc.used.empty()) return;
  pc.pool.push_back(pc.used.back());
  pc.used.pop_back();
}

}  // namespace ivg

#define API_CK(x) do { hipError_t _e = (x); if (_e != hipSuccess) { e->err = std::string(#x) + ": " + hipGetErrorString(_e); return IVG_ERR_HIP; } } while (0)

// Every entry point first walks its own allocation plan (host arithmetic only) and grows the arena if this call
// needs more than any earlier one; then runs for real.  f(Run&) must be the same call in both passes.
template <typename F>
static int plan_then_run(ivg_engine* e, hipStream_t st, F&& f, bool may_grow = true) {
  e->ws.planning = true; e->ws.off = 0; e->ws.high = 0; e->ws.overflow = false;
  Run p{e, nullptr, true};
  int rc = f(p);
  const size_t need = e->ws.high + (1 << 20);
  e->ws.planning = false; e->ws.off = 0;
  if (rc) return rc;
  // (an entry that promises not to synchronise the host stays inside what ivg_create planned, or says so)
  if (need > e->ws.cap && !may_grow) return e->fail(IVG_ERR_CAPACITY, "internal: the call needs more workspace than the engine was created with");
  if (need > e->ws.cap) {
    API_CK(hipDeviceSynchronize());
    if (e->ws.base) API_CK(hipFree(e->ws.base));
    e->ws.base = nullptr; e->ws.cap = 0;
    API_CK(hipMalloc((void**)&e->ws.base, need));
    e->ws.cap = need;
  }
  Run r{e, st, false};
  rc = f(r);
  if (rc == 0 && e->ws.overflow) return e->fail(IVG_ERR_CAPACITY, "internal: workspace plan was smaller than the run");
  return rc;
}

static int plan_and_allocate(ivg_engine* e) {
  const ivg_config& c = e->cfg;
  e->ws.planning = true; e->ws.off = 0; e->ws.high = 0;
  Run r{e, nullptr, true};
  const int B = c.max_batch, T = c.max_frames;
  if (c.n_levels > 0) {
    const int saved = e->ctx;
    for (int ctx = 1; ctx <= c.context_length; ++ctx) {  // any context length set_context_length may select later
      e->ctx = ctx;
      if (T > ctx) {
        int rc = r.tokenize(nullptr, F32, B, T, nullptr, 257 * ctx - 1 + 17 * (T - ctx), nullptr, false); if (rc) return rc;
        rc = r.detokenize(nullptr, B, T - ctx, nullptr, F32, nullptr, 0); if (rc) return rc;
      }
    }
    e->ctx = saved;
  }
  if (c.num_layers > 0) {
    const int Lpre = std::min(e->Lmax - 1, 514);  // typical prompt (2 context frames); larger calls grow the arena on demand
    GenerateReq q; q.B = B; q.L0 = Lpre; q.n_new = 1;
    int rc = r.generate(q); if (rc) return rc;
    e->ws.reset(0);
    (void)e->ws.alloc(kv_select_scratch_bytes(e));   // ivg_kv_select stages rows here and never grows the arena (no host synchronisation)
  }
  e->ws.cap = e->ws.high + (1 << 20);
  API_CK(hipMalloc((void**)&e->ws.base, e->ws.cap));
  e->ws.planning = false; e->ws.off = 0;
  return 0;
}

// the fields every GEMM / convolution hook takes over from the caller's struct as they are
static void igemm_op_args(IgemmArgs& g, const ivg_igemm_args* a) {
  g.X = a->X; g.W = a->W; g.Y = a->Y; g.R = a->R; g.bias = a->bias;
  g.Nimg = a->Nimg; g.Hin = a->Hin; g.Win = a->Win; g.Cin = a->Cin; g.ldx = a->ldx; g.Hout = a->Hout; g.Wout = a->Wout;
  g.KH = a->KH; g.KW = a->KW; g.stride = a->stride; g.pad = a->pad; g.ups = a->ups; g.N = a->N; g.ldw = a->ldw;
  g.c_img = a->c_img; g.c_pix = a->c_pix; g.c_ch = a->c_ch; g.c_grp = a->c_grp; g.c_grp_stride = a->c_grp_stride;
  g.flags = a->flags; g.alpha = a->alpha;
}

// Unit-test hooks of one decode step: a device StepState at position pos (step j = 1) for the launch f(state, st) makes; waits for it
template <typename F>
static int one_step(int pos, ivg_stream stream, F&& f) {
  StepState* state = nullptr;
  if (hipMalloc((void**)&state, sizeof(StepState)) != hipSuccess) return IVG_ERR_HIP;
  hipStream_t st = (hipStream_t)stream;
  int rc = launch_state_set(state, pos, 1, st);
  if (!rc) rc = f(state, st);
  (void)hipStreamSynchronize(st);
  (void)hipFree(state);
  return rc == 0 ? IVG_OK : (rc > 0 ? IVG_ERR_HIP : IVG_ERR_INVALID);
}

extern "C" {

const char* ivg_version(void) { return "libivg 0.1 (gfx950)"; }

const char* ivg_last_error(const ivg_engine* e) { return e ? e->err.c_str() : g_create_err.c_str(); }

void ivg_destroy(ivg_engine* e) {
  if (!e) return;
  (void)hipSetDevice(e->device);
  (void)hipDeviceSynchronize();
  for (auto& kv : e->graphs) (void)hipGraphExecDestroy(kv.second);
  for (int k = 0; k < IVG_K_COUNT; ++k) {
    for (auto& s : e->prof[k].used) { (void)hipEventDestroy(s.a); (void)hipEventDestroy(s.b); }
    for (auto& s : e->prof[k].pool) { (void)hipEventDestroy(s.a); (void)hipEventDestroy(s.b); }
  }
  if (e->ws.base) (void)hipFree(e->ws.base);
  if (e->ee_c) (void)hipFree(e->ee_c);
  if (e->ee_d) (void)hipFree(e->ee_d);
  e->kvc.destroy();
  if (e->vt) (void)hipFree(e->vt);
  if (e->gen_buf) (void)hipFree(e->gen_buf);
  if (e->ones) (void)hipFree(e->ones);
  if (e->attn_prof) (void)hipFree(e->attn_prof);
  if (e->emb_snap) (void)hipFree(e->emb_snap);
  if (e->gemm_prof) (void)hipFree(e->gemm_prof);
  if (e->h_flag) (void)hipHostFree(e->h_flag);
  delete e;
}

int ivg_create(const ivg_config* cfg, const ivg_tensor* weights, int n_weights, int device, ivg_engine** out) {
  if (!cfg || !out) { g_create_err = "ivg_create: null argument"; return IVG_ERR_INVALID; }
  ivg_engine* e = new ivg_engine();
  e->cfg = *cfg; e->device = device;
  auto bail = [&](int code) { g_create_err = e->err; ivg_destroy(e); return code; };
  if (hipSetDevice(device) != hipSuccess) { e->err = "hipSetDevice failed (no MI355X visible?)"; return bail(IVG_ERR_HIP); }
  reload_switches();   // the one place the environment is read (switches.h)
  // Decode steps are launched eagerly by default: on ROCm 7.2 a replayed hipGraph leaves ~1 us MORE between two dependent kernel
  // nodes than the same kernels launched one by one on the stream (config-2 rollout: 166 ms replayed, 149 ms eager; the host
  // issues a launch in ~4 us against ~10 us of device time per kernel, so it stays ahead).  IVG_GRAPH=1 captures the step into
  // a hipGraph (8 steps per launch) for callers that need the host thread back early.
  e->use_graph = sw().graph != 0;
  if (cfg->decode_lds_kb != 0 && (cfg->decode_lds_kb < 16 || cfg->decode_lds_kb > 160)) { e->err = "ivg_create: decode_lds_kb must be 0 (process default) or 16 .. 160"; return bail(IVG_ERR_INVALID); }
  e->decode_lds_kb = cfg->decode_lds_kb;
  if (cfg->encode_dtype == IVG_F32X3) { e->err = "ivg_create: encode_dtype cannot be IVG_F32X3 (bit-exact VQ indices need the exact fp32 chain)"; return bail(IVG_ERR_INVALID); }
  // IVG_F32X3: fp32 tensors, split-bf16 matrix arithmetic (conv3x3.hip / igemm.hip X3 instances)
  e->dec_x3 = cfg->decode_dtype == IVG_F32X3; e->llm_x3 = cfg->llm_dtype == IVG_F32X3;
  e->enc_dt = (DType)cfg->encode_dtype; e->dec_dt = e->dec_x3 ? F32 : (DType)cfg->decode_dtype; e->llm_dt = e->llm_x3 ? F32 : (DType)cfg->llm_dtype;
  e->ctx = cfg->context_length > 0 ? cfg->context_length : 1;
  for (int i = 0; i < n_weights; ++i) e->wmap[weights[i].name] = weights[i];
  if (cfg->max_batch <= 0 || cfg->max_frames <= 0) { e->err = "ivg_create: max_batch / max_frames must be positive"; return bail(IVG_ERR_INVALID); }
  if (cfg->num_layers > 0) {   // transformer shape checks, before anything is built or launched
    if (cfg->num_heads <= 0 || cfg->hidden_size <= 0 || cfg->hidden_size % cfg->num_heads != 0) {
      e->err = "ivg_create: hidden_size must be a positive multiple of num_heads"; return bail(IVG_ERR_INVALID);
    }
    const int hd = cfg->hidden_size / cfg->num_heads;
    if (!decode_attn_covers(hd, e->llm_dt)) {
      e->err = "ivg_create: head_dim " + std::to_string(hd) + " is not supported by the decode-attention kernel (" +
               (e->llm_dt == BF16 ? "bf16: 8, 16, 32, 64, 128 or 256)" : "fp32: 4, 8, 16, 32, 64, 128 or 256)");
      return bail(IVG_ERR_INVALID);
    }
    if (cfg->max_seq > cfg->max_position_embeddings) {   // the RoPE tables hold max_position_embeddings rows
      e->err = "ivg_create: max_seq " + std::to_string(cfg->max_seq) + " exceeds max_position_embeddings " +
               std::to_string(cfg->max_position_embeddings);
      return bail(IVG_ERR_INVALID);
    }
  }
  if (cfg->n_levels > 0) {
    const ivg_config& c = *cfg;
    if (c.n_levels > 8 || c.vq_embed_dim != 64 || c.patch_size != 4 || (c.resolution >> (c.n_levels - 1)) != 16 || c.latent_channels % 32 != 0) {
      e->err = "ivg_create: unsupported tokenizer geometry (needs vq_embed_dim 64, patch 4, 16x16 latent grid)"; return bail(IVG_ERR_INVALID);
    }
    int rc = build_tokenizer(e); if (rc) return bail(rc);
    if (hipMalloc((void**)&e->ee_c, (size_t)c.num_vq_embeddings * 4) != hipSuccess || hipMalloc((void**)&e->ee_d, (size_t)c.num_dyn_embeddings * 4) != hipSuccess) {
      e->err = "hipMalloc failed"; return bail(IVG_ERR_HIP);
    }
    if (launch_sqnorm_rows(e->cb_c, e->ee_c, c.num_vq_embeddings, c.vq_embed_dim, nullptr) || launch_sqnorm_rows(e->cb_d, e->ee_d, c.num_dyn_embeddings, c.vq_embed_dim, nullptr)) {
      e->err = "codebook norm kernel failed to launch (is this a gfx950 device?)"; return bail(IVG_ERR_HIP);
    }
  }
  if (cfg->num_layers > 0) {
    int rc = build_transformer(e); if (rc) return bail(rc);
    const bool planes24 = e->llm_x3 && e->hd == 64 && sw().x3 && sw().kv24;   // (IVG_X3=0: an x3 engine IS the fp32 engine)
    if (!e->kvc.create(cfg->num_layers, e->heads, e->hd, e->Lmax, cfg->max_batch, e->llm_dt, e->llm_x3, planes24)) { e->err = "hipMalloc of the KV cache failed"; return bail(IVG_ERR_HIP); }
    const size_t vtb = (size_t)e->kvc.chunk * e->heads * e->hd * ((e->Lmax + 63) / 64 * 64) * dtype_size(e->llm_dt);
    e->gen_bytes = gen_buffer_bytes(e);
    if (hipMalloc((void**)&e->vt, vtb) != hipSuccess || hipMalloc((void**)&e->gen_buf, e->gen_bytes) != hipSuccess) {
      e->err = "hipMalloc of the KV cache failed"; return bail(IVG_ERR_HIP);
    }
    {
      std::vector<float> one((size_t)cfg->hidden_size, 1.0f);
      if (hipMalloc((void**)&e->ones, one.size() * 4) != hipSuccess || hipMemcpy(e->ones, one.data(), one.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
        e->err = "hipMalloc failed"; return bail(IVG_ERR_HIP);
      }
    }
    if (hipMalloc((void**)&e->attn_prof, (size_t)cfg->num_layers * IVG_ATTN_PROF_SLOTS * 2 * e->Lmax * 8) != hipSuccess) { e->err = "hipMalloc failed"; return bail(IVG_ERR_HIP); }
    (void)hipMemset(e->attn_prof, 0, (size_t)cfg->num_layers * IVG_ATTN_PROF_SLOTS * 2 * e->Lmax * 8);
    (void)hipMemset(e->vt, 0, vtb);
    (void)hipMemset(e->gen_buf, 0, e->gen_bytes);
  }
  int rc = plan_and_allocate(e);
  if (rc) return bail(rc);
  if (hipDeviceSynchronize() != hipSuccess) { e->err = "device error during engine construction"; return bail(IVG_ERR_HIP); }
  *out = e;
  return IVG_OK;
}

int ivg_set_context_length(ivg_engine* e, int k) {
  if (!e) return IVG_ERR_INVALID;
  if (k < 1 || k > e->cfg.context_length) return e->fail(IVG_ERR_INVALID, "set_context_length: k must be in [1, pretrained context_length]");
  e->ctx = k;
  return IVG_OK;
}

static int check_tok(ivg_engine* e, int B, int T, const char* who) {
  if (e->cfg.n_levels <= 0) return e->fail(IVG_ERR_INVALID, std::string(who) + ": engine was created without a tokenizer");
  if (B <= 0 || B > e->cfg.max_batch || T > e->cfg.max_frames)
    return e->fail(IVG_ERR_CAPACITY, std::string(who) + ": batch " + std::to_string(B) + " x " + std::to_string(T) + " frames exceeds the capacity the engine was created with (" +
                   std::to_string(e->cfg.max_batch) + " x " + std::to_string(e->cfg.max_frames) + ")");
  return 0;
}

int ivg_tokenize(ivg_engine* e, const void* pixels, int pixel_dtype, int B, int T, int64_t* ids_out, int64_t* labels_out, ivg_stream stream) {
  if (!e) return IVG_ERR_INVALID;
  IVG_TRY(check_tok(e, B, T, "tokenize"));
  if (T < e->ctx + 1) return e->fail(IVG_ERR_INVALID, "tokenize: needs at least one future frame (T >= context_length + 1)");
  return plan_then_run(e, (hipStream_t)stream, [&](Run& r) {
    return r.tokenize(pixels, (DType)pixel_dtype, B, T, ids_out, 257L * e->ctx - 1 + 17L * (T - e->ctx), labels_out, false); });
}

int ivg_encode_context(ivg_engine* e, const void* pixels, int pixel_dtype, int B, int T, int64_t* ids_out, int64_t ids_stride, ivg_stream stream) {
  if (!e) return IVG_ERR_INVALID;
  IVG_TRY(check_tok(e, B, std::min(T, e->cfg.max_frames), "encode_context"));
  if (T < e->ctx || ids_stride < 257L * e->ctx) return e->fail(IVG_ERR_INVALID, "encode_context: T < context_length or ids_stride < 257*ctx");
  return plan_then_run(e, (hipStream_t)stream, [&](Run& r) {
    return r.tokenize(pixels, (DType)pixel_dtype, B, T, ids_out, ids_stride, nullptr, true); });
}

// ---- the encoder's context cache: the conditional encoder's cross-attention K / V projections of a context, kept per trajectory
int ivg_enc_cache_create(ivg_engine* e, int B, ivg_enc_cache** out) {
  if (!e || !out || e->cfg.n_levels <= 0) return IVG_ERR_INVALID;
  const ivg_config& c = e->cfg;
  if (B <= 0 || B > c.max_batch) return e->fail(IVG_ERR_CAPACITY, "enc_cache_create: batch " + std::to_string(B) + " exceeds the engine's max_batch");
  ivg_enc_cache* k = new ivg_enc_cache();
  k->owner = e; k->B = B;
  bool ok = true;
  for (const XAttW& x : e->cenc.xatt) {   // sized for the pretrained context length: any ivg_set_context_length fits
    const size_t bytes = (size_t)B * x.kv_rows * x.C * dtype_size(e->enc_dt);
    void* kp = nullptr; void* vp = nullptr;
    if (ok && hipMalloc(&kp, bytes) == hipSuccess) k->Kp.push_back(kp); else ok = false;
    if (ok && hipMalloc(&vp, bytes) == hipSuccess) k->VpT.push_back(vp); else ok = false;
  }
  if (!ok) {
    (void)hipGetLastError();
    for (void* p : k->Kp) (void)hipFree(p);
    for (void* p : k->VpT) (void)hipFree(p);
    delete k;
    return e->fail(IVG_ERR_HIP, "enc_cache_create: hipMalloc failed");
  }
  *out = k;
  return IVG_OK;
}

void ivg_enc_cache_destroy(ivg_engine* e, ivg_enc_cache* c) {
  if (!c) return;
  if (e) (void)hipSetDevice(e->device);
  (void)hipDeviceSynchronize();
  for (void* p : c->Kp) (void)hipFree(p);
  for (void* p : c->VpT) (void)hipFree(p);
  delete c;
}

int ivg_encode_context_cached(ivg_engine* e, const void* pixels, int pixel_dtype, int B, int T, int64_t* ids_out, int64_t ids_stride,
                              ivg_enc_cache* cache, ivg_stream stream) {
  if (!e) return IVG_ERR_INVALID;
  IVG_TRY(check_tok(e, B, std::min(T, e->cfg.max_frames), "encode_context_cached"));
  if (T < e->ctx || ids_stride < 257L * e->ctx) return e->fail(IVG_ERR_INVALID, "encode_context_cached: T < context_length or ids_stride < 257*ctx");
  if (pixel_dtype != IVG_F32 && pixel_dtype != IVG_BF16) return e->fail(IVG_ERR_INVALID, "encode_context_cached: pixels are float32 or bfloat16");
  if (!cache || cache->owner != e) return e->fail(IVG_ERR_INVALID, "encode_context_cached: null cache, or a cache of another engine");
  if (cache->B != B)
    return e->fail(IVG_ERR_INVALID, "encode_context_cached: cache was created for " + std::to_string(cache->B) + " trajectories, this call has " + std::to_string(B));
  return plan_then_run(e, (hipStream_t)stream, [&](Run& r) {
    return r.tokenize(pixels, (DType)pixel_dtype, B, T, ids_out, ids_stride, nullptr, true, cache); });
}

int ivg_tokenize_frames(ivg_engine* e, const void* frames, int pixel_dtype, int B, int n, const ivg_enc_cache* cache, int64_t* ids_out,
                        int64_t ids_stride, ivg_stream stream) {
  if (!e) return IVG_ERR_INVALID;
  if (e->cfg.n_levels <= 0) return e->fail(IVG_ERR_INVALID, "tokenize_frames: engine was created without a tokenizer");
  if (!cache || cache->owner != e) return e->fail(IVG_ERR_INVALID, "tokenize_frames: null cache, or a cache of another engine");
  if (!cache->filled) return e->fail(IVG_ERR_INVALID, "tokenize_frames: the cache is empty (ivg_encode_context_cached fills it)");
  if (B <= 0 || B > e->cfg.max_batch)
    return e->fail(IVG_ERR_CAPACITY, "tokenize_frames: batch " + std::to_string(B) + " exceeds the engine's max_batch (" + std::to_string(e->cfg.max_batch) + ")");
  if (cache->B != B)
    return e->fail(IVG_ERR_INVALID, "tokenize_frames: cache holds " + std::to_string(cache->B) + " trajectories, this call has " + std::to_string(B));
  if (cache->ctx != e->ctx)
    return e->fail(IVG_ERR_INVALID, "tokenize_frames: cache was filled under context length " + std::to_string(cache->ctx) + ", " + std::to_string(e->ctx) +
                                        " is in force (fill it again)");
  if (n < 1) return e->fail(IVG_ERR_INVALID, "tokenize_frames: n must be at least 1");
  if (pixel_dtype != IVG_F32 && pixel_dtype != IVG_BF16) return e->fail(IVG_ERR_INVALID, "tokenize_frames: frames are float32 or bfloat16");
  if (!frames || !ids_out || ids_stride < 17L * n) return e->fail(IVG_ERR_INVALID, "tokenize_frames: null argument, or ids_stride < 17*n");
  if (n > e->cfg.max_frames - e->ctx)
    return e->fail(IVG_ERR_CAPACITY, "tokenize_frames: " + std::to_string(n) + " frames exceed max_frames - context_length (" +
                                         std::to_string(e->cfg.max_frames - e->ctx) + "): the workspace is never grown by this call");
  return plan_then_run(e, (hipStream_t)stream, [&](Run& r) {
    return r.tokenize_frames(frames, (DType)pixel_dtype, B, n, cache, ids_out, ids_stride); }, false);
}

int ivg_enc_cache_select(ivg_engine* e, const ivg_enc_cache* src, const int32_t* parents, int n, ivg_enc_cache** out, ivg_stream stream) {
  if (!e || !out || e->cfg.n_levels <= 0) return IVG_ERR_INVALID;
  if (!src || src->owner != e || !src->filled || src->ctx <= 0) return e->fail(IVG_ERR_INVALID, "enc_cache_select: the source cache is empty (or of another engine)");
  if (!parents) return e->fail(IVG_ERR_INVALID, "enc_cache_select: null argument");
  for (int i = 0; i < n; ++i)
    if (parents[i] < 0 || parents[i] >= src->B) return e->fail(IVG_ERR_INVALID, "enc_cache_select: every parent must be a row of the source cache, [0, " + std::to_string(src->B) + ")");
  ivg_enc_cache* k = nullptr;
  IVG_TRY(ivg_enc_cache_create(e, n, &k));
  k->filled = true; k->ctx = src->ctx;
  // rows are dense in the context length of the fill: ctx * side * side * C elements per trajectory, K and V^T alike
  int rc = 0;
  for (size_t s = 0; s < src->Kp.size() && rc == 0; ++s) {
    const XAttW& x = e->cenc.xatt[s];
    const long row = (long)src->ctx * x.side * x.side * x.C * (long)dtype_size(e->enc_dt);
    rc = launch_gather_rows_by_parent(src->Kp[s], k->Kp[s], row, parents, n, (hipStream_t)stream);
    if (rc == 0) rc = launch_gather_rows_by_parent(src->VpT[s], k->VpT[s], row, parents, n, (hipStream_t)stream);
  }
  if (rc) { ivg_enc_cache_destroy(e, k); return e->fail(IVG_ERR_HIP, "enc_cache_select: gather launch failed: hip error " + std::to_string(rc)); }
  *out = k;
  return IVG_OK;
}

void ivg_reload_switches(void) { reload_switches(); }

int ivg_set_temperature(ivg_engine* e, float temperature) {
  if (!e) return IVG_ERR_INVALID;
  if (!(temperature > 0.0f) || !std::isfinite(temperature)) return e->fail(IVG_ERR_INVALID, "temperature must be a strictly positive float");   // HF raises the same
  e->temperature = temperature;
  return IVG_OK;
}

int ivg_set_top_p(ivg_engine* e, float top_p) {
  if (!e) return IVG_ERR_INVALID;
  if (!(top_p >= 0.0f && top_p <= 1.0f)) return e->fail(IVG_ERR_INVALID, "top_p must be a float in [0, 1]");   // HF raises the same (NaN included)
  e->top_p = top_p;
  return IVG_OK;
}

int ivg_engine::effective_lds_kb() const { return decode_lds_kb > 0 ? decode_lds_kb : ivg::sw().decode_lds_kb; }

int ivg_set_decode_lds_kb(ivg_engine* e, int kb) {
  if (!e) return IVG_ERR_INVALID;
  if (kb != 0 && (kb < 16 || kb > 160)) return e->fail(IVG_ERR_INVALID, "decode_lds_kb must be 0 (process default) or 16 .. 160");
  e->decode_lds_kb = kb;
  return IVG_OK;
}

// the FP8 cache's entries: engines it is not for are refused in the same words
static int need_fp8(ivg_engine* e, const char* who) { return e->kvc.fp8_eligible() ? 0 : e->fail(IVG_ERR_INVALID, std::string(who) + ": " + KvCache::kFp8Needs); }

int ivg_set_kv_format(ivg_engine* e, int format, float k_scale, float v_scale) {
  if (!e) return IVG_ERR_INVALID;
  if (format != IVG_KV_NATIVE && format != IVG_KV_FP8_E4M3) return e->fail(IVG_ERR_INVALID, "set_kv_format: format must be IVG_KV_NATIVE or IVG_KV_FP8_E4M3");
  if (!kv8_scale_ok(k_scale) || !kv8_scale_ok(v_scale))
    return e->fail(IVG_ERR_INVALID, "set_kv_format: k_scale and v_scale must be finite, positive powers of two (2^-126 .. 2^126)");
  if (format == IVG_KV_FP8_E4M3) IVG_TRY(need_fp8(e, "set_kv_format"));
  e->kvc.set_format(format == IVG_KV_FP8_E4M3, k_scale, v_scale);
  return IVG_OK;
}

int ivg_set_kv_scales(ivg_engine* e, const float* scales) {
  if (!e) return IVG_ERR_INVALID;
  IVG_TRY(need_fp8(e, "set_kv_scales"));
  if (!scales) return e->fail(IVG_ERR_INVALID, "set_kv_scales: null argument");
  for (size_t i = 0; i < e->kvc.table_n(); ++i)
    if (!kv8_scale_ok(scales[i])) return e->fail(IVG_ERR_INVALID, "set_kv_scales: " + e->kvc.name(i) + ": every scale must be a finite, positive power of two (2^-126 .. 2^126)");
  return e->kvc.set_scales(scales, e->err);
}

int ivg_get_kv_scales(ivg_engine* e, float* scales_out) {
  if (!e) return IVG_ERR_INVALID;
  if (e->cfg.num_layers <= 0 || !scales_out) return e->fail(IVG_ERR_INVALID, "get_kv_scales: engine without a transformer, or null argument");
  e->kvc.get_scales(scales_out);
  return IVG_OK;
}

int ivg_kv_calibration_reset(ivg_engine* e) {
  if (!e) return IVG_ERR_INVALID;
  IVG_TRY(need_fp8(e, "kv_calibration_reset"));
  return e->kvc.reset_amax(e->err);
}

// the action table (rows x action_dim, or null) embedded into workspace memory of the running pass: *out [rows][H] llm dtype, or null
static int embed_actions(Run& r, const float* actions, int rows, const void** out) {
  ivg_engine* e = r.e;
  *out = nullptr;
  if (!actions) return 0;
  char* buf = (char*)e->ws.alloc((size_t)rows * e->cfg.hidden_size * dtype_size(e->llm_dt));
  if (!r.planning && launch_action_embed(actions, e->act_w, e->act_b, buf, e->llm_dt, rows, e->cfg.action_dim, e->cfg.hidden_size, r.st))
    return e->fail(IVG_ERR_HIP, "action_embed launch failed");
  *out = buf;
  return 0;
}

int ivg_kv_calibrate(ivg_engine* e, const int64_t* ids, int64_t ids_stride, int B, int L, const float* actions, int act_T, int ctx, ivg_stream stream) {
  if (!e) return IVG_ERR_INVALID;
  IVG_TRY(need_fp8(e, "kv_calibrate"));
  if (!ids || ids_stride < L) return e->fail(IVG_ERR_INVALID, "kv_calibrate: null ids, or ids_stride below L");
  if (B <= 0 || L < 1 || L > e->Lmax) return e->fail(IVG_ERR_CAPACITY, "kv_calibrate: batch or length exceeds capacity");
  if (actions && (e->cfg.action_dim <= 0 || !e->act_w)) return e->fail(IVG_ERR_INVALID, "kv_calibrate: actions given but the model is action-free");
  if (actions && (ctx < 1 || act_T < 1 || act_T > e->cfg.max_frames)) return e->fail(IVG_ERR_INVALID, "kv_calibrate: bad ctx / act_T");
  const int Bc = e->kvc.chunk;   // the prompt pass's chunk: the cache (and its scratch) holds that many trajectories
  e->kvc.forget_kept();          // the pass overwrites cache rows
  int rc = plan_then_run(e, (hipStream_t)stream, [&](Run& r) {
    r.kv_amax = e->kvc.amax;
    for (int b0 = 0; b0 < B; b0 += Bc) {
      const size_t m = e->ws.mark();
      // the teacher-forced prompt pass (actions on every sdf slot, as ivg_logits), no lm_head: kv_absmax_kernel follows each layer's rope_kv
      PrefillReq q; q.ids = r.planning ? nullptr : ids + (long)b0 * ids_stride; q.ids_stride = ids_stride; q.B = std::min(Bc, B - b0); q.L = L;
      q.act_T = act_T; q.ctx = ctx; q.all_slots = true;
      IVG_TRY(embed_actions(r, actions ? actions + (size_t)b0 * act_T * e->cfg.action_dim : nullptr, q.B * act_T, &q.act_emb));
      IVG_TRY(r.prefill(q));
      e->ws.reset(m);
    }
    return 0;
  });
  if (rc == 0) { e->kvc.calib_stream = (hipStream_t)stream; e->kvc.calib_pending = true; }
  return rc;
}

int ivg_kv_calibration_finish(ivg_engine* e, int headroom_log2, float* amax_out, float* scales_out) {
  if (!e) return IVG_ERR_INVALID;
  IVG_TRY(need_fp8(e, "kv_calibration_finish"));
  if (headroom_log2 < 0 || headroom_log2 > 8) return e->fail(IVG_ERR_INVALID, "kv_calibration_finish: headroom_log2 must be in [0, 8]");
  std::vector<uint32_t> bits; std::vector<float> sc;
  long bad = -1;
  IVG_TRY(e->kvc.calibrated_scales(headroom_log2, bits, sc, &bad, e->err));
  if (amax_out) memcpy(amax_out, bits.data(), bits.size() * 4);
  if (bad >= 0)
    return e->fail(IVG_ERR_INVALID, "kv_calibration_finish: " + e->kvc.name(bad) + " saw " + (bits[bad] > 0x7f800000u ? "NaN" : "Inf") + ": no scales installed");
  IVG_TRY(ivg_set_kv_scales(e, sc.data()));
  if (scales_out) memcpy(scales_out, sc.data(), sc.size() * 4);
  return IVG_OK;
}

int ivg_set_output_clamp(ivg_engine* e, int on) {
  if (!e) return IVG_ERR_INVALID;
  e->clamp_out = on != 0;
  return IVG_OK;
}

int ivg_detokenize_to(ivg_engine* e, const int64_t* ids, int B, int F, void* pixels_out, int pixel_dtype, ivg_cache* cache, int cache_mode,
                      ivg_stream stream) {
  if (!e) return IVG_ERR_INVALID;
  IVG_TRY(check_tok(e, B, e->ctx + F, "detokenize"));
  if (F < 0) return e->fail(IVG_ERR_INVALID, "detokenize: token count does not match 257*ctx - 1 + 17*F");
  if (pixel_dtype != IVG_F32 && pixel_dtype != IVG_BF16) return e->fail(IVG_ERR_INVALID, "detokenize: pixels are float32 or bfloat16");
  return plan_then_run(e, (hipStream_t)stream, [&](Run& r) { return r.detokenize(ids, B, F, pixels_out, (DType)pixel_dtype, cache, cache ? cache_mode : 0); });
}

int ivg_detokenize_shared(ivg_engine* e, const int64_t* ids, int n_groups, int group_size, int F, void* pixels_out, int pixel_dtype, ivg_stream stream) {
  if (!e) return IVG_ERR_INVALID;
  if (n_groups <= 0 || group_size <= 0) return e->fail(IVG_ERR_INVALID, "detokenize_shared: n_groups and group_size must be positive");
  const int B = n_groups * group_size;
  IVG_TRY(check_tok(e, B, e->ctx + F, "detokenize"));
  if (F < 0) return e->fail(IVG_ERR_INVALID, "detokenize: token count does not match 257*ctx - 1 + 17*F");
  if (pixel_dtype != IVG_F32 && pixel_dtype != IVG_BF16) return e->fail(IVG_ERR_INVALID, "detokenize: pixels are float32 or bfloat16");
  return plan_then_run(e, (hipStream_t)stream, [&](Run& r) { return r.detokenize(ids, B, F, pixels_out, (DType)pixel_dtype, nullptr, 0, group_size); });
}

int ivg_detokenize(ivg_engine* e, const int64_t* ids, int B, int F, float* pixels_out, ivg_cache* cache, int cache_mode, ivg_stream stream) {
  return ivg_detokenize_to(e, ids, B, F, pixels_out, IVG_F32, cache, cache_mode, stream);
}

int ivg_cache_create(ivg_engine* e, int B, ivg_cache** out) {
  if (!e || !out || e->cfg.n_levels <= 0) return IVG_ERR_INVALID;
  const ivg_config& c = e->cfg;
  if (B <= 0 || B > c.max_batch) return e->fail(IVG_ERR_CAPACITY, "cache_create: batch " + std::to_string(B) + " exceeds the engine's max_batch");
  ivg_cache* k = new ivg_cache();
  k->B = B;
  const int ctx = c.context_length, res = c.resolution, nl = c.n_levels;
  bool ok = hipMalloc((void**)&k->ctx_pixels, (size_t)B * ctx * 3 * res * res * 4) == hipSuccess;
  // same order as decoder_feature_plan: [1] then every up level whose side <= max_att
  auto add = [&](int side, int C) {
    void* p = nullptr;
    if (ok && hipMalloc(&p, (size_t)B * ctx * side * side * C * dtype_size(e->dec_dt)) == hipSuccess) k->feat.push_back(p);
    else ok = false;
  };
  add(16, c.block_out_channels[nl - 1]);
  int s = 16;
  for (int i = 0; i < nl; ++i) { if (i != nl - 1) s *= 2; if (s <= c.max_att_resolution) add(s, c.block_out_channels[nl - 1 - i]); }
  if (!ok) {   // a partial cache would be overrun by the feature writes of detokenize: release everything
    (void)hipGetLastError();
    if (k->ctx_pixels) (void)hipFree(k->ctx_pixels);
    for (void* p : k->feat) (void)hipFree(p);
    delete k;
    return e->fail(IVG_ERR_HIP, "cache_create: hipMalloc failed");
  }
  *out = k;
  return IVG_OK;
}

int ivg_cache_select(ivg_engine* e, const ivg_cache* src, const int32_t* parents, int n, ivg_cache** out, ivg_stream stream) {
  if (!e || !out || e->cfg.n_levels <= 0) return IVG_ERR_INVALID;
  if (!src || !src->filled || src->ctx <= 0) return e->fail(IVG_ERR_INVALID, "cache_select: the source cache is empty");
  if (!parents) return e->fail(IVG_ERR_INVALID, "cache_select: null argument");
  for (int i = 0; i < n; ++i)
    if (parents[i] < 0 || parents[i] >= src->B) return e->fail(IVG_ERR_INVALID, "cache_select: every parent must be a row of the source cache, [0, " + std::to_string(src->B) + ")");
  ivg_cache* k = nullptr;
  IVG_TRY(ivg_cache_create(e, n, &k));
  if (k->feat.size() != src->feat.size()) { ivg_cache_destroy(e, k); return e->fail(IVG_ERR_INVALID, "cache_select: cache layout mismatch"); }
  k->pix_dt = src->pix_dt; k->clamped = src->clamped; k->filled = true; k->ctx = src->ctx;
  // rows are contiguous per trajectory, in the sizes Run::detokenize filled them with: ctx frames of pixels / of every feature map
  const ivg_config& c = e->cfg;
  const int nl = c.n_levels;
  const long ctx = src->ctx, res = c.resolution;
  hipStream_t st = (hipStream_t)stream;
  int rc = launch_gather_rows_by_parent(src->ctx_pixels, k->ctx_pixels, ctx * 3 * res * res * (src->pix_dt == (int)F32 ? 4 : 2), parents, n, st);
  size_t fi = 0;
  auto feat = [&](long side, long C) {
    if (rc == 0) rc = launch_gather_rows_by_parent(src->feat[fi], k->feat[fi], ctx * side * side * C * (long)dtype_size(e->dec_dt), parents, n, st);
    ++fi;
  };
  feat(16, c.block_out_channels[nl - 1]);   // (the order of ivg_cache_create)
  long s = 16;
  for (int i = 0; i < nl; ++i) { if (i != nl - 1) s *= 2; if (s <= c.max_att_resolution) feat(s, c.block_out_channels[nl - 1 - i]); }
  if (rc) { ivg_cache_destroy(e, k); return e->fail(IVG_ERR_HIP, "cache_select: gather launch failed: hip error " + std::to_string(rc)); }
  *out = k;
  return IVG_OK;
}

void ivg_cache_destroy(ivg_engine* e, ivg_cache* c) {
  if (!c) return;
  if (e) (void)hipSetDevice(e->device);
  (void)hipDeviceSynchronize();
  if (c->ctx_pixels) (void)hipFree(c->ctx_pixels);
  for (void* p : c->feat) (void)hipFree(p);
  delete c;
}

// The opening checks of the ivg_generate* entries, in the order and the words each entry has always used (callers match on both).
// own_err: the outcome of the entry's own argument check, which comes right after the transformer check (null: passed)
enum GenEntry { GEN_PLAIN, GEN_SHARED, GEN_CONTINUE, GEN_EMBEDS };
static int check_generate(ivg_engine* e, GenEntry entry, const char* own_err, int B, int L0, int n_new, const float* actions, int act_T, int ctx) {
  const bool shared = entry == GEN_SHARED, cont = entry == GEN_CONTINUE, emb = entry == GEN_EMBEDS;
  if (e->cfg.num_layers <= 0) return e->fail(IVG_ERR_INVALID, "generate: engine was created without a transformer");
  if (own_err) return e->fail(IVG_ERR_INVALID, own_err);
  const int Bmax = emb ? e->kvc.chunk : B;   // an embeds call is one chunk of the cache
  if (B <= 0 || B > Bmax || n_new < 1 || L0 < (shared || cont ? 2 : 1) || L0 + n_new > e->Lmax)
    return e->fail(IVG_ERR_CAPACITY, emb ? "generate_embeds: batch " + std::to_string(B) + " / sequence of " + std::to_string(L0 + n_new) + " tokens exceeds the capacity (" +
                                               std::to_string(Bmax) + " x " + std::to_string(e->Lmax) + ")"
                                         : "generate: sequence of " + std::to_string(L0 + n_new) + " tokens exceeds the KV cache (" + std::to_string(e->Lmax) + ")");
  if (!actions) return 0;
  if (e->cfg.action_dim <= 0 || !e->act_w) return e->fail(IVG_ERR_INVALID, "generate: actions given but the model is action-free");
  // a shared prefix is [0, L0 - 1): it may not contain an action slot (those carry per-trajectory actions), so the prompt is the
  // context alone -- its last token, the first sdf slot, is fed per trajectory
  if (shared && L0 != 257 * ctx) return e->fail(IVG_ERR_INVALID, "generate_shared: an action-conditioned shared prompt must hold exactly 257*ctx tokens");
  if (L0 < 257 * ctx || (L0 - 257 * ctx) % 17 != 0) return e->fail(IVG_ERR_INVALID, "generate: action-conditioned prompt must hold 257*ctx + 17*t tokens");
  const int last = (L0 - 257 * ctx) / 17 + n_new / 17 + ctx - 1;  // highest action row read (prompt slots + forced sdf slots)
  if (last >= act_T || act_T > e->cfg.max_frames) return e->fail(IVG_ERR_INVALID, "generate: action tensor too short (or longer than max_frames)");
  return 0;
}

// What an id-prompt entry adds to the checks they all share (generate_checked tries them in the order of the fields)
struct GenRules {
  GenEntry kind = GEN_PLAIN; const char* own_err = nullptr;   // check_generate's entry kind and the entry's own argument error
  bool need_frames = false;        // ivg_generate_frames' conditions on the schedule and the lengths
  bool kept = false;               // the prefix [0, L0 - 1) is the kept cache of the same B trajectories (ivg_generate_continue) ...
  bool fanout = false;             // ... or of the B / group trajectories the candidates fan out of (ivg_generate_fanout)
};

static GenerateReq id_request(const int64_t* prompt, int64_t prompt_stride, int B, int L0, int n_new, const float* actions, int act_T, int ctx,
                              const float* uniforms, int top_k, int64_t* ids_out) {
  GenerateReq q; q.prompt = prompt; q.prompt_stride = prompt_stride; q.B = B; q.L0 = L0; q.n_new = n_new; q.actions = actions; q.act_T = act_T; q.ctx = ctx;
  q.uniforms = uniforms; q.top_k = top_k; q.ids_out = ids_out;
  return q;
}

static int run_generate(ivg_engine* e, const GenerateReq& q, ivg_stream stream) {
  return plan_then_run(e, (hipStream_t)stream, [&](Run& r) { return r.generate(q); });
}

// Every id-prompt entry: the checks in the order they have always been tried, then the rollout
static int generate_checked(ivg_engine* e, const GenerateReq& q, const GenRules& r, ivg_stream stream) {
  const int B = q.B, L0 = q.L0;
  IVG_TRY(check_generate(e, r.kind, r.own_err, B, L0, q.n_new, q.actions, q.act_T, q.ctx));
  if (r.need_frames && q.n_new < 17) return e->fail(IVG_ERR_INVALID, "generate_frames: a frame needs 17 new tokens (its 16th must be fed)");
  if (r.need_frames && (q.ctx < 1 || L0 < 257 * q.ctx || (L0 - 257 * q.ctx) % 17 != 0))
    return e->fail(IVG_ERR_INVALID, "generate_frames: the prompt must hold 257*ctx + 17*t tokens (frames count from the first new token)");
  if (q.frame_rewards_out && !e->rew_w) return e->fail(IVG_ERR_MISSING, "generate_frames: rewards requested but reward_linear is not loaded");
  if (q.frame_hidden_out && !e->final_norm) return e->fail(IVG_ERR_MISSING, "generate_frames: hidden states requested but 'llm.norm' is not in the weight table");
  if (r.kept) {
    if (!e->kvc.holds(B, L0 - 1))
      return e->fail(IVG_ERR_INVALID, "generate_continue: the KV cache holds " + std::to_string(e->kvc.len) + " positions of " + std::to_string(e->kvc.B) +
                                          " trajectories, the call needs " + std::to_string(L0 - 1) + " of " + std::to_string(B));
    // same (batch, length) is not enough: another caller may have used the model in between.  Compare the cached prefix
    // (token ids + the action rows baked into its sdf slots) with the prompt on the device (one stream synchronisation).
    bool same = false;
    IVG_TRY(kv_prefix_matches_ids(e, q.prompt, q.prompt_stride, B, L0 - 1, q.actions, q.act_T, q.ctx, (hipStream_t)stream, &same));
    if (!same) return e->fail(IVG_ERR_INVALID, "generate_continue: the KV cache was built from a different prefix (tokens or actions differ)");
  }
  if (r.fanout) {
    const int n_groups = B / q.group;
    if (B > e->kvc.chunk)
      return e->fail(IVG_ERR_CAPACITY, "generate_fanout: " + std::to_string(B) + " candidates exceed the KV-cache chunk (" + std::to_string(e->kvc.chunk) + ")");
    if (!e->kvc.ids_valid || !e->kvc.holds(n_groups, L0 - 1))
      return e->fail(IVG_ERR_INVALID, "generate_fanout: the kept KV cache holds " + std::to_string(e->kvc.len) + " positions of " + std::to_string(e->kvc.B) +
                                          " trajectories built from ids, the call needs " + std::to_string(L0 - 1) + " of " + std::to_string(n_groups));
    bool same = false;
    IVG_TRY(kv_prefix_matches_ids(e, q.prompt, q.prompt_stride, n_groups, L0 - 1, q.actions, q.act_T, q.ctx, (hipStream_t)stream, &same, true));
    if (!same) return e->fail(IVG_ERR_INVALID, "generate_fanout: the kept KV cache was built from a different prefix (tokens, context length or action conditioning differ)");
  }
  return run_generate(e, q, stream);
}

static const char* continue_err(const ivg_engine* e, const float* actions) {
  return actions && e->cfg.action_dim > 0 && e->act_w ? nullptr : "generate_continue: action-conditioned models only";
}

int ivg_generate(ivg_engine* e, const int64_t* prompt, int64_t prompt_stride, int B, int L0, int n_new, const float* actions, int act_T,
                 int ctx, const float* uniforms, int top_k, int64_t* ids_out, float* reward_out, ivg_stream stream) {
  if (!e) return IVG_ERR_INVALID;
  GenerateReq q = id_request(prompt, prompt_stride, B, L0, n_new, actions, act_T, ctx, uniforms, top_k, ids_out);
  q.reward_out = reward_out;
  return generate_checked(e, q, GenRules(), stream);
}

int ivg_generate_shared(ivg_engine* e, const int64_t* prompts, int64_t prompt_stride, int n_groups, int group_size, int L0, int n_new,
                        const float* actions, int act_T, int ctx, const float* uniforms, int top_k, int force_sdf, int64_t* ids_out, float* reward_out,
                        ivg_stream stream) {
  if (!e) return IVG_ERR_INVALID;
  const bool sized = n_groups > 0 && group_size > 0;
  GenerateReq q = id_request(prompts, prompt_stride, sized ? n_groups * group_size : 1, L0, n_new, actions, act_T, ctx, uniforms, top_k, ids_out);
  q.reward_out = reward_out; q.force_sdf = force_sdf != 0;
  q.group = group_size;   // 1: nothing to share -- the plain entry (one prefill over all rows)
  GenRules r; r.kind = GEN_SHARED; r.own_err = sized ? nullptr : "generate_shared: n_groups and group_size must be positive";
  return generate_checked(e, q, r, stream);
}

int ivg_generate_forced_sdf(ivg_engine* e, const int64_t* prompt, int64_t prompt_stride, int B, int L0, int n_new, int ctx, const float* uniforms,
                            int top_k, int64_t* ids_out, ivg_stream stream) {
  if (!e) return IVG_ERR_INVALID;
  GenerateReq q = id_request(prompt, prompt_stride, B, L0, n_new, nullptr, 0, ctx, uniforms, top_k, ids_out);
  q.force_sdf = true;
  return generate_checked(e, q, GenRules(), stream);
}

int ivg_generate_continue(ivg_engine* e, const int64_t* prompt, int64_t prompt_stride, int B, int L0, int n_new, const float* actions,
                          int act_T, int ctx, const float* uniforms, int top_k, int64_t* ids_out, float* reward_out, ivg_stream stream) {
  if (!e) return IVG_ERR_INVALID;
  GenerateReq q = id_request(prompt, prompt_stride, B, L0, n_new, actions, act_T, ctx, uniforms, top_k, ids_out);
  q.reward_out = reward_out; q.reuse_kv = true;
  GenRules r; r.kind = GEN_CONTINUE; r.own_err = continue_err(e, actions); r.kept = true;
  return generate_checked(e, q, r, stream);
}

int ivg_kv_select(ivg_engine* e, const int32_t* parents, int n, ivg_stream stream) {
  if (!e) return IVG_ERR_INVALID;
  if (e->cfg.num_layers <= 0) return e->fail(IVG_ERR_INVALID, "kv_select: engine was created without a transformer");
  return kv_select(e, parents, n, (hipStream_t)stream);
}

int ivg_kv_snapshot_create(ivg_engine* e, ivg_kv_snapshot** out, ivg_stream stream) {
  if (!e) return IVG_ERR_INVALID;
  if (!out) return e->fail(IVG_ERR_INVALID, "kv_snapshot_create: null argument");
  if (e->cfg.num_layers <= 0) return e->fail(IVG_ERR_INVALID, "kv_snapshot_create: engine was created without a transformer");
  return kv_snapshot_create(e, out, (hipStream_t)stream);
}

int ivg_kv_snapshot_restore(ivg_engine* e, const ivg_kv_snapshot* s, const int32_t* parents, int n, ivg_stream stream) {
  if (!e) return IVG_ERR_INVALID;
  if (!s) return e->fail(IVG_ERR_INVALID, "kv_snapshot_restore: null snapshot");
  if (e->cfg.num_layers <= 0) return e->fail(IVG_ERR_INVALID, "kv_snapshot_restore: engine was created without a transformer");
  return kv_snapshot_restore(e, s, parents, n, (hipStream_t)stream);
}

void ivg_kv_snapshot_destroy(ivg_kv_snapshot* s) {
  if (!s) return;
  (void)hipFree(s->mem);   // (waits for the device: copies of a create or restore still queued have finished)
  delete s;
}

int ivg_kv_snapshot_info(const ivg_kv_snapshot* s, int64_t* out) {
  if (!s || !out) return IVG_ERR_INVALID;
  const int64_t v[IVG_KV_SNAPSHOT_INFO_INTS] = {s->B, s->len, (int64_t)s->bytes, s->snap_valid ? 1 : 0, s->act_T, s->ctx,
                                                s->format == KvFormat::Fp8 ? IVG_KV_FP8_E4M3 : s->format == KvFormat::Planes24 ? 2 : IVG_KV_NATIVE, s->device};
  for (int i = 0; i < IVG_KV_SNAPSHOT_INFO_INTS; ++i) out[i] = v[i];
  return IVG_OK;
}

// ivg_kv_extend and ivg_kv_extend_scored: one body, `who` the entry's name in its messages; the three outputs of the latter are null for the former
static int kv_extend_checked(ivg_engine* e, const std::string& who, const int64_t* prompt, int64_t prompt_stride, int B, int keep_len, int L0,
                             const float* actions, int act_T, int ctx, float* token_nll_out, float* token_scores_out, float* frame_rewards_out,
                             void* frame_hidden_out, ivg_stream stream) {
  if (!e) return IVG_ERR_INVALID;
  if (e->cfg.num_layers <= 0) return e->fail(IVG_ERR_INVALID, who + ": engine was created without a transformer");
  const KvCache& k = e->kvc;
  if (!prompt) return e->fail(IVG_ERR_INVALID, who + ": null prompt");
  IVG_TRY(need_kept_cache(e, who.c_str()));
  if (!k.ids_valid) return e->fail(IVG_ERR_INVALID, who + ": the kept cache was built from input embeddings (only caches built from ids are extended)");
  if (L0 - 1 > e->Lmax) return e->fail(IVG_ERR_CAPACITY, who + ": " + std::to_string(L0 - 1) + " positions exceed the KV cache (" + std::to_string(e->Lmax) + ")");
  if (B != k.B) return e->fail(IVG_ERR_INVALID, who + ": the kept cache holds " + std::to_string(k.B) + " trajectories, the call presents " + std::to_string(B));
  if (keep_len < 1 || keep_len > k.len || keep_len > L0 - 1)
    return e->fail(IVG_ERR_INVALID, who + ": keep_len must lie in [1, min(" + std::to_string(k.len) + " kept positions, L0 - 1)]");
  if (actions) {
    if (e->cfg.action_dim <= 0 || !e->act_w) return e->fail(IVG_ERR_INVALID, who + ": actions given but the model is action-free");
    const int slots = std::max(0, (L0 - 1 - (257 * ctx - 1) + 16) / 17);   // sdf slots among positions [0, L0 - 1)
    if (ctx < 1 || act_T < 1 || act_T > e->cfg.max_frames || (slots > 0 && ctx - 1 + slots > act_T))
      return e->fail(IVG_ERR_INVALID, who + ": action tensor too short for the sdf slots of the prompt (or longer than max_frames)");
  }
  if (frame_rewards_out && !e->rew_w) return e->fail(IVG_ERR_MISSING, who + ": rewards requested but reward_linear is not loaded");
  if (frame_hidden_out && !e->final_norm) return e->fail(IVG_ERR_MISSING, who + ": hidden states requested but 'llm.norm' is not in the weight table");
  bool same = false;
  IVG_TRY(kv_prefix_matches_ids(e, prompt, prompt_stride, B, keep_len, actions, act_T, ctx, (hipStream_t)stream, &same));
  if (!same) return e->fail(IVG_ERR_INVALID, who + ": the kept cache was built from a different prefix (tokens, actions or context length differ)");
  if (keep_len == L0 - 1) {   // a pure rewind: the kept rows [0, keep_len) are what they were, nothing is launched
    e->kvc.len = keep_len;
    return IVG_OK;
  }
  ExtendReq q; q.prompt = prompt; q.prompt_stride = prompt_stride; q.B = B; q.keep_len = keep_len; q.L0 = L0; q.actions = actions; q.act_T = act_T; q.ctx = ctx;
  q.token_nll = token_nll_out; q.chunk = kv_extend_chunk_covers(e);
  q.token_scores = token_scores_out; q.frame_rewards = frame_rewards_out; q.frame_hidden = frame_hidden_out;
  return plan_then_run(e, (hipStream_t)stream, [&](Run& r) { return r.extend(q); });
}

int ivg_kv_extend(ivg_engine* e, const int64_t* prompt, int64_t prompt_stride, int B, int keep_len, int L0, const float* actions, int act_T, int ctx,
                  float* token_nll_out, ivg_stream stream) {
  return kv_extend_checked(e, "kv_extend", prompt, prompt_stride, B, keep_len, L0, actions, act_T, ctx, token_nll_out, nullptr, nullptr, nullptr, stream);
}

int ivg_kv_extend_scored(ivg_engine* e, const int64_t* prompt, int64_t prompt_stride, int B, int keep_len, int L0, const float* actions, int act_T,
                         int ctx, float* token_nll_out, float* token_scores_out, float* frame_rewards_out, void* frame_hidden_out, ivg_stream stream) {
  return kv_extend_checked(e, "kv_extend_scored", prompt, prompt_stride, B, keep_len, L0, actions, act_T, ctx, token_nll_out, token_scores_out,
                           frame_rewards_out, frame_hidden_out, stream);
}

// ivg_generate_frames, ivg_generate_scored and ivg_generate_fanout each stand for several rollouts: which one, from group_size / kept_cache /
// fanout.  need_frames: always for ivg_generate_frames, for the others only when a frame output is asked for (without one
// ivg_generate_scored also stands for the action-free ivg_generate).  fanout: B = n_groups * group_size candidates whose groups' prefixes
// are the kept cache's rows -- lengths and action table checked as for a kept-cache call (the prompt may hold generated frames)
static GenRules frames_rules(const ivg_engine* e, GenerateReq& q, bool need_frames, int group_size, int kept_cache, int force_sdf, bool fanout) {
  const int B = q.B;
  const bool shared = group_size > 1 && !fanout, cont = kept_cache != 0;
  q.force_sdf = force_sdf != 0; q.group = group_size; q.reuse_kv = cont; q.fanout = fanout;
  GenRules r; r.kind = shared ? GEN_SHARED : (cont || fanout) ? GEN_CONTINUE : GEN_PLAIN; r.need_frames = need_frames; r.kept = cont; r.fanout = fanout;
  if (group_size < 1 || (shared && (B <= 0 || B % group_size != 0))) r.own_err = "generate_frames: B must be a positive multiple of a positive group_size";
  else if (fanout && (B <= 0 || B % group_size != 0)) r.own_err = "generate_fanout: n_groups and group_size must be positive";
  else if (cont && shared) r.own_err = "generate_frames: a kept cache is per trajectory (group_size must be 1)";
  else if (need_frames && !q.actions && !force_sdf) r.own_err = "generate_frames: frames exist under the forced-sdf schedule only (actions or force_sdf)";
  else if (cont) r.own_err = continue_err(e, q.actions);
  return r;
}

int ivg_generate_frames(ivg_engine* e, const int64_t* prompt, int64_t prompt_stride, int B, int L0, int n_new, const float* actions, int act_T,
                        int ctx, const float* uniforms, int top_k, int group_size, int kept_cache, int force_sdf, int64_t* ids_out,
                        float* frame_rewards_out, void* frame_hidden_out, ivg_stream stream) {
  if (!e) return IVG_ERR_INVALID;
  GenerateReq q = id_request(prompt, prompt_stride, B, L0, n_new, actions, act_T, ctx, uniforms, top_k, ids_out);
  q.frame_rewards_out = frame_rewards_out; q.frame_hidden_out = frame_hidden_out;
  return generate_checked(e, q, frames_rules(e, q, true, group_size, kept_cache, force_sdf, false), stream);
}

int ivg_generate_scored(ivg_engine* e, const int64_t* prompt, int64_t prompt_stride, int B, int L0, int n_new, const float* actions, int act_T,
                        int ctx, const float* uniforms, int top_k, int group_size, int kept_cache, int force_sdf, int64_t* ids_out,
                        float* frame_rewards_out, void* frame_hidden_out, float* token_scores_out, ivg_stream stream) {
  return ivg_generate_filtered(e, prompt, prompt_stride, B, L0, n_new, actions, act_T, ctx, uniforms, top_k, group_size, kept_cache, force_sdf, ids_out,
                               frame_rewards_out, frame_hidden_out, token_scores_out, nullptr, stream);
}

int ivg_generate_filtered(ivg_engine* e, const int64_t* prompt, int64_t prompt_stride, int B, int L0, int n_new, const float* actions, int act_T,
                          int ctx, const float* uniforms, int top_k, int group_size, int kept_cache, int force_sdf, int64_t* ids_out,
                          float* frame_rewards_out, void* frame_hidden_out, float* token_scores_out, float* filtered_scores_out, ivg_stream stream) {
  if (!e) return IVG_ERR_INVALID;
  GenerateReq q = id_request(prompt, prompt_stride, B, L0, n_new, actions, act_T, ctx, uniforms, top_k, ids_out);
  q.frame_rewards_out = frame_rewards_out; q.frame_hidden_out = frame_hidden_out; q.token_scores_out = token_scores_out;
  q.filtered_scores_out = filtered_scores_out;
  return generate_checked(e, q, frames_rules(e, q, frame_rewards_out || frame_hidden_out, group_size, kept_cache, force_sdf, false), stream);
}

int ivg_generate_fanout(ivg_engine* e, const int64_t* prompt, int64_t prompt_stride, int n_groups, int group_size, int L0, int n_new,
                        const float* actions, int act_T, int ctx, const float* uniforms, int top_k, int force_sdf, int64_t* ids_out,
                        float* frame_rewards_out, void* frame_hidden_out, float* token_scores_out, ivg_stream stream) {
  return ivg_generate_fanout_filtered(e, prompt, prompt_stride, n_groups, group_size, L0, n_new, actions, act_T, ctx, uniforms, top_k, force_sdf, ids_out,
                                      frame_rewards_out, frame_hidden_out, token_scores_out, nullptr, stream);
}

int ivg_generate_fanout_filtered(ivg_engine* e, const int64_t* prompt, int64_t prompt_stride, int n_groups, int group_size, int L0, int n_new,
                                 const float* actions, int act_T, int ctx, const float* uniforms, int top_k, int force_sdf, int64_t* ids_out,
                                 float* frame_rewards_out, void* frame_hidden_out, float* token_scores_out, float* filtered_scores_out,
                                 ivg_stream stream) {
  if (!e) return IVG_ERR_INVALID;
  const bool sized = n_groups > 0 && group_size > 0 && (long)n_groups * group_size <= INT32_MAX;
  GenerateReq q = id_request(prompt, prompt_stride, sized ? n_groups * group_size : 0, L0, n_new, actions, act_T, ctx, uniforms, top_k, ids_out);
  q.frame_rewards_out = frame_rewards_out; q.frame_hidden_out = frame_hidden_out; q.token_scores_out = token_scores_out;
  q.filtered_scores_out = filtered_scores_out;
  return generate_checked(e, q, frames_rules(e, q, frame_rewards_out || frame_hidden_out, sized ? group_size : 0, 0, force_sdf, true), stream);
}

int ivg_generate_embeds(ivg_engine* e, const void* embeds, int B, int L0, int n_new, const float* uniforms, int top_k, int64_t* new_ids_out,
                        void* hidden_out, int allow_reuse, int* reused_out, ivg_stream stream) {
  return ivg_generate_embeds_filtered(e, embeds, B, L0, n_new, uniforms, top_k, new_ids_out, hidden_out, allow_reuse, reused_out, nullptr, nullptr, stream);
}

int ivg_generate_embeds_scored(ivg_engine* e, const void* embeds, int B, int L0, int n_new, const float* uniforms, int top_k, int64_t* new_ids_out,
                               void* hidden_out, int allow_reuse, int* reused_out, float* token_scores_out, ivg_stream stream) {
  return ivg_generate_embeds_filtered(e, embeds, B, L0, n_new, uniforms, top_k, new_ids_out, hidden_out, allow_reuse, reused_out, token_scores_out, nullptr,
                                      stream);
}

int ivg_generate_embeds_filtered(ivg_engine* e, const void* embeds, int B, int L0, int n_new, const float* uniforms, int top_k, int64_t* new_ids_out,
                                 void* hidden_out, int allow_reuse, int* reused_out, float* token_scores_out, float* filtered_scores_out,
                                 ivg_stream stream) {
  if (!e) return IVG_ERR_INVALID;
  if (reused_out) *reused_out = 0;
  IVG_TRY(check_generate(e, GEN_EMBEDS, embeds && new_ids_out ? nullptr : "generate_embeds: null argument", B, L0, n_new, nullptr, 0, 1));
  bool reuse = false;
  if (allow_reuse && L0 >= 2) IVG_TRY(kv_prefix_matches_embeds(e, embeds, B, L0, (hipStream_t)stream, &reuse));
  if (reused_out) *reused_out = reuse ? 1 : 0;
  GenerateReq q; q.B = B; q.L0 = L0; q.n_new = n_new; q.uniforms = uniforms; q.top_k = top_k;
  q.reuse_kv = reuse; q.embeds = embeds; q.new_ids_out = new_ids_out; q.hidden_out = hidden_out; q.token_scores_out = token_scores_out;
  q.filtered_scores_out = filtered_scores_out;
  return run_generate(e, q, stream);
}

int ivg_embed_tokens(ivg_engine* e, const int64_t* ids, int64_t ids_stride, int B, int L, void* out, ivg_stream stream) {
  if (!e) return IVG_ERR_INVALID;
  if (e->cfg.num_layers <= 0 || !e->embed) return e->fail(IVG_ERR_INVALID, "embed_tokens: engine was created without a transformer");
  if (B <= 0 || L <= 0) return IVG_OK;
  if (launch_embed(ids, ids_stride, e->embed, out, e->llm_dt, B, L, e->cfg.hidden_size, e->cfg.vocab_size, (hipStream_t)stream))
    return e->fail(IVG_ERR_HIP, "embed_tokens: launch failed");
  return IVG_OK;
}

int ivg_action_linear(ivg_engine* e, const float* actions, int rows, void* out, ivg_stream stream) {
  if (!e) return IVG_ERR_INVALID;
  if (e->cfg.action_dim <= 0 || !e->act_w) return e->fail(IVG_ERR_INVALID, "action_linear: the model is action-free");
  if (launch_action_embed(actions, e->act_w, e->act_b, out, e->llm_dt, rows, e->cfg.action_dim, e->cfg.hidden_size, (hipStream_t)stream))
    return e->fail(IVG_ERR_HIP, "action_linear: launch failed");
  return IVG_OK;
}

int ivg_reward_linear(ivg_engine* e, const void* hidden, int rows, float* out, ivg_stream stream) {
  if (!e) return IVG_ERR_INVALID;
  if (!e->rew_w_raw || !e->rew_b) return e->fail(IVG_ERR_MISSING, "reward_linear: the model has no reward head");
  if (launch_rowdot(hidden, e->rew_w_raw, e->rew_b, out, rows, e->cfg.hidden_size, -1.0f, e->llm_dt, (hipStream_t)stream))
    return e->fail(IVG_ERR_HIP, "reward_linear: launch failed");
  return IVG_OK;
}

int ivg_logits(ivg_engine* e, const int64_t* ids, int B, int L, const float* actions, int act_T, int ctx, float* logits_out, ivg_stream stream) {
  if (!e) return IVG_ERR_INVALID;
  if (e->cfg.num_layers <= 0) return e->fail(IVG_ERR_INVALID, "logits: engine was created without a transformer");
  if (B <= 0 || B > e->kvc.chunk || L > e->Lmax) return e->fail(IVG_ERR_CAPACITY, "logits: batch or length exceeds capacity");
  if (actions && (e->cfg.action_dim <= 0 || !e->act_w)) return e->fail(IVG_ERR_INVALID, "logits: actions given but the model is action-free");
  return plan_then_run(e, (hipStream_t)stream, [&](Run& r) {
    PrefillReq q; q.ids = ids; q.ids_stride = L; q.B = B; q.L = L; q.act_T = act_T; q.ctx = ctx; q.all_slots = true; q.logits_all = logits_out;
    IVG_TRY(embed_actions(r, actions, B * act_T, &q.act_emb));
    return r.prefill(q);
  });
}

int ivg_eval_forward(ivg_engine* e, const int64_t* ids, const int64_t* labels, int B, int L, const float* actions, int act_T, int ctx,
                     float* token_nll_out, float* loss_rows_out, void* hidden_out, ivg_stream stream) {
  if (!e) return IVG_ERR_INVALID;
  if (e->cfg.num_layers <= 0) return e->fail(IVG_ERR_INVALID, "eval_forward: engine was created without a transformer");
  if (!ids || !labels || !token_nll_out || !loss_rows_out) return e->fail(IVG_ERR_INVALID, "eval_forward: null argument");
  if (B <= 0 || B > e->kvc.chunk || L < 2 || L > e->Lmax) return e->fail(IVG_ERR_CAPACITY, "eval_forward: batch or length exceeds capacity");
  if (actions && (e->cfg.action_dim <= 0 || !e->act_w)) return e->fail(IVG_ERR_INVALID, "eval_forward: actions given but the model is action-free");
  return plan_then_run(e, (hipStream_t)stream, [&](Run& r) {
    PrefillReq q; q.ids = ids; q.ids_stride = L; q.B = B; q.L = L; q.act_T = act_T; q.ctx = ctx; q.all_slots = true;
    q.hidden_all = hidden_out; q.labels = labels; q.token_nll = token_nll_out;
    IVG_TRY(embed_actions(r, actions, B * act_T, &q.act_emb));
    IVG_TRY(r.prefill(q));
    if (!r.planning && launch_ce_reduce(token_nll_out, labels, B, L, e->cfg.vocab_size, loss_rows_out, r.st)) return e->fail(IVG_ERR_HIP, "ce_reduce launch failed");
    return 0;
  });
}

int ivg_action_recon_sqerr(ivg_engine* e, const void* hidden, const float* actions, int B, int L, int act_T, int ctx, int prelude, float* out,
                           ivg_stream stream) {
  if (!e) return IVG_ERR_INVALID;
  if (!e->ar_w || !e->ar_b) return e->fail(IVG_ERR_MISSING, "action_recon: 'action_recon_linear' is not in the weight table");
  if (!hidden || !actions || !out || B <= 0 || prelude < 0 || prelude >= L) return e->fail(IVG_ERR_INVALID, "action_recon: bad argument");
  if (ctx - 1 + (L - 1 - prelude) / 17 >= act_T) return e->fail(IVG_ERR_INVALID, "action_recon: action tensor too short");
  if (launch_action_recon(hidden, e->ar_w, e->ar_b, actions, B, L, e->cfg.hidden_size, e->cfg.action_dim, act_T, ctx, prelude, out, e->llm_dt,
                          (hipStream_t)stream))
    return e->fail(IVG_ERR_HIP, "action_recon: launch failed");
  return IVG_OK;
}

int ivg_ingest_frames(const uint8_t* frames, int T, int H, int W, int center_crop, void* clip_out, int out_dtype, int resolution, ivg_stream stream) {
  if (!frames || !clip_out || (out_dtype != IVG_F32 && out_dtype != IVG_BF16)) return IVG_ERR_INVALID;
  const int rc = launch_ingest(frames, T, H, W, center_crop, clip_out, (DType)out_dtype, resolution, (hipStream_t)stream);
  return rc == 0 ? IVG_OK : (rc == (int)hipErrorInvalidValue ? IVG_ERR_INVALID : IVG_ERR_HIP);
}

int ivg_ingest_clips(const uint8_t* staging, size_t staging_bytes, const ivg_clip_desc* clips, int B, int T, int center_crop, void* out, int out_dtype,
                     int resolution, ivg_stream stream) {
  static_assert(sizeof(ivg_clip_desc) == sizeof(IngestClipDesc) && offsetof(ivg_clip_desc, frames) == offsetof(IngestClipDesc, frames) &&
                offsetof(ivg_clip_desc, W) == offsetof(IngestClipDesc, W), "ivg_clip_desc is passed through as IngestClipDesc");
  if (!staging || !clips || !out || (out_dtype != IVG_F32 && out_dtype != IVG_BF16)) return IVG_ERR_INVALID;
  const int rc = launch_ingest_clips(staging, staging_bytes, reinterpret_cast<const IngestClipDesc*>(clips), B, T, center_crop, out, (DType)out_dtype,
                                     resolution, (hipStream_t)stream);
  return rc == 0 ? IVG_OK : (rc == (int)hipErrorInvalidValue ? IVG_ERR_INVALID : IVG_ERR_HIP);
}

size_t ivg_frame_metrics_ws_bytes(int n_samples, int T, int H, int W) { return frame_metrics_ws_bytes(n_samples, T, H, W); }

int ivg_frame_metrics(const void* gt, int gt_dtype, int B, int T_gt, int gt_t0, const float* pred, int n_samples, int T_pr, int pr_t0, int T, int H,
                      int W, float* rows_out, void* ws, size_t ws_bytes, ivg_stream stream) {
  if (!gt || !pred || !rows_out || !ws) return IVG_ERR_INVALID;
  if (B <= 0 || n_samples <= 0 || n_samples % B != 0 || T <= 0 || gt_t0 < 0 || pr_t0 < 0 || gt_t0 + T > T_gt || pr_t0 + T > T_pr || H < 11 || W < 11)
    return IVG_ERR_INVALID;
  if (ws_bytes < frame_metrics_ws_bytes(n_samples, T, H, W)) return IVG_ERR_CAPACITY;
  return launch_frame_metrics(gt, (DType)gt_dtype, B, T_gt, gt_t0, pred, n_samples, T_pr, pr_t0, T, H, W, rows_out, ws, (hipStream_t)stream) ? IVG_ERR_HIP
                                                                                                                                                : IVG_OK;
}

// ---- LPIPS (lpips.hip): a handle is the table of the caller's 13 + 13 + 5 weight tensors
struct ivg_lpips {
  int device = 0;
  const float* cw[13];
  const float* cb[13];
  const float* lin[5];
};

int ivg_lpips_create(const ivg_tensor* weights, int n_weights, int device, ivg_lpips** out) {
  if (!out) return IVG_ERR_INVALID;
  *out = nullptr;
  if (!weights || n_weights <= 0) { g_create_err = "no weight table"; return IVG_ERR_MISSING; }
  static const int idx[13] = {0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28}, slice[13] = {1, 1, 2, 2, 3, 3, 3, 4, 4, 4, 5, 5, 5};
  static const int cin[13] = {3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512}, cout[13] = {64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512};
  static const int tapc[5] = {64, 128, 256, 512, 512};
  int status = IVG_OK;
  auto find = [&](const std::string& name, int64_t numel) -> const float* {
    for (int i = 0; i < n_weights; ++i) {
      if (!weights[i].name || name != weights[i].name) continue;
      int64_t n = 1;
      for (int d = 0; d < weights[i].ndim; ++d) n *= weights[i].shape[d];
      if (weights[i].dtype != IVG_F32 || n != numel || !weights[i].data || ((uintptr_t)weights[i].data & 15)) {
        if (status == IVG_OK) { status = IVG_ERR_INVALID; g_create_err = "LPIPS weight tensor '" + name + "': expected " + std::to_string(numel) + " float32 elements, 16-byte aligned"; }
        return nullptr;
      }
      return (const float*)weights[i].data;
    }
    if (status == IVG_OK) { status = IVG_ERR_MISSING; g_create_err = "missing LPIPS weight tensor '" + name + "'"; }
    return nullptr;
  };
  ivg_lpips h;
  h.device = device;
  for (int l = 0; l < 13; ++l) {
    const std::string n = "net.slice" + std::to_string(slice[l]) + "." + std::to_string(idx[l]);
    h.cw[l] = find(n + ".weight", (int64_t)cout[l] * 9 * cin[l]);
    h.cb[l] = find(n + ".bias", cout[l]);
  }
  for (int k = 0; k < 5; ++k) h.lin[k] = find("lin" + std::to_string(k) + ".model.1.weight", tapc[k]);
  if (status != IVG_OK) return status;
  *out = new ivg_lpips(h);
  return IVG_OK;
}

void ivg_lpips_destroy(ivg_lpips* p) { delete p; }

size_t ivg_lpips_ws_bytes(int max_images_per_chunk, int H, int W) {
  return (max_images_per_chunk <= 0 || H <= 0 || W <= 0) ? 0 : lpips_ws_bytes(max_images_per_chunk, H, W);
}

static int lpips_status(int rc) { return rc == 0 ? IVG_OK : (rc == -4 ? IVG_ERR_CAPACITY : IVG_ERR_HIP); }

int ivg_lpips_rows(ivg_lpips* p, const void* gt, int gt_dtype, int B, int T_gt, int gt_t0, const float* pred, int n_samples, int T_pr, int pr_t0, int T,
                   int H, int W, float* frames_out, float* rows_out, void* ws, size_t ws_bytes, ivg_stream stream) {
  if (!p || !gt || !pred || !rows_out || !ws || (gt_dtype != IVG_F32 && gt_dtype != IVG_BF16)) return IVG_ERR_INVALID;
  if (B <= 0 || n_samples <= 0 || n_samples % B != 0 || T <= 0 || gt_t0 < 0 || pr_t0 < 0 || gt_t0 + T > T_gt || pr_t0 + T > T_pr) return IVG_ERR_INVALID;
  if (!lpips_shape_ok(H, W)) return IVG_ERR_INVALID;
  float* frames = frames_out;
  if (!frames) {   // the per-frame values live at the end of the workspace
    const size_t need = ((size_t)n_samples * T * sizeof(float) + 255) & ~(size_t)255;
    if (ws_bytes < need + 256) return IVG_ERR_CAPACITY;
    ws_bytes -= need;
    frames = (float*)(((uintptr_t)ws + ws_bytes) & ~(uintptr_t)255);
    ws_bytes = (size_t)((char*)frames - (char*)ws);
  }
  if (lpips_ws_images(ws_bytes, H, W) < 2) return IVG_ERR_CAPACITY;
  return lpips_status(launch_lpips_rows(p->cw, p->cb, p->lin, gt, (DType)gt_dtype, B, T_gt, gt_t0, pred, n_samples, T_pr, pr_t0, T, H, W, frames, rows_out,
                                        ws, ws_bytes, (hipStream_t)stream));
}

int ivg_op_lpips_features(ivg_lpips* p, const void* images, int dtype, int n, int H, int W, float* const* taps_out, void* ws, size_t ws_bytes,
                          ivg_stream stream) {
  if (!p || !images || !taps_out || !ws || n <= 0 || (dtype != IVG_F32 && dtype != IVG_BF16) || !lpips_shape_ok(H, W)) return IVG_ERR_INVALID;
  if (lpips_ws_images(ws_bytes, H, W) < 1) return IVG_ERR_CAPACITY;
  return lpips_status(launch_lpips_features(p->cw, p->cb, images, (DType)dtype, n, H, W, taps_out, ws, ws_bytes, (hipStream_t)stream));
}

int ivg_op_lpips_head(const float* f0, const float* f1, const float* lin, int n0, int n1, int P, int C, float* out, void* ws, size_t ws_bytes,
                      ivg_stream stream) {
  if (!f0 || !f1 || !lin || !out || !ws || n0 <= 0 || n1 <= 0 || P <= 0 || (C != 64 && C != 128 && C != 256 && C != 512)) return IVG_ERR_INVALID;
  if (((uintptr_t)f0 & 15) || ((uintptr_t)f1 & 15) || ((uintptr_t)lin & 15) || ((uintptr_t)ws & 7)) return IVG_ERR_INVALID;
  if (ws_bytes < lpips_head_part_bytes(n1, P)) return IVG_ERR_CAPACITY;
  return lpips_status(launch_lpips_head(f0, f1, lin, n0, n1, P, C, out, n0, 0, (double*)ws, (hipStream_t)stream));
}

int ivg_op_lpips_conv_in(const void* images, int dtype, const float* w, const float* bias, float* Y, int n, int H, int W, ivg_stream stream) {
  if (!images || !w || !bias || !Y || n <= 0 || H <= 0 || W <= 0 || (dtype != IVG_F32 && dtype != IVG_BF16) || ((uintptr_t)Y & 15)) return IVG_ERR_INVALID;
  return lpips_status(launch_lpips_input_layer(images, (DType)dtype, w, bias, Y, n, H, W, (hipStream_t)stream));
}

int ivg_op_maxpool2(const float* X, float* Y, int N, int H, int W, int C, ivg_stream stream) {
  if (!X || !Y || N <= 0 || H < 2 || W < 2 || H % 2 || W % 2 || C <= 0 || C % 4 || ((uintptr_t)X & 15) || ((uintptr_t)Y & 15)) return IVG_ERR_INVALID;
  return lpips_status(launch_maxpool2(X, Y, N, H, W, C, (hipStream_t)stream));
}

// ---- I3D (i3d.hip): a handle owns the unit table built from the caller's weight tensors
struct ivg_i3d {
  I3dNet* net = nullptr;
};

int ivg_i3d_create(const ivg_tensor* weights, int n_weights, int device, int resize, ivg_i3d** out) {
  if (!out) return IVG_ERR_INVALID;
  *out = nullptr;
  if (!weights || n_weights <= 0) { g_create_err = "no weight table"; return IVG_ERR_MISSING; }
  if (resize < 0) { g_create_err = "I3D: resize must be 0 (off) or the side the frames are resized to"; return IVG_ERR_INVALID; }
  int status = IVG_OK;
  I3dNet* net = i3d_create(weights, n_weights, device, resize, &status);
  if (!net) return status;
  *out = new ivg_i3d{net};
  return IVG_OK;
}

void ivg_i3d_destroy(ivg_i3d* p) {
  if (p) i3d_destroy(p->net);
  delete p;
}

int ivg_i3d_units(ivg_i3d* p) { return p ? i3d_units(p->net) : IVG_ERR_INVALID; }

size_t ivg_i3d_ws_bytes(ivg_i3d* p, int max_clips, int T, int H, int W) { return p ? i3d_ws_bytes(p->net, max_clips, T, H, W) : 0; }

static int i3d_status(int rc) { return rc == 0 ? IVG_OK : (rc == -4 ? IVG_ERR_CAPACITY : (rc == -1 ? IVG_ERR_INVALID : IVG_ERR_HIP)); }

int ivg_i3d_features(ivg_i3d* p, const void* video, int dtype, int B, int T, int H, int W, float* features_out, void* ws, size_t ws_bytes,
                     ivg_stream stream) {
  if (!p || !video || !features_out || !ws || B <= 0 || (dtype != IVG_F32 && dtype != IVG_BF16)) return IVG_ERR_INVALID;
  if (i3d_check_shape(p->net, T, H, W)) return IVG_ERR_INVALID;
  if (ws_bytes < i3d_ws_bytes(p->net, 1, T, H, W)) return IVG_ERR_CAPACITY;
  return i3d_status(i3d_features(p->net, video, (DType)dtype, B, T, H, W, features_out, ws, ws_bytes, (hipStream_t)stream));
}

int ivg_op_i3d_tap(ivg_i3d* p, const void* video, int dtype, int B, int T, int H, int W, int unit_index, float* out, int64_t* dims_out, void* ws,
                   size_t ws_bytes, ivg_stream stream) {
  if (!p || B <= 0 || (dtype != IVG_F32 && dtype != IVG_BF16) || i3d_check_shape(p->net, T, H, W)) return IVG_ERR_INVALID;
  if (out && (!video || !ws)) return IVG_ERR_INVALID;
  if (out && ws_bytes < i3d_ws_bytes(p->net, 1, T, H, W)) return IVG_ERR_CAPACITY;
  return i3d_status(i3d_tap(p->net, video, (DType)dtype, B, T, H, W, unit_index, out, dims_out, ws, ws_bytes, (hipStream_t)stream));
}

int ivg_op_conv3d(const ivg_conv3d_args* a, ivg_stream stream) {
  if (!a) return IVG_ERR_INVALID;
  Conv3dArgs c{a->X, a->W, a->bias, a->Y, a->n, a->D, a->H, a->Wd, a->Cin, a->ldx, a->Do, a->Ho, a->Wo, {a->k[0], a->k[1], a->k[2]},
               {a->s[0], a->s[1], a->s[2]}, {a->p[0], a->p[1], a->p[2]}, a->Cout, a->ldy, a->coff, a->relu};
  const int rc = launch_conv3d(c, (hipStream_t)stream);
  return rc == 0 ? IVG_OK : (rc == (int)hipErrorInvalidValue ? IVG_ERR_INVALID : IVG_ERR_HIP);
}

int ivg_op_pool3d(const ivg_pool3d_args* a, ivg_stream stream) {
  if (!a) return IVG_ERR_INVALID;
  Pool3dArgs c{a->X, a->Y, a->n, a->D, a->H, a->Wd, a->C, a->ldx, a->Do, a->Ho, a->Wo, {a->k[0], a->k[1], a->k[2]}, {a->s[0], a->s[1], a->s[2]},
               {a->p[0], a->p[1], a->p[2]}, a->ldy, a->coff};
  const int rc = launch_pool3d(c, (hipStream_t)stream);
  return rc == 0 ? IVG_OK : (rc == (int)hipErrorInvalidValue ? IVG_ERR_INVALID : IVG_ERR_HIP);
}

int ivg_op_i3d_head(const float* X, const float* W, const float* bias, float* out, int n, int D, int P, int C, int Nout, void* ws, size_t ws_bytes,
                    ivg_stream stream) {
  if (!X || !W || !bias || !out || !ws || n <= 0 || D < 2 || P <= 0 || C <= 0 || Nout <= 0 || ((uintptr_t)ws & 3)) return IVG_ERR_INVALID;
  if (ws_bytes < i3d_head_ws_bytes(n, D, C)) return IVG_ERR_CAPACITY;
  return launch_i3d_head(X, W, bias, out, n, D, P, C, Nout, (float*)ws, (hipStream_t)stream) ? IVG_ERR_HIP : IVG_OK;
}

int ivg_op_i3d_ingest(const void* video, int dtype, int frames, int H, int W, int S, float* out, ivg_stream stream) {
  if (!video || !out || frames <= 0 || H <= 0 || W <= 0 || S <= 0 || (dtype != IVG_F32 && dtype != IVG_BF16)) return IVG_ERR_INVALID;
  return launch_i3d_ingest(video, (DType)dtype, out, frames, H, W, S, (hipStream_t)stream) ? IVG_ERR_HIP : IVG_OK;
}

int ivg_profile_attn_fit(ivg_engine* e, double* fixed_us, double* gbps) {
  if (!e || !fixed_us || !gbps) return IVG_ERR_INVALID;
  *fixed_us = e->attn_fit_fixed_us; *gbps = e->attn_fit_gbps;
  return IVG_OK;
}

int ivg_profile_enable(ivg_engine* e, int k, int enable) {
  if (!e || k < 0 || k >= IVG_K_COUNT) return IVG_ERR_INVALID;
  if (k == IVG_K_DECODE_ATTN) { e->attn_prof_on = enable != 0 && e->attn_prof; return IVG_OK; }
  if (k == IVG_K_DECODE_GEMM) {
    if (enable && !e->gemm_prof && e->cfg.num_layers > 0) {
      const size_t n = (size_t)(4 * e->cfg.num_layers + 1) * IVG_GEMM_PROF_SLOTS * 2 * e->Lmax * 8;
      API_CK(hipMalloc((void**)&e->gemm_prof, n));
      API_CK(hipMemset(e->gemm_prof, 0, n));
    }
    e->gemm_prof_on = enable != 0 && e->gemm_prof;
    return IVG_OK;
  }
  e->prof[k].enabled = enable != 0;
  return IVG_OK;
}

int ivg_profile_read(ivg_engine* e, int k, ivg_profile_stats* out) {
  if (!e || !out || k < 0 || k >= IVG_K_COUNT) return IVG_ERR_INVALID;
  API_CK(hipDeviceSynchronize());
  out->launches = 0; out->total_ms = 0; out->total_flops = 0; out->total_bytes = 0;
  if (k == IVG_K_DECODE_ATTN) {
    // launch windows stamped by the kernel itself (it runs inside a replayed hipGraph, where HIP events cannot bracket
    // single launches): last ivg_generate call only; bytes = K and V rows read per launch
    if (!e->attn_prof) return IVG_OK;
    const int L = e->Lmax, nl = e->cfg.num_layers, NS = IVG_ATTN_PROF_SLOTS;
    std::vector<unsigned long long> h((size_t)nl * NS * 2 * L);
    API_CK(hipMemcpy(h.data(), e->attn_prof, h.size() * 8, hipMemcpyDeviceToHost));
    // least-squares line  duration = fixed + bytes / rate  over the launches (they differ in cache length)
    double sn = 0, sx = 0, sy = 0, sxx = 0, sxy = 0;
    for (int l = 0; l < nl; ++l)
      for (int p = 0; p < L; ++p) {
        unsigned long long s = ~0ull, t = 0;
        for (int k = 0; k < NS; ++k) {
          const unsigned long long cs = h[((size_t)(l * NS + k) * 2) * L + p], ct = h[((size_t)(l * NS + k) * 2 + 1) * L + p];
          if (cs) s = std::min(s, ~cs);
          t = std::max(t, ct);
        }
        if (t == 0 || s == ~0ull || t < s) continue;
        const double ms = (double)(t - s) * 1e-5;   // 100 MHz wall clock -> ms
        const double bytes = 2.0 * e->attn_prof_B * e->heads * (double)(p + 1) * e->hd * (double)e->kvc.profiled_elem_bytes();
        out->launches++;
        out->total_ms += ms;
        out->total_bytes += bytes;
        out->total_flops += 4.0 * e->attn_prof_B * e->heads * (double)(p + 1) * e->hd;
        sn += 1; sx += bytes; sy += ms; sxx += bytes * bytes; sxy += bytes * ms;
      }
    const double den = sn * sxx - sx * sx;
    e->attn_fit_fixed_us = 0; e->attn_fit_gbps = 0;
    if (sn > 2 && den > 0) {
      const double slope = (sn * sxy - sx * sy) / den;            // ms per byte
      e->attn_fit_fixed_us = (sy - slope * sx) / sn * 1e3;
      e->attn_fit_gbps = slope > 0 ? 1e-6 / slope : 0;             // bytes/ms -> GB/s
    }
    return IVG_OK;
  }
  if (k == IVG_K_DECODE_GEMM) {
    // launch windows stamped by the GEMM kernels of the last ivg_generate call; bytes = the weight matrix a launch streams
    if (!e->gemm_prof) return IVG_OK;
    const int L = e->Lmax, nl = e->cfg.num_layers, NS = IVG_GEMM_PROF_SLOTS, ng = 4 * nl + 1;
    const double H = e->cfg.hidden_size, I = e->cfg.intermediate_size, V = e->cfg.vocab_size, es = (double)dtype_size(e->llm_dt);
    const double wbytes[5] = {3 * H * H * es, H * H * es, 2 * I * H * es, H * I * es, V * H * es};
    std::vector<unsigned long long> h((size_t)ng * NS * 2 * L);
    API_CK(hipMemcpy(h.data(), e->gemm_prof, h.size() * 8, hipMemcpyDeviceToHost));
    for (int i = 0; i < 5; ++i) { e->gemm_kind_ms[i] = 0; e->gemm_kind_n[i] = 0; }
    for (int g = 0; g < ng; ++g)
      for (int p = 0; p < L; ++p) {
        unsigned long long s = ~0ull, t = 0;
        for (int q = 0; q < NS; ++q) {
          const unsigned long long cs = h[((size_t)(g * NS + q) * 2) * L + p], ct = h[((size_t)(g * NS + q) * 2 + 1) * L + p];
          if (cs) s = std::min(s, ~cs);
          t = std::max(t, ct);
        }
        if (t == 0 || s == ~0ull || t < s) continue;
        const double wb = g == 4 * nl ? wbytes[4] : wbytes[g & 3];
        out->launches++;
        out->total_ms += (double)(t - s) * 1e-5;
        e->gemm_kind_ms[g == 4 * nl ? 4 : (g & 3)] += (double)(t - s) * 1e-5;
        e->gemm_kind_n[g == 4 * nl ? 4 : (g & 3)] += 1;
        out->total_bytes += wb;
        out->total_flops += wb / es * 2.0 * e->gemm_prof_B;
      }
    return IVG_OK;
  }
  ProfClass& pc = e->prof[k];
  for (auto& s : pc.used) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, s.a, s.b) == hipSuccess) { out->launches++; out->total_ms += ms; out->total_flops += s.flops; out->total_bytes += s.bytes; }
    pc.pool.push_back(s);
  }
  pc.used.clear();
  return IVG_OK;
}

int ivg_profile_gemm_kinds(ivg_engine* e, double* mean_us, int64_t* launches) {
  if (!e || !mean_us || !launches) return IVG_ERR_INVALID;
  for (int i = 0; i < 5; ++i) { launches[i] = e->gemm_kind_n[i]; mean_us[i] = e->gemm_kind_n[i] ? 1e3 * e->gemm_kind_ms[i] / (double)e->gemm_kind_n[i] : 0.0; }
  return IVG_OK;
}

// ---------------------------------------------------------------------------------------------- op-level hooks
int ivg_op_igemm(const ivg_igemm_args* a, int dtype, ivg_stream stream) {
  IgemmArgs g;
  igemm_op_args(g, a);
  g.nb0 = a->nb0; g.nb1 = a->nb1; g.nb2 = a->nb2;
  for (int i = 0; i < 3; ++i) { g.sa[i] = a->sa[i]; g.sw[i] = a->sw[i]; g.sy[i] = a->sy[i]; }
  if (dtype == IVG_F32X3) { g.x3 = true; dtype = IVG_F32; }   // fp32 tensors, split-bf16 arithmetic: what Run::gemm sets for an x3 engine
  if (g.KH == 3 && g.KW == 3 && g.stride == 1 && !g.x3) {  // same dispatch as the engine: LDS-halo kernel first
    const int rc = launch_conv3x3(g, (DType)dtype, (hipStream_t)stream);
    if (rc == 0) return IVG_OK;
    if (rc > 0) return IVG_ERR_HIP;
  }
  {  // large dense GEMMs: the 256 x 256-tile kernel first, as the engine does
    const int rc = launch_gemm256(g, (DType)dtype, (hipStream_t)stream);
    if (rc == 0) return IVG_OK;
    if (rc > 0) return IVG_ERR_HIP;
  }
  return launch_igemm(g, (DType)dtype, (hipStream_t)stream) ? IVG_ERR_HIP : IVG_OK;
}

int ivg_op_conv_gn(const ivg_igemm_args* a, int dtype, void* gn_part, int groups, const float* gamma, const float* beta, void* gn_out, float eps,
                   int silu, ivg_stream stream) {
  // unit-test hook of the fused path: 3x3 convolution whose epilogue reduces the GroupNorm statistics of its output, followed by
  // the apply-only GroupNorm that consumes them.  Returns the number of statistics chunks per image (> 0) or a negative status.
  IgemmArgs g;
  igemm_op_args(g, a);
  g.gn_part = gn_part; g.gn_groups = groups;
  const int rc = launch_conv3x3(g, (DType)dtype, (hipStream_t)stream);
  if (rc != 0 || g.gn_chunks <= 0) return rc > 0 ? IVG_ERR_HIP : IVG_ERR_INVALID;
  if (launch_groupnorm_apply(a->Y, gn_out, gn_part, g.gn_chunks, gamma, beta, nullptr, a->Nimg, a->Hout * a->Wout, a->N, groups, eps, silu,
                             (DType)dtype, (hipStream_t)stream))
    return IVG_ERR_HIP;
  return g.gn_chunks;
}

int ivg_op_conv_subpixel(const ivg_igemm_args* a, int dtype, const void* w_sub, const void* w_x3, const void* w_sub_x3, void* gn_part, int groups,
                         ivg_stream stream) {
  // unit-test hook: the nearest-x2 upsampling convolution in sub-pixel form (a->ups must be 1; a->W = the plain [N][9 Cin] matrix,
  // unused unless the shape falls back).  w_x3 / w_sub_x3 != NULL: split-bf16 arithmetic on fp32 tensors.  gn_part != NULL: output
  // statistics from the epilogue; returns the chunks per image then (0 without), IVG_ERR_INVALID when the sub-pixel kernel did not run.
  if (!a->ups || !w_sub) return IVG_ERR_INVALID;
  IgemmArgs g;
  igemm_op_args(g, a);
  g.W_sub = w_sub; g.W_x3 = w_x3; g.W_sub_x3 = w_sub_x3;
  g.gn_part = gn_part; g.gn_groups = groups;
  const long long before = conv3x3_subpixel_launches();
  const int rc = launch_conv3x3(g, (DType)dtype, (hipStream_t)stream);
  if (rc != 0) return rc > 0 ? IVG_ERR_HIP : IVG_ERR_INVALID;
  if (conv3x3_subpixel_launches() == before) return IVG_ERR_INVALID;
  return gn_part ? g.gn_chunks : 0;
}

int ivg_op_xattn(const void* q, const void* Kp, const void* VpT, void* out, int M, int F, int P, int kv, int C, int nh, int dtype, ivg_stream stream) {
  const int rc = launch_xattn(q, Kp, VpT, out, M, F, P, kv, C, nh, (DType)dtype, (hipStream_t)stream);
  return rc == 0 ? IVG_OK : (rc > 0 ? IVG_ERR_HIP : IVG_ERR_INVALID);
}

int ivg_op_gn_conv(const ivg_igemm_args* a, int dtype, int groups, const float* gamma, const float* beta, float eps, void* ws, ivg_stream stream) {
  // unit-test hook: y = conv3x3(silu(GroupNorm(x))) with the normalisation applied inside the convolution's input staging.
  // ws: scratch of at least Nimg * (ceil(H*W/1024) * groups * 16 + Cin * 8) bytes.  Returns IVG_ERR_INVALID when the fused kernel
  // does not cover the shape.
  IgemmArgs g;
  igemm_op_args(g, a);
  const int P = a->Hin * a->Win, nch = gn_num_chunks(P);
  char* part = (char*)ws;
  char* coef = part + (size_t)a->Nimg * nch * groups * 16;
  if (launch_groupnorm_partial(a->X, part, a->Nimg, P, a->Cin, groups, (DType)dtype, (hipStream_t)stream)) return IVG_ERR_HIP;
  if (launch_gn_coef(part, nch, gamma, beta, a->Nimg, P, a->Cin, groups, eps, coef, (hipStream_t)stream)) return IVG_ERR_HIP;
  g.gn_in_coef = coef;
  const int rc = launch_conv3x3(g, (DType)dtype, (hipStream_t)stream);
  return rc == 0 ? IVG_OK : (rc > 0 ? IVG_ERR_HIP : IVG_ERR_INVALID);
}

int ivg_op_conv_x3(const ivg_igemm_args* a, const void* w_x3, int groups, const float* gamma, const float* beta, float eps, void* ws, ivg_stream stream) {
  // unit-test hook of the split-bf16 3x3 convolution (fp32 tensors, weights pre-split by packing.py pack_x3); gamma != NULL: with
  // GroupNorm + SiLU of the input applied (and the result split) inside the staging, ws as in ivg_op_gn_conv
  IgemmArgs g;
  igemm_op_args(g, a);
  g.W_x3 = w_x3;
  if (!w_x3) return IVG_ERR_INVALID;
  if (gamma) {
    const int P = a->Hin * a->Win, nch = gn_num_chunks(P);
    char* part = (char*)ws;
    char* coef = part + (size_t)a->Nimg * nch * groups * 16;
    if (launch_groupnorm_partial(a->X, part, a->Nimg, P, a->Cin, groups, F32, (hipStream_t)stream)) return IVG_ERR_HIP;
    if (launch_gn_coef(part, nch, gamma, beta, a->Nimg, P, a->Cin, groups, eps, coef, (hipStream_t)stream)) return IVG_ERR_HIP;
    g.gn_in_coef = coef;
  }
  const int rc = launch_conv3x3(g, F32, (hipStream_t)stream);
  return rc == 0 ? IVG_OK : (rc > 0 ? IVG_ERR_HIP : IVG_ERR_INVALID);
}

static bool conv3x3_op_args(IgemmArgs& g, DType& dt, const ivg_igemm_args* a, int dtype, const void* w_x3, const void* w_sub, const void* w_sub_x3) {
  if (!a || (dtype != IVG_F32 && dtype != IVG_BF16 && dtype != IVG_F32X3)) return false;
  if (dtype == IVG_F32X3 && !w_x3) return false;
  igemm_op_args(g, a);
  g.nb0 = a->nb0; g.nb1 = a->nb1; g.nb2 = a->nb2;
  g.W_x3 = w_x3; g.W_sub = w_sub; g.W_sub_x3 = w_sub_x3;
  dt = dtype == IVG_BF16 ? BF16 : F32;
  return true;
}

int ivg_op_conv3x3(const ivg_igemm_args* a, int dtype, const float* gamma, const float* beta, int in_groups, float eps, void* ws,
                   const void* in_part, int in_chunks, void* gn_part, int groups, const void* w_x3, const void* w_sub, const void* w_sub_x3,
                   ivg_stream stream) {
  // unit-test hook: ONE launch_conv3x3 with every option a production launch combines (Run::norm_conv / Run::resnet); no fall-back
  IgemmArgs g;
  DType dt;
  if (!conv3x3_op_args(g, dt, a, dtype, w_x3, w_sub, w_sub_x3)) return IVG_ERR_INVALID;
  g.gn_part = gn_part; g.gn_groups = groups;
  char* coef = nullptr;
  const int P = a->Hin * a->Win;
  if (gamma) {
    if (!beta || !ws || in_groups <= 0 || a->Cin % in_groups != 0 || P <= 0 || a->Nimg <= 0 || (in_part && in_chunks <= 0)) return IVG_ERR_INVALID;
    coef = (char*)ws + (size_t)a->Nimg * gn_num_chunks(P) * in_groups * 16;
    g.gn_in_coef = coef;
  }
  if (conv3x3_plan(g, dt).covered != 1) return IVG_ERR_INVALID;   // before the statistics kernels write the workspace
  if (gamma) {
    const void* part = in_part;
    int nch = in_chunks;
    if (!part) {
      if (launch_groupnorm_partial(a->X, ws, a->Nimg, P, a->Cin, in_groups, dt, (hipStream_t)stream)) return IVG_ERR_HIP;
      part = ws; nch = gn_num_chunks(P);
    }
    if (launch_gn_coef(part, nch, gamma, beta, a->Nimg, P, a->Cin, in_groups, eps, coef, (hipStream_t)stream)) return IVG_ERR_HIP;
  }
  const int rc = launch_conv3x3(g, dt, (hipStream_t)stream);
  if (rc != 0) return rc > 0 ? IVG_ERR_HIP : IVG_ERR_INVALID;
  return g.gn_chunks;
}

int ivg_op_conv3x3_plan(const ivg_igemm_args* a, int dtype, int gn_in, int gn_groups, const void* w_x3, const void* w_sub,
                        const void* w_sub_x3, int32_t* out) {
  IgemmArgs g;
  DType dt;
  if (!out || !conv3x3_op_args(g, dt, a, dtype, w_x3, w_sub, w_sub_x3)) return IVG_ERR_INVALID;
  if (gn_in) g.gn_in_coef = (const void*)out;        // (only its presence matters to the plan)
  if (gn_groups > 0) { g.gn_part = (void*)out; g.gn_groups = gn_groups; }
  const Conv3Plan p = conv3x3_plan(g, dt);
  const int32_t v[IVG_CONV3X3_PLAN_INTS] = {p.covered, p.kind, p.bn, p.tw, p.ups, p.gna, p.tpb2, p.subpix, p.tiles_x, p.tiles_per_img, p.tiles_n,
                                            p.chunks, p.staged, p.gn_chunks, p.lds_bytes};
  for (int i = 0; i < IVG_CONV3X3_PLAN_INTS; ++i) out[i] = v[i];
  return IVG_OK;
}

int64_t ivg_debug_counter(const char* name) {
  if (name && !strcmp(name, "conv3x3_subpixel")) return conv3x3_subpixel_launches();
  if (name && !strcmp(name, "gemm256x3")) return gemm256x3_launches();
  if (name && !strcmp(name, "decode_attn24")) return decode_attn24_launches();
  if (name && !strcmp(name, "decode_attn8")) return decode_attn8_launches();
  if (name && !strcmp(name, "decode_gemm_gen3")) return decode_gemm_launches(3);
  if (name && !strcmp(name, "decode_gemm_gen2")) return decode_gemm_launches(2);
  if (name && !strcmp(name, "lpips_trunk_images")) return lpips_trunk_images();
  if (name && !strcmp(name, "frame_heads")) return frame_heads_hits();
  if (name && !strcmp(name, "token_scores")) return token_scores_launches();
  if (name && !strcmp(name, "filtered_scores")) return filtered_scores_launches();
  if (name && !strcmp(name, "kv_select_direct")) return kv_select_rows(0);
  if (name && !strcmp(name, "kv_select_staged")) return kv_select_rows(1);
  if (name && !strcmp(name, "kv_snapshot_rows_saved")) return kv_snapshot_rows(0);
  if (name && !strcmp(name, "kv_snapshot_rows_restored")) return kv_snapshot_rows(1);
  if (name && !strcmp(name, "kv_extend_chunk_rows")) return kv_extend_rows(0);
  if (name && !strcmp(name, "kv_extend_step_rows")) return kv_extend_rows(1);
  if (name && !strcmp(name, "kv_extend_frame_rows")) return kv_extend_heads_rows(0);
  if (name && !strcmp(name, "kv_extend_scored_rows")) return kv_extend_heads_rows(1);
  if (name && !strcmp(name, "enc_plain_images")) return enc_counter(0);
  if (name && !strcmp(name, "enc_cond_images")) return enc_counter(1);
  if (name && !strcmp(name, "enc_kv_projections")) return enc_counter(2);
  return -1;
}

int ivg_op_skinny(const void* X, const void* W, void* Y, int M, int N, int K, int ldx, int ldw, int ldy, int flags, int dtype, ivg_stream stream) {
  return ivg_op_skinny_policy(X, W, Y, M, N, K, ldx, ldw, ldy, flags, dtype, 0, 0, stream);
}

// dtype IVG_F32X3: fp32 tensors with SkinnyArgs::x3 (split-bf16 arithmetic where dgemm3.hip covers the shape), as Run::gemm sets it
static bool skinny_op_args(SkinnyArgs& s, DType& dt, int M, int N, int K, int ldx, int ldw, int ldy, int flags, int dtype, int lds_kb) {
  if (dtype != IVG_F32 && dtype != IVG_BF16 && dtype != IVG_F32X3) return false;
  if (lds_kb != 0 && (lds_kb < 16 || lds_kb > 160)) return false;
  s.M = M; s.N = N; s.K = K; s.ldx = ldx; s.ldw = ldw; s.ldy = ldy; s.flags = flags; s.lds_kb = lds_kb;
  s.x3 = dtype == IVG_F32X3;
  dt = dtype == IVG_BF16 ? BF16 : F32;
  return true;
}

int ivg_op_skinny_policy(const void* X, const void* W, void* Y, int M, int N, int K, int ldx, int ldw, int ldy, int flags, int dtype, int lds_kb,
                         int w_shared, ivg_stream stream) {
  SkinnyArgs s;
  DType dt;
  if (!skinny_op_args(s, dt, M, N, K, ldx, ldw, ldy, flags, dtype, lds_kb)) return IVG_ERR_INVALID;
  s.X = X; s.W = W; s.Y = Y; s.w_shared = w_shared != 0;
  return launch_skinny(s, dt, (hipStream_t)stream) ? IVG_ERR_HIP : IVG_OK;
}

int ivg_op_skinny_plan(int M, int N, int K, int ldx, int ldw, int ldy, int flags, int dtype, int lds_kb, const void* X, const void* W,
                       const void* Y, int32_t* out) {
  SkinnyArgs s;
  DType dt;
  if (!out || !skinny_op_args(s, dt, M, N, K, ldx, ldw, ldy, flags, dtype, lds_kb)) return IVG_ERR_INVALID;
  s.X = X; s.W = W; s.Y = (void*)Y;
  const SkinnyPlan p = skinny_plan(s, dt);
  const int32_t v[IVG_SKINNY_PLAN_INTS] = {p.gen, p.mf, p.fn, p.waves, p.klw, p.ring, p.lg, p.nburst, p.wmax, p.wr, p.x3};
  for (int i = 0; i < IVG_SKINNY_PLAN_INTS; ++i) out[i] = v[i];
  return IVG_OK;
}

int ivg_op_groupnorm(const void* X, void* Y, void* ws, const float* gamma, const float* beta, const float* pos, int N, int P, int C, int groups,
                     float eps, int silu, int dtype, ivg_stream stream) {
  return launch_groupnorm(X, Y, ws, gamma, beta, pos, N, P, C, groups, eps, silu, (DType)dtype, (hipStream_t)stream) ? IVG_ERR_HIP : IVG_OK;
}

int ivg_op_softmax(const float* S, void* P, int64_t rows, int Lq, int Lk, int lds, int ldp, int causal, int dtype, ivg_stream stream) {
  return launch_softmax(S, P, rows, Lq, Lk, lds, ldp, causal, (DType)dtype, (hipStream_t)stream) ? IVG_ERR_HIP : IVG_OK;
}

int ivg_op_vq_argmin(const float* z, const float* codebook, float* ee_ws, int64_t* out, int R, int n_e, ivg_stream stream) {
  if (launch_sqnorm_rows(codebook, ee_ws, n_e, 64, (hipStream_t)stream)) return IVG_ERR_HIP;
  TokMap mp{1, 1, 1, 0, 1};  // identity: row r -> out[r]
  return launch_vq_argmin(z, codebook, ee_ws, out, mp, 0, R, n_e, (hipStream_t)stream) ? IVG_ERR_HIP : IVG_OK;
}

int ivg_op_add_rmsnorm(void* x, const float* w, void* out, int M, int H, float eps, int dtype, ivg_stream stream) {
  return launch_add_rmsnorm(x, H, w, out, M, H, eps, (DType)dtype, (hipStream_t)stream) ? IVG_ERR_HIP : IVG_OK;
}

int ivg_op_conv_in(const void* video, int video_dtype, const float* w, const float* bias, void* Y, int dtype, int N, int per, int T_total, int t0,
                   int H, int W, int C0, ivg_stream stream) {
  return launch_conv_in(video, (DType)video_dtype, w, bias, Y, (DType)dtype, N, per, T_total, t0, H, W, C0, (hipStream_t)stream) ? IVG_ERR_HIP : IVG_OK;
}

int ivg_op_shared_decode_attn(const void* qkv, void* kc, void* vc, void* out, const float* cos_t, const float* sin_t, int B, int heads, int hd, int Lmax,
                              int pos, int P, int G, int row0, int dtype, ivg_stream stream) {
  // unit-test hook of one decode-attention step of a shared-context rollout (decode_attn_kernel SHARED)
  if (B <= 0 || heads <= 0 || G < 1 || P < 0 || P > pos || pos >= Lmax || row0 > 0) return IVG_ERR_INVALID;
  // a head dim the kernel has no instance for is refused here, before anything is allocated or launched
  if ((dtype != IVG_F32 && dtype != IVG_BF16) || !decode_attn_covers(hd, (DType)dtype)) return IVG_ERR_INVALID;
  return one_step(pos, stream, [&](StepState* state, hipStream_t st) {
    return launch_decode_attn(qkv, kc, vc, out, cos_t, sin_t, B, heads, hd, Lmax, state, nullptr, (DType)dtype, st, P, G, row0); });
}

int ivg_op_prefill_attn(void* qkv, void* kc, void* vc, void* vt, void* out, const float* cos_t, const float* sin_t, int B, int L, int heads,
                        int hd, int Lmax, int dtype, ivg_stream stream) {
  // unit-test hook of one prefill layer's attention: rope_kv (q in place, K / V appended at positions [0, L), V^T with pitch
  // rup(L, 64)) then, with out, flash_prefill_kernel -- what Run::prefill launches per layer
  if (B <= 0 || heads <= 0 || L < 1 || L > Lmax || hd <= 0 || hd % 2 || (dtype != IVG_F32 && dtype != IVG_BF16)) return IVG_ERR_INVALID;
  // the one-pass kernel covers bf16 at head_dim 64 and loads / stores in 16- / 8-byte vectors: refused before anything is written
  if (out && (dtype != IVG_BF16 || hd != 64 || !vt || ((uintptr_t)qkv & 15) || ((uintptr_t)out & 7))) return IVG_ERR_INVALID;
  const int Lp = (L + 63) / 64 * 64;
  hipStream_t st = (hipStream_t)stream;
  int rc = launch_rope_kv(qkv, kc, vc, vt, Lp, cos_t, sin_t, B, L, heads, hd, Lmax, nullptr, 0, (DType)dtype, st);
  if (rc == 0 && out) rc = launch_flash_prefill(qkv, kc, vt, out, B, L, Lp, heads, hd, Lmax, (DType)dtype, st);
  return rc == 0 ? IVG_OK : (rc > 0 ? IVG_ERR_HIP : IVG_ERR_INVALID);
}

int ivg_op_chunk_attn(void* qkv, void* kc, void* vc, void* out, const float* cos_t, const float* sin_t, int B, int T, int heads, int hd, int Lmax,
                      int pos0, int dtype, ivg_stream stream) {
  // unit-test hook of one layer's attention in ivg_kv_extend's chunk pass: rope_kv at pos0 (q in place, K / V appended at positions
  // [pos0, pos0 + T), no V^T) then chunk_attn_kernel -- what Run::prefill launches per layer in append mode.  Everything it does not
  // cover is refused before anything is written
  if (dtype != IVG_BF16 || hd != 64 || B <= 0 || heads <= 0 || T < 1 || pos0 < 0 || (long)pos0 + T > Lmax) return IVG_ERR_INVALID;
  if (((uintptr_t)qkv & 15) || ((uintptr_t)out & 7) || ((uintptr_t)kc & 15) || ((uintptr_t)vc & 15)) return IVG_ERR_INVALID;
  hipStream_t st = (hipStream_t)stream;
  int rc = launch_rope_kv(qkv, kc, vc, nullptr, 0, cos_t, sin_t, B, T, heads, hd, Lmax, nullptr, pos0, BF16, st);
  if (rc == 0) rc = launch_chunk_attn(qkv, kc, vc, out, B, T, heads, hd, Lmax, pos0, BF16, st);
  return rc == 0 ? IVG_OK : (rc > 0 ? IVG_ERR_HIP : IVG_ERR_INVALID);
}

int ivg_op_kv24_pack(const float* k32, const float* v32, void* kc, void* vc, int BH, int L, int Lmax, ivg_stream stream) {
  if (BH <= 0 || L < 0 || L > Lmax) return IVG_ERR_INVALID;
  return launch_kv24_pack(k32, v32, kc, vc, BH, L, Lmax, (hipStream_t)stream) ? IVG_ERR_HIP : IVG_OK;
}

int ivg_op_decode_attn24(const float* qkv, void* kc, void* vc, float* out, const float* cos_t, const float* sin_t, int B, int heads, int Lmax, int pos,
                         int P, int G, int row0, ivg_stream stream) {
  // unit-test hook of one decode-attention step over the 24-bit K / V cache of the x3 rollout (decode_attn24_kernel; G > 1: SHARED)
  if (B <= 0 || G < 1 || P < 0 || P > pos || pos >= Lmax || row0 > 0) return IVG_ERR_INVALID;
  return one_step(pos, stream, [&](StepState* state, hipStream_t st) {
    return launch_decode_attn24(qkv, kc, vc, out, cos_t, sin_t, B, heads, Lmax, state, nullptr, st, P, G, row0); });
}

int ivg_op_kv8_pack(const void* k16, const void* v16, void* kc, void* vc, int BH, int L, int Lmax, float k_scale, float v_scale, ivg_stream stream) {
  if (BH <= 0 || L < 0 || L > Lmax || !kv8_scale_ok(k_scale) || !kv8_scale_ok(v_scale)) return IVG_ERR_INVALID;
  return launch_kv8_pack(k16, v16, kc, vc, BH, L, Lmax, k_scale, v_scale, (hipStream_t)stream) ? IVG_ERR_HIP : IVG_OK;
}

int ivg_op_decode_attn8(const void* qkv, void* kc, void* vc, void* out, const float* cos_t, const float* sin_t, int B, int heads, int Lmax, int pos,
                        int P, int G, int row0, float k_scale, float v_scale, ivg_stream stream) {
  // unit-test hook of one decode-attention step over the FP8 K / V cache of a bf16 rollout (decode_attn8_kernel; G > 1: SHARED)
  if (B <= 0 || heads <= 0 || G < 1 || P < 0 || P > pos || pos >= Lmax || row0 > 0) return IVG_ERR_INVALID;
  if (!kv8_scale_ok(k_scale) || !kv8_scale_ok(v_scale)) return IVG_ERR_INVALID;
  return one_step(pos, stream, [&](StepState* state, hipStream_t st) {
    return launch_decode_attn8(qkv, kc, vc, out, cos_t, sin_t, B, heads, Lmax, state, nullptr, k_scale, v_scale, st, P, G, row0); });
}

// the [heads] tables of a test hook are device memory: read back (after the stream's earlier work) and checked as ivg_set_kv_scales checks
static bool op_scales_ok(const float* k_scales, const float* v_scales, int heads, hipStream_t st) {
  if (!k_scales || !v_scales || heads <= 0) return false;
  std::vector<float> h(2 * (size_t)heads);
  if (hipStreamSynchronize(st) != hipSuccess) return false;
  if (hipMemcpy(h.data(), k_scales, heads * 4, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(h.data() + heads, v_scales, heads * 4, hipMemcpyDeviceToHost) != hipSuccess) return false;
  for (float f : h) if (!kv8_scale_ok(f)) return false;
  return true;
}

int ivg_op_kv8_pack_heads(const void* k16, const void* v16, void* kc, void* vc, int B, int heads, int L, int Lmax, const float* k_scales, const float* v_scales,
                          ivg_stream stream) {
  if (B <= 0 || heads <= 0 || L < 0 || L > Lmax || !op_scales_ok(k_scales, v_scales, heads, (hipStream_t)stream)) return IVG_ERR_INVALID;
  return launch_kv8_pack(k16, v16, kc, vc, B * heads, L, Lmax, 1.0f, 1.0f, (hipStream_t)stream, heads, k_scales, v_scales) ? IVG_ERR_HIP : IVG_OK;
}

int ivg_op_decode_attn8_heads(const void* qkv, void* kc, void* vc, void* out, const float* cos_t, const float* sin_t, int B, int heads, int Lmax, int pos,
                              int P, int G, int row0, const float* k_scales, const float* v_scales, ivg_stream stream) {
  if (B <= 0 || heads <= 0 || G < 1 || P < 0 || P > pos || pos >= Lmax || row0 > 0) return IVG_ERR_INVALID;
  if (!op_scales_ok(k_scales, v_scales, heads, (hipStream_t)stream)) return IVG_ERR_INVALID;
  return one_step(pos, stream, [&](StepState* state, hipStream_t st) {
    return launch_decode_attn8(qkv, kc, vc, out, cos_t, sin_t, B, heads, Lmax, state, nullptr, 1.0f, 1.0f, st, P, G, row0, k_scales, v_scales); });
}

int ivg_op_kv_absmax(const void* k16, const void* v16, int B, int heads, int L, int Lmax, uint32_t* out, ivg_stream stream) {
  if (!k16 || !v16 || !out || B <= 0 || heads <= 0 || L < 0 || L > Lmax) return IVG_ERR_INVALID;
  return launch_kv_absmax(k16, v16, B, heads, L, Lmax, out, (hipStream_t)stream) ? IVG_ERR_HIP : IVG_OK;
}

int ivg_op_kv_select(void* base, int layers, int chunk, int heads, int Lmax, int row_bytes_a, int row_bytes_b, int len, int B_old, const int32_t* parents,
                     int n, void* scratch, size_t scratch_bytes, ivg_stream stream) {
  if (!base || layers <= 0 || heads <= 0 || Lmax <= 0 || row_bytes_a <= 0 || row_bytes_b < 0 || row_bytes_a % 16 || row_bytes_b % 16 || len < 1 || len > Lmax)
    return IVG_ERR_INVALID;
  KvSelectPlan plan;
  const int prc = kv_select_plan(parents, n, B_old, chunk, &plan);
  if (prc != KV_PLAN_OK) return prc == KV_PLAN_CAPACITY ? IVG_ERR_CAPACITY : IVG_ERR_INVALID;
  KvSelectBuf b;   // [layers][2][chunk][heads]{[Lmax] rows of row_bytes_a | [Lmax] rows of row_bytes_b}
  b.base = (char*)base; b.slabs = layers * 2; b.heads = heads;
  b.head_stride = (long)Lmax * (row_bytes_a + row_bytes_b); b.row_stride = heads * b.head_stride; b.slab_stride = chunk * b.row_stride;
  b.bytes_a = (long)len * row_bytes_a; b.bytes_b = (long)len * row_bytes_b; b.plane_b = (long)Lmax * row_bytes_a;
  const int rc = launch_kv_select(b, plan, scratch, scratch_bytes, (hipStream_t)stream);
  if (rc == 0) kv_select_note(plan.n_direct, plan.n_staged);
  return rc == 0 ? IVG_OK : (rc == -4 ? IVG_ERR_CAPACITY : IVG_ERR_HIP);
}

int ivg_op_kv_snapshot(void* base, int layers, int chunk, int heads, int Lmax, int row_bytes_a, int row_bytes_b, int len, int B, void* dense,
                       size_t dense_bytes, const int32_t* parents, int n, int direction, ivg_stream stream) {
  if (!base || !dense || layers <= 0 || heads <= 0 || Lmax <= 0 || row_bytes_a <= 0 || row_bytes_b < 0 || row_bytes_a % 16 || row_bytes_b % 16 || len < 1 ||
      len > Lmax || chunk <= 0 || chunk > KV_SELECT_MAX_ROWS || B <= 0 || B > chunk || (direction != 0 && direction != 1))
    return IVG_ERR_INVALID;
  if (direction == 1) {
    if (!parents || n <= 0) return IVG_ERR_INVALID;
    if (n > chunk) return IVG_ERR_CAPACITY;
    for (int i = 0; i < n; ++i)
      if (parents[i] < 0 || parents[i] >= B) return IVG_ERR_INVALID;
  }
  KvSelectBuf b;   // [layers][2][chunk][heads]{[Lmax] rows of row_bytes_a | [Lmax] rows of row_bytes_b}
  b.base = (char*)base; b.slabs = layers * 2; b.heads = heads;
  b.head_stride = (long)Lmax * (row_bytes_a + row_bytes_b); b.row_stride = heads * b.head_stride; b.slab_stride = chunk * b.row_stride;
  b.bytes_a = (long)len * row_bytes_a; b.bytes_b = (long)len * row_bytes_b; b.plane_b = (long)Lmax * row_bytes_a;
  if ((size_t)b.slabs * B * heads * (size_t)(b.bytes_a + b.bytes_b) > dense_bytes) return IVG_ERR_CAPACITY;
  const int rc = launch_kv_snapshot(b, dense, B, parents, direction ? n : B, direction == 1, (hipStream_t)stream);
  if (rc == 0) kv_snapshot_note(direction ? 0 : B, direction ? n : 0);
  return rc == 0 ? IVG_OK : IVG_ERR_HIP;
}

int ivg_op_sample(const float* logits, int B, int V, int top_k, float temperature, const float* uniforms, int64_t* out, ivg_stream stream) {
  return ivg_op_sample_top_p(logits, B, V, top_k, temperature, 1.0f /* SampleArgs' default: no nucleus filter */, uniforms, out, stream);
}

int ivg_op_sample_top_p(const float* logits, int B, int V, int top_k, float temperature, float top_p, const float* uniforms, int64_t* out,
                        ivg_stream stream) {
  if (!(temperature > 0.0f) || !std::isfinite(temperature)) return IVG_ERR_INVALID;   // as ivg_set_temperature
  if (!(top_p >= 0.0f && top_p <= 1.0f)) return IVG_ERR_INVALID;                       // as ivg_set_top_p
  // one draw per row through the rollout's sampler kernel (token j = 1 of a prompt of length 0; no embedding: H = 0)
  return one_step(0, stream, [&](StepState* state, hipStream_t st) {
    SampleArgs sa{};
    sa.logits = logits; sa.V = V; sa.uniforms = uniforms; sa.n_uni = 1; sa.top_k = top_k;
    sa.ids_out = out; sa.ids_stride = 1; sa.L0 = 0; sa.forced_period = 0; sa.forced_token = 0;
    sa.E = logits; sa.x = out; sa.H = 0; sa.act = nullptr; sa.act_T = 0; sa.ctx = 1; sa.slot0 = 0; sa.state = state;
    sa.temperature = temperature;
    sa.top_p = top_p;
    return launch_sample_embed(sa, B, F32, st);
  });
}

int ivg_op_token_scores(const float* logits, const int64_t* ids, int B, int V, float* out, ivg_stream stream) {
  if (!logits || !ids || !out || B <= 0 || V < 1 || V > 256 * 72) return IVG_ERR_INVALID;
  // the rollout's score kernel on given rows and ids: new token j = 1 of a prompt of length 0, no forced schedule, one column
  return one_step(0, stream, [&](StepState* state, hipStream_t st) { return launch_token_scores(logits, V, state, ids, 1, 0, 0, out, 1, B, st); });
}

int ivg_op_filtered_scores(const float* logits, const int64_t* ids, int B, int V, int top_k, float temperature, float top_p, int greedy, float* out,
                           ivg_stream stream) {
  if (!logits || !ids || !out || B <= 0 || V < 1 || V > 256 * 72) return IVG_ERR_INVALID;
  if (!(temperature > 0.0f) || !std::isfinite(temperature)) return IVG_ERR_INVALID;   // as ivg_set_temperature
  if (!(top_p >= 0.0f && top_p <= 1.0f)) return IVG_ERR_INVALID;                       // as ivg_set_top_p
  // the rollout's kernel on given rows and ids: new token j = 1 of a prompt of length 0, no forced schedule, one column
  return one_step(0, stream, [&](StepState* state, hipStream_t st) {
    return launch_filtered_scores(logits, V, state, ids, 1, 0, 0, top_k, temperature, top_p, greedy != 0, out, 1, B, st);
  });
}

int ivg_op_token_scores_rows(const float* logits, const int64_t* ids, int64_t ids_stride, int64_t row0, int rows, int Tc, int V, int first_forced,
                             int period, float* out, int64_t out_ld, ivg_stream stream) {
  if (!logits || !ids || !out || rows <= 0 || Tc < 1 || row0 < 0 || V < 1 || V > 256 * 72 || first_forced < 0 || period < 0) return IVG_ERR_INVALID;
  return launch_token_scores_rows(logits, ids, (long)ids_stride, (long)row0, rows, Tc, V, first_forced, period, out, (long)out_ld, (hipStream_t)stream) == 0
             ? IVG_OK : IVG_ERR_HIP;
}

}  // extern "C"
