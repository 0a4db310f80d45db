// Layer graphs of the compressive tokenizer on the hand-written kernels.
//
// Follows (structure only; all arithmetic is in the .hip kernels):
//   Encoder.forward            ivideogpt/vq_model/vae.py:141-195
//   ConditionalEncoder.forward ivideogpt/vq_model/conditional_vae.py:108-132
//   Decoder.forward            ivideogpt/vq_model/vae.py:298-371
//   ConditionalDecoder.forward ivideogpt/vq_model/conditional_vae.py:186-212
//   CrossAttentionBlock        ivideogpt/vq_model/conditional_vae.py:38-55
//   tokenize / detokenize      ivideogpt/vq_model/compressive_vq_model.py:164-277
// MI355X-first differences from the reference's op sequence (results identical):
//   * activations live in NHWC, so a feature map already IS the [tokens, C] matrix attention needs;
//   * context features are never repeated F times (compressive_vq_model.py:176-187, 257-266): the
//     cross-attention K / V projections are computed once per trajectory and shared by its F frames
//     through batch strides of 0;
//   * nearest-x2 upsampling, the stride-2 right/bottom zero pad and 4x4 patchify are index arithmetic
//     inside the implicit-GEMM gather, never materialised.
#include <atomic>

#include "engine_impl.h"
#include "switches.h"

namespace ivg {

#define CK(x) do { int _e = (x); if (_e != 0) return R.e->fail(IVG_ERR_HIP, std::string(#x) + " failed: hip error " + std::to_string(_e)); } while (0)

static size_t esz(DType d) { return d == BF16 ? 2 : 4; }

// -------------------------------------------------------------------------------------------- primitive wrappers
size_t Run::gn_stats_bytes(int N, int H, int W, int C) const {
  return (size_t)N * conv3x3_gn_chunks_bound(H, W, C) * e->cfg.norm_num_groups * sizeof(double) * 2;
}

int Run::conv(DType dt, const void* X, int N, int H, int W, const ConvW& c, void* Y, int stride, int ups, const void* Rres, int flags,
              int out_f32, GnStats* out_stats, const void* in_coef) {
  Run& R = *this;
  if (out_stats) out_stats->chunks = 0;
  const int k = c.k;
  int Ho, Wo, pad;
  if (ups) { Ho = 2 * H; Wo = 2 * W; pad = 1; }
  else if (stride == 2) { Ho = H / 2; Wo = W / 2; pad = 0; }       // F.pad(0,1,0,1) + stride-2 conv, padding 0
  else if (stride == k && k > 1) { Ho = H / k; Wo = W / k; pad = 0; }  // patchify conv (quant_linear)
  else { Ho = H; Wo = W; pad = (k - 1) / 2; }
  IgemmArgs a;
  a.X = X; a.W = c.w; a.Y = Y; a.R = Rres; a.bias = c.b;
  a.Nimg = N; a.Hin = H; a.Win = W; a.Cin = c.cin; a.ldx = c.cin; a.Hout = Ho; a.Wout = Wo;
  a.KH = k; a.KW = k; a.stride = stride; a.pad = pad; a.ups = ups;
  a.N = c.cout; a.ldw = k * k * c.cin;
  a.c_img = (long)Ho * Wo * c.cout; a.c_pix = c.cout; a.c_ch = 1;
  a.flags = flags | (c.b ? IG_BIAS_N : 0) | (Rres ? IG_RESIDUAL : 0) | (out_f32 ? IG_OUT_F32 : 0);
  if (planning) return 0;
  if (out_stats && out_stats->part) { a.gn_part = out_stats->part; a.gn_groups = e->cfg.norm_num_groups; }
  a.gn_in_coef = in_coef;
  if (dt == F32 && x3 && sw().x3) { a.x3 = true; a.W_x3 = c.w3; }   // split-bf16 arithmetic (IVG_F32X3 decode; IVG_X3=0: f32-input MFMAs)
  if (ups) { a.W_sub = c.wsub; a.W_sub_x3 = a.W_x3 ? c.wsub3 : nullptr; }   // upsampling convolutions in sub-pixel form (conv3x3.hip SUBPIX)
  const double flops = 2.0 * N * Ho * Wo * (double)c.cout * k * k * c.cin;
  const double bytes = (double)esz(dt) * ((double)N * H * W * c.cin + (double)c.cout * k * k * c.cin) + (double)(out_f32 ? 4 : esz(dt)) * N * Ho * Wo * c.cout;
  if (k == 3 && stride == 1) {  // FLOP majority: LDS-halo kernel; shapes it does not cover fall through to the implicit GEMM
    prof_begin(dt, flops, bytes, 2);
    const int rc = launch_conv3x3(a, dt, st);
    if (rc == 0) { prof_end(dt, 2); if (out_stats) out_stats->chunks = a.gn_chunks; return 0; }
    prof_cancel(dt, 2);
    if (rc > 0) CK(rc);
  }
  if (in_coef) return -100;   // only the 3x3 kernel can normalise its input on the fly: the caller materialises the GroupNorm instead
  prof_begin(dt, flops, bytes);
  int rc = -1;
  // 1x1 shortcuts with Cout a multiple of 256 (32 x 32 level: 512 -> 256 over 917,504 pixels): a plain GEMM -- 256 x 256 tiles with
  // whole-line LDS-DMA instead of the implicit GEMM's 128 x 128 gather (7-16 % MFMA-busy there, round-4 review)
  if (k == 1 && stride == 1 && !ups) rc = launch_gemm256(a, dt, st);
  if (rc == -1) rc = launch_igemm(a, dt, st);
  CK(rc);
  prof_end(dt);
  return 0;
}

int Run::gemm(DType dt, const IgemmArgs& a0, double flops, double bytes) {
  Run& R = *this;
  if (planning) return 0;
  IgemmArgs a = a0;
  a.x3 = dt == F32 && x3 && sw().x3;
  prof_begin(dt, flops, bytes);
  int rc = launch_gemm256(a, dt, st);   // large dense GEMMs (prompt pass); -1 = not covered
  if (rc == -1) rc = launch_igemm(a, dt, st);
  CK(rc);
  prof_end(dt);
  return 0;
}

int Run::linear(DType dt, const void* X, long rows, const ConvW& c, void* Y, const void* Rres, int flags, int out_f32) {
  // rows x cin  ->  rows x cout, all dense row-major
  IgemmArgs a;
  a.X = X; a.W = c.w; a.Y = Y; a.R = Rres; a.bias = c.b;
  a.Nimg = 1; a.Hin = 1; a.Win = (int)rows; a.Cin = c.cin; a.ldx = c.cin; a.Hout = 1; a.Wout = (int)rows;
  a.N = c.cout; a.ldw = c.cin;
  a.c_img = 0; a.c_pix = c.cout; a.c_ch = 1;
  a.flags = flags | (c.b ? IG_BIAS_N : 0) | (Rres ? IG_RESIDUAL : 0) | (out_f32 ? IG_OUT_F32 : 0);
  return gemm(dt, a, 2.0 * rows * c.cin * (double)c.cout,
              (double)esz(dt) * ((double)rows * c.cin + (double)c.cout * c.cin) + (double)(out_f32 ? 4 : esz(dt)) * rows * c.cout);
}

int Run::gnorm(DType dt, const void* X, void* Y, int N, int P, int C, const NormW& n, float eps, int silu, const float* pos,
               const GnStats* stats) {
  Run& R = *this;
  const int groups = e->cfg.norm_num_groups;
  if (stats && stats->part && stats->chunks > 0 && !planning) {   // the producer's epilogue already reduced the statistics
    CK(launch_groupnorm_apply(X, Y, stats->part, stats->chunks, n.g, n.b, pos, N, P, C, groups, eps, silu, dt, st));
    return 0;
  }
  const size_t m = e->ws.mark();
  void* part = e->ws.alloc((size_t)N * gn_num_chunks(P) * groups * sizeof(double) * 2);
  int rc = 0;
  if (!planning) rc = launch_groupnorm(X, Y, part, n.g, n.b, pos, N, P, C, groups, eps, silu, dt, st);
  e->ws.reset(m);  // stream-ordered: the next user of this scratch runs after these kernels
  CK(rc);
  return 0;
}

// GroupNorm + SiLU applied inside the conv3x3 input staging instead of a separate apply pass (the normalised tensor never exists
// in HBM; tests/test_gpu_ops.py::test_conv3x3_with_fused_input_groupnorm).  With the round-1 conv3x3 loop, whose vector pipe was
// already the busier one, this cost more than the apply pass it removed (decode 65.5 vs 63.0 ms,
// profiles/r02_eager_vs_graph_and_gn_fusion.txt); with the rebuilt loop (2 vector instructions per step) it wins: 214.0 vs 216.2 ms
// per step (encode -1.1, decode -1.0; profiles/r02_gn_apply_fusion_ab.txt).  IVG_GN_APPLY_FUSE=0: separate apply pass (A/B).
static bool gn_apply_fuse_enabled() { return sw().gn_apply_fuse != 0; }

int Run::norm_conv(DType dt, const void* x, int N, int H, int W, const NormW& n, float eps, const GnStats* x_stats, const ConvW& c, void* Y,
                   const void* Rres, void* scratch, GnStats* out_stats) {
  Run& R = *this;
  const int groups = e->cfg.norm_num_groups, P = H * W, C = c.cin;
  const size_t m = e->ws.mark();
  void* part = e->ws.alloc((size_t)N * gn_num_chunks(P) * groups * sizeof(double) * 2);
  void* coef = e->ws.alloc((size_t)N * C * sizeof(float) * 2);
  int rc = 0;
  if (!planning) {
    // (every N tile of the fused kernel normalises the whole input halo again; fusing only where a convolution has one or two N
    // tiles measured within the run-to-run spread in round 3, so it is fused wherever the 3x3 kernel covers the shape)
    const bool fuse = gn_apply_fuse_enabled() && c.k == 3;
    const void* st_part = x_stats && x_stats->chunks > 0 ? x_stats->part : nullptr;
    int chunks = st_part ? x_stats->chunks : 0;
    if (!st_part) {   // x has no statistics from its producer: one pass over it
      CK(launch_groupnorm_partial(x, part, N, P, C, groups, dt, st));
      st_part = part; chunks = gn_num_chunks(P);
    }
    rc = -100;
    if (fuse) {
      CK(launch_gn_coef(st_part, chunks, n.g, n.b, N, P, C, groups, eps, coef, st));
      rc = conv(dt, x, N, H, W, c, Y, 1, 0, Rres, 0, 0, out_stats, coef);
    }
    if (rc == -100) {   // not covered by the fused kernel: materialise silu(GroupNorm(x)), then convolve
      CK(launch_groupnorm_apply(x, scratch, st_part, chunks, n.g, n.b, nullptr, N, P, C, groups, eps, 1, dt, st));
      rc = conv(dt, scratch, N, H, W, c, Y, 1, 0, Rres, 0, 0, out_stats);
    }
  } else if (out_stats) {
    out_stats->chunks = 0;
  }
  e->ws.reset(m);
  return rc;
}

// x [N,H,W,cin] -> out [N,H,W,cout]
int Run::resnet(DType dt, const void* x, int N, int H, int W, const ResnetW& r, void* out, const GnStats* x_stats, GnStats* out_stats) {
  Run& R = *this;
  const size_t m = e->ws.mark();
  const size_t px = (size_t)N * H * W;
  void* t = e->ws.alloc(px * std::max(r.cin, r.cout) * esz(dt));
  void* h = e->ws.alloc(px * r.cout * esz(dt));
  GnStats hs;   // statistics of h for norm2, reduced by conv1's epilogue (h is read once less)
  hs.part = e->ws.alloc(gn_stats_bytes(N, H, W, r.cout));
  // h = conv1(silu(norm1(x)));  out = conv2(silu(norm2(h))) + shortcut(x): both GroupNorms are applied inside the convolutions'
  // input staging (t is only touched when a shape falls back to the implicit GEMM)
  IVG_TRY(norm_conv(dt, x, N, H, W, r.n1, 1e-6f, x_stats, r.c1, h, nullptr, t, &hs));
  const void* res = x;
  if (r.has_sc) {
    IVG_TRY(conv(dt, x, N, H, W, r.sc, out, 1, 0, nullptr, 0, 0));
    res = out;  // in-place residual: every element is read then written by the same thread
  }
  IVG_TRY(norm_conv(dt, h, N, H, W, r.n2, 1e-6f, &hs, r.c2, out, res, t, out_stats));
  e->ws.reset(m);
  return 0;
}

// diffusers Attention with one head of dim C: x [N, P tokens, C] -> out
int Run::self_attention(DType dt, const void* x, int N, int P, int C, const AttnW& a, void* out) {
  Run& R = *this;
  const size_t m = e->ws.mark();
  const size_t tok = (size_t)N * P;
  void* t = e->ws.alloc(tok * C * esz(dt));
  void* q = e->ws.alloc(tok * C * esz(dt));
  void* k = e->ws.alloc(tok * C * esz(dt));
  void* vT = e->ws.alloc(tok * C * esz(dt));
  void* o = e->ws.alloc(tok * C * esz(dt));
  // one pass (bf16: xattn_kernel with one head of C channels, every frame attending to itself) -- no score matrix in HBM; the
  // predicate is pure (shape, dtype), so the planning walk skips the score workspaces as well
  const bool fused = xattn_covers(P, P, C, 1, dt);
  float* S = fused ? nullptr : (float*)e->ws.alloc((size_t)N * P * P * sizeof(float));
  void* Pm = fused ? nullptr : e->ws.alloc((size_t)N * P * P * esz(dt));
  IVG_TRY(gnorm(dt, x, t, N, P, C, a.gn, 1e-6f, 0, nullptr));
  IVG_TRY(linear(dt, t, tok, a.q, q, nullptr, 0, 0));
  IVG_TRY(linear(dt, t, tok, a.k, k, nullptr, 0, 0));
  {  // V^T[n][c][tok] = Wv[c][:] . t[n][tok][:] + bv[c]
    IgemmArgs g;
    g.X = a.v.w; g.W = t; g.Y = vT; g.bias = a.v.b;
    g.Nimg = 1; g.Hin = 1; g.Win = C; g.Cin = C; g.ldx = C; g.Hout = 1; g.Wout = C;
    g.N = P; g.ldw = C; g.c_pix = P; g.c_ch = 1;
    g.flags = IG_BIAS_M;
    g.nb0 = N; g.sa[0] = 0; g.sw[0] = (long)P * C; g.sy[0] = (long)C * P;
    IVG_TRY(gemm(dt, g, 2.0 * tok * C * (double)C, (double)esz(dt) * (2.0 * tok * C + (double)C * C)));
  }
  if (fused) {
    if (!planning) {
      const int rc = launch_xattn(q, k, vT, o, N, 1, P, P, C, 1, dt, st);
      if (rc != 0) return e->fail(IVG_ERR_HIP, "one-pass self-attention launch failed: " + std::to_string(rc));
    }
  } else {
  {  // S = Q K^T / sqrt(C)
    IgemmArgs g;
    g.X = q; g.W = k; g.Y = S;
    g.Nimg = 1; g.Hin = 1; g.Win = P; g.Cin = C; g.ldx = C; g.Hout = 1; g.Wout = P;
    g.N = P; g.ldw = C; g.c_pix = P; g.c_ch = 1; g.flags = IG_OUT_F32; g.alpha = 1.0f / sqrtf((float)C);
    g.nb0 = N; g.sa[0] = (long)P * C; g.sw[0] = (long)P * C; g.sy[0] = (long)P * P;
    IVG_TRY(gemm(dt, g, 2.0 * N * (double)P * P * C, (double)esz(dt) * 2.0 * tok * C + 4.0 * N * P * P));
  }
  if (!planning) CK(launch_softmax(S, Pm, (long)N * P, P, P, P, P, 0, dt, st));
  {  // O = P V
    IgemmArgs g;
    g.X = Pm; g.W = vT; g.Y = o;
    g.Nimg = 1; g.Hin = 1; g.Win = P; g.Cin = P; g.ldx = P; g.Hout = 1; g.Wout = P;
    g.N = C; g.ldw = P; g.c_pix = C; g.c_ch = 1;
    g.nb0 = N; g.sa[0] = (long)P * P; g.sw[0] = (long)C * P; g.sy[0] = (long)P * C;
    IVG_TRY(gemm(dt, g, 2.0 * N * (double)P * P * C, (double)esz(dt) * ((double)N * P * P + 2.0 * tok * C)));
  }
  }
  IVG_TRY(linear(dt, o, tok, a.o, out, x, 0, 0));
  e->ws.reset(m);
  return 0;
}

// Per-trajectory K / V^T projections of the context feature (once per trajectory, shared by its F frames).
// feat [B][ctx*side*side][C] (NHWC frames of one trajectory are contiguous) -> Kp [B][kv][C], VpT [B][C][kv]
int Run::xatt_project_kv(DType dt, const void* feat, int B, const XAttW& x, void* Kp, void* VpT) {
  Run& R = *this;
  const int C = x.C, kv = e->ctx * x.side * x.side;
  const size_t m = e->ws.mark();
  void* kvn = e->ws.alloc((size_t)B * kv * C * esz(dt));
  const float* pos = x.kv_pos + (size_t)(x.kv_rows - kv) * C;  // set_context_length keeps the LAST k frames' rows
  IVG_TRY(gnorm(dt, feat, kvn, B, kv, C, x.kvn, 1e-5f, 0, pos));
  IVG_TRY(linear(dt, kvn, (long)B * kv, x.k, Kp, nullptr, 0, 0));
  IgemmArgs g;
  g.X = x.v.w; g.W = kvn; g.Y = VpT; g.bias = x.v.b;
  g.Nimg = 1; g.Hin = 1; g.Win = C; g.Cin = C; g.ldx = C; g.Hout = 1; g.Wout = C;
  g.N = kv; g.ldw = C; g.c_pix = kv; g.c_ch = 1; g.flags = IG_BIAS_M;
  g.nb0 = B; g.sa[0] = 0; g.sw[0] = (long)kv * C; g.sy[0] = (long)C * kv;
  IVG_TRY(gemm(dt, g, 2.0 * B * (double)kv * C * C, (double)esz(dt) * (2.0 * B * kv * C + (double)C * C)));
  e->ws.reset(m);
  return 0;
}

// z [B*F][P][C] (P = side^2 query tokens per frame) attends to its trajectory's context: out = silu(z + MHA(...))
int Run::cross_attention(DType dt, const void* z, int B, int F, const XAttW& x, const void* Kp, const void* VpT, void* out) {
  Run& R = *this;
  const int C = x.C, P = x.side * x.side, kv = e->ctx * P, nh = 4, hd = C / nh;
  const long M = (long)B * F;
  const size_t m = e->ws.mark();
  void* qn = e->ws.alloc((size_t)M * P * C * esz(dt));
  void* q = e->ws.alloc((size_t)M * P * C * esz(dt));
  void* o = e->ws.alloc((size_t)M * P * C * esz(dt));
  // one-pass attention kernel (bf16): no score matrix in HBM -- and, the predicate being pure (shape, dtype), none in the
  // workspace plan either (1.9 GB of S / P at config 2 were planned and never touched)
  const bool fused = xattn_covers(P, kv, C, nh, dt);
  float* S = fused ? nullptr : (float*)e->ws.alloc((size_t)M * nh * P * kv * sizeof(float));
  void* Pm = fused ? nullptr : e->ws.alloc((size_t)M * nh * P * kv * esz(dt));
  IVG_TRY(gnorm(dt, z, qn, (int)M, P, C, x.qn, 1e-5f, 0, x.q_pos));
  IVG_TRY(linear(dt, qn, M * P, x.q, q, nullptr, 0, 0));
  if (fused && !planning) {
    const int rc = launch_xattn(q, Kp, VpT, o, (int)M, F, P, kv, C, nh, dt, st);
    if (rc != 0) return e->fail(IVG_ERR_HIP, "one-pass cross-attention launch failed: " + std::to_string(rc));
  }
  if (!fused) {
  {  // S[b][f][h] = Q_h K_h^T / sqrt(hd)
    IgemmArgs g;
    g.X = q; g.W = Kp; g.Y = S;
    g.Nimg = 1; g.Hin = 1; g.Win = P; g.Cin = hd; g.ldx = C; g.Hout = 1; g.Wout = P;
    g.N = kv; g.ldw = C; g.c_pix = kv; g.c_ch = 1; g.flags = IG_OUT_F32; g.alpha = 1.0f / sqrtf((float)hd);
    g.nb0 = B; g.nb1 = F; g.nb2 = nh;
    g.sa[0] = (long)F * P * C; g.sa[1] = (long)P * C; g.sa[2] = hd;
    g.sw[0] = (long)kv * C; g.sw[1] = 0; g.sw[2] = hd;
    g.sy[0] = (long)F * nh * P * kv; g.sy[1] = (long)nh * P * kv; g.sy[2] = (long)P * kv;
    IVG_TRY(gemm(dt, g, 2.0 * M * nh * (double)P * kv * hd, (double)esz(dt) * (M * P * C + (double)B * kv * C) + 4.0 * M * nh * P * kv));
  }
  if (!planning) CK(launch_softmax(S, Pm, M * nh * P, P, kv, kv, kv, 0, dt, st));
  {  // O[b][f][:, h*hd..] = P V_h
    IgemmArgs g;
    g.X = Pm; g.W = VpT; g.Y = o;
    g.Nimg = 1; g.Hin = 1; g.Win = P; g.Cin = kv; g.ldx = kv; g.Hout = 1; g.Wout = P;
    g.N = hd; g.ldw = kv; g.c_pix = C; g.c_ch = 1;
    g.nb0 = B; g.nb1 = F; g.nb2 = nh;
    g.sa[0] = (long)F * nh * P * kv; g.sa[1] = (long)nh * P * kv; g.sa[2] = (long)P * kv;
    g.sw[0] = (long)C * kv; g.sw[1] = 0; g.sw[2] = (long)hd * kv;
    g.sy[0] = (long)F * P * C; g.sy[1] = (long)P * C; g.sy[2] = hd;
    IVG_TRY(gemm(dt, g, 2.0 * M * nh * (double)P * kv * hd, (double)esz(dt) * ((double)M * nh * P * kv + (double)B * kv * C + M * P * C)));
  }
  }
  IVG_TRY(linear(dt, o, M * P, x.o, out, z, IG_SILU, 0));
  e->ws.reset(m);
  return 0;
}

// -------------------------------------------------------------------------------------------- encoders
// Plain or conditional encoder trunk.  frames: images [N] = clip frames (t0 .. t0+per) of B trajectories.
// cond != null: conditional encoder, cross-attending to cond features (index = level + 1).
// keep != null: plain encoder; keep[i] (i = feature index) receives persistent copies of the features that
// a conditional pass will need.  latent: [N,16,16,latent] in dt.
static std::atomic<long long> g_enc_counter[3] = {{0}, {0}, {0}};
long long enc_counter(int which) { return g_enc_counter[which].load(std::memory_order_relaxed); }

int Run::encoder_trunk(const TrunkW& w, const void* pixels, DType pix_dt, int B, int per, int T_total, int t0,
                       std::vector<Feature>* keep, const std::vector<Feature>* cond, void* latent, const ivg_enc_cache* kept) {
  Run& R = *this;
  const bool xatt = cond || kept;
  if (!planning) g_enc_counter[xatt ? 1 : 0].fetch_add((long long)B * per, std::memory_order_relaxed);
  const DType dt = e->enc_dt;
  const ivg_config& c = e->cfg;
  const int N = B * per, nl = c.n_levels;
  int side = c.resolution;
  size_t max_el = 0;
  {
    int s = side;
    for (int i = 0; i < nl; ++i) {
      max_el = std::max(max_el, (size_t)s * s * c.block_out_channels[i]);
      if (i > 0) max_el = std::max(max_el, (size_t)s * s * c.block_out_channels[i - 1]);
      if (i != nl - 1) s /= 2;
    }
  }
  const size_t m = e->ws.mark();
  // cross-attention K/V of every site first (persist for the whole trunk)
  std::vector<void*> Kp, Vp;
  if (kept) {   // ... or those an earlier call kept (ivg_encode_context_cached): nothing is projected
    Kp = kept->Kp; Vp = kept->VpT;
    if (Kp.size() != w.xatt.size()) return e->fail(IVG_ERR_INVALID, "encoder cache layout mismatch");
  } else if (cond) {
    int s = side, k = 0;
    for (int i = 0; i < nl; ++i) {
      if (i != nl - 1) s /= 2;
      if (s <= c.max_att_resolution) {
        const XAttW& x = w.xatt[k++];
        const int kv = e->ctx * x.side * x.side;
        void* kp = e->ws.alloc((size_t)B * kv * x.C * esz(dt));
        void* vp = e->ws.alloc((size_t)B * kv * x.C * esz(dt));
        IVG_TRY(xatt_project_kv(dt, (*cond)[i + 1].p, B, x, kp, vp));
        if (!planning) g_enc_counter[2].fetch_add(1, std::memory_order_relaxed);
        Kp.push_back(kp); Vp.push_back(vp);
      }
    }
  }
  void* a = e->ws.alloc((size_t)N * max_el * esz(dt));
  void* b = e->ws.alloc((size_t)N * max_el * esz(dt));
  // GroupNorm statistics travel with the activation: a conv3x3 that produces a tensor also reduces its (sum, sum of squares) per
  // group, so the next block's first GroupNorm does not read the tensor once more just for that (sa / sb belong to a / b)
  size_t st_bytes = 0;
  {
    int s = side;
    for (int i = 0; i < nl; ++i) { st_bytes = std::max(st_bytes, gn_stats_bytes(N, s, s, c.block_out_channels[i])); if (i != nl - 1) s /= 2; }
  }
  GnStats sa, sb;
  sa.part = e->ws.alloc(st_bytes); sb.part = e->ws.alloc(st_bytes);
  if (!planning)
    CK(launch_conv_in(pixels, pix_dt, w.conv_in_raw_w, w.conv_in.b, a, dt, N, per, T_total, t0, side, side, c.block_out_channels[0], st));
  int k = 0;
  for (int i = 0; i < nl; ++i) {
    for (size_t j = 0; j < w.blocks[i].size(); ++j) {
      IVG_TRY(resnet(dt, a, N, side, side, w.blocks[i][j], b, &sa, &sb));
      std::swap(a, b); std::swap(sa, sb);
    }
    if (i != nl - 1) {
      IVG_TRY(conv(dt, a, N, side, side, w.resample[i], b, 2, 0, nullptr, 0, 0));
      std::swap(a, b); std::swap(sa, sb); sa.chunks = 0;   // (stride-2 conv: implicit GEMM, no statistics)
      side /= 2;
    }
    const int C = c.block_out_channels[i];
    if (xatt && side <= c.max_att_resolution) {
      IVG_TRY(cross_attention(dt, a, B, per, w.xatt[k], Kp[k], Vp[k], b));
      std::swap(a, b); std::swap(sa, sb); sa.chunks = 0;
      ++k;
    }
    if (keep && (*keep)[i + 1].p && !planning)
      CK((int)hipMemcpyAsync((*keep)[i + 1].p, a, (size_t)N * side * side * C * esz(dt), hipMemcpyDeviceToDevice, st));
  }
  const int C = c.block_out_channels[nl - 1];
  IVG_TRY(resnet(dt, a, N, side, side, w.mid0, b, &sa, &sb)); std::swap(a, b); std::swap(sa, sb);
  if (w.has_attn) { IVG_TRY(self_attention(dt, a, N, side * side, C, w.attn, b)); std::swap(a, b); std::swap(sa, sb); sa.chunks = 0; }
  IVG_TRY(resnet(dt, a, N, side, side, w.mid1, b, &sa, &sb)); std::swap(a, b); std::swap(sa, sb);
  IVG_TRY(gnorm(dt, a, b, N, side * side, C, w.norm_out, 1e-6f, 1, nullptr, &sa));
  IVG_TRY(conv(dt, b, N, side, side, w.conv_out, latent, 1, 0, nullptr, 0, 0));
  e->ws.reset(m);
  return 0;
}

// which encoder features the conditional encoder needs (index = level + 1), with their geometry
static void encoder_feature_plan(const ivg_config& c, std::vector<Feature>& f) {
  f.assign(c.n_levels + 2, Feature());
  int s = c.resolution;
  for (int i = 0; i < c.n_levels; ++i) {
    if (i != c.n_levels - 1) s /= 2;
    if (s <= c.max_att_resolution) { f[i + 1].side = s; f[i + 1].C = c.block_out_channels[i]; }
  }
}

int Run::tokenize(const void* pixels, DType pix_dt, int B, int T, int64_t* ids, int64_t ids_stride, int64_t* labels, bool ctx_only,
                  ivg_enc_cache* fill) {
  Run& R = *this;
  x3 = false;   // bit-exact ids: the exact fp32 chain, always
  const ivg_config& c = e->cfg;
  const DType dt = e->enc_dt;
  const int ctx = e->ctx, F = T - ctx, lat = c.latent_channels, dim = c.vq_embed_dim;
  const int64_t nvq = c.num_vq_embeddings, ndyn = c.num_dyn_embeddings;
  const size_t m = e->ws.mark();
  std::vector<Feature> feats;
  encoder_feature_plan(c, feats);
  const bool keep_feats = !ctx_only || fill;
  if (keep_feats)
    for (auto& f : feats)
      if (f.side) f.p = e->ws.alloc((size_t)B * ctx * f.side * f.side * f.C * esz(dt));
  const int N = B * ctx;
  void* h = e->ws.alloc((size_t)N * 256 * lat * esz(dt));
  IVG_TRY(encoder_trunk(e->enc, pixels, pix_dt, B, ctx, T, 0, keep_feats ? &feats : nullptr, nullptr, h));
  if (fill) {   // the conditional encoder's K / V projections of this context, per site (the order encoder_trunk projects them in)
    size_t k = 0;
    for (int i = 0; i < c.n_levels; ++i) {
      if (!feats[i + 1].side) continue;
      if (k >= e->cenc.xatt.size() || (!planning && k >= fill->Kp.size())) return e->fail(IVG_ERR_INVALID, "encode_context_cached: cache layout mismatch");
      IVG_TRY(xatt_project_kv(dt, feats[i + 1].p, B, e->cenc.xatt[k], planning ? nullptr : fill->Kp[k], planning ? nullptr : fill->VpT[k]));
      if (!planning) g_enc_counter[2].fetch_add(1, std::memory_order_relaxed);
      ++k;
    }
    if (!planning) { fill->filled = true; fill->ctx = ctx; }
  }
  float* hq = (float*)e->ws.alloc((size_t)N * 256 * dim * sizeof(float));
  IVG_TRY(conv(dt, h, N, 16, 16, e->quant_conv, hq, 1, 0, nullptr, 0, 1));
  if (!planning) {
    TokMap mp{256, ctx, ids_stride, 0, 257};
    CK(launch_vq_argmin(hq, e->cb_c, e->ee_c, ids, mp, 0, N * 256, (int)nvq, st));
  }
  int L = 257 * ctx;
  if (!ctx_only) {
    const int M = B * F;
    void* d = e->ws.alloc((size_t)M * 256 * lat * esz(dt));
    IVG_TRY(encoder_trunk(e->cenc, pixels, pix_dt, B, F, T, ctx, nullptr, &feats, d));
    float* dq = (float*)e->ws.alloc((size_t)M * 16 * dim * sizeof(float));
    IVG_TRY(conv(dt, d, M, 16, 16, e->quant_linear, dq, c.patch_size, 0, nullptr, 0, 1));  // 4x4 / stride-4 conv == patchify + Linear
    if (!planning) {
      TokMap mp{16, F, ids_stride, 257 * ctx, 17};
      CK(launch_vq_argmin(dq, e->cb_d, e->ee_d, ids, mp, nvq, M * 16, (int)ndyn, st));
    }
    L = 257 * ctx - 1 + 17 * F;
  }
  if (!planning) {
    if (ids_stride != L && labels) return e->fail(IVG_ERR_INVALID, "labels need a dense token matrix");
    CK(launch_finish_tokens(ids, ids_stride, labels, B, L, ctx, nvq + ndyn, nvq + ndyn + 1, st));
  }
  e->ws.reset(m);
  return 0;
}

// The dyn tokens of n observed frames per trajectory against a kept encoder context (ivg_tokenize_frames): the conditional trunk of
// tokenize over B * n frames with the cache's K / V projections -- no plain encoder, no projection.  frames (B, n, 3, H, W);
// ids columns 17 i + j (j < 16): dyn token j of frame i, column 17 i + 16: sdf.
int Run::tokenize_frames(const void* frames, DType pix_dt, int B, int n, const ivg_enc_cache* cache, int64_t* ids, int64_t ids_stride) {
  Run& R = *this;
  x3 = false;
  const ivg_config& c = e->cfg;
  const DType dt = e->enc_dt;
  const int lat = c.latent_channels, dim = c.vq_embed_dim, M = B * n;
  const int64_t nvq = c.num_vq_embeddings, ndyn = c.num_dyn_embeddings;
  const size_t m = e->ws.mark();
  void* d = e->ws.alloc((size_t)M * 256 * lat * esz(dt));
  IVG_TRY(encoder_trunk(e->cenc, frames, pix_dt, B, n, n, 0, nullptr, nullptr, d, cache));
  float* dq = (float*)e->ws.alloc((size_t)M * 16 * dim * sizeof(float));
  IVG_TRY(conv(dt, d, M, 16, 16, e->quant_linear, dq, c.patch_size, 0, nullptr, 0, 1));
  if (!planning) {
    TokMap mp{16, n, ids_stride, 0, 17};
    CK(launch_vq_argmin(dq, e->cb_d, e->ee_d, ids, mp, nvq, M * 16, (int)ndyn, st));
    CK(launch_sdf_columns(ids, ids_stride, B, n, nvq + ndyn + 1, st));
  }
  e->ws.reset(m);
  return 0;
}

// -------------------------------------------------------------------------------------------- decoders
static void decoder_feature_plan(const ivg_config& c, std::vector<Feature>& f) {
  // features: [conv_in out, mid out, each up level out]; the conditional decoder uses [1] and [i+2] where side <= max_att
  f.assign(c.n_levels + 2, Feature());
  const int nl = c.n_levels;
  int s = 16;
  f[1].side = 16; f[1].C = c.block_out_channels[nl - 1];
  for (int i = 0; i < nl; ++i) {
    if (i != nl - 1) s *= 2;
    if (s <= c.max_att_resolution) { f[i + 2].side = s; f[i + 2].C = c.block_out_channels[nl - 1 - i]; }
  }
}

// z [N,16,16,latent] -> pixels written (fp32, planar) into out_pixels frames (b, t0 + n % per)
int Run::decoder_trunk(const TrunkW& w, const void* z, int B, int per, int T_total, int t0, std::vector<Feature>* keep,
                       const std::vector<Feature>* cond, void* out_pixels, DType out_dt) {
  Run& R = *this;
  const DType dt = e->dec_dt;
  const ivg_config& c = e->cfg;
  const int N = B * per, nl = c.n_levels;
  const int res = c.resolution;
  size_t max_el = 0;
  {
    int s = 16;
    for (int i = 0; i < nl; ++i) {
      const int C = c.block_out_channels[nl - 1 - i];
      const int Cp = c.block_out_channels[nl - 1 - (i > 0 ? i - 1 : 0)];
      max_el = std::max(max_el, (size_t)s * s * std::max(C, Cp));
      if (i != nl - 1) { s *= 2; max_el = std::max(max_el, (size_t)s * s * C); }
    }
  }
  const size_t m = e->ws.mark();
  std::vector<void*> Kp, Vp;
  if (cond) {
    for (size_t k = 0; k < w.xatt.size(); ++k) {
      const XAttW& x = w.xatt[k];
      const int kv = e->ctx * x.side * x.side;
      void* kp = e->ws.alloc((size_t)B * kv * x.C * esz(dt));
      void* vp = e->ws.alloc((size_t)B * kv * x.C * esz(dt));
      // site 0 uses cond[1]; site k>0 belongs to the k-th up level whose output side <= max_att: cond[i+2]
      int fi = 1;
      if (k > 0) {
        int s = 16, seen = 0;
        for (int i = 0; i < nl; ++i) {
          if (i != nl - 1) s *= 2;
          if (s <= c.max_att_resolution) { ++seen; if (seen == (int)k) { fi = i + 2; break; } }
        }
      }
      IVG_TRY(xatt_project_kv(dt, (*cond)[fi].p, B / kv_group, x, kp, vp));   // (shared context: one K / V projection per GROUP)
      Kp.push_back(kp); Vp.push_back(vp);
    }
  }
  // cross-attention K / V addressing: frame n belongs to trajectory n / per; with kv_group trajectories sharing one context that is
  // context n / (per * kv_group) -- the same kernel with (B / kv_group) "trajectories" of (per * kv_group) frames
  const int Bk = B / kv_group, perk = per * kv_group;
  void* a = e->ws.alloc((size_t)N * max_el * esz(dt));
  void* b = e->ws.alloc((size_t)N * max_el * esz(dt));
  size_t st_bytes = 0;   // GroupNorm statistics travel with the activation (see encoder_trunk)
  {
    int s = 16;
    for (int i = 0; i < nl; ++i) {
      const int Cl = c.block_out_channels[nl - 1 - i];
      st_bytes = std::max(st_bytes, gn_stats_bytes(N, s, s, Cl));
      if (i != nl - 1) { s *= 2; st_bytes = std::max(st_bytes, gn_stats_bytes(N, s, s, Cl)); }
    }
  }
  GnStats sa, sb;
  sa.part = e->ws.alloc(st_bytes); sb.part = e->ws.alloc(st_bytes);
  int side = 16;
  const int Ctop = c.block_out_channels[nl - 1];
  IVG_TRY(conv(dt, z, N, side, side, w.conv_in, a, 1, 0, nullptr, 0, 0, &sa));
  IVG_TRY(resnet(dt, a, N, side, side, w.mid0, b, &sa, &sb)); std::swap(a, b); std::swap(sa, sb);
  if (w.has_attn) { IVG_TRY(self_attention(dt, a, N, side * side, Ctop, w.attn, b)); std::swap(a, b); std::swap(sa, sb); sa.chunks = 0; }
  IVG_TRY(resnet(dt, a, N, side, side, w.mid1, b, &sa, &sb)); std::swap(a, b); std::swap(sa, sb);
  if (keep && (*keep)[1].p && !planning)
    CK((int)hipMemcpyAsync((*keep)[1].p, a, (size_t)N * side * side * Ctop * esz(dt), hipMemcpyDeviceToDevice, st));
  int k = 0;
  if (cond) { IVG_TRY(cross_attention(dt, a, Bk, perk, w.xatt[0], Kp[0], Vp[0], b)); std::swap(a, b); std::swap(sa, sb); sa.chunks = 0; k = 1; }
  for (int i = 0; i < nl; ++i) {
    const int C = c.block_out_channels[nl - 1 - i];
    for (size_t j = 0; j < w.blocks[i].size(); ++j) {
      IVG_TRY(resnet(dt, a, N, side, side, w.blocks[i][j], b, &sa, &sb));
      std::swap(a, b); std::swap(sa, sb);
    }
    if (i != nl - 1) {
      IVG_TRY(conv(dt, a, N, side, side, w.resample[i], b, 1, 1, nullptr, 0, 0, &sb));  // nearest x2 folded into the gather
      std::swap(a, b); std::swap(sa, sb);
      side *= 2;
    }
    if (cond && side <= c.max_att_resolution) {
      IVG_TRY(cross_attention(dt, a, Bk, perk, w.xatt[k], Kp[k], Vp[k], b));
      std::swap(a, b); std::swap(sa, sb); sa.chunks = 0;
      ++k;
    }
    if (keep && (*keep)[i + 2].p && !planning)
      CK((int)hipMemcpyAsync((*keep)[i + 2].p, a, (size_t)N * side * side * C * esz(dt), hipMemcpyDeviceToDevice, st));
  }
  const int C0 = c.block_out_channels[0];
  {  // conv_norm_out -> SiLU -> conv_out straight into the planar (B, T, 3, H, W) clip: float32, or the decode path's own bfloat16
    const bool out32 = out_dt == F32;
    IgemmArgs g;
    g.W = w.conv_out.w; g.Y = (char*)out_pixels + (size_t)t0 * 3 * res * res * (out32 ? 4 : 2); g.bias = w.conv_out.b;
    g.Nimg = N; g.Hin = side; g.Win = side; g.Cin = C0; g.ldx = C0; g.Hout = side; g.Wout = side;
    g.KH = 3; g.KW = 3; g.stride = 1; g.pad = 1;
    g.N = 3; g.ldw = 9 * C0;
    g.c_img = 3L * res * res; g.c_pix = 1; g.c_ch = (long)res * res;
    g.c_grp = per; g.c_grp_stride = (long)T_total * 3 * res * res;
    g.flags = IG_BIAS_N | (out32 ? IG_OUT_F32 : 0) | (e->clamp_out ? IG_CLAMP01 : 0);   // clamp(0, 1) of predict.py:73 in the epilogue
    const double flops = 2.0 * N * side * side * 27.0 * C0;
    const double bytes = (double)esz(dt) * N * side * side * C0 + (out32 ? 4.0 : 2.0) * N * 3 * side * side;
    // Round 5: the tail as ONE launch -- the normalisation inside the 3x3 kernel's halo staging (its 64-channel instance computes 61
    // output channels nobody stores: still cheaper than a GroupNorm pass that writes the normalised tensor plus an implicit GEMM that
    // re-gathers it nine times; bf16 decode path with the producer's statistics at hand -- other modes keep the two launches)
    int rc = -1;
    if (dt == BF16 && !x3 && gn_apply_fuse_enabled() && sa.part && sa.chunks > 0 && !planning) {
      void* coef = e->ws.alloc((size_t)N * C0 * sizeof(float) * 2);
      CK(launch_gn_coef(sa.part, sa.chunks, w.norm_out.g, w.norm_out.b, N, side * side, C0, c.norm_num_groups, 1e-6f, coef, st));
      g.X = a; g.gn_in_coef = coef;
      prof_begin(dt, flops, bytes);   // (accounted with the class conv_out has always been in -- "GEMMs / convs other than the trunks' 3x3": 3 output
      rc = launch_conv3x3(g, dt, st); //  channels are memory-bound work, and the conv3x3 class stays the set of launches earlier rounds measured)
      if (rc == 0) prof_end(dt); else prof_cancel(dt);
      if (rc > 0) CK(rc);
    } else if (planning) {
      (void)e->ws.alloc((size_t)N * C0 * sizeof(float) * 2);
    }
    if (rc != 0) {
      IVG_TRY(gnorm(dt, a, b, N, side * side, C0, w.norm_out, 1e-6f, 1, nullptr, &sa));
      g.X = b; g.gn_in_coef = nullptr;
      IVG_TRY(gemm(dt, g, flops, bytes));
    }
  }
  e->ws.reset(m);
  return 0;
}

// group > 1 (ivg_detokenize_shared): rows [g * group, (g + 1) * group) of `ids` hold the SAME context tokens (the samples / candidate
// action sequences of one clip: predict.py:65-72, vp/ivideogpt_interface.py:155-202).  The context frames are then decoded once per
// GROUP (its first row's tokens) and copied to the group's other rows, the context decoder's features exist once per group, and the
// predicted frames' cross-attention reads its K / V projections per group -- the reference decodes and projects them per row
// (compressive_vq_model.py:236-266).
int Run::detokenize(const int64_t* ids, int B, int F, void* out_pixels, DType out_dt, ivg_cache* cache, int cache_mode, int group) {
  Run& R = *this;
  x3 = e->dec_x3;
  if (group < 1 || B % group != 0) return e->fail(IVG_ERR_INVALID, "detokenize: the batch is not a whole number of groups");
  if (group > 1 && cache) return e->fail(IVG_ERR_INVALID, "detokenize: a cache and a shared context cannot be combined");
  const int NG = B / group;   // contexts to decode
  if (out_dt != F32 && out_dt != e->dec_dt)
    return e->fail(IVG_ERR_INVALID, "detokenize: bfloat16 pixels are written by the bfloat16 decode path only (decode_dtype = IVG_BF16)");
  const size_t psz = out_dt == F32 ? 4 : 2;
  const ivg_config& c = e->cfg;
  const DType dt = e->dec_dt;
  const int ctx = e->ctx, T = ctx + F, lat = c.latent_channels, dim = c.vq_embed_dim, p = c.patch_size;
  const long L = 257L * ctx - 1 + 17L * F;
  const int res = c.resolution;
  const size_t m = e->ws.mark();
  std::vector<Feature> feats;
  decoder_feature_plan(c, feats);
  const bool use_cache = cache && cache_mode == 2;
  if (use_cache && (!cache->filled || cache->B != B)) return e->fail(IVG_ERR_INVALID, "detokenize: cache is empty or was made for another batch size");
  // the kept context frames are pixels as they were written at fill time: reusing them under the other clamp mode would hand back
  // clamped context frames beside raw predicted ones (or the reverse) -- refuse instead of mixing
  if (use_cache && cache->pix_dt != (int)out_dt)
    return e->fail(IVG_ERR_INVALID, "detokenize: cache holds context pixels of another element type than this call writes (fill it again)");
  if (use_cache && cache->clamped != e->clamp_out)
    return e->fail(IVG_ERR_INVALID, std::string("detokenize: cache was filled with clamp ") + (cache->clamped ? "on" : "off") +
                                        ", this call runs with clamp " + (e->clamp_out ? "on" : "off") + " (fill it again in this mode)");
  if (cache && cache_mode == 1 && cache->B != B)   // the fill writes B trajectories of features / pixels into buffers sized for cache->B
    return e->fail(IVG_ERR_INVALID, "detokenize: cache was created for " + std::to_string(cache->B) + " trajectories, this call has " + std::to_string(B));
  {
    size_t fi = 0;
    for (auto& f : feats) {
      if (!f.side) continue;
      const size_t bytes = (size_t)NG * ctx * f.side * f.side * f.C * esz(dt);
      if (cache && cache_mode) {
        if (!planning) {
          if (fi >= cache->feat.size()) return e->fail(IVG_ERR_INVALID, "detokenize: cache layout mismatch");
          f.p = cache->feat[fi];
        }
        ++fi;
      } else {
        f.p = e->ws.alloc(bytes);
      }
    }
  }
  if (!use_cache) {
    const int N = NG * ctx;
    void* qc = e->ws.alloc((size_t)N * 256 * dim * esz(dt));
    void* q2 = e->ws.alloc((size_t)N * 256 * lat * esz(dt));
    if (!planning) {
      TokMap mp{256, ctx, L * group, 0, 257};   // (the first row of every group)
      CK(launch_gather_rows(ids, mp, e->cb_c, qc, dt, N * 256, dim, 0, c.num_vq_embeddings, st));
    }
    IVG_TRY(conv(dt, qc, N, 16, 16, e->post_quant_conv, q2, 1, 0, nullptr, 0, 0));
    // (clip stride T * group: context g lands in output row g * group; the group's other rows get copies below)
    IVG_TRY(decoder_trunk(e->dec, q2, NG, ctx, T * group, 0, &feats, nullptr, out_pixels, out_dt));
    if (group > 1 && !planning) {
      const size_t clip = (size_t)T * 3 * res * res * psz, cpart = (size_t)ctx * 3 * res * res * psz;
      for (int k = 1; k < group; ++k)
        CK((int)hipMemcpy2DAsync((char*)out_pixels + (size_t)k * clip, clip * group, out_pixels, clip * group, cpart, NG, hipMemcpyDeviceToDevice, st));
    }
    if (cache && cache_mode == 1 && !planning) {
      // keep the decoded context frames: rows (b, t < ctx) of out_pixels
      CK((int)hipMemcpy2DAsync(cache->ctx_pixels, (size_t)ctx * 3 * res * res * psz, out_pixels, (size_t)T * 3 * res * res * psz,
                               (size_t)ctx * 3 * res * res * psz, B, hipMemcpyDeviceToDevice, st));
      cache->filled = true;
      cache->clamped = e->clamp_out;
      cache->pix_dt = (int)out_dt;
      cache->ctx = ctx;
    }
  } else if (!planning) {
    CK((int)hipMemcpy2DAsync(out_pixels, (size_t)T * 3 * res * res * psz, cache->ctx_pixels, (size_t)ctx * 3 * res * res * psz,
                             (size_t)ctx * 3 * res * res * psz, B, hipMemcpyDeviceToDevice, st));
  }
  if (F > 0) {
    const int M = B * F;
    void* qd = e->ws.alloc((size_t)M * 16 * dim * esz(dt));
    void* q2 = e->ws.alloc((size_t)M * 16 * p * p * lat * esz(dt));
    void* z = e->ws.alloc((size_t)M * 256 * lat * esz(dt));
    if (!planning) {
      TokMap mp{16, F, L, 257 * ctx, 17};
      CK(launch_gather_rows(ids, mp, e->cb_d, qd, dt, M * 16, dim, c.num_vq_embeddings, c.num_dyn_embeddings, st));
    }
    IVG_TRY(linear(dt, qd, (long)M * 16, e->post_quant_linear, q2, nullptr, 0, 0));
    if (!planning) CK(launch_unpatchify(q2, z, dt, M, 16 / p, lat, p, st));
    kv_group = group;
    const int rc = decoder_trunk(e->cdec, z, B, F, T, ctx, nullptr, &feats, out_pixels, out_dt);
    kv_group = 1;
    IVG_TRY(rc);
  }
  e->ws.reset(m);
  return 0;
}

}  // namespace ivg
