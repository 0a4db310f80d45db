// Host-side launchers of every hand-written kernel (all return hipError_t as int, 0 = ok).
#pragma once
#include "../../include/ivg.h"
#include "common.h"
#include "igemm.h"
#include "kv_select_plan.h"

namespace ivg {

// ---- norm.hip
int gn_num_chunks(int P);
// GroupNorm over [N][P][C] (stats per (n, group) over P*C/groups values), optional SiLU and position embedding
// pos[P][C] (fp32).  part_ws: N * gn_num_chunks(P) * groups double2 of scratch.
int launch_groupnorm(const void* X, void* Y, void* part_ws, const float* gamma, const float* beta, const float* pos,
                     int N, int P, int C, int groups, float eps, int silu, DType dt, hipStream_t st);
// the statistics half alone, and the (scale, shift) table [N][C] float2 the conv3x3 kernel applies to its input while staging it
int launch_groupnorm_partial(const void* X, void* part_ws, int N, int P, int C, int groups, DType dt, hipStream_t st);
int launch_gn_coef(const void* part, int nchunks, const float* gamma, const float* beta, int N, int P, int C, int groups, float eps, void* coef,
                   hipStream_t st);
// the apply half alone, with statistics produced by a conv3x3 epilogue (IgemmArgs::gn_part): double2 [N][nchunks][groups]
int launch_groupnorm_apply(const void* X, void* Y, const void* part, int nchunks, const float* gamma, const float* beta, const float* pos,
                           int N, int P, int C, int groups, float eps, int silu, DType dt, hipStream_t st);
// out = rmsnorm(x) * w  (rows of x at stride x_stride; HF semantics: normalised row rounded to T before the weight)
int launch_add_rmsnorm(void* x, long x_stride, const float* w, void* out, int M, int H, float eps, DType dt, hipStream_t st);
int launch_softmax(const float* S, void* Pm, long rows, int Lq, int Lk, int lds, int ldp, int causal, DType dt, hipStream_t st);

// ---- conv_small.hip
// First conv of the encoders: reads frames straight from the (B, T, 3, H, W) video (planar, fp32 or bf16),
// writes NHWC.  Image n of the launch is frame (n / per) * T_total + t0 + (n % per) of the clip tensor.
int launch_conv_in(const void* video, DType video_dt, const float* w /*[C0][3][3][3]*/, const float* bias, void* Y, DType dt,
                   int N, int per, int T_total, int t0, int H, int W, int C0, hipStream_t st);

// ---- vq.hip
// token row r = (g, i): g = r / tpf is a global frame, i = r % tpf;  b = g / nf, f = g % nf
//   -> element  b * stride + start + f * fstride + i  of the int64 token matrix (compressive_vq_model.py:205-215)
struct TokMap {
  int tpf, nf;
  long stride;
  int start, fstride;
};
int launch_sqnorm_rows(const float* E, float* out, int rows, int dim, hipStream_t st);
// out[map(r)] = argmin_j dist(z_r, e_j) + offset;  z fp32 [R][64];  lowest index on ties
int launch_vq_argmin(const float* z, const float* E, const float* ee, int64_t* out, const TokMap& map, int64_t offset, int R,
                     int n_e, hipStream_t st);
// Y[r][:] = E[clamp(ids[map(r)] - sub, 0, n_e - 1)][:]  (codebook fp32 -> T)
int launch_gather_rows(const int64_t* ids, const TokMap& map, const float* E, void* Y, DType dt, int R, int dim, int64_t sub,
                       int n_e, hipStream_t st);
// un-patchify: q[M*np*np][p*p*C] with feature order (ph, pw, c) -> NHWC [M][np*p][np*p][C]   (compressive_vq_model.py:247-250)
int launch_unpatchify(const void* q, void* out, DType dt, int M, int np, int C, int p, hipStream_t st);
// special tokens (scf / sdf slots) and labels (-100 over the context part)                    (compressive_vq_model.py:205-218)
int launch_finish_tokens(int64_t* ids, long stride, int64_t* labels, int B, int L, int ctx, int64_t scf, int64_t sdf, hipStream_t st);
// ids[b][17 i + 16] = sdf for i < n, rows `stride` apart: the separators of n frame slots (ivg_tokenize_frames)
int launch_sdf_columns(int64_t* ids, long stride, int B, int n, int64_t sdf, hipStream_t st);

// ---- llama_ops.hip
struct StepState {  // device-resident per-generate state (so one captured step graph can be replayed)
  int pos;          // number of tokens already in the KV cache (= position of the token being fed)
  int j;            // 1-based index of the NEW token being decided at this step
};
// x[b][:] = E[tok[b]] (+ act[b][slot][:] when add_act), T
// (x_bstride: elements between the outputs of consecutive trajectories; 0 = dense [B][L][H])
int launch_embed(const int64_t* ids, long id_stride, const void* E, void* x, DType dt, int B, int L, int H, int V, hipStream_t st,
                 long x_bstride = 0);
// RoPE on q,k of qkv[M][3H] (in place) and append k,v to the cache [B][heads][Lmax][hd]; position of row (b, l) = pos0 + l
// (pos0 from *state when state != null).  vt (optional): transposed V scratch [B][heads][hd][ldvt] for the prefill P.V GEMM;
// without a state its columns [L, ldvt) are zeroed.
int launch_rope_kv(void* qkv, void* kc, void* vc, void* vt, int ldvt, const float* cosT, const float* sinT, int B, int L,
                   int heads, int hd, int Lmax, const StepState* state, int pos0, DType dt, hipStream_t st);
// single-token step: RoPE of q / new k at position *pos, append k, v to the cache, then
// out[b][h*hd..] = softmax(q.K^T / sqrt(hd)) V over positions [0, *pos]
// causal prompt attention in one kernel (bf16, head_dim 64); -1 = not covered, use the score GEMM / softmax / P.V path
int launch_flash_prefill(const void* qkv, const void* kc, const void* vt, void* out, int B, int L, int Lp, int heads, int hd, int Lmax,
                         DType dt, hipStream_t st);
// attention of T appended tokens per trajectory (ivg_kv_extend's chunk pass; bf16, head_dim 64): query row (b, t) at position pos0 + t
// against cache rows [0, pos0 + t], after launch_rope_kv(.., vt = null, .., pos0) appended rows [pos0, pos0 + T).  V is read row-major from
// the cache.  -1 = not covered / does not fit / misaligned (nothing launched)
int launch_chunk_attn(const void* qkv, const void* kc, const void* vc, void* out, int B, int T, int heads, int hd, int Lmax, int pos0,
                      DType dt, hipStream_t st);
void kv_extend_note(int chunk_rows, int step_rows);   // B * T of an ivg_kv_extend by route (test hook, ivg_debug_counter("kv_extend_chunk_rows" / "_step_rows"))
long long kv_extend_rows(int stepwise);
void kv_extend_heads_note(int frame_rows, int scored_rows);   // B * F_out / B * T of an ivg_kv_extend_scored (test hook, "kv_extend_frame_rows" / "_scored_rows")
long long kv_extend_heads_rows(int scored);
// tokenizer attention in one pass (bf16): cross-attention, 4 heads of 32 / 64 / 128 / 192 channels, and the single-head
// self-attention of the conditional mid blocks (512 / 768 channels; M frames attending to themselves: F = 1, B = M); -1 = not covered
int launch_xattn(const void* q, const void* Kp, const void* VpT, void* out, int M, int F, int P, int kv, int C, int nh, DType dt, hipStream_t st);
bool xattn_covers(int P, int kv, int C, int nh, DType dt);   // pure predicate (shape, dtype): usable while planning the workspace
// prof (nullable): [IVG_ATTN_PROF_SLOTS][Lmax starts | Lmax ends] wall-clock stamps (100 MHz) of the launch at each cache
// position; workgroups spread over the slots so the atomics do not serialise on one address
#define IVG_ATTN_PROF_SLOTS 32
// the head dims decode_attn_kernel is instantiated for: hd / VEC lanes (VEC = 8 bf16, 4 fp32) share a key row and must divide the
// 256 lanes of a workgroup -- bf16 {8, 16, 32, 64, 128, 256}, fp32 {4, 8, 16, 32, 64, 128, 256}.  The prompt path (RoPE kernels, score
// and P.V GEMMs) covers every one of them; ivg_create refuses a transformer whose head dim fails this, launch_decode_attn any launch
bool decode_attn_covers(int hd, DType dt);
// sh_G > 1 (shared-context rollout): chunk row b belongs to group slot (b - sh_row0) / sh_G (sh_row0 <= 0); key rows t < sh_P are read
// from cache row `slot` (where the prefill of the group's prompt wrote them), rows t >= sh_P from the trajectory's own cache row b
int launch_decode_attn(const void* qkv, void* kc, void* vc, void* out, const float* cosT, const float* sinT, int B, int heads, int hd,
                       int Lmax, const StepState* state, unsigned long long* prof, DType dt, hipStream_t st, int sh_P = 0, int sh_G = 1,
                       int sh_row0 = 0);
// 24-bit K / V cache of the x3 rollout (llama_ops.hip): per (trajectory, head) [Lmax][64] uint16 (upper halves) | [Lmax][64] uint8 (next byte);
// head_dim 64, fp32 q / output.  launch_kv24_pack: fp32 rows [0, L) of [BH][Lmax][64] K and V (the prefill's scratch) -> the planes
int launch_decode_attn24(const void* qkv, void* kc, void* vc, void* out, const float* cosT, const float* sinT, int B, int heads, int Lmax,
                         const StepState* state, unsigned long long* prof, hipStream_t st, int sh_P = 0, int sh_G = 1, int sh_row0 = 0);
long long decode_attn24_launches();   // launches over the 24-bit cache since load (test hook: which cache format an x3 engine really ran)
int launch_kv24_pack(const void* k32, const void* v32, void* kc, void* vc, int BH, int L, int Lmax, hipStream_t st);
// FP8 (OCP e4m3fn) K / V cache of a bf16 rollout, opt-in (ivg_set_kv_format; llama_ops.hip): per (trajectory, head) [Lmax][64] bytes,
// byte = e4m3_rne(clamp(x_bf16 / scale, -448, 448)); head_dim 64, bf16 q / output.  launch_kv8_pack: bf16 rows [0, L) of [BH][Lmax][64]
// K and V (the prefill's scratch; must not overlap the byte rows) -> the cache
int launch_decode_attn8(const void* qkv, void* kc, void* vc, void* out, const float* cosT, const float* sinT, int B, int heads, int Lmax,
                        const StepState* state, unsigned long long* prof, float k_scale, float v_scale, hipStream_t st, int sh_P = 0, int sh_G = 1,
                        int sh_row0 = 0, const float* k_scales = nullptr, const float* v_scales = nullptr);
long long decode_attn8_launches();    // launches over the FP8 cache since load (test hook)
int launch_kv8_pack(const void* k16, const void* v16, void* kc, void* vc, int BH, int L, int Lmax, float k_scale, float v_scale, hipStream_t st,
                    int heads = 1, const float* k_scales = nullptr, const float* v_scales = nullptr);
// k_scales / v_scales (device, [heads], both or neither): per-head scales of one layer (ivg_set_kv_scales) used instead of the scalars;
// head = (b * heads + h) % heads.  launch_kv_absmax: amax [2][heads] (device, fp32 bit patterns) = max(amax, max |x|) per head over
// rows [0, L) of bf16 k16 / v16 [B * heads][Lmax][64] (kv_absmax_kernel: the calibration's observation; rows >= L are never read)
int launch_kv_absmax(const void* k16, const void* v16, int B, int heads, int L, int Lmax, unsigned int* amax, hipStream_t st);
bool kv8_scale_ok(float s);           // a finite, positive power of two whose reciprocal is a normal float (2^-126 .. 2^126)
int launch_expand_prompt_rows(const int64_t* prompts, long pstride, int64_t* ids, long ids_ld, int rows, int L, int G, int b0, hipStream_t st);
// token decision + embedding of the decided token (+ action embedding on forced sdf slots) + state advance
struct SampleArgs {
  const float* logits; int V;            // [B][V] fp32 (row stride V)
  const float* uniforms; int n_uni;      // [B][n_uni] or null (greedy)
  int top_k;
  int64_t* ids_out; long ids_stride; int L0;   // ids_out[b*ids_stride + L0 + j - 1] = token j
  int forced_period; int64_t forced_token;     // j % period == 0 -> forced token (0 = never)
  const void* E; void* x; int H;               // next input embedding x[b][:] (T)
  const void* act; int act_T; int ctx;         // act[B][act_T][H] (T) or null: added on forced slots, index slot0 + j/period + ctx - 1
  int slot0;                                   // sdf slots already inside the prompt beyond the first: (L0 - 257*ctx) / 17
  StepState* state;
  float temperature;                           // logits / temperature before the top-k filter (HF TemperatureLogitsWarper); 1.0: none
  float top_p = 1.0f;                          // nucleus filter after the top-k filter (include/ivg.h ivg_set_top_p); 1.0: none
};
int launch_sample_embed(const SampleArgs& a, int B, DType dt, hipStream_t st);
int launch_state_set(StepState* state, int pos, int j, hipStream_t st);
// y[b][t][:] = W[H][A] a[b][t][:] + bias  (tiny; fp32 in, T out)
int launch_action_embed(const float* act, const float* W, const float* bias, void* out, DType dt, int BT, int A, int H,
                        hipStream_t st);
int launch_add_rows(void* x, long x_stride, const void* add, long add_stride, int B, int H, DType dt, hipStream_t st);
// r[b] = rsqrt(mean(h[b]^2) + eps) * dot(h[b], w) + bias   (reward head on the RMS-normed hidden state);  eps < 0: plain dot + bias
int launch_rowdot(const void* h, const float* w, const float* bias, float* out, int B, int H, float eps, DType dt, hipStream_t st);
// out[b] = final RMSNorm of the residual rows x[b] as HF reports them in hidden_states[-1] (normalised row rounded to T, times w)
int launch_final_hidden(const void* x, const float* w, void* out, int B, int H, float eps, DType dt, hipStream_t st);
// per-frame heads of a forced-sdf rollout (ivg_generate_frames), launched once per decode step BEFORE the lm_head that advances the
// state: when the new token this step fed, state->j, is a frame's 16th (j = 17 i + 16, i < F), rew[b][i] = launch_rowdot's value and
// hid[b][i][:] = launch_final_hidden's row of the residual row x[b] (bit for bit); any other step writes nothing.  rew / hid: [B][F]
// floats / [B][F][H] T, either may be null
int launch_frame_heads(const void* x, const StepState* state, const float* rew_w, const float* rew_b, const float* norm_w, float* rew, void* hid,
                       int B, int H, int F, float eps, DType dt, hipStream_t st);
// the same heads on residual rows picked out of a matrix (ivg_kv_extend_scored): workgroup (b, k), b < B, k < F, reads row
// row0 + b * row_stride + k * frame_stride of x and writes rew[b * out_F + out_k0 + k], hid[b * out_F + out_k0 + k][:] -- on a given row
// the bits of launch_rowdot / launch_final_hidden
int launch_frame_rows_heads(const void* x, long row0, long row_stride, long frame_stride, const float* rew_w, const float* rew_b, const float* norm_w,
                            float* rew, void* hid, int B, int H, int F, int out_k0, int out_F, float eps, DType dt, hipStream_t st);
void frame_heads_note(int hits);   // the host's count of the launches above that hit a frame (test hook, ivg_debug_counter("frame_heads"))
long long frame_heads_hits();
// token scores of a rollout (ivg_generate_scored), launched directly after launch_sample_embed: out[b][j - 1][0..2] = { logprob of the
// id the sampler stored for new token j = state->j, entropy, max logprob } of the raw fp32 row logits[b][:]; three zeros on a forced
// column (j % forced_period == 0), nothing for j = 0 or j > cols.  out: [B][cols][3] floats
int launch_token_scores(const float* logits, int V, const StepState* state, const int64_t* ids, long ids_stride, int L0, int forced_period,
                        float* out, int cols, int B, hipStream_t st);
// launch_token_scores' row arithmetic per row of a chunk of logits rows whose targets are given ids, addressed as launch_token_nll's rows:
// scores of chunk row i = row r = row0 + i to out[((r / Tc) * out_ld + r % Tc) * 3 ..]; column c = r % Tc is three zeros when
// period > 0, c >= first_forced and (c - first_forced) % period == 0
int launch_token_scores_rows(const float* logits, const int64_t* ids, long ids_stride, long row0, int rows, int Tc, int V, int first_forced, int period,
                             float* out, long out_ld, hipStream_t st);
void token_scores_note(int launches);   // the host's count of the launches above (test hook, ivg_debug_counter("token_scores"))
long long token_scores_launches();
// filtered scores of a rollout (ivg_generate_filtered), launched in launch_token_scores' slot: out[b][j - 1][0..3] = { logprob of the id the
// sampler stored for new token j = state->j under the row after temperature, top-k and top-p (-inf outside the survivors), the entropy of
// that distribution, log of the share of the tempered softmax that survived, the number of survivors }; greedy: the raw row, no filter;
// four zeros on a forced column, nothing for j = 0 or j > cols.  out: [B][cols][4] floats
int launch_filtered_scores(const float* logits, int V, const StepState* state, const int64_t* ids, long ids_stride, int L0, int forced_period, int top_k,
                           float temperature, float top_p, bool greedy, float* out, int cols, int B, hipStream_t st);
void filtered_scores_note(int launches);   // the host's count of the launches above (test hook, ivg_debug_counter("filtered_scores"))
long long filtered_scores_launches();
// eval heads: shifted cross-entropy per row of a logits chunk, per-trajectory (sum, count), action reconstruction squared error
int launch_ce_rows(const float* logits, const int64_t* labels, long row0, int rows, int L, int V, float* nll, hipStream_t st);
// ce_rows_kernel's arithmetic for rows whose targets are given ids: chunk row i = row r = row0 + i of [B][Tc] rows, target
// ids[(r / Tc) * ids_stride + r % Tc], nll to out[(r / Tc) * out_ld + r % Tc]
int launch_token_nll(const float* logits, const int64_t* ids, long ids_stride, long row0, int rows, int Tc, int V, float* out, long out_ld,
                     hipStream_t st);
int launch_ce_reduce(const float* nll, const int64_t* labels, int B, int L, int V, float* out, hipStream_t st);
int launch_action_recon(const void* hidden, const float* W, const float* bias, const float* act, int B, int L, int H, int A, int act_T,
                        int ctx, int prelude, float* out, DType dt, hipStream_t st);
// *flag += number of differing 32-bit words between `rows` rows of row_bytes bytes (strides in bytes)
int launch_compare_rows(const void* a, long a_stride_bytes, const void* b, long b_stride_bytes, int rows, long row_bytes, int* flag,
                        hipStream_t st);

// ---- kv_select.hip (ivg_kv_select / ivg_cache_select: rows of a buffer gathered by a parents map)
// one buffer whose trajectory rows a select gathers: `slabs` slabs of rows at row_stride, each row `heads` blocks at head_stride, of
// which the first bytes_a bytes move -- and bytes_b more from plane_b on (0: one plane).  vec: 16 (every stride, offset and byte count a
// multiple of 16: the K / V slabs, the embeddings snapshot) or 4 (multiples of 4: the id rows, the action table)
struct KvSelectBuf {
  char* base = nullptr;
  int slabs = 1; long slab_stride = 0, row_stride = 0;
  int heads = 1; long head_stride = 0;
  long bytes_a = 0, bytes_b = 0, plane_b = 0;
  int vec = 16;
  size_t staged_bytes_per_slab(int n_staged) const { return (size_t)n_staged * heads * (bytes_a + bytes_b); }
};
// the plan's moves on one buffer: staged rows out to scratch, direct rows in place, staged rows back in -- slabs in groups as large as
// the scratch allows.  0, a hipError_t, or -4 (nothing launched) when the scratch does not hold one slab's staged rows
int launch_kv_select(const KvSelectBuf& b, const KvSelectPlan& plan, void* scratch, size_t scratch_bytes, hipStream_t st);
// dst row i := src row parents[i], 0 <= i < n, rows of row_bytes (a multiple of 16) bytes, contiguous, in two buffers that do not
// overlap; any n and any parents[i] >= 0 (the rows go in launches of at most 128 moves within windows of 256 rows)
int launch_gather_rows_by_parent(const void* src, void* dst, long row_bytes, const int32_t* parents, int n, hipStream_t st);
// ivg_kv_snapshot_create / _restore: b's rows against their compact image dense = [slabs][dense_rows][heads]{bytes_a |
// bytes_b} (aligned to b.vec).  restore false: image row i := row i, i < n == dense_rows; true: row i := image row parents[i], i < n
// (host array, [0, dense_rows); the caller keeps n within the rows b has room for).  At most 256 rows either way.  0 or a hipError_t
int launch_kv_snapshot(const KvSelectBuf& b, void* dense, int dense_rows, const int32_t* parents, int n, bool restore, hipStream_t st);
void kv_snapshot_note(int saved, int restored);   // trajectory rows saved / restored (test hook, ivg_debug_counter("kv_snapshot_rows_saved" / "_restored"))
long long kv_snapshot_rows(int restored);
void kv_select_note(int direct, int staged);   // trajectory rows a select moved (test hook, ivg_debug_counter("kv_select_direct" / "_staged"))
long long kv_select_rows(int staged);

// ---- ingest.hip
// uint8 frames [T][H][W][3] -> planar [T][3][R][R] in [0, 1]: / 255, optional centre crop, antialiased bilinear resize (ATen semantics)
int launch_ingest(const unsigned char* src, int T, int H, int W, int crop, void* dst, DType dst_dt, int R, hipStream_t st);
// the batched form (ivg_ingest_clips): B clips inside one buffer of total_bytes, clip b = `frames` stored H x W frames from byte `offset`
// (a multiple of 16) on -> dst [B][T][3][R][R], output frame t = what launch_ingest writes for stored frame min(t, frames - 1).
// `clips` is a host array; everything is checked before the first launch (hipErrorInvalidValue), nothing synchronises the host
struct IngestClipDesc { int64_t offset; int32_t frames, H, W; };   // == ivg_clip_desc
int launch_ingest_clips(const unsigned char* src, size_t total_bytes, const IngestClipDesc* clips, int B, int T, int crop, void* dst, DType dst_dt,
                        int R, hipStream_t st);

// ---- metrics.hip
// per-trajectory (mse, psnr, ssim) of predicted frames, mean over frames, best of the n_samples / B samples per trajectory
size_t frame_metrics_ws_bytes(int n_samples, int T, int H, int W);
int launch_frame_metrics(const void* gt, DType gt_dt, int B, int T_gt, int gt_t0, const float* pred, int n_samples, int T_pr, int pr_t0, int T,
                         int H, int W, float* rows, void* ws, hipStream_t st);

// ---- lpips.hip (LPIPS, VGG-16 variant: the fourth frame metric)
// cw / cb: the 13 convolutions' weights [Cout][kh][kw][Cin] fp32 and biases; lin: the 5 tap weight vectors.  Return values: 0, a
// hipError_t, or -4 when the workspace holds less than one image (features) / one image pair (rows).
bool lpips_shape_ok(int H, int W);                                  // H, W multiples of 16 (four 2 x 2 pools), >= 16
size_t lpips_ws_bytes(int max_images, int H, int W);
long lpips_ws_images(size_t ws_bytes, int H, int W);                // images of H x W a workspace of that size carries through the trunk
long long lpips_trunk_images();                                     // images sent through the trunk since load (test hook)
int launch_maxpool2(const float* X, float* Y, int N, int H, int W, int C, hipStream_t st);   // NHWC fp32, 2 x 2 / stride 2
int launch_lpips_input_layer(const void* images, DType dt, const float* w, const float* bias, float* Y, int n, int H, int W, hipStream_t st);
size_t lpips_head_part_bytes(int n1, int P);
// out[(i / n0) * group_stride + i % n0] (+)= sum_c lin[c] (f0n - f1n)^2 averaged over the P pixels, image i of f1 against image i % n0 of f0
int launch_lpips_head(const float* f0, const float* f1, const float* lin, int n0, int n1, int P, int C, float* out, long group_stride, int accumulate,
                      double* part, hipStream_t st);
int launch_lpips_features(const float* const* cw, const float* const* cb, const void* images, DType dt, int n, int H, int W, float* const* taps_out,
                          void* ws, size_t ws_bytes, hipStream_t st);
int launch_lpips_rows(const float* const* cw, const float* const* cb, const float* const* lin, const void* gt, DType gt_dt, int B, int T_gt, int gt_t0,
                      const float* pred, int n_samples, int T_pr, int pr_t0, int T, int H, int W, float* frames, float* rows, void* ws, size_t ws_bytes,
                      hipStream_t st);

// ---- i3d.hip (Kinetics-400 Inception-I3D, the FVD detector: fp32, channels-last [clip][d][h][w][c])
// conv3d: implicit GEMM on the f32-input MFMA, K = (kd, kh, kw, c); W [Cout][K], bias [Cout]; p: FRONT pad per axis (the back pad is the
// bounds check); input channel stride ldx, output channel stride ldy and offset coff; any Cin, Cout >= 1; kernel extents 1 .. 7, strides 1 / 2
struct Conv3dArgs {
  const float* X; const float* W; const float* bias; float* Y;
  int n, D, H, Wd, Cin, ldx, Do, Ho, Wo;
  int k[3], s[3], p[3];
  int Cout, ldy, coff, relu;
};
int launch_conv3d(const Conv3dArgs& a, hipStream_t st);
// pool3d: max-pool whose out-of-tensor taps read 0 (TensorFlow SAME padding: the zeros take part in the maximum)
struct Pool3dArgs {
  const float* X; float* Y;
  int n, D, H, Wd, C, ldx, Do, Ho, Wo;
  int k[3], s[3], p[3];
  int ldy, coff;
};
int launch_pool3d(const Pool3dArgs& a, hipStream_t st);
// head: X (n, D, P pixels, C) -> mean over (2, P) windows, stride 1 in time -> W [Nout][C] + bias -> mean over the D - 1 steps -> out (n, Nout)
size_t i3d_head_ws_bytes(int n, int D, int C);
int launch_i3d_head(const float* X, const float* W, const float* bias, float* out, int n, int D, int P, int C, int Nout, float* ws, hipStream_t st);
// front end: frames (F, 3, H, W) in [0, 1] -> (F, S, S, 3) fp32 = 2 * bilinear(x) - 1 (align_corners = False)
int launch_i3d_ingest(const void* video, DType dt, float* Y, long frames, int H, int W, int S, hipStream_t st);
struct I3dNet;
I3dNet* i3d_create(const ivg_tensor* weights, int n_weights, int device, int resize, int* status_out);   // failure: nullptr, the text set through set_create_error
void i3d_destroy(I3dNet* p);
int i3d_features_dim(const I3dNet* p);
int i3d_units(const I3dNet* p);
int i3d_check_shape(const I3dNet* p, int T, int H, int W);
size_t i3d_ws_bytes(const I3dNet* p, int max_clips, int T, int H, int W);
int i3d_features(const I3dNet* p, const void* video, DType dt, int B, int T, int H, int W, float* out, void* ws, size_t ws_bytes, hipStream_t st);
int i3d_tap(const I3dNet* p, const void* video, DType dt, int B, int T, int H, int W, int unit, float* out, int64_t* dims, void* ws, size_t ws_bytes,
            hipStream_t st);

}  // namespace ivg
