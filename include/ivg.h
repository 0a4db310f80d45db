/* libivg -- C ABI of the MI355X-native iVideoGPT prediction engine (gfx950 / ROCm).
 *
 * The reference (thuml/iVideoGPT) has no FFI layer: its drop-in boundary is the Python object API of
 *   CompressiveVQModel.{tokenize, detokenize, set_context_length}   ivideogpt/vq_model/compressive_vq_model.py:154-277
 *   LlamaForCausalLM.generate / HeadModelWithAction.generate       ivideogpt/transformer/action_model.py:56-121
 * (SURVEY.md 8b).  Each entry point below replaces one of those methods; the Python mirror of the
 * reference classes (the ivideogpt_amd package) binds them with ctypes, and INTEGRATION.md shows the stub a
 * maintainer of the reference would add.
 *
 * Conventions
 *   - every function returns 0 on success, a negative ivg_status otherwise; ivg_last_error(engine) holds the text;
 *   - all data pointers are DEVICE pointers owned by the caller (e.g. torch tensor data_ptr()); the engine borrows
 *     them for the duration of the call; weight tensors passed to ivg_create must stay alive until ivg_destroy;
 *   - work is enqueued on the caller's HIP stream and is asynchronous; no host synchronisation inside, except
 *     ivg_create / ivg_destroy / ivg_profile_read and the kept-cache verification of ivg_generate_continue / ivg_generate_embeds;
 *   - an engine is bound to one device and is not thread-safe (one engine per process per GPU);
 *   - token ids are int64, pixels are float32 or bfloat16 planar (B, T, 3, H, W) in [0, 1].
 */
#ifndef IVG_H_
#define IVG_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ivg_engine ivg_engine;
typedef struct ivg_cache ivg_cache;
typedef void* ivg_stream; /* hipStream_t */

/* IVG_F32X3 (ivg_config.decode_dtype / llm_dtype only): the tensors are float32 in HBM (pass IVG_F32 pointers), the matrix products of
 * the path run in split-bf16 arithmetic -- every operand as bf16 hi + bf16 lo (2^-17), all four partial products on the bf16 MFMA
 * path, fp32 accumulation: the mode that meets the 1e-3 parity bar on pixels / logits without the f32-input MFMA rate (1/16 of bf16). */
enum ivg_dtype { IVG_F32 = 0, IVG_BF16 = 1, IVG_F32X3 = 2 };

enum ivg_status {
  IVG_OK = 0,
  IVG_ERR_INVALID = -1,   /* bad argument / shape (the reference raises AssertionError here) */
  IVG_ERR_MISSING = -2,   /* a weight tensor is missing from the table */
  IVG_ERR_HIP = -3,       /* a HIP call or kernel launch failed */
  IVG_ERR_CAPACITY = -4   /* batch / frames exceed what the engine was created for */
};

/* A named weight tensor (device pointer).  Names are the checkpoint keys of the reference
 * (SURVEY.md Appendix C); layouts are the packed ones produced by ivideogpt_amd/packing.py. */
typedef struct {
  const char* name;
  const void* data;
  int32_t dtype;
  int32_t ndim;
  int64_t shape[4];
} ivg_tensor;

typedef struct {
  /* ---- tokenizer (CompressiveVQModel.__init__ kwargs, compressive_vq_model.py:36-60); n_levels = 0: no tokenizer */
  int32_t n_levels;
  int32_t block_out_channels[8];
  int32_t layers_per_block;
  int32_t latent_channels;
  int32_t vq_embed_dim;
  int32_t num_vq_embeddings;
  int32_t num_dyn_embeddings;
  int32_t norm_num_groups;
  int32_t mid_block_add_attention;
  int32_t context_length;
  int32_t max_att_resolution;
  int32_t resolution;
  int32_t patch_size;
  /* ---- transformer (HF LlamaConfig); num_layers = 0: no transformer */
  int32_t hidden_size;
  int32_t intermediate_size;
  int32_t num_layers;
  int32_t num_heads;       /* must divide hidden_size; head_dim = hidden_size / num_heads must be one the decode-attention kernel
                            * covers (bf16: 8, 16, 32, 64, 128, 256; fp32 and IVG_F32X3: 4 and those): IVG_ERR_INVALID at create otherwise */
  int32_t vocab_size;
  int32_t max_position_embeddings;
  float rms_norm_eps;
  int32_t action_dim;      /* 0: action-free LlamaForCausalLM; >0: HeadModelWithAction */
  int32_t reward_head;     /* 1: reward_linear present */
  /* ---- arithmetic types */
  int32_t encode_dtype;    /* tokenize path (default IVG_F32: VQ indices must match the fp32 reference; IVG_F32X3 is refused) */
  int32_t decode_dtype;    /* detokenize path: IVG_F32, IVG_BF16 or IVG_F32X3 */
  int32_t llm_dtype;       /* transformer: IVG_F32, IVG_BF16 or IVG_F32X3 */
  /* ---- capacity the workspace / KV cache are sized for */
  int32_t max_batch;       /* trajectories per call */
  int32_t max_frames;      /* frames per clip (T) */
  int32_t max_seq;         /* KV-cache length (0: max_position_embeddings; above it: IVG_ERR_INVALID, the RoPE tables end there) */
  /* ---- launch policy of THIS engine (no process-global state on the data path: a latency engine and a throughput engine can
   * live in one process, e.g. mbrl/video_predictor.py's step-wise rollout beside a batch evaluator) */
  int32_t decode_lds_kb;   /* LDS budget of a decode-step GEMM workgroup in KiB (16 .. 160); 0: the process default (IVG_DECODE_LDS_KB,
                            * 160 = a whole CU: fastest for one batch alone; <= 52: three or four workgroups of DIFFERENT engines share a CU --
                            * what several batches in flight on one GPU want.  A budget in force BELOW 160 -- set here or through the process
                            * default -- is the engine's BATCHES-IN-FLIGHT PROFILE: its decode GEMMs also request weights with the default
                            * cache policy -- the other engines over the same copy ask for the same lines -- and do not warm the next launch's
                            * weights; an explicit 160 is the one-batch profile, like 0 with the default untouched.  Best effort: shapes whose
                            * smallest plan is larger keep it.
                            * The budget picks the kernel generation and therefore the fp32 summation order: tokens of two budgets are
                            * each deterministic and batch-invariant but not bit-comparable with one another. */
} ivg_config;

int ivg_create(const ivg_config* cfg, const ivg_tensor* weights, int n_weights, int device, ivg_engine** out);
void ivg_destroy(ivg_engine* e);
const char* ivg_last_error(const ivg_engine* e);   /* e may be NULL: error of the last failed ivg_create */
const char* ivg_version(void);

/* The run-time switches (IVG_* environment variables, listed in ivideogpt_amd/csrc/switches.h) are read when the library is
 * loaded and at every ivg_create; a process that changes one afterwards (the A/B tests do) calls this to publish the change. */
void ivg_reload_switches(void);

/* `temperature` of every generate call of the reference (HF generate(..., temperature=...): inference/predict.py:61,
 * ivideogpt/transformer/action_model.py:61,89,104,128,143): the logits are divided by it before the top-k filter
 * (TemperatureLogitsWarper).  Engine state, default 1.0; IVG_ERR_INVALID unless strictly positive and finite (HF raises). */
int ivg_set_temperature(ivg_engine* e, float temperature);
/* `top_p` of HF generate (TopPLogitsWarper; the reference's callers never pass it).  Engine state, default 1.0 (no filter);
 * IVG_ERR_INVALID outside [0, 1] or NaN (HF raises).  It covers every generate entry of the engine.  Per row, the sampler runs
 *   1. logits / temperature (fp32);
 *   2. the top-k kept set, ties at the threshold kept;
 *   3. (top_p < 1) with e_i = exp(l_i - max) in fp64 over the kept set, Z = sum of e_i and S(i) = sum of e_j over the kept j with
 *      l_j <= l_i: token i survives iff S(i) > (1 - (double)top_p) * Z.  The maximum always survives, so top_p = 0 keeps the maximum
 *      and the tokens tied with it;
 *   4. the inverse CDF in ascending id order with the step's uniform over the survivors (fp64).
 * HF sums an fp32 cumsum where step 3 sums in fp64, and its unstable sort picks which tokens tied AT the nucleus boundary survive
 * where step 3 keeps all of them: both differ only on measure-zero boundaries.  A row of NaN logits still decides token 0. */
int ivg_set_top_p(ivg_engine* e, float top_p);
/* ivg_config.decode_lds_kb of a live engine (0 = back to the process default); takes effect at the next generate call */
int ivg_set_decode_lds_kb(ivg_engine* e, int kb);

/* K / V cache format of the transformer's rollouts.  IVG_KV_NATIVE (0, the default): the cache holds the engine's own element type
 * (bf16, fp32, or the 24-bit planes of an IVG_F32X3 engine) -- nothing differs from an engine that never called this.
 * IVG_KV_FP8_E4M3 (1): an opt-in, LOSSY one-byte cache for bf16 rollouts run for throughput.
 *   Availability  llm_dtype = IVG_BF16 and head_dim 64 only; every other engine answers IVG_ERR_INVALID, before anything is
 *                 allocated or launched, and keeps its format.
 *   Layout        per (layer, k|v, trajectory, head) [Lmax][64] bytes, dense in that order from the start of the allocation the bf16
 *                 cache occupies (the allocation does not change; its second half is unused).
 *   Element       OCP e4m3fn (gfx950's native FP8; not fnuz): byte = e4m3_rne(clamp(x_bf16 / scale, -448, +448)), where x_bf16 is exactly
 *                 the value the bf16 cache holds (the fp32 rotation rounded to bf16) and `scale` is k_scale for K, v_scale for V:
 *                 per engine, a finite positive power of two in [2^-126, 2^126] (the division is exact), default 1.0.  The clamp is
 *                 explicit: a finite value never becomes NaN (460 -> 448), NaN stores a NaN code.  Reference: torch on the CPU,
 *                 (x / scale).clamp(-448, 448).to(torch.float8_e4m3fn).
 *   Decode step   ropes q and the fed k as the bf16 step does; rounds the fed k and v to bf16, then to e4m3, BEFORE using them for
 *                 this step's own score and output (a later step reads exactly what this one computed with); appends them at `pos`;
 *                 out = softmax(q (k_scale K8)^T / 8) (v_scale V8) over rows [0, pos].  q and out are bf16, accumulation is fp32 in
 *                 a fixed order, no atomics on data; bf16 x e4m3 products are exact in fp32.
 *   Prompt pass   unchanged and bit-identical: it writes and reads bf16 K / V (a per-layer scratch), the rows are packed afterwards.
 * Bad format, or a scale that is not such a power of two: IVG_ERR_INVALID.  Takes effect at the next generate call on every entry
 * (ivg_generate, _shared, _forced_sdf, _continue, _embeds) and ALWAYS invalidates the kept cache: ivg_generate_continue and the
 * reuse path of ivg_generate_embeds then behave as for a cache never filled.  ivg_config does not change. */
enum ivg_kv_format { IVG_KV_NATIVE = 0, IVG_KV_FP8_E4M3 = 1 };
int ivg_set_kv_format(ivg_engine* e, int format, float k_scale, float v_scale);

/* Per-layer, per-head scales of the FP8 K / V cache, and their calibration on the device.
 * ivg_set_kv_scales   `scales` (host) is [num_layers][2 (k, v)][heads]: the element rule of ivg_set_kv_format with `scale` = the entry of the
 *     element's (layer, tensor, head), everything else unchanged (a decode step's output is softmax(q (ks[h] K8)^T / 8) (vs[h] V8)).
 *     Every entry must be such a power of two, and the engine one the FP8 format is available on; otherwise IVG_ERR_INVALID and
 *     nothing changes.  The format itself does not change: the table is in force while the format is IVG_KV_FP8_E4M3, until the next
 *     ivg_set_kv_format (any format: it sets uniform scales and drops the table).  Takes effect at the next generate call and ALWAYS
 *     invalidates the kept cache, as ivg_set_kv_format does.  SYNCHRONISES the device (launches still running may read the table it
 *     rewrites).  Step graphs are keyed by a counter every call of either setter bumps: none is replayed across a change.
 *     Shared-context rollouts use the table like the plain ones; every engine (lane, replica) owns its table.
 * ivg_get_kv_scales   the [num_layers][2][heads] scales in force (host), expanded from k_scale / v_scale when no table is set.
 * ivg_kv_calibrate    observes K and V.  Runs the teacher-forced prompt pass (the one behind ivg_logits; actions added on every sdf slot;
 *     no lm_head, no sampling) over ids (B, L), B in chunks of the KV cache's batch, and after each layer's RoPE folds max |x| over
 *     trajectories, positions [0, L) and elements of that layer's bf16 K and V into an engine-owned table amax[layer][k|v][head].
 *     The maximum is taken on integer bit patterns (order-independent; NaN ranks above Inf above every finite value, so a non-finite
 *     K / V is never hidden).  Feed whole ground-truth token rows: the pass then sees the positions a rollout appends, not only the
 *     context.  Calls accumulate until ivg_kv_calibration_reset (which synchronises the device and zeroes the table).  Enqueued on
 *     `stream`, no synchronisation; overwrites cache rows, so the kept cache is invalidated.  Works in either cache format and changes
 *     neither format nor scales.  Engines the FP8 format is not available on: IVG_ERR_INVALID.
 * ivg_kv_calibration_finish   SYNCHRONISES the stream of the last ivg_kv_calibrate call (as ivg_profile_read synchronises), reads amax,
 *     derives scale = 2^(p + headroom_log2) clamped to [2^-126, 2^126], where amax = m 2^e with m in [0.5, 1) and p = e - 9 if
 *     m <= 0.875, else e - 8 (2^p is the smallest power of two s with amax / s <= 448; integer arithmetic, no logarithm; amax = 0
 *     gives 1.0), and installs the table as ivg_set_kv_scales would.  amax_out / scales_out (host, [num_layers][2][heads], or NULL)
 *     receive what was observed / installed.  A NaN or Inf amax (ivg_last_error names layer, tensor and head) or headroom_log2
 *     outside [0, 8]: IVG_ERR_INVALID, nothing installed.  One bit of headroom (the Python default) costs a floating-point format no
 *     mantissa, only range at the subnormal end, and covers rows a rollout appends that the calibration set did not contain. */
int ivg_set_kv_scales(ivg_engine* e, const float* scales);
int ivg_get_kv_scales(ivg_engine* e, float* scales_out);
int ivg_kv_calibrate(ivg_engine* e, const int64_t* ids, int64_t ids_stride, int B, int L, const float* actions, int act_T, int ctx, ivg_stream stream);
int ivg_kv_calibration_reset(ivg_engine* e);
int ivg_kv_calibration_finish(ivg_engine* e, int headroom_log2, float* amax_out, float* scales_out);

/* CompressiveVQModel.set_context_length (compressive_vq_model.py:154-158): keeps the LAST k frames of kv_pos_emb. */
int ivg_set_context_length(ivg_engine* e, int context_length);

/* CompressiveVQModel.tokenize (compressive_vq_model.py:164-220).
 * pixels (B, T, 3, H, W); ids_out / labels_out int64 (B, 257*ctx - 1 + 17*(T - ctx)); labels_out may be NULL. */
int ivg_tokenize(ivg_engine* e, const void* pixels, int pixel_dtype, int B, int T, int64_t* ids_out, int64_t* labels_out,
                 ivg_stream stream);

/* Context-only fast path for prediction: what predict.py:53-54 / vp/ivideogpt_interface.py:158-169 /
 * mbrl/video_predictor.py:281-283 obtain by tokenizing zero-padded clips and slicing [:, :257*ctx].
 * pixels (B, T >= ctx, 3, H, W): only the first ctx frames are read.  ids_out int64 (B, ids_stride >= 257*ctx):
 * columns [0, 257*ctx) are written (context tokens, scf separators, trailing sdf). */
int ivg_encode_context(ivg_engine* e, const void* pixels, int pixel_dtype, int B, int T, int64_t* ids_out, int64_t ids_stride,
                       ivg_stream stream);

/* ---- The encoder's context cache: tokens of OBSERVED frames without encoding the context again.
 * The reference's tokenize encodes every future frame on its own; a frame sees the context only through the cross-attention K / V of the
 * conditional encoder (compressive_vq_model.py:174-196).  An ivg_enc_cache keeps those projections per trajectory -- for every
 * cross-attention site the projected Kp [kv][C] and VpT [C][kv] (kv = ctx * side * side) in the encode dtype, the context length in
 * force when it was filled, its row count and a filled flag; the engine owns the device memory.  Create / destroy: the refusals of
 * ivg_cache_create (B against max_batch: IVG_ERR_CAPACITY). */
typedef struct ivg_enc_cache ivg_enc_cache;
int ivg_enc_cache_create(ivg_engine* e, int B, ivg_enc_cache** out);
void ivg_enc_cache_destroy(ivg_engine* e, ivg_enc_cache* c);
/* ivg_encode_context that also fills `cache` (created for the same B): the plain encoder runs over the context frames once, the
 * features the conditional encoder reads are kept (as the full ivg_tokenize keeps them) and projected per site into the cache.  The
 * ids are those of ivg_encode_context, bit for bit. */
int ivg_encode_context_cached(ivg_engine* e, const void* pixels, int pixel_dtype, int B, int T, int64_t* ids_out, int64_t ids_stride,
                              ivg_enc_cache* cache, ivg_stream stream);
/* The tokens of n observed frames per trajectory against a filled cache.  frames (B, n, 3, H, W), planar, IVG_F32 or IVG_BF16;
 * ids_out int64 (B, ids_stride >= 17 n): column 17 i + j, j < 16, is dyn token j of frame i (with the num_vq_embeddings offset),
 * column 17 i + 16 is the sdf token, columns >= 17 n are not touched.  For the first n future frames of a clip that is
 * ivg_tokenize(clip) columns [257*ctx, 257*ctx + 17 n - 1) followed by the sdf the next frame's slot needs: what a prompt ending in
 * sdf is extended by (ivg_kv_extend).  The call runs the conditional encoder trunk over the B * n frames with the cached projections,
 * quant_linear and the argmin against the dyn codebook -- no plain-encoder launch, no projection launch -- on `stream`, without
 * synchronising the host, and never grows the workspace: n <= max_frames - ctx, else IVG_ERR_CAPACITY (as B above max_batch).
 * IVG_ERR_INVALID, before anything is launched or written: an engine without a tokenizer, a null or unfilled cache, a cache of another
 * engine or of another B, a cache filled under another context length than the one in force, n < 1, a pixel_dtype other than the two.
 * Arithmetic: the ids are those of ivg_tokenize bit for bit on an fp32 encoder, whose kernels sum every output element in one K order
 * whatever the number of images.  A bf16 encoder's ids are promised equal only where both calls dispatch the same kernels: its 1x1
 * convolutions and dense GEMMs with an output width that is a multiple of 256 go to the 256 x 256-tile kernel from 4096 rows on (a
 * multiple of 128: from 2^18 rows; gemm256.hip), and the row count is B * n * pixels here, B * (T - ctx) * pixels there. */
int ivg_tokenize_frames(ivg_engine* e, const void* frames, int pixel_dtype, int B, int n, const ivg_enc_cache* cache, int64_t* ids_out,
                        int64_t ids_stride, ivg_stream stream);
/* ivg_cache_select for the encoder's cache: a NEW cache of n rows, row i gathered from row parents[i] of src (a HOST array; src is
 * unchanged and stays the caller's), with the context length of src's fill.  Contract and refusals as there. */
int ivg_enc_cache_select(ivg_engine* e, const ivg_enc_cache* src, const int32_t* parents, int n, ivg_enc_cache** out, ivg_stream stream);

/* CompressiveVQModel.detokenize (compressive_vq_model.py:222-277).
 * ids int64 (B, 257*ctx - 1 + 17*F); pixels_out float32 (B, ctx + F, 3, H, W), unclamped.
 * cache: NULL, or a handle from ivg_cache_create.  cache_mode 1 = fill it (return_cache=True), 2 = reuse it
 * (cache=...): context frames are then not decoded again (their pixels are copied from the cache). */
int ivg_detokenize(ivg_engine* e, const int64_t* ids, int B, int F, float* pixels_out, ivg_cache* cache, int cache_mode,
                   ivg_stream stream);
/* The same with the element type of the result chosen by the caller: pixel_dtype IVG_F32, or IVG_BF16 when the engine decodes in
 * bfloat16 (decode_dtype = IVG_BF16) -- what the reference's callers get under torch.autocast(bfloat16)
 * (vp/ivideogpt_interface.py:180, mbrl/video_predictor.py:269): half the bytes of the clip, written by the last convolution's
 * epilogue.  A cache remembers the element type it was filled with; reuse with another one is IVG_ERR_INVALID. */
int ivg_detokenize_to(ivg_engine* e, const int64_t* ids, int B, int F, void* pixels_out, int pixel_dtype, ivg_cache* cache, int cache_mode,
                      ivg_stream stream);
/* detokenize for a batch whose rows come in groups of `group_size` consecutive trajectories with the SAME context tokens (the samples of
 * one clip, predict.py:65-72; VP2's candidates, vp/ivideogpt_interface.py:184-198): ids int64 (n_groups * group_size, 257*ctx - 1 + 17*F),
 * of which columns [0, 257*ctx - 1) are read from the FIRST row of every group.  The context frames are decoded once per group (and copied
 * to its other rows), the context decoder's features and the cross-attention K / V projections of the predicted frames exist once per
 * group.  pixels_out (n_groups * group_size, ctx + F, 3, H, W) in pixel_dtype, as ivg_detokenize_to.  No cache. */
int ivg_detokenize_shared(ivg_engine* e, const int64_t* ids, int n_groups, int group_size, int F, void* pixels_out, int pixel_dtype, ivg_stream stream);
/* on != 0: ivg_detokenize writes clamp(frames, 0, 1) -- the post-processing every caller of the reference applies to the decoded
 * clip (inference/predict.py:73, vp/ivideogpt_interface.py:199, train_gpt.py:438) -- from the epilogue of the decoders' last
 * convolution instead of a separate pass over the clip.  Default off: CompressiveVQModel.detokenize returns the raw output. */
int ivg_set_output_clamp(ivg_engine* e, int on);
int ivg_cache_create(ivg_engine* e, int B, ivg_cache** out);
void ivg_cache_destroy(ivg_engine* e, ivg_cache* c);
/* A NEW cache of n rows, row i gathered from row parents[i] of src (what ivg_kv_select does to the transformer's kept cache, for the
 * detokenizer's context cache; parents is a HOST array; src is unchanged and stays the caller's).  src must be filled.  The new cache
 * inherits the element type of the kept pixels, the clamp mode and the fill of src; its context pixels and every feature map are
 * gathered per trajectory on `stream`.  Refusals are those of ivg_cache_create (n against max_batch: IVG_ERR_CAPACITY) plus
 * IVG_ERR_INVALID for an empty src or a parent outside [0, rows of src); on failure everything allocated is released and *out is
 * not written. */
int ivg_cache_select(ivg_engine* e, const ivg_cache* src, const int32_t* parents, int n, ivg_cache** out, ivg_stream stream);

/* LlamaForCausalLM.generate (predict.py:57-69) when actions == NULL: every new token is sampled;
 * HeadModelWithAction.generate (action_model.py:56-121) when actions != NULL: the action embedding is added to the
 * i-th sdf slot (action index i + ctx - 1) and the sdf after every 16 tokens is forced.
 *   prompt   int64 (B, L0) row stride prompt_stride, L0 = 257*ctx
 *   actions  float32 (B, act_T, action_dim) or NULL;  ctx = context length (only used with actions)
 *   uniforms float32 (B, n_new) in [0,1) or NULL (NULL = greedy argmax); column j-1 drives new token j
 *   ids_out  int64 (B, L0 + n_new): prompt followed by the new tokens
 *   reward_out float32 (B) or NULL: reward_linear(last hidden state of the final step) (mbrl/video_predictor.py:311-313) */
int ivg_generate(ivg_engine* e, const int64_t* prompt, int64_t prompt_stride, int B, int L0, int n_new, const float* actions,
                 int act_T, int ctx, const float* uniforms, int top_k, int64_t* ids_out, float* reward_out, ivg_stream stream);

/* Shared-context rollouts.  Three of the reference's four callers hand generate() rows whose prompt is ONE clip's context repeated:
 * inference/predict.py:65 (gen_input.repeat(repeat_times, 1)), train_gpt.py:165-184 (generate_multiple_times: t samples per clip),
 * vp/ivideogpt_interface.py:155-202 (VP2: every candidate action sequence starts from the same two frames).  Here the prompt is given
 * ONCE per group of `group_size` consecutive trajectories: it is prefilled once, its K / V rows are stored once, and every decode step
 * of the group's trajectories reads those rows from the one copy (L2 / Infinity Cache hits instead of group_size HBM streams); only
 * positions >= L0 - 1 -- the prompt's last token, which carries the trajectory's own action, and the new tokens -- are per trajectory.
 *   prompts  int64 (n_groups, L0) row stride prompt_stride; trajectory b = g * group_size + k uses prompts[g]
 *   actions  float32 (n_groups * group_size, act_T, action_dim) or NULL (with actions: L0 must be 257*ctx, the context alone)
 *   uniforms float32 (n_groups * group_size, n_new) or NULL (greedy);  force_sdf != 0: ivg_generate_forced_sdf's schedule
 *   ids_out  int64 (n_groups * group_size, L0 + n_new);  reward_out float32 (n_groups * group_size) or NULL
 * Same tokens as ivg_generate on the repeated prompt up to the rounding of the prompt's LAST position (fed through the decode-step
 * kernels here, through the prompt pass there): identical except at near-ties of the sampler. */
int ivg_generate_shared(ivg_engine* e, const int64_t* prompts, int64_t prompt_stride, int n_groups, int group_size, int L0, int n_new,
                        const float* actions, int act_T, int ctx, const float* uniforms, int top_k, int force_sdf, int64_t* ids_out, float* reward_out,
                        ivg_stream stream);

/* HeadModelWithAction.generate_without_action (action_model.py:123-152; no caller in the reference): 16 sampled tokens per future
 * frame, then the forced sdf separator -- ivg_generate's action-conditioned schedule without any action embedding.  Same
 * arguments as ivg_generate minus actions / reward. */
int ivg_generate_forced_sdf(ivg_engine* e, const int64_t* prompt, int64_t prompt_stride, int B, int L0, int n_new, int ctx, const float* uniforms,
                            int top_k, int64_t* ids_out, ivg_stream stream);

/* Step-wise rollout (mbrl/video_predictor.py:286-317 calls generate once per environment step on a prompt that grew by the 17
 * tokens of the previous step): same contract as ivg_generate with actions != NULL, but the engine's KV cache is taken to
 * hold positions [0, L0 - 1) of these B trajectories from the previous ivg_generate / ivg_generate_continue call, so only
 * the prompt's last token (the sdf slot that receives the new action) is fed before the 16 + 1 new tokens -- no prefill.
 * Returns IVG_ERR_INVALID when the cache does not hold exactly that: other batch, other length, cache never filled, or built from
 * other tokens / actions (the cached prefix is compared with the prompt on the device: one stream synchronisation). */
int ivg_generate_continue(ivg_engine* e, const int64_t* prompt, int64_t prompt_stride, int B, int L0, int n_new, const float* actions,
                          int act_T, int ctx, const float* uniforms, int top_k, int64_t* ids_out, float* reward_out, ivg_stream stream);

/* Resample the kept cache (HF's _reorder_cache): new row i of the kept cache := old row parents[i], 0 <= i < n.  parents is a HOST
 * array.  For callers that act on rewards / uncertainties in the middle of a step-wise rollout -- drop trajectories, duplicate them,
 * reorder them -- and go on with ivg_generate_continue (or the reuse path of ivg_generate_embeds) instead of a new prompt pass.
 *
 * Precondition: the engine holds a kept cache, i.e. the last call was ivg_generate, _continue, _forced_sdf, _frames / _scored with
 * group_size == 1, or ivg_generate_embeds, with B within the cache chunk (min(max_batch, 128) rows).
 * Refusals, each before anything is launched or written -- the kept cache stays usable exactly as it was:
 *   IVG_ERR_INVALID   no kept cache (a fresh engine; after a shared-context call, ivg_set_kv_format, ivg_set_kv_scales, ivg_kv_calibrate);
 *                     n <= 0; a parents[i] outside [0, rows of the kept cache)
 *   IVG_ERR_CAPACITY  n above the cache chunk
 * Effect: as if the rows were gathered from a snapshot taken before the call -- duplicates, drops, growth (n above the kept rows) and
 * any permutation.  Gathered by the same map: positions [0, len) of every (layer, K | V) slab in the cache's own format (native bf16 /
 * fp32, both planes of the 24-bit format, FP8 bytes; FP8 scales are per head, not per trajectory: untouched), columns [0, len] of the
 * engine's id rows, the rows of the kept action table, and rows [0, len) of the embeddings snapshot of an embeds call.  Afterwards the
 * kept cache holds n trajectories at the same length, built under the same context length and action-table shape.  The kept-cache
 * entries then accept a prompt / actions / embeds the caller gathered by the same parents, and still refuse anything else: the
 * on-device verification stays the guard.
 * Rows >= n, positions >= len and rows with parents[i] == i are neither read nor written; parents equal to the identity over the kept
 * rows launches nothing.  Rows whose source is not itself overwritten (it keeps its place, or is dropped) are copied in place in one
 * launch; the others pass through the engine's workspace (planned at ivg_create: the call never grows it).  The work is enqueued on
 * `stream`; there is no host synchronisation, and no captured step graph is invalidated (a graph does not bake in which trajectory
 * a row is). */
int ivg_kv_select(ivg_engine* e, const int32_t* parents, int n, ivg_stream stream);

/* Set the kept cache aside and bring it back (HF: copy.deepcopy(past_key_values)): a snapshot is a caller-held copy of everything
 * ivg_kv_select gathers, in device memory of its own.  For callers whose engine must do something else between two steps of a
 * step-wise rollout -- imagine a batch beside a tracked session, serve several sessions, grow its batch -- and then go on with
 * ivg_generate_continue / ivg_kv_extend / ivg_generate_fanout instead of a prompt pass over the whole prefix; and for checkpointing a
 * node of a search that is left along another path than a rewind walks back.
 *
 * ivg_kv_snapshot_create.  Precondition: that of ivg_kv_select (the engine holds a kept cache).  Allocates exactly the kept state's
 * size -- [layers * 2][B][heads]{len * row_bytes_a | len * row_bytes_b} of the K / V slabs in the cache's own format (native bf16 /
 * fp32, both planes of the 24-bit format, FP8 bytes), then rows [0, len) of the embeddings snapshot of an embeds call, columns [0, len]
 * of the id rows and the rows of the kept action table, each dense: the layout depends neither on the engine's cache chunk nor on its
 * cache length -- and enqueues the copies on `stream`.  Recorded on the host: the kept state (len, B, built from ids or embeds, act_T,
 * ctx); layers, heads, head_dim, hidden size, action_dim, llm dtype and K / V format; the FP8 scales in force, by value (the two scalars
 * or the whole table); the device; and a weights tag, the device addresses of the packed embed_tokens and lm_head tensors the engine
 * was created with.  No host synchronisation beyond what hipMalloc implies; the live kept cache is unchanged.
 *   IVG_ERR_INVALID   no kept cache (as ivg_kv_select); an engine without a transformer; out == NULL
 *   IVG_ERR_HIP       the allocation failed: nothing is leaked, *out is not written
 * The snapshot belongs to the caller and outlives the engine: ivg_kv_snapshot_destroy takes no engine (its hipFree waits for the device).
 *
 * ivg_kv_snapshot_restore.  Afterwards the engine's kept cache holds n trajectories at the snapshot's length, row i = snapshot row
 * parents[i] (HOST array; NULL: the identity over the snapshot's rows, n is ignored) -- duplicates, drops, any order, more rows than
 * the snapshot has, up to the cache chunk -- and the kept host state is the snapshot's with B = n.  The kept-cache entries then accept
 * a prompt / actions / embeds gathered by the same parents exactly as after ivg_kv_select, and refuse anything else: the on-device
 * verification stays the guard.  Cache rows >= n, positions >= len and id columns beyond len are neither read nor written; no captured
 * step graph is invalidated.  The snapshot is const: it is restored any number of times, into the engine that made it or into another
 * engine over the SAME weights (the engine a model rebuilds for a larger batch, a second lane).  Enqueued on `stream`, which must be
 * ordered after the create's; no host synchronisation (the first restore of an embeds snapshot into an engine that never ran an embeds
 * call allocates that engine's embeddings snapshot).
 * Refusals, each before anything is launched or written -- the engine's kept cache stays usable exactly as it was:
 *   IVG_ERR_INVALID   a null snapshot; n <= 0 with parents != NULL; a parent outside the snapshot's rows; another device; any recorded
 *                     geometry, dtype or format that differs from the engine's; FP8 scales in force that differ from the recorded ones in
 *                     any bit; another weights tag; an engine without a transformer
 *   IVG_ERR_CAPACITY  n above the cache chunk; the snapshot's length beyond this engine's cache and id rows; its action table longer
 *                     than max_frames
 * ivg_kv_snapshot_info: out[IVG_KV_SNAPSHOT_INFO_INTS] = rows, length, device bytes, built from embeds (0 / 1), act_T, ctx, K / V format
 * (enum ivg_kv_format; 2: the 24-bit planes), device.  ivg_debug_counter("kv_snapshot_rows_saved" / "kv_snapshot_rows_restored") count
 * trajectory rows. */
typedef struct ivg_kv_snapshot ivg_kv_snapshot;
int ivg_kv_snapshot_create(ivg_engine* e, ivg_kv_snapshot** out, ivg_stream stream);
int ivg_kv_snapshot_restore(ivg_engine* e, const ivg_kv_snapshot* s, const int32_t* parents, int n, ivg_stream stream);
void ivg_kv_snapshot_destroy(ivg_kv_snapshot* s);
#define IVG_KV_SNAPSHOT_INFO_INTS 8
int ivg_kv_snapshot_info(const ivg_kv_snapshot* s, int64_t* out);

/* Extend the kept cache with GIVEN tokens (teacher forcing), or rewind it: afterwards it holds positions [0, L0 - 1) of prompt, of which
 * [0, keep_len) are the kept rows as they were and [keep_len, L0 - 1) are appended by this call.  T = L0 - 1 - keep_len.  For callers
 * that replace an imagined frame by the one they then observed, teacher-force ground-truth frames after the context, or rewind a few
 * frames and branch -- without a prompt pass over the whole prefix.
 *
 * Precondition: the engine holds a kept cache built from ids (ivg_generate, _continue, _forced_sdf, _frames / _scored with
 * group_size == 1, ivg_kv_select or this entry) of exactly B trajectories at length len; 1 <= keep_len <= min(len, L0 - 1);
 * prompt[:, :keep_len] equals the kept id rows; the cache was built the same way (with / without actions, the same ctx, the same act_T)
 * and the action rows baked into the sdf slots at positions < keep_len equal the presented ones.  Verified on the device as for
 * ivg_generate_continue: one stream synchronisation.
 * Refusals, each before anything but that comparison is launched -- outputs untouched, the kept cache usable exactly as it was:
 *   IVG_ERR_INVALID   no kept cache; a cache built from input embeddings (ivg_generate_embeds); another B; keep_len out of range; any
 *                     mismatch; an action table too short for the sdf slots among positions [0, L0 - 1) (or longer than max_frames)
 *   IVG_ERR_CAPACITY  L0 - 1 above the cache length
 * Effect: position p in [keep_len, L0 - 1) is fed embed_tokens[prompt[b][p]], plus action_linear(actions[b][i + ctx - 1]) when
 * p = 257*ctx - 1 + 17 i is an sdf slot and actions != NULL, and every layer's K / V rows are appended at p in the cache's own format.
 * The kept state is then: length L0 - 1, id columns [keep_len, L0 - 1] equal to prompt, the kept action table equal to actions -- so
 * ivg_generate_continue(prompt, L0, ..) is accepted, and ivg_kv_select, another ivg_kv_extend or ivg_generate_fanout.  Cache rows at
 * positions >= L0 - 1 are neither read nor written.  T == 0 is a pure rewind (also with keep_len < len: branch from an earlier frame):
 * nothing is launched after the verification.  No captured step graph is invalidated.
 *   token_nll_out  float32 (B, T) or NULL: column c = -log softmax(z_p)[prompt[b][p + 1]], p = keep_len + c, z_p the fp32 lm_head row of
 *                  position p (natural logarithm, the arithmetic of ivg_eval_forward's token_nll): how surprised the model was by each
 *                  given token.  An id outside [0, vocab) gives 0.
 * Two routes.  A native bf16 cache at head_dim 64 makes ONE pass over the B * T rows through the prompt-pass GEMMs with
 * chunk_attn_kernel as its attention (every K / V row read once per 32 query rows).  Every other engine (fp32, other head dims, the FP8
 * and 24-bit caches; or IVG_KV_EXTEND_CHUNK=0 under IVG_DEV=1) runs T decode steps with the given inputs instead of sampled ones, which
 * appends bit for bit what a rollout that had sampled these tokens would have appended.  ivg_debug_counter("kv_extend_chunk_rows" /
 * "kv_extend_step_rows") count B * T per call of either route. */
int ivg_kv_extend(ivg_engine* e, const int64_t* prompt, int64_t prompt_stride, int B, int keep_len, int L0,
                  const float* actions, int act_T, int ctx, float* token_nll_out /* (B, L0 - 1 - keep_len) or NULL */, ivg_stream stream);

/* ivg_kv_extend that also returns what the model thinks of the OBSERVED tokens it is given: token scores, and the reward and hidden
 * state of every frame whose 16th token this call feeds -- the values ivg_generate_scored returns for imagined frames, without a
 * prompt pass over the whole row (ivg_eval_forward + ivg_logits).  Preconditions, verification, effect on the kept cache, the two routes
 * and every refusal are ivg_kv_extend's, in its order and with its statuses (messages begin "kv_extend_scored: ").
 * With T = L0 - 1 - keep_len and p = keep_len + c:
 * Frames.  Predicted frame i >= 0 has its 16th token at position q_i = 257*ctx + 17 i + 15.  The call has outputs for exactly the frames
 *   with keep_len <= q_i <= L0 - 2, i.e. those whose 16th token this call feeds, written in increasing i from column 0; F_out is their
 *   number and i_first the first one.
 *   frame_hidden[b][k][:]  the final RMSNorm of the residual stream left by the pass that fed position q_{i_first + k}, with
 *                          final_hidden_kernel's rounding
 *   frame_rewards[b][k]    reward_linear on that row, in rowdot_kernel's arithmetic -- both as ivg_generate_frames defines them
 * Scores.  token_scores[b][c] = { z_p[g] - lse(z_p), H(softmax z_p), max z_p - lse(z_p) } with g = prompt[b][p + 1], in
 *   token_scores_kernel's arithmetic (ivg_generate_scored): NaN in all three for a maximum that is not finite, a NaN logprob for an id
 *   outside [0, V).  With actions != NULL (the forced schedule) a column whose TARGET position p + 1 is an sdf slot -- p + 1 >= 257*ctx - 1
 *   and (p + 1 - (257*ctx - 1)) % 17 == 0 -- is exactly 0, 0, 0, as ivg_generate_scored's forced columns; without actions every column
 *   is scored.  token_nll_out keeps ce_row_nll's arithmetic: -logprob and nll are the same quantity in two summation orders and are
 *   not promised bit-equal.
 * On the decode-step route the frame outputs and the score columns are bit for bit what ivg_generate_scored's own steps produce for a
 * rollout that had sampled these tokens; on the chunk pass the frame rows are bit for bit launch_rowdot / launch_final_hidden of the
 * pass's residual rows (frame_rows_heads_kernel: only the F_out rows per trajectory are normed) and lm_head runs only when
 * token_nll_out or token_scores_out is given.
 * Extra refusals, after ivg_kv_extend's argument checks and before the on-device comparison, outputs and kept cache untouched:
 *   IVG_ERR_MISSING   frame_rewards_out without a reward head; frame_hidden_out without 'llm.norm'
 * A rewind (T == 0) launches nothing after the verification and writes nothing; with F_out == 0 no frame kernel is launched and the
 * frame outputs are not written.  With all three new outputs NULL the entry launches exactly what ivg_kv_extend launches.
 * ivg_debug_counter("kv_extend_frame_rows") counts B * F_out per call, ("kv_extend_scored_rows") B * T per call that asked for scores. */
int ivg_kv_extend_scored(ivg_engine* e, const int64_t* prompt, int64_t prompt_stride, int B, int keep_len, int L0,
                         const float* actions, int act_T, int ctx,
                         float* token_nll_out      /* (B, T) or NULL: exactly ivg_kv_extend's */,
                         float* token_scores_out   /* (B, T, 3) or NULL */,
                         float* frame_rewards_out  /* (B, F_out) or NULL */,
                         void*  frame_hidden_out   /* (B, F_out, hidden), llm dtype, or NULL */,
                         ivg_stream stream);

/* Per-frame rewards and hidden states of one rollout call (the reference's generate is declared to return `reward (B, segment -
 * context)` and leaves it a TODO, action_model.py:83-99,118-120; its forward reads reward_linear at the hidden state of every frame's
 * 16th token, :198-204).
 *
 * Definition.  Under the forced-sdf schedule the new tokens are, per frame, 16 sampled tokens and then the forced sdf: new token j
 * (1-based) is forced when j % 17 == 0.  Frame i (0-based, counted from THIS call's first new token) has outputs iff its 16th token,
 * new token 17 i + 16, is FED to the transformer, i.e. 17 i + 16 <= n_new - 1 (the last new token is decided, never fed).  The number
 * of frames with outputs is therefore F_out = n_new / 17 (integer division).
 *   frame_hidden[b][i][:]  the final RMSNorm of the residual stream left by the forward pass that fed new token 17 i + 16, with the
 *                          rounding of HF's hidden_states[-1] (what ivg_eval_forward's hidden_out and ivg_generate_embeds' hidden_out hold)
 *   frame_rewards[b][i]    reward_linear on that state, in the arithmetic of ivg_generate's reward_out (norm weight folded into the
 *                          head's weights)
 * Consequences:
 *   - all F frames of a rollout: pass n_new = 17 F; the last forced sdf is decided and dropped by the caller, as the MBRL loop does
 *     with its 17 (mbrl/video_predictor.py:298-313);
 *   - n_new % 17 == 0: frame_rewards[:, F_out - 1] is bit for bit the value reward_out of the entry below would hold;
 *   - n_new = 17 F - 1 (the usual rollout length): F_out = F - 1, the last frame's 16th token is decided but not fed.
 * Both outputs are produced inside the decode steps (one small kernel per step that acts only on a frame's 16th token, captured with
 * the step graphs) into engine-owned buffers and copied out per cache chunk: no host work between the steps, any B.
 *
 * The entry stands for one of three: group_size == 1 and kept_cache == 0: ivg_generate (actions != NULL) / ivg_generate_forced_sdf
 * (actions == NULL, force_sdf != 0); group_size > 1: ivg_generate_shared (prompt holds one row per group, B = groups * group_size rows
 * of everything else); kept_cache != 0: ivg_generate_continue (group_size must be 1).  Arguments, tokens, the kept-cache verification
 * and the cache kept afterwards are those of that entry.  On top of its checks, before anything is launched or written:
 * IVG_ERR_INVALID unless the schedule is forced (actions != NULL or force_sdf != 0), n_new >= 17, L0 >= 257*ctx and
 * (L0 - 257*ctx) % 17 == 0, B a multiple of group_size, and group_size == 1 with kept_cache; IVG_ERR_MISSING for frame_rewards_out
 * without a reward head; IVG_ERR_CAPACITY for L0 + n_new beyond the cache.
 *   ids_out            int64 (B, L0 + n_new)
 *   frame_rewards_out  float32 (B, n_new / 17) or NULL
 *   frame_hidden_out   (B, n_new / 17, hidden) in the llm dtype, or NULL
 * With both NULL the call launches exactly what the entry it stands for launches. */
int ivg_generate_frames(ivg_engine* e, const int64_t* prompt, int64_t prompt_stride, int B, int L0, int n_new,
                        const float* actions, int act_T, int ctx, const float* uniforms, int top_k,
                        int group_size,   /* 1: as ivg_generate; > 1: as ivg_generate_shared (prompt: one row per group, B = groups * group_size) */
                        int kept_cache,   /* != 0: as ivg_generate_continue (group_size must be 1) */
                        int force_sdf, int64_t* ids_out,
                        float* frame_rewards_out /* (B, n_new / 17) or NULL */,
                        void* frame_hidden_out /* (B, n_new / 17, hidden) llm dtype or NULL */, ivg_stream stream);

/* Token log-probabilities and predictive entropy of a rollout: how sure the model was at every decision (HF generate's
 * output_logits = True with compute_transition_scores(..., normalize_logits = True), without the (B, V) logits ever leaving the device).
 *
 * Definition.  For every DECIDED new token j (1-based) of trajectory b let z be the fp32 logits row (V entries) the sampler reads for
 * that decision: the raw row as lm_head or the prompt pass left it, BEFORE the temperature division and before top-k and top-p, and
 * tok the id the sampler wrote.  Natural logarithms.
 *   logprob     = z[tok] - logsumexp(z)
 *   entropy     = - sum_i p_i log p_i,  p = softmax(z), a term with p_i = 0 counted as 0 (rows may hold -inf)
 *   max_logprob = max(z) - logsumexp(z), the log-confidence of the arg-max
 * All three describe the MODEL's distribution: they do not depend on the temperature, top_k, top_p, or on greedy against sampled
 * decoding (HF's `logits`, not its `scores`).  With greedy decoding logprob == max_logprob bit for bit.  Columns that decide nothing
 * are exactly 0.0 in all three: the forced sdf tokens (j % 17 == 0 under the forced schedule); the j = 0 step of kept-cache and
 * shared-context calls writes nothing at all.  A row whose maximum is not finite (NaN, +inf, all -inf) gives NaN in all three (such a
 * row decides token 0); nothing is read outside the row.
 * The probability under the FILTERED distribution actually drawn from (HF `scores`) is ivg_generate_filtered's output, defined with
 * that entry below; the sampler's instances stay instruction-identical under both.  The scores come from a kernel of their own
 * (token_scores_kernel, one workgroup per trajectory) launched inside the decode steps right after the sampler and captured with the
 * step graphs: fp32 with max subtraction, entropy as log s - (sum e_i (z_i - m)) / s, every sum in one fixed order -- the same bits
 * run to run, eager or replayed, in one call or step by step on the kept cache.  Engine-owned buffer, copied out per cache chunk.
 *
 * ivg_generate_scored: the arguments of ivg_generate_frames plus token_scores_out, and it stands for the same three entries.  The
 * forced-schedule, n_new >= 17 and prompt-length conditions of ivg_generate_frames apply ONLY when a frame output is requested: with
 * both frame outputs NULL it also serves the action-free ivg_generate (actions == NULL, force_sdf == 0).  With all three outputs NULL
 * it launches exactly what the entry it stands for launches.  Rows are in the engine's order (group-major for a shared context).
 * Refusals come before anything is launched or written and leave the outputs and the kept cache untouched.
 *   token_scores_out  float32 (B, n_new, 3): logprob, entropy, max_logprob; or NULL
 * ivg_generate_embeds_scored: ivg_generate_embeds (below) plus the same output; no column is forced there. */
int ivg_generate_scored(ivg_engine* e, const int64_t* prompt, int64_t prompt_stride, int B, int L0, int n_new,
                        const float* actions, int act_T, int ctx, const float* uniforms, int top_k,
                        int group_size, int kept_cache, int force_sdf, int64_t* ids_out,
                        float* frame_rewards_out /* (B, n_new / 17) or NULL */,
                        void* frame_hidden_out /* (B, n_new / 17, hidden) llm dtype or NULL */,
                        float* token_scores_out /* (B, n_new, 3): logprob, entropy, max_logprob; or NULL */, ivg_stream stream);

/* Embeds-level boundary of the step-wise caller (mbrl/video_predictor.py:286-317 runs these five ops per environment step).
 *
 * ivg_embed_tokens      HeadModelWithAction.get_input_embeddings (action_model.py:47-54): out[b][l][:] = embed_tokens[ids[b][l]],
 *                       out (B, L, hidden) in the engine's llm dtype.
 * ivg_action_linear     action_linear (action_model.py:36): out[r][:] = W a[r] + b, actions float32 (rows, action_dim),
 *                       out (rows, hidden) llm dtype.
 * ivg_generate_embeds   llm.generate(inputs_embeds=..., max_new_tokens, return_dict_in_generate=True, output_hidden_states=True)
 *                       (mbrl/video_predictor.py:298-313): embeds (B, L0, hidden) llm dtype; every new token is sampled (uniforms
 *                       (B, n_new) or NULL = greedy); new_ids_out int64 (B, n_new) = result.sequences (the inputs_embeds form of HF
 *                       generate returns only the new tokens); hidden_out (B, hidden) llm dtype or NULL = result.hidden_states[-1][-1],
 *                       the post-final-norm hidden state of the LAST forward pass (the one that produced the logits of new token n_new).
 *                       allow_reuse != 0: when the KV cache of the previous call on this engine was built from exactly
 *                       embeds[:, :L0 - 1] (verified on the device against a kept copy of the fed inputs -- one stream
 *                       synchronisation), only the last row is fed instead of a prefill of the grown prompt; *reused_out says which.
 * ivg_reward_linear     reward_linear (action_model.py:41; mbrl/video_predictor.py:313) on post-norm hidden rows (rows, hidden) llm
 *                       dtype -> float32 (rows). */
/* Scores of every decided new token under the distribution it was DRAWN from: the row after temperature, top-k and top-p (HF generate's
 * output_scores = True with compute_transition_scores(..., normalize_logits = True)): the proposal log-probability an importance weight
 * or a likelihood ratio over candidates needs, without the (B, V) logits leaving the device.
 *
 * Definition.  z, tok and j as for ivg_generate_scored; temperature, top_k, top_p the engine's settings in force for the call.
 *   l = z / temperature, an fp32 IEEE division, skipped when temperature == 1 (as the sampler's).
 *   K: the top-k kept set: the entries >= the top_k-th largest, ties at that threshold kept, -inf entries never; top_k <= 0 or
 *      top_k >= V keeps every finite entry.
 *   S: the survivors of ivg_set_top_p step 3: with e_i = exp((double)(l_i - max)) (the subtraction in fp32) and Z = sum of e_i over K,
 *      token i survives iff the mass of the kept tokens not above it exceeds (1 - (double)top_p) * Z; the maximum always survives;
 *      top_p >= 1 gives S = K.
 *   filtered_logprob = (l_tok - max) - log(sum_S e_i), -inf when tok is not in S
 *   filtered_entropy = the entropy of e_i / sum_S e over S
 *   kept_logmass     = log(sum_S e_i) - log(sum over all finite entries of e_i): at most 0, exactly 0 when nothing is filtered -- the
 *                      share of the tempered softmax that survived
 *   support          = |S| as a float
 * Natural logarithms; every sum in fp64 in one fixed order (no atomics: the same bits run to run, eager or replayed, in one call or
 * step by step on the kept cache), results rounded to fp32.  filtered_logprob + kept_logmass is the tempered raw log-probability.
 * Greedy calls (uniforms == NULL): HF builds no warpers -- S is every finite entry and the temperature is ignored: the four describe
 * the raw row.  Forced sdf columns are exactly 0 in all four; the j = 0 step writes nothing.  A row whose maximum is not finite, or that
 * holds a NaN, gives NaN in all four, an id outside [0, V) a NaN logprob without a read (ivg_generate_scored's rules).  V up to the
 * sampler's 256 * 72.
 * The scores come from filtered_scores_kernel, one workgroup of 256 threads per trajectory, launched inside the decode steps directly
 * after token_scores_kernel's slot -- after the sampler stored its id, before this step's lm_head overwrites the row -- and captured
 * with the step graphs.  It restates the filter (bisection of both thresholds over the key space, as the sampler's general path); the
 * sampler and token_scores_kernel are untouched.  Engine-owned buffer, copied out per cache chunk.
 *
 * ivg_generate_filtered = ivg_generate_scored plus filtered_scores_out, and stands for the same three entries; ivg_generate_fanout_filtered
 * and ivg_generate_embeds_filtered likewise.  With filtered_scores_out NULL each launches exactly what the entry it stands for launches
 * (ivg_debug_counter("filtered_scores") counts this kernel's launches, "token_scores" is unaffected).  Rows are in the engine's order
 * (group-major for a shared context).  Refusals are those of the entry it stands for, before anything is launched or written.
 *   filtered_scores_out  float32 (B, n_new, 4): filtered_logprob, filtered_entropy, kept_logmass, support; or NULL
 * Not covered: filtered scores of GIVEN tokens (ivg_kv_extend_scored has no sampler settings of its own). */
int ivg_generate_filtered(ivg_engine* e, const int64_t* prompt, int64_t prompt_stride, int B, int L0, int n_new,
                          const float* actions, int act_T, int ctx, const float* uniforms, int top_k,
                          int group_size, int kept_cache, int force_sdf, int64_t* ids_out,
                          float* frame_rewards_out /* (B, n_new / 17) or NULL */,
                          void* frame_hidden_out /* (B, n_new / 17, hidden) llm dtype or NULL */,
                          float* token_scores_out /* (B, n_new, 3) or NULL */,
                          float* filtered_scores_out /* (B, n_new, 4) or NULL */, ivg_stream stream);
int ivg_generate_fanout_filtered(ivg_engine* e, const int64_t* prompt, int64_t prompt_stride, int n_groups, int group_size, int L0, int n_new,
                                 const float* actions, int act_T, int ctx, const float* uniforms, int top_k, int force_sdf, int64_t* ids_out,
                                 float* frame_rewards_out, void* frame_hidden_out, float* token_scores_out /* (n_groups * group_size, n_new, 3) or NULL */,
                                 float* filtered_scores_out /* (n_groups * group_size, n_new, 4) or NULL */, ivg_stream stream);
int ivg_generate_embeds_filtered(ivg_engine* e, const void* embeds, int B, int L0, int n_new, const float* uniforms, int top_k,
                                 int64_t* new_ids_out, void* hidden_out, int allow_reuse, int* reused_out,
                                 float* token_scores_out /* (B, n_new, 3) or NULL */,
                                 float* filtered_scores_out /* (B, n_new, 4) or NULL */, ivg_stream stream);

int ivg_embed_tokens(ivg_engine* e, const int64_t* ids, int64_t ids_stride, int B, int L, void* out, ivg_stream stream);
int ivg_action_linear(ivg_engine* e, const float* actions, int rows, void* out, ivg_stream stream);
/* Fan candidates out of the kept cache: ivg_generate_scored with group_size > 1 whose shared prefix is not prefilled -- it IS the kept
 * cache.  prompt has one row per group; actions, uniforms and every output have n_groups * group_size rows, group-major.  Arguments,
 * outputs and the frame / score conditions are those of ivg_generate_scored, except that an action-conditioned prompt may hold
 * generated frames (L0 = 257*ctx + 17 t, as for ivg_generate_continue).
 * Precondition: the kept cache, built from ids, holds positions [0, L0 - 1) of exactly n_groups trajectories that equal
 * prompt[:, :L0 - 1], under the same ctx and the same with / without actions (verified as for ivg_generate_continue).  The action rows
 * of the candidates that belong to sdf slots already in the cache are neither read nor compared: the kept action table defined those
 * cache rows.  Candidate b = s * group_size + k reads key rows < L0 - 1 from cache row s and appends its own from position L0 - 1 on
 * in cache row b (decode_attn_kernel SHARED), in every cache format.
 * Refusals, before anything is launched or written, kept cache untouched: IVG_ERR_CAPACITY for n_groups * group_size above the cache
 * chunk (min(max_batch, 128)); IVG_ERR_INVALID without such a kept cache or on a mismatch; everything ivg_generate_scored refuses.
 * Afterwards the kept state is exactly what it was -- length L0 - 1, n_groups rows, the same ids, the same action table (the
 * candidates' rows lie at positions >= L0 - 1, outside it): the caller can fan out again, ivg_generate_continue with the chosen action,
 * or ivg_kv_extend with what it observed. */
int ivg_generate_fanout(ivg_engine* e, const int64_t* prompt, int64_t prompt_stride, int n_groups, int group_size, int L0, int n_new,
                        const float* actions, int act_T, int ctx, const float* uniforms, int top_k, int force_sdf, int64_t* ids_out,
                        float* frame_rewards_out /* (n_groups * group_size, n_new / 17) or NULL */,
                        void* frame_hidden_out /* (n_groups * group_size, n_new / 17, hidden) llm dtype or NULL */,
                        float* token_scores_out /* (n_groups * group_size, n_new, 3) or NULL */, ivg_stream stream);

int ivg_generate_embeds(ivg_engine* e, const void* embeds, int B, int L0, int n_new, const float* uniforms, int top_k, int64_t* new_ids_out,
                        void* hidden_out, int allow_reuse, int* reused_out, ivg_stream stream);
int ivg_generate_embeds_scored(ivg_engine* e, const void* embeds, int B, int L0, int n_new, const float* uniforms, int top_k,
                               int64_t* new_ids_out, void* hidden_out, int allow_reuse, int* reused_out,
                               float* token_scores_out /* (B, n_new, 3) as ivg_generate_scored; or NULL */, ivg_stream stream);
int ivg_reward_linear(ivg_engine* e, const void* hidden, int rows, float* out, ivg_stream stream);

/* Teacher-forced logits (LlamaForCausalLM.forward / HeadModelWithAction.forward, action_model.py:154-185):
 * ids int64 (B, L); actions as above or NULL (added on every sdf slot 257*ctx - 1 + 17*i < L); logits_out float32 (B, L, vocab). */
int ivg_logits(ivg_engine* e, const int64_t* ids, int B, int L, const float* actions, int act_T, int ctx, float* logits_out,
               ivg_stream stream);

/* Eval forward with labels (HeadModelWithAction.forward / LlamaForCausalLM.forward, action_model.py:154-205; train_gpt.py:356-376):
 * HF shifted cross-entropy, ignore_index -100, WITHOUT materialising the (B, L, vocab) fp32 logits (lm_head runs over row chunks that
 * are reduced to per-position losses in place).
 *   ids, labels    int64 (B, L); actions as in ivg_logits (added on every sdf slot) or NULL
 *   token_nll_out  float32 (B, L): -log p(labels[b][l+1] | ids[b][:l+1]) at position l; 0 where the target is ignored / l = L - 1
 *   loss_rows_out  float32 (B, 2): per trajectory (sum of token_nll, number of non-ignored targets); the HF loss of the batch is
 *                  sum(sums) / sum(counts), a trajectory's perplexity exp(sum / count)
 *   hidden_out     NULL or (B, L, hidden) llm dtype: post-final-norm hidden states (output_hidden_states=True, [-1]) -- what
 *                  reward_linear (action_model.py:198-204) and action_recon_linear (:187-196) read */
int ivg_eval_forward(ivg_engine* e, const int64_t* ids, const int64_t* labels, int B, int L, const float* actions, int act_T, int ctx,
                     float* token_nll_out, float* loss_rows_out, void* hidden_out, ivg_stream stream);
/* action reconstruction term (action_model.py:187-196): out[b] = sum over positions p >= prelude and action dims of
 * (action_recon_linear(hidden[b][p]) - actions[b][ctx - 1 + (p - prelude) / 17])^2;  mse_loss = sum(out) / (B * (L - prelude) * action_dim) */
int ivg_action_recon_sqerr(ivg_engine* e, const void* hidden, const float* actions, int B, int L, int act_T, int ctx, int prelude, float* out,
                           ivg_stream stream);

/* Clip ingest on the device: NPZParser.preprocess / EvalDataset.data_augmentation of the reference (inference/utils.py:12-16,
 * ivideogpt/data/simple_dataloader.py:512-516): frames uint8 (T, H, W, 3) as stored in the episode files -> / 255 -> optional centre
 * crop to the short side -> torchvision resize to (resolution, resolution), whose tensor path is antialiased bilinear interpolation
 * (ATen upsample_bilinear2d_aa semantics, width first) -> clip_out (T, 3, resolution, resolution) float32 or bfloat16 in [0, 1].
 * Downscale factors up to 15.  Engine-free. */
int ivg_ingest_frames(const uint8_t* frames, int T, int H, int W, int center_crop, void* clip_out, int out_dtype, int resolution,
                      ivg_stream stream);

/* The batched form: B clips that lie in ONE device buffer (the upload of a loader's pinned staging buffer), each with its own
 * frame count and frame size, in one launch.
 *   out[b][t] == bit for bit what ivg_ingest_frames writes for stored frame min(t, frames_b - 1) of clip b (its own H, W; the same
 *   crop, resolution and dtype): a clip longer than T is truncated, a shorter one repeats its last frame (EvalDataset.get_segment,
 *   simple_dataloader.py:522-526) -- on the device, from source bytes that are still read once.
 * `clips` is a HOST array of B entries: it travels in the kernel arguments (64 clips per launch; a larger B takes ceil(B / 64)
 * launches), so there is no device table to keep alive and no host synchronisation.  The kernel's aligned 32-bit loads stay inside
 * [staging, staging + staging_bytes).  Engine-free.
 * IVG_ERR_INVALID, before anything is launched or written: B <= 0, T <= 0 (or above 65535); a clip with frames, H or W < 1, an
 * offset that is negative or no multiple of 16, or offset + frames * H * W * 3 > staging_bytes; any clip ivg_ingest_frames refuses
 * (a downscale beyond 15, resolution above 1024). */
typedef struct { int64_t offset; int32_t frames, H, W; } ivg_clip_desc;   /* offset: bytes from `staging` to the clip's first stored frame */
int ivg_ingest_clips(const uint8_t* staging /* device */, size_t staging_bytes, const ivg_clip_desc* clips /* HOST, B entries */, int B, int T,
                     int center_crop, void* out /* (B, T, 3, R, R) */, int out_dtype, int resolution, ivg_stream stream);

/* Frame metrics of predicted clips on the device: Evaluator.forward of the reference without LPIPS
 * (ivideogpt/utils/video_metric.py:63-100; piqa PSNR(epsilon 1e-8, range 1) and SSIM(11 x 11 Gaussian, sigma 1.5, no padding)):
 * per frame mse / psnr / ssim, mean over the T frames of a trajectory, then the best of its t = n_samples / B samples
 * (min mse, max psnr, max ssim).  Engine-free (no weights).
 *   gt    (B, T_gt, 3, H, W) float32 or bfloat16 in [0, 1]; frames [gt_t0, gt_t0 + T) are compared
 *   pred  float32 (n_samples, T_pr, 3, H, W), frames [pr_t0, pr_t0 + T); sample k of trajectory b is row k * B + b
 *         (the layout of video_1.repeat([t, 1, 1, 1, 1]), video_metric.py:69-71)
 *   rows_out float32 (B, 3) = (mse, psnr, ssim): the per-trajectory rows the multi-GPU path all-gathers (train_gpt.py:476-479)
 *   ws    scratch of at least ivg_frame_metrics_ws_bytes(n_samples, T, H, W) bytes */
size_t ivg_frame_metrics_ws_bytes(int n_samples, int T, int H, int W);
int ivg_frame_metrics(const void* gt, int gt_dtype, int B, int T_gt, int gt_t0, const float* pred, int n_samples, int T_pr, int pr_t0, int T, int H,
                      int W, float* rows_out, void* ws, size_t ws_bytes, ivg_stream stream);

/* LPIPS (VGG-16 variant, v0.1, spatial = False) of predicted clips on the device: the fourth value of Evaluator.forward
 * (ivideogpt/utils/video_metric.py:75-88; network ivideogpt/vq_model/lpips.py), fp32 arithmetic.  The weights are the caller's: the
 * engine ships none.  Engine-free; a handle is bound to one device and borrows the weight tensors until ivg_lpips_destroy.
 *   weights  31 float32 tensors under the state-dict keys of the reference's LPIPS class: net.slice{1..5}.{i}.weight / .bias for
 *            i in (0, 2 | 5, 7 | 10, 12, 14 | 17, 19, 21 | 24, 26, 28) with the weights packed [Cout][kh][kw][Cin]
 *            (ivideogpt_amd/packing.py pack_lpips), and lin{0..4}.model.1.weight as vectors of 64 / 128 / 256 / 512 / 512.
 *            A missing tensor: IVG_ERR_MISSING; a wrong dtype or element count: IVG_ERR_INVALID (text in ivg_last_error(NULL)).
 *   gt, pred, the frame windows and the sample layout: as ivg_frame_metrics.  H and W: multiples of 16, >= 16 (IVG_ERR_INVALID).
 *   frames_out  float32 (n_samples, T) per-frame values, or NULL;  rows_out float32 (B): mean over the T frames, min over the t samples
 *   ws       scratch; the images pass the network in chunks of as many as it holds, and the result does not depend on that number,
 *            bit for bit.  ivg_lpips_ws_bytes(n, H, W): bytes that carry n images per chunk (a frame pair needs 2; with frames_out
 *            NULL the per-frame values take n_samples * T * 4 + 256 bytes more).  Too small for one pair: IVG_ERR_CAPACITY.
 * Every ground-truth frame passes the network once, every predicted frame once: B * T * (1 + t) images.  Nothing is launched and
 * nothing is written when a status other than IVG_OK / IVG_ERR_HIP is returned. */
typedef struct ivg_lpips ivg_lpips;
int ivg_lpips_create(const ivg_tensor* weights, int n_weights, int device, ivg_lpips** out);
void ivg_lpips_destroy(ivg_lpips* p);
size_t ivg_lpips_ws_bytes(int max_images_per_chunk, int H, int W);
int ivg_lpips_rows(ivg_lpips* p, const void* gt, int gt_dtype, int B, int T_gt, int gt_t0, const float* pred, int n_samples, int T_pr, int pr_t0, int T,
                   int H, int W, float* frames_out, float* rows_out, void* ws, size_t ws_bytes, ivg_stream stream);

/* ---- measurement hooks (bench.py): time one kernel class with HIP events on the launching stream; the decode attention
 * (which runs inside a replayed hipGraph) stamps its own launch windows with the 100 MHz wall clock instead */
enum ivg_kernel_class { IVG_K_IGEMM_BF16 = 0, IVG_K_IGEMM_F32 = 1, IVG_K_CONV3X3_BF16 = 2, IVG_K_CONV3X3_F32 = 3, IVG_K_DECODE_ATTN = 4,
                        IVG_K_DECODE_GEMM = 5,   /* the decode step's GEMMs (q/k/v, o, gate/up, down, lm_head): HBM-bound, bytes = weights */
                        IVG_K_COUNT = 6 };
typedef struct {
  int64_t launches;
  double total_ms;      /* sum of per-launch durations (hipEventElapsedTime) */
  double total_flops;   /* algorithmic: 2 * M * N * K per launch */
  double total_bytes;   /* algorithmic: operands read once + output written once */
} ivg_profile_stats;
int ivg_profile_enable(ivg_engine* e, int kernel_class, int enable);
int ivg_profile_read(ivg_engine* e, int kernel_class, ivg_profile_stats* out);   /* synchronises, then resets */
/* after ivg_profile_read(IVG_K_DECODE_ATTN): least-squares line  launch duration = fixed_us + bytes / gbps  over the launches
 * of the last ivg_generate (their cache lengths differ) -- separates the per-launch overhead from the streaming rate */
int ivg_profile_attn_fit(ivg_engine* e, double* fixed_us, double* gbps);
/* after ivg_profile_read(IVG_K_DECODE_GEMM): mean launch window (us) and launch count of the decode-step GEMMs by kind --
 * [0] q/k/v, [1] o-proj, [2] gate/up, [3] down, [4] lm_head (arrays of 5) */
int ivg_profile_gemm_kinds(ivg_engine* e, double* mean_us, int64_t* launches);

/* ---- op-level entry points (unit parity tests call the kernels through these) */
typedef struct {
  const void* X; const void* W; void* Y; const void* R; const float* bias;
  int32_t Nimg, Hin, Win, Cin, ldx, Hout, Wout, KH, KW, stride, pad, ups, N, ldw;
  int64_t c_img, c_pix, c_ch, c_grp_stride;
  int32_t c_grp, flags;
  float alpha;
  int32_t nb0, nb1, nb2;
  int64_t sa[3], sw[3], sy[3];
} ivg_igemm_args;
/* dtype IVG_F32X3: fp32 tensors, split-bf16 arithmetic (what an x3 engine's GEMMs run: gemm256x3_kernel where it covers the shape,
 * else igemm_kernel<float, ..., X3>); flags = IG_* of csrc/igemm.h */
int ivg_op_igemm(const ivg_igemm_args* a, int dtype, ivg_stream stream);
/* 3x3 convolution whose epilogue also reduces the GroupNorm statistics of its output into gn_part (double2 [Nimg][chunks][groups],
 * at least Nimg * ceil(Hout*Wout/256) * ceil(N/64) * groups entries), then GroupNorm(+SiLU) of that output from those statistics
 * into gn_out.  Returns the number of chunks per image (> 0) or a negative ivg_status. */
int ivg_op_conv_gn(const ivg_igemm_args* a, int dtype, void* gn_part, int groups, const float* gamma, const float* beta, void* gn_out, float eps,
                   int silu, ivg_stream stream);
/* y = conv3x3(silu(GroupNorm(x))) (+ bias, residual) with the GroupNorm applied inside the convolution's input staging: the
 * normalised tensor is never written.  ws: scratch of at least Nimg * (ceil(Hin*Win/1024) * groups * 16 + Cin * 8) bytes. */
int ivg_op_gn_conv(const ivg_igemm_args* a, int dtype, int groups, const float* gamma, const float* beta, float eps, void* ws, ivg_stream stream);
/* 3x3 convolution on fp32 tensors in split-bf16 arithmetic (the "x3" decode mode): w_x3 = the [N][9 * Cin] weight matrix with every 4
 * consecutive K elements stored as [bf16 hi(4) | bf16 lo(4)] (ivideogpt_amd/packing.py: pack_x3), activations split the same way
 * inside the kernel, fp32 accumulate.  gamma != NULL: y = conv3x3(silu(GroupNorm(x))) with the normalisation inside the staging
 * (ws as ivg_op_gn_conv).  IVG_ERR_INVALID when the 3x3 kernel does not cover the shape. */
int ivg_op_conv_x3(const ivg_igemm_args* a, const void* w_x3, int groups, const float* gamma, const float* beta, float eps, void* ws,
                   ivg_stream stream);
/* Nearest-x2 upsampling followed by a 3x3 convolution (diffusers Upsample2D: vae.py:271-284) in SUB-PIXEL form: four 2x2 convolutions over
 * the low-resolution input, one per output-pixel parity, with the weights pre-summed per parity (ivideogpt_amd/packing.py pack_subpixel:
 * w_sub [4][N][4 * Cin] in the element type of X) -- 2.25 x fewer multiplies, same result.  a->ups must be 1 and a->Hout = 2 a->Hin.
 * w_x3 / w_sub_x3 (both or neither): the split-bf16 arithmetic on fp32 tensors.  gn_part / groups as in ivg_op_conv_gn (NULL: no
 * statistics).  Returns the statistics chunks per image (0 without gn_part), IVG_ERR_INVALID when the sub-pixel kernel does not cover
 * the shape. */
int ivg_op_conv_subpixel(const ivg_igemm_args* a, int dtype, const void* w_sub, const void* w_x3, const void* w_sub_x3, void* gn_part, int groups,
                         ivg_stream stream);
/* The LDS-halo 3x3 kernel (csrc/conv3x3.hip) alone, with every option of a production launch at once -- never the implicit-GEMM fall-back.
 * gamma != NULL: GroupNorm(in_groups) + SiLU of the input inside the staging; ws as in ivg_op_gn_conv (statistics partials, then the
 * (scale, shift) table float2 [Nimg][Cin] at byte offset Nimg * ceil(Hin*Win/1024) * in_groups * 16, which the caller may read back).
 * in_part != NULL: the input's statistics come from a preceding convolution's epilogue (double2 [Nimg][in_chunks][in_groups]) instead of
 * a pass over X.  gn_part / groups: output statistics as in ivg_op_conv_gn (NULL: none).  w_x3: split-bf16 arithmetic (dtype IVG_F32 or
 * IVG_F32X3); w_sub / w_sub_x3: the sub-pixel weights of an upsampling convolution.  a->R, a->flags, c_* addressing as ivg_op_igemm.
 * Returns the statistics chunks per image (0 without gn_part); IVG_ERR_INVALID, before anything is launched or written, when the
 * kernel does not cover the call. */
int ivg_op_conv3x3(const ivg_igemm_args* a, int dtype, const float* gamma, const float* beta, int in_groups, float eps, void* ws,
                   const void* in_part, int in_chunks, void* gn_part, int groups, const void* w_x3, const void* w_sub, const void* w_sub_x3,
                   ivg_stream stream);
/* The instance and launch geometry launch_conv3x3 chooses for such a call, without launching (the launcher launches from the very same
 * plan): gn_in != 0 stands for gamma, gn_groups > 0 for gn_part with that many groups; a->X, a->W, w_sub count for their alignment
 * only.  out[0..14]: covered (1; 0: not covered; -1: invalid), kind (0 bf16, 1 fp32, 2 split-bf16), BN, TW, UPS, GNA, TPB2, SUBPIX,
 * tiles_x, tiles_per_img, tiles_n, channel chunks, staged epilogue, statistics chunks per image, dynamic LDS bytes. */
#define IVG_CONV3X3_PLAN_INTS 15
int ivg_op_conv3x3_plan(const ivg_igemm_args* a, int dtype, int gn_in, int gn_groups, const void* w_x3, const void* w_sub,
                        const void* w_sub_x3, int32_t* out);
/* Tokenizer cross-attention in one pass (bf16 only; IVG_ERR_INVALID when the shape is not covered): q [M][P][C], Kp [M/F][kv][C],
 * VpT [M/F][C][kv] -> out [M][P][C], heads of C / nh channels, softmax(q k^T / sqrt(C / nh)) v per head
 * (ivideogpt/vq_model/conditional_vae.py:38-55). */
int ivg_op_xattn(const void* q, const void* Kp, const void* VpT, void* out, int M, int F, int P, int kv, int C, int nh, int dtype, ivg_stream stream);
/* decode-step GEMM (M <= 128 rows; K bytes a multiple of 128): Y = epi(X W^T), flags = IG_* | SK_NORM of csrc/igemm.h */
int ivg_op_skinny(const void* X, const void* W, void* Y, int M, int N, int K, int ldx, int ldw, int ldy, int flags, int dtype,
                  ivg_stream stream);
/* the same under an engine's launch policy: lds_kb = ivg_config.decode_lds_kb (0: process default), w_shared != 0: default-policy weight
 * requests -- together the batches-in-flight profile, i.e. the kernel plans bench.py's lanes run (tests compare THOSE with fp64) */
int ivg_op_skinny_policy(const void* X, const void* W, void* Y, int M, int N, int K, int ldx, int ldw, int ldy, int flags, int dtype, int lds_kb,
                         int w_shared, ivg_stream stream);
/* dtype of both: IVG_F32, IVG_BF16, or IVG_F32X3 (fp32 tensors, split-bf16 arithmetic on the third-generation kernel; the second ignores
 * it and runs fp32); any other dtype, or lds_kb outside {0} u [16, 160], is IVG_ERR_INVALID before anything launches.
 * The plan the two would launch for these arguments (X / W / Y only for their alignment; nothing is read or launched), into out[0..10]:
 * generation (3: dgemm3.hip, 2: dgemm.hip, 0: not covered or nothing to do), row tiles MF, weight tiles FN, waves, then gen 3: lines of
 * K per wave, ring slots; gen 2: lines per burst LG, bursts, launch-bound class (4 / 8 / 16 waves); then rows of W per workgroup and
 * the split-bf16 flag.  Test hook: it calls the very plan functions the launchers use. */
#define IVG_SKINNY_PLAN_INTS 11
int ivg_op_skinny_plan(int M, int N, int K, int ldx, int ldw, int ldy, int flags, int dtype, int lds_kb, const void* X, const void* W,
                       const void* Y, int32_t* out);
int ivg_op_groupnorm(const void* X, void* Y, void* ws /* >= N*chunks*groups*16 B */, const float* gamma, const float* beta,
                     const float* pos, int N, int P, int C, int groups, float eps, int silu, int dtype, ivg_stream stream);
int ivg_op_softmax(const float* S, void* P, int64_t rows, int Lq, int Lk, int lds, int ldp, int causal, int dtype,
                   ivg_stream stream);
int ivg_op_vq_argmin(const float* z, const float* codebook, float* ee_ws /* n_e floats */, int64_t* out, int R, int n_e,
                     ivg_stream stream);
int ivg_op_add_rmsnorm(void* x, const float* w, void* out, int M, int H, float eps, int dtype, ivg_stream stream);
int ivg_op_conv_in(const void* video, int video_dtype, const float* w, const float* bias, void* Y, int dtype, int N, int per,
                   int T_total, int t0, int H, int W, int C0, ivg_stream stream);
/* One decode-attention step of a shared-context rollout (ivg_generate_shared): qkv (B, 3 * heads * hd) of the tokens being fed (RoPE
 * at `pos` is applied inside, the new k / v are appended at cache position `pos` of every row), caches kc / vc
 * (rows, heads, Lmax, hd) in which group slot s = (b - row0) / G (row0 <= 0) holds the shared prompt rows [0, P) in cache row s and
 * every trajectory b its own rows [P, pos) in cache row b; out (B, heads * hd).  With G = 1 and P = 0: the plain step.  A head dim
 * the kernel does not cover (include/ivg.h ivg_config.num_heads), a dtype other than IVG_F32 / IVG_BF16 or inconsistent positions:
 * IVG_ERR_INVALID before anything is allocated or launched. */
int ivg_op_shared_decode_attn(const void* qkv, void* kc, void* vc, void* out, const float* cos_t, const float* sin_t, int B, int heads, int hd, int Lmax,
                              int pos, int P, int G, int row0, int dtype, ivg_stream stream);
/* One prefill layer's attention over a prompt at positions [0, L) (1 <= L <= Lmax; hd even; dtype IVG_F32 or IVG_BF16): qkv [B * L][3 * heads * hd]
 * gets RoPE applied to q in place; the roped k and the v of row (b, l) are written to row l of kc / vc [B][heads][Lmax][hd] (rows >= L are
 * not touched); vt [B][heads][hd][Lp], Lp = rup(L, 64), receives V^T with columns [L, Lp) zeroed (NULL: skipped).  With out != NULL
 * (needs vt, qkv 16-byte and out 8-byte aligned), out [B * L][heads * hd] = softmax(q k^T / sqrt(hd), causal) v by the one-pass kernel,
 * which covers bf16 and hd = 64 only: IVG_ERR_INVALID otherwise.  cos_t / sin_t: [Lmax][hd / 2] fp32 as the engine holds them. */
int ivg_op_prefill_attn(void* qkv, void* kc, void* vc, void* vt, void* out, const float* cos_t, const float* sin_t, int B, int L, int heads, int hd,
                        int Lmax, int dtype, ivg_stream stream);
/* One layer's attention of ivg_kv_extend's chunk pass: T tokens per trajectory at positions [pos0, pos0 + T) against a cache that holds
 * [0, pos0).  qkv [B * T][3 * heads * hd] gets RoPE (at pos0 + t) applied to q in place; the roped k and the v of row (b, t) are written
 * to row pos0 + t of kc / vc [B][heads][Lmax][hd] (no other row is touched); out [B * T][heads * hd] = softmax(q k^T / sqrt(hd), key j
 * visible to row t iff j <= pos0 + t) v by chunk_attn_kernel.  bf16 and hd = 64 only; IVG_ERR_INVALID before any launch otherwise, and
 * for pos0 < 0, T < 1, pos0 + T > Lmax, or qkv / kc / vc not 16-byte, out not 8-byte aligned. */
int ivg_op_chunk_attn(void* qkv, void* kc, void* vc, void* out, const float* cos_t, const float* sin_t, int B, int T, int heads, int hd, int Lmax,
                      int pos0, int dtype, ivg_stream stream);
/* one top-k draw per logits row [B][V] fp32 with the rollout's sampler (uniforms [B] in [0,1), or NULL = greedy): HF
 * TemperatureLogitsWarper (logits / temperature, > 0) + TopKLogitsWarper + softmax + draw as restated by oracle/llama.py
 * sample_from_logits */
/* The 24-bit K / V cache of the IVG_F32X3 rollout (head_dim 64): per (trajectory, head) a block of Lmax * 192 bytes -- [Lmax][64] uint16,
 * the upper halves of the fp32 values rounded to 24 bits (nearest even), then [Lmax][64] uint8, the next byte.  ivg_op_kv24_pack: fp32
 * rows [0, L) of k32 / v32 [BH][Lmax][64] -> the planes (what the prefill does per layer).  ivg_op_decode_attn24: one decode-attention
 * step at cache position pos (RoPE of q / the new k, append of the rounded k / v, softmax(q K^T / 8) V over [0, pos]); qkv [B][3 * heads * 64]
 * fp32, out [B][heads * 64] fp32; P / G / row0 as ivg_op_shared_decode_attn (G = 1: every trajectory reads its own rows). */
int ivg_op_kv24_pack(const float* k32, const float* v32, void* kc, void* vc, int BH, int L, int Lmax, ivg_stream stream);
int ivg_op_decode_attn24(const float* qkv, void* kc, void* vc, float* out, const float* cos_t, const float* sin_t, int B, int heads, int Lmax, int pos,
                         int P, int G, int row0, ivg_stream stream);
/* The FP8 K / V cache (ivg_set_kv_format has the format): per (trajectory, head) [Lmax][64] bytes.  ivg_op_kv8_pack: bf16 rows [0, L) of
 * k16 / v16 [BH][Lmax][64] -> the byte rows of kc / vc (what the prefill does per layer; rows >= L are not touched; kc / vc must not
 * overlap k16 / v16).  ivg_op_decode_attn8: one decode-attention step at cache position pos; qkv [B][3 * heads * 64] bf16, out
 * [B][heads * 64] bf16; P / G / row0 as ivg_op_shared_decode_attn.  Scales as ivg_set_kv_format (IVG_ERR_INVALID otherwise). */
int ivg_op_kv8_pack(const void* k16, const void* v16, void* kc, void* vc, int BH, int L, int Lmax, float k_scale, float v_scale, ivg_stream stream);
int ivg_op_decode_attn8(const void* qkv, void* kc, void* vc, void* out, const float* cos_t, const float* sin_t, int B, int heads, int Lmax, int pos,
                        int P, int G, int row0, float k_scale, float v_scale, ivg_stream stream);
/* the same two with per-head scales (ivg_set_kv_scales): k_scales / v_scales are DEVICE arrays [heads] of one layer, BH = B * heads;
 * ivg_op_kv_absmax: the calibration's observation -- out [2][heads] (device, fp32 bit patterns, k then v) = max(out, max |x| per head over
 * rows [0, L) of bf16 k16 / v16 [B * heads][Lmax][64]); rows >= L are never read; the caller zeroes `out` to start over */
int ivg_op_kv8_pack_heads(const void* k16, const void* v16, void* kc, void* vc, int B, int heads, int L, int Lmax, const float* k_scales,
                          const float* v_scales, ivg_stream stream);
int ivg_op_decode_attn8_heads(const void* qkv, void* kc, void* vc, void* out, const float* cos_t, const float* sin_t, int B, int heads, int Lmax, int pos,
                              int P, int G, int row0, const float* k_scales, const float* v_scales, ivg_stream stream);
int ivg_op_kv_absmax(const void* k16, const void* v16, int B, int heads, int L, int Lmax, uint32_t* out, ivg_stream stream);
/* ivg_kv_select's move planner and kv_gather_rows_kernel on a caller-owned buffer laid out as the cache is:
 * [layers][2][chunk][heads]{[Lmax] rows of row_bytes_a | [Lmax] rows of row_bytes_b} (row_bytes_b = 0: one plane; both multiples of
 * 16, chunk <= 128).  New row i := old row parents[i] (host array, [0, B_old)) for i < n, positions [0, len); every other byte stays.
 * scratch (device, 16-byte aligned) stages the rows whose source is itself overwritten, slabs in groups as large as scratch_bytes
 * allows; IVG_ERR_CAPACITY, with nothing launched, when it does not hold one slab's staged rows or n > chunk.  Enqueued on `stream`. */
int ivg_op_kv_select(void* base, int layers, int chunk, int heads, int Lmax, int row_bytes_a, int row_bytes_b /* second plane, 0 if none */,
                     int len, int B_old, const int32_t* parents, int n, void* scratch, size_t scratch_bytes, ivg_stream stream);
/* ivg_kv_snapshot_create / _restore's copy on a caller-owned buffer laid out as for ivg_op_kv_select, against dense (device, 16-byte
 * aligned) = [layers * 2][B][heads]{len * row_bytes_a | len * row_bytes_b}.  direction 0: dense := the compact image of rows [0, B)
 * (parents, n ignored); 1: rows [0, n) := dense rows parents[i] (host array, [0, B)).  Every other byte of either side stays.
 * IVG_ERR_CAPACITY, with nothing launched, when dense_bytes is smaller than the image or n > chunk.  Enqueued on `stream`. */
int ivg_op_kv_snapshot(void* base, int layers, int chunk, int heads, int Lmax, int row_bytes_a, int row_bytes_b /* second plane, 0 if none */,
                       int len, int B, void* dense, size_t dense_bytes, const int32_t* parents, int n, int direction, ivg_stream stream);
int ivg_op_sample(const float* logits, int B, int V, int top_k, float temperature, const float* uniforms, int64_t* out, ivg_stream stream);
/* ivg_op_sample followed by the nucleus filter of ivg_set_top_p (steps 1-4 there); top_p outside [0, 1] or NaN: IVG_ERR_INVALID */
int ivg_op_sample_top_p(const float* logits, int B, int V, int top_k, float temperature, float top_p, const float* uniforms, int64_t* out,
                        ivg_stream stream);
/* the arithmetic of token_scores_kernel (ivg_generate_scored has the definition) on given rows: logits (B, V) float32, ids (B) the
 * chosen token of each row (not forced, j >= 1), out (B, 3) = logprob, entropy, max_logprob; V <= 256 * 72; an id outside [0, V) gives
 * a NaN logprob without a read */
int ivg_op_token_scores(const float* logits, const int64_t* ids, int B, int V, float* out, ivg_stream stream);
/* the arithmetic of filtered_scores_kernel (ivg_generate_filtered has the definition) on given rows under the given sampler settings:
 * logits (B, V) float32, ids (B), greedy != 0 as a call without uniforms; out (B, 4) float32.  IVG_ERR_INVALID for V outside
 * [1, 256 * 72], a temperature that is not positive and finite, a top_p outside [0, 1] */
int ivg_op_filtered_scores(const float* logits, const int64_t* ids, int B, int V, int top_k, float temperature, float top_p, int greedy,
                           float* out, ivg_stream stream);
/* token_scores_rows_kernel (ivg_kv_extend_scored): the same arithmetic per row of a chunk of `rows` logits rows (rows, V); chunk row i is
 * row r = row0 + i of (B, Tc) rows, (b, c) = (r / Tc, r % Tc), its target id ids[b * ids_stride + c], its scores out[(b * out_ld + c) * 3 ..];
 * column c is three zeros when period > 0, c >= first_forced and (c - first_forced) % period == 0.  Nothing else is written. */
int ivg_op_token_scores_rows(const float* logits, const int64_t* ids, int64_t ids_stride, int64_t row0, int rows, int Tc, int V,
                             int first_forced, int period, float* out, int64_t out_ld, ivg_stream stream);
/* LPIPS pieces (csrc/lpips.hip).  ivg_op_lpips_features: n images (n, 3, H, W) in [0, 1] (IVG_F32 / IVG_BF16) through the VGG-16 trunk,
 * taps_out[k] (n, H >> k, W >> k, 64 / 128 / 256 / 512 / 512) NHWC float32 (NULL entries are skipped); ws as ivg_lpips_rows (one image
 * at least).  ivg_op_lpips_head: out[i] = mean over the P pixels of sum_c lin[c] (f0n - f1n)^2 with f normalised per pixel by
 * sqrt(sum_c f^2) + 1e-10, image i of f1 (n1, P, C) against image i % n0 of f0 (n0, P, C); C in {64, 128, 256, 512};
 * ws of at least n1 * 128 bytes.  ivg_op_lpips_conv_in: the input layer alone, (n, 3, H, W) -> relu(conv(((2 x - 1) - shift) / scale))
 * (n, H, W, 64), w packed [64][3][3][3] as (co, kh, kw, ci).  ivg_op_maxpool2: 2 x 2 / stride 2 max-pool, NHWC float32, C % 4 == 0. */
int ivg_op_lpips_features(ivg_lpips* p, const void* images, int dtype, int n, int H, int W, float* const* taps_out, void* ws, size_t ws_bytes,
                          ivg_stream stream);
int ivg_op_lpips_head(const float* f0, const float* f1, const float* lin, int n0, int n1, int P, int C, float* out, void* ws, size_t ws_bytes,
                      ivg_stream stream);
int ivg_op_lpips_conv_in(const void* images, int dtype, const float* w, const float* bias, float* Y, int n, int H, int W, ivg_stream stream);
int ivg_op_maxpool2(const float* X, float* Y, int N, int H, int W, int C, ivg_stream stream);

/* FVD detector: Kinetics-400 Inception-I3D (csrc/i3d.hip), inference only, fp32 arithmetic on the f32-input MFMA.  The weights are the
 * caller's: the engine ships none.  Engine-free; a handle is bound to one device and borrows the weight tensors until ivg_i3d_destroy.
 *   weights  float32, 16-byte aligned, packed by ivideogpt_amd/packing.py pack_i3d: per convolution unit "<unit>.weight" (Cout, K) with
 *            batch norm folded in and K ordered (kd, kh, kw, c), "<unit>.bias" (Cout); "logits.weight" (400, C), "logits.bias".  Units:
 *            Conv3d_1a_7x7, Conv3d_2b_1x1, Conv3d_2c_3x3, Mixed_{3b,3c,4b..4f,5b,5c}.{b0,b1a,b1b,b2a,b2b,b3b}.  Channel counts are read
 *            from the shapes.  A missing tensor: IVG_ERR_MISSING; one whose shape does not fit its place: IVG_ERR_INVALID; the text
 *            in ivg_last_error(NULL) names it.
 *   resize   side S every frame is resized to (bilinear, align_corners = False, no antialias) before the trunk; 0: no resize (H == W)
 *   video    (B, T, 3, H, W) in [0, 1], IVG_F32 or IVG_BF16.  S must be a multiple of 32 and T leave two time steps in front of the
 *            average pool (T >= 9): IVG_ERR_INVALID otherwise.
 *   features_out  (B, 400) float32: the pre-softmax logits
 *   ws       scratch; ivg_i3d_ws_bytes(h, n, T, H, W): bytes that carry n clips per chunk (0 for a shape the detector refuses).  The
 *            batch is walked in chunks of as many clips as the scratch holds; a clip's features do not depend on the chunking, bit
 *            for bit.  Too small for one clip: IVG_ERR_CAPACITY.
 * Nothing is written when a status other than IVG_OK / IVG_ERR_HIP is returned. */
typedef struct ivg_i3d ivg_i3d;
int ivg_i3d_create(const ivg_tensor* weights, int n_weights, int device, int resize, ivg_i3d** out);
void ivg_i3d_destroy(ivg_i3d* p);
size_t ivg_i3d_ws_bytes(ivg_i3d* p, int max_clips, int T, int H, int W);
int ivg_i3d_features(ivg_i3d* p, const void* video, int dtype, int B, int T, int H, int W, float* features_out, void* ws, size_t ws_bytes,
                     ivg_stream stream);

/* I3D pieces (csrc/i3d.hip); tensors are channels-last float32 [clip][d][h][w][c].
 * ivg_op_conv3d: Y[.., coff + co] = act(sum_k X[..] W[co][k] + bias[co]), W (Cout, kd kh kw Cin) with K ordered (kd, kh, kw, c); any
 *   Cin, Cout >= 1, kernel extents 1 .. 7, strides 1 / 2; p = the FRONT pad per axis, taps outside the tensor read 0; ldx / ldy: channel
 *   strides of input and output, coff: first output channel written (nothing else of Y is touched).
 * ivg_op_pool3d: max-pool with the same geometry fields; taps outside the tensor count as 0 (TensorFlow SAME padding).
 * ivg_op_i3d_head: X (n, D, P, C) -> mean over (2, P) windows with stride 1 in time -> W (Nout, C) + bias -> mean over the D - 1 steps ->
 *   out (n, Nout); D >= 2; ws of n (D - 1) C floats.
 * ivg_op_i3d_ingest: frames (F, 3, H, W) in [0, 1] (IVG_F32 / IVG_BF16) -> (F, S, S, 3) = 2 bilinear(x) - 1.
 * ivg_op_i3d_tap: the activation after unit `unit_index` of a full forward of ivg_i3d_features' arguments, (B, D, H, W, C) contiguous.
 *   Units are numbered in execution order, pools included (Mixed: b0, b1a, b1b, b2a, b2b, b3a (pool), b3b); -1 is the front end's output.
 *   dims_out[8] (may be NULL) = D, H, W, C and the up to four units whose outputs, concatenated on channels, the unit reads (-1: the
 *   front end, -2: none).  out == NULL: the dims alone, nothing is launched.  ivg_i3d_units: the number of units. */
typedef struct {
  const float* X; const float* W; const float* bias; float* Y;
  int32_t n, D, H, Wd, Cin, ldx, Do, Ho, Wo;
  int32_t k[3], s[3], p[3];
  int32_t Cout, ldy, coff, relu;
} ivg_conv3d_args;
typedef struct {
  const float* X; float* Y;
  int32_t n, D, H, Wd, C, ldx, Do, Ho, Wo;
  int32_t k[3], s[3], p[3];
  int32_t ldy, coff;
} ivg_pool3d_args;
int ivg_op_conv3d(const ivg_conv3d_args* a, ivg_stream stream);
int ivg_op_pool3d(const ivg_pool3d_args* a, ivg_stream stream);
int ivg_op_i3d_head(const float* X, const float* W, const float* bias, float* out, int n, int D, int P, int C, int Nout, void* ws, size_t ws_bytes,
                    ivg_stream stream);
int ivg_op_i3d_ingest(const void* video, int dtype, int frames, int H, int W, int S, float* out, ivg_stream stream);
int ivg_op_i3d_tap(ivg_i3d* p, const void* video, int dtype, int B, int T, int H, int W, int unit_index, float* out, int64_t* dims_out, void* ws,
                   size_t ws_bytes, ivg_stream stream);
int ivg_i3d_units(ivg_i3d* p);
/* test hook: launches since the library was loaded of the kernel family `name` selects ("decode_gemm_gen3" / "decode_gemm_gen2":
 * decode-step GEMMs the dispatcher sent to dgemm3.hip / dgemm.hip; "conv3x3_subpixel": upsampling convolutions run as four 2x2 phase
 * convolutions; "decode_attn24" / "decode_attn8": decode-attention launches over the 24-bit / FP8 cache; "lpips_trunk_images": images sent through the VGG-16 trunk of the LPIPS metric; "frame_heads": decode steps whose frame_heads_kernel hit a frame; "token_scores": token_scores_kernel launches, one per step that ran the sampler of a scored call; "kv_select_direct" / "kv_select_staged": trajectory rows ivg_kv_select / ivg_op_kv_select moved in place / through scratch; "kv_snapshot_rows_saved" / "kv_snapshot_rows_restored": trajectory rows ivg_kv_snapshot_create / _restore (and ivg_op_kv_snapshot) copied out / in; "kv_extend_chunk_rows" / "kv_extend_step_rows": B * T of the ivg_kv_extend calls that took the chunk pass / the decode steps; "kv_extend_frame_rows" / "kv_extend_scored_rows": B * F_out of the ivg_kv_extend_scored calls / B * T of those that asked for scores; "enc_plain_images" / "enc_cond_images": images sent through the plain / the conditional encoder trunk; "enc_kv_projections": cross-attention K / V projections made for an encoder, one per site and call) -- lets a test assert WHICH kernel produced the tensor it checked; -1 for an unknown name */
int64_t ivg_debug_counter(const char* name);

#ifdef __cplusplus
}
#endif
#endif /* IVG_H_ */
