"""Thin Python handle on a libivg engine (one per process per GPU).  All compute happens in the HIP
library; PyTorch only owns the device buffers (weights, inputs, outputs) and the stream."""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .packing import config_code, dtype_code


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


# The id-prompt rollout entries of include/ivg.h in the order they are tried: (entry, the input that selects it, the inputs it has no
# parameter for).  The entries differ in their checks, so which one a call reaches is part of its behaviour.
_ROLLOUT_ENTRIES = (
    ("ivg_generate_fanout", "fanout", ("reuse_kv", "reward")),
    ("ivg_generate_scored", "token_scores", ("reward",)),
    ("ivg_generate_frames", "frame_outputs", ("reward",)),
    ("ivg_generate_shared", "shared", ("reuse_kv",)),
    ("ivg_generate_continue", "reuse_kv", ("force_sdf",)),
    ("ivg_generate_forced_sdf", "force_sdf", ("reward", "actions")),
    ("ivg_generate", None, ()),
)


# the entry that stands for one of the above and also takes filtered_scores_out (include/ivg.h ivg_generate_filtered)
_FILTERED_ENTRY = {"ivg_generate_scored": "ivg_generate_filtered", "ivg_generate_fanout": "ivg_generate_fanout_filtered"}


def rollout_entry(fanout=False, token_scores=False, frame_outputs=False, group_size=1, reuse_kv=False, force_sdf=False, reward=False,
                  actions=False):
    """The libivg entry that serves a rollout with these inputs (each but ``group_size`` a truth value: asked for / present).
    ValueError when the entry the inputs select cannot take one of them -- never a neighbouring entry that would drop it."""
    given = dict(fanout=fanout, token_scores=token_scores, frame_outputs=frame_outputs, shared=group_size > 1, reuse_kv=reuse_kv,
                 force_sdf=force_sdf, reward=reward, actions=actions)
    for name, when, lacks in _ROLLOUT_ENTRIES:
        if when is None or given[when]:
            bad = [k for k in lacks if given[k]]
            if bad:
                raise ValueError(f"rollout: {name} takes no {' / '.join(bad)}")
            return name


class KeptCache:
    """A transformer's kept K / V cache set aside (include/ivg.h ivg_kv_snapshot): device memory of its own, independent of the engine
    that made it -- it outlives that engine and is restored, any number of times, into it or into any engine over the same weights.
    ``rows``, ``length`` (kept positions), ``nbytes`` (device memory); ``from_embeds``, ``act_T``, ``ctx``, ``kv_format``, ``device_index``:
    how the cache was built.  ``close()`` releases the memory (idempotent; also on garbage collection); a context manager."""

    _FIELDS = ("rows", "length", "nbytes", "from_embeds", "act_T", "ctx", "kv_format", "device_index")

    def __init__(self, lib, h, weights_version=None):
        self.lib, self.h = lib, h
        self.weights_version = weights_version   # set by the model that saved it (LlamaForCausalLM.save_kept_cache)
        info = (C.c_int64 * _lib.IVG_KV_SNAPSHOT_INFO_INTS)()
        _lib.check(lib.ivg_kv_snapshot_info(h, info), None, "kv_snapshot_info")
        for k, v in zip(self._FIELDS, info):
            setattr(self, k, int(v))
        self.from_embeds = bool(self.from_embeds)

    @property
    def closed(self):
        return self.h is None

    def close(self):
        h, self.h = getattr(self, "h", None), None
        if h is not None:
            self.lib.ivg_kv_snapshot_destroy(h)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Engine:
    def __init__(self, device, tensors, tok_cfg=None, llm_cfg=None, action_dim=0, reward_head=False,
                 encode_dtype="fp32", decode_dtype="bf16", llm_dtype="bf16", max_batch=1, max_frames=16, max_seq=0,
                 decode_lds_kb=0):
        self.lib = _lib.load()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("ivideogpt_amd runs on an MI355X only (device must be 'cuda'); there is no CPU path")
        self.tensors = tensors  # keep the packed weights alive: the engine borrows their device memory
        cfg = _lib.IvgConfig()
        if tok_cfg is not None:
            ch = list(tok_cfg["block_out_channels"])
            cfg.n_levels = len(ch)
            for i, c in enumerate(ch):
                cfg.block_out_channels[i] = c
            for k in ("layers_per_block", "latent_channels", "vq_embed_dim", "num_vq_embeddings", "num_dyn_embeddings",
                      "norm_num_groups", "context_length", "max_att_resolution", "resolution", "patch_size"):
                setattr(cfg, k, int(tok_cfg[k]))
            cfg.mid_block_add_attention = int(bool(tok_cfg["mid_block_add_attention"]))
        if llm_cfg is not None:
            cfg.hidden_size, cfg.intermediate_size = llm_cfg["hidden_size"], llm_cfg["intermediate_size"]
            cfg.num_layers, cfg.num_heads = llm_cfg["num_hidden_layers"], llm_cfg["num_attention_heads"]
            cfg.vocab_size, cfg.max_position_embeddings = llm_cfg["vocab_size"], llm_cfg["max_position_embeddings"]
            cfg.rms_norm_eps = llm_cfg["rms_norm_eps"]
            cfg.action_dim, cfg.reward_head = int(action_dim or 0), int(bool(reward_head))
        cfg.encode_dtype, cfg.decode_dtype, cfg.llm_dtype = config_code(encode_dtype), config_code(decode_dtype), config_code(llm_dtype)
        cfg.max_batch, cfg.max_frames, cfg.max_seq = int(max_batch), int(max_frames), int(max_seq)
        cfg.decode_lds_kb = int(decode_lds_kb or 0)   # this engine's launch policy (include/ivg.h): 0 = the process default
        self.cfg = cfg
        names = [n.encode() for n in tensors]
        table = (_lib.IvgTensor * len(tensors))()
        for i, (n, t) in enumerate(tensors.items()):
            assert t.is_cuda and t.is_contiguous(), n
            table[i].name = names[i]
            table[i].data = t.data_ptr()
            table[i].dtype = dtype_code(t.dtype)
            table[i].ndim = min(t.dim(), 4)
            shp = list(t.shape) if t.dim() <= 4 else [t.numel()]
            for j, s in enumerate(shp[:4]):
                table[i].shape[j] = s
            if t.dim() > 4:
                table[i].ndim = 1
        self._names = names
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            rc = self.lib.ivg_create(C.byref(cfg), table, len(tensors), self.device.index or 0, C.byref(h))
        _lib.check(rc, None, "ivg_create")
        self.h = h
        self.max_batch, self.max_frames = int(max_batch), int(max_frames)
        # dedicated non-default stream for callers on the legacy default stream (graph capture needs one) -- created on first use: a
        # stream nobody runs on still takes a slot in the round-robin over the (4) hardware queues, and two batches in flight whose
        # streams land on the SAME hardware queue do not overlap at all (bench.py --lanes: 4,230 instead of 5,050 frames/s)
        self._stream = None
        self._caches = set()   # live detokenize caches (device memory owned here: released with the engine)
        self._enc_caches = set()   # live encoder context caches, likewise
        self._clamp_out = False
        self._temperature = 1.0
        self._top_p = 1.0
        self._run = None       # the stream of the last call (the dedicated one, or the caller's own)

    def close(self):
        if getattr(self, "h", None):
            for c in list(getattr(self, "_caches", ())):
                self.lib.ivg_cache_destroy(self.h, C.c_void_p(c))
            self._caches = set()
            for c in list(getattr(self, "_enc_caches", ())):
                self.lib.ivg_enc_cache_destroy(self.h, C.c_void_p(c))
            self._enc_caches = set()
            self.lib.ivg_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- stream plumbing.  A caller that made a stream of its own current (`with torch.cuda.stream(s):`, one per batch in flight) gets
    # the launches on THAT stream, like any PyTorch op; under the legacy default stream the engine runs on its dedicated stream,
    # ordered after the caller's current stream and before its future work.  The engine's workspace belongs to one stream at a time:
    # a call on another stream than the previous call's first waits for it.
    class _On:
        def __init__(self, eng):
            self.eng = eng

        def __enter__(self):
            eng = self.eng
            cur = torch.cuda.current_stream(eng.device)
            if cur == torch.cuda.default_stream(eng.device):
                if eng._stream is None:
                    eng._stream = torch.cuda.Stream(device=eng.device)
                run = eng._stream
            else:
                run = cur
            if eng._run is not None and eng._run != run:
                run.wait_stream(eng._run)
            if run != cur:
                run.wait_stream(cur)
            eng._run, self.cur = run, cur
            return C.c_void_p(run.cuda_stream)

        def __exit__(self, *exc):
            if self.eng._run != self.cur:
                self.cur.wait_stream(self.eng._run)
            return False

    def stream(self):
        return Engine._On(self)

    def check(self, rc, what):
        _lib.check(rc, self.h, what)

    def _record(self, *tensors):
        """The caller's tensors a call reads or writes are in use on the stream it ran on."""
        for t in tensors:
            if t is not None:
                t.record_stream(self._run)

    # ---- entry points
    def set_temperature(self, t):
        """``temperature`` of the reference's generate calls (engine state: rarely anything but 1.0)."""
        t = float(t)
        if t != self._temperature:
            self.check(self.lib.ivg_set_temperature(self.h, t), "set_temperature")
            self._temperature = t
        return self

    def set_top_p(self, p):
        """``top_p`` of HF generate (nucleus filter after the top-k filter, include/ivg.h ivg_set_top_p; 1.0: none).  Engine state."""
        p = float(p)
        if p != self._top_p:
            self.check(self.lib.ivg_set_top_p(self.h, p), "set_top_p")
            self._top_p = p
        return self

    def set_decode_lds_kb(self, kb):
        """LDS budget of this engine's decode-step GEMMs (``ivg_config.decode_lds_kb``; 0 = process default, 16 .. 160 KiB)."""
        self.check(self.lib.ivg_set_decode_lds_kb(self.h, int(kb or 0)), "set_decode_lds_kb")
        return self

    def set_kv_format(self, fmt, k_scale=1.0, v_scale=1.0):
        """``ivg_set_kv_format``: K / V cache format of the rollouts (``_lib.IVG_KV_NATIVE`` / ``IVG_KV_FP8_E4M3``) and its scales; takes
        effect at the next generate call and invalidates the kept cache."""
        self.check(self.lib.ivg_set_kv_format(self.h, int(fmt), float(k_scale), float(v_scale)), "set_kv_format")
        return self

    def _kv_table_shape(self):
        return (int(self.cfg.num_layers), 2, int(self.cfg.num_heads))

    def set_kv_scales(self, scales):
        """``ivg_set_kv_scales``: per (layer, k|v, head) scales of the FP8 K / V cache, a ``(layers, 2, heads)`` tensor or nested list of
        powers of two; in force while the format is FP8, until the next ``set_kv_format``.  Invalidates the kept cache; synchronises."""
        t = torch.as_tensor(scales, dtype=torch.float32).cpu().contiguous()
        if tuple(t.shape) != self._kv_table_shape():
            raise ValueError(f"set_kv_scales: scales must have shape {self._kv_table_shape()}, not {tuple(t.shape)}")
        self.check(self.lib.ivg_set_kv_scales(self.h, _ptr(t)), "set_kv_scales")
        return self

    def get_kv_scales(self):
        """``ivg_get_kv_scales``: the scales in force as a ``(layers, 2, heads)`` float32 CPU tensor (the two scalars expanded when no table is set)."""
        t = torch.empty(self._kv_table_shape(), dtype=torch.float32)
        self.check(self.lib.ivg_get_kv_scales(self.h, _ptr(t)), "get_kv_scales")
        return t

    def kv_calibrate(self, ids, actions=None, ctx=1, reset=False):
        """``ivg_kv_calibrate``: the teacher-forced prompt pass over ``ids (B, L)`` that folds max |K|, max |V| per (layer, head) into the
        engine's table (calls accumulate; ``reset``: ``ivg_kv_calibration_reset`` first).  Enqueued, no synchronisation."""
        if reset:
            self.check(self.lib.ivg_kv_calibration_reset(self.h), "kv_calibration_reset")
        B, L = ids.shape
        act_T = actions.shape[1] if actions is not None else 0
        with self.stream() as s:
            self.check(self.lib.ivg_kv_calibrate(self.h, _ptr(ids), ids.stride(0), B, L, _ptr(actions), act_T, int(ctx), s), "kv_calibrate")
            self._record(ids, actions)
        return self

    def kv_calibration_finish(self, headroom=1):
        """``ivg_kv_calibration_finish`` (synchronises): -> (amax, scales), ``(layers, 2, heads)`` float32 CPU tensors; the scales are installed."""
        amax, scales = torch.empty(self._kv_table_shape(), dtype=torch.float32), torch.empty(self._kv_table_shape(), dtype=torch.float32)
        self.check(self.lib.ivg_kv_calibration_finish(self.h, int(headroom), _ptr(amax), _ptr(scales)), "kv_calibration_finish")
        return amax, scales

    def set_context_length(self, k):
        self.check(self.lib.ivg_set_context_length(self.h, int(k)), "set_context_length")

    def tokenize(self, pixels, ids, labels):
        B, T = pixels.shape[:2]
        with self.stream() as s:
            self.check(self.lib.ivg_tokenize(self.h, _ptr(pixels), dtype_code(pixels.dtype), B, T, _ptr(ids), _ptr(labels), s), "tokenize")
            self._record(pixels, ids, labels)

    def encode_context(self, pixels, ids):
        B, T = pixels.shape[:2]
        with self.stream() as s:
            self.check(self.lib.ivg_encode_context(self.h, _ptr(pixels), dtype_code(pixels.dtype), B, T, _ptr(ids), ids.stride(0), s),
                       "encode_context")
            pixels.record_stream(self._run); ids.record_stream(self._run)

    def enc_cache_create(self, B):
        h = C.c_void_p()
        self.check(self.lib.ivg_enc_cache_create(self.h, int(B), C.byref(h)), "enc_cache_create")
        self._enc_caches.add(h.value)
        return h

    def enc_cache_destroy(self, h):
        if self.h is not None and h.value in self._enc_caches:   # (already released when the engine was closed first)
            self._enc_caches.discard(h.value)
            self.lib.ivg_enc_cache_destroy(self.h, h)

    def enc_cache_select(self, h, parents):
        """``ivg_enc_cache_select``: a new encoder cache whose row i is row ``parents[i]`` (host integers) of cache ``h``; ``h`` is unchanged."""
        p = np.ascontiguousarray(parents, dtype=np.int32)
        out = C.c_void_p()
        with self.stream() as s:
            self.check(self.lib.ivg_enc_cache_select(self.h, h, p.ctypes.data_as(C.c_void_p), int(p.size), C.byref(out), s), "enc_cache_select")
        self._enc_caches.add(out.value)
        return out

    def encode_context_cached(self, pixels, ids, cache):
        """``ivg_encode_context_cached``: ``encode_context`` that also fills the encoder cache ``cache`` (a handle of ``enc_cache_create``)."""
        B, T = pixels.shape[:2]
        with self.stream() as s:
            self.check(self.lib.ivg_encode_context_cached(self.h, _ptr(pixels), dtype_code(pixels.dtype), B, T, _ptr(ids), ids.stride(0), cache, s),
                       "encode_context_cached")
            self._record(pixels, ids)

    def tokenize_frames(self, frames, cache, ids):
        """``ivg_tokenize_frames``: ``frames`` (B, n, 3, H, W) against the filled encoder cache -> columns [0, 17 n) of ``ids`` (B, >= 17 n)."""
        B, n = frames.shape[:2]
        with self.stream() as s:
            self.check(self.lib.ivg_tokenize_frames(self.h, _ptr(frames), dtype_code(frames.dtype), B, n, cache, _ptr(ids), ids.stride(0), s),
                       "tokenize_frames")
            self._record(frames, ids)

    def detokenize(self, ids, F, out, cache=None, cache_mode=0, clamp=False):
        if clamp != self._clamp_out:   # clamp(0, 1) in the epilogue of the decoders' last convolution (engine state, rarely toggled)
            self.check(self.lib.ivg_set_output_clamp(self.h, int(bool(clamp))), "set_output_clamp")
            self._clamp_out = bool(clamp)
        with self.stream() as s:
            self.check(self.lib.ivg_detokenize_to(self.h, _ptr(ids), ids.shape[0], int(F), _ptr(out), dtype_code(out.dtype), cache, int(cache_mode), s),
                       "detokenize")
            ids.record_stream(self._run); out.record_stream(self._run)

    def detokenize_shared(self, ids, group_size, F, out, clamp=False):
        """ivg_detokenize_shared: rows of ``ids`` / ``out`` in groups of ``group_size`` consecutive trajectories with the same context tokens."""
        if clamp != self._clamp_out:
            self.check(self.lib.ivg_set_output_clamp(self.h, int(bool(clamp))), "set_output_clamp")
            self._clamp_out = bool(clamp)
        with self.stream() as s:
            self.check(self.lib.ivg_detokenize_shared(self.h, _ptr(ids), ids.shape[0] // int(group_size), int(group_size), int(F), _ptr(out),
                                                      dtype_code(out.dtype), s), "detokenize_shared")
            ids.record_stream(self._run); out.record_stream(self._run)

    def cache_create(self, B):
        h = C.c_void_p()
        self.check(self.lib.ivg_cache_create(self.h, int(B), C.byref(h)), "cache_create")
        self._caches.add(h.value)
        return h

    def cache_destroy(self, h):
        if self.h is not None and h.value in self._caches:   # (already released when the engine was closed first)
            self._caches.discard(h.value)
            self.lib.ivg_cache_destroy(self.h, h)

    def cache_select(self, h, parents):
        """``ivg_cache_select``: a new detokenizer cache whose row i is row ``parents[i]`` (host integers) of cache ``h``; ``h`` is unchanged."""
        p = np.ascontiguousarray(parents, dtype=np.int32)
        out = C.c_void_p()
        with self.stream() as s:
            self.check(self.lib.ivg_cache_select(self.h, h, p.ctypes.data_as(C.c_void_p), int(p.size), C.byref(out), s), "cache_select")
        self._caches.add(out.value)
        return out

    def kv_select(self, parents):
        """``ivg_kv_select``: new row i of the kept K / V cache := old row ``parents[i]`` (host integers).  Enqueued, no synchronisation."""
        p = np.ascontiguousarray(parents, dtype=np.int32)
        with self.stream() as s:
            self.check(self.lib.ivg_kv_select(self.h, p.ctypes.data_as(C.c_void_p), int(p.size), s), "kv_select")
        return self

    def kv_snapshot(self):
        """``ivg_kv_snapshot_create``: -> ``KeptCache``, a copy of the kept K / V cache in device memory of its own.  Enqueued."""
        h = C.c_void_p()
        with self.stream() as s:
            self.check(self.lib.ivg_kv_snapshot_create(self.h, C.byref(h), s), "kv_snapshot_create")
        return KeptCache(self.lib, h)

    def kv_restore(self, kept, parents=None):
        """``ivg_kv_snapshot_restore``: row i of the kept K / V cache := row ``parents[i]`` (host integers; None: every row) of ``kept``."""
        if kept.h is None:
            raise ValueError("kv_restore: the KeptCache is closed")
        p = np.ascontiguousarray(parents, dtype=np.int32) if parents is not None else None
        with self.stream() as s:
            self.check(self.lib.ivg_kv_snapshot_restore(self.h, kept.h, p.ctypes.data_as(C.c_void_p) if p is not None else None,
                                                        int(p.size) if p is not None else 0, s), "kv_snapshot_restore")
        return self

    def kv_extend(self, prompt, keep_len, actions=None, ctx=1, token_nll=None, token_scores=None, frame_rewards=None, frame_hidden=None):
        """``ivg_kv_extend``: positions [keep_len, L0 - 1) of ``prompt`` (B, L0) teacher-forced onto the kept K / V cache (``keep_len`` ==
        L0 - 1: a rewind); ``token_nll`` (B, L0 - 1 - keep_len) float32 receives the model's surprise at each given token.  With
        ``token_scores`` (B, T, 3) float32, ``frame_rewards`` (B, F_out) float32 or ``frame_hidden`` (B, F_out, hidden) in the llm dtype
        the call is ``ivg_kv_extend_scored``'s (``transformer.extend_frames`` gives F_out)."""
        B, L0 = prompt.shape
        act_T = actions.shape[1] if actions is not None else 0
        with self.stream() as s:
            if token_scores is None and frame_rewards is None and frame_hidden is None:
                self.check(self.lib.ivg_kv_extend(self.h, _ptr(prompt), prompt.stride(0), B, int(keep_len), L0, _ptr(actions), act_T, int(ctx),
                                                  _ptr(token_nll), s), "kv_extend")
            else:
                self.check(self.lib.ivg_kv_extend_scored(self.h, _ptr(prompt), prompt.stride(0), B, int(keep_len), L0, _ptr(actions), act_T, int(ctx),
                                                         _ptr(token_nll), _ptr(token_scores), _ptr(frame_rewards), _ptr(frame_hidden), s),
                           "kv_extend_scored")
            self._record(prompt, actions, token_nll, token_scores, frame_rewards, frame_hidden)
        return self

    def rollout(self, prompt, n_new, out, *, actions=None, ctx=1, uniforms=None, top_k=100, group_size=1, reuse_kv=False, force_sdf=False,
                fanout=False, reward=None, frame_rewards=None, frame_hidden=None, token_scores=None, filtered_scores=None):
        """One rollout from an id prompt through the entry ``rollout_entry`` names: ``prompt`` (B, L0) -> ``out`` (B, L0 + n_new).
        ``group_size`` > 1 (ivg_generate_shared) and ``fanout`` (ivg_generate_fanout, the groups' prefix is the kept K / V cache):
        ``prompt`` holds one row per group and everything else B = groups * group_size rows, row g * group_size + k = sample k of
        prompt g.  ``reuse_kv``: ivg_generate_continue's kept cache.  ``force_sdf``: the forced-sdf schedule without actions.
        Outputs beside the tokens: ``reward`` (B) float32 at the last forward pass; ``frame_rewards`` (B, n_new // 17) float32 and
        ``frame_hidden`` (B, n_new // 17, hidden) in the llm dtype at the 16th token of every frame that was fed; ``token_scores``
        (B, n_new, 3) float32, logprob, entropy and max_logprob of every decided new token (zeros on forced columns);
        ``filtered_scores`` (B, n_new, 4) float32, the same tokens under the temperature / top-k / top-p distribution they were drawn
        from: the entry is then the ``_filtered`` sibling of the scored or fan-out entry (include/ivg.h ivg_generate_filtered)."""
        filtered = filtered_scores is not None
        name = rollout_entry(fanout, filtered or token_scores is not None, frame_rewards is not None or frame_hidden is not None, group_size,
                             reuse_kv, force_sdf, reward is not None, actions is not None)
        rows, L0 = prompt.shape
        act = (_ptr(actions), actions.shape[1] if actions is not None else 0, int(ctx))
        sample = (_ptr(uniforms), int(top_k))
        if name == "ivg_generate_fanout" or name == "ivg_generate_shared":
            args = (rows, int(group_size), L0, int(n_new), *act, *sample, int(bool(force_sdf)), _ptr(out))
            args += (_ptr(reward),) if name == "ivg_generate_shared" else (_ptr(frame_rewards), _ptr(frame_hidden), _ptr(token_scores))
            args += (_ptr(filtered_scores),) if filtered else ()
        elif name == "ivg_generate_scored" or name == "ivg_generate_frames":
            args = (out.shape[0], L0, int(n_new), *act, *sample, int(group_size), int(bool(reuse_kv)), int(bool(force_sdf)), _ptr(out),
                    _ptr(frame_rewards), _ptr(frame_hidden))
            args += (_ptr(token_scores),) if name == "ivg_generate_scored" else ()
            args += (_ptr(filtered_scores),) if filtered else ()
        elif name == "ivg_generate_forced_sdf":
            args = (rows, L0, int(n_new), int(ctx), *sample, _ptr(out))
        else:   # ivg_generate, ivg_generate_continue
            args = (rows, L0, int(n_new), *act, *sample, _ptr(out), _ptr(reward))
        with self.stream() as s:
            self.check(getattr(self.lib, _FILTERED_ENTRY[name] if filtered else name)(self.h, _ptr(prompt), prompt.stride(0), *args, s),
                       "generate" if name == "ivg_generate_continue" else name[4:])
            self._record(prompt, out, actions, uniforms, reward, frame_rewards, frame_hidden, token_scores, filtered_scores)

    def embed_tokens(self, ids, out):
        B, L = ids.shape
        with self.stream() as s:
            self.check(self.lib.ivg_embed_tokens(self.h, _ptr(ids), ids.stride(0), B, L, _ptr(out), s), "embed_tokens")
            ids.record_stream(self._run); out.record_stream(self._run)

    def action_linear(self, actions, out):
        with self.stream() as s:
            self.check(self.lib.ivg_action_linear(self.h, _ptr(actions), actions.numel() // actions.shape[-1], _ptr(out), s), "action_linear")
            actions.record_stream(self._run); out.record_stream(self._run)

    def reward_linear(self, hidden, out):
        with self.stream() as s:
            self.check(self.lib.ivg_reward_linear(self.h, _ptr(hidden), hidden.numel() // hidden.shape[-1], _ptr(out), s), "reward_linear")
            hidden.record_stream(self._run); out.record_stream(self._run)

    def generate_embeds(self, embeds, n_new, out, hidden=None, uniforms=None, top_k=100, allow_reuse=True, token_scores=None, filtered_scores=None):
        """-> True when the kept KV cache was reused (only the last row of ``embeds`` was fed).  ``token_scores`` (B, n_new, 3) float32:
        ivg_generate_embeds_scored instead, which also leaves logprob, entropy and max_logprob of every new token; ``filtered_scores``
        (B, n_new, 4) float32: ivg_generate_embeds_filtered, which takes both."""
        B, L0 = embeds.shape[:2]
        reused = C.c_int(0)
        with self.stream() as s:
            if filtered_scores is not None:
                self.check(self.lib.ivg_generate_embeds_filtered(self.h, _ptr(embeds), B, L0, int(n_new), _ptr(uniforms), int(top_k), _ptr(out),
                                                                 _ptr(hidden), int(bool(allow_reuse)), C.byref(reused), _ptr(token_scores),
                                                                 _ptr(filtered_scores), s), "generate_embeds_filtered")
            elif token_scores is None:
                self.check(self.lib.ivg_generate_embeds(self.h, _ptr(embeds), B, L0, int(n_new), _ptr(uniforms), int(top_k), _ptr(out),
                                                        _ptr(hidden), int(bool(allow_reuse)), C.byref(reused), s), "generate_embeds")
            else:
                self.check(self.lib.ivg_generate_embeds_scored(self.h, _ptr(embeds), B, L0, int(n_new), _ptr(uniforms), int(top_k), _ptr(out),
                                                               _ptr(hidden), int(bool(allow_reuse)), C.byref(reused), _ptr(token_scores), s),
                           "generate_embeds_scored")
            self._record(embeds, out, hidden, uniforms, token_scores, filtered_scores)
        return bool(reused.value)

    def logits(self, ids, out, actions=None, ctx=1):
        B, L = ids.shape
        act_T = actions.shape[1] if actions is not None else 0
        with self.stream() as s:
            self.check(self.lib.ivg_logits(self.h, _ptr(ids), B, L, _ptr(actions), act_T, int(ctx), _ptr(out), s), "logits")
            self._record(ids, out, actions)

    def eval_forward(self, ids, labels, token_nll, loss_rows, actions=None, ctx=1, hidden=None):
        B, L = ids.shape
        act_T = actions.shape[1] if actions is not None else 0
        with self.stream() as s:
            self.check(self.lib.ivg_eval_forward(self.h, _ptr(ids), _ptr(labels), B, L, _ptr(actions), act_T, int(ctx), _ptr(token_nll),
                                                 _ptr(loss_rows), _ptr(hidden), s), "eval_forward")
            self._record(ids, labels, token_nll, loss_rows, actions, hidden)

    def action_recon_sqerr(self, hidden, actions, ctx, prelude, out):
        B, L = hidden.shape[:2]
        with self.stream() as s:
            self.check(self.lib.ivg_action_recon_sqerr(self.h, _ptr(hidden), _ptr(actions), B, L, actions.shape[1], int(ctx), int(prelude),
                                                       _ptr(out), s), "action_recon_sqerr")
            self._record(hidden, actions, out)

    def profile_enable(self, kclass, on=True):
        self.check(self.lib.ivg_profile_enable(self.h, kclass, int(on)), "profile_enable")

    def profile_attn_fit(self):
        """(fixed microseconds per launch, streaming GB/s) of the decode attention, after profile_read(IVG_K_DECODE_ATTN)."""
        f, r = C.c_double(0), C.c_double(0)
        self.check(self.lib.ivg_profile_attn_fit(self.h, C.byref(f), C.byref(r)), "profile_attn_fit")
        return f.value, r.value

    def profile_gemm_kinds(self):
        """{kind: (mean launch window in us, launches)} of the decode-step GEMMs, after profile_read(IVG_K_DECODE_GEMM)."""
        us, n = (C.c_double * 5)(), (C.c_int64 * 5)()
        self.check(self.lib.ivg_profile_gemm_kinds(self.h, us, n), "profile_gemm_kinds")
        return {k: (us[i], n[i]) for i, k in enumerate(("qkv", "o_proj", "gate_up", "down", "lm_head"))}

    def profile_read(self, kclass):
        st = _lib.IvgProfileStats()
        self.check(self.lib.ivg_profile_read(self.h, kclass, C.byref(st)), "profile_read")
        return dict(launches=st.launches, total_ms=st.total_ms, total_flops=st.total_flops, total_bytes=st.total_bytes)
