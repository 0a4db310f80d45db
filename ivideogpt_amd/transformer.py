"""Drop-in mirrors of the transformer-side objects the reference's callers use:

  * ``LlamaForCausalLM``   -- what ``AutoModelForCausalLM.from_pretrained(path, subfolder='transformer')``
    returns in inference/predict.py:111-113 (``.generate(input_ids, do_sample, temperature, top_k,
    max_new_tokens, pad_token_id)`` -> prompt + new tokens; ``.config.vocab_size``).
  * ``HeadModelWithAction`` -- /root/reference/ivideogpt/transformer/action_model.py:8-121, same
    constructor signature, ``load_state_dict(load_file(...), strict=True)``, ``generate(..., action=...)``,
    ``token_for_sdf``.

Sampling: ``torch.multinomial`` streams are device- and version-specific even inside the reference, so the
engine draws by inverse CDF from explicit uniforms (``torch.rand`` on the model's device, default or
supplied generator) over the top-k kept tokens in ascending id order; ``do_sample=False`` is greedy argmax.
All compute is in libivg (HIP); this file is tensor plumbing and checkpoint I/O.
"""
import math
from types import SimpleNamespace
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib
from . import weights as W
from .engine import Engine
from .packing import dtype_code, is_x3, pack_llama, torch_dtype


class _Embedding:
    """What ``llm.get_input_embeddings()`` returns (an ``nn.Embedding`` in HF): callable on int64 ids -> (…, hidden) rows of
    ``model.embed_tokens.weight`` in the engine's transformer dtype (libivg ``ivg_embed_tokens``)."""

    def __init__(self, llm):
        self._llm = llm

    def __call__(self, input_ids):
        llm = self._llm
        ids = input_ids.to(device=llm.device, dtype=torch.int64)
        shape = ids.shape
        ids2 = ids.reshape(-1, shape[-1]).contiguous() if ids.dim() > 1 else ids.reshape(1, -1).contiguous()
        out = torch.empty(*ids2.shape, llm._cfg["hidden_size"], dtype=llm.torch_dtype, device=llm.device)
        llm._ensure(ids2.shape[0]).embed_tokens(ids2, out)
        return out.reshape(*shape, -1)

    forward = __call__


class _ActionLinear:
    """``HeadModelWithAction.action_linear`` (action_model.py:36): float (…, action_dim) -> (…, hidden), transformer dtype."""

    def __init__(self, llm):
        self._llm = llm

    def __call__(self, action):
        llm = self._llm
        a = action.to(device=llm.device, dtype=torch.float32).contiguous()
        out = torch.empty(*a.shape[:-1], llm._cfg["hidden_size"], dtype=llm.torch_dtype, device=llm.device)
        llm._ensure(max(1, a.shape[0] if a.dim() > 1 else 1)).action_linear(a, out)
        return out

    forward = __call__


class _RewardLinear:
    """``HeadModelWithAction.reward_linear`` (action_model.py:41): post-norm hidden states (…, hidden) -> float32 (…, 1)."""

    def __init__(self, llm):
        self._llm = llm

    def __call__(self, hidden):
        llm = self._llm
        h = hidden.to(device=llm.device, dtype=llm.torch_dtype).contiguous()
        out = torch.empty(*h.shape[:-1], 1, dtype=torch.float32, device=llm.device)
        llm._ensure(max(1, h.shape[0] if h.dim() > 1 else 1)).reward_linear(h, out)
        return out

    forward = __call__


def shared_prompt_groups(ids, repeat_times):
    """The reference's multi-sample callers build their prompts as ``gen_input.repeat(t, 1)`` (inference/predict.py:65,
    train_gpt.py:170,179): row ``k * B0 + b`` is sample k of prompt b.  ``repeat_times``:
      * an int t > 1 -- the caller says so; checked on the device (one comparison kernel + a host read: a generate call is >= 100 ms);
      * ``"auto"`` -- detect it: the largest t dividing B for which rows b, b + B0, ... are equal (1: nothing shared).
    -> (t, B0).  Raises ValueError when an explicit t does not describe ``ids``."""
    B = ids.shape[0]
    if repeat_times == "auto":
        for t in range(B, 1, -1):
            if B % t == 0 and torch.equal(ids.reshape(t, B // t, -1), ids[:B // t].unsqueeze(0).expand(t, -1, -1)):
                return t, B // t
        return 1, B
    t = int(repeat_times)
    if t <= 1:
        return 1, B
    if B % t != 0 or not torch.equal(ids.reshape(t, B // t, -1), ids[:B // t].unsqueeze(0).expand(t, -1, -1)):
        raise ValueError(f"shared_context={t}: input_ids is not `prompts.repeat({t}, 1)` (rows b, b + B/{t}, ... must be identical)")
    return t, B // t


def _to_group_major(x, t, B0):
    """rows (k * B0 + b) -> rows (b * t + k): the engine keeps the t samples of a prompt in consecutive rows"""
    if x is None or t == 1 or B0 == 1:
        return x
    return x.view(t, B0, *x.shape[1:]).transpose(0, 1).reshape(x.shape).contiguous()


def _from_group_major(x, t, B0):
    if x is None or t == 1 or B0 == 1:
        return x
    return x.view(B0, t, *x.shape[1:]).transpose(0, 1).reshape(x.shape).contiguous()


class TokenScores(NamedTuple):
    """``generate(..., output_token_scores=True)``: how sure the MODEL was at every new token (include/ivg.h ivg_generate_scored), each
    float32 (B, max_new_tokens), natural logarithms, of the raw logits row ``z`` the sampler read -- before temperature, top-k and top-p
    (HF's ``output_logits`` / ``compute_transition_scores(..., normalize_logits=True)``): ``logprob = z[tok] - logsumexp(z)``,
    ``entropy`` of ``softmax(z)``, ``max_logprob = max(z) - logsumexp(z)``.  Forced ``sdf`` columns are exactly 0 in all three."""
    logprob: torch.Tensor
    entropy: torch.Tensor
    max_logprob: torch.Tensor

    def per_frame(self):
        """-> ``(frame_logprob, frame_entropy)``, each (B, F), ``F = (max_new_tokens + 1) // 17``: the SUM of ``logprob`` and the MEAN of
        ``entropy`` over each frame's 16 sampled tokens (the 17th column of a frame, the forced ``sdf`` and its zeros, is left out).
        Added column by column in one order, so that a frame of a long call and the same frame of a 17-token call give the same bits."""
        n = self.logprob.shape[1]
        F = (n + 1) // 17
        if F < 1:
            raise ValueError(f"per_frame needs at least one frame of 16 tokens, not {n} columns")
        col = torch.arange(F, device=self.logprob.device) * 17
        lp, en = self.logprob[:, col], self.entropy[:, col]
        for k in range(1, 16):
            lp, en = lp + self.logprob[:, col + k], en + self.entropy[:, col + k]
        return lp, en / 16


class FilteredTokenScores(NamedTuple):
    """``generate(..., output_filtered_scores=True)``: every new token under the distribution it was DRAWN from -- the logits row after
    temperature, top-k and top-p (include/ivg.h ivg_generate_filtered; HF's ``output_scores`` /
    ``compute_transition_scores(..., normalize_logits=True)``), each float32 (B, max_new_tokens), natural logarithms: ``logprob`` of the
    token under the filtered distribution (the proposal log-probability of an importance weight), ``entropy`` of that distribution,
    ``kept_logmass`` = log of the share of the tempered softmax the filter kept (<= 0; ``logprob + kept_logmass`` is the tempered raw
    log-probability), ``support`` = the number of tokens that could have been drawn.  Greedy calls: no filter, the raw row.  Forced
    ``sdf`` columns are exactly 0 in all four."""
    logprob: torch.Tensor
    entropy: torch.Tensor
    kept_logmass: torch.Tensor
    support: torch.Tensor

    def per_frame(self):
        """-> ``(frame_logprob, frame_entropy)``, each (B, F): the SUM of ``logprob`` and the MEAN of ``entropy`` over each frame's 16
        sampled tokens, in the column order of ``TokenScores.per_frame``."""
        return TokenScores.per_frame(self)


def _token_scores_buffer(B, n_new, device):
    return torch.empty(B, n_new, 3, dtype=torch.float32, device=device)


def _token_scores_of(ts, t=1, B0=1, n=None):
    """(B, n_new, 3) in the engine's row order -> TokenScores of (B, n) in the caller's"""
    ts = _from_group_major(ts, t, B0)
    return TokenScores(*(ts[:, :n, k].contiguous() for k in range(3)))


def _filtered_scores_of(fs, t=1, B0=1, n=None):
    """(B, n_new, 4) in the engine's row order -> FilteredTokenScores of (B, n) in the caller's"""
    fs = _from_group_major(fs, t, B0)
    return FilteredTokenScores(*(fs[:, :n, k].contiguous() for k in range(4)))


class ExtendOutputs(NamedTuple):
    """``extend_kept_cache`` with any of ``output_frame_hidden_states``, ``output_token_scores``, ``return_reward="frames"``
    (include/ivg.h ivg_kv_extend_scored): what the model thinks of the tokens it was GIVEN.  ``token_nll`` (B, T) as ``return_nll``;
    ``frame_rewards`` (B, F) and ``frame_hidden`` (B, F, hidden) for the F frames whose 16th token the call fed (``extend_frames``);
    ``token_scores``: ``TokenScores`` of (B, T), column c scoring ``input_ids[:, keep + c + 1]``.  None what was not asked for."""
    token_nll: Optional[torch.Tensor]
    frame_rewards: Optional[torch.Tensor]
    frame_hidden: Optional[torch.Tensor]
    token_scores: Optional[TokenScores]


def extend_frames(keep, L0, ctx):
    """-> ``(i_first, F_out)``: the predicted frames (0-based after the ``ctx`` context frames) whose 16th token, position
    ``257 * ctx + 17 * i + 15``, is among the positions [keep, L0 - 1) an ``extend_kept_cache(input_ids (B, L0), keep=keep)`` feeds --
    frames ``i_first .. i_first + F_out - 1``, the columns of its frame outputs."""
    q0 = 257 * int(ctx) + 15
    first = 0 if keep <= q0 else (keep - q0 + 16) // 17
    if L0 - 2 < q0:
        return first, 0
    return first, max(0, (L0 - 2 - q0) // 17 - first + 1)


def _top_p_of(top_p, do_sample):
    """The engine's ``top_p`` for a generate call, checked before any engine work as HF does: only when sampling (HF builds its
    TopPLogitsWarper only then, so ``do_sample=False`` ignores any value), after ``float(top_p)`` (numpy scalars, 0-d tensors and
    numeric strings are accepted), ValueError outside [0, 1].  One difference: NaN raises too (HF's range test lets it through and
    filters nothing).  ``None`` -> 1.0, no filter."""
    if top_p is None or not do_sample:
        return 1.0
    p = float(top_p)
    if not (0.0 <= p <= 1.0):
        raise ValueError(f"`top_p` has to be a float >= 0 and <= 1, but is {top_p}")
    return p


def _check_temperature(temperature):
    if not (isinstance(temperature, (int, float)) and temperature > 0):   # HF's TemperatureLogitsWarper raises the same way
        raise ValueError(f"`temperature` (={temperature}) has to be a strictly positive float")


def _result(*values):
    """What a generate call returns: the values it was asked for (the others are None), a single one bare."""
    res = tuple(v for v in values if v is not None)
    return res if len(res) > 1 else res[0]


KV_CACHE_DTYPES = ("auto", "fp8_e4m3")


def _kv_scale_checked(what, s):
    try:
        f = float(s)
    except (TypeError, ValueError):
        f = float("nan")
    if not (math.isfinite(f) and f > 0.0 and math.frexp(f)[0] == 0.5 and 2.0 ** -126 <= f <= 2.0 ** 126):
        raise ValueError(f"{what} must be a finite, positive power of two in [2^-126, 2^126], not {s!r}")
    return f


def _kv_cache_setting(name, k_scale, v_scale, dtype, cfg, scales=None):
    """The (name, k_scale, v_scale) of ``kv_cache_dtype`` / ``set_kv_cache_dtype``, checked before any engine work (include/ivg.h
    ivg_set_kv_format): ValueError for an unknown name, a scale that is not a finite positive power of two in [2^-126, 2^126], or
    ``"fp8_e4m3"`` on a model that is not bf16 with head_dim 64.  With ``scales`` -- a (layers, 2, heads) tensor or nested list, every
    entry such a power of two (ivg_set_kv_scales) -- the result has a fourth element, the table as nested tuples; ValueError for a
    wrong shape or entry, for ``scales`` together with a non-default ``k_scale`` / ``v_scale``, or on a model the FP8 cache is not for."""
    if name not in KV_CACHE_DTYPES:
        raise ValueError(f"kv_cache_dtype must be one of {KV_CACHE_DTYPES}, not {name!r}")
    ks, vs = _kv_scale_checked("k_scale", k_scale), _kv_scale_checked("v_scale", v_scale)
    hd = cfg["hidden_size"] // max(1, cfg["num_attention_heads"])
    fp8_model = not is_x3(dtype) and dtype_code(dtype) == _lib.IVG_BF16 and hd == 64
    if name == "fp8_e4m3" and not fp8_model:
        raise ValueError(f"kv_cache_dtype='fp8_e4m3' needs a bf16 model with head_dim 64 (this one: dtype {dtype!r}, head_dim {hd})")
    if scales is None:
        return name, ks, vs
    if (ks, vs) != (1.0, 1.0):
        raise ValueError("pass either scales (per layer and head) or k_scale / v_scale, not both")
    if not fp8_model:
        raise ValueError(f"K / V scales need a bf16 model with head_dim 64 (this one: dtype {dtype!r}, head_dim {hd})")
    shape = (cfg["num_hidden_layers"], 2, cfg["num_attention_heads"])
    try:
        t = torch.as_tensor(scales, dtype=torch.float32).cpu()
    except (TypeError, ValueError, RuntimeError):
        raise ValueError(f"scales must be a tensor or nested list of shape {shape}") from None
    if tuple(t.shape) != shape:
        raise ValueError(f"scales must have shape {shape} (layers, k|v, heads), not {tuple(t.shape)}")
    table = tuple(tuple(tuple(_kv_scale_checked(f"scales[{l}][{w}][{h}]", x) for h, x in enumerate(row)) for w, row in enumerate(lay))
                  for l, lay in enumerate(t.tolist()))
    return name, ks, vs, table


def normalize_parents(parents, rows=None):
    """``parents`` of a row selection (a list, a numpy array or a tensor of integers, one dimension, at least one entry) -> a
    contiguous int32 numpy array on the host.  A device tensor is copied to the host, which synchronises.  ValueError for anything
    else: another shape, no entry, a type that is not an integer type (bool included), and -- with ``rows`` -- an entry outside
    ``[0, rows)``."""
    if isinstance(parents, torch.Tensor):
        if parents.dtype in (torch.bool,) or parents.is_floating_point() or parents.is_complex():
            raise ValueError(f"parents must hold integers, not {parents.dtype}")
        a = parents.detach().cpu().numpy()
    else:
        a = np.asarray(parents)
        if a.size == 0 and a.ndim == 1:
            raise ValueError("parents must hold at least one row")
        if a.dtype.kind not in "iu":
            raise ValueError(f"parents must hold integers, not {a.dtype}")
    if a.ndim != 1 or a.size == 0:
        raise ValueError(f"parents must be one-dimensional with at least one row, not of shape {tuple(a.shape)}")
    lo, hi = int(a.min()), int(a.max())
    if lo < 0 or hi > 2 ** 31 - 1 or (rows is not None and hi >= rows):
        raise ValueError(f"every parent must be a row index in [0, {rows if rows is not None else 2 ** 31}), not {lo if lo < 0 else hi}")
    return np.ascontiguousarray(a, dtype=np.int32)


def stable_parents(parents, B):
    """The same multiset of ``parents`` (rows of a batch of ``B``), arranged so that every surviving parent keeps its own row wherever
    possible: ``arranged[v] == v`` for every value ``v < len(parents)`` that occurs in ``parents`` -- the largest number of fixed points
    any arrangement has -- and the other entries fill the remaining rows in their original order.  ``select_kept_cache(arranged)`` then
    copies every moved row in place from a row that stays (ivg_kv_select: direct moves only, nothing staged).
    -> ``(arranged, perm)``, int64 CPU tensors with ``arranged == parents[perm]``: ``perm`` reorders whatever the caller keeps per
    CHOSEN row (weights, ranks) the same way."""
    p = normalize_parents(parents, B)
    n = p.size
    perm = np.full(n, -1, dtype=np.int64)
    used = np.zeros(n, dtype=bool)
    for j, v in enumerate(p):          # the first copy of every surviving parent goes to the parent's own row
        if v < n and perm[v] < 0:
            perm[v] = j
            used[j] = True
    rest = iter(np.flatnonzero(~used))
    for i in range(n):
        if perm[i] < 0:
            perm[i] = next(rest)
    return torch.from_numpy(p[perm].astype(np.int64)), torch.from_numpy(perm)


class LlamaForCausalLM:
    supports_shared_context = True   # generate / detokenize accept shared_context= (libivg ivg_generate_shared / ivg_detokenize_shared)
    def __init__(self, config, state_dict=None, dtype="bf16", prefix="", action_dim=None, reward_prediction=False, decode_lds_kb=0,
                 max_seq=0, kv_cache_dtype="auto"):
        self._decode_lds_kb = int(decode_lds_kb or 0)   # launch policy of THIS model's engine (set_decode_lds_kb)
        self._max_seq = int(max_seq or 0)               # KV-cache length (0: max_position_embeddings; never more, ivg_config.max_seq)
        self._cfg = dict(W.LLAMA_SMALL)
        self._cfg.update({k: v for k, v in dict(config).items() if k in self._cfg})
        self.config = SimpleNamespace(**self._cfg)
        self.config.n_embd = self._cfg["hidden_size"]
        self._sd, self._prefix = state_dict, prefix
        self._action_dim, self._reward = action_dim, reward_prediction
        self.dtype = dtype
        self.torch_dtype = torch_dtype(dtype_code(dtype))
        self.device = torch.device("cpu")
        self._engine = None
        self._kv = _kv_cache_setting(kv_cache_dtype, 1.0, 1.0, dtype, self._cfg)   # K / V cache format of this model's engines (set_kv_cache_dtype)
        # the packed weights in HBM, kept across engine rebuilds and shared by replicas.  Validity is an explicit version counter
        # bumped by every load_state_dict (never id(dict): a reloaded or in-place mutated dict keeps its id, a collected one's is reused)
        self._packed, self._packed_key, self._sd_version = None, None, 0

    def _pack_key(self):
        return (self._sd_version, self._prefix, str(self.device), self.dtype)

    def _invalidate_pack(self):
        """Called whenever the weights, their key prefix or the device change: the old pack is released with the engine that used it."""
        self._sd_version += 1
        self._packed, self._packed_key = None, None

    def _packed_weights(self):
        if self._packed is None or self._packed_key != self._pack_key():
            self._packed = pack_llama(self._sd, self._cfg, self.device, dtype_code(self.dtype), prefix=self._prefix)
            self._packed_key = self._pack_key()
        return self._packed

    def replica(self):
        """A second model object over the SAME weights in HBM (the engine only reads them): its own engine -- KV cache, workspace --
        for a second batch in flight on another stream / host thread (bench.py --lanes; INTEGRATION.md, streams)."""
        if self.device.type != "cuda":
            raise RuntimeError("replica(): call .to('cuda') first")
        r = LlamaForCausalLM(self._cfg, self._sd, dtype=self.dtype, prefix=self._prefix, action_dim=self._action_dim,
                             reward_prediction=self._reward, decode_lds_kb=self._decode_lds_kb, max_seq=self._max_seq)
        r._kv = self._kv
        r.device = self.device
        r._sd_version = self._sd_version
        if hasattr(self, "_wrapper_heads"):
            r._wrapper_heads = self._wrapper_heads
        r._packed, r._packed_key = self._packed_weights(), self._pack_key()
        return r

    # HF keyword arguments of from_config / from_pretrained that have no meaning for an inference engine (eval semantics, one
    # attention implementation, local files only): accepted and ignored -- anything else raises TypeError
    _IGNORED_HF_KWARGS = frozenset({"trust_remote_code", "attn_implementation", "torch_dtype", "attention_dropout", "use_cache", "revision",
                                    "cache_dir", "local_files_only", "device_map", "use_safetensors", "token"})

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, subfolder="transformer", low_cpu_mem_usage=False, dtype="bf16",
                        kv_cache_dtype="auto", **unused):
        if kv_cache_dtype not in KV_CACHE_DTYPES:   # (before the checkpoint is read; the dtype / head_dim checks follow in __init__)
            raise ValueError(f"kv_cache_dtype must be one of {KV_CACHE_DTYPES}, not {kv_cache_dtype!r}")
        cfg, sd = W.load_transformer_checkpoint(pretrained_model_name_or_path, subfolder)
        W.validate_state_dict(sd, W.llama_param_shapes(cfg), "transformer")
        return cls(cfg, sd, dtype=dtype, kv_cache_dtype=kv_cache_dtype)

    @classmethod
    def from_config(cls, config, seed=None, dtype="bf16", kv_cache_dtype="auto", **hf_kwargs):
        """``AutoModelForCausalLM.from_config(config)`` (mbrl/video_predictor.py:72, train_gpt.py:593): ``config`` = a dict, an object
        with the HF field names, or a path to a ``config.json`` / its directory (what ``AutoConfig.from_pretrained`` takes).
        seed = None: no weights yet (load_state_dict follows); otherwise seeded random weights in the checkpoint schema.
        Of HF's keyword arguments only the ones with no meaning here are accepted (and ignored): a misspelt name raises."""
        unknown = set(hf_kwargs) - cls._IGNORED_HF_KWARGS
        if unknown:
            raise TypeError(f"from_config() got unexpected keyword argument(s) {sorted(unknown)}")
        if isinstance(config, (str, bytes)) or hasattr(config, "__fspath__"):
            config = W.load_llama_config(config)
        cfg = dict(W.LLAMA_SMALL)
        cfg.update({k: v for k, v in (vars(config) if not isinstance(config, dict) else config).items() if k in cfg})
        _kv_cache_setting(kv_cache_dtype, 1.0, 1.0, dtype, cfg)   # (a bad setting raises before any weights are drawn)
        sd = W.random_llama_state_dict(cfg, seed) if seed is not None else None
        return cls(cfg, sd, dtype=dtype, kv_cache_dtype=kv_cache_dtype)

    def state_dict(self):
        return self._sd

    def load_state_dict(self, sd, strict=True):
        if strict:
            W.validate_state_dict(sd, W.llama_param_shapes(self._cfg), "transformer")
        heads = getattr(self, "_wrapper_heads", None)
        if heads is not None:   # ``model.llm.load_state_dict(...)`` of a HeadModelWithAction (mbrl/video_predictor.py:82-83, load_internal_llm):
            # only the transformer's weights change, the wrapper's heads stay what they are
            old = self._sd if (self._sd is not None and self._prefix == "llm.") else None
            self._sd = HeadModelWithAction._with_fresh_heads(sd, self._cfg["hidden_size"], heads[0], heads[1], old=old)
            self._prefix = "llm."
        else:
            self._sd, self._prefix = sd, ""
        self._drop_engine()
        self._invalidate_pack()

    def save_pretrained(self, path, subfolder="transformer"):
        W.save_transformer_checkpoint(path, self._cfg, self._sd, subfolder)

    def to(self, device=None, *a, **k):
        if device is not None and not isinstance(device, torch.dtype):
            dev = torch.device(device)
            if dev.type == "cuda" and dev.index is None:
                dev = torch.device("cuda", torch.cuda.current_device())
            if dev != self.device:
                self.device = dev
                self._drop_engine()
                self._packed, self._packed_key = None, None   # the pack lives on the old device
        return self

    def cuda(self, index=None):
        return self.to(torch.device("cuda", index if index is not None else torch.cuda.current_device()))

    def eval(self):
        return self

    def _drop_engine(self):
        if self._engine is not None:
            self._engine.close()
        self._engine = None

    def _ensure(self, B, frames=32):
        e = self._engine
        if e is not None and B <= e.max_batch and frames <= e.max_frames:
            return e
        if self.device.type != "cuda":
            raise RuntimeError("call .to('cuda') first -- the engine runs on an MI355X only (no CPU path)")
        if self._sd is None:
            raise RuntimeError("model has no weights: use from_pretrained / load_state_dict")
        cap_b = max(B, e.max_batch if e else 0)
        cap_t = max(frames, e.max_frames if e else 0)
        self._drop_engine()
        self._engine = Engine(self.device, self._packed_weights(), llm_cfg=self._cfg, action_dim=self._action_dim or 0,
                              reward_head=self._reward, llm_dtype=self.dtype, max_batch=cap_b, max_frames=cap_t,
                              decode_lds_kb=self._decode_lds_kb, max_seq=self._max_seq)
        self._apply_kv(self._engine, fresh=True)
        return self._engine

    def _apply_kv(self, eng, fresh=False):
        """``self._kv`` -> the engine: the format with its uniform scales, then the table when there is one (set_kv_format drops a table)."""
        kv = self._kv
        if not fresh or kv[0] != "auto":
            eng.set_kv_format(_lib.IVG_KV_NATIVE if kv[0] == "auto" else _lib.IVG_KV_FP8_E4M3, kv[1], kv[2])
        if len(kv) > 3:
            eng.set_kv_scales(kv[3])

    def set_kv_cache_dtype(self, name, k_scale=1.0, v_scale=1.0, scales=None):
        """K / V cache format of this model's rollouts (include/ivg.h ivg_set_kv_format).  ``"auto"``: the model's own element type, the
        default.  ``"fp8_e4m3"`` (bf16 models with head_dim 64): an opt-in, lossy one-byte cache, element = e4m3(clamp(x / scale, +-448))
        with ``k_scale`` / ``v_scale`` powers of two, or with ``scales``: one power of two per (layer, k|v, head), a (layers, 2, heads)
        tensor or nested list -- what ``calibrate_kv_cache`` returns and ``kv_scales`` reads (ivg_set_kv_scales).  Without ``scales`` the
        scales are uniform and a table set earlier is dropped.  ValueError, before any engine work, for a wrong name, model dtype, scale
        or table, or for ``scales`` together with ``k_scale`` / ``v_scale``.  Applies to the live engine from its next generate call on
        -- whose kept KV cache it invalidates (``reuse_cache`` / ``use_cache`` callers start over) -- and to every engine this model
        builds later."""
        kv = _kv_cache_setting(name, k_scale, v_scale, self.dtype, self._cfg, scales)
        if kv != self._kv:
            self._kv = kv
            if self._engine is not None:
                self._apply_kv(self._engine)
        return self

    @property
    def kv_scales(self):
        """The K / V scales of this model's FP8 cache as a (layers, 2, heads) float32 CPU tensor: the table when one is set (``scales=``,
        ``calibrate_kv_cache``), else ``k_scale`` / ``v_scale`` expanded.  Read-only."""
        L, H = self._cfg["num_hidden_layers"], self._cfg["num_attention_heads"]
        if len(self._kv) > 3:
            return torch.tensor(self._kv[3], dtype=torch.float32)
        return torch.tensor([self._kv[1], self._kv[2]], dtype=torch.float32).view(1, 2, 1).expand(L, 2, H).contiguous()

    @torch.no_grad()
    def calibrate_kv_cache(self, input_ids, headroom=1, reset=True, _actions=None, _ctx=1):
        """Calibrates the FP8 cache's scales on the device (ivg_kv_calibrate / ivg_kv_calibration_finish): runs the teacher-forced prompt
        pass over ``input_ids (B, L)`` -- whole ground-truth token rows, so that it sees the positions a rollout appends --, takes
        max |K| and max |V| per (layer, head), and installs per (layer, k|v, head) the smallest power of two that keeps the maximum
        within +-448, times 2^``headroom`` (0 .. 8; the default leaves one bit for rows the calibration set did not contain: it costs no
        mantissa).  ``reset=False`` accumulates over several calls.  -> the scales, a (layers, 2, heads) float32 CPU tensor, also kept
        for rebuilt engines and ``replica()``; the observed maxima are in ``last_kv_amax``.  Does NOT switch the format on, and a later
        ``set_kv_cache_dtype`` without ``scales`` drops the table: turn the format on first, or pass ``scales=model.kv_scales``.
        Synchronises.  ValueError on a model the FP8 cache is not for; AssertionError (ivg_last_error names layer, tensor and head) when
        K or V held a NaN or Inf."""
        if not (isinstance(headroom, int) and 0 <= headroom <= 8):
            raise ValueError(f"headroom must be an integer in [0, 8], not {headroom!r}")
        _kv_cache_setting("fp8_e4m3", 1.0, 1.0, self.dtype, self._cfg)   # (the model check, before any engine work)
        ids = input_ids.to(device=self.device, dtype=torch.int64).contiguous()
        eng = self._ensure(ids.shape[0], _actions.shape[1] if _actions is not None else 32)
        eng.kv_calibrate(ids, actions=_actions, ctx=_ctx, reset=reset)
        self.last_kv_amax, scales = eng.kv_calibration_finish(headroom)
        self._kv = self._kv[:3] + (_kv_cache_setting("auto", 1.0, 1.0, self.dtype, self._cfg, scales)[3],)   # (the engine has it installed)
        return scales

    # LDS budget (KiB) of a decode-step GEMM workgroup for a model whose batch shares the GPU with other batches in flight (bench.py
    # --lanes, INTEGRATION.md "streams"): with a whole CU's LDS per workgroup (the default, fastest for one batch alone) the decode
    # GEMMs of one batch lock the other batches' kernels out of the CU for their whole duration; at <= 52 KiB three or four
    # workgroups of different engines fit, and four batches in flight reach 5,680 instead of 5,350 predicted frames/s
    # (profiles/r04_lanes.txt).  A property of the ENGINE (ivg_config.decode_lds_kb), not of the process: a latency-bound model
    # (MBRL step-wise rollout) and throughput lanes can live side by side.
    BATCHES_IN_FLIGHT_LDS_KB = 40

    def set_decode_lds_kb(self, kb):
        """``kb`` = 0: the process default (``IVG_DECODE_LDS_KB``, 160); 16 .. 160 otherwise.  Applies to the live engine and to every
        engine this model builds later; the budget picks the kernel generation, so tokens of two budgets are each deterministic
        but not bit-comparable with one another."""
        self._decode_lds_kb = int(kb or 0)
        if self._engine is not None:
            self._engine.set_decode_lds_kb(self._decode_lds_kb)
        return self

    def select_kept_cache(self, parents):
        """Resamples the KV cache the last ``generate`` call kept (include/ivg.h ivg_kv_select; HF: ``_reorder_cache``): row i of the
        kept cache becomes what row ``parents[i]`` was -- duplicates, drops, any order, and more rows than before up to the batch the
        engine was built for (the largest batch this model has run).  A following ``reuse_cache=True`` / ``use_cache=True`` call then
        accepts the prompt, actions or embeddings gathered by the same ``parents`` (``x[parents]``) and feeds only the last token;
        anything else is still refused by the on-device comparison.  ``parents``: a list, numpy array or tensor of integers; a device
        tensor is brought to the host, which synchronises -- the call itself only enqueues copies.  ``stable_parents`` arranges a
        resampling so that survivors stay in place, the cheapest case.  ValueError, with the kept cache untouched, when there is no
        kept cache (no call yet, a shared-context call, a change of the K / V format or scales since), for an index outside the kept
        rows, or for more rows than the engine holds."""
        p = normalize_parents(parents)
        if self._engine is None:
            raise ValueError("select_kept_cache: no kept cache (the model has not generated yet)")
        try:
            self._engine.kv_select(p)
        except (AssertionError, _lib.IvgError) as err:
            raise ValueError(f"select_kept_cache: {err}") from None
        return self

    def save_kept_cache(self):
        """Sets the KV cache the last ``generate`` call kept aside (include/ivg.h ivg_kv_snapshot_create; HF:
        ``copy.deepcopy(past_key_values)``) -> ``KeptCache``: a copy in device memory of its own -- ``.rows``, ``.length``, ``.nbytes``,
        ``.close()`` -- that survives whatever this model does next, its engine being rebuilt included.  The live kept cache is
        unchanged; the copy is enqueued.  ValueError when there is no kept cache (``select_kept_cache`` has the cases)."""
        if self._engine is None:
            raise ValueError("save_kept_cache: no kept cache (the model has not generated yet)")
        try:
            kept = self._engine.kv_snapshot()
        except (AssertionError, _lib.IvgError) as err:
            raise ValueError(f"save_kept_cache: {err}") from None
        kept.weights_version = self._pack_key()
        return kept

    def restore_kept_cache(self, kept, parents=None):
        """Brings a ``KeptCache`` back (ivg_kv_snapshot_restore): row i of this model's kept cache becomes row ``parents[i]`` of ``kept``
        (``select_kept_cache``'s ``parents``; None: every row), at the saved length -- continue with ``reuse_cache=True`` /
        ``use_cache=True`` on the prompt, actions or embeddings gathered by the same ``parents``, ``extend_kept_cache``, ``fan_out``,
        ``select_kept_cache``.  ``kept`` is unchanged and may be restored again, into this model, into the larger engine it builds when
        the restored rows need one (the only case in which this call builds an engine), or into a ``replica()``.  ValueError, with this
        model's kept cache as it was, where the engine refuses: a model with other weights or another config, a K / V format or FP8
        scale other than the saved one, a parent outside ``kept.rows``, more rows than the cache chunk (128) or more positions than
        ``max_seq`` holds."""
        if kept.closed:
            raise ValueError("restore_kept_cache: the KeptCache is closed")
        p = normalize_parents(parents, kept.rows) if parents is not None else None
        if kept.weights_version is not None and kept.weights_version != self._pack_key():
            raise ValueError("restore_kept_cache: the KeptCache was saved by a model with other weights (or on another device, or in another dtype)")
        n, frames = int(p.size) if p is not None else kept.rows, kept.act_T if kept.act_T > 0 else 32
        try:
            eng = self._engine
            if eng is None or (n <= 128 and (n > eng.max_batch or frames > eng.max_frames)):   # (more than the chunk: the engine refuses, nothing is rebuilt)
                eng = self._ensure(min(n, 128), frames)
            eng.kv_restore(kept, p)
        except (AssertionError, _lib.IvgError) as err:
            raise ValueError(f"restore_kept_cache: {err}") from None
        return self

    def extend_kept_cache(self, input_ids, keep, return_nll=False, output_frame_hidden_states=False, output_token_scores=False, _actions=None,
                          _ctx=1, _frame_rewards=False):
        """Appends GIVEN tokens to the KV cache the last ``generate`` call kept (include/ivg.h ivg_kv_extend): afterwards it holds
        ``input_ids[:, :-1]``, of which positions [0, keep) are the kept rows as they were (verified on the device) and [keep, L0 - 1)
        are teacher-forced by this call -- a following ``generate`` on the kept cache (``HeadModelWithAction.generate(reuse_cache=True)``),
        ``select_kept_cache``, ``fan_out`` or another extend then accepts ``input_ids``.  ``keep == L0 - 1`` only rewinds the cache to
        that length.  ``return_nll=True``: -> float32 (B, L0 - 1 - keep), ``-log p(input_ids[:, p + 1] | input_ids[:, :p + 1])`` for
        p = keep .. L0 - 2, the model's surprise at each given token; else None.  ``output_frame_hidden_states`` /
        ``output_token_scores`` (include/ivg.h ivg_kv_extend_scored): -> ``ExtendOutputs`` instead.  ValueError, with the kept cache
        untouched, where the engine refuses: no kept cache built from ids, another batch, ``keep`` outside [1, min(kept length, L0 - 1)],
        other tokens."""
        if self._engine is None:
            raise ValueError("extend_kept_cache: no kept cache (the model has not generated yet)")
        ids = input_ids.to(device=self.device, dtype=torch.int64).contiguous()
        B, L0 = ids.shape
        T = max(L0 - 1 - int(keep), 0)
        nll = torch.empty(B, T, dtype=torch.float32, device=self.device) if return_nll and T > 0 else None
        F = extend_frames(int(keep), L0, _ctx)[1] if T > 0 else 0
        ts = _token_scores_buffer(B, T, self.device) if output_token_scores else None
        fr = torch.empty(B, F, dtype=torch.float32, device=self.device) if _frame_rewards else None
        fh = torch.empty(B, F, self._cfg["hidden_size"], dtype=self.torch_dtype, device=self.device) if output_frame_hidden_states else None
        try:
            self._engine.kv_extend(ids, keep, actions=_actions, ctx=_ctx, token_nll=nll, token_scores=ts, frame_rewards=fr, frame_hidden=fh)
        except (AssertionError, _lib.IvgError) as err:
            raise ValueError(f"extend_kept_cache: {err}") from None
        if return_nll and nll is None:
            nll = torch.empty(B, 0, dtype=torch.float32, device=self.device)
        if ts is None and fr is None and fh is None:
            return nll if return_nll else None
        return ExtendOutputs(nll if return_nll else None, fr, fh, _token_scores_of(ts) if ts is not None else None)

    def _fan_out(self, ids, samples, act, ctx, gk, force_sdf=False):
        """``fan_out`` of both classes: ``ivg_generate_fanout`` under ``generate``'s keywords.  Rows b * samples + k throughout (the
        engine's group-major order is the public one here)."""
        known = {"do_sample", "temperature", "top_k", "max_new_tokens", "pad_token_id", "generator", "uniforms", "top_p", "output_token_scores",
                 "return_reward", "output_frame_hidden_states", "output_filtered_scores"}
        if set(gk) - known:
            raise TypeError(f"fan_out: unexpected keyword(s) {sorted(set(gk) - known)}")
        do_sample, temperature, top_k = gk.get("do_sample", True), gk.get("temperature", 1.0), gk.get("top_k", 100)
        n, rr, want_h, want_s = gk.get("max_new_tokens"), gk.get("return_reward", False), gk.get("output_frame_hidden_states", False), \
            gk.get("output_token_scores", False)
        _check_temperature(temperature)
        top_p = _top_p_of(gk.get("top_p"), do_sample)
        if not (isinstance(samples, int) and samples >= 1):
            raise ValueError(f"fan_out: samples must be a positive integer, not {samples!r}")
        if rr not in (False, "frames"):
            raise ValueError("fan_out: return_reward must be False or 'frames' (candidates are ranked frame by frame)")
        if rr == "frames" and not self._reward:
            raise ValueError("return_reward='frames' needs a model with reward_prediction=True")
        frames = rr == "frames" or want_h
        if frames:
            _frames_of(n)
        eng = self._engine
        B = ids.shape[0] * samples
        if eng is None:
            raise ValueError("fan_out: no kept cache (the model has not generated yet)")
        if B > eng.max_batch:
            raise ValueError(f"fan_out: {B} candidates exceed the batch the engine was built for ({eng.max_batch}); run the model once at that batch first")
        try:
            r = self._rollout(ids, n, (do_sample, temperature, top_k, top_p, gk.get("generator"), gk.get("uniforms")), act=act, ctx=ctx, fan=samples,
                              force_sdf=act is None and (frames or force_sdf), sdf_tail=frames, frame_rewards=rr == "frames", frame_hidden=want_h,
                              scores=want_s, filtered=gk.get("output_filtered_scores", False))
        except (AssertionError, _lib.IvgError) as err:
            raise ValueError(f"fan_out: {err}") from None
        return r.result(r.tokens.contiguous(), r.frame_rewards, r.frame_hidden, r.token_scores, r.filtered_scores)

    @torch.no_grad()
    def fan_out(self, input_ids, samples, **generate_kwargs):
        """``samples`` candidate continuations of every row of the kept KV cache (include/ivg.h ivg_generate_fanout): ``input_ids``
        (B, L0) is what the kept cache was built from plus the token to feed next, and row ``b * samples + k`` of every result is
        candidate k of row b.  No prompt pass: the candidates read the kept rows in place, and the kept cache is afterwards exactly
        what it was -- fan out again, continue, or ``extend_kept_cache``.  ``generate``'s keywords (``do_sample``, ``temperature``,
        ``top_k``, ``top_p``, ``max_new_tokens``, ``uniforms`` (B * samples, n), ``generator``, ``output_token_scores``,
        ``output_filtered_scores``); results as
        ``generate``'s.  ValueError where the engine refuses (no such kept cache, more candidates than the engine holds)."""
        ids = input_ids.to(device=self.device, dtype=torch.int64).contiguous()
        return self._fan_out(ids, samples, None, 1, generate_kwargs)

    # ------------------------------------------------------------------ hot path
    def _uniforms(self, B, n, do_sample, generator):
        if not do_sample:
            return None
        return torch.rand(B, n, device=self.device, dtype=torch.float32, generator=generator)

    def _sampling_engine(self, B, frames, temperature, top_p, existing=False):
        """The engine (``existing``: the live one, whose kept cache the call is about) with the call's temperature and top_p set."""
        eng = self._engine if existing else self._ensure(B, frames)
        return eng.set_temperature(temperature).set_top_p(top_p)

    def _rollout(self, ids, n, sampling, act=None, ctx=1, groups=None, fan=0, reuse_kv=False, force_sdf=False, sdf_tail=False, reward=False,
                 frame_rewards=False, frame_hidden=False, scores=False, filtered=False):
        """One ``Engine.rollout`` of ``n`` new tokens after ``ids``, from the uniforms to the results, for every id-prompt entry of both
        classes.  ``sampling``: (do_sample, temperature, top_k, top_p, generator, uniforms).  ``groups`` = (t, B0): ``ids`` is
        ``prompts.repeat(t, 1)``, run as B0 groups of t -- inputs and results stay in the caller's row order, translated to and from
        the engine's group-major one.  ``fan`` = samples > 0: ``ids`` holds one row per kept trajectory, everything else
        ``rows * samples`` rows, group-major (the public order there); the live engine is used as it is.  ``sdf_tail``: the engine is
        asked for one token more, the forced sdf that feeds the last frame's 16th token: the uniforms get a column (never read) and a
        table that ends with the last frame's action a zero row (the token is dropped and never fed, the row reaches no output).
        -> namespace(tokens (B, L0 + n), reward (B), frame_rewards (B, F), frame_hidden (B, F, hidden), token_scores: TokenScores of
        (B, n), filtered_scores: FilteredTokenScores of (B, n)), None what was not asked for; ``.result(*values)``: the values that are not None, a single one bare."""
        do_sample, temperature, top_k, top_p, generator, u = sampling
        L0 = ids.shape[1]
        B = ids.shape[0] * fan if fan else ids.shape[0]
        t, B0 = groups or (1, B)
        n_new = n + 1 if sdf_tail else n
        if u is None:
            u = self._uniforms(B, n, do_sample, generator)
        if u is not None:
            u = u.to(device=self.device, dtype=torch.float32)
            if u.shape[1] < n_new:
                u = torch.cat([u, u.new_zeros(B, n_new - u.shape[1])], 1)
            u = u[:, :n_new].contiguous()
        if act is not None and sdf_tail:
            need = (L0 - 257 * ctx) // 17 + n_new // 17 + ctx
            if act.shape[1] < need:
                act = torch.cat([act, act.new_zeros(B, need - act.shape[1], act.shape[2])], 1)
        dev, F = self.device, n_new // 17
        out = torch.empty(B, L0 + n_new, dtype=torch.int64, device=dev)
        rw = torch.empty(B, dtype=torch.float32, device=dev) if reward else None
        fr = torch.empty(B, F, dtype=torch.float32, device=dev) if frame_rewards else None
        fh = torch.empty(B, F, self._cfg["hidden_size"], dtype=self.torch_dtype, device=dev) if frame_hidden else None
        ts = _token_scores_buffer(B, n_new, dev) if scores else None
        fs = torch.empty(B, n_new, 4, dtype=torch.float32, device=dev) if filtered else None
        self._sampling_engine(B, act.shape[1] if act is not None else 32, temperature, top_p, existing=bool(fan)).rollout(
            ids[:B0].contiguous() if t > 1 else ids, n_new, out, actions=_to_group_major(act, t, B0), ctx=ctx, uniforms=_to_group_major(u, t, B0),
            top_k=top_k or self._cfg["vocab_size"], group_size=fan or t, reuse_kv=reuse_kv, force_sdf=force_sdf, fanout=bool(fan), reward=rw,
            frame_rewards=fr, frame_hidden=fh, token_scores=ts, filtered_scores=fs)
        tokens = _from_group_major(out, t, B0)
        return SimpleNamespace(tokens=tokens[:, :-1] if sdf_tail else tokens, reward=_from_group_major(rw, t, B0),
                               frame_rewards=_from_group_major(fr, t, B0), frame_hidden=_from_group_major(fh, t, B0),
                               token_scores=_token_scores_of(ts, t, B0, n) if scores else None,
                               filtered_scores=_filtered_scores_of(fs, t, B0, n) if filtered else None, result=_result)

    def get_input_embeddings(self):
        return _Embedding(self)

    @torch.no_grad()
    def generate(self, input_ids=None, do_sample=True, temperature=1.0, top_k=100, max_new_tokens=None, pad_token_id=None,
                 generator=None, uniforms=None, inputs_embeds=None, return_dict_in_generate=False, output_hidden_states=False,
                 use_cache=True, shared_context=None, top_p=None, output_token_scores=False, output_filtered_scores=False, **unused):
        """``input_ids`` prompt -> int64 (B, L0 + max_new_tokens), prompt included (HF convention).
        ``output_token_scores=True`` (HF: ``output_logits`` + ``compute_transition_scores(normalize_logits=True)``, computed on the device
        inside the decode steps): the result becomes ``(tokens, TokenScores)``; on the ``inputs_embeds`` path with
        ``return_dict_in_generate`` the field ``.token_scores``.  The tokens are those of the call without it.
        ``output_filtered_scores=True`` (HF: ``output_scores`` + ``compute_transition_scores(normalize_logits=True)``) appends the
        ``FilteredTokenScores`` -- the tokens under the temperature / top-k / top-p distribution they were drawn from -- after it
        (field ``.filtered_scores``).
        ``top_p``: HF's nucleus filter after the top-k filter (include/ivg.h ivg_set_top_p); ``None`` / 1.0: none, ignored without
        ``do_sample``, ValueError outside [0, 1] or NaN (``_top_p_of``).
        ``shared_context`` (not in HF; round 6): ``t`` or ``"auto"`` when ``input_ids`` is ``prompts.repeat(t, 1)`` -- what
        inference/predict.py:65 and train_gpt.py:170-184 pass.  The prompt is then prefilled ONCE per distinct row, its K / V rows are kept
        once and shared by the t samples at every decode step (libivg ``ivg_generate_shared``); row order, uniforms and results are those
        of the plain call (same tokens up to near-ties of the sampler: the prompt's last position goes through the decode-step kernels).
        ``inputs_embeds`` prompt (B, L0, hidden) -> only the new tokens (B, max_new_tokens), as HF does for embeddings prompts
        (action_model.py:101-110, mbrl/video_predictor.py:298-313).  With ``return_dict_in_generate`` the result has
        ``.sequences`` and, with ``output_hidden_states``, ``.hidden_states`` of which only what the callers read exists:
        ``hidden_states[-1][-1]`` = last layer (post final norm) of the LAST forward pass, (B, 1, hidden).
        When the engine's KV cache was built from exactly ``inputs_embeds[:, :-1]`` (the step-wise rollout: previous prompt +
        the embeddings of the tokens it generated), only the last row is fed -- verified on the device, never assumed."""
        _check_temperature(temperature)
        top_p = _top_p_of(top_p, do_sample)
        if inputs_embeds is not None:
            emb = inputs_embeds.to(device=self.device, dtype=self.torch_dtype).contiguous()
            B, L0, _ = emb.shape
            out = torch.empty(B, max_new_tokens, dtype=torch.int64, device=self.device)
            hidden = torch.empty(B, 1, emb.shape[-1], dtype=self.torch_dtype, device=self.device) if output_hidden_states else None
            u = uniforms if uniforms is not None else self._uniforms(B, max_new_tokens, do_sample, generator)
            ts = _token_scores_buffer(B, max_new_tokens, self.device) if output_token_scores else None
            fs = torch.empty(B, max_new_tokens, 4, dtype=torch.float32, device=self.device) if output_filtered_scores else None
            self.last_generate_reused_cache = self._sampling_engine(B, 32, temperature, top_p).generate_embeds(
                emb, max_new_tokens, out, hidden=hidden, uniforms=u, top_k=top_k or self._cfg["vocab_size"], allow_reuse=use_cache, token_scores=ts,
                filtered_scores=fs)
            scores = _token_scores_of(ts) if output_token_scores else None
            filtered = _filtered_scores_of(fs) if output_filtered_scores else None
            if not return_dict_in_generate:
                return _result(out, scores, filtered)
            res = SimpleNamespace(sequences=out, hidden_states=((hidden,),) if output_hidden_states else None)
            if output_token_scores:
                res.token_scores = scores
            if output_filtered_scores:
                res.filtered_scores = filtered
            return res
        ids = input_ids.to(device=self.device, dtype=torch.int64).contiguous()
        B, L0 = ids.shape
        t, B0 = shared_prompt_groups(ids, shared_context) if shared_context else (1, B)
        if not (t > 1 and L0 >= 2):   # (nothing to share)
            t, B0 = 1, B
        r = self._rollout(ids, max_new_tokens, (do_sample, temperature, top_k, top_p, generator, uniforms), groups=(t, B0), scores=output_token_scores,
                          filtered=output_filtered_scores)
        return r.result(r.tokens, r.token_scores, r.filtered_scores)

    @torch.no_grad()
    def logits(self, input_ids):
        """Teacher-forced logits, float32 (B, L, vocab)  (``model(input_ids).logits`` in the reference)."""
        ids = input_ids.to(device=self.device, dtype=torch.int64).contiguous()
        B, L = ids.shape
        out = torch.empty(B, L, self._cfg["vocab_size"], dtype=torch.float32, device=self.device)
        self._ensure(B).logits(ids, out)
        return out

    @torch.no_grad()
    def _eval_forward(self, input_ids, labels, action=None, ctx=1, want_hidden=False, frames=32):
        """-> namespace(loss, token_nll (B, L), sample_loss (B), sample_perplexity (B), hidden_states or None): HF shifted
        cross-entropy (ignore_index -100; mean over the batch's valid targets) computed by libivg ``ivg_eval_forward`` without the
        (B, L, vocab) logits tensor."""
        ids = input_ids.to(device=self.device, dtype=torch.int64).contiguous()
        lab = labels.to(device=self.device, dtype=torch.int64).contiguous()
        B, L = ids.shape
        nll = torch.empty(B, L, dtype=torch.float32, device=self.device)
        rows = torch.empty(B, 2, dtype=torch.float32, device=self.device)
        hidden = torch.empty(B, L, self._cfg["hidden_size"], dtype=self.torch_dtype, device=self.device) if want_hidden else None
        act = action.to(device=self.device, dtype=torch.float32).contiguous() if action is not None else None
        self._ensure(B, frames).eval_forward(ids, lab, nll, rows, actions=act, ctx=ctx, hidden=hidden)
        sums, counts = rows[:, 0], rows[:, 1]
        per = sums / counts.clamp_min(1.0)
        return SimpleNamespace(loss=sums.sum() / counts.sum().clamp_min(1.0), token_nll=nll, sample_loss=per,
                               sample_perplexity=torch.exp(per), hidden_states=(hidden,) if want_hidden else None, logits=None)

    def __call__(self, input_ids=None, labels=None, output_hidden_states=False, **unused):
        """``model(input_ids=tokens, labels=labels)`` of the eval loop (train_gpt.py:356-376): ``.loss`` (+ per-sample loss /
        perplexity); without labels: ``.logits`` (B, L, vocab) fp32."""
        if labels is None:
            return SimpleNamespace(logits=self.logits(input_ids), loss=None)
        return self._eval_forward(input_ids, labels, want_hidden=output_hidden_states)

    forward = __call__


def _frames_of(max_new_tokens):
    """Frames with per-frame outputs of a rollout of ``max_new_tokens`` (include/ivg.h ivg_generate_frames): the engine is asked for
    ``max_new_tokens + 1`` tokens, whole frames of 16 + the forced sdf, so that the last frame's 16th token is fed too."""
    if not (isinstance(max_new_tokens, int) and max_new_tokens >= 16 and (max_new_tokens + 1) % 17 == 0):
        raise ValueError(f"per-frame outputs need max_new_tokens = 17 * frames - 1 (16 tokens per frame + the sdf between frames), not {max_new_tokens!r}")
    return (max_new_tokens + 1) // 17


class HeadModelWithAction:
    """action_model.py:8-45: wraps an ``llm`` and adds ``action_linear`` (+ optional ``reward_linear``)."""
    supports_shared_context = True   # generate / detokenize accept shared_context= (libivg ivg_generate_shared / ivg_detokenize_shared)

    def __init__(self, llm, action_dim, prelude_tokens_num, tokens_num_per_dyna, context, segment_length, model_type="llama",
                 reward_prediction=False, action_recon=None, **kwargs):
        if model_type != "llama":
            raise ValueError(f"model_type {model_type} is not supported.")
        self.llm = llm
        self.action_dim = action_dim
        self.prelude_tokens_num = prelude_tokens_num
        self.tokens_num_per_dyna = tokens_num_per_dyna
        self.context = context
        self.segment_length = segment_length
        self.model_type = model_type
        self.token_for_sdf = llm.config.vocab_size - 1
        self.reward_prediction = reward_prediction
        self.action_recon = action_recon
        if (llm._action_dim, llm._reward, llm._prefix) != (action_dim, reward_prediction, "llm."):
            if llm._sd is not None and llm._prefix == "":
                # wrapping an llm that already holds weights (AutoModelForCausalLM.from_config / from_pretrained, then
                # HeadModelWithAction(model, ...): mbrl/video_predictor.py:74-79): its keys move under "llm." and the new heads get the
                # reference constructor's initial values (action_model.py:36-42)
                llm._sd = self._with_fresh_heads(llm._sd, llm._cfg["hidden_size"], action_dim, reward_prediction)
            llm._action_dim, llm._reward, llm._prefix = action_dim, reward_prediction, "llm."
            llm._invalidate_pack()   # other key prefix / extra heads: whatever was packed for the bare llm is stale
        llm._wrapper_heads = (action_dim, reward_prediction)   # llm.load_state_dict(...) under this wrapper keeps the heads (load_internal_llm)
        llm._drop_engine()   # an engine built for the bare llm has no action / reward head
        self.device = llm.device
        self.action_linear = _ActionLinear(llm)
        if reward_prediction:
            self.reward_linear = _RewardLinear(llm)

    @staticmethod
    def _with_fresh_heads(llm_sd, hidden, action_dim, reward_prediction, old=None, seed=0):
        """{"llm." + k: v} plus the heads: kept from ``old`` (a previous wrapper state dict) when present, else as the reference's
        constructor leaves them -- ``action_linear`` zero-initialised (action_model.py:36-39), ``reward_linear`` with nn.Linear's
        default initialiser (:41-42; seeded here, the reference draws from the global generator)."""
        sd = {"llm." + k: v for k, v in llm_sd.items()}
        old = old or {}
        heads = {"action_linear.weight": torch.zeros(hidden, action_dim), "action_linear.bias": torch.zeros(hidden)}
        if reward_prediction:
            lin = torch.nn.Linear(hidden, 1)
            g = torch.Generator().manual_seed(seed)
            bound = 1.0 / hidden ** 0.5
            with torch.no_grad():
                lin.weight.uniform_(-bound, bound, generator=g)
                lin.bias.uniform_(-bound, bound, generator=g)
            heads["reward_linear.weight"], heads["reward_linear.bias"] = lin.weight.detach(), lin.bias.detach()
        for k, v in heads.items():
            sd[k] = old.get(k, v)
        for k, v in old.items():
            if k.startswith("action_recon_linear"):
                sd[k] = v
        return sd

    def get_input_embeddings(self, input_ids):
        """action_model.py:47-54."""
        return self.llm.get_input_embeddings()(input_ids)

    def set_decode_lds_kb(self, kb):
        self.llm.set_decode_lds_kb(kb)
        return self

    def set_kv_cache_dtype(self, name, k_scale=1.0, v_scale=1.0, scales=None):
        self.llm.set_kv_cache_dtype(name, k_scale, v_scale, scales)
        return self

    @property
    def kv_scales(self):
        return self.llm.kv_scales

    def select_kept_cache(self, parents):
        """``LlamaForCausalLM.select_kept_cache``: the kept cache of the last ``generate`` call (its action table included) gathered by
        ``parents``; continue with ``reuse_cache=True`` on ``inputs_token[parents]`` and ``action[parents]``."""
        self.llm.select_kept_cache(parents)
        return self

    def save_kept_cache(self):
        """``LlamaForCausalLM.save_kept_cache``: -> ``KeptCache``, the kept cache of the last call (its action table included) set aside."""
        return self.llm.save_kept_cache()

    def restore_kept_cache(self, kept, parents=None):
        """``LlamaForCausalLM.restore_kept_cache``; continue with ``reuse_cache=True`` on ``inputs_token[parents]`` and ``action[parents]``."""
        self.llm.restore_kept_cache(kept, parents)
        return self

    def extend_kept_cache(self, inputs_token, action=None, keep=None, return_nll=False, return_reward=False, output_frame_hidden_states=False,
                          output_token_scores=False):
        """``LlamaForCausalLM.extend_kept_cache`` with ``action_linear(action[:, i + context - 1])`` added on the i-th sdf slot among
        the appended positions, as ``generate`` does; ``action`` (B, T, D) becomes the kept action table, and its rows of the slots
        before ``keep`` must equal the kept ones.  ``keep`` is required.  Continue with ``generate(inputs_token, action=action,
        reuse_cache=True)``.  ``return_reward="frames"``, ``output_frame_hidden_states``, ``output_token_scores``: -> ``ExtendOutputs``,
        the values ``generate`` returns for imagined frames, here for the given ones (forced ``sdf`` columns score 0)."""
        if keep is None:
            raise ValueError("extend_kept_cache: keep (the number of kept positions to keep) is required")
        if return_reward not in (False, "frames"):
            raise ValueError("extend_kept_cache: return_reward must be False or 'frames'")
        if return_reward == "frames" and not self.reward_prediction:
            raise ValueError("return_reward='frames' needs a model with reward_prediction=True")
        act = action.to(device=self.llm.device, dtype=torch.float32).contiguous() if action is not None else None
        return self.llm.extend_kept_cache(inputs_token, keep, return_nll=return_nll, output_frame_hidden_states=output_frame_hidden_states,
                                          output_token_scores=output_token_scores, _actions=act, _ctx=self.context,
                                          _frame_rewards=return_reward == "frames")

    @torch.no_grad()
    def fan_out(self, inputs_token, samples, action=None, **generate_kwargs):
        """``LlamaForCausalLM.fan_out`` under this wrapper's forced-sdf schedule: ``action`` (B * samples, T, D), one table per
        candidate in row order ``b * samples + k`` (``rollout_actions``' order); its rows of sdf slots already in the kept cache are
        not looked at.  Also takes ``return_reward="frames"`` and ``output_frame_hidden_states``, as ``generate``."""
        llm = self.llm
        ids = inputs_token.to(device=llm.device, dtype=torch.int64).contiguous()
        act = action.to(device=llm.device, dtype=torch.float32).contiguous() if action is not None else None
        return llm._fan_out(ids, samples, act, self.context, generate_kwargs, force_sdf=True)   # (without actions: generate_without_action's schedule)

    def calibrate_kv_cache(self, input_ids, action=None, headroom=1, reset=True):
        """``LlamaForCausalLM.calibrate_kv_cache`` with the action embeddings added on every sdf slot (as ``logits``) at this wrapper's
        context length."""
        act = action.to(device=self.llm.device, dtype=torch.float32).contiguous() if action is not None else None
        return self.llm.calibrate_kv_cache(input_ids, headroom=headroom, reset=reset, _actions=act, _ctx=self.context)

    def replica(self):
        """As LlamaForCausalLM.replica: a second wrapper (own engine) over the same weights in HBM."""
        llm = self.llm.replica()   # (carries action_dim / reward / prefix and the shared pack: the wrapper below changes none of them)
        return HeadModelWithAction(llm, self.action_dim, self.prelude_tokens_num, self.tokens_num_per_dyna, self.context, self.segment_length,
                                   model_type=self.model_type, reward_prediction=self.reward_prediction, action_recon=self.action_recon)

    def load_state_dict(self, sd, strict=True):
        if strict:
            W.validate_state_dict({k: v for k, v in sd.items() if not k.startswith("action_recon_linear")},
                                  W.llama_param_shapes(self.llm._cfg, self.action_dim, self.reward_prediction), "HeadModelWithAction")
        self.llm._sd, self.llm._prefix = sd, "llm."
        self.llm._drop_engine()
        self.llm._invalidate_pack()

    def state_dict(self):
        return self.llm._sd

    def to(self, device=None, *a, **k):
        self.llm.to(device)
        self.device = self.llm.device
        return self

    def eval(self):
        return self

    @torch.no_grad()
    def generate(self, inputs_token, do_sample=True, temperature=1.0, top_k=100, max_new_tokens=None, pad_token_id=50256,
                 action=None, generator=None, uniforms=None, return_reward=False, reuse_cache=False, shared_context=None, top_p=None,
                 output_frame_hidden_states=False, output_token_scores=False, output_filtered_scores=False):
        """action_model.py:56-121: action (B, T, D); new token j is the forced sdf when j % 17 == 0; the i-th sdf slot's
        embedding gets ``action_linear(action[:, i + context - 1])``.  -> int64 (B, L0 + max_new_tokens).
        ``shared_context``: as ``LlamaForCausalLM.generate`` -- ``inputs_token`` is ``prompts.repeat(t, 1)`` (train_gpt.py:170, VP2's
        candidate action sequences over one context: vp/ivideogpt_interface.py:155-202); the ACTIONS stay per row (the shared prefix ends
        before the first action slot).
        ``reuse_cache=True`` (step-wise rollouts, mbrl/video_predictor.py:286-317): the prompt is the previous call's full
        output plus the forced ``sdf``; the engine keeps the KV cache of that call and feeds only the last prompt token
        instead of prefilling the grown prompt again (raises AssertionError when the cache holds something else).
        ``top_p`` (not in the reference's signature; an extension like ``shared_context``): as ``LlamaForCausalLM.generate``.
        ``return_reward="frames"`` (the reference declares ``reward (B, segment - context)`` and leaves it a TODO, action_model.py:83-99):
        -> ``(tokens (B, L0 + max_new_tokens), rewards (B, F))``, ``F = (max_new_tokens + 1) // 17``: ``reward_linear`` at the hidden
        state of every predicted frame's 16th token, the position the head is trained on (action_model.py:198-204), from ONE call
        (include/ivg.h ivg_generate_frames).  ``max_new_tokens + 1`` must be a multiple of 17 (ValueError): the engine runs one token
        more, the forced ``sdf`` that feeds the last frame's 16th token, and that column is dropped.  ``return_reward=True`` keeps its
        meaning: one value (B), read at the last forward pass.
        ``output_frame_hidden_states=True`` appends the post-norm hidden states (B, F, hidden) at those positions to the result, under
        the same condition on ``max_new_tokens`` (with ``return_reward`` False or "frames").  Both work with ``shared_context`` and ``reuse_cache``.
        ``output_token_scores=True`` appends, as the LAST element of the result (a bare tensor becomes a 2-tuple), the ``TokenScores``
        ``(logprob, entropy, max_logprob)``, each float32 (B, max_new_tokens), of the model's distribution at every new token, forced
        ``sdf`` columns 0 (include/ivg.h ivg_generate_scored); the other results are those of the call without it.  With
        ``return_reward=True`` the single reward is read off the per-frame rewards of the same call, which needs
        ``max_new_tokens`` a positive multiple of 17 (the step-wise callers' 17; ValueError otherwise).
        ``output_filtered_scores=True`` appends the ``FilteredTokenScores`` after it, under the same conditions (include/ivg.h
        ivg_generate_filtered)."""
        _check_temperature(temperature)
        scored = output_token_scores or output_filtered_scores   # (either output goes through the scored entry)
        top_p = _top_p_of(top_p, do_sample)
        per_frame = isinstance(return_reward, str)
        if per_frame and return_reward != "frames":
            raise ValueError(f"return_reward must be False, True or 'frames', not {return_reward!r}")
        if per_frame or output_frame_hidden_states:
            _frames_of(max_new_tokens)   # (ValueError before any engine work)
            if per_frame and not self.reward_prediction:
                raise ValueError("return_reward='frames' needs a model with reward_prediction=True")
            if return_reward is True:   # (its value is read one token earlier than a frame's: no single call yields both)
                raise ValueError("output_frame_hidden_states goes with return_reward='frames' or False, not True")
        if scored and return_reward is True and not (isinstance(max_new_tokens, int) and max_new_tokens >= 17 and max_new_tokens % 17 == 0):
            # (the scored entry has the per-frame rewards only; the last of them is reward_out iff the call ends with a frame's sdf)
            raise ValueError(f"output_{'token' if output_token_scores else 'filtered'}_scores with return_reward=True needs max_new_tokens a positive "
                             f"multiple of 17, not {max_new_tokens!r}")
        llm = self.llm
        ids = inputs_token.to(device=llm.device, dtype=torch.int64).contiguous()
        B, L0 = ids.shape
        act = action.to(device=llm.device, dtype=torch.float32).contiguous()
        frames = per_frame or output_frame_hidden_states
        single = bool(return_reward) and not frames   # one value (B); the scored entry has the per-frame rewards only: their last one
        t, B0 = shared_prompt_groups(ids, shared_context) if (shared_context and not reuse_cache) else (1, B)
        if not (t > 1 and L0 == 257 * self.context):   # (a shared prefix ends before the first action slot)
            t, B0 = 1, B
        r = llm._rollout(ids, max_new_tokens, (do_sample, temperature, top_k, top_p, generator, uniforms), act=act, ctx=self.context, groups=(t, B0),
                         reuse_kv=reuse_cache, sdf_tail=frames, reward=single and not scored,
                         frame_rewards=per_frame or (single and scored), frame_hidden=output_frame_hidden_states, scores=output_token_scores,
                         filtered=output_filtered_scores)
        rewards = r.frame_rewards[:, -1].contiguous() if single and scored else r.frame_rewards
        return r.result(r.tokens, r.reward, rewards, r.frame_hidden, r.token_scores, r.filtered_scores)

    @torch.no_grad()
    def generate_without_action(self, inputs_token, do_sample=True, temperature=1.0, top_k=100, max_new_tokens=None, generator=None,
                                uniforms=None, top_p=None, output_frame_hidden_states=False, output_token_scores=False,
                                output_filtered_scores=False):
        """action_model.py:123-152 (no caller in the reference): per future frame 16 sampled tokens, then the forced ``sdf`` -- the
        schedule of ``generate`` without any action embedding; the last forced ``sdf`` is dropped.  -> int64 (B, L0 + max_new_tokens).
        One prefill + cached steps instead of the reference's per-frame re-prefill (token-identical: same argument as ``generate``).
        ``top_p`` (an extension, as in ``generate``): as ``LlamaForCausalLM.generate``.
        ``output_frame_hidden_states=True``: -> ``(tokens, hidden (B, F, hidden))``, the post-norm hidden state at every predicted
        frame's 16th token (as ``generate``); the tokens are those of the plain call.
        ``output_token_scores=True`` appends the ``TokenScores`` as the last element (as ``generate``), ``output_filtered_scores=True`` the
        ``FilteredTokenScores`` after it."""
        _check_temperature(temperature)
        top_p = _top_p_of(top_p, do_sample)
        if output_frame_hidden_states:
            _frames_of(max_new_tokens)   # (ValueError before any engine work)
        llm = self.llm
        ids = inputs_token.to(device=llm.device, dtype=torch.int64).contiguous()
        assert (max_new_tokens + 1) % (self.segment_length - self.context) == 0, "max_new_tokens must be (tokens_per_dyna + 1) * frames - 1"
        r = llm._rollout(ids, max_new_tokens, (do_sample, temperature, top_k, top_p, generator, uniforms), ctx=self.context, force_sdf=True,
                         sdf_tail=output_frame_hidden_states, frame_hidden=output_frame_hidden_states, scores=output_token_scores,
                         filtered=output_filtered_scores)
        return r.result(r.tokens, r.frame_hidden, r.token_scores, r.filtered_scores)

    @torch.no_grad()
    def __call__(self, input_ids=None, attention_mask=None, labels=None, position_ids=None, action=None):
        """``HeadModelWithAction.forward`` (action_model.py:154-205) as the eval loop calls it (train_gpt.py:356-376):
        ``x.loss`` = HF shifted cross-entropy (+ ``action_recon`` * MSE of the reconstructed actions, :187-196); with
        ``reward_prediction`` returns ``(x, reward_pred)`` with ``reward_pred`` (B, segment - context, 1) read from the hidden
        state of the last token of every predicted frame (:198-204).  No logits tensor is materialised (``x.logits`` is None;
        ``self.logits(ids, action)`` returns them when needed)."""
        assert attention_mask is None and position_ids is None, "the reference's callers never pass masks / position ids"
        llm = self.llm
        F = self.segment_length - self.context
        need_hidden = bool(self.reward_prediction or self.action_recon)
        if labels is None:
            return SimpleNamespace(logits=self.logits(input_ids, action), loss=None)
        x = llm._eval_forward(input_ids, labels, action=action, ctx=self.context, want_hidden=need_hidden, frames=action.shape[1])
        hidden = x.hidden_states[-1] if need_hidden else None
        if self.action_recon:
            B, L = hidden.shape[:2]
            act = action.to(device=llm.device, dtype=torch.float32).contiguous()
            err = torch.empty(B, dtype=torch.float32, device=llm.device)
            llm._engine.action_recon_sqerr(hidden, act, self.context, self.prelude_tokens_num, err)
            self.action_recon_loss = err.sum() / (B * (L - self.prelude_tokens_num) * self.action_dim)
            x.loss = x.loss + self.action_recon * self.action_recon_loss
        if self.reward_prediction:
            start = self.prelude_tokens_num + torch.arange(F, device=llm.device) * (self.tokens_num_per_dyna + 1)
            reward_pred = self.reward_linear(hidden[:, start + self.tokens_num_per_dyna])   # (B, F, 1)
            return x, reward_pred
        return x

    forward = __call__

    @torch.no_grad()
    def logits(self, input_ids, action):
        """Teacher-forced logits with the action embeddings added on every sdf slot (action_model.py:154-185)."""
        llm = self.llm
        ids = input_ids.to(device=llm.device, dtype=torch.int64).contiguous()
        act = action.to(device=llm.device, dtype=torch.float32).contiguous()
        out = torch.empty(ids.shape[0], ids.shape[1], llm._cfg["vocab_size"], dtype=torch.float32, device=llm.device)
        llm._ensure(ids.shape[0], act.shape[1]).logits(ids, out, actions=act, ctx=self.context)
        return out
