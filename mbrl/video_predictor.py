"""Inference half of the reference's MBRL world model (/root/reference/mbrl/video_predictor.py): construction from the hydra
``world_model`` block -- ``get_tokenizer`` (:40-56), ``load_models`` (:59-89), ``VideoPredictor(device, args)`` (:100-110; what
``mbrl/train_metaworld_mbpo.py:41-42`` calls) -- and ``VideoPredictor.rollout`` (:267-339).
Model / tokenizer TRAINING (``update_*``, the optimisers and LPIPS of the constructor, :112-265) is out of scope.

The rollout runs the reference's own per-step op sequence against the mirror objects, at the embeddings level (:286-317):
``get_input_embeddings`` of the context tokens once; then per environment step ``action_linear(action)`` added to the last
embedding (the step's ``sdf`` slot), ``llm.generate(inputs_embeds=..., max_new_tokens=17, return_dict_in_generate=True,
output_hidden_states=True)``, reward = ``reward_linear(hidden_states[-1][-1])``, the 16 predicted tokens + a forced ``sdf``
embedded and appended, the new frame decoded with the detokenizer cache and pushed onto the 3-frame stack.  What differs from
the reference is inside the engine: from the second step on ``generate`` recognises (device-side comparison with the inputs it
kept) that the KV cache already holds everything but the last embedding and feeds only that row -- 17 cached decode steps per
environment step instead of a prefill of the grown prompt.

Not in the reference: ``rollout_actions`` (open-loop plans in three calls) and ``track`` -> ``TrackedEpisode``, the closed loop of a
caller that acts, observes and re-plans, on the encoder's context cache and the transformer's kept cache."""
import os
import sys
from typing import NamedTuple

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TOKENS_PER_DYN = 16


def symexp(x):
    return torch.sign(x) * (torch.exp(torch.abs(x)) - 1)


def _arg(args, name, default=None):
    """hydra DictConfig, argparse Namespace or plain dict."""
    if isinstance(args, dict):
        return args.get(name, default)
    return getattr(args, name, default) if not hasattr(args, "get") else args.get(name, default)


def get_tokenizer(args):
    """mbrl/video_predictor.py:40-56: the compressive tokenizer from ``pretrained_model_name_or_path`` (random weights of that
    config when ``load_pretrained_model`` is off), ``set_context_length`` with the reference's warning when the checkpoint's context
    length differs from ``args.context_length``; -> (tokenizer, vocab_size = context codes + dynamics codes + 2 special tokens)."""
    from ivideogpt_amd import CompressiveVQModel
    if _arg(args, "vqgan_type") != "ctx_vqgan":
        raise NotImplementedError
    path = _arg(args, "pretrained_model_name_or_path")
    dt = dict(encode_dtype=_arg(args, "encode_dtype", "fp32"), decode_dtype=_arg(args, "decode_dtype", "bf16"))   # (the reference runs under bf16 autocast, :269)
    if not _arg(args, "load_pretrained_model"):
        vq_model = CompressiveVQModel.from_config(path, **dt)
    else:
        vq_model = CompressiveVQModel.from_pretrained(path, subfolder=None, revision=None, variant=None, use_safetensor=True,
                                                      low_cpu_mem_usage=False, device_map=None, **dt)
    if _arg(args, "context_length") != vq_model.context_length:
        print(f"[Warning] pretrained context length of vq_model mismatch, change from {vq_model.context_length} to {_arg(args, 'context_length')}")
        vq_model.set_context_length(_arg(args, "context_length"))
    return vq_model, vq_model.num_vq_embeddings + vq_model.num_dyn_embeddings + 2


def load_models(args):
    """mbrl/video_predictor.py:59-89: tokenizer + ``HeadModelWithAction(AutoModelForCausalLM.from_config(config), action_dim,
    prelude = 257 * context - 1, 16 tokens per frame, context, segment_length, model_type = parent directory of config_name,
    reward_prediction=True)``; with ``load_pretrained_model`` the transformer weights come from
    ``pretrained_transformer_path/model.safetensors`` -- into ``model.llm`` only when ``load_internal_llm`` (an action-free
    pretrained transformer under freshly initialised action / reward heads), else into the whole wrapper, strictly.
    (``llama_attn_drop`` configures training-time dropout: no effect on the inference path, accepted and ignored.)"""
    from safetensors.torch import load_file
    from ivideogpt_amd import HeadModelWithAction, LlamaForCausalLM
    from ivideogpt_amd import weights as W
    tokenizer, vocab_size = get_tokenizer(args)
    config_name = _arg(args, "config_name")
    assert config_name, "world_model.config_name is required"
    config = W.load_llama_config(config_name)
    config["vocab_size"] = vocab_size
    load = bool(_arg(args, "load_pretrained_model"))
    model = LlamaForCausalLM.from_config(config, seed=None if load else _arg(args, "seed", 0), dtype=_arg(args, "llm_dtype", "bf16"))
    ctx = _arg(args, "context_length")
    model = HeadModelWithAction(model, action_dim=_arg(args, "action_dim"), prelude_tokens_num=(256 + 1) * ctx - 1, tokens_num_per_dyna=16,
                                context=ctx, segment_length=_arg(args, "segment_length"), model_type=os.path.normpath(config_name).split(os.sep)[-2],
                                reward_prediction=True)
    if load:
        state_dict = load_file(os.path.join(_arg(args, "pretrained_transformer_path"), "model.safetensors"))
        if _arg(args, "load_internal_llm"):
            model.llm.load_state_dict(state_dict, strict=True)
        else:
            model.load_state_dict(state_dict, strict=True)
    return model, tokenizer


class Observation(NamedTuple):
    """``TrackedEpisode.observe(..., return_outputs=True)``: the model's view of the frame it was just shown.  ``surprise`` (B,): the
    sum of the frame's 16 token NLLs (the default return); ``reward`` (B, 1): ``reward_linear(hidden)``, through ``symexp`` under
    ``symlog`` -- what ``plan`` reports for an imagined frame; ``hidden`` (B, H): the post-norm hidden state at the frame's 16th token,
    the features at the root of the next plan; ``entropy`` (B,): the mean predictive entropy over the frame's 16 tokens
    (``TokenScores.per_frame``), to set beside ``plan``'s uncertainty."""
    surprise: torch.Tensor
    reward: torch.Tensor
    hidden: torch.Tensor
    entropy: torch.Tensor


class TrackedEpisode:
    """The closed loop of ``VideoPredictor.track``: the model follows an episode as it is OBSERVED.  Both contexts are kept on the
    device -- the encoder's (``EncodeCache``: no context frame is encoded again) and the transformer's (the kept K / V cache: no
    prompt pass) -- so a control step costs one conditional-encoder pass over the new frame plus 17 teacher-forced positions, and a
    ``plan`` fans candidates out of the very cache ``observe`` extends.  Existing primitives only; no arithmetic of its own.

    ``tokens`` (B, 257*ctx + 17*steps): the context tokens and the tokens of the ``steps`` frames observed since, ending in the sdf
    of the next frame's slot.  ``table`` (B, ctx - 1 + max_steps, A): the actions taken, row ``i + ctx - 1`` on the i-th sdf slot
    (rows not yet taken are zero).  ``reanchors``: how often the positions were used up and the episode was anchored again.

    The transformer has ONE kept cache, so one session of a predictor is the active one; the others, and the active one while the
    predictor rolls out, are suspended: ``suspend`` sets the kept cache aside in a ``KeptCache`` (``save_kept_cache``), ``resume`` brings
    it back (``restore_kept_cache``: a copy, no prompt pass).  ``observe``, ``plan`` and ``select`` make their session the active one
    first, so sessions and rollouts of one predictor interleave freely.  ``restore_fallbacks``: how often a resume found its snapshot
    unusable (the model was given new weights) and paid the prompt pass of a fresh kept cache instead."""

    def __init__(self, predictor, obs, max_steps=None, on_full="reanchor", grow="prefill"):
        if on_full not in ("reanchor", "raise"):
            raise ValueError(f"track: on_full must be 'reanchor' or 'raise', not {on_full!r}")
        if grow not in ("prefill", "restore"):
            raise ValueError(f"track: grow must be 'prefill' or 'restore', not {grow!r}")
        predictor._suspend_active()   # the session about to be anchored takes the model's kept cache
        self.p, self.on_full, self.grow = predictor, on_full, grow
        self.suspended, self._kept, self.restore_fallbacks = False, None, 0
        ctx, llm = predictor.context_length, predictor.model.llm
        room = ((llm._max_seq or llm._cfg["max_position_embeddings"]) + 1 - 257 * ctx) // 17   # observe needs 257*ctx + 17*steps - 1 kept positions
        if room < 1:
            raise ValueError("track: max_position_embeddings leaves no room for a frame after the context")
        self.max_steps = room if max_steps is None else min(int(max_steps), room)
        if self.max_steps < 1:
            raise ValueError("track: max_steps must be at least 1")
        obs = obs.to(predictor.device).float() / 255.
        self.stack = list(torch.chunk(obs, 3, dim=1))                          # frame_stack = 3
        self.reanchors = 0
        self._anchor()
        predictor._active = self

    def suspend(self):
        """Sets this session's kept cache aside (``save_kept_cache``); the model is then free for anything else.  The session keeps the
        snapshot beside its tokens, table, frame stack and encoder cache.  No effect on a suspended session."""
        if not self.suspended:
            try:
                self._kept = self.p.model.save_kept_cache()
            except ValueError:   # the model holds no kept cache any more (new weights, a call made past the predictor): resume starts afresh
                self._kept = None
            self.suspended = True
        if self.p._active is self:
            self.p._active = None
        return self

    def resume(self):
        """Makes the model's kept cache this session's again: the snapshot is restored, or, where the model refuses it (it was given
        new weights since) or nothing could be saved, a fresh kept cache is established with a prompt pass over ``tokens`` and ``restore_fallbacks`` counts it.
        The caller sees to it that no other session is active (``VideoPredictor`` does).  No effect on a session that is not suspended."""
        if self.suspended:
            kept, self._kept = self._kept, None
            try:
                if kept is None:
                    raise ValueError("nothing was saved")
                self.p.model.restore_kept_cache(kept)
            except ValueError:
                self._establish()
                self.restore_fallbacks += 1
            finally:
                if kept is not None:
                    kept.close()
            self.suspended = False
        self.p._active = self
        return self

    def _anchor(self):
        """The last ``ctx`` frames of the stack become the context: a fresh encoder cache, fresh tokens and table, a fresh kept cache."""
        p, ctx = self.p, self.p.context_length
        self.tokens, self.enc_cache = p.tokenizer.encode_context(torch.stack(self.stack[-ctx:], dim=1), ctx, return_cache=True)
        B = self.tokens.shape[0]
        self.table = torch.zeros(B, ctx - 1 + self.max_steps, p.model.action_dim, dtype=torch.float32, device=p.device)
        self.steps = 0
        self._establish()

    def _establish(self, rows=None):
        """The transformer's kept cache at ``tokens[:, :-1]``: a one-token ``generate`` (the prompt pass), then a pure rewind in front
        of the last sdf slot, whose action is not known yet.  ``rows``: the batch the engine must hold (``plan``'s candidates), with one
        action row more than the table has for the forced sdf behind a plan's last frame."""
        model, L0 = self.p.model, self.tokens.shape[1]
        model.llm._ensure(max(rows or 0, self.tokens.shape[0]), self.table.shape[1] + 1)
        model.generate(self.tokens, do_sample=False, max_new_tokens=1, action=self.table)
        model.extend_kept_cache(self.tokens, action=self.table, keep=L0 - 1)

    @property
    def batch(self):
        return self.tokens.shape[0]

    @torch.no_grad()
    def observe(self, frame, action, return_outputs=False):
        """The environment's answer to ``action``: ``frame`` [B, 3, H, W] in 0..255, ``action`` [B, A].  The frame is tokenized against
        the encoder cache and teacher-forced onto the kept cache (``extend_kept_cache`` with the action on its sdf slot).
        -> float32 (B,): the model's surprise at that frame, the sum of its 16 token NLLs (nats); with ``return_outputs=True`` an
        ``Observation`` -- that surprise, the reward and hidden state the model assigns to the frame and its predictive entropy, from
        the same extend (no prompt pass).  ``tokens`` and ``steps`` advance.
        When the positions are used up, the last ``ctx`` frames observed SO FAR become the new context first (real frames: the model's
        own episode start; ``reanchors`` counts it) and this frame is its first step -- or, with ``on_full="raise"``, RuntimeError
        with the session as it was."""
        p, ctx = self.p, self.p.context_length
        p._activate(self)
        if self.steps >= self.max_steps:
            if self.on_full == "raise":
                raise RuntimeError(f"track: the {self.max_steps} steps the positions allow are used up (on_full='raise')")
            self._anchor()
            self.reanchors += 1
        frame = frame.to(p.device).float() / 255.
        dyn = p.tokenizer.tokenize_frames(frame[:, None], self.enc_cache)      # (B, 17): 16 dyn tokens + the next slot's sdf
        table = self.table.clone()
        table[:, self.steps + ctx - 1] = action.to(p.device).float()
        tokens = torch.cat([self.tokens, dyn], 1)
        keep = self.tokens.shape[1] - 1
        if return_outputs:   # one frame: its 16th token is fed at column 15
            out = p.model.extend_kept_cache(tokens, action=table, keep=keep, return_nll=True, output_frame_hidden_states=True, output_token_scores=True)
            nll = out.token_nll
        else:
            nll = p.model.extend_kept_cache(tokens, action=table, keep=keep, return_nll=True)   # (B, 17); column 16: the forced sdf
        self.tokens, self.table, self.steps = tokens, table, self.steps + 1
        self.stack = self.stack[1:] + [frame]
        surprise = nll[:, :TOKENS_PER_DYN].sum(1)
        if not return_outputs:
            return surprise
        hidden = out.frame_hidden[:, 0]
        reward = p.model.reward_linear(hidden)                                # (B, 1)
        if p.symlog:
            reward = symexp(reward)
        return Observation(surprise, reward.float(), hidden, out.token_scores.per_frame()[1][:, 0])

    @torch.no_grad()
    def plan(self, plans, samples=1, return_uncertainty=False, uniforms=None, generator=None, return_proposal_logprob=False):
        """Imagines ``samples`` action plans per tracked history: ``plans`` [B * samples, horizon, A], rows ``b * samples + k`` the
        candidates of history b (``rollout_actions``' order, also of ``uniforms`` [B * samples, 17 * horizon - 1] and every result).
        One ``fan_out`` of the kept cache and one ``detokenize`` of the imagined frames; the kept cache is afterwards what it was.
        -> (obss [B * samples, horizon + 1, 9, H, W], actions [B * samples, horizon + 1, A], rewards [B * samples, horizon + 1, 1])
        and, with ``return_uncertainty``, uncertainty [B * samples, horizon + 1, 1]; with ``return_proposal_logprob``, after it, the
        proposal log-probability [B * samples, horizon + 1, 1]: ``rollout_actions``' results, step 0 being the observed stack."""
        p, ctx, model, k = self.p, self.p.context_length, self.p.model, int(samples)
        p._activate(self)
        B, horizon = self.batch, plans.shape[1]
        assert k >= 1 and plans.shape[0] == B * k, "plans must hold `samples` consecutive rows per tracked history"
        if self.steps + horizon > self.max_steps:
            raise ValueError(f"plan: {self.steps} observed + {horizon} imagined frames exceed the {self.max_steps} the positions allow")
        if B * k > model.llm._engine.max_batch:   # the engine is rebuilt for the candidates
            self._grow(B * k)
        act = plans.to(p.device).float()
        table = self.table.repeat_interleave(k, 0)
        table[:, self.steps + ctx - 1:self.steps + ctx - 1 + horizon] = act
        L0 = self.tokens.shape[1]
        tokens, hidden, *scores = model.fan_out(self.tokens, k, action=table, do_sample=True, temperature=1.0, top_k=100,
                                                max_new_tokens=17 * horizon - 1, uniforms=uniforms, generator=generator,
                                                output_frame_hidden_states=True, output_token_scores=return_uncertainty,
                                                output_filtered_scores=return_proposal_logprob)
        rewards = model.reward_linear(hidden).squeeze(-1)                      # (B * samples, horizon)
        # every frame is decoded against the context alone: the imagined frames directly behind the context tokens
        clip = p.tokenizer.detokenize(torch.cat([tokens[:, :257 * ctx], tokens[:, L0:]], 1), ctx)
        frames = [f.repeat_interleave(k, 0) if k > 1 else f for f in self.stack] + list(clip[:, ctx:].clamp(0.0, 1.0).unbind(1))
        obss = torch.stack([torch.cat(frames[s:s + 3], dim=1) for s in range(horizon + 1)], 1).float()
        actions = torch.cat([torch.zeros_like(act[:, :1]), act], 1).float()
        rewards = torch.cat([torch.zeros_like(rewards[:, :1]), rewards], 1).unsqueeze(-1)
        if p.symlog:
            rewards = symexp(rewards)
        extra = []
        if return_uncertainty:
            extra.append(scores[0].per_frame()[1])                             # (B * samples, horizon)
        if return_proposal_logprob:
            extra.append(scores[-1].per_frame()[0])
        return (obss, actions, rewards.float(), *(torch.cat([torch.zeros_like(x[:, :1]), x], 1).unsqueeze(-1).float() for x in extra))

    def _grow(self, rows):
        """The kept cache in an engine that holds ``rows`` trajectories.  ``grow="prefill"``: one prompt pass over ``tokens`` brings it
        back; ``"restore"``: the rows ``observe`` built are saved, the model rebuilds its engine, and they are restored into it."""
        model = self.p.model
        if self.grow != "restore":
            return self._establish(rows=rows)
        with model.save_kept_cache() as kept:
            model.llm._ensure(rows, self.table.shape[1] + 1)   # (one action row more: the forced sdf behind a plan's last frame)
            model.restore_kept_cache(kept)

    def select(self, parents):
        """Row i of the session becomes what row ``parents[i]`` was (particle resampling, dropping finished environments): the kept
        cache (``select_kept_cache``), the encoder cache (``EncodeCache.select``), the tokens, the action table and the frame stack."""
        from ivideogpt_amd.transformer import normalize_parents
        q = normalize_parents(parents, self.batch)
        self.p._activate(self)
        self.p.model.select_kept_cache(q)
        self.enc_cache = self.enc_cache.select(q)
        idx = torch.from_numpy(q).to(self.p.device, torch.int64)
        self.tokens, self.table = self.tokens[idx].contiguous(), self.table[idx].contiguous()
        self.stack = [f[idx] for f in self.stack]
        return self


class VideoPredictor:
    _active = None   # the TrackedEpisode whose kept cache the model holds (None: nobody's, or a rollout's)

    def __init__(self, device, args=None, reuse_cache=True):
        """``VideoPredictor('cuda', cfg.world_model)`` -- the reference's constructor (:100-110): models built by ``load_models(args)``
        and moved to ``device``.  ``reuse_cache=False`` forces a prefill of the whole prompt at every step (the reference's behaviour;
        A/B and tests).  ``VideoPredictor.from_models(tokenizer, model, ...)`` wraps objects that already exist."""
        self.args, self.device = args, torch.device(device)
        self.model, self.tokenizer = load_models(args)
        self.model = self.model.to(self.device)
        self.tokenizer = self.tokenizer.to(self.device)
        self.context_length, self.symlog, self.reuse_cache = _arg(args, "context_length"), bool(_arg(args, "symlog", True)), reuse_cache
        self.steps_with_kept_cache = 0

    @classmethod
    def from_models(cls, tokenizer, model, context_length=2, symlog=True, device="cuda", reuse_cache=True):
        """tokenizer: ivideogpt_amd.CompressiveVQModel; model: ivideogpt_amd.HeadModelWithAction(reward_prediction=True)."""
        self = cls.__new__(cls)
        self.args = None
        self.tokenizer, self.model, self.device = tokenizer, model, torch.device(device)
        self.context_length, self.symlog, self.reuse_cache = context_length, symlog, reuse_cache
        self.steps_with_kept_cache = 0
        return self

    # ---- one model, one kept cache: which session it belongs to.  Sessions of THIS predictor and its rollouts arbitrate here; a call that
    # goes to the model directly, past the predictor, overwrites the kept cache unseen, and the active session's next call is refused by
    # the engine's on-device verification, as it always was
    def _suspend_active(self):
        """The active session, if any, sets its kept cache aside: called before anything else touches the model."""
        if self._active is not None:
            self._active.suspend()
        self._active = None

    def _activate(self, session):
        """``session`` becomes the active one: the previous one is suspended first, then ``session`` resumes."""
        if self._active is not session:
            self._suspend_active()
            session.resume()
            self._active = session

    @torch.no_grad()
    def rollout(self, obs, policy, horizon, return_uncertainty=False, select=None):
        """obs [B, 9, H, W] in 0..255 (3 stacked RGB frames); policy(obs, t) -> [B, A].
        -> (obss [B, horizon+1, 9, H, W], actions [B, horizon+1, A], rewards [B, horizon+1, 1])
        ``return_uncertainty=True`` appends ``uncertainty [B, horizon+1, 1]``: per imagined step the mean predictive entropy (nats) of
        the model over the frame's 16 sampled tokens (``TokenScores.per_frame``), 0 for the dummy step 0; no ``symexp``, no transform --
        for MOPO / MOReL-style penalties and rollout truncation.
        ``select`` (not in the reference): resampling in the middle of the rollout -- truncation of uncertain trajectories, particle
        resampling, beam or successive-halving planners.  After every imagined step ``select(t, obs [B, 9, H, W], reward [B, 1],
        uncertainty [B, 1] or None)`` -- this step's values as the results hold them -- returns ``None`` (go on) or ``parents``
        (list / array / tensor of n row indices): row i of the rollout becomes a copy of row ``parents[i]``.  The engine's kept KV
        cache (``select_kept_cache``), the detokenizer cache (``DetokenizeCache.select``), the prompt, the embeddings, the frame stack
        and every earlier entry of the trace are gathered, so the next step still runs on the kept cache (``steps_with_kept_cache``),
        ``policy`` sees n rows from then on, and the returned tensors are the genealogies of the FINAL rows, with batch dimension n.
        n may exceed B up to the batch the models' engines were built for.  ``ivideogpt_amd.transformer.stable_parents`` keeps
        survivors in their rows, the cheapest resampling.  ``select=None``: exactly the rollout without it."""
        from ivideogpt_amd.transformer import normalize_parents
        self._suspend_active()
        ctx, model, llm = self.context_length, self.model, self.model.llm
        B = obs.shape[0]
        obs = obs.to(self.device).float() / 255.
        first_obs = obs
        stack = list(torch.chunk(obs, 3, dim=1))                               # frame_stack = 3
        prompt = self.tokenizer.encode_context(torch.stack(stack[-ctx:], dim=1), ctx)   # [B, 257*ctx], ends with the first sdf
        embeds = model.get_input_embeddings(prompt)
        sdf_col = torch.full((B, 1), model.token_for_sdf, dtype=prompt.dtype, device=self.device)
        cache, trace = None, {"obs": [], "act": [], "rew": [], "unc": []}
        self.steps_with_kept_cache = 0
        for t in range(horizon):
            action = policy(obs, t).to(self.device).float()
            embeds[:, -1] += model.action_linear(action)                       # this step's sdf slot carries the action
            result = llm.generate(inputs_embeds=embeds, do_sample=True, temperature=1.0, top_k=100, pad_token_id=50256,
                                  use_cache=self.reuse_cache, max_new_tokens=TOKENS_PER_DYN + 1, return_dict_in_generate=True,
                                  output_hidden_states=True, output_token_scores=return_uncertainty)
            self.steps_with_kept_cache += int(llm.last_generate_reused_cache)
            predicted = result.sequences[:, :-1]                               # the 17th token is replaced by the forced sdf
            reward = model.reward_linear(result.hidden_states[-1][-1]).squeeze(-2)   # last layer, last forward pass
            embeds = torch.cat([embeds, model.get_input_embeddings(torch.cat([predicted, sdf_col], 1))], 1)
            fmap, cache = self.tokenizer.detokenize(torch.cat([prompt, predicted], 1), ctx, cache=cache, return_cache=True)
            stack = stack[1:] + [fmap.clamp(0.0, 1.0)[:, -1]]
            obs = torch.cat(stack, dim=1)
            trace["obs"].append(obs); trace["act"].append(action); trace["rew"].append(reward)
            if return_uncertainty:
                trace["unc"].append(result.token_scores.per_frame()[1])       # [B, 1]: the 16 sampled tokens of this step's frame
            if select is not None:
                parents = select(t, obs, symexp(reward) if self.symlog else reward, trace["unc"][-1] if return_uncertainty else None)
                if parents is not None:
                    p = normalize_parents(parents, obs.shape[0])
                    if p.tolist() != list(range(obs.shape[0])):                   # (the identity: nothing to do)
                        llm.select_kept_cache(p)
                        cache = cache.select(p)
                        idx = torch.from_numpy(p).to(self.device, torch.int64)
                        embeds, prompt, obs, first_obs = embeds[idx], prompt[idx], obs[idx], first_obs[idx]
                        stack = [f[idx] for f in stack]
                        trace = {k: [x[idx] for x in v] for k, v in trace.items()}
                        sdf_col = sdf_col[:1].expand(p.size, 1)
        # dummy step 0: the initial observation with a zero action / reward
        obss = torch.stack([first_obs] + trace["obs"], 1).float()
        actions = torch.stack([torch.zeros_like(trace["act"][0])] + trace["act"], 1).float()
        rewards = [torch.zeros_like(trace["rew"][0])] + trace["rew"]
        if self.symlog:
            rewards = [symexp(r) for r in rewards]
        if return_uncertainty:
            uncertainty = torch.stack([torch.zeros_like(trace["unc"][0])] + trace["unc"], 1).float()
            return obss, actions, torch.stack(rewards, 1).float(), uncertainty
        return obss, actions, torch.stack(rewards, 1).float()

    @torch.no_grad()
    def track(self, obs, max_steps=None, on_full="reanchor", grow="prefill"):
        """Starts a closed-loop session (act, observe, re-plan: MPC, MBRL on real transitions, monitoring the model's surprise) at
        ``obs`` [B, 9, H, W] in 0..255, as for ``rollout``: its last ``ctx`` frames are encoded once, with the encoder's context cache
        kept, and the transformer's kept cache is established at the context.  -> ``TrackedEpisode``: ``plan`` imagines candidate action
        sequences from where the episode stands, ``observe`` moves it on by the frame that was really seen and returns the model's
        surprise, ``select`` resamples its rows.  ``max_steps``: frames to observe before the session anchors itself again at the
        last ``ctx`` observed frames (default and upper bound: what ``max_position_embeddings`` allows); ``on_full="raise"``:
        RuntimeError instead.  ``grow``: how a ``plan`` whose candidates need a larger engine than the model has built brings the kept
        cache into the new one -- ``"prefill"``, a prompt pass over the tracked tokens, or ``"restore"``, a copy of the very rows
        ``observe`` built (``save_kept_cache`` / ``restore_kept_cache``; bit-different from a prompt pass over the same tokens, hence opt-in).
        A predictor serves any number of sessions, and ``rollout`` / ``rollout_actions`` beside them: whoever touches the model first
        suspends the session whose kept cache it holds, and a session resumes by a copy when it is used next (``TrackedEpisode``).
        Only calls made on the model or tokenizer objects directly, past the predictor, still end a session."""
        return TrackedEpisode(self, obs, max_steps=max_steps, on_full=on_full, grow=grow)

    @torch.no_grad()
    def rollout_actions(self, obs, actions, samples=1, generator=None, uniforms=None, return_uncertainty=False, return_proposal_logprob=False):
        """Open-loop rollout of given action sequences (a CEM / MPPI / MPC planner's candidates, MBPO with a fixed plan) in three calls
        instead of ``horizon`` steps: one ``encode_context``, one ``generate`` that also returns the hidden state at every frame's
        16th token, where the reward head is trained (include/ivg.h ivg_generate_frames), and one ``detokenize``.  The rewards are
        ``reward_linear`` of those hidden states, the very arithmetic of ``rollout``: for the same actions and uniforms the two give the
        same rewards bit for bit (``generate(return_reward="frames")`` folds the final norm into the head and differs in the last bit).
        obs [B, 9, H, W] in 0..255; actions [B * samples, horizon, A]: with ``samples`` > 1, rows ``b * samples .. (b + 1) * samples - 1``
        are the candidates of observation b, whose context is prefilled, kept and decoded once (``shared_context``).
        ``uniforms`` [B * samples, 17 * horizon - 1] (rows as ``actions``) or ``generator`` drive the sampler.
        -> (obss [B * samples, horizon + 1, 9, H, W], actions [B * samples, horizon + 1, A], rewards [B * samples, horizon + 1, 1]):
        ``rollout``'s layout, with its dummy step 0 and ``symexp``.  ``return_uncertainty=True`` appends ``uncertainty
        [B * samples, horizon + 1, 1]`` as ``rollout`` does: the per-frame mean predictive entropy from the same ``generate`` call
        (``output_token_scores``), equal to ``rollout``'s bit for bit on the same actions and uniforms.
        ``return_proposal_logprob=True`` appends, after it, ``proposal_logprob [B * samples, horizon + 1, 1]``: per imagined frame the
        summed log-probability of its 16 sampled tokens under the temperature / top-k / top-p distribution they were drawn from
        (``FilteredTokenScores.per_frame``, ``output_filtered_scores``), 0 for step 0 -- the proposal term of an importance weight or a
        likelihood ratio over candidates."""
        from ivideogpt_amd.transformer import _from_group_major, _to_group_major
        self._suspend_active()
        ctx, model = self.context_length, self.model
        B, t = obs.shape[0], int(samples)
        N, horizon = actions.shape[0], actions.shape[1]
        assert t >= 1 and N == B * t, "actions must hold `samples` consecutive rows per observation"
        obs = obs.to(self.device).float() / 255.
        stack = list(torch.chunk(obs, 3, dim=1))                               # frame_stack = 3
        prompt = self.tokenizer.encode_context(torch.stack(stack[-ctx:], dim=1), ctx)   # [B, 257*ctx], ends with the first sdf
        act = actions.to(self.device).float()
        # the engine's action table: row i + ctx - 1 goes onto the i-th sdf slot (rows below ctx - 1 are never read)
        table = torch.cat([act.new_zeros(N, ctx - 1, act.shape[2]), act], 1)
        # generate / detokenize take the candidates in ``prompt.repeat(t, 1)`` order (row k * B + b)
        u = _from_group_major(uniforms.to(self.device).float().contiguous(), t, B) if uniforms is not None else None
        tokens, hidden, *scores = model.generate(prompt.repeat(t, 1), do_sample=True, temperature=1.0, top_k=100, max_new_tokens=17 * horizon - 1,
                                                 action=_from_group_major(table.contiguous(), t, B), generator=generator, uniforms=u,
                                                 output_frame_hidden_states=True, shared_context=t if t > 1 else None,
                                                 output_token_scores=return_uncertainty, output_filtered_scores=return_proposal_logprob)
        rewards = model.reward_linear(hidden).squeeze(-1)                      # (B * samples, horizon)
        clip = self.tokenizer.detokenize(tokens, ctx, shared_context=t if t > 1 else None)
        rewards, clip = _to_group_major(rewards, t, B), _to_group_major(clip, t, B)
        frames = [f.repeat_interleave(t, 0) if t > 1 else f for f in stack] + list(clip[:, ctx:].clamp(0.0, 1.0).unbind(1))
        obss = torch.stack([torch.cat(frames[s:s + 3], dim=1) for s in range(horizon + 1)], 1).float()
        actions = torch.cat([torch.zeros_like(act[:, :1]), act], 1).float()
        rewards = torch.cat([torch.zeros_like(rewards[:, :1]), rewards], 1).unsqueeze(-1)
        if self.symlog:
            rewards = symexp(rewards)
        extra = []
        if return_uncertainty:
            extra.append(_to_group_major(scores[0].per_frame()[1], t, B))     # (B * samples, horizon)
        if return_proposal_logprob:
            extra.append(_to_group_major(scores[-1].per_frame()[0], t, B))
        return (obss, actions, rewards.float(), *(torch.cat([torch.zeros_like(x[:, :1]), x], 1).unsqueeze(-1).float() for x in extra))
