"""The closed loop of mbrl/video_predictor.py (VideoPredictor.track -> TrackedEpisode: observe / plan / select / re-anchoring) on the
MI355X, with the tiny action-conditioned world model with a reward head of helpers.world_model_files (fp32 tokenizer; fp32 and bf16
transformers, i.e. both routes of ivg_kv_extend).  The session adds no arithmetic, so every check is an equality with the same
primitives called by hand."""
import json

import pytest
import torch

from helpers import world_model_files

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CTX = 2
DTYPES = pytest.mark.parametrize("llm_dtype", ["fp32", "bf16"])


def lib():
    from ivideogpt_amd import _lib
    return _lib.load()


def extend_rows():
    return lib().ivg_debug_counter(b"kv_extend_chunk_rows") + lib().ivg_debug_counter(b"kv_extend_step_rows")


def predictors(tmp_path, llm_dtype, n=1, max_pos=None):
    from mbrl.video_predictor import VideoPredictor
    args, *_ = world_model_files(tmp_path, False)
    if max_pos is not None:
        with open(args["config_name"]) as f:
            cfg = json.load(f)
        with open(args["config_name"], "w") as f:
            json.dump(dict(cfg, max_position_embeddings=max_pos), f)
    args.update(encode_dtype="fp32", decode_dtype="fp32", llm_dtype=llm_dtype)
    return [VideoPredictor("cuda", args) for _ in range(n)]


def episode(B, steps, seed=8):
    g = torch.Generator().manual_seed(seed)
    obs = torch.randint(0, 256, (B, 9, 64, 64), generator=g).float()
    frames = [torch.randint(0, 256, (B, 3, 64, 64), generator=g).float() for _ in range(steps)]
    acts = [torch.randn(B, 4, generator=g) for _ in range(steps)]
    return obs, frames, acts


def context_of(obs):
    return torch.stack(list(torch.chunk(obs.to(DEV) / 255., 3, dim=1))[-CTX:], dim=1)


@DTYPES
def test_tracked_tokens_and_surprise(tmp_path, llm_dtype):
    vp, by_hand = predictors(tmp_path, llm_dtype, n=2)
    B = 2
    obs, (f1, f2), (a1, a2) = episode(B, 2)
    trk = vp.track(obs)
    assert trk.steps == 0 and trk.tokens.shape == (B, 257 * CTX) and trk.reanchors == 0
    r0 = extend_rows()
    s1 = trk.observe(f1, a1)
    assert extend_rows() - r0 == B * 17
    s2 = trk.observe(f2, a2)
    assert extend_rows() - r0 == 2 * B * 17
    assert trk.steps == 2 and s1.shape == (B,) and s1.dtype == torch.float32 and torch.isfinite(s1).all() and (s1 > 0).all()
    # the tokens: the context's, then each observed frame's against the kept context -- and those of tokenize over the whole clip
    tok = vp.tokenizer
    ctx_px = context_of(obs)
    ids0, cache = tok.encode_context(ctx_px, CTX, return_cache=True)
    d1, d2 = (tok.tokenize_frames(f.to(DEV)[:, None] / 255., cache) for f in (f1, f2))
    assert torch.equal(trk.tokens, torch.cat([ids0, d1, d2], 1))
    full, _ = tok.tokenize(torch.cat([ctx_px, f1.to(DEV)[:, None] / 255., f2.to(DEV)[:, None] / 255.], 1), CTX)
    assert full.shape[1] == 257 * CTX - 1 + 17 * 2 and torch.equal(trk.tokens[:, :full.shape[1]], full)
    # the surprise: extend_kept_cache by hand, on a second model object taken through the same calls
    model = by_hand.model
    table = torch.zeros_like(trk.table)
    model.generate(ids0, do_sample=False, max_new_tokens=1, action=table)
    model.extend_kept_cache(ids0, action=table, keep=ids0.shape[1] - 1)
    tokens = ids0
    for d, a, s in ((d1, a1, s1), (d2, a2, s2)):
        table = table.clone()
        table[:, (tokens.shape[1] - 257 * CTX) // 17 + CTX - 1] = a.to(DEV)
        nll = model.extend_kept_cache(torch.cat([tokens, d], 1), action=table, keep=tokens.shape[1] - 1, return_nll=True)
        assert nll.shape == (B, 17)
        assert torch.equal(s, nll[:, :16].sum(1)), "observe's surprise is not the sum of the frame's 16 token NLLs"
        tokens = torch.cat([tokens, d], 1)
    assert torch.equal(trk.table, table)


@DTYPES
def test_plan_equals_fan_out_and_keeps_the_cache(tmp_path, llm_dtype):
    (vp,) = predictors(tmp_path, llm_dtype)
    B, k, horizon = 2, 3, 2
    obs, (f1,), (a1,) = episode(B, 1)
    trk = vp.track(obs)
    trk.observe(f1, a1)
    g = torch.Generator().manual_seed(3)
    plans = torch.randn(B * k, horizon, 4, generator=g)
    uni = torch.rand(B * k, 17 * horizon - 1, generator=g).to(DEV)
    obss, actions, rewards, unc = trk.plan(plans, samples=k, return_uncertainty=True, uniforms=uni)
    assert obss.shape == (B * k, horizon + 1, 9, 64, 64) and actions.shape == (B * k, horizon + 1, 4)
    assert rewards.shape == (B * k, horizon + 1, 1) and unc.shape == (B * k, horizon + 1, 1)
    again = trk.plan(plans, samples=k, return_uncertainty=True, uniforms=uni)
    for x, y, what in zip((obss, actions, rewards, unc), again, ("observations", "actions", "rewards", "uncertainty")):
        assert torch.equal(x, y), f"a second plan gave other {what}: the kept cache changed"
    # by hand
    from mbrl.video_predictor import symexp
    L0 = trk.tokens.shape[1]
    table = trk.table.repeat_interleave(k, 0)
    table[:, trk.steps + CTX - 1:trk.steps + CTX - 1 + horizon] = plans.to(DEV)
    tokens, hidden, scores = vp.model.fan_out(trk.tokens, k, action=table, max_new_tokens=17 * horizon - 1, uniforms=uni,
                                              output_frame_hidden_states=True, output_token_scores=True)
    clip = vp.tokenizer.detokenize(torch.cat([tokens[:, :257 * CTX], tokens[:, L0:]], 1), CTX)
    assert torch.equal(obss[:, 1:, 6:], clip[:, CTX:].clamp(0.0, 1.0)), "imagined frames"
    stack0 = torch.cat([obs.to(DEV)[:, 3:] / 255., f1.to(DEV) / 255.], 1)
    assert torch.equal(obss[:, 0], stack0.repeat_interleave(k, 0)), "step 0 is the observed stack, one copy per candidate"
    assert torch.equal(rewards[:, 1:, 0], symexp(vp.model.reward_linear(hidden).squeeze(-1)).float()) and (rewards[:, 0] == 0).all()
    assert torch.equal(unc[:, 1:, 0], scores.per_frame()[1].float())
    assert torch.equal(actions[:, 1:], plans.to(DEV)) and (actions[:, 0] == 0).all()
    # the kept cache is still the tracked prefix: a rollout on it is accepted
    out = vp.model.generate(trk.tokens, action=trk.table, reuse_cache=True, max_new_tokens=17)
    assert out.shape == (B, L0 + 17) and torch.equal(out[:, :L0], trk.tokens)


def test_select_then_observe_equals_the_gathered_rows(tmp_path):
    moved, untouched = predictors(tmp_path, "fp32", n=2)
    B = 2
    obs, (f1, f2), (a1, a2) = episode(B, 2)
    a, b = moved.track(obs), untouched.track(obs)
    for t in (a, b):
        t.observe(f1, a1)
    parents = [1, 1]                        # row 1 twice, row 0 dropped
    a.select(parents)
    assert a.batch == 2 and torch.equal(a.tokens, b.tokens[parents])
    sa, sb = a.observe(f2[parents], a2[parents]), b.observe(f2, a2)
    assert torch.equal(sa, sb[parents]), "surprise after select"
    assert torch.equal(a.tokens, b.tokens[parents]) and torch.equal(a.table, b.table[parents])
    for x, y in zip(a.stack, b.stack):
        assert torch.equal(x, y[parents])
    with pytest.raises(ValueError):
        a.select([0, 2])


def test_reanchor(tmp_path):
    (vp,) = predictors(tmp_path, "fp32", max_pos=257 * CTX + 17 * 2)
    B = 2
    obs, (f1, f2, f3), (a1, a2, a3) = episode(B, 3)
    trk = vp.track(obs)
    assert trk.max_steps == 2
    trk.observe(f1, a1)
    trk.observe(f2, a2)
    assert trk.reanchors == 0 and trk.steps == 2
    s3 = trk.observe(f3, a3)
    assert trk.reanchors == 1 and trk.steps == 1 and trk.tokens.shape == (B, 257 * CTX + 17)
    anchor = torch.stack([f1, f2], 1).to(DEV) / 255.   # the last ctx frames observed before this one
    ids0, cache = vp.tokenizer.encode_context(anchor, CTX, return_cache=True)
    assert torch.equal(trk.tokens[:, :257 * CTX], ids0)
    assert torch.equal(trk.tokens[:, 257 * CTX:], vp.tokenizer.tokenize_frames(f3.to(DEV)[:, None] / 255., cache))
    assert torch.isfinite(s3).all() and torch.equal(trk.table[:, CTX - 1], a3.to(DEV))
    # on_full="raise": RuntimeError, and the session is what it was
    trk = vp.track(obs, on_full="raise")
    trk.observe(f1, a1)
    trk.observe(f2, a2)
    tokens, table = trk.tokens.clone(), trk.table.clone()
    with pytest.raises(RuntimeError):
        trk.observe(f3, a3)
    assert trk.steps == 2 and trk.reanchors == 0 and torch.equal(trk.tokens, tokens) and torch.equal(trk.table, table)
    vp.model.extend_kept_cache(trk.tokens, action=trk.table, keep=trk.tokens.shape[1] - 1)   # the kept cache still is the tracked prefix
    trk.select([1, 0])
    assert torch.equal(trk.tokens, tokens[[1, 0]])
    with pytest.raises(ValueError):
        vp.track(obs, on_full="sometimes")
