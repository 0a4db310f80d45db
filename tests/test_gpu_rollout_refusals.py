"""What the rollout entries of include/ivg.h refuse, in which words: a table of (entry, arguments) -> (status, the whole ivg_last_error
string) on the tiny MBRL fixture model, an action-free model and one without a reward head.  Callers match on both the text and the
order of the checks, so both are pinned here.  Every case is an argument check that returns before any rollout launch; the greedy
rollout after the table equals the one before it."""
import ctypes as C

import numpy as np
import pytest
import torch

import frame_heads_ref as FR
from helpers import llama_fixture

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OK, INVALID, MISSING, CAPACITY = 0, -1, -2, -4
SENT = -12345
NO_KEPT = ("the engine holds no kept cache (the last call was not a per-trajectory generate within the cache chunk, or the format or scales "
           "changed since)")


def _p(t):
    from ivideogpt_amd.engine import _ptr
    return _ptr(t)


def call(eng, name, *args):
    """-> (status, ivg_last_error) of ``name(engine, *args, stream)``"""
    with eng.stream() as s:
        rc = getattr(eng.lib, name)(eng.h, *args, s)
    torch.cuda.synchronize()
    return rc, (eng.lib.ivg_last_error(eng.h) or b"").decode()


def make_models():
    """(wrapper with actions and reward head, the same without a reward head, action-free llm) on the fixture's config, fp32."""
    from ivideogpt_amd import HeadModelWithAction, LlamaForCausalLM, weights as W
    cfg, _, g = llama_fixture("llama_tiny_ctx2_mbrl.npz")
    adim, ctx, seed = int(g["action_dim"]), int(g["ctx"]), int(g["seed"])
    heads = []
    for reward in (True, False):
        head = HeadModelWithAction(LlamaForCausalLM(cfg, None, dtype="fp32"), adim, 257 * ctx - 1, 16, ctx, ctx + 3, reward_prediction=reward)
        head.load_state_dict(W.random_llama_state_dict(cfg, seed, action_dim=adim, reward_prediction=reward), strict=True)
        heads.append(head.to(DEV))
    free = LlamaForCausalLM(cfg, W.random_llama_state_dict(cfg, seed), dtype="fp32").to(DEV)
    return cfg, g, heads[0], heads[1], free


def test_refusals_by_status_and_text():
    cfg, g, head, bare, free = make_models()
    ctx = int(g["ctx"])
    prompt = torch.from_numpy(g["prompt"]).to(DEV).contiguous()                  # (2, 514)
    table = FR.fixture_action_table(g).to(DEV).contiguous()                      # (2, 5, A)
    T, L0 = table.shape[1], prompt.shape[1]
    assert (prompt.shape[0], L0, ctx) == (2, 514, 2)
    eng, beng, feng = head.llm._ensure(4, T), bare.llm._ensure(4, T), free._ensure(4)
    Lmax = int(eng.cfg.max_seq) or int(eng.cfg.max_position_embeddings)
    chunk = min(int(eng.cfg.max_batch), 128)
    assert chunk == 4
    ids = torch.full((8 * (Lmax + 8),), SENT, dtype=torch.int64, device=DEV)
    fr = torch.full((8 * 64,), float(SENT), dtype=torch.float32, device=DEV)
    fh = torch.full((8 * 64 * cfg["hidden_size"],), float(SENT), dtype=torch.float32, device=DEV)
    ts = torch.full((8 * Lmax * 3,), float(SENT), dtype=torch.float32, device=DEV)

    def greedy():
        out = torch.empty(2, L0 + 17, dtype=torch.int64, device=DEV)
        rc, err = call(eng, "ivg_generate", _p(prompt), prompt.stride(0), 2, L0, 17, _p(table), T, ctx, None, 100, _p(out), None)
        assert rc == OK, err
        return out

    before = greedy()                                                            # keeps a cache of 530 positions of 2 trajectories
    grown = before.contiguous()                                                  # (2, 531): ends with the forced sdf
    other = grown.clone()
    other[0, 520] = (other[0, 520] + 1) % 100
    longer = torch.cat([prompt, prompt[:, :1]], 1).contiguous()                  # L0 = 515
    table6 = table.repeat(3, 1, 1).contiguous()
    emb = torch.zeros(5, 4, cfg["hidden_size"], dtype=torch.float32, device=DEV)
    new_ids = ids[:5 * 8]
    parents = np.zeros(2, dtype=np.int32)
    reused = C.c_int(0)

    def gen(p, B, L, n, act, aT, reward=None):
        return (_p(p), p.stride(0), B, L, n, _p(act), aT, ctx, None, 100, _p(ids), _p(reward))

    def shared(p, groups, size, L, n, act, aT, force=0):
        return (_p(p), p.stride(0), groups, size, L, n, _p(act), aT, ctx, None, 100, force, _p(ids), None)

    def frames(p, B, L, n, act, aT, group=1, kept=0, force=0, rew=fr, hid=fh):
        return (_p(p), p.stride(0), B, L, n, _p(act), aT, ctx, None, 100, group, kept, force, _p(ids), _p(rew), _p(hid))

    def fanout(p, groups, size, L, n, act, aT, rew=fr):
        return (_p(p), p.stride(0), groups, size, L, n, _p(act), aT, ctx, None, 100, 0, _p(ids), _p(rew), None, _p(ts))

    def embeds(e, B, L, n):
        return (_p(e), B, L, n, None, 100, _p(new_ids), None, 1, C.byref(reused))

    act_free = "generate: actions given but the model is action-free"
    prompt_len = "generate: action-conditioned prompt must hold 257*ctx + 17*t tokens"
    cont_only = "generate_continue: action-conditioned models only"
    sizes = "generate_frames: B must be a positive multiple of a positive group_size"
    cases = [
        # ---- capacity and actions
        ("over the cache", eng, "ivg_generate", gen(prompt, 2, L0, Lmax - L0 + 1, table, T), CAPACITY,
         f"generate: sequence of {Lmax + 1} tokens exceeds the KV cache ({Lmax})"),
        ("actions on an action-free model", feng, "ivg_generate", gen(prompt, 2, L0, 17, table, T), INVALID, act_free),
        ("action prompt of 515 tokens", eng, "ivg_generate", gen(longer, 2, 515, 17, table, T), INVALID, prompt_len),
        ("action table too short", eng, "ivg_generate", gen(prompt, 2, L0, 17, table, 2), INVALID,
         "generate: action tensor too short (or longer than max_frames)"),
        ("action table longer than max_frames", eng, "ivg_generate", gen(prompt, 2, L0, 17, table, T + 1), INVALID,
         "generate: action tensor too short (or longer than max_frames)"),
        # ---- ivg_generate_shared
        ("shared: no groups", eng, "ivg_generate_shared", shared(prompt, 0, 2, L0, 17, None, 0), INVALID,
         "generate_shared: n_groups and group_size must be positive"),
        ("shared: group_size 0", eng, "ivg_generate_shared", shared(prompt, 2, 0, L0, 17, None, 0), INVALID,
         "generate_shared: n_groups and group_size must be positive"),
        ("shared: action prompt beyond the context", eng, "ivg_generate_shared", shared(grown, 2, 2, 531, 17, table6, T), INVALID,
         "generate_shared: an action-conditioned shared prompt must hold exactly 257*ctx tokens"),
        ("shared: group_size 1 and L0 1 (the shared length rule, nothing shared)", eng, "ivg_generate_shared", shared(prompt, 2, 1, 1, 4, None, 0), CAPACITY,
         f"generate: sequence of 5 tokens exceeds the KV cache ({Lmax})"),
        # ---- ivg_generate_continue
        ("continue: action-free model", feng, "ivg_generate_continue", gen(grown, 2, 531, 17, None, 0), INVALID, cont_only),
        ("continue: no actions", eng, "ivg_generate_continue", gen(grown, 2, 531, 17, None, 0), INVALID, cont_only),
        ("continue: no kept cache", beng, "ivg_generate_continue", gen(grown, 2, 531, 17, table, T), INVALID,
         "generate_continue: the KV cache holds 0 positions of 0 trajectories, the call needs 530 of 2"),
        ("continue: kept cache of another length", eng, "ivg_generate_continue", gen(prompt, 2, L0, 17, table, T), INVALID,
         "generate_continue: the KV cache holds 530 positions of 2 trajectories, the call needs 513 of 2"),
        ("continue: another prefix", eng, "ivg_generate_continue", gen(other, 2, 531, 17, table, T), INVALID,
         "generate_continue: the KV cache was built from a different prefix (tokens or actions differ)"),
        # ---- ivg_generate_frames
        ("frames: 16 new tokens", eng, "ivg_generate_frames", frames(prompt, 2, L0, 16, table, T), INVALID,
         "generate_frames: a frame needs 17 new tokens (its 16th must be fed)"),
        ("frames: unforced schedule", eng, "ivg_generate_frames", frames(prompt, 2, L0, 17, None, 0), INVALID,
         "generate_frames: frames exist under the forced-sdf schedule only (actions or force_sdf)"),
        ("frames: 515 tokens with actions (the transformer check comes first)", eng, "ivg_generate_frames", frames(longer, 2, 515, 17, table, T), INVALID, prompt_len),
        ("frames: 515 tokens under force_sdf", eng, "ivg_generate_frames", frames(longer, 2, 515, 17, None, 0, force=1), INVALID,
         "generate_frames: the prompt must hold 257*ctx + 17*t tokens (frames count from the first new token)"),
        ("frames: rewards without a reward head", beng, "ivg_generate_frames", frames(prompt, 2, L0, 17, table, T, hid=None), MISSING,
         "generate_frames: rewards requested but reward_linear is not loaded"),
        ("frames: kept cache with a group", eng, "ivg_generate_frames", frames(grown, 2, 531, 17, table, T, group=2, kept=1), INVALID,
         "generate_frames: a kept cache is per trajectory (group_size must be 1)"),
        ("frames: B no multiple of the group", eng, "ivg_generate_frames", frames(prompt, 3, L0, 17, table6, T, group=2), INVALID, sizes),
        ("frames: kept cache of another prefix", eng, "ivg_generate_frames", frames(other, 2, 531, 17, table, T, kept=1), INVALID,
         "generate_continue: the KV cache was built from a different prefix (tokens or actions differ)"),
        ("scored: kept cache without actions", eng, "ivg_generate_scored", frames(grown, 2, 531, 17, None, 0, kept=1, rew=None, hid=None) + (_p(ts),), INVALID,
         cont_only),
        # ---- ivg_generate_fanout
        ("fanout: no groups (the frames entry's words)", eng, "ivg_generate_fanout", fanout(grown, 0, 2, 531, 17, table6, T), INVALID, sizes),
        ("fanout: group_size 0", eng, "ivg_generate_fanout", fanout(grown, 2, 0, 531, 17, table6, T), INVALID, sizes),
        ("fanout: more candidates than the chunk", eng, "ivg_generate_fanout", fanout(grown, 2, 3, 531, 17, table6, T), CAPACITY,
         f"generate_fanout: 6 candidates exceed the KV-cache chunk ({chunk})"),
        ("fanout: no kept cache", beng, "ivg_generate_fanout", fanout(grown, 2, 2, 531, 17, table6, T, rew=None), INVALID,
         "generate_fanout: the kept KV cache holds 0 positions of 0 trajectories built from ids, the call needs 530 of 2"),
        ("fanout: another prefix", eng, "ivg_generate_fanout", fanout(other, 2, 2, 531, 17, table6, T), INVALID,
         "generate_fanout: the kept KV cache was built from a different prefix (tokens, context length or action conditioning differ)"),
        # ---- ivg_generate_embeds
        ("embeds: null argument", eng, "ivg_generate_embeds", embeds(None, 2, 4, 4), INVALID, "generate_embeds: null argument"),
        ("embeds: batch over the chunk", eng, "ivg_generate_embeds", embeds(emb, 5, 4, 4), CAPACITY,
         f"generate_embeds: batch 5 / sequence of 8 tokens exceeds the capacity ({chunk} x {Lmax})"),
        ("embeds: over the cache", eng, "ivg_generate_embeds", embeds(emb, 2, 4, Lmax), CAPACITY,
         f"generate_embeds: batch 2 / sequence of {Lmax + 4} tokens exceeds the capacity ({chunk} x {Lmax})"),
        # ---- the kept-cache operations
        ("kv_select: no kept cache", beng, "ivg_kv_select", (parents.ctypes.data_as(C.c_void_p), 2), INVALID, "kv_select: " + NO_KEPT),
        ("kv_extend: no kept cache", beng, "ivg_kv_extend", (_p(grown), grown.stride(0), 2, 530, 531, _p(table), T, ctx, None), INVALID,
         "kv_extend: " + NO_KEPT),
    ]
    for what, e, name, args, status, text in cases:
        rc, err = call(e, name, *args)
        assert (rc, err) == (status, text), f"{what}: {name} -> status {rc}, {err!r}"
    for buf in (ids, fr, fh, ts):
        assert (buf == SENT).all(), "a refused call wrote an output"
    assert reused.value == 0
    assert torch.equal(greedy(), before), "the greedy rollout after the refusals differs from the one before them"
