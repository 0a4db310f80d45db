"""Per-frame rewards and hidden states of a forced-sdf rollout (include/ivg.h ivg_generate_frames), restated on the CPU oracle for
tests/test_frame_heads_cpu.py and tests/test_gpu_frame_heads.py.  No GPU import.

The reference is a TEACHER-FORCED pass of ``oracle.llama.LlamaRef`` over the finished token rows with the action embeddings on every
sdf slot (HeadModelWithAction.forward, action_model.py:154-205): causal attention makes the hidden state at a position the one the
rollout's forward pass of that token left, so ``hid`` at the position of frame i's 16th token, 257*ctx - 1 + 17*i + 16, is
``frame_hidden[:, i]`` and ``reward_linear`` of it ``frame_rewards[:, i]``."""
import numpy as np
import torch

from oracle.llama import LlamaRef

PER = 17   # 16 tokens of a frame + the forced sdf


def frames_out(n_new):
    """F_out of a call with ``n_new`` new tokens."""
    return n_new // PER


def frames_by_walking_the_step_loop(n_new):
    """The same number, counted the way the engine produces it: new tokens 1 .. n_new are decided, 1 .. n_new - 1 are fed (the last
    one is decided only), and the step that FEEDS new token j yields a frame when j is a frame's 16th token."""
    hits = []
    for j in range(1, n_new + 1):       # decide token j ...
        if j == n_new:
            break                       # ... the last one is never fed
        if j % PER == PER - 1:          # fed token j = 17 i + 16
            hits.append(j // PER)
    assert hits == list(range(len(hits))), "frames come in order, none skipped"
    return len(hits)


def frame_positions(ctx, n_frames, slot0=0):
    """Positions (in the token row) of the 16th token of frames 0 .. n_frames-1 of a call whose prompt already held ``slot0`` frames."""
    return [257 * ctx - 1 + PER * (slot0 + i) + 16 for i in range(n_frames)]


def fixture_state_dict(cfg, g, dtype=torch.float32):
    from ivideogpt_amd import weights as W
    sd = W.random_llama_state_dict(cfg, int(g["seed"]), action_dim=int(g["action_dim"]), reward_prediction=True)
    return {k: v.to(dtype) for k, v in sd.items()}


def fixture_action_table(g, extra_rows=1):
    """(B, ctx - 1 + steps + extra_rows, A): row i + ctx - 1 is the action of step i (zero rows elsewhere)."""
    ctx, acts = int(g["ctx"]), torch.from_numpy(g["actions"])
    table = torch.zeros(acts.shape[1], ctx - 1 + acts.shape[0] + extra_rows, acts.shape[2])
    for t in range(acts.shape[0]):
        table[:, ctx - 1 + t] = acts[t]
    return table


def fixture_final_ids(g, vocab):
    """prompt + per step (16 reference tokens + sdf): the finished rows of the reference's three steps, (B, 257*ctx + 17*steps)."""
    cols = [torch.from_numpy(g["prompt"])]
    sdf = torch.full((g["prompt"].shape[0], 1), vocab - 1, dtype=torch.int64)
    for t in range(g["step_tokens"].shape[0]):
        cols += [torch.from_numpy(g["step_tokens"][t]), sdf]
    return torch.cat(cols, 1)


@torch.no_grad()
def teacher_forced(sd, cfg, ids, table, ctx):
    """One pass over ``ids (B, L)`` with ``action_linear(table[:, i + ctx - 1])`` added on sdf slot i (position 257*ctx - 1 + 17*i)
    for every slot inside the row.  ``sd``: a HeadModelWithAction state dict, float32 or float64.
    -> (logits (B, L, V) fp32, hid (B, L, H) post final norm, in the state dict's dtype)."""
    dt = sd["llm.model.embed_tokens.weight"].dtype
    m = LlamaRef(sd, cfg["num_hidden_layers"], cfg["num_attention_heads"], cfg["rms_norm_eps"], cfg["rope_theta"],
                 cfg["max_position_embeddings"], prefix="llm.model.")
    x = m.embed(ids).clone()
    emb = torch.nn.functional.linear(table.to(dt), sd["action_linear.weight"], sd["action_linear.bias"])
    i = 0
    while 257 * ctx - 1 + PER * i < ids.shape[1]:
        x[:, 257 * ctx - 1 + PER * i] += emb[:, i + ctx - 1]
        i += 1
    logits, _, hid = m.forward_embeds(x, return_hidden=True)
    return logits, hid


def frame_outputs(sd, hid, ctx, n_frames, slot0=0):
    """-> (frame_hidden (B, F, H), frame_rewards (B, F)) read off a teacher-forced ``hid``."""
    fh = hid[:, frame_positions(ctx, n_frames, slot0)]
    fr = torch.nn.functional.linear(fh, sd["reward_linear.weight"], sd["reward_linear.bias"]).squeeze(-1)
    return fh, fr


_CACHE = {}


def fixture_reference(name="llama_tiny_ctx2_mbrl.npz", dtype=torch.float32):
    """The reference of the committed MBRL fixture, computed once per process and shared (read-only):
    dict(cfg, g, sd, ids, table, logits, hid, frame_hidden, frame_rewards)."""
    key = (name, dtype)
    if key not in _CACHE:
        from helpers import llama_fixture
        cfg, _, g = llama_fixture(name)
        ctx, steps = int(g["ctx"]), g["step_tokens"].shape[0]
        sd = fixture_state_dict(cfg, g, dtype)
        ids, table = fixture_final_ids(g, cfg["vocab_size"]), fixture_action_table(g)
        logits, hid = teacher_forced(sd, cfg, ids, table, ctx)
        fh, fr = frame_outputs(sd, hid, ctx, steps)
        _CACHE[key] = dict(cfg=cfg, g=g, sd=sd, ids=ids, table=table, logits=logits, hid=hid, frame_hidden=fh, frame_rewards=fr)
    return _CACHE[key]


def greedy_margin_and_tokens(ref):
    """The tokens the teacher-forced logits decide greedily at every sampled slot of the fixture's steps, (steps, B, 16), and the
    smallest top-2 logit margin among those decisions."""
    g, ctx = ref["g"], int(ref["g"]["ctx"])
    steps = g["step_tokens"].shape[0]
    toks, margin = [], np.inf
    for t in range(steps):
        p0 = 257 * ctx + PER * t                      # position of the frame's first token; it is decided at p0 - 1
        lg = ref["logits"][:, p0 - 1:p0 + 15]         # (B, 16, V)
        top = torch.topk(lg, 2, -1).values
        margin = min(margin, float((top[..., 0] - top[..., 1]).min()))
        toks.append(lg.argmax(-1).numpy())
    return np.stack(toks), margin
