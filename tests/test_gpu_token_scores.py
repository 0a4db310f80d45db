"""Token log-probabilities and predictive entropy from rollouts (include/ivg.h ivg_generate_scored; token_scores_kernel inside the decode
steps) on the MI355X: the kernel through ivg_op_token_scores against the fp64 reference of tests/token_scores_ref.py on its whole case
table, the in-engine scores against the teacher-forced oracle and ``token_nll``, bit for bit against the step-by-step route, their
independence from the sampler's settings, shared contexts and the second cache chunk, the untouched off path, the refusals through the
C ABI with guarded buffers, and ``VideoPredictor``'s ``return_uncertainty``.  Tiny model throughout (hidden 128, 2 layers, 2 heads of
64, L0 = 514), B = 3, 50 or 51 new tokens: the eager first step, the 8-step graph, the single-step tail and the decide-only last step."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import frame_heads_ref as FR
import token_scores_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PROFILES = pytest.mark.parametrize("lds_kb", [0, 40], ids=["one_batch", "batches_in_flight"])
OK, INVALID, MISSING, CAPACITY = 0, -1, -2, -4
L0 = 514
FORCED = [c for c in range(51) if (c + 1) % 17 == 0]       # columns of new tokens 17, 34, 51
SAMPLED = [c for c in range(51) if (c + 1) % 17 != 0]


def lib():
    from ivideogpt_amd import _lib
    return _lib.load()


def counter(name=b"token_scores"):
    return lib().ivg_debug_counter(name)


def make_head(dtype="fp32", lds_kb=0, kv=None):
    """The MBRL fixture's model (seeded weights) under the wrapper; 3 future frames."""
    from ivideogpt_amd import HeadModelWithAction, LlamaForCausalLM, weights as W
    ref = FR.fixture_reference()
    cfg, g = ref["cfg"], ref["g"]
    adim, ctx = int(g["action_dim"]), int(g["ctx"])
    sd = W.random_llama_state_dict(cfg, int(g["seed"]), action_dim=adim, reward_prediction=True)
    head = HeadModelWithAction(LlamaForCausalLM(cfg, None, dtype=dtype, decode_lds_kb=lds_kb), adim, 257 * ctx - 1, 16, ctx, ctx + 3,
                               reward_prediction=True)
    head.load_state_dict(sd, strict=True)
    head.to(DEV)
    if kv is not None:
        head.set_kv_cache_dtype("fp8_e4m3", **kv)
    return head


def three_rows(seed=7):
    """B = 3 prompts (the fixture's two and a splice of them), an action table and a (3, 51) table of uniforms."""
    ref = FR.fixture_reference()
    prompt = torch.from_numpy(ref["g"]["prompt"]).to(DEV)
    third = prompt[1].clone()
    third[5:200] = prompt[0, 5:200]
    g = torch.Generator().manual_seed(seed)
    table = torch.randn(3, ref["table"].shape[1], ref["table"].shape[2], generator=g).to(DEV)
    uni = torch.rand(3, 51, generator=g).to(DEV)
    return torch.cat([prompt, third[None]], 0), table, uni


def stack(sc):
    """TokenScores -> (B, n, 3) float64 numpy"""
    return torch.stack(list(sc), -1).double().cpu().numpy()


def oracle_scores(tokens, table, n):
    """The teacher-forced oracle over the finished rows ``tokens (B, L0 + n)``: the logits at position L0 + j - 2 are the row the
    sampler read for new token j.  -> (reference (B, n, 3) with the forced columns zero, entropy sensitivity (B, n))."""
    ref = FR.fixture_reference()
    logits, _ = FR.teacher_forced(ref["sd"], ref["cfg"], tokens.cpu(), table.cpu(), int(ref["g"]["ctx"]))
    rows = logits[:, L0 - 1:L0 - 1 + n].numpy()
    new = tokens[:, L0:L0 + n].cpu().numpy()
    want = np.stack([R.reference_columns(rows[b], new[b], R.PER) for b in range(rows.shape[0])])
    sens = np.stack([R.entropy_sensitivity(rows[b]) for b in range(rows.shape[0])])
    return want, sens


def assert_close_to_oracle(got, want, sens, what):
    """The bounds of a 1e-3 logits parity: 2e-3 on the two log-probabilities, 1e-3 * sum p |log p + H| + 1e-4 on the entropy."""
    n = got.shape[1]
    forced = [c for c in FORCED if c < n]
    sampled = [c for c in SAMPLED if c < n]
    assert (got[:, forced] == 0).all(), f"{what}: a forced column is not exactly 0"
    d = np.abs(got - want)[:, sampled]
    e_bound = 1e-3 * sens[:, sampled] + 1e-4
    print(f"{what}: |d logprob| {d[..., 0].max():.2e}, |d max_logprob| {d[..., 2].max():.2e} (bound 2e-3); |d entropy| {d[..., 1].max():.2e} "
          f"(smallest bound {e_bound.min():.2e}, largest ratio {(d[..., 1] / e_bound).max():.3f})")
    assert d[..., 0].max() <= 2e-3 and d[..., 2].max() <= 2e-3, what
    assert (d[..., 1] <= e_bound).all(), what


# ------------------------------------------------------------------------------------------------ 1. the kernel against fp64
SENT_F, SENT_I, GUARD = -777.25, -12345, 64


class Guarded:
    """A device buffer of ``n`` elements with GUARD sentinel elements on both sides, all filled with the sentinel."""

    def __init__(self, n, dtype, sentinel):
        self.n, self.sent = n, sentinel
        self.buf = torch.full((n + 2 * GUARD,), sentinel, dtype=dtype, device=DEV)
        self.view = self.buf[GUARD:GUARD + n]

    def guards_intact(self):
        return bool((self.buf[:GUARD] == self.sent).all() and (self.buf[GUARD + self.n:] == self.sent).all())

    def untouched(self):
        return bool((self.buf == self.sent).all())

    def filled(self):
        return bool((self.view != self.sent).all())


def op_scores(z, tok):
    from ivideogpt_amd.engine import _ptr
    B, V = z.shape
    zd, td = torch.from_numpy(np.array(z)).to(DEV), torch.from_numpy(np.array(tok)).to(DEV)      # (copies: the table is read-only)
    out = Guarded(B * 3, torch.float32, SENT_F)
    rc = lib().ivg_op_token_scores(_ptr(zd), _ptr(td), B, V, _ptr(out.view), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == OK and out.guards_intact(), "a guard word around `out` was overwritten"
    return out.view.view(B, 3).cpu().numpy()


@pytest.mark.parametrize("case", list(R.cases()))
def test_kernel_against_fp64(case):
    """Every row of the table, per output, under 1e-4 absolute (-inf matches -inf); the non-finite rows give NaN in all three.  The rows
    of V = 1001 are 4-byte aligned, those of 130 and the odd rows of 16,386 8-byte, the rest 16-byte: all three load paths."""
    z, tok = R.cases()[case]
    got, want = op_scores(z, tok), R.reference(z, tok)
    ok = R.within(got, want)
    fin = np.isfinite(want)
    if fin.any():
        print(f"{case}: worst |kernel - fp64| = {np.abs(got[fin] - want[fin]).max():.2e}")
    for b in range(z.shape[0]):
        for k, name in enumerate(("logprob", "entropy", "max_logprob")):
            assert ok[b, k], f"{case} row {b}: {name} {got[b, k]!r} against fp64 {want[b, k]!r}"
    if case == "nonfinite":
        assert np.isnan(got).all()
    else:
        assert got[1, 0] == got[1, 2] and got[4, 0] == got[4, 2], "id = arg-max: logprob and max_logprob are the same bits"
        # an id outside [0, V): NaN logprob, the other two as before; nothing is read for it
        bad = np.array(tok)
        bad[0], bad[1] = z.shape[1], -1
        g2 = op_scores(z, bad)
        assert np.isnan(g2[:2, 0]).all() and np.array_equal(g2[:, 1:], got[:, 1:]) and np.array_equal(g2[2:, 0], got[2:, 0])


# ------------------------------------------------------------------------------------------------ 2. in the engine against the oracle
@PROFILES
def test_scores_match_the_teacher_forced_oracle(lds_kb):
    """Sampled with uniforms and actions, fp32: per column against the oracle's logits of the same tokens, and -logprob against
    ``token_nll`` of ``model(input_ids=tokens, labels=tokens)`` at the shifted positions."""
    head = make_head(lds_kb=lds_kb)
    ids, table, uni = three_rows()
    u = uni[:, :50].contiguous()
    c0 = counter()
    out, sc = head.generate(ids, do_sample=True, top_k=100, max_new_tokens=50, action=table, uniforms=u, output_token_scores=True)
    assert counter() - c0 == 50
    assert type(sc).__name__ == "TokenScores" and sc._fields == ("logprob", "entropy", "max_logprob")
    assert all(t.shape == (3, 50) and t.dtype == torch.float32 for t in sc)
    plain = head.generate(ids, do_sample=True, top_k=100, max_new_tokens=50, action=table, uniforms=u)
    assert torch.equal(out, plain), "the scored call decides other tokens than the plain one"
    got = stack(sc)
    want, sens = oracle_scores(out, table, 50)
    assert_close_to_oracle(got, want, sens, f"lds_kb {lds_kb}")
    assert (got[..., 0] <= 0).all() and (got[..., 2] >= got[..., 0]).all() and (got[:, SAMPLED, 1] > 0).all()
    x, _ = head(input_ids=out, labels=out, action=table)
    nll = x.token_nll.double().cpu().numpy()
    cols = np.array(SAMPLED)
    d = np.abs(-got[:, cols, 0] - nll[:, L0 - 1 + cols]).max()      # new token j = c + 1 sits at position L0 + c, predicted at L0 + c - 1
    print(f"|-logprob - token_nll| = {d:.2e}")
    assert d <= 2e-3
    flp, fen = sc.per_frame()
    assert flp.shape == fen.shape == (3, 3)
    for i in range(3):
        assert np.abs(flp[:, i].double().cpu().numpy() - got[:, 17 * i:17 * i + 16, 0].sum(-1)).max() < 1e-4
        assert np.abs(fen[:, i].double().cpu().numpy() - got[:, 17 * i:17 * i + 16, 1].mean(-1)).max() < 1e-5


# ------------------------------------------------------------------------------------------------ 3. bitwise: one call == step by step
FLAVOURS = {"fp32": ("fp32", None), "bf16": ("bf16", None), "bf16_fp8": ("bf16", dict(k_scale=1.0, v_scale=1.0)), "x3": ("x3", None)}


@pytest.mark.parametrize("flavour", list(FLAVOURS))
def test_one_call_equals_step_by_step_bitwise(flavour):
    dtype, kv = FLAVOURS[flavour]
    head = make_head(dtype, kv=kv)
    ids, table, uni = three_rows()
    c0 = counter()
    out, sc = head.generate(ids, do_sample=True, top_k=100, max_new_tokens=51, action=table, uniforms=uni, output_token_scores=True)
    assert counter() - c0 == 51, "one launch per step that ran the sampler"
    again, sc2 = head.generate(ids, do_sample=True, top_k=100, max_new_tokens=51, action=table, uniforms=uni, output_token_scores=True)
    assert torch.equal(again, out) and all(torch.equal(a, b) for a, b in zip(sc, sc2)), "two identical calls differ (eager / replayed graph)"
    tokens, steps = ids, []
    c0 = counter()
    for t in range(3):
        tokens, s = head.generate(tokens, do_sample=True, top_k=100, max_new_tokens=17, action=table, uniforms=uni[:, 17 * t:17 * t + 17].contiguous(),
                                  reuse_cache=t > 0, output_token_scores=True)
        steps.append(s)
    assert counter() - c0 == 17 + 18 + 18, "a kept-cache call runs the sampler once more, for j = 0, which writes nothing"
    assert torch.equal(out, tokens), f"{(out != tokens).sum().item()} tokens differ between one call and three"
    for k, name in enumerate(sc._fields):
        whole, parts = sc[k], torch.cat([s[k] for s in steps], 1)
        print(f"{flavour} {name}: max |one call - step by step| = {(whole - parts).abs().max().item():.3e}")
        assert torch.equal(whole, parts), f"{name} differs between one call and three kept-cache calls"
        assert (whole[:, FORCED] == 0).all() and torch.isfinite(whole).all()
    assert (sc.entropy[:, SAMPLED] > 0).all() and (sc.entropy <= math.log(16386) + 1e-4).all()
    # greedy: the chosen token is the arg-max
    _, g = head.generate(ids, do_sample=False, max_new_tokens=51, action=table, output_token_scores=True)
    assert torch.equal(g.logprob, g.max_logprob), "greedy: logprob and max_logprob are not the same bits"
    assert (sc.logprob <= sc.max_logprob).all()


# ------------------------------------------------------------------------------------------------ 4. the sampler's settings
def test_scores_do_not_depend_on_the_samplers_settings():
    """The first new column is decided on the prompt pass's logits, the same row whatever the sampler does with it: entropy and
    max_logprob are the same bits across temperature and top_p, and logprob on the rows whose first token coincides."""
    head = make_head()
    ids, table, uni = three_rows(5)
    u = uni[:, :17].contiguous()
    runs = {}
    for temperature in (1.0, 0.7):
        for top_p in (None, 0.9):
            out, sc = head.generate(ids, do_sample=True, top_k=100, temperature=temperature, top_p=top_p, max_new_tokens=17, action=table, uniforms=u,
                                    output_token_scores=True)
            runs[(temperature, top_p)] = (out[:, L0], sc)
    tok0, sc0 = runs[(1.0, None)]
    for key, (tok, sc) in runs.items():
        assert torch.equal(sc.entropy[:, 0], sc0.entropy[:, 0]) and torch.equal(sc.max_logprob[:, 0], sc0.max_logprob[:, 0]), key
        same = tok == tok0
        print(f"{key}: {int(same.sum())} of 3 first tokens coincide")
        assert torch.equal(sc.logprob[same, 0], sc0.logprob[same, 0]), key
    _, g = head.generate(ids, do_sample=False, max_new_tokens=17, action=table, output_token_scores=True)
    assert torch.equal(g.entropy[:, 0], sc0.entropy[:, 0]) and torch.equal(g.max_logprob[:, 0], sc0.max_logprob[:, 0]), "greedy"


# ------------------------------------------------------------------------------------------------ 5. shared context, chunks
def test_shared_context_rows_in_the_callers_order():
    ref = FR.fixture_reference()
    prompt = torch.from_numpy(ref["g"]["prompt"]).to(DEV)
    g = torch.Generator().manual_seed(13)
    ids = prompt.repeat(2, 1)                                             # rows k * 2 + b: sample k of prompt b
    table = torch.randn(4, ref["table"].shape[1], ref["table"].shape[2], generator=g).to(DEV)
    head = make_head()
    plain, ps = head.generate(ids, do_sample=False, max_new_tokens=50, action=table, output_token_scores=True)
    c0 = counter()
    shared, ss = head.generate(ids, do_sample=False, max_new_tokens=50, action=table, output_token_scores=True, shared_context=2)
    assert counter() - c0 == 51, "a shared-context call runs the sampler once more, for j = 0"
    assert torch.equal(shared, plain), "shared-context tokens differ from the plain run"
    want, sens = oracle_scores(plain, table, 50)
    assert_close_to_oracle(stack(ps), want, sens, "plain")
    assert_close_to_oracle(stack(ss), stack(ps), sens, "shared against plain")
    assert not torch.equal(ps.entropy[0], ps.entropy[2]), "rows 0 and 2 share a prompt, not their actions"
    # action-free model, HF-style generate
    from ivideogpt_amd import LlamaForCausalLM, weights as W
    llm = LlamaForCausalLM(ref["cfg"], W.random_llama_state_dict(ref["cfg"], 5), dtype="fp32").to(DEV)
    p, s1 = llm.generate(ids, do_sample=False, max_new_tokens=20, output_token_scores=True)
    sh, s2 = llm.generate(ids, do_sample=False, max_new_tokens=20, output_token_scores=True, shared_context="auto")
    assert torch.equal(p, llm.generate(ids, do_sample=False, max_new_tokens=20)) and torch.equal(sh, p)
    assert (s1.entropy > 0).all(), "no forced columns without the forced schedule"
    assert np.abs(stack(s1) - stack(s2))[..., [0, 2]].max() <= 2e-3 and torch.equal(s1.logprob, s1.max_logprob)


def test_rows_of_the_second_chunk():
    """B = 130 > the 128-row cache chunk: rows 126 .. 129 (two of each chunk) equal the same rows run alone as a batch of 4."""
    ref = FR.fixture_reference()
    prompt = torch.from_numpy(ref["g"]["prompt"]).to(DEV)
    g = torch.Generator().manual_seed(19)
    V = ref["cfg"]["vocab_size"]
    ids = prompt[torch.arange(130) % 2].clone()
    ids[:, 5:200] = torch.randint(0, V - 2, (130, 195), generator=g).to(DEV)
    table = torch.randn(130, 3, 4, generator=g).to(DEV)
    head = make_head()
    c0 = counter()
    out, sc = head.generate(ids, do_sample=False, max_new_tokens=16, action=table, output_token_scores=True)
    assert counter() - c0 == 32, "16 launches per chunk"
    sel = slice(126, 130)
    o4, s4 = head.generate(ids[sel].contiguous(), do_sample=False, max_new_tokens=16, action=table[sel].contiguous(), output_token_scores=True)
    assert torch.equal(out[sel], o4), "tokens of rows 126..129 differ from the batch of 4"
    for k, name in enumerate(sc._fields):
        print(f"rows 126..129 vs alone, {name}: {(sc[k][sel] - s4[k]).abs().max().item():.3e}")
        assert torch.equal(sc[k][sel], s4[k]), name
    assert torch.isfinite(sc.entropy).all() and (sc.entropy > 0).all()


# ------------------------------------------------------------------------------------------------ 6. the off path
def test_off_path_is_untouched():
    ids, table, uni = three_rows(23)
    u = uni[:, :50].contiguous()
    head = make_head()

    def off_calls(**kw):
        a = head.generate(ids, do_sample=True, max_new_tokens=50, action=table, uniforms=u, **kw)
        b = head.generate(ids, do_sample=True, max_new_tokens=50, action=table, uniforms=uni, return_reward="frames", output_frame_hidden_states=True, **kw)
        emb = head.get_input_embeddings(ids)
        e = head.llm.generate(inputs_embeds=emb, do_sample=True, max_new_tokens=17, uniforms=uni[:, :17].contiguous(), use_cache=False,
                              return_dict_in_generate=True, output_hidden_states=True, **kw)
        assert not hasattr(e, "token_scores")
        return [a, *b, e.sequences, e.hidden_states[-1][-1]]

    c0 = counter()
    before = off_calls()
    assert counter() == c0, "a call without scores ran the score kernel"
    out, sc = head.generate(ids, do_sample=True, max_new_tokens=50, action=table, uniforms=u, output_token_scores=True)
    o2, fr, fh, sc2 = head.generate(ids, do_sample=True, max_new_tokens=50, action=table, uniforms=uni, return_reward="frames",
                                    output_frame_hidden_states=True, output_token_scores=True)
    e = head.llm.generate(inputs_embeds=head.get_input_embeddings(ids), do_sample=True, max_new_tokens=17, uniforms=uni[:, :17].contiguous(), use_cache=False,
                          return_dict_in_generate=True, output_hidden_states=True, output_token_scores=True)
    assert counter() - c0 == 50 + 51 + 17
    c1 = counter()
    after = off_calls()
    explicit = off_calls(output_token_scores=False)
    assert counter() == c1
    for x, y, z in zip(before, after, explicit):
        assert torch.equal(x, y) and torch.equal(x, z), "an unscored call changed after a scored one"
    # the scored calls give the other results of the unscored ones, and one another's scores
    for x, y in zip(before, [out, o2, fr, fh, e.sequences, e.hidden_states[-1][-1]]):
        assert torch.equal(x, y), "a scored call's tokens / rewards / hidden states differ from the unscored call's"
    assert all(torch.equal(a, b) for a, b in zip(sc, sc2)), "scores with and without the frame outputs differ"
    assert e.token_scores.logprob.shape == (3, 17) and (e.token_scores.entropy > 0).all(), "the embeds path forces no column"
    # with the single reward of a whole number of frames; generate_without_action
    o17, r17 = head.generate(ids, do_sample=True, max_new_tokens=17, action=table, uniforms=uni[:, :17].contiguous(), return_reward=True)
    s17 = head.generate(ids, do_sample=True, max_new_tokens=17, action=table, uniforms=uni[:, :17].contiguous(), return_reward=True, output_token_scores=True)
    assert len(s17) == 3 and torch.equal(s17[0], o17) and torch.equal(s17[1], r17) and torch.equal(s17[2].logprob, sc.logprob[:, :17])
    w = head.generate_without_action(ids, do_sample=True, max_new_tokens=50, uniforms=u)
    w2, ws = head.generate_without_action(ids, do_sample=True, max_new_tokens=50, uniforms=u, output_token_scores=True)
    w3, wh, ws3 = head.generate_without_action(ids, do_sample=True, max_new_tokens=50, uniforms=u, output_frame_hidden_states=True, output_token_scores=True)
    assert torch.equal(w2, w) and torch.equal(w3, w) and torch.equal(ws.entropy, ws3.entropy) and (ws.entropy[:, [16, 33]] == 0).all()


# ------------------------------------------------------------------------------------------------ 7. refusals, column counts (C ABI)
def raw_scored(eng, prompt, B, L0_, n_new, actions, ctx, ids, fr, fh, ts, uniforms=None, group=1, kept=0, force=0):
    from ivideogpt_amd.engine import _ptr
    act_T = actions.shape[1] if actions is not None else 0
    with eng.stream() as s:
        rc = eng.lib.ivg_generate_scored(eng.h, _ptr(prompt), prompt.stride(0), B, L0_, n_new, _ptr(actions), act_T, ctx, _ptr(uniforms), 100,
                                         group, kept, force, _ptr(ids), _ptr(fr), _ptr(fh), _ptr(ts), s)
    torch.cuda.synchronize()
    return rc


def test_refusals_and_column_counts():
    ref = FR.fixture_reference()
    prompt, table = torch.from_numpy(ref["g"]["prompt"]).to(DEV), ref["table"].to(DEV)
    head = make_head()
    eng = head.llm._ensure(2, 32)      # (no later call of this test asks for more: the handle stays the live engine's)
    first = head.generate(prompt, do_sample=False, max_new_tokens=17, action=table).contiguous()     # keeps the cache of 514 + 16 positions
    ids, fr, ts = Guarded(2 * 1100, torch.int64, SENT_I), Guarded(2 * 64, torch.float32, SENT_F), Guarded(2 * 600 * 3, torch.float32, SENT_F)
    cases = {
        "a frame output with an unforced schedule": (INVALID, dict(n_new=17, actions=None, fr=fr.view)),
        "a frame output with n_new = 16": (INVALID, dict(n_new=16, actions=table, fr=fr.view)),
        "beyond the cache": (CAPACITY, dict(n_new=511, actions=table, fr=None)),
        "beyond the cache, action-free": (CAPACITY, dict(n_new=511, actions=None, fr=None)),
    }
    c0 = counter()
    for what, (status, kw) in cases.items():
        rc = raw_scored(eng, prompt, 2, L0, kw["n_new"], kw["actions"], 2, ids.view, kw["fr"], None, ts.view)
        assert rc == status, f"{what}: status {rc}, expected {status}"
        assert ids.untouched() and fr.untouched() and ts.untouched(), f"{what}: an output was written"
    assert counter() == c0
    # the kept cache is still the first call's: the continuation is accepted (verified on the device) and gives the greedy tokens
    ts17 = Guarded(2 * 17 * 3, torch.float32, SENT_F)
    assert raw_scored(eng, first, 2, 531, 17, table, 2, ids.view[:2 * 548], None, None, ts17.view, kept=1) == OK
    assert counter() - c0 == 18
    assert torch.equal(ids.view[:2 * 548].view(2, 548)[:, 531:547].cpu(), torch.from_numpy(ref["g"]["step_tokens"][1]))
    assert ts17.guards_intact() and ts17.filled() and (ts17.view.view(2, 17, 3)[:, 16] == 0).all()
    # n_new = 1 and an n_new that is no multiple of 17 write exactly n_new columns; without frame outputs the entry needs no forced
    # schedule and no whole frame, and serves the action-free ivg_generate too
    for n_new, actions in ((1, table), (20, table), (20, None)):
        out, t = Guarded(2 * (L0 + n_new), torch.int64, SENT_I), Guarded(2 * n_new * 3, torch.float32, SENT_F)
        assert raw_scored(eng, prompt, 2, L0, n_new, actions, 2, out.view, None, None, t.view) == OK
        assert out.guards_intact() and out.filled() and t.guards_intact() and t.filled(), f"n_new = {n_new}"
        cols = t.view.view(2, n_new, 3)
        zero = (cols == 0).all(-1)
        assert zero.sum().item() == (2 if (actions is not None and n_new >= 17) else 0), "exactly the forced column is zero"
        want = head.generate(prompt, do_sample=False, max_new_tokens=n_new, action=table) if actions is not None else \
            head.llm.generate(prompt, do_sample=False, max_new_tokens=n_new)
        assert torch.equal(out.view.view(2, -1), want)
    # all three outputs NULL: the entry it stands for
    out = Guarded(2 * (L0 + 20), torch.int64, SENT_I)
    c0 = counter()
    assert raw_scored(eng, prompt, 2, L0, 20, table, 2, out.view, None, None, None) == OK
    assert counter() == c0 and torch.equal(out.view.view(2, -1), head.generate(prompt, do_sample=False, max_new_tokens=20, action=table))


# ------------------------------------------------------------------------------------------------ 8. MBRL
class Dealer:
    """Stands in for ``LlamaForCausalLM._uniforms``: deals consecutive columns of one table, so that ``rollout`` (17 per step) and
    ``rollout_actions`` (17 * horizon - 1 at once) draw the same numbers for the same new tokens."""

    def __init__(self, table):
        self.table, self.col = table, 0

    def __call__(self, B, n, do_sample, generator):
        u = self.table[:B, self.col:self.col + n].contiguous()
        self.col += n
        return u


def test_rollout_uncertainty(tmp_path):
    from helpers import world_model_files
    from mbrl.video_predictor import VideoPredictor
    args, *_ = world_model_files(tmp_path, False)
    args.update(encode_dtype="fp32", decode_dtype="fp32", llm_dtype="fp32")
    vp = VideoPredictor("cuda", args)
    g = torch.Generator().manual_seed(8)
    obs = torch.randint(0, 256, (2, 9, 64, 64), generator=g).float()
    acts = torch.randn(2, 3, 4, generator=g)
    table = torch.rand(4, 51, generator=g).to(DEV)
    llm = vp.model.llm
    llm._uniforms = Dealer(table)
    o1, a1, r1, u1 = vp.rollout(obs, lambda o, t: acts[:, t], 3, return_uncertainty=True)
    llm._uniforms = Dealer(table)
    o0, a0, r0 = vp.rollout(obs, lambda o, t: acts[:, t], 3)
    llm._uniforms = Dealer(table)
    o2, a2, r2, u2 = vp.rollout_actions(obs, acts, return_uncertainty=True)
    del llm._uniforms
    assert torch.equal(o1, o0) and torch.equal(r1, r0), "return_uncertainty changed the rollout"
    assert u1.shape == u2.shape == (2, 4, 1) and u1.dtype == torch.float32
    V = llm._cfg["vocab_size"]
    print(f"uncertainty {u1[:, 1:].min().item():.4f} .. {u1[:, 1:].max().item():.4f} nats (log V = {math.log(V):.4f}); "
          f"rollout_actions vs rollout {(u2 - u1).abs().max().item():.3e}")
    assert torch.equal(r2, r1) and torch.equal(u2, u1), "uncertainty differs between the open-loop and the step-wise rollout"
    assert (u1[:, 0] == 0).all() and (u1[:, 1:] > 0).all() and (u1[:, 1:] <= math.log(V)).all()
    o4, a4, r4, u4 = vp.rollout_actions(obs, torch.randn(4, 3, 4, generator=g), samples=2, uniforms=table[:, :50], return_uncertainty=True)
    assert u4.shape == (4, 4, 1) and (u4[:, 0] == 0).all() and (u4[:, 1:] > 0).all() and (u4[:, 1:] <= math.log(V)).all()
