"""Nucleus (top-p) sampling on the MI355X: the sampler kernel through ivg_op_sample_top_p and every generate entry against the fp64
restatement of include/ivg.h (tests/top_p_ref.py).  Runs on the MI355X only (-m gpu)."""
import ctypes as C

import pytest
import torch

from helpers import llama_fixture, oracle_llama
from top_p_ref import nucleus, sample

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def lib():
    from ivideogpt_amd import _lib
    return _lib.load()


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def op(l, logits, k, p, u, temperature=1.0):
    B, V = logits.shape
    lg = logits.to(DEV)
    out = torch.full((B,), -7, dtype=torch.int64, device=DEV)
    rc = l.ivg_op_sample_top_p(P(lg), B, V, k, temperature, p, P(u.to(DEV) if u is not None else None), P(out), stream())
    assert rc == 0
    return out.cpu()


def op_plain(l, logits, k, u):
    B, V = logits.shape
    lg = logits.to(DEV)
    out = torch.full((B,), -7, dtype=torch.int64, device=DEV)
    assert l.ivg_op_sample(P(lg), B, V, k, 1.0, P(u.to(DEV) if u is not None else None), P(out), stream()) == 0
    return out.cpu()


# (case, V, top_k, top_p): the op-test family of test_gpu_ops.py plus the nucleus's own edges.  top_k = V + 5 / None reach the
# full-vocabulary path (bisection), 1000 the list built after the radix select, the rest the pre-filtered list
CASES = [("normal", 8194, 100, 0.9), ("wide_vocab", 16386, 100, 0.9), ("k1000", 16386, 1000, 0.7), ("ties_at_threshold", 8194, 100, 0.8),
         ("all_equal", 8194, 100, 0.5), ("heavy_ties", 8194, 100, 0.9), ("topk_ge_vocab", 8194, 8199, 0.9), ("tiny_vocab", 70, 100, 0.6),
         ("p_zero", 8194, 100, 0.0), ("boundary_ties", 8194, 100, None), ("full_vocab", 16386, None, 0.9), ("full_vocab_p03", 8194, None, 0.3)]


def case_logits(case, V, k, B=64):
    g = torch.Generator().manual_seed(sum(map(ord, case)) + 17)
    logits = torch.randn(B, V, generator=g) * 3
    if case == "ties_at_threshold":          # 300 copies of the 100-th largest value
        kth = torch.topk(logits, k, dim=-1).values[:, -1:]
        logits.scatter_(1, torch.randint(0, V, (B, 300), generator=g), kth.expand(B, 300))
    if case == "all_equal":
        logits = torch.full((B, V), 1.25)
    if case == "heavy_ties":
        logits = torch.round(logits)
    top_p = None
    if case == "boundary_ties":
        # six copies of the 10-th largest value per row, and top_p chosen so the nucleus boundary falls inside that group:
        # the engine keeps all six (HF's sort would keep some)
        tenth = torch.topk(logits, 10, dim=-1).values[:, -1:]
        logits.scatter_(1, torch.randint(0, V, (B, 6), generator=g), tenth.expand(B, 6))
        kth = torch.topk(logits, k, dim=-1).values[:, -1:]
        e = torch.where(logits >= kth, torch.exp((logits - logits.max(-1, keepdim=True).values).double()), torch.zeros((), dtype=torch.double))
        below = torch.where(logits < tenth, e, torch.zeros((), dtype=torch.double)).sum(-1)
        grp = torch.where(logits == tenth, e, torch.zeros((), dtype=torch.double)).sum(-1)
        cut = (below + 0.5 * grp) / e.sum(-1)                 # row-wise, but the op takes one top_p: use row 0's and let the rows differ
        top_p = float(1.0 - cut[0])
    logits[1, 7] = float("-inf")
    u = torch.rand(B, generator=g)
    u[0], u[2] = 0.0, 0.99999994
    return logits, u, top_p


@pytest.mark.parametrize("case,V,k,p", CASES, ids=[c[0] for c in CASES])
def test_op_matches_restatement(case, V, k, p):
    l = lib()
    logits, u, p_case = case_logits(case, V, k)
    p = p_case if p is None else p
    kk = k if k is not None else V
    got = op(l, logits, kk, p, u)
    want, near = sample(logits, k, p, u)
    print(f"{case}: top_p={p:.6f}, {int(near.sum())} of {len(u)} rows near the boundary")
    assert near.sum() <= len(u) // 8
    bad = [b for b in range(len(u)) if not near[b] and got[b] != want[b]]
    assert not bad, f"rows {bad}: engine {got[bad].tolist()} vs restatement {want[bad].tolist()}"
    base = op_plain(l, logits, kk, u)
    if case == "all_equal":
        assert torch.equal(got, base), "every token ties: the nucleus keeps them all"
    else:
        assert not torch.equal(got, base), "the case must tell top_p apart from no filter"
    if case == "boundary_ties":
        # the ENGINE's survivors of row 0: one row per uniform of a fine sweep of [0, 1) draws every survivor whose share exceeds
        # the sweep step, so the set of drawn tokens is the engine's surviving set -- the whole tied group at the boundary included
        keep, e, _, tie = nucleus(logits[:1], k, p)
        vals, counts = logits[0].unique(return_counts=True)
        grp = logits[0] == vals[counts >= 6][-1]
        assert tie[0] and keep[0][grp].all(), "row 0: the restatement keeps the whole tied group"
        n = 8192
        share = e[0][keep[0]] / e[0][keep[0]].sum()
        assert share.min() > 4.0 / n, "the sweep must be fine enough to reach every survivor"
        sweep = (torch.arange(n, dtype=torch.float64) + 0.5) / n
        drawn = op(l, logits[:1].expand(n, -1).contiguous(), kk, p, sweep.float())
        assert set(drawn.tolist()) == set(keep[0].nonzero().flatten().tolist()), "engine survivors differ from the restatement"
    if case == "p_zero":
        assert torch.equal(got, logits.argmax(-1)), "top_p = 0: the maximum alone"
    # greedy is unaffected, and the same call twice draws the same tokens
    assert torch.equal(op(l, logits, kk, p, None), logits.argmax(-1))
    assert torch.equal(op(l, logits, kk, p, u), got)


@pytest.mark.parametrize("case,V,k,p", CASES, ids=[c[0] for c in CASES])
def test_op_top_p_one_is_the_plain_sampler(case, V, k, p):
    l = lib()
    logits, u, _ = case_logits(case, V, k)
    kk = k if k is not None else V
    assert torch.equal(op(l, logits, kk, 1.0, u), op_plain(l, logits, kk, u))
    assert torch.equal(op(l, logits, kk, 1.0, None), op_plain(l, logits, kk, None))


@pytest.mark.parametrize("k", [100, None])
def test_op_row_does_not_depend_on_batch(k):
    l = lib()
    logits, u, _ = case_logits("normal", 16386, 100)
    kk = k or 16386
    full = op(l, logits, kk, 0.8, u)
    for b0, n in ((0, 1), (5, 3), (17, 20)):
        assert torch.equal(op(l, logits[b0:b0 + n].contiguous(), kk, 0.8, u[b0:b0 + n].contiguous()), full[b0:b0 + n])


def test_op_rejects_invalid_top_p():
    l = lib()
    logits, u, _ = case_logits("normal", 8194, 100, B=4)
    out = torch.zeros(4, dtype=torch.int64, device=DEV)
    lg, ud = logits.to(DEV), u.to(DEV)
    for bad in (1.5, -0.1, float("nan")):
        assert l.ivg_op_sample_top_p(P(lg), 4, 8194, 100, 1.0, bad, P(ud), P(out), stream()) == -1


# ------------------------------------------------------------------------------------------------ generate
def check_rollout(seq, logits_of, u, top_k, top_p, L0, forced=None, what="rollout"):
    """Every sampled step j of seq (B, L0 + n) against the restatement over the teacher-forced logits of seq's own prefix
    (logits_of(ids) -> (B, L, V)).  A step may differ only where the nucleus boundary or the uniform is within what a logit error of
    ~1e-4 can move (near / CDF margin); those are counted.  Teacher forcing makes every step its own check: a differing step does
    not carry over to the next one.  Returns the number of such steps."""
    seq = seq.cpu()
    B, L = seq.shape
    lg = logits_of(seq[:, :-1]).float().cpu()[:, L0 - 1:]
    flagged = 0
    for j in range(L - L0):
        if forced is not None and (j + 1) % forced == 0:
            continue
        tok, near = sample(lg[:, j], top_k, top_p, u[:, j].cpu(), tol=1e-4)
        surv, e, _, _ = nucleus(lg[:, j], top_k, top_p)
        cdf = torch.cumsum(torch.where(surv, e, torch.zeros((), dtype=torch.double)), -1)
        margin = ((cdf - u[:, j].cpu().double().view(-1, 1) * cdf[:, -1:]).abs() / cdf[:, -1:]).min(-1).values
        for b in range(B):
            if tok[b] != seq[b, L0 + j]:
                assert near[b] or margin[b] < 1e-3, f"{what}: row {b}, new token {j + 1}: {int(seq[b, L0 + j])} vs restatement {int(tok[b])}"
                flagged += 1
    assert flagged <= max(1, B * (L - L0) // 50), f"{what}: {flagged} flagged steps"
    return flagged


PROFILES = pytest.mark.parametrize("lds_kb", [0, 40], ids=["one_batch", "batches_in_flight"])


def make_llm(cfg, sd, lds_kb=0):
    from ivideogpt_amd import LlamaForCausalLM
    return LlamaForCausalLM(cfg, sd, dtype="fp32", decode_lds_kb=lds_kb).to(DEV)


@PROFILES
@pytest.mark.parametrize("top_k,top_p", [(100, 0.8), (None, 0.9)])
def test_generate_matches_restatement(lds_kb, top_k, top_p):
    cfg, sd, g = llama_fixture("llama_tiny_ctx2_free.npz")
    m = make_llm(cfg, sd, lds_kb)
    ora = oracle_llama(cfg, sd)
    prompt = torch.from_numpy(g["prompt"])
    n_new = 50
    u = torch.rand(prompt.shape[0], n_new, generator=torch.Generator().manual_seed(11))
    out = m.generate(prompt.to(DEV), do_sample=True, top_k=top_k, top_p=top_p, max_new_tokens=n_new, uniforms=u.to(DEV)).cpu()
    n = check_rollout(out, ora.logits, u, top_k, top_p, prompt.shape[1], what=f"generate(top_k={top_k}, top_p={top_p})")
    print(f"lds_kb={lds_kb} top_k={top_k} top_p={top_p}: {n} flagged steps")
    plain = m.generate(prompt.to(DEV), do_sample=True, top_k=top_k, max_new_tokens=n_new, uniforms=u.to(DEV)).cpu()
    assert not torch.equal(out, plain), "top_p must change the samples"
    again = m.generate(prompt.to(DEV), do_sample=True, top_k=top_k, top_p=top_p, max_new_tokens=n_new, uniforms=u.to(DEV)).cpu()
    assert torch.equal(out, again)
    greedy = m.generate(prompt.to(DEV), do_sample=False, top_p=top_p, max_new_tokens=n_new).cpu()
    assert torch.equal(greedy, m.generate(prompt.to(DEV), do_sample=False, max_new_tokens=n_new).cpu()), "do_sample=False ignores top_p"


def test_shared_context_and_inputs_embeds_with_top_p():
    cfg, sd, g = llama_fixture("llama_tiny_ctx2_free.npz")
    m = make_llm(cfg, sd)
    ora = oracle_llama(cfg, sd)
    prompt = torch.from_numpy(g["prompt"])
    t, n_new, L0 = 3, 40, prompt.shape[1]
    rep = prompt.repeat(t, 1)
    u = torch.rand(rep.shape[0], n_new, generator=torch.Generator().manual_seed(13))
    kw = dict(do_sample=True, top_k=100, top_p=0.7, max_new_tokens=n_new, uniforms=u.to(DEV))
    plain = m.generate(rep.to(DEV), **kw).cpu()
    shared = m.generate(rep.to(DEV), shared_context=t, **kw).cpu()
    check_rollout(plain, ora.logits, u, 100, 0.7, L0, what="plain")
    check_rollout(shared, ora.logits, u, 100, 0.7, L0, what="shared_context")
    emb = m.get_input_embeddings()(rep.to(DEV))
    new = m.generate(inputs_embeds=emb, **kw).cpu()
    assert new.shape == (rep.shape[0], n_new)
    check_rollout(torch.cat([rep, new], 1), ora.logits, u, 100, 0.7, L0, what="inputs_embeds")
    assert not torch.equal(new, m.generate(inputs_embeds=emb, do_sample=True, top_k=100, max_new_tokens=n_new, uniforms=u.to(DEV)).cpu())


def test_action_paths_with_top_p():
    from ivideogpt_amd import HeadModelWithAction, LlamaForCausalLM
    cfg, sd, g = llama_fixture("llama_tiny_ctx2_act.npz")
    ctx, adim = int(g["ctx"]), int(g["action_dim"])
    prompt, action = torch.from_numpy(g["prompt"]), torch.from_numpy(g["action"])
    head = HeadModelWithAction(LlamaForCausalLM(cfg, None, dtype="fp32"), adim, 257 * ctx - 1, 16, ctx, action.shape[1])
    head.load_state_dict(sd, strict=True)
    head.to(DEV)
    n_new = 17 * 3 - 1
    t = 2
    rep, act = prompt.repeat(t, 1), action.repeat(t, 1, 1)
    u = torch.rand(rep.shape[0], n_new, generator=torch.Generator().manual_seed(17))
    kw = dict(do_sample=True, top_k=100, top_p=0.75, max_new_tokens=n_new, uniforms=u.to(DEV))
    out = head.generate(rep.to(DEV), action=act.to(DEV), **kw).cpu()
    V = cfg["vocab_size"]
    assert (out[:, 257 * ctx + 16::17] == V - 1).all(), "forced sdf slots"
    check_rollout(out, lambda ids: head.logits(ids.to(DEV), act.to(DEV)), u, 100, 0.75, rep.shape[1], forced=17, what="action generate")
    assert torch.equal(head.generate(rep.to(DEV), action=act.to(DEV), shared_context=t, **kw).cpu(), out), "shared_context == plain"
    assert not torch.equal(out, head.generate(rep.to(DEV), action=act.to(DEV), do_sample=True, top_k=100, max_new_tokens=n_new,
                                              uniforms=u.to(DEV)).cpu())
    free = head.generate_without_action(rep.to(DEV), **kw).cpu()
    assert not torch.equal(free, head.generate_without_action(rep.to(DEV), do_sample=True, top_k=100, max_new_tokens=n_new,
                                                              uniforms=u.to(DEV)).cpu())


def test_graph_replay_keys_on_top_p(switches):
    """IVG_GRAPH=1: one engine runs top_p 1.0 then 0.5 with everything else equal; the second call must not replay the first
    call's step graph (top_p is part of the key) and equals a fresh eager engine's tokens."""
    cfg, sd, g = llama_fixture("llama_tiny_ctx1_free.npz")
    prompt = torch.from_numpy(g["prompt"]).to(DEV)
    u = torch.rand(prompt.shape[0], 40, generator=torch.Generator().manual_seed(19)).to(DEV)
    kw = dict(do_sample=True, top_k=100, max_new_tokens=40, uniforms=u)
    eager = make_llm(cfg, sd).generate(prompt, top_p=0.5, **kw).cpu()
    switches(IVG_GRAPH="1")
    m = make_llm(cfg, sd)
    first = m.generate(prompt, top_p=1.0, **kw).cpu()
    second = m.generate(prompt, top_p=0.5, **kw).cpu()
    assert not torch.equal(first, second)
    assert torch.equal(second, eager)


def test_lanes_do_not_share_top_p():
    """replica() lanes own their engines: a top_p set through one does not reach the other."""
    cfg, sd, g = llama_fixture("llama_tiny_ctx2_free.npz")
    a = make_llm(cfg, sd)
    b = a.replica()
    prompt = torch.from_numpy(g["prompt"]).to(DEV)
    u = torch.rand(prompt.shape[0], 30, generator=torch.Generator().manual_seed(23)).to(DEV)
    kw = dict(do_sample=True, top_k=100, max_new_tokens=30, uniforms=u)
    ref_a, ref_b = make_llm(cfg, sd).generate(prompt, top_p=0.3, **kw).cpu(), make_llm(cfg, sd).generate(prompt, **kw).cpu()
    assert not torch.equal(ref_a, ref_b)
    out_a = a.generate(prompt, top_p=0.3, **kw).cpu()
    assert torch.equal(out_a, ref_a)
    b.generate(prompt, max_new_tokens=2, do_sample=False)      # lane b's engine exists
    # lane a's C engine is set to 0.3 through the C ABI; lane b's C engine then runs WITHOUT any set_top_p call of its own (the
    # engine-level entry, below the Python cache): only its own state, still 1.0, may decide
    assert lib().ivg_set_top_p(a._engine.h, 0.3) == 0
    out_b = torch.empty(prompt.shape[0], prompt.shape[1] + 30, dtype=torch.int64, device=DEV)
    b._engine.rollout(prompt.contiguous(), 30, out_b, uniforms=u, top_k=100)
    assert torch.equal(out_b.cpu(), ref_b), "lane a's top_p reached lane b's engine"
    # and the other way round: b at 0.3 through the C ABI, a's engine (left at 0.3 by its own call) back to 1.0 by the C ABI
    assert lib().ivg_set_top_p(b._engine.h, 0.3) == 0 and lib().ivg_set_top_p(a._engine.h, 1.0) == 0
    out_a2 = torch.empty_like(out_b)
    a._engine.rollout(prompt.contiguous(), 30, out_a2, uniforms=u, top_k=100)
    assert torch.equal(out_a2.cpu(), ref_b), "lane b's top_p reached lane a's engine"
    a._engine._top_p = 1.0
