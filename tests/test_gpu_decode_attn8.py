"""The FP8 (e4m3) K / V cache of bf16 rollouts (include/ivg.h ivg_set_kv_format) on the GPU: ivg_op_kv8_pack bit-exact against the store
rule, one decode-attention step of ivg_op_decode_attn8 against fp64 per output row, and the engine / model with the format on.

Reference, store rule and bound: tests/decode_attn8_ref.py; tests/test_decode_attn8_cpu.py shows on the CPU that the rule is torch's
float8_e4m3fn conversion after an explicit clamp and that the bound rejects each kernel mutant by >= 10x.

Every attention case checks, besides out within its bound row by row: unread cache bytes are NaN codes (rows [pos, Lmax) of every
cache row -- the first fetch round asks for rows [0, 512) before pos is known --, rows [0, P) of rows that are no group's slot, rows
[P, pos) of the row past the last trajectory); both caches keep their bytes except row pos of cache rows [0, B), where v is the store
rule of the fed v and k the store rule of ONE rotation form, bit for bit; out is not written past its end.
"""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

import decode_attn8_ref as R8
import decode_attn_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 512
SENTINEL = 1536.0
STEP = R8.STEP
B_OP, HEADS_OP, LMAX_OP = 3, 2, 2 * R8.STEP + 64


def lib():
    from ivideogpt_amd import _lib
    return _lib.load()


def ptr(t):
    return C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ------------------------------------------------------------------------------------------------ ivg_op_kv8_pack
_PACK = {}


def pack_input():
    """bf16 [2][6][96][64]: magnitudes from below e4m3's smallest subnormal (2^-9 at scale 1, 2^-11 at 2^-2) to beyond 448 * 2^3, exact
    +-448 * scale and the clamp edges, both zeros, every midpoint of two neighbouring e4m3 values, a few NaN."""
    if not _PACK:
        gen = torch.Generator().manual_seed(88)
        x = torch.randn(2, 6, 96, 64, generator=gen) * 10.0 ** (torch.rand(2, 6, 96, 64, generator=gen) * 8.0 - 4.5)
        flat = x.view(-1)
        pos = torch.from_numpy(R8.e4m3_decode(np.arange(0x7F, dtype=np.uint8)).astype(np.float32))
        special = torch.cat([(pos[:-1] + pos[1:]) / 2, pos, torch.tensor([447.9, 448.0, 460.0, 464.0, 470.0, 1e9, float("inf"), 0.0])])
        special = torch.cat([special, -special, special * 0.25, -special * 8.0, torch.tensor([float("nan")] * 4)])
        idx = torch.randperm(flat.numel(), generator=gen)[:4 * special.numel()]
        flat[idx] = special.repeat(4)
        _PACK["x"] = x.to(torch.bfloat16)
    return _PACK["x"]


@pytest.mark.parametrize("L", [1, 31, 32, 33, 96])
def test_kv8_pack_is_the_store_rule_bit_for_bit(L):
    """BH = 6, Lmax = 96: rows [0, L) of both caches equal e4m3_rne(clamp(x / scale, +-448)) byte for byte (a NaN's sign aside) at the
    scale pairs (1, 1), (2^-2, 2^3) and (2^3, 2^-2); rows >= L keep their poison; a finite input never stores a NaN code."""
    BH, Lmax = 6, 96
    x = pack_input()
    xd = x.to(DEV)
    for ks, vs in ((1.0, 1.0), (0.25, 8.0), (8.0, 0.25)):
        kc = torch.full((BH, Lmax, 64), 0xA5, dtype=torch.uint8, device=DEV)
        vc = torch.full((BH, Lmax, 64), 0x5A, dtype=torch.uint8, device=DEV)
        assert lib().ivg_op_kv8_pack(ptr(xd[0]), ptr(xd[1]), ptr(kc), ptr(vc), BH, L, Lmax, ks, vs, stream()) == 0
        torch.cuda.synchronize()
        for name, got, src, sc, poison in (("k", kc.cpu().numpy(), x[0], ks, 0xA5), ("v", vc.cpu().numpy(), x[1], vs, 0x5A)):
            want = R8.store8(src.float().numpy(), sc)
            diff = R8.canon(got[:, :L]) != R8.canon(want[:, :L])
            assert not diff.any(), (f"{name} scale {sc}: {int(diff.sum())} bytes differ from the store rule, first at {tuple(np.argwhere(diff)[0])}: "
                                    f"x = {float(src.float().numpy()[:, :L][diff][0])!r} -> {int(got[:, :L][diff][0]):#x}, rule {int(want[:, :L][diff][0]):#x}")
            assert (got[:, L:] == poison).all(), f"{name}: rows >= L were written"
            fin = np.isfinite(src.float().numpy()[:, :L])
            assert ((got[:, :L][fin] & 0x7F) != 0x7F).all(), f"{name}: a finite value became a NaN code"
            assert ((got[:, :L][~fin & np.isnan(src.float().numpy()[:, :L])] & 0x7F) == 0x7F).all(), f"{name}: NaN must store a NaN code"


# ------------------------------------------------------------------------------------------------ ivg_op_decode_attn8
def positions():
    return [0, 1, STEP - 1, STEP, STEP + 1, 2 * STEP - 1, 2 * STEP, LMAX_OP - 1]


def attn_cases():
    """(pos, P, G, row0, k_scale, v_scale, saturate): every pos plain (G = 1), and with P in {0, 1, step, pos} (those <= pos) under
    G in {2, 3} and row0 in {0, -1}, the pairs cycling so that every (G, row0) meets every kind of P and both sides of every round
    boundary; one case with scales != 1 and one whose inputs saturate."""
    out = []
    for i, pos in enumerate(positions()):
        out.append((pos, 0, 1, 0, 1.0, 1.0, False))
        for j, P in enumerate(sorted({p for p in (0, 1, STEP, pos) if p <= pos})):
            n = i + j
            out.append((pos, P, (2, 3)[n % 2], (0, -1)[(n // 2) % 2], 1.0, 1.0, False))
    out.append((STEP + 1, 0, 1, 0, 0.25, 8.0, False))
    out.append((2 * STEP, STEP, 3, -1, 4.0, 0.5, False))
    out.append((STEP + 1, 0, 1, 0, 1.0, 1.0, True))
    out.append((2 * STEP - 1, 1, 2, -1, 0.25, 8.0, True))
    return out


CASES = attn_cases()


def case_id(c):
    pos, P, G, row0, ks, vs, sat = c
    return f"pos{pos}" + (f"-P{P}-G{G}-r{row0}" if G > 1 else "") + (f"-ks{ks}-vs{vs}" if (ks, vs) != (1.0, 1.0) else "") + ("-sat" if sat else "")


def run_step(pos, P, G, row0, ks, vs, sat, family, seed):
    B, heads, Lmax = B_OP, HEADS_OP, LMAX_OP
    case = R8.make_case8(heads, B, Lmax, pos, P, G, row0, family=family, seed=seed, k_scale=ks, v_scale=vs, saturate=sat)
    kc0, vc0 = case["K8"], case["V8"]
    kd, vd = kc0.to(DEV), vc0.to(DEV)
    qkv = case["qkv"].to(DEV)
    out = torch.full((B * heads * 64 + GUARD,), SENTINEL, dtype=torch.bfloat16, device=DEV)
    cos, sin = case["cos"].to(DEV), case["sin"].to(DEV)
    rc = lib().ivg_op_decode_attn8(ptr(qkv), ptr(kd), ptr(vd), ptr(out), ptr(cos), ptr(sin), B, heads, Lmax, pos, P, G, row0, ks, vs, stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    kc1, vc1 = kd.cpu(), vd.cpu()
    assert (out[B * heads * 64:].cpu().float() == SENTINEL).all(), "out written past B * heads * 64"
    for name, before, after in (("kc", kc0, kc1), ("vc", vc0, vc1)):
        a = after.clone()
        a[:B, :, pos] = before[:B, :, pos]
        diff = a != before
        assert not diff.any(), f"{name}: {int(diff.sum())} bytes changed outside row pos of the trajectories' own cache rows"
    kgot, vgot = kc1[:B, :, pos].numpy(), vc1[:B, :, pos].numpy()
    q, k, v = R.split_qkv(case["qkv"], heads, 64)
    cand = {f: R8.store8(x, ks) for f, x in R.rope_candidates(k, case["cos"][pos].numpy(), case["sin"][pos].numpy(), "bf16").items()}
    forms = [f for f in R.ROPE_FORMS if np.array_equal(cand[f], kgot)]
    assert forms, "the appended k bytes equal the store rule of none of the rotation forms: " + ", ".join(
        f"{f}: {int((cand[f] != kgot).sum())} bytes differ" for f in R.ROPE_FORMS)
    assert np.array_equal(vgot, R8.store8(R.to_bf16(v), vs)), "the appended v bytes are not the store rule of the fed v"
    ref = R8.decode_ref8(case["qkv"], case["K8"], case["V8"], case["cos"], case["sin"], heads, pos, P, G, row0, ks, vs, form=forms[0])
    assert np.isfinite(ref["out"]).all(), "the reference read a poisoned byte (a mistake in the test's own case)"
    got = out[:B * heads * 64].cpu().double().view(B, heads, 64).numpy()
    assert np.isfinite(got).all(), f"{int((~np.isfinite(got)).any(-1).sum())} rows are not finite"
    ratio = np.abs(got - ref["out"]).max(-1) / ref["bound"]
    worst = np.unravel_index(int(ratio.argmax()), ratio.shape)
    msg = (f"{case_id((pos, P, G, row0, ks, vs, sat))} {family}: worst row (b, h) = {tuple(int(x) for x in worst)}: err / bound {ratio.max():.3f}; "
           f"{int((ratio > 1).sum())} of {ratio.size} rows beyond; k forms {forms}")
    print(msg)
    assert (ratio <= 1).all(), msg
    if sat:
        assert ((vgot[..., :8] & 0x7F) == 0x7E).all(), "the fed v beyond the range must store +-448"


@pytest.mark.parametrize("family", ["random", "needle"])
@pytest.mark.parametrize("pos,P,G,row0,ks,vs,sat", CASES, ids=[case_id(c) for c in CASES])
def test_decode_attention8_step_vs_fp64(pos, P, G, row0, ks, vs, sat, family):
    """B = 3, heads = 2, Lmax = 2 * 512 + 64 (module docstring: what a case checks)."""
    run_step(pos, P, G, row0, ks, vs, sat, family, seed=zlib.crc32(f"{family}-{case_id((pos, P, G, row0, ks, vs, sat))}".encode()) % 100003)


# ------------------------------------------------------------------------------------------------ engine and model
def tiny_cfg(heads=2, hidden=128):
    from ivideogpt_amd import weights as W
    return dict(W.LLAMA_SMALL, hidden_size=hidden, intermediate_size=256, num_hidden_layers=2, num_attention_heads=heads,
                num_key_value_heads=heads, vocab_size=1026)


def counter():
    return lib().ivg_debug_counter(b"decode_attn8")


def tiny_llm(lds_kb=0, kv="auto", seed=31):
    from ivideogpt_amd import LlamaForCausalLM, weights as W
    cfg = tiny_cfg()
    return LlamaForCausalLM(cfg, W.random_llama_state_dict(cfg, seed), dtype="bf16", decode_lds_kb=lds_kb, kv_cache_dtype=kv).to(DEV), cfg


@pytest.mark.parametrize("lds_kb", [0, 40], ids=["one_batch", "batches_in_flight"])
def test_rollouts_with_the_fp8_cache(lds_kb):
    """Seeded 2-layer model, hidden 128, 2 heads: (a) "auto" launches no decode_attn8 and gives the tokens of a model that was never
    told about the format, also after fp8 was on and off again; (b) fp8_e4m3 launches layers x (n_new - 1) of them; (c) rows of a
    26-row batch are token-identical to their 10- and 16-row shards, greedy and sampled; (d) the format changes some token (it is on)."""
    n_new, L0, layers = 40, 257, 2
    gen = torch.Generator().manual_seed(4)
    m, cfg = tiny_llm(lds_kb)
    prompt = torch.randint(0, 1024, (26, L0), generator=gen).to(DEV)
    u = torch.rand(26, n_new, generator=gen).to(DEV)
    c0 = counter()
    today_g = m.generate(prompt, do_sample=False, max_new_tokens=n_new).cpu()
    today_s = m.generate(prompt, do_sample=True, top_k=100, max_new_tokens=n_new, uniforms=u).cpu()
    assert counter() == c0, "an engine in the default format launched the FP8 attention"
    assert m.set_kv_cache_dtype("fp8_e4m3") is m
    g8 = m.generate(prompt, do_sample=False, max_new_tokens=n_new).cpu()
    assert counter() - c0 == layers * (n_new - 1), (counter() - c0, layers * (n_new - 1))
    s8 = m.generate(prompt, do_sample=True, top_k=100, max_new_tokens=n_new, uniforms=u).cpu()
    assert torch.equal(g8[:, :L0], prompt.cpu()) and ((g8 >= 0) & (g8 < cfg["vocab_size"])).all()
    for lo, hi in ((0, 10), (10, 26)):
        part = m.generate(prompt[lo:hi], do_sample=False, max_new_tokens=n_new).cpu()
        assert torch.equal(part, g8[lo:hi]), f"greedy rows [{lo}, {hi}) differ between the 26-row batch and the shard"
        part = m.generate(prompt[lo:hi], do_sample=True, top_k=100, max_new_tokens=n_new, uniforms=u[lo:hi]).cpu()
        assert torch.equal(part, s8[lo:hi]), f"sampled rows [{lo}, {hi}) differ between the 26-row batch and the shard"
    agree = (g8[:, L0:] == today_g[:, L0:]).float().mean().item()
    print(f"lds_kb {lds_kb}: greedy tokens equal to the bf16 cache's: {agree:.3f}; sampled: {(s8[:, L0:] == today_s[:, L0:]).float().mean().item():.3f}")
    c1 = counter()
    m.set_kv_cache_dtype("auto")
    assert torch.equal(m.generate(prompt, do_sample=False, max_new_tokens=n_new).cpu(), today_g)
    assert torch.equal(m.generate(prompt, do_sample=True, top_k=100, max_new_tokens=n_new, uniforms=u).cpu(), today_s)
    assert counter() == c1
    # a model built with the format on from the start, and its replica, run it too
    m2, _ = tiny_llm(lds_kb, kv="fp8_e4m3")
    assert torch.equal(m2.generate(prompt, do_sample=False, max_new_tokens=n_new).cpu(), g8)
    r = m2.replica()
    assert r._kv == m2._kv and torch.equal(r.generate(prompt[:10], do_sample=False, max_new_tokens=n_new).cpu(), g8[:10])
    assert counter() - c1 == layers * (n_new - 1) * 2


def test_scales_reach_the_kernels_and_the_step_graph_key(monkeypatch):
    """k_scale = 2^-3 / v_scale = 2^2 on a model whose K / V are O(1) use more of e4m3's range: the rollout runs the FP8 attention
    and stays close to scale 1's tokens; with IVG_GRAPH=1 a replayed step graph follows a change of format and of scales (the key holds
    them): tokens equal the eager engine's."""
    n_new, L0 = 40, 257
    prompt = torch.randint(0, 1024, (4, L0), generator=torch.Generator().manual_seed(6)).to(DEV)
    m, _ = tiny_llm(kv="fp8_e4m3")
    a = m.generate(prompt, do_sample=False, max_new_tokens=n_new).cpu()
    m.set_kv_cache_dtype("fp8_e4m3", k_scale=2.0 ** -3, v_scale=2.0 ** 2)
    b = m.generate(prompt, do_sample=False, max_new_tokens=n_new).cpu()
    m.set_kv_cache_dtype("auto")
    c = m.generate(prompt, do_sample=False, max_new_tokens=n_new).cpu()
    monkeypatch.setenv("IVG_GRAPH", "1")
    g, _ = tiny_llm()
    c0 = counter()
    assert torch.equal(g.generate(prompt, do_sample=False, max_new_tokens=n_new).cpu(), c)
    assert counter() == c0
    g.set_kv_cache_dtype("fp8_e4m3")
    assert torch.equal(g.generate(prompt, do_sample=False, max_new_tokens=n_new).cpu(), a)
    g.set_kv_cache_dtype("fp8_e4m3", k_scale=2.0 ** -3, v_scale=2.0 ** 2)
    assert torch.equal(g.generate(prompt, do_sample=False, max_new_tokens=n_new).cpu(), b)
    assert counter() > c0   # (host launch calls: a replayed graph launches without them)
    g.set_kv_cache_dtype("auto")
    assert torch.equal(g.generate(prompt, do_sample=False, max_new_tokens=n_new).cpu(), c)


def test_shared_context_rollout_over_the_fp8_cache():
    """t = 6 samples of 2 prompts through ivg_generate_shared with the format on: the prompt rows are stored once per group (as bytes)
    and read by the group's trajectories.  Agreement as tests/test_gpu_shared.py defines it for a bf16 engine (the prompt's last position
    goes through the decode-step kernels in the shared call, so a near-tie may flip against the plain call): rows of a group with the
    same uniforms are identical, rows with different uniforms differ, the prompt is copied, tokens are in range; greedy rows of a group
    are all equal.  The shared call launches layers x n_new FP8 attentions (one more step: it feeds the prompt's last token)."""
    t, n_new, L0 = 6, 30, 257
    gen = torch.Generator().manual_seed(12)
    m, cfg = tiny_llm(kv="fp8_e4m3")
    prompt = torch.randint(0, 1024, (2, L0), generator=gen)
    rep = prompt.repeat(t, 1).to(DEV)
    u = torch.rand(2 * t, n_new, generator=gen)
    u[6], u[7] = u[2], u[3]                                  # samples 1 and 3 of both prompts share their uniforms
    c0 = counter()
    shared = m.generate(rep, do_sample=True, top_k=100, max_new_tokens=n_new, uniforms=u.to(DEV), shared_context=t).cpu()
    assert counter() - c0 == 2 * n_new
    plain = m.generate(rep, do_sample=True, top_k=100, max_new_tokens=n_new, uniforms=u.to(DEV)).cpu()
    for out in (shared, plain):
        assert torch.equal(out[2], out[6]) and torch.equal(out[3], out[7]), "rows of a group with the same uniforms must be identical"
        assert (out[0] != out[2]).any() and torch.equal(out[:, :L0], rep.cpu()) and ((out >= 0) & (out < cfg["vocab_size"])).all()
    print(f"shared vs plain over the FP8 cache: {(shared[:, L0:] == plain[:, L0:]).float().mean().item():.3f} of the sampled tokens equal")
    g = m.generate(rep, do_sample=False, max_new_tokens=n_new, shared_context="auto").cpu()
    for k in range(1, t):
        assert torch.equal(g[2 * k:2 * k + 2], g[:2]), "greedy samples of one prompt differ"


def test_kept_cache_and_format_changes():
    """HeadModelWithAction, step-wise: after a generate with the FP8 cache, generate(reuse_cache=True) continues over the kept bytes and
    equals the one-shot rollout token for token (greedy: the same kernels on the same bytes); a change of format -- or of a scale --
    invalidates the kept cache: the continue call is refused (IVG_ERR_INVALID -> AssertionError), never run over bytes of the other
    format; generate_embeds does not reuse across a change either."""
    from ivideogpt_amd import HeadModelWithAction, LlamaForCausalLM, weights as W
    cfg = tiny_cfg()
    lsd = W.random_llama_state_dict(cfg, 83, action_dim=4, reward_prediction=True)
    head = HeadModelWithAction(LlamaForCausalLM(cfg, None, dtype="bf16", kv_cache_dtype="fp8_e4m3"), 4, 513, 16, 2, 16, reward_prediction=True)
    head.load_state_dict(lsd, strict=True)
    head.to(DEV)
    gen = torch.Generator().manual_seed(9)
    B = 5
    prompt = torch.randint(0, 1024, (B, 514), generator=gen)
    prompt[:, -1] = 1025
    prompt = prompt.to(DEV)
    act = torch.randn(B, 6, 4, generator=gen).to(DEV)
    c0 = counter()
    whole = head.generate(prompt, do_sample=False, max_new_tokens=34, action=act).cpu()
    assert counter() - c0 == 2 * 33
    first = head.generate(prompt, do_sample=False, max_new_tokens=17, action=act)
    assert torch.equal(first.cpu(), whole[:, :531])
    cont = head.generate(first, do_sample=False, max_new_tokens=17, action=act, reuse_cache=True).cpu()
    assert torch.equal(cont, whole), f"{(cont != whole).sum().item()} tokens differ between the continued and the one-shot rollout"
    for change in (lambda: head.set_kv_cache_dtype("auto"), lambda: head.set_kv_cache_dtype("fp8_e4m3"),
                   lambda: head.set_kv_cache_dtype("fp8_e4m3", k_scale=0.5)):
        first = head.generate(prompt, do_sample=False, max_new_tokens=17, action=act)
        change()
        with pytest.raises(AssertionError, match="libivg error -1"):
            head.generate(first, do_sample=False, max_new_tokens=17, action=act, reuse_cache=True)
    # embeds path: the reuse is verified, and a format change in between means a prefill
    llm = head.llm
    head.set_kv_cache_dtype("fp8_e4m3")
    emb = llm.get_input_embeddings()(prompt)
    new = llm.generate(inputs_embeds=emb, do_sample=False, max_new_tokens=17)
    assert llm.last_generate_reused_cache is False
    grown = torch.cat([emb, llm.get_input_embeddings()(new)], 1)
    llm.generate(inputs_embeds=grown, do_sample=False, max_new_tokens=17)
    assert llm.last_generate_reused_cache is True
    llm.generate(inputs_embeds=emb, do_sample=False, max_new_tokens=17)
    head.set_kv_cache_dtype("fp8_e4m3", v_scale=2.0)
    llm.generate(inputs_embeds=grown, do_sample=False, max_new_tokens=17)
    assert llm.last_generate_reused_cache is False, "a kept cache of another format / scale was reused"


@pytest.mark.parametrize("dtype,heads,hidden", [("fp32", 2, 128), ("x3", 2, 128), ("bf16", 4, 128), ("bf16", 1, 128)],
                         ids=["fp32", "x3", "bf16-hd32", "bf16-hd128"])
def test_engines_the_format_is_not_for_refuse(dtype, heads, hidden):
    """ivg_set_kv_format(IVG_KV_FP8_E4M3) on an fp32 or x3 engine, or at head_dim != 64: IVG_ERR_INVALID with a message, the engine keeps
    its format (its next rollout launches no FP8 attention and equals the one before); IVG_KV_NATIVE is accepted everywhere; an
    unknown format or a scale that is no power of two is refused on an engine the format is for."""
    from ivideogpt_amd import LlamaForCausalLM, _lib, weights as W
    cfg = tiny_cfg(heads, hidden)
    m = LlamaForCausalLM(cfg, W.random_llama_state_dict(cfg, 5), dtype=dtype).to(DEV)
    prompt = torch.randint(0, 1024, (2, 257), generator=torch.Generator().manual_seed(1)).to(DEV)
    before = m.generate(prompt, do_sample=False, max_new_tokens=8).cpu()
    eng = m._ensure(2)
    c0 = counter()
    with pytest.raises(AssertionError, match="llm_dtype IVG_BF16 and head_dim 64"):
        eng.set_kv_format(_lib.IVG_KV_FP8_E4M3, 1.0, 1.0)
    eng.set_kv_format(_lib.IVG_KV_NATIVE, 1.0, 1.0)
    assert torch.equal(m.generate(prompt, do_sample=False, max_new_tokens=8).cpu(), before) and counter() == c0
    ok, _ = tiny_llm()
    e2 = ok._ensure(2)
    for fmt, ks, vs in ((2, 1.0, 1.0), (-1, 1.0, 1.0), (1, 3.0, 1.0), (1, 1.0, 0.0), (0, float("nan"), 1.0), (1, 1.0, float("inf"))):
        with pytest.raises(AssertionError, match="libivg error -1"):
            e2.set_kv_format(fmt, ks, vs)
