"""Per-layer, per-head scales of the FP8 K / V cache and their calibration on the device (include/ivg.h ivg_set_kv_scales, ivg_kv_calibrate,
ivg_kv_calibration_finish), on the GPU.

G1  kv_absmax_kernel through ivg_op_kv_absmax: bit-exact against torch, rows >= L never read, Inf / NaN come back, accumulation.
G2  ivg_op_kv8_pack_heads bit for bit against the store rule with each head's scale; one step of ivg_op_decode_attn8_heads against the
    fp64 reference of tests/decode_attn8_ref.py run once per head's scale pair (its bound carries over: only powers of two changed).
G3  the engine: calibrate_kv_cache returns exactly the rule of tests/kv_scales_ref.py applied to the observed maxima, layer 0 agrees
    with the oracle's K / V; the table reaches the rollout, is dropped by uniform scales, invalidates the kept cache, and is followed by
    a replayed step graph.
G4  invariance, exact: a twin of the model whose heads are rescaled by powers of two gives the same tokens over the FP8 cache once both
    are calibrated -- and does not with uniform scales.  Exponents used: q 2^-10 / k 2^10 on head 0, v 2^-12 / o 2^12 on head 1.
G5  refusals.
"""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

import decode_attn8_ref as R8
import decode_attn_ref as R
import kv_scales_ref as KS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 512
SENTINEL = 1536.0
STEP = R8.STEP
B_OP, HEADS_OP, LMAX_OP = 3, 2, 2 * R8.STEP + 64
K_SCALES, V_SCALES = (2.0 ** -3, 2.0 ** 5), (2.0 ** 2, 2.0 ** -7)


def lib():
    from ivideogpt_amd import _lib
    return _lib.load()


def ptr(t):
    return C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def dev_f32(xs):
    return torch.tensor(xs, dtype=torch.float32, device=DEV)


# ------------------------------------------------------------------------------------------------ G1: ivg_op_kv_absmax
def pattern_max(x, L, B, heads):
    """bf16 [B * heads][Lmax][64] -> per head the maximum over rows [0, L) of the integer pattern of |x|, widened to the fp32 pattern."""
    bits = (x.view(torch.int16).to(torch.int32) & 0x7FFF).view(B, heads, x.shape[1], 64)[:, :, :L]
    return (bits.permute(1, 0, 2, 3).reshape(heads, -1).max(1).values << 16).to(torch.int64)


def absmax_call(k, v, L, out, B=3, heads=2, Lmax=96):
    assert lib().ivg_op_kv_absmax(ptr(k), ptr(v), B, heads, L, Lmax, ptr(out), stream()) == 0
    torch.cuda.synchronize()
    return out.cpu().to(torch.int64) & 0xFFFFFFFF


@pytest.mark.parametrize("L", [1, 31, 32, 33, 96])
def test_kv_absmax_is_exact(L):
    """B = 3, heads = 2, Lmax = 96, rows >= L filled with NaN: out [2][heads] equals x[:, :, :L].abs().amax() bit for bit with the maximum
    planted at (row 0, element 0), (row L - 1, element 63), in the last trajectory, and as a negative value; an Inf and a NaN planted
    inside [0, L) come back as their patterns; a second call with smaller data leaves the table, a zeroed table follows the new data."""
    B, heads, Lmax = 3, 2, 96
    gen = torch.Generator().manual_seed(100 + L)
    base = (torch.randn(2, B * heads, Lmax, 64, generator=gen) * 3.0).to(torch.bfloat16)
    base[:, :, L:] = float("nan")
    plants = [(0, 0, 0, 0, 1000.0), (0, 1, L - 1, 63, 1000.0), (B - 1, 1, L // 2, 17, 1000.0), (1, 0, L - 1, 5, -1000.0),
              (B - 1, heads - 1, L - 1, 63, float("inf")), (0, 1, 0, 31, float("nan"))]
    for b, h, row, el, val in plants:
        for which in (0, 1):
            x = base.clone()
            x[which, b * heads + h, row, el] = val
            xd = x.to(DEV)
            out = torch.zeros(2, heads, dtype=torch.int32, device=DEV)
            got = absmax_call(xd[0], xd[1], L, out)
            want = torch.stack([pattern_max(x[0], L, B, heads), pattern_max(x[1], L, B, heads)])
            assert torch.equal(got, want), f"plant {(b, h, row, el, val)} in {'kv'[which]}: got {got.tolist()}, want {want.tolist()}"
            if np.isfinite(val):   # the pattern maximum IS the value maximum
                ref = x.float().view(2, B, heads, Lmax, 64)[:, :, :, :L].abs().amax((1, 3, 4))
                assert torch.equal(got.to(torch.int32).view(torch.float32), ref) and ref[which, h] == 1000.0
            elif np.isinf(val):
                assert int(got[which, h]) == 0x7F800000
            else:
                assert int(got[which, h]) > 0x7F800000, "a NaN must rank above everything"
    # accumulation: smaller data changes nothing; a zeroed table follows the new data
    x = base.clone()
    xd = x.to(DEV)
    out = torch.zeros(2, heads, dtype=torch.int32, device=DEV)
    first = absmax_call(xd[0], xd[1], L, out)
    small = (x.float() * 0.5).to(torch.bfloat16)
    sd = small.to(DEV)
    assert torch.equal(absmax_call(sd[0], sd[1], L, out), first), "a call with smaller data changed the table"
    out.zero_()
    want = torch.stack([pattern_max(small[0], L, B, heads), pattern_max(small[1], L, B, heads)])
    assert torch.equal(absmax_call(sd[0], sd[1], L, out), want) and (want < first).all()


# ------------------------------------------------------------------------------------------------ G2: per-head pack and step
def pack_input():
    """bf16 [2][6][96][64] as tests/test_gpu_decode_attn8.py builds it: magnitudes across and beyond the format's range at every scale
    used, the clamp edges, both zeros, every midpoint of two neighbouring e4m3 values, a few NaN."""
    gen = torch.Generator().manual_seed(88)
    x = torch.randn(2, 6, 96, 64, generator=gen) * 10.0 ** (torch.rand(2, 6, 96, 64, generator=gen) * 8.0 - 4.5)
    flat = x.view(-1)
    pos = torch.from_numpy(R8.e4m3_decode(np.arange(0x7F, dtype=np.uint8)).astype(np.float32))
    special = torch.cat([(pos[:-1] + pos[1:]) / 2, pos, torch.tensor([447.9, 448.0, 460.0, 464.0, 470.0, 1e9, float("inf"), 0.0])])
    special = torch.cat([special, -special, special * 2.0 ** -3, -special * 2.0 ** 5, special * 4.0, special * 2.0 ** -7, torch.tensor([float("nan")] * 4)])
    idx = torch.randperm(flat.numel(), generator=gen)[:4 * special.numel()]
    flat[idx] = special.repeat(4)
    return x.to(torch.bfloat16)


@pytest.mark.parametrize("L", [1, 33, 96])
def test_kv8_pack_heads_is_the_store_rule_per_head(L):
    """B * heads = 6 (head = row % 2), Lmax = 96, k_scales (2^-3, 2^5), v_scales (2^2, 2^-7): rows [0, L) equal the store rule with the
    row's head's scale byte for byte (a NaN's sign aside); rows >= L keep their poison."""
    B, heads, Lmax = 3, 2, 96
    x = pack_input()
    xd = x.to(DEV)
    kc = torch.full((B * heads, Lmax, 64), 0xA5, dtype=torch.uint8, device=DEV)
    vc = torch.full((B * heads, Lmax, 64), 0x5A, dtype=torch.uint8, device=DEV)
    ks, vs = dev_f32(K_SCALES), dev_f32(V_SCALES)
    assert lib().ivg_op_kv8_pack_heads(ptr(xd[0]), ptr(xd[1]), ptr(kc), ptr(vc), B, heads, L, Lmax, ptr(ks), ptr(vs), stream()) == 0
    torch.cuda.synchronize()
    for name, got, src, scales, poison in (("k", kc.cpu().numpy(), x[0], K_SCALES, 0xA5), ("v", vc.cpu().numpy(), x[1], V_SCALES, 0x5A)):
        for bh in range(B * heads):
            want = R8.store8(src[bh].float().numpy(), scales[bh % heads])
            diff = R8.canon(got[bh, :L]) != R8.canon(want[:L])
            assert not diff.any(), f"{name} row {bh} (scale {scales[bh % heads]}): {int(diff.sum())} bytes differ from the store rule"
        assert (got[:, L:] == poison).all(), f"{name}: rows >= L were written"
    bad = dev_f32((1.0, 3.0))
    assert lib().ivg_op_kv8_pack_heads(ptr(xd[0]), ptr(xd[1]), ptr(kc), ptr(vc), B, heads, L, Lmax, ptr(bad), ptr(vs), stream()) == -1


STEP_CASES = [(0, 0, 1, 0), (STEP - 1, 0, 1, 0), (STEP, 0, 1, 0), (LMAX_OP - 1, 0, 1, 0), (2 * STEP, STEP, 3, -1)]


def per_head_case(pos, P, G, row0, family, seed):
    """make_case8 once per head's scale pair (same seed: the same K / V values), the caches assembled from each head's own bytes."""
    cases = [R8.make_case8(HEADS_OP, B_OP, LMAX_OP, pos, P, G, row0, family=family, seed=seed, k_scale=K_SCALES[h], v_scale=V_SCALES[h])
             for h in range(HEADS_OP)]
    assert all(torch.equal(c["qkv"], cases[0]["qkv"]) for c in cases)
    K8 = torch.stack([cases[h]["K8"][:, h] for h in range(HEADS_OP)], 1).contiguous()
    V8 = torch.stack([cases[h]["V8"][:, h] for h in range(HEADS_OP)], 1).contiguous()
    return cases, K8, V8


def launch_heads(case, K8, V8, pos, P, G, row0, ks, vs):
    kd, vd = K8.to(DEV), V8.to(DEV)
    qkv, cos, sin = case["qkv"].to(DEV), case["cos"].to(DEV), case["sin"].to(DEV)
    out = torch.full((B_OP * HEADS_OP * 64 + GUARD,), SENTINEL, dtype=torch.bfloat16, device=DEV)
    ksd, vsd = dev_f32(ks), dev_f32(vs)
    rc = lib().ivg_op_decode_attn8_heads(ptr(qkv), ptr(kd), ptr(vd), ptr(out), ptr(cos), ptr(sin), B_OP, HEADS_OP, LMAX_OP, pos, P, G, row0,
                                         ptr(ksd), ptr(vsd), stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    return out.cpu(), kd.cpu(), vd.cpu()


@pytest.mark.parametrize("family", ["random", "needle"])
@pytest.mark.parametrize("pos,P,G,row0", STEP_CASES, ids=[f"pos{c[0]}" + (f"-P{c[1]}-G{c[2]}-r{c[3]}" if c[2] > 1 else "") for c in STEP_CASES])
def test_decode_attention8_step_with_per_head_scales(pos, P, G, row0, family):
    """B = 3, heads = 2, Lmax = 2 * 512 + 64, k_scales (2^-3, 2^5), v_scales (2^2, 2^-7): per head, out lies within the bound of
    decode_ref8 run with that head's scale pair; the appended codes equal its k_new / v_new; no other byte of the caches changes (the
    unread ones stay NaN codes); out is not written past its end.  With both heads given one scale pair the launch is bit-identical
    to ivg_op_decode_attn8 with those scalars."""
    B, heads = B_OP, HEADS_OP
    seed = zlib.crc32(f"heads-{family}-{pos}-{P}-{G}-{row0}".encode()) % 100003
    cases, K8, V8 = per_head_case(pos, P, G, row0, family, seed)
    out, kc1, vc1 = launch_heads(cases[0], K8, V8, pos, P, G, row0, K_SCALES, V_SCALES)
    assert (out[B * heads * 64:].float() == SENTINEL).all(), "out written past B * heads * 64"
    for name, before, after in (("kc", K8, kc1), ("vc", V8, vc1)):
        a = after.clone()
        a[:B, :, pos] = before[:B, :, pos]
        assert torch.equal(a, before), f"{name}: bytes changed outside row pos of the trajectories' own cache rows"
    got = out[:B * heads * 64].double().view(B, heads, 64).numpy()
    assert np.isfinite(got).all()
    q, k, v = R.split_qkv(cases[0]["qkv"], heads, 64)
    for h in range(heads):
        ks, vs, case = K_SCALES[h], V_SCALES[h], cases[h]
        kgot, vgot = kc1[:B, h, pos].numpy(), vc1[:B, h, pos].numpy()
        cand = {f: R8.store8(x, ks)[:, h] for f, x in R.rope_candidates(k, case["cos"][pos].numpy(), case["sin"][pos].numpy(), "bf16").items()}
        forms = [f for f in R.ROPE_FORMS if np.array_equal(cand[f], kgot)]
        assert forms, f"head {h}: the appended k bytes equal the store rule of none of the rotation forms"
        ref = R8.decode_ref8(case["qkv"], case["K8"], case["V8"], case["cos"], case["sin"], heads, pos, P, G, row0, ks, vs, form=forms[0])
        assert np.array_equal(kgot, ref["k_new"][:, h]) and np.array_equal(vgot, ref["v_new"][:, h]), f"head {h}: appended codes differ from k_new / v_new"
        assert np.isfinite(ref["out"][:, h]).all(), "the reference read a poisoned byte (a mistake in the test's own case)"
        ratio = np.abs(got[:, h] - ref["out"][:, h]).max(-1) / ref["bound"][:, h]
        msg = f"pos {pos} P {P} G {G} {family} head {h} (ks {ks}, vs {vs}): worst err / bound {ratio.max():.3f}; k forms {forms}"
        print(msg)
        assert (ratio <= 1).all(), msg
    # one scale pair for both heads: the table path equals the scalar path bit for bit
    ks, vs = 0.25, 8.0
    case = R8.make_case8(heads, B, LMAX_OP, pos, P, G, row0, family=family, seed=seed, k_scale=ks, v_scale=vs)
    o_t, k_t, v_t = launch_heads(case, case["K8"], case["V8"], pos, P, G, row0, (ks, ks), (vs, vs))
    kd, vd = case["K8"].to(DEV), case["V8"].to(DEV)
    qkv, cos, sin = case["qkv"].to(DEV), case["cos"].to(DEV), case["sin"].to(DEV)
    o_s = torch.full((B * heads * 64 + GUARD,), SENTINEL, dtype=torch.bfloat16, device=DEV)
    assert lib().ivg_op_decode_attn8(ptr(qkv), ptr(kd), ptr(vd), ptr(o_s), ptr(cos), ptr(sin), B, heads, LMAX_OP, pos, P, G, row0, ks, vs, stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(o_t.view(torch.int16), o_s.cpu().view(torch.int16)) and torch.equal(k_t, kd.cpu()) and torch.equal(v_t, vd.cpu()), \
        "equal per-head scales must be bit-identical to the scalar launch"


# ------------------------------------------------------------------------------------------------ engine and model
LAYERS, HEADS, N_NEW, L0 = 2, 2, 40, 257


def tiny_cfg(heads=2, hidden=128):
    from ivideogpt_amd import weights as W
    return dict(W.LLAMA_SMALL, hidden_size=hidden, intermediate_size=256, num_hidden_layers=LAYERS, num_attention_heads=heads,
                num_key_value_heads=heads, vocab_size=1026)


def counter():
    return lib().ivg_debug_counter(b"decode_attn8")


def tiny_sd(seed=31):
    from ivideogpt_amd import weights as W
    return W.random_llama_state_dict(tiny_cfg(), seed)


def tiny_llm(lds_kb=0, kv="auto", sd=None):
    from ivideogpt_amd import LlamaForCausalLM
    cfg = tiny_cfg()
    return LlamaForCausalLM(cfg, sd if sd is not None else tiny_sd(), dtype="bf16", decode_lds_kb=lds_kb, kv_cache_dtype=kv).to(DEV)


def prompts(n, seed):
    return torch.randint(0, 1024, (n, L0), generator=torch.Generator().manual_seed(seed)).to(DEV)


def threshold_close(amax):
    """True where a bf16 amax lies within one bf16 ulp of a threshold of the rule (0.875 * 2^k)"""
    m, e = np.frexp(amax.astype(np.float64))
    return np.abs(m - 0.875) <= 2.0 ** -8 + 1e-12       # (one bf16 ulp of a value in [0.5, 1) is 2^-8)


def test_calibration_returns_the_rule_of_the_observed_maxima():
    """4 prompts of 257 tokens on the seeded 2-layer model: the scales calibrate_kv_cache returns equal scale_from_amax(amax, 1) of the
    maxima the engine reports, exactly; they are positive finite; for layer 0 they equal the scales of the oracle's K / V (bf16 weights,
    fp32 arithmetic, rounded to bf16), or lie one power of two apart on at most the entries whose amax is within one bf16 ulp of a rule
    threshold.  A second call with reset=False over a subset changes nothing; headroom shifts every scale by that power of two."""
    from oracle.llama import LlamaRef
    m = tiny_llm()
    p = prompts(4, 6)
    scales = m.calibrate_kv_cache(p)
    amax = m.last_kv_amax
    assert tuple(scales.shape) == (LAYERS, 2, HEADS) and scales.dtype == torch.float32 and scales.device.type == "cpu"
    assert torch.isfinite(amax).all() and (amax > 0).all()
    assert np.array_equal(scales.numpy(), KS.scale_from_amax(amax.numpy(), 1)), (scales, amax)
    assert torch.equal(m.kv_scales, scales) and m._kv[0] == "auto", "calibration must not switch the format on"
    assert torch.equal(m.calibrate_kv_cache(p[:2], reset=False), scales) and torch.equal(m.last_kv_amax, amax)
    assert torch.equal(m.calibrate_kv_cache(p, headroom=0), scales / 2) and torch.equal(m.calibrate_kv_cache(p, headroom=3), scales * 4)
    sd16 = {k: v.to(torch.bfloat16).float() for k, v in tiny_sd().items()}
    ref = LlamaRef(sd16, 1, HEADS, max_pos=L0)
    _, past = ref.forward_embeds(ref.embed(p.cpu()))
    o_amax = np.stack([t.to(torch.bfloat16).float().abs().amax((0, 2, 3)).numpy() for t in past[0]])     # [k|v][head]
    o_scales = KS.scale_from_amax(o_amax, 1)
    got = scales[0].numpy()
    differ = got != o_scales
    ratio = np.maximum(got / o_scales, o_scales / got)
    allowed = threshold_close(o_amax) | threshold_close(amax[0].numpy())
    msg = (f"layer 0: engine amax {amax[0].tolist()}, oracle amax {o_amax.tolist()}; scales {got.tolist()} vs {o_scales.tolist()}; entries "
           f"that differ {np.argwhere(differ).tolist()}, of which near a threshold {np.argwhere(differ & allowed).tolist()}")
    print(msg)
    assert (ratio[differ] == 2.0).all() and not (differ & ~allowed).any(), msg


def test_the_table_reaches_the_rollout_and_uniform_scales_drop_it():
    """with the format on, after calibration: the rollout launches layers x (n_new - 1) FP8 attentions, the engine reports the table,
    a rebuilt engine and a replica carry it (token-identical rollouts), tokens differ from scale 1's somewhere or equal them (printed),
    set_kv_cache_dtype("fp8_e4m3") with default scalars drops the table (the engine reports ones and gives scale 1's tokens again)."""
    p = prompts(4, 6)
    m = tiny_llm(kv="fp8_e4m3")
    ones = m.generate(p, do_sample=False, max_new_tokens=N_NEW).cpu()
    scales = m.calibrate_kv_cache(p)
    c0 = counter()
    tab = m.generate(p, do_sample=False, max_new_tokens=N_NEW).cpu()
    assert counter() - c0 == LAYERS * (N_NEW - 1)
    eng = m._ensure(4)
    assert torch.equal(eng.get_kv_scales(), scales) and torch.equal(m.kv_scales, scales)
    r = m.replica()
    assert r._kv == m._kv and torch.equal(r.generate(p, do_sample=False, max_new_tokens=N_NEW).cpu(), tab)
    assert torch.equal(r._ensure(4).get_kv_scales(), scales)
    big = m.generate(prompts(6, 7), do_sample=False, max_new_tokens=4)     # (a larger batch: the engine is rebuilt, the table with it)
    assert m._engine is not eng and torch.equal(m._engine.get_kv_scales(), scales) and big.shape == (6, L0 + 4)
    assert torch.equal(m.generate(p, do_sample=False, max_new_tokens=N_NEW).cpu(), tab)
    print(f"greedy tokens equal between calibrated and unit scales: {(tab[:, L0:] == ones[:, L0:]).float().mean().item():.3f}")
    m.set_kv_cache_dtype("fp8_e4m3")
    assert torch.equal(m._engine.get_kv_scales(), torch.ones(LAYERS, 2, HEADS)) and torch.equal(m.kv_scales, torch.ones(LAYERS, 2, HEADS))
    assert torch.equal(m.generate(p, do_sample=False, max_new_tokens=N_NEW).cpu(), ones)
    m.set_kv_cache_dtype("fp8_e4m3", scales=scales)
    assert torch.equal(m.generate(p, do_sample=False, max_new_tokens=N_NEW).cpu(), tab)


def test_set_kv_scales_invalidates_the_kept_cache():
    """HeadModelWithAction, step-wise: generate(reuse_cache=True) continues over the kept bytes with a table in force and equals the
    one-shot rollout; ivg_set_kv_scales in between -- also with the very same table -- and a calibration pass invalidate the kept
    cache: the continue call is refused.  The wrapper's calibrate_kv_cache passes its actions and context."""
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
    scales = head.calibrate_kv_cache(prompt, action=act)
    assert torch.equal(head.kv_scales, scales) and np.array_equal(scales.numpy(), KS.scale_from_amax(head.llm.last_kv_amax.numpy(), 1))
    no_act = head.llm.calibrate_kv_cache(prompt)
    print(f"amax with / without the action embeddings equal: {torch.equal(no_act, scales)}")
    head.calibrate_kv_cache(prompt, action=act)
    whole = head.generate(prompt, do_sample=False, max_new_tokens=34, action=act).cpu()
    first = head.generate(prompt, do_sample=False, max_new_tokens=17, action=act)
    cont = head.generate(first, do_sample=False, max_new_tokens=17, action=act, reuse_cache=True).cpu()
    assert torch.equal(cont, whole), f"{(cont != whole).sum().item()} tokens differ between the continued and the one-shot rollout"
    eng = head.llm._engine
    for change in (lambda: eng.set_kv_scales(scales), lambda: eng.set_kv_scales(scales * 2), lambda: eng.kv_calibrate(prompt, actions=act, ctx=2)):
        eng.set_kv_scales(scales)
        first = head.generate(prompt, do_sample=False, max_new_tokens=17, action=act)
        change()
        with pytest.raises(AssertionError, match="libivg error -1"):
            head.generate(first, do_sample=False, max_new_tokens=17, action=act, reuse_cache=True)


def test_a_replayed_step_graph_follows_table_scalars_table(monkeypatch):
    """IVG_GRAPH=1: table -> uniform scalars -> another table -> the first table again; the graph engine's tokens equal the eager
    engine's each time (the step-graph key holds a counter every setter bumps)."""
    p = prompts(4, 6)
    m = tiny_llm(kv="fp8_e4m3")
    t1 = m.calibrate_kv_cache(p)
    t2 = t1.clone()
    t2[:, 0, 0] *= 4.0
    t2[:, 1, 1] /= 4.0
    settings = [dict(scales=t1), dict(k_scale=2.0 ** -3, v_scale=2.0 ** 2), dict(scales=t2), dict(scales=t1)]
    eager = []
    for s in settings:
        m.set_kv_cache_dtype("fp8_e4m3", **s)
        eager.append(m.generate(p, do_sample=False, max_new_tokens=N_NEW).cpu())
    assert torch.equal(eager[0], eager[3])
    monkeypatch.setenv("IVG_GRAPH", "1")
    g = tiny_llm(kv="fp8_e4m3")
    for s, want in zip(settings, eager):
        g.set_kv_cache_dtype("fp8_e4m3", **s)
        got = g.generate(p, do_sample=False, max_new_tokens=N_NEW).cpu()
        assert torch.equal(got, want), f"graph engine under {list(s)}: {(got != want).sum().item()} tokens differ from the eager engine's"


# ------------------------------------------------------------------------------------------------ G4: invariance
Q_EXP, K_EXP, V_EXP, O_EXP = -10, 10, -12, 12


def rescaled_twin(sd):
    """q_proj rows of head 0 x 2^-10, k_proj rows of head 0 x 2^10, v_proj rows of head 1 x 2^-12, o_proj columns of head 1 x 2^12, in
    every layer: powers of two, so no product, sum or rounding differs (bf16 / fp32 have the exponent range to spare)."""
    tw = {k: v.clone() for k, v in sd.items()}
    for l in range(LAYERS):
        pre = f"model.layers.{l}.self_attn."
        tw[pre + "q_proj.weight"][0:64] *= 2.0 ** Q_EXP
        tw[pre + "k_proj.weight"][0:64] *= 2.0 ** K_EXP
        tw[pre + "v_proj.weight"][64:128] *= 2.0 ** V_EXP
        tw[pre + "o_proj.weight"][:, 64:128] *= 2.0 ** O_EXP
    return tw


@pytest.mark.parametrize("lds_kb", [0, 40], ids=["one_batch", "batches_in_flight"])
def test_calibrated_fp8_cache_is_invariant_under_per_head_rescaling(lds_kb):
    """The seeded model and its rescaled twin, 26 rows, 40 new tokens, greedy and sampled.  (a) bf16 cache: the same tokens (checks the
    construction).  (b) calibrated on the same prompts, the twin's scales are the original's times the planted factors.  (c) FP8 cache
    with the calibrated tables: the same tokens, exactly.  (d) FP8 cache with uniform scale 1: the twin differs from (c) in some token
    (its head-0 keys sit near 2^10 and are clamped, its head-1 values are stored as zero)."""
    gen = torch.Generator().manual_seed(4)
    p = torch.randint(0, 1024, (26, L0), generator=gen).to(DEV)
    u = torch.rand(26, N_NEW, generator=gen).to(DEV)
    sd = tiny_sd()
    orig, twin = tiny_llm(lds_kb, sd=sd), tiny_llm(lds_kb, sd=rescaled_twin(sd))

    def rollouts(m):
        return (m.generate(p, do_sample=False, max_new_tokens=N_NEW).cpu(),
                m.generate(p, do_sample=True, top_k=100, max_new_tokens=N_NEW, uniforms=u).cpu())

    for a, b, what in zip(rollouts(orig), rollouts(twin), ("greedy", "sampled")):
        assert torch.equal(a, b), f"(a) bf16 cache, {what}: {(a != b).sum().item()} tokens differ: the construction is not exact"
    orig.set_kv_cache_dtype("fp8_e4m3")
    twin.set_kv_cache_dtype("fp8_e4m3")
    twin_ones = rollouts(twin)
    so, st = orig.calibrate_kv_cache(p), twin.calibrate_kv_cache(p)
    factor = torch.ones(LAYERS, 2, HEADS)
    factor[:, 0, 0], factor[:, 1, 1] = 2.0 ** K_EXP, 2.0 ** V_EXP
    assert torch.equal(st, so * factor), f"(b) twin scales {st.tolist()} are not the original's {so.tolist()} times the planted factors"
    c0 = counter()
    ro, rt = rollouts(orig), rollouts(twin)
    assert counter() - c0 == 4 * LAYERS * (N_NEW - 1)
    for a, b, what in zip(ro, rt, ("greedy", "sampled")):
        assert torch.equal(a, b), f"(c) FP8 cache, calibrated, {what}: {(a != b).sum().item()} of {a.numel()} tokens differ"
    assert any((a != b).any() for a, b in zip(twin_ones, rt)), "(d) uniform scale 1 gave the twin the calibrated tokens: the planted scales do not bite"


# ------------------------------------------------------------------------------------------------ G5: refusals
@pytest.mark.parametrize("dtype,heads", [("fp32", 2), ("x3", 2), ("bf16", 4), ("bf16", 1)], ids=["fp32", "x3", "bf16-hd32", "bf16-hd128"])
def test_engines_the_format_is_not_for_refuse_scales_and_calibration(dtype, heads):
    """ivg_set_kv_scales / ivg_kv_calibrate / _reset / _finish on an fp32 or x3 engine, or at head_dim != 64: IVG_ERR_INVALID with a
    message; the engine keeps its state (uniform ones reported, the next rollout equals the one before, no FP8 attention launched)."""
    from ivideogpt_amd import LlamaForCausalLM, weights as W
    cfg = tiny_cfg(heads)
    m = LlamaForCausalLM(cfg, W.random_llama_state_dict(cfg, 5), dtype=dtype).to(DEV)
    p = torch.randint(0, 1024, (2, L0), generator=torch.Generator().manual_seed(1)).to(DEV)
    before = m.generate(p, do_sample=False, max_new_tokens=8).cpu()
    eng = m._ensure(2)
    c0 = counter()
    for call in (lambda: eng.set_kv_scales(torch.ones(LAYERS, 2, heads)), lambda: eng.kv_calibrate(p), lambda: eng.kv_calibrate(p, reset=True),
                 lambda: eng.kv_calibration_finish(1)):
        with pytest.raises(AssertionError, match="llm_dtype IVG_BF16 and head_dim 64"):
            call()
    assert torch.equal(eng.get_kv_scales(), torch.ones(LAYERS, 2, heads))
    assert torch.equal(m.generate(p, do_sample=False, max_new_tokens=8).cpu(), before) and counter() == c0


def test_bad_tables_headroom_and_non_finite_data_are_refused():
    """a table with a 3.0, a 0, a negative or a NaN entry is refused whole (the table in force stays); headroom outside [0, 8] is refused;
    after a pass over data whose embedding row is Inf, finish names the layer, installs nothing, and the model keeps its setting."""
    from ivideogpt_amd import LlamaForCausalLM
    m = tiny_llm(kv="fp8_e4m3")
    p = prompts(4, 6)
    scales = m.calibrate_kv_cache(p)
    eng = m._engine
    for entry in (3.0, 0.0, -2.0, float("nan")):
        t = scales.clone()
        t[1, 1, 0] = entry
        with pytest.raises(AssertionError, match="layer 1, v, head 0.*power of two"):
            eng.set_kv_scales(t)
        assert torch.equal(eng.get_kv_scales(), scales)
    for h in (-1, 9):
        with pytest.raises(AssertionError, match="headroom_log2"):
            eng.kv_calibration_finish(h)
    with pytest.raises(ValueError, match="shape"):
        eng.set_kv_scales(torch.ones(LAYERS, 2, HEADS + 1))
    assert torch.equal(eng.get_kv_scales(), scales)
    sd = tiny_sd()
    sd["model.embed_tokens.weight"] = sd["model.embed_tokens.weight"].clone()
    sd["model.embed_tokens.weight"][1024] = float("inf")
    bad = LlamaForCausalLM(tiny_cfg(), sd, dtype="bf16", kv_cache_dtype="fp8_e4m3").to(DEV)
    q = p.clone()
    q[1, 100] = 1024
    good = bad.calibrate_kv_cache(p)                   # (token 1024 does not occur in p: a table is installed)
    assert (p != 1024).all()
    with pytest.raises(AssertionError, match=r"layer 0, [kv], head \d saw (NaN|Inf)"):
        bad.calibrate_kv_cache(q)
    assert torch.equal(bad._engine.get_kv_scales(), good) and torch.equal(bad.kv_scales, good), "a refused finish installed something"
    assert torch.equal(bad.calibrate_kv_cache(p), good), "reset must clear the non-finite observation"
