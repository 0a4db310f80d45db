"""One decode-attention step at op level against fp64, per output row, at every instance of decode_attn_kernel and decode_attn24_kernel
(ivg_op_shared_decode_attn with G = 1, P = 0: the plain step the engine launches; G > 1: SHARED; ivg_op_decode_attn24), and the model
at head dims and cache lengths no fixture has.

Reference and bound: tests/decode_attn_ref.py (module docstring: the rotation forms, the per-row bound and its derivation);
tests/test_decode_attn_cpu.py shows on the CPU that the bound rejects each kernel mutant by >= 10x.

Every case checks, besides out within its bound row by row:
  - poison: every cache element the step must not read is NaN (0xFF bytes on the 24-bit planes) -- rows [pos, Lmax) of every cache
    row, rows [0, P) of rows that are no group's slot, rows [P, pos) of rows >= B (one whole cache row past the last trajectory);
    the first round of key rows is fetched with limit = Lmax before pos is known, so this is what makes "rows >= pos are never used"
    (llama_ops.hip, load_rows) a tested statement;
  - writes: both caches keep their bits except row pos of cache rows [0, B), where v is bit-exact and k equals one rotation form bit
    for bit (the same form for every element); guard elements past out's B * heads * hd still hold their sentinel.
"""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

import decode_attn_ref as R
from helpers import assert_sampled_rollout_matches, oracle_llama

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INSTANCES = [("bf16", hd) for hd in (8, 16, 32, 64, 128, 256)] + [("fp32", hd) for hd in (4, 8, 16, 32, 64, 128, 256)] + [("kv24", 64)]
GUARD = 512
SENTINEL = 1536.0          # exact in bf16 and fp32


def positions(step, Lmax):
    p = [0, 1, step - 1, step, step + 1, 2 * step - 1, 2 * step, 2 * step + 1, 3 * step, Lmax - 1]
    return sorted({x for x in p if 0 <= x < Lmax})


def plain_cases():
    out = []
    for kind, hd in INSTANCES:
        _, _, step = R.geometry(kind, hd)
        B = 40 if hd == 64 else 5
        for Lmax in (1024, 777):
            for i, pos in enumerate(positions(step, Lmax)):
                out.append((kind, hd, (12, 16, 1)[i % 3], B, Lmax, pos, 0, 1, 0))
    out.append(("bf16", 64, 12, 40, 2048, 2047, 0, 1, 0))
    return out


def shared_cases():
    out = []
    for kind, hd in [("bf16", 64), ("fp32", 64), ("kv24", 64), ("bf16", 256), ("fp32", 16), ("fp32", 128)]:
        _, _, step = R.geometry(kind, hd)
        heads = 12 if hd <= 64 else 3
        P = min(step + 1, 600)
        out.append((kind, hd, heads, 37, 1024, P + 44, P, 16, -5))                  # row0 < 0, ragged last group
        out.append((kind, hd, heads, 7, 1024, step, step, 3, 0))                    # pos == P
        for P in (step - 1, step, step + 1):                                        # P at a round edge
            out.append((kind, hd, heads, 9, 1024, P + 70, P, 4, -2))
        out.append((kind, hd, heads, 40 if hd == 64 else 6, 1024, 700, 513, 40 if hd == 64 else 6, 0))   # G = B
    return out


CASES = plain_cases() + shared_cases()


def case_id(c):
    kind, hd, heads, B, Lmax, pos, P, G, row0 = c
    return f"{kind}-hd{hd}-h{heads}-B{B}-L{Lmax}-pos{pos}" + (f"-P{P}-G{G}-r{row0}" if G > 1 else "")


def launch(kind, qkv, kc, vc, out, cos, sin, B, heads, hd, Lmax, pos, P, G, row0):
    from ivideogpt_amd import _lib
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    lib = _lib.load()
    if kind == "kv24":
        rc = lib.ivg_op_decode_attn24(p(qkv), p(kc), p(vc), p(out), p(cos), p(sin), B, heads, Lmax, pos, P, G, row0, st)
    else:
        rc = lib.ivg_op_shared_decode_attn(p(qkv), p(kc), p(vc), p(out), p(cos), p(sin), B, heads, hd, Lmax, pos, P, G, row0,
                                           1 if kind == "bf16" else 0, st)
    torch.cuda.synchronize()
    return rc


def bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else (t.view(torch.int32) if t.dtype == torch.float32 else t)


def run_step(kind, hd, heads, B, Lmax, pos, P, G, row0, family, seed):
    """one checked step -> (worst err / bound, the rotation forms the appended k matches)."""
    case = R.make_case(kind, hd, heads, B, Lmax, pos, P, G, row0, family=family, seed=seed)
    tdt = torch.bfloat16 if kind == "bf16" else torch.float32
    if kind == "kv24":
        kc0, vc0 = R.kv24_planes(case["K"]), R.kv24_planes(case["V"])
    else:
        kc0, vc0 = case["K"].to(tdt), case["V"].to(tdt)
    kd, vd = kc0.to(DEV), vc0.to(DEV)
    qkv = case["qkv"].to(DEV)
    out = torch.full((B * heads * hd + GUARD,), SENTINEL, dtype=tdt, device=DEV)
    rc = launch(kind, qkv, kd, vd, out, case["cos"].to(DEV), case["sin"].to(DEV), B, heads, hd, Lmax, pos, P, G, row0)
    assert rc == 0, rc
    kc1, vc1 = kd.cpu(), vd.cpu()
    assert torch.equal(bits(out[B * heads * hd:].cpu()), bits(torch.full((GUARD,), SENTINEL, dtype=tdt))), "out written past B * heads * hd"
    # writes: everything but row pos of cache rows [0, B) keeps its bits
    for name, before, after in (("kc", kc0, kc1), ("vc", vc0, vc1)):
        a = after.clone()
        if kind == "kv24":
            for lo, n in ((pos * hd * 2, hd * 2), (Lmax * hd * 2 + pos * hd, hd)):
                a[:B, :, lo:lo + n] = before[:B, :, lo:lo + n]
        else:
            a[:B, :, pos] = before[:B, :, pos]
        diff = bits(a) != bits(before)
        assert not diff.any(), f"{name}: {int(diff.sum())} elements changed outside row pos of the trajectories' own cache rows"
    kgot = (R.kv24_values(kc1, Lmax) if kind == "kv24" else kc1.float())[:B, :, pos].numpy()
    vgot = (R.kv24_values(vc1, Lmax) if kind == "kv24" else vc1.float())[:B, :, pos].numpy()
    q, k, v = R.split_qkv(case["qkv"], heads, hd)
    cand = R.rope_candidates(k, case["cos"][pos].numpy(), case["sin"][pos].numpy(), kind)
    forms = [f for f in R.ROPE_FORMS if np.array_equal(cand[f].view(np.uint32), kgot.view(np.uint32))]
    assert forms, "the appended k equals none of the rotation forms bit for bit: " + ", ".join(
        f"{f}: {int((cand[f].view(np.uint32) != kgot.view(np.uint32)).sum())} elements differ" for f in R.ROPE_FORMS)
    assert np.array_equal(vgot.view(np.uint32), R.store_round(v, kind).view(np.uint32)), "the appended v is not the fed v bit for bit"
    ref = R.decode_ref(case["qkv"], case["K"], case["V"], case["cos"], case["sin"], kind, heads, hd, pos, P, G, row0, form=forms[0])
    got = out[:B * heads * hd].cpu().double().view(B, heads, hd).numpy()
    assert np.isfinite(got).all(), f"{int((~np.isfinite(got)).any(-1).sum())} rows are not finite"
    ratio = np.abs(got - ref["out"]).max(-1) / ref["bound"]
    worst = np.unravel_index(int(ratio.argmax()), ratio.shape)
    msg = (f"{case_id((kind, hd, heads, B, Lmax, pos, P, G, row0))} {family}: worst row (b, h) = {tuple(int(x) for x in worst)}"
           + (f" (needle at key {int(case['needles'][worst])})" if case["needles"] is not None else "")
           + f": err / bound {ratio.max():.3f}; {int((ratio > 1).sum())} of {ratio.size} rows beyond; k forms {forms}")
    print(msg)
    assert (ratio <= 1).all(), msg
    return float(ratio.max()), forms


@pytest.mark.parametrize("family", ["random", "needle"])
@pytest.mark.parametrize("kind,hd,heads,B,Lmax,pos,P,G,row0", CASES, ids=[case_id(c) for c in CASES])
def test_decode_attention_step_vs_fp64(kind, hd, heads, B, Lmax, pos, P, G, row0, family):
    """one decode step (module docstring): out per row within the bound of decode_attn_ref, poison never read, caches written only at
    row pos of the trajectories' rows (k in one rotation form, v bit-exact), out not written past its end."""
    run_step(kind, hd, heads, B, Lmax, pos, P, G, row0, family,
             seed=zlib.crc32(f"{family}-{case_id((kind, hd, heads, B, Lmax, pos, P, G, row0))}".encode()) % 100003)


@pytest.mark.parametrize("kind,hd", [("bf16", 24), ("bf16", 48), ("bf16", 512), ("fp32", 12), ("fp32", 2)])
def test_decode_hook_refuses_uncovered_head_dims_untouched(kind, hd):
    """a head dim decode_attn_kernel has no instance for: IVG_ERR_INVALID, and out / both caches keep their bits."""
    B, heads, Lmax, pos = 2, 2, 16, 3
    tdt = torch.bfloat16 if kind == "bf16" else torch.float32
    gen = torch.Generator().manual_seed(hd)
    kc = torch.randn(B, heads, Lmax, hd, generator=gen).to(tdt).to(DEV)
    vc = torch.randn(B, heads, Lmax, hd, generator=gen).to(tdt).to(DEV)
    qkv = torch.randn(B, 3 * heads * hd, generator=gen).to(tdt).to(DEV)
    out = torch.full((B * heads * hd,), SENTINEL, dtype=tdt, device=DEV)
    cos = torch.ones(Lmax, hd // 2, device=DEV)
    k0, v0, o0 = kc.clone(), vc.clone(), out.clone()
    assert launch(kind, qkv, kc, vc, out, cos, cos, B, heads, hd, Lmax, pos, 0, 1, 0) == -1
    assert torch.equal(bits(kc), bits(k0)) and torch.equal(bits(vc), bits(v0)) and torch.equal(bits(out), bits(o0))


# ------------------------------------------------------------------------------------------------ the model at other shapes
def tiny_cfg(heads):
    from ivideogpt_amd import weights as W
    return dict(W.LLAMA_SMALL, hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=heads,
                num_key_value_heads=heads)


@pytest.mark.parametrize("heads", [1, 4], ids=["hd128", "hd32"])
def test_fp32_rollouts_at_other_head_dims_match_oracle(heads):
    """hidden 128 with 1 head (hd 128: DPP-only reduction, generic instance) and 4 heads (hd 32): greedy rollout token-identical to
    the oracle; sampled rollout equal up to near-ties of the inverse CDF (tests/helpers.py)."""
    from ivideogpt_amd import LlamaForCausalLM, weights as W
    from oracle.llama import generate_cached
    cfg = tiny_cfg(heads)
    sd = W.random_llama_state_dict(cfg, 60 + heads)
    m = LlamaForCausalLM(cfg, sd, dtype="fp32").to(DEV)
    ora = oracle_llama(cfg, sd)
    gen = torch.Generator().manual_seed(heads)
    prompt = torch.randint(0, cfg["vocab_size"], (3, 257), generator=gen)
    n_new = 48
    out = m.generate(prompt.to(DEV), do_sample=False, max_new_tokens=n_new).cpu()
    assert torch.equal(out, generate_cached(ora, prompt, n_new)), "greedy rollout differs from the oracle"
    u = torch.rand(3, n_new, generator=gen)
    out = m.generate(prompt.to(DEV), do_sample=True, top_k=100, max_new_tokens=n_new, uniforms=u.to(DEV)).cpu()
    ref = generate_cached(ora, prompt, n_new, top_k=100, uniforms=u)
    assert_sampled_rollout_matches(out, ref, ora, u, 100, prompt.shape[1], what=f"sampled rollout at hd {128 // heads}")


@pytest.mark.parametrize("heads", [1, 4], ids=["hd128", "hd32"])
def test_bf16_at_other_head_dims_close_to_oracle(heads):
    """bf16 engine at hd 128 / 32, held to test_llama_bf16_mode_close's bar (engine deviation from the fp32 oracle <= 1.5x that of
    the same model in plain bf16 PyTorch, or 5e-2, and < 0.25): prompt-pass logits, and every greedy decode step -- the token the
    engine picked has an oracle logit within that bar of the oracle's best, teacher-forced on the engine's own rollout."""
    from ivideogpt_amd import LlamaForCausalLM, weights as W
    cfg = tiny_cfg(heads)
    sd = W.random_llama_state_dict(cfg, 70 + heads)
    m = LlamaForCausalLM(cfg, sd, dtype="bf16").to(DEV)
    ora = oracle_llama(cfg, sd)
    ids = torch.randint(0, cfg["vocab_size"], (2, 300), generator=torch.Generator().manual_seed(heads))
    ref = ora.logits(ids)
    lg = m.logits(ids.to(DEV)).cpu().float()
    e = (lg - ref).abs().max().item()
    ora16 = oracle_llama(cfg, {k: v.to(torch.bfloat16) for k, v in sd.items()})
    ora16.cos, ora16.sin = ora16.cos.to(torch.bfloat16), ora16.sin.to(torch.bfloat16)
    e16 = (ora16.logits(ids).float() - ref).abs().max().item()
    bar = min(max(1.5 * e16, 5e-2), 0.25)
    print(f"hd {128 // heads} bf16 logits: engine max abs err {e:.3e}; torch-bf16 {e16:.3e}; bar {bar:.3e}")
    assert e < bar, (e, e16)
    L0, n_new = 257, 48
    out = m.generate(ids[:, :L0].to(DEV), do_sample=False, max_new_tokens=n_new).cpu()
    lr = ora.logits(out)[:, L0 - 1:-1].double()                        # oracle logits before each new token
    picked = lr.gather(-1, out[:, L0:, None])[..., 0]
    gap = (lr.max(-1).values - picked).max().item()
    print(f"hd {128 // heads} bf16 decode: largest oracle-logit gap of a picked token {gap:.3e}")
    assert gap < bar, f"a greedy bf16 decode step picked a token {gap:.3e} below the oracle's best"


def test_rollout_to_the_last_slot_of_a_shorter_cache():
    """max_seq = 777 < max_position_embeddings (a cache length that is not a multiple of 64): the rollout fills the cache to its last
    slot token-identical to the oracle; one more token is IVG_ERR_CAPACITY."""
    from ivideogpt_amd import LlamaForCausalLM, weights as W
    from oracle.llama import generate_cached
    cfg = tiny_cfg(2)
    sd = W.random_llama_state_dict(cfg, 77)
    m = LlamaForCausalLM(cfg, sd, dtype="fp32", max_seq=777).to(DEV)
    prompt = torch.randint(0, cfg["vocab_size"], (2, 257), generator=torch.Generator().manual_seed(7))
    out = m.generate(prompt.to(DEV), do_sample=False, max_new_tokens=777 - 257).cpu()
    assert out.shape == (2, 777)
    assert torch.equal(out[:1], generate_cached(oracle_llama(cfg, sd), prompt[:1], 777 - 257))
    with pytest.raises(RuntimeError, match="libivg error -4"):
        m.generate(prompt.to(DEV), do_sample=False, max_new_tokens=777 - 257 + 1)


@pytest.mark.parametrize("what,dtype,hidden,heads,max_seq,match", [
    ("hidden % heads", "bf16", 130, 4, 0, "multiple of num_heads"),
    ("bf16 hd 48", "bf16", 96, 2, 0, "head_dim 48"),
    ("bf16 hd 512", "bf16", 1024, 2, 0, "head_dim 512"),
    ("bf16 hd 4", "bf16", 128, 32, 0, "head_dim 4"),
    ("fp32 hd 12", "fp32", 48, 4, 0, "head_dim 12"),
    ("max_seq > max_position_embeddings", "fp32", 128, 2, 1025, "max_seq 1025"),
])
def test_engine_refuses_unusable_transformer_configs(what, dtype, hidden, heads, max_seq, match):
    """ivg_create refuses, with IVG_ERR_INVALID and a message, before anything is built or launched (no weights are given: the
    shape checks come first)."""
    from ivideogpt_amd.engine import Engine
    cfg = dict(tiny_cfg(heads), hidden_size=hidden)
    with pytest.raises(AssertionError, match=match):
        Engine(DEV, {}, llm_cfg=cfg, llm_dtype=dtype, max_seq=max_seq)
