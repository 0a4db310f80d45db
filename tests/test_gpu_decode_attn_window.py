"""The rolling-window body of the bf16 head_dim-64 decode attention (llama_ops.hip, decode_attn_kernel WINDOW: one buffer of eight row
chunks, chunk u of the next round requested into the registers chunk u was just consumed from) against the two-buffer body it replaces
(IVG_DECODE_ATTN_WINDOW=0 under IVG_DEV=1), through ivg_op_shared_decode_attn on the same inputs.

The window changes register allocation and load scheduling only: per key the same instructions, per lane group the value rows in the
same order.  So `out` and both caches after the step are compared BIT FOR BIT between the two bodies, and against the caches before
the step everywhere but row `pos` of the trajectories' own cache rows (the appended rows; their neighbours keep their bits).  Positions:
both sides of the 256-row round, an odd and an even number of rounds, an empty cache, the last slot; a cache shorter than one round;
SHARED with the prefix ending inside, at and behind a round.  One case per family also goes through the fp64 reference, bound and
poison / write checks of tests/test_gpu_decode_attn.py (run_step), with the window body (the default) launched.
"""
import pytest
import torch

import decode_attn_ref as R
from test_gpu_decode_attn import DEV, GUARD, SENTINEL, bits, launch, run_step

pytestmark = pytest.mark.gpu
B, HEADS, HD = 2, 3, 64

PLAIN = [(1024, pos, 0, 1, 0) for pos in (0, 1, 255, 256, 257, 511, 512, 513, 1022, 1023)] + [(64, pos, 0, 1, 0) for pos in (0, 63)]
SHARED = [(1024, pos, P, 2, 0) for pos in (300, 513) for P in (0, 255, 256, 300)]


def case_id(c):
    Lmax, pos, P, G, row0 = c
    return f"L{Lmax}-pos{pos}" + (f"-P{P}-G{G}" if G > 1 else "")


def one_step(case, Lmax, pos, P, G, row0):
    kd, vd = case["K"].to(torch.bfloat16).to(DEV), case["V"].to(torch.bfloat16).to(DEV)
    out = torch.full((B * HEADS * HD + GUARD,), SENTINEL, dtype=torch.bfloat16, device=DEV)
    rc = launch("bf16", case["qkv"].to(DEV), kd, vd, out, case["cos"].to(DEV), case["sin"].to(DEV), B, HEADS, HD, Lmax, pos, P, G, row0)
    assert rc == 0, rc
    return bits(out.cpu()), bits(kd.cpu()), bits(vd.cpu())


@pytest.mark.parametrize("Lmax,pos,P,G,row0", PLAIN + SHARED, ids=[case_id(c) for c in PLAIN + SHARED])
def test_window_body_bit_identical_to_two_buffer_body(switches, Lmax, pos, P, G, row0):
    case = R.make_case("bf16", HD, HEADS, B, Lmax, pos, P, G, row0, family="random", seed=1000 * G + pos + P)
    k0, v0 = bits(case["K"].to(torch.bfloat16)), bits(case["V"].to(torch.bfloat16))
    switches(IVG_DECODE_ATTN_WINDOW=None)                 # the default: the window body
    o_new, k_new, v_new = one_step(case, Lmax, pos, P, G, row0)
    switches(IVG_DECODE_ATTN_WINDOW="0")
    o_old, k_old, v_old = one_step(case, Lmax, pos, P, G, row0)
    assert torch.equal(o_new[B * HEADS * HD:], bits(torch.full((GUARD,), SENTINEL, dtype=torch.bfloat16))), "out written past its end"
    assert torch.isfinite(o_new[:B * HEADS * HD].view(torch.bfloat16).float()).all(), "out is not finite (a poisoned row was used)"
    nd = int((o_new != o_old).sum())
    assert nd == 0, f"out: {nd} of {B * HEADS * HD} elements differ between the two bodies"
    for name, new, old, before in (("kc", k_new, k_old, k0), ("vc", v_new, v_old, v0)):
        assert torch.equal(new[:B, :, pos], old[:B, :, pos]), f"{name}: the appended rows differ between the two bodies"
        assert (new[:B, :, pos] != before[:B, :, pos]).any(), f"{name}: row pos was not written"
        rest = new.clone()
        rest[:B, :, pos] = before[:B, :, pos]
        nd = int((rest != before).sum())
        assert nd == 0, f"{name}: {nd} elements changed outside row pos of the trajectories' cache rows"


@pytest.mark.parametrize("Lmax,pos,P,G,row0", [(1024, 513, 0, 1, 0), (64, 63, 0, 1, 0), (1024, 513, 256, 2, 0)],
                         ids=["plain", "short_cache", "shared"])
@pytest.mark.parametrize("family", ["random", "needle"])
def test_window_body_vs_fp64(Lmax, pos, P, G, row0, family):
    """the default body at the reference, bound, poison and write checks of test_gpu_decode_attn.run_step."""
    run_step("bf16", HD, HEADS, B, Lmax, pos, P, G, row0, family, seed=77 + pos + P)


@pytest.mark.parametrize("lds_kb", [0, 40], ids=["one_batch", "batches_in_flight"])
def test_sampled_continuation_identical_under_both_bodies(switches, lds_kb):
    """the tiny bf16 Llama, 24 sampled tokens with given uniforms behind a 514-token prompt (two full rounds of key rows and a
    partial one at every step), under both launch profiles: the same tokens with the window body and the two-buffer body."""
    from helpers import llama_fixture
    from ivideogpt_amd import LlamaForCausalLM
    cfg, sd, g = llama_fixture("llama_tiny_ctx2_free.npz")
    m = LlamaForCausalLM(cfg, sd, dtype="bf16", decode_lds_kb=lds_kb).to(DEV)
    prompt = torch.from_numpy(g["prompt"]).to(DEV)
    u = torch.rand(prompt.shape[0], 24, generator=torch.Generator().manual_seed(24)).to(DEV)
    switches(IVG_DECODE_ATTN_WINDOW=None)
    new = m.generate(prompt, do_sample=True, top_k=100, max_new_tokens=24, uniforms=u).cpu()
    switches(IVG_DECODE_ATTN_WINDOW="0")
    old = m.generate(prompt, do_sample=True, top_k=100, max_new_tokens=24, uniforms=u).cpu()
    assert new.shape == (prompt.shape[0], prompt.shape[1] + 24)
    assert torch.equal(new, old), f"{int((new != old).sum())} sampled tokens differ between the two bodies"
