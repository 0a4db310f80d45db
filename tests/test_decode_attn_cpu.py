"""CPU self-check of tests/decode_attn_ref.py: the per-row bound of test_gpu_decode_attn.py rejects each kernel mutant by at least
MARGIN on the needle inputs built to expose it, and the reference itself agrees with a plain per-trajectory fp64 einsum."""
import math

import numpy as np
import pytest
import torch

import decode_attn_ref as R

MARGIN = 10.0
INSTANCES = [("bf16", hd) for hd in (8, 16, 32, 64, 128, 256)] + [("fp32", hd) for hd in (4, 8, 16, 32, 64, 128, 256)] + [("kv24", 64)]


def mutants(kind, hd, pos, step, P, shared):
    """the kernel bugs a case at (pos, step, P) is built to expose (needle_positions plants a needle at every key named here)."""
    m = {"key pos-1 dropped": ("drop", pos - 1), "key 0 dropped": ("drop", 0), "fed token dropped": ("drop", pos),
         "V shifted by one against K": ("v_shift",), "RoPE at pos-1": ("rope_pos", pos - 1), "RoPE at pos+1": ("rope_pos", pos + 1),
         "row pos+1 included": ("include_next",)}
    for t in (step - 1, step):
        if t < pos - 1:
            m[f"block-edge key {t} dropped"] = ("drop", t)
            m[f"block-edge key {t} read from row {t + 1}"] = ("key_from", t, t + 1)
    if hd != 64:
        m["scale 1/8 at hd != 64"] = ("scale", 0.125)
    if shared:
        m[f"key P-1 = {P - 1} read from the own row"] = ("prefix_own", P - 1)
        m[f"key P = {P} read from the slot row"] = ("own_from_slot", P)
        m["slot computed without row0"] = ("slot_no_row0",)
    return m


def independent_fp64(case, kind, heads, hd, pos, P, G, row0, ref):
    """softmax(q K^T / sqrt(hd)) V per trajectory with torch einsum, from the reference's own roped q and appended k / v."""
    B = case["qkv"].shape[0]
    out = torch.empty(B, heads, hd, dtype=torch.float64)
    q, kn, vn = torch.from_numpy(ref["q"]), torch.from_numpy(ref["k_new"]).double(), torch.from_numpy(ref["v_new"]).double()
    for b in range(B):
        s_ = (b - row0) // G
        K = torch.cat([case["K"][s_, :, :P], case["K"][b, :, P:pos]], 1).double()
        V = torch.cat([case["V"][s_, :, :P], case["V"][b, :, P:pos]], 1).double()
        K, V = torch.cat([K, kn[b][:, None]], 1), torch.cat([V, vn[b][:, None]], 1)
        w = torch.softmax(torch.einsum("hd,hkd->hk", q[b], K) / math.sqrt(hd), -1)
        out[b] = torch.einsum("hk,hkd->hd", w, V)
    return out.numpy()


@pytest.mark.parametrize("shared", [False, True], ids=["plain", "shared"])
@pytest.mark.parametrize("kind,hd", INSTANCES, ids=[f"{k}-hd{h}" for k, h in INSTANCES])
def test_decode_reference_detects_kernel_mutants(kind, hd, shared):
    """Needle inputs at the instance's (hd, step), unread rows finite (a trap needle at row pos + 1): every mutant of
    decode_attn_ref.decode_ref misses the true reference by >= MARGIN x the bound on at least one output row, and the unmutated
    reference is within 1e-6 x its bound of an independent fp64 einsum."""
    _, _, step = R.geometry(kind, hd)
    Lmax = min(1024, 2 * step + 8)
    pos = min(2 * step + 1, Lmax - 2)
    B, heads = (6, 8) if shared else (2, 8)
    G, row0 = (3, -1) if shared else (1, 0)
    P = (step if step + 2 < pos else pos // 2) if shared else 0
    case = R.make_case(kind, hd, heads, B, Lmax, pos, P, G, row0, family="needle", seed=hd + 7 * shared, poison=False)
    args = (case["qkv"], case["K"], case["V"], case["cos"], case["sin"], kind, heads, hd, pos, P, G, row0)
    ref = R.decode_ref(*args)
    bound = ref["bound"]
    assert np.isfinite(ref["out"]).all() and (bound > 0).all()
    ind = independent_fp64(case, kind, heads, hd, pos, P, G, row0, ref)
    assert (np.abs(ind - ref["out"]).max(-1) <= 1e-6 * bound).all(), "the reference disagrees with a plain fp64 einsum"
    worst = {}
    for name, mut in mutants(kind, hd, pos, step, P, shared).items():
        miss = np.abs(R.decode_ref(*args, mutant=mut)["out"] - ref["out"]).max(-1) / bound
        worst[name] = float(miss.max())
    print(f"{kind} hd {hd} step {step} pos {pos} P {P}: smallest rejection {min(worst.values()):.1f}x ({min(worst, key=worst.get)})")
    weak = {k: round(v, 2) for k, v in worst.items() if not v >= MARGIN}
    assert not weak, f"mutants the bound does not reject by {MARGIN}x: {weak}"


def test_decode_hook_refuses_uncovered_head_dims_before_any_launch():
    """ivg_op_shared_decode_attn checks decode_attn_covers (the predicate ivg_create uses) before it allocates or launches anything
    (no GPU needed): bf16 head dims 24, 48, 512, fp32 12 and an unknown dtype are IVG_ERR_INVALID; so are heads <= 0 and B <= 0."""
    import ctypes as C
    from ivideogpt_amd import _lib
    f = _lib.load().ivg_op_shared_decode_attn
    x = C.c_void_p(16)
    for B, heads, hd, dt in ((2, 2, 24, 1), (2, 2, 48, 1), (2, 2, 512, 1), (2, 2, 12, 0), (2, 2, 6, 0), (2, 2, 64, 2), (2, 0, 64, 1),
                             (0, 2, 64, 1)):
        assert f(x, x, x, x, x, x, B, heads, hd, 16, 3, 0, 1, 0, dt, None) == -1, (B, heads, hd, dt)
