"""CPU self-check of tests/decode_gemm_ref.py: the per-element bound of test_gpu_decode_gemm.py rejects each kernel mutant by at least
MARGIN on an input built to expose it, a plain fp32 evaluation of the same GEMM stays within it, and the reference agrees with a
plain torch fp64 statement of the epilogues."""
import pytest
import torch
import torch.nn.functional as F

import decode_gemm_ref as R

MARGIN = 10.0
NORM, GLU, RES, F32OUT = R.SK_NORM, R.IG_GLU, R.IG_RESIDUAL, R.IG_OUT_F32
# a gen3 plan of 4 waves x 3 lines (K = 12 lines of 128 bytes) and a gen2 plan of 2 waves x 2 bursts x 3 lines
PLANS = {"gen3": dict(gen=3, mf=1, fn=1, waves=4, klw=3, ring=2, lg=0, nburst=0, wmax=0, wr=16, x3=0),
         "gen2": dict(gen=2, mf=1, fn=1, waves=2, klw=0, ring=0, lg=3, nburst=2, wmax=4, wr=16, x3=0)}


def stored(t, kind):
    return t.to(torch.bfloat16) if kind == "bf16" else t.float()


def case(kind, plan, mutant, seed=3):
    """-> (X, W, flags, R0): an input that exposes `mutant` (row / line / column structure chosen for it)"""
    g = torch.Generator().manual_seed(seed)
    epl = 128 // R.elem_bytes(kind)
    lines = plan["waves"] * R.lines_per_wave(plan)
    K, M, N = lines * epl, 8, 64
    flags = 0
    X = torch.randn(M, K, generator=g)
    if mutant in ("drop_line", "dup_line"):
        j = (plan["waves"] - 1) * R.lines_per_wave(plan)
        X[:, j * epl:(j + 2) * epl] *= 16.0                    # the lines the mutant loses / repeats carry most of y
        X[:, (j + 1) * epl:(j + 2) * epl] *= -1.0
    if mutant == "rs_xor1":
        flags = NORM
        X *= torch.tensor([1.0, 2.5] * (M // 2))[:, None]      # neighbouring rows' RMS differ by 2.5x
    if mutant == "no_eps":
        flags = NORM
        X *= 1e-3                                              # mean x^2 ~ eps
    if mutant == "inv_k_minus1":
        flags = NORM | F32OUT if kind == "bf16" else NORM
    if mutant in ("glu_swap", "glu_rs_one"):
        flags = NORM | GLU
        X *= 4.0                                               # rs = 1/4: a missing rs is a factor 4
    if mutant in ("res_missing", "res_twice"):
        flags = RES
    if mutant == "tail_col_shift":
        N = 40                                                 # a partial last tile of 8 columns
    if mutant == "trunc_store":
        flags = NORM
    W = torch.randn(N, K, generator=g) / K ** 0.5
    n_out = N // 2 if flags & GLU else N
    R0 = stored(torch.randn(M, n_out, generator=g), kind) if flags & RES else None
    return stored(X, kind), stored(W, kind), flags, R0


def margin(kind, plan, mutant):
    X, W, flags, R0 = case(kind, plan, mutant)
    ref = R.reference(X, W, flags, kind, plan, R=R0)
    mut = R.reference(X, W, flags, kind, plan, R=R0, mutant=(mutant,))
    return R.check(mut["out"], ref), R.check(ref["out"], ref)


MUTANT_CASES = [(name, mt[0], kind, pn) for name, (mt, kinds) in R.MUTANTS.items() for kind in kinds for pn in PLANS
                if not (kind == "x3" and pn == "gen2")]


@pytest.mark.parametrize("name,mutant,kind,pn", MUTANT_CASES, ids=[f"{c[1]}-{c[2]}-{c[3]}" for c in MUTANT_CASES])
def test_bound_rejects_mutant(name, mutant, kind, pn):
    bad, good = margin(kind, PLANS[pn], mutant)
    assert good["ratio"] <= 0.5 and good["mismatched"] == 0       # the true result, correctly rounded, passes with room
    assert bad["ratio"] >= MARGIN, f"{name} ({kind}, {pn}): err/bound only {bad['ratio']:.2f}"


@pytest.mark.parametrize("kind", ["bf16"])
@pytest.mark.parametrize("pn", list(PLANS))
def test_truncating_store_is_caught_by_the_rounding_predicate_not_the_bound(kind, pn):
    """A bf16 store that truncates is off by less than one bf16 ulp: within the 2 * 2^-8 |y| of the bound (so the bound cannot
    reject it), but the exact-rounding predicate finds its bits wrong wherever it decides an element."""
    bad, good = margin(kind, PLANS[pn], "trunc_store")
    assert bad["ratio"] <= 1.0
    assert good["decided"] > 0.75 * good["total"]
    assert bad["mismatched"] > 0.3 * bad["decided"]


def fp32_emulation(X, W, flags, kind, R0):
    """the same GEMM in plain fp32 torch arithmetic (another sum order, one rounding per operation), rounded to the output type"""
    x, w = X.float(), W.float()
    if kind == "x3":
        xh, xl = (t.float() for t in R.bf16_split(x))
        wh, wl = (t.float() for t in R.bf16_split(w))
        y = ((xh @ wh.T + xl @ wh.T) + xh @ wl.T) + xl @ wl.T
    else:
        y = x @ w.T
    if flags & NORM:
        y = y * torch.rsqrt((x * x).sum(1, keepdim=True) * (1.0 / x.shape[1]) + R.EPS)
    if flags & GLU:
        nb = w.shape[0] // 32
        gi = (torch.arange(nb)[:, None] * 32 + torch.arange(16)[None, :]).reshape(-1)
        y = F.silu(y[:, gi]) * y[:, gi + 16]
    if flags & RES:
        y = R0.float() + y
    return y if (kind != "bf16" or flags & F32OUT) else y.to(torch.bfloat16)


EPILOGUES = [0, NORM, NORM | GLU, RES, NORM | RES, F32OUT, NORM | F32OUT]


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("flags", EPILOGUES)
def test_fp32_evaluation_within_bound_and_reference_matches_plain_fp64(kind, flags):
    g = torch.Generator().manual_seed(flags + 7)
    plan = PLANS["gen3"]
    K = 12 * 128 // R.elem_bytes(kind)
    M, N = 9, 96
    X = stored(torch.randn(M, K, generator=g) * torch.logspace(-3, 3, M, base=2.0)[:, None], kind)
    W = stored(torch.randn(N, K, generator=g) / K ** 0.5, kind)
    n_out = N // 2 if flags & GLU else N
    R0 = stored(torch.randn(M, n_out, generator=g), kind) if flags & RES else None
    ref = R.reference(X, W, flags, kind, plan, R=R0)
    res = R.check(fp32_emulation(X, W, flags, kind, R0), ref)
    assert res["ratio"] <= 1.0 and res["mismatched"] == 0, res
    # the reference's pre-rounding value against a plain fp64 statement (x3: of the split operands)
    if kind == "x3":
        xh, xl = R.bf16_split(X)
        wh, wl = R.bf16_split(W)
        x64, w64 = xh + xl, wh + wl
    else:
        x64, w64 = X.double(), W.double()
    y = x64 @ w64.T
    if flags & NORM:
        y = y * torch.rsqrt(X.double().pow(2).mean(1, keepdim=True) + R.EPS)
    if flags & GLU:
        gate = torch.cat([y[:, i:i + 16] for i in range(0, N, 32)], 1)
        up = torch.cat([y[:, i + 16:i + 32] for i in range(0, N, 32)], 1)
        y = F.silu(gate) * up
    if flags & RES:
        y = y + R0.double()
    assert torch.allclose(ref["pre"], y, rtol=1e-12, atol=1e-12 * float(y.abs().max()))
