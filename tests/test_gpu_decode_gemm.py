"""The decode-step GEMMs at op level against fp64, per element, at every plan the dispatchers produce (ivg_op_skinny_policy:
dg3_kernel of dgemm3.hip, dgemm_kernel of dgemm.hip; ivg_op_skinny_plan names the plan without launching).

Reference and bound: tests/decode_gemm_ref.py (module docstring: the split-bf16 operands, the per-element bound and its derivation,
the exact-rounding predicate); tests/test_decode_gemm_cpu.py shows on the CPU that the bound rejects each kernel mutant by >= 10x.

Every case (kind, K, N, flags, LDS budget, IVG_DG3) runs at every batch size of MS on the same 128 rows of X (X[:M]):
  - M = 128: every element within its bound, and every bf16 element the predicate decides equal to RNE of the fp64 value;
  - every other M: rows [0, M) bit-identical to the M = 128 run (batch invariance: the K partition and every sum order depend on
    (K bytes, N, dtype, flags) only), with ldx > K on odd-indexed batch sizes (the padding NaN, never read);
  - M = 128 again with the odd rows replaced: the even rows keep their bits (batch-mates do not matter);
  - Y's rows [M, M + 16) and columns [N_out, ldy) are NaN before and after (residual: Y == R in place).
Inputs: "mixed" rows (random; scaled from 2^-8 to 2^8; cancelling: W = [w | w] and x = [v | -v + d]; mean x^2 ~ eps; an all-zero
row) and, for the epilogue and model cases, "outlier" channels scaled by up to 2^12.
"""
import ctypes as C

import pytest
import torch

import decode_gemm_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NORM, GLU, RES, F32OUT = R.SK_NORM, R.IG_GLU, R.IG_RESIDUAL, R.IG_OUT_F32
CODE = {"fp32": 0, "bf16": 1, "x3": 2}
MS = (1, 2, 15, 16, 17, 31, 32, 33, 48, 49, 63, 64, 65, 100, 127, 128)
STATS = {}

# (kind, K, N, flags, lds_kb, IVG_DG3): together these reach every plan of EXPECTED_DG3 / EXPECTED_DG2 (a greedy cover over the
# batch sizes of MS, found with ivg_op_skinny_plan)
COVER = [
    ("bf16", 128, 256, 80, 160, 1), ("bf16", 128, 6144, 0, 160, 1), ("bf16", 128, 16386, 0, 16, 1), ("bf16", 128, 16386, 0, 160, 1),
    ("bf16", 192, 256, 80, 160, 1), ("bf16", 192, 6144, 0, 16, 1), ("bf16", 192, 6144, 0, 160, 1), ("bf16", 192, 16386, 0, 160, 1),
    ("bf16", 256, 1024, 0, 160, 1), ("bf16", 256, 2304, 80, 160, 1), ("bf16", 512, 1024, 0, 160, 1), ("bf16", 512, 2304, 80, 160, 1),
    ("bf16", 512, 6144, 0, 16, 1), ("bf16", 768, 768, 0, 160, 1), ("bf16", 768, 4096, 80, 160, 1), ("bf16", 1024, 256, 80, 160, 0),
    ("bf16", 1024, 1030, 0, 160, 1), ("bf16", 1024, 6144, 0, 160, 0), ("bf16", 1152, 6144, 0, 40, 1), ("bf16", 1152, 6144, 0, 160, 1),
    ("bf16", 1152, 16386, 0, 160, 1), ("bf16", 1536, 1024, 0, 160, 1), ("bf16", 1536, 1024, 80, 160, 0), ("bf16", 2048, 40, 0, 96, 0),
    ("bf16", 2048, 1024, 80, 160, 1), ("bf16", 2048, 6144, 0, 160, 0), ("bf16", 4608, 6144, 0, 160, 0), ("bf16", 5120, 16386, 0, 160, 1),
    ("fp32", 64, 256, 80, 160, 1), ("fp32", 64, 6144, 0, 160, 1), ("fp32", 64, 16386, 0, 16, 1), ("fp32", 64, 16386, 0, 160, 1),
    ("fp32", 96, 256, 80, 160, 1), ("fp32", 96, 6144, 0, 16, 1), ("fp32", 96, 6144, 0, 160, 1), ("fp32", 96, 16386, 0, 160, 1),
    ("fp32", 128, 1024, 0, 160, 1), ("fp32", 128, 2304, 80, 160, 1), ("fp32", 256, 1024, 0, 160, 1), ("fp32", 256, 2304, 80, 160, 1),
    ("fp32", 256, 6144, 0, 16, 1), ("fp32", 384, 1024, 0, 160, 1), ("fp32", 384, 4096, 80, 160, 1), ("fp32", 512, 256, 80, 160, 0),
    ("fp32", 512, 1030, 0, 160, 1), ("fp32", 512, 6144, 0, 160, 0), ("fp32", 576, 6144, 0, 40, 1), ("fp32", 576, 6144, 0, 160, 1),
    ("fp32", 576, 16386, 0, 160, 1), ("fp32", 768, 1024, 80, 160, 0), ("fp32", 1024, 40, 0, 96, 0), ("fp32", 1024, 1024, 80, 160, 1),
    ("fp32", 1024, 6144, 0, 160, 0), ("fp32", 2304, 6144, 0, 160, 0), ("fp32", 2560, 16386, 0, 160, 1),
    ("x3", 128, 1024, 0, 160, 1), ("x3", 128, 2304, 80, 160, 1), ("x3", 256, 1024, 0, 160, 1), ("x3", 256, 2304, 80, 160, 1),
    ("x3", 384, 1024, 0, 160, 1), ("x3", 384, 4096, 80, 160, 1), ("x3", 512, 1030, 0, 160, 1), ("x3", 1024, 1024, 80, 160, 1),
]
# every epilogue on both generations (x3: the third only; the second ignores the flag), ragged N: N % 16 != 0, N % 4 != 0 where the
# epilogue allows it, N < 4 on the second generation
EPILOGUES = [0, NORM, NORM | GLU, RES, NORM | RES, F32OUT, NORM | F32OUT]


def _epi_n(flags):
    return 1056 if flags & GLU else (1036 if flags & RES else 1030)


EPI = [(kind, 1536 if kind == "bf16" else 768, _epi_n(f), f, 160, dg3) for kind in R.KINDS for f in EPILOGUES for dg3 in (1, 0)
       if not (kind == "x3" and dg3 == 0)]
EPI += [("bf16", 512, 2, 0, 160, 1), ("fp32", 256, 3, NORM | F32OUT, 160, 1), ("bf16", 256, 3, RES, 160, 1)]
# the decode-step GEMMs of the small and medium transformers (test_gpu_ops.DECODE_SHAPES) under the budgets the headline runs with:
# 160 KiB alone, 40 KiB with shared-weight requests as bench.py's lanes launch them (lds_kb = -40 below)
_MODEL = [(768, 2304, NORM), (768, 768, RES), (768, 6144, NORM | GLU), (3072, 768, RES), (1024, 3072, NORM), (1024, 1024, RES),
          (1024, 8192, NORM | GLU), (4096, 1024, RES), (768, 16386, NORM | F32OUT), (1024, 16386, NORM | F32OUT)]
MODEL = [(kind, K, N, f, lds, 1) for kind in ("bf16", "fp32", "x3") for (K, N, f) in _MODEL for lds in (160, -40)
         if not (kind == "x3" and lds == -40)]

# every instance launch_dg3_w / launch_dg_t instantiate, less the ones no arguments reach:
#   dg3 (kind, MF, FN, WAVES): MF = 4 with FN = 2 at 16 waves stages 16 x (4 + 2) x 2 KiB = 192 KiB > 160 KiB, the most any budget
#     allows (dg3_plan halves MF instead)
#   gen2 (kind, MF, FN, LG, launch bound): every instance whose staging LG x waves x (MF + FN) x 2 KiB exceeds 160 KiB at the fewest
#     waves of its launch bound (bound 16: >= 12 waves; bound 8: >= 6 waves), so dg_plan shortens the bursts first -- and
#     (MF x FN = 8, LG 2, bound 8): 8 waves stage 192 KiB; 6 waves arise only from LG 3 with an odd burst count (dg_split), which
#     has no even split into bursts of 2 lines, so the budget takes LG from 3 straight to 1
EXPECTED_DG3 = {(k, mf, fn, w) for k in R.KINDS for mf in (1, 2, 4) for fn in (1, 2) for w in (16, 12, 8, 4)} - \
    {(k, 4, 2, 16) for k in R.KINDS}
_DG2_ALL = {(k, mf, fn, lg, wm) for k in ("bf16", "fp32") for mf in (1, 2, 4) for fn in (1, 2, 4) for lg in (1, 2, 3)
            for wm in (4, 8, 16) if not (wm == 8 and mf * fn > 8) and not (wm == 16 and mf * fn > 2)}
_DG2_UNREACHABLE = {(1, 2, 3, 16), (2, 1, 3, 16), (1, 4, 3, 8), (4, 1, 3, 8), (2, 4, 3, 8), (4, 2, 3, 8), (2, 4, 2, 8), (4, 2, 2, 8)}
EXPECTED_DG2 = {p for p in _DG2_ALL if p[1:] not in _DG2_UNREACHABLE}


def lib():
    from ivideogpt_amd import _lib
    return _lib, _lib.load()


def P(t):
    return C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def tdt(kind):
    return torch.bfloat16 if kind == "bf16" else torch.float32


def ldy_of(n_out):
    """Y's row stride in these tests: a multiple of 4 (the residual epilogue's vector loads) with padding columns past N_out"""
    return (n_out + 3) // 4 * 4 + 4


def skinny_plan(l, kind, M, N, K, flags, lds, X=4096, W=4096, Y=4096):
    out = (C.c_int32 * 11)()
    n_out = N // 2 if flags & GLU else N
    assert l.ivg_op_skinny_plan(M, N, K, K, K, ldy_of(n_out), flags, CODE[kind], abs(lds), X, W, Y, out) == 0
    return R.plan_dict(out)


def plan_key(kind, p):
    if p["gen"] == 3:
        return ("dg3", kind if (kind != "x3" or p["x3"]) else "fp32", p["mf"], p["fn"], p["waves"])
    return ("dg2", "bf16" if kind == "bf16" else "fp32", p["mf"], p["fn"], p["lg"], p["wmax"])


def inputs(kind, K, N, flags, which, seed):
    """-> X [128][K], W [N][K], R0 [128][N_out] (or None) as stored"""
    g = torch.Generator().manual_seed(seed)
    M = 128
    X = torch.randn(M, K, generator=g)
    W = torch.randn(N, K, generator=g) / K ** 0.5
    if which == "mixed":
        h = K // 2
        W[:, h:2 * h] = W[:, :h]
        for r in range(M):
            c = r % 8
            if c in (1, 2):
                X[r] *= 2.0 ** (((r * 5) % 17) - 8)                       # rows scaled from 2^-8 to 2^8
            elif c in (3, 4):
                X[r, h:2 * h] = -X[r, :h] + 2.0 ** -7 * torch.randn(h, generator=g)   # cancelling: |y| << sum |x w|
            elif c == 5:
                X[r] *= 1e-3 / X[r].pow(2).mean().sqrt()                  # mean x^2 ~ eps
        X[7] = 0.0                                                        # an all-zero row
    else:
        ch = torch.randperm(K, generator=g)[:8]
        X[:, ch] *= 2.0 ** torch.arange(5, 13, dtype=torch.float32)       # outlier channels up to 2^12
    n_out = N // 2 if flags & GLU else N
    R0 = (torch.randn(M, n_out, generator=g) * 2.0).to(tdt(kind)) if flags & RES else None
    return X.to(tdt(kind)), W.to(tdt(kind)), R0


def launch(l, kind, X, W, R0, M, N, K, flags, lds, pad_x):
    """-> Y [M + 16][ldy] after one launch on X[:M] (ldx = K + pad_x), NaN everywhere else"""
    es = R.elem_bytes(kind)
    ldx = K + pad_x
    n_out = N // 2 if flags & GLU else N
    ldy = ldy_of(n_out)
    xd = torch.full((M, ldx), float("nan"), dtype=tdt(kind), device=DEV)
    xd[:, :K] = X[:M].to(DEV)
    wd = W.to(DEV)
    odt = torch.float32 if (flags & F32OUT or kind != "bf16") else torch.bfloat16
    Y = torch.full((M + 16, ldy), float("nan"), dtype=odt, device=DEV)
    if R0 is not None:
        Y[:M, :n_out] = R0[:M].to(DEV, odt)
    assert (ldx * es) % 16 == 0
    rc = l.ivg_op_skinny_policy(P(xd), P(wd), P(Y), M, N, K, ldx, K, ldy, flags, CODE[kind], abs(lds), 1 if lds < 0 else 0, stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    Y = Y.cpu()
    assert torch.isnan(Y[M:]).all(), "rows below M were written"
    assert torch.isnan(Y[:, n_out:]).all(), "padding columns of Y were written"
    return Y[:M, :n_out]


def bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def run_case(case, which, switches, seed):
    kind, K, N, flags, lds, dg3 = case
    L, l = lib()
    switches(IVG_DG3=None if dg3 else "0", IVG_DECODE_LDS_KB=None)
    X, W, R0 = inputs(kind, K, N, flags, which, seed)
    plans = {M: skinny_plan(l, kind, M, N, K, flags, lds) for M in MS}
    p128 = plans[128]
    assert p128["gen"] in (2, 3), (case, p128)
    for M, p in plans.items():   # coverage and the K partition do not depend on the batch
        assert (p["gen"], p["waves"], R.lines_per_wave(p)) == (p128["gen"], p128["waves"], R.lines_per_wave(p128)), (M, p, p128)
    pad = 16 // R.elem_bytes(kind)
    Y128 = launch(l, kind, X, W, R0, 128, N, K, flags, lds, 0)
    # an x3 call the third generation does not cover (lm_head: 1025 W tiles) runs the second's fp32 arithmetic
    ref = R.reference(X, W, flags, "fp32" if (kind == "x3" and not p128["x3"]) else kind, p128, R=R0)
    res = R.check(Y128, ref)
    key = (p128["gen"], kind if (kind != "x3" or p128["x3"]) else "fp32", flags)
    s = STATS.setdefault(key, dict(ratio=0.0, decided=0, total=0))
    s["ratio"] = max(s["ratio"], res["ratio"])
    s["decided"] += res["decided"]
    s["total"] += res["total"] if ref["out_bf16"] else 0
    print(f"DGEMM_STAT {case} {which} gen{p128['gen']} ratio {res['ratio']:.3f} decided {res['decided']}/{res['total']}")
    assert res["ratio"] <= 1.0, (case, which, res)
    assert res["mismatched"] == 0, (case, which, res)
    if flags & NORM:   # the all-zero row: exactly 0, or the residual unchanged
        want = R0[7].float() if flags & RES else torch.zeros(Y128.shape[1])
        if which == "mixed":
            assert torch.equal(Y128[7].float(), want)
    for i, M in enumerate(MS[:-1]):
        Y = launch(l, kind, X, W, R0, M, N, K, flags, lds, pad if i % 2 else 0)
        assert torch.equal(bits(Y), bits(Y128[:M])), f"rows of M = {M} differ from the same rows at M = 128 ({case})"
    X2 = X.clone()
    X2[1::2] = torch.randn(64, K, generator=torch.Generator().manual_seed(seed + 1)).to(X.dtype)
    Y2 = launch(l, kind, X2, W, R0, 128, N, K, flags, lds, pad)
    assert torch.equal(bits(Y2[0::2]), bits(Y128[0::2])), f"rows changed with their batch-mates ({case})"
    return {plan_key(kind, p) for p in plans.values()} | {("ring", p["ring"]) for p in plans.values() if p["gen"] == 3} | \
        {("wr", p["wr"]) for p in plans.values() if p["gen"] == 3}


def _id(c):
    return f"{c[0]}-K{c[1]}-N{c[2]}-f{c[3]}-lds{c[4]}-dg3{c[5]}"


@pytest.mark.parametrize("case", COVER, ids=[_id(c) for c in COVER])
def test_cover_case(case, switches):
    run_case(case, "mixed", switches, seed=case[1] + case[2])


@pytest.mark.parametrize("which", ["mixed", "outlier"])
@pytest.mark.parametrize("case", EPI + MODEL, ids=[_id(c) for c in EPI + MODEL])
def test_epilogue_and_model_case(case, which, switches):
    run_case(case, which, switches, seed=case[1] * 3 + case[2] + case[3])


def test_plan_coverage(switches):
    """the plans the case tables reach through ivg_op_skinny_plan are exactly every instance the dispatchers can produce"""
    L, l = lib()
    reached = set()
    for kind, K, N, flags, lds, dg3 in COVER + EPI + MODEL:
        switches(IVG_DG3=None if dg3 else "0", IVG_DECODE_LDS_KB=None)
        for M in MS:
            p = skinny_plan(l, kind, M, N, K, flags, lds)
            reached.add(plan_key(kind, p))
            if p["gen"] == 3:
                reached |= {("ring", p["ring"]), ("wr", p["wr"])}
    assert {k[1:] for k in reached if k[0] == "dg3"} == EXPECTED_DG3
    assert {k[1:] for k in reached if k[0] == "dg2"} == EXPECTED_DG2
    assert {("ring", 1), ("ring", 2), ("wr", 12)} <= reached
    print(f"DGEMM_COVER dg3 {len(EXPECTED_DG3)} of 72, gen2 {len(EXPECTED_DG2)} of {len(_DG2_ALL)}")


@pytest.mark.parametrize("kind", ["bf16", "fp32"])
@pytest.mark.parametrize("K,N,flags", [(768, 2304, NORM), (768, 768, RES), (768, 6144, NORM | GLU), (3072, 768, RES),
                                       (1024, 16386, NORM | F32OUT), (1536, 1024, 0)])
def test_rows_bit_identical_across_lds_budgets_within_a_generation(kind, K, N, flags, switches):
    """dg3 changes only MF with the budget; gen2 changes LG, the burst count and MF and claims the sum order stays (dgemm.hip): the
    same rows give the same bits under every budget that keeps the generation (both generations, IVG_DG3=0 for the second)"""
    L, l = lib()
    X, W, R0 = inputs(kind, K, N, flags, "mixed", K + N)
    for dg3 in (1, 0):
        switches(IVG_DG3=None if dg3 else "0", IVG_DECODE_LDS_KB=None)
        by_gen = {}
        for lds in (160, 128, 96, 64, 40, 16):
            p = skinny_plan(l, kind, 128, N, K, flags, lds)
            Y = launch(l, kind, X, W, R0, 128, N, K, flags, lds, 0)
            by_gen.setdefault(p["gen"], []).append((lds, p, Y))
        for gen, runs in by_gen.items():
            for lds, p, Y in runs[1:]:
                assert torch.equal(bits(Y), bits(runs[0][2])), (gen, lds, p, runs[0][0], runs[0][1])


def test_x3_runs_the_split_instance_and_meets_its_bound(switches):
    """IVG_F32X3 through the op: the plan names the X3 instance, the gen3 counter moves, and the result meets the x3 bound -- which
    one bf16 product per element misses by orders of magnitude on the same input"""
    L, l = lib()
    switches(IVG_DG3=None, IVG_DECODE_LDS_KB=None)
    K, N, flags = 768, 2304, NORM
    X, W, _ = inputs("x3", K, N, flags, "outlier", 11)
    p = skinny_plan(l, "x3", 64, N, K, flags, 160)
    assert p["gen"] == 3 and p["x3"] == 1
    assert skinny_plan(l, "fp32", 64, N, K, flags, 160)["x3"] == 0
    c0 = l.ivg_debug_counter(b"decode_gemm_gen3")
    Y = launch(l, "x3", X, W, None, 64, N, K, flags, 160, 0)
    assert l.ivg_debug_counter(b"decode_gemm_gen3") - c0 == 1
    ref = R.reference(X[:64], W, flags, "x3", p)
    assert R.check(Y, ref)["ratio"] <= 1.0
    one = R.reference(X[:64], W, flags, "x3", p, mutant=("x3_one_bf16",))
    assert R.check(one["out"], ref)["ratio"] >= 10.0
    Yf = launch(l, "fp32", X, W, None, 64, N, K, flags, 160, 0)   # the f32-input instance: other bits
    assert not torch.equal(Y, Yf)


def test_plan_refusals(switches):
    """shapes neither generation covers: answered as gen 0 by the plan hook (never launched here)"""
    L, l = lib()
    switches(IVG_DG3=None, IVG_DECODE_LDS_KB=None)
    assert skinny_plan(l, "bf16", 128, 768, 768, 0, 160)["gen"] == 3
    assert skinny_plan(l, "bf16", 129, 768, 768, 0, 160)["gen"] == 0                     # M > 128
    assert skinny_plan(l, "bf16", 64, 768, 760, 0, 160)["gen"] == 0                      # K bytes not a multiple of 128
    assert skinny_plan(l, "fp32", 64, 768, 760, 0, 160)["gen"] == 0
    assert skinny_plan(l, "bf16", 64, 768, 768, 0, 160, X=4096 + 8)["gen"] == 0          # unaligned X
    assert skinny_plan(l, "bf16", 64, 768, 768, 0, 160, W=4096 + 4)["gen"] == 0          # unaligned W
    assert skinny_plan(l, "bf16", 64, 784, 768, NORM | GLU, 160)["gen"] == 0             # GLU with N % 32 != 0
    assert skinny_plan(l, "bf16", 0, 768, 768, 0, 160)["gen"] == 0                       # nothing to launch
    out = (C.c_int32 * 11)()
    assert l.ivg_op_skinny_plan(64, 768, 768, 768, 768, 768, 0, 3, 0, 4096, 4096, 4096, out) == -1
    assert l.ivg_op_skinny_plan(64, 768, 768, 768, 768, 768, 0, 1, 8, 4096, 4096, 4096, out) == -1


def test_op_refusals_leave_y_untouched():
    """dtype 3 and an LDS budget outside [16, 160] are IVG_ERR_INVALID before anything launches; M = 0 is a no-op"""
    L, l = lib()
    K, N = 768, 768
    x = torch.randn(16, K, device=DEV).to(torch.bfloat16)
    w = torch.randn(N, K, device=DEV).to(torch.bfloat16)
    Y = torch.full((16, N), 3.0, device=DEV, dtype=torch.bfloat16)
    for dtype, lds in ((3, 0), (-1, 0), (1, 8), (1, 161)):
        assert l.ivg_op_skinny_policy(P(x), P(w), P(Y), 16, N, K, K, K, N, 0, dtype, lds, 0, stream()) == -1
    assert l.ivg_op_skinny(P(x), P(w), P(Y), 16, N, K, K, K, N, 0, 3, stream()) == -1
    assert l.ivg_op_skinny(P(x), P(w), P(Y), 0, N, K, K, K, N, 0, 1, stream()) == 0
    torch.cuda.synchronize()
    assert (Y.float() == 3.0).all()


def test_zz_report():
    for key in sorted(STATS):
        s = STATS[key]
        frac = f"{s['decided'] / s['total']:.4f}" if s["total"] else "-"
        print(f"DGEMM_WORST gen{key[0]} {key[1]} flags {key[2]}: err/bound {s['ratio']:.3f}, exact-rounding decided {frac}")
