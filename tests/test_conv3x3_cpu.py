"""CPU self-check of tests/conv3x3_ref.py: the per-element bound of test_gpu_conv3x3.py rejects every kernel mutant by at least MARGIN
on an input built to expose it, an honest fp32 evaluation of the same convolution stays inside it, the reference equals plain torch
fp64, the case table reaches every instance the dispatcher can select, and the shares that make the predicates strong (decided bf16
outputs, decided fused-GroupNorm inputs) hold for the seeded inputs of every case -- a GPU run cannot hide behind a weak predicate."""
import pytest
import torch
import torch.nn.functional as F

import conv3x3_ref as R

MARGIN = 10.0
B = R.IG_BIAS_N


def built(c, mutant=None):
    plan = R.expected_plan(c)
    assert plan is not None, c
    inp = R.make_inputs(c)
    ref = R.case_reference(c, plan, inp)
    mut = R.case_reference(c, plan, inp, mutant=mutant) if mutant else None
    return plan, inp, ref, mut


def exposing_case(mk, kind):
    """a small case on which the mutant `mk` changes the result"""
    c3 = 96 if kind == "bf16" else 48          # three channel chunks
    if mk in ("drop_step", "stale_halo", "skip_last_chunk"):
        return R.case(kind, 16, 16, c3, 64, Nb=1)
    if mk in ("halo_col", "halo_row"):
        return R.case(kind, 16, 64, c3 // 3, 64, Nb=1)                     # 2 x 2 tiles of 8 x 32
    if mk in ("pad_normalised", "coef_xor1", "coef_next_image"):
        return R.case(kind, 16, 16, 2 * c3 // 3, 64, gn=16, Nb=2)
    if mk == "phase_transposed":
        return R.case(kind, 16, 16, c3 // 3, 64, ups=1)
    if mk == "x3_drop_hilo":
        return R.case(kind, 16, 16, c3, 64)
    if mk == "bias_shift":
        return R.case(kind, 16, 16, c3 // 3, 192 - 56)                     # tiles of 128: the second holds 8 columns
    if mk in ("res_missing", "res_twice"):
        return R.case(kind, 16, 16, c3 // 3, 64, res=1)
    raise KeyError(mk)


def fp32_emulation(c, inp, coef, plan=None):
    """the same operation in plain fp32 torch arithmetic (another summation order, one rounding per operation); a sub-pixel plan is
    evaluated as its four phase convolutions with the packed weights as stored, which is what the kernel multiplies"""
    kind = c["kind"]
    x = inp["x"].float()
    if c["gn"]:
        x = F.silu(x * coef[:, None, None, :, 0] + coef[:, None, None, :, 1])
        x = x.to(R.tdt(kind)).float()
    sub = bool(plan and plan["subpix"])
    w = (inp["w_sub"] if sub else inp["w"]).float()
    if kind == "x3":
        (xh, xl), (wh, wl) = R.bf16_split(x), R.bf16_split(w)
        x, w = (xh + xl).float(), (wh + wl).float()
    xin = x.permute(0, 3, 1, 2)
    if sub:
        N, Cin = c["N"], c["Cin"]
        y = R._conv(xin, w.reshape(4, N, 2, 2, Cin).permute(0, 1, 4, 2, 3).contiguous(), plan, 1) + inp["bias"].float()[None, :, None, None]
    else:
        if c["ups"]:
            xin = F.interpolate(xin, scale_factor=2.0, mode="nearest")
        y = F.conv2d(xin, R._w4(w, c["Cin"]), inp["bias"].float(), padding=1)
    if c["res"]:
        y = y + inp["res"].float().permute(0, 3, 1, 2)
    if c["flags"] & R.IG_SILU:
        y = F.silu(y)
    if c["flags"] & R.IG_RELU:
        y = y.clamp_min(0.0)
    if c["flags"] & R.IG_CLAMP01:
        y = y.clamp(0.0, 1.0)
    y = y.permute(0, 2, 3, 1)
    return y.to(torch.bfloat16) if (kind == "bf16" and not c["flags"] & R.IG_OUT_F32) else y


MUTANT_CASES = [(name, mt[0], kind) for name, mt in R.MUTANTS.items() for kind in R.KINDS if not (mt[0] == "x3_drop_hilo" and kind != "x3")]


@pytest.mark.parametrize("name,mk,kind", MUTANT_CASES, ids=[f"{m[1]}-{m[2]}" for m in MUTANT_CASES])
def test_bound_rejects_mutant(name, mk, kind):
    c = exposing_case(mk, kind)
    plan, inp, ref, mut = built(c, (mk,))
    coef = R.coef_model(inp["x"], inp["gamma"], inp["beta"], c["gn"]) if c["gn"] else None
    good, bad = R.check(fp32_emulation(c, inp, coef, plan), ref), R.check(mut["out"], ref)   # good: an honest fp32 run of this very case
    print(f"CONV3_MUTANT {mk} {kind}: err/bound {bad['ratio']:.1f} (honest fp32 evaluation {good['ratio']:.3f})")
    assert good["ratio"] <= 1.0 and good["mismatched"] == 0, good
    assert bad["ratio"] >= MARGIN, f"{name} ({kind}): err/bound only {bad['ratio']:.2f}"


def test_truncating_store_is_caught_by_the_rounding_predicate_not_the_bound():
    _, _, ref, mut = built(R.case("bf16", 16, 16, 64, 64, res=1), ("trunc_store",))
    good, bad = R.check(ref["out"], ref), R.check(mut["out"], ref)
    print(f"CONV3_MUTANT trunc_store: err/bound {bad['ratio']:.2f}, decided {good['decided']}/{good['total']}, mismatched {bad['mismatched']}")
    assert bad["ratio"] <= 1.0
    assert good["decided"] > 0.75 * good["total"] and good["mismatched"] == 0
    assert bad["mismatched"] > 0.3 * bad["decided"]


@pytest.mark.parametrize("name,mk", [(n, m[0]) for n, m in R.STATS_MUTANTS.items()], ids=[m[0] for m in R.STATS_MUTANTS.values()])
def test_statistics_bound_rejects_mutant(name, mk):
    c = R.case("bf16", 32, 16, 32, 192, stats=32, res=1)                  # 6 channels per group: group 21 straddles channel 128
    plan, _, ref, mut = built(c, (mk,))
    ratio = lambda S: float(((S - ref["stats"]).abs() / ref["stats_bound"]).max())   # noqa: E731
    assert R.check_stats(ref["stats"], ref["out"], 32, plan) == 0.0
    print(f"CONV3_MUTANT {mk}: err/bound {ratio(mut['stats']):.1f}")
    assert ratio(mut["stats"]) >= MARGIN, name


PLAIN = [R.case(k, 16, 16, 96, 80, Nb=2, res=1, cls=cls) for k in R.KINDS for cls in ("random", "scaled")] + \
    [R.case(k, 8, 16, 96, 64, ups=1, sub=0) for k in R.KINDS] + \
    [R.case(k, 16, 16, 64, 64, gn=16, Nb=2, res=1, cls=cls) for k in R.KINDS for cls in ("random", "gn_edge")] + \
    [R.case("fp32", 16, 16, 32, 64, flags=B | R.IG_RELU), R.case("bf16", 16, 16, 32, 64, flags=B | R.IG_SILU),
     R.case("bf16", 16, 16, 32, 3, flags=B | R.IG_CLAMP01)]


@pytest.mark.parametrize("c", PLAIN, ids=[R.case_id(c) for c in PLAIN])
def test_fp32_evaluation_within_bound_and_reference_matches_plain_fp64(c):
    plan, inp, ref, _ = built(c)
    coef = R.coef_model(inp["x"], inp["gamma"], inp["beta"], c["gn"]) if c["gn"] else None
    res = R.check(fp32_emulation(c, inp, coef, plan), ref)
    print(f"CONV3_FP32 {R.case_id(c)}: err/bound {res['ratio']:.3f}, decided {res['decided']}/{res['total']}, mismatched {res['mismatched']}")
    assert res["ratio"] <= 1.0 and res["mismatched"] == 0, res
    # the reference's value against a plain fp64 statement: torch's own conv2d / group_norm / interpolate on the operands the kernel
    # multiplies (x3: the split pairs; bf16 GroupNorm: the normalised tensor rounded to bf16).  GroupNorm cases take the reference
    # with the fp64 coefficients of coef_reference in place of the fp32 table, so that nothing but fp64 rounding separates the two.
    kind = c["kind"]
    x, w = inp["x"].double(), inp["w"].double()
    tol = 1e-12
    if kind == "x3":
        wh, wl = R.bf16_split(inp["w"])
        w = wh + wl
    if c["gn"]:
        sc, sh, _, _ = R.coef_reference(inp["x"], inp["gamma"], inp["beta"], c["gn"], 0)
        ref = R.case_reference(c, plan, inp, coef=torch.stack([sc, sh], -1))
        x = F.silu(F.group_norm(x.permute(0, 3, 1, 2), c["gn"], inp["gamma"].double(), inp["beta"].double(), eps=R.EPS)).permute(0, 2, 3, 1)
        if kind == "bf16":
            x = torch.from_numpy(R.rne_bf16(x.numpy()))
        # coef_reference takes the variance as E[x^2] - E[x]^2 like the device: the mean-30, spread-0.5 group of gn_edge loses
        # 900 / 0.25 = 3.6e3 of fp64's 1.1e-16 there, ~4e-13 of the variance -> 1e-10 leaves two orders
        tol = 1e-10
    elif kind == "x3":
        xh, xl = R.bf16_split(inp["x"])
        x = xh + xl
    xin = x.permute(0, 3, 1, 2)
    if c["ups"]:
        xin = F.interpolate(xin, scale_factor=2.0, mode="nearest")
    y = F.conv2d(xin, R._w4(w, c["Cin"]), inp["bias"].double(), padding=1)
    if c["res"]:
        y = y + inp["res"].double().permute(0, 3, 1, 2)
    if c["flags"] & R.IG_SILU:
        y = F.silu(y)
    if c["flags"] & R.IG_RELU:
        y = y.clamp_min(0.0)
    if c["flags"] & R.IG_CLAMP01:
        y = y.clamp(0.0, 1.0)
    assert torch.allclose(ref["pre"], y.permute(0, 2, 3, 1), rtol=tol, atol=tol * float(y.abs().max()))


@pytest.mark.parametrize("kind", R.KINDS)
def test_subpixel_reference_equals_the_nine_tap_statement(kind):
    """the four phase convolutions with fp64 pre-summed weights are the upsampled convolution exactly"""
    from ivideogpt_amd.packing import pack_subpixel
    c = R.case(kind, 16, 16, 32, 64, ups=1)
    plan, inp = R.expected_plan(c), R.make_inputs(c)
    assert plan["subpix"] == 1
    w4 = R._w4(inp["w"].double(), 32)
    sub = pack_subpixel(w4.float()).double() if kind == "bf16" else None   # bf16 weights: the fp32 sums are exact
    if sub is None:
        rows = ((w4[:, :, 0], w4[:, :, 1] + w4[:, :, 2]), (w4[:, :, 0] + w4[:, :, 1], w4[:, :, 2]))
        blk = []
        for py in range(2):
            for px in range(2):
                taps = []
                for kh2 in range(2):
                    r = rows[py][kh2]
                    cols = (r[:, :, 0], r[:, :, 1] + r[:, :, 2]) if px == 0 else (r[:, :, 0] + r[:, :, 1], r[:, :, 2])
                    taps += [cols[0], cols[1]]
                blk.append(torch.stack(taps, 1).reshape(64, -1))
        sub = torch.cat(blk, 0)
    x = inp["x"].double()
    got = R._conv(x.permute(0, 3, 1, 2), sub.reshape(4, 64, 2, 2, 32).permute(0, 1, 4, 2, 3).contiguous(), plan, 1)
    want = F.conv2d(F.interpolate(x.permute(0, 3, 1, 2), scale_factor=2.0, mode="nearest"), w4, padding=1)
    assert torch.allclose(got, want, rtol=1e-12, atol=1e-12)


def test_case_table_reaches_every_instance_the_dispatcher_can_select():
    reached = {R.instance(R.expected_plan(c)) for c in R.CASES}
    assert reached == R.EXPECTED, (R.EXPECTED - reached, reached - R.EXPECTED)
    assert not (reached & R.UNREACHABLE) and len(R.EXPECTED) == 50
    ids = [R.case_id(c) for c in R.CASES]
    assert len(set(ids)) == len(ids)


def test_axes_of_the_case_table():
    cs = R.CASES
    plans = [R.expected_plan(c) for c in cs]
    assert {1, 2, 3, 5, 8, 24} <= {p["chunks"] for p in plans}
    assert {1, 2, 6} <= {p["tiles_n"] for p in plans}
    assert {3, 16, 17, 64, 65, 66, 192, 768} <= {c["N"] for c in cs}
    assert {(8, 32), (24, 64), (16, 96), (32, 16)} <= {(c["H"], c["W"]) for c in cs}
    assert any(c["ups"] and (c["H"], c["W"]) == (8, 16) and p["ups"] == 1 for c, p in zip(cs, plans))
    assert any(c["N"] == 768 and c["stats"] == 32 for c in cs)
    for k in R.KINDS:
        for bn in (64, 128):
            assert any(c["kind"] == k and c["gn"] and c["stats"] and c["res"] and p["bn"] == bn and c["src"] == s for c, p in zip(cs, plans)
                       for s in ("conv",)), (k, bn)
            assert any(c["kind"] == k and c["gn"] and c["stats"] and c["res"] and p["bn"] == bn and c["src"] == "partial" for c, p in zip(cs, plans))


BF16_CASES = [c for c in R.CASES if c["kind"] == "bf16"]
_SHARES = {}


@pytest.mark.parametrize("c", BF16_CASES, ids=[R.case_id(c) for c in BF16_CASES])
def test_decided_shares_of_the_seeded_inputs(c):
    """>= 0.3 of the bf16 outputs decided in every case, >= 0.9 in the sparse-K ones; <= 1 % of the fused-GroupNorm inputs undecided"""
    plan, inp, ref, _ = built(c)
    res = R.check(ref["out"], ref)
    assert res["mismatched"] == 0 and res["ratio"] <= 0.5
    if ref["out_bf16"]:
        share = res["decided"] / res["total"]
        _SHARES[R.case_id(c)] = share
        print(f"CONV3_SHARE {R.case_id(c)}: decided {share:.3f}, undecided GroupNorm inputs {ref['undecided_in']:.2e}")
        assert share >= (0.9 if c["cls"] == "sparse" else 0.3)
    if c["gn"]:
        assert ref["undecided_in"] <= 0.01
    if c["cls"] == "sparse":
        nz = (inp["w"].float().reshape(c["N"], 9, c["Cin"] // 32, 32) != 0)
        assert nz.sum((1, 3)).max() <= 1, "at most one term per (row, chunk)"
        assert nz.any(0).any(0).any(0).all() and nz.any(0).any(1).any(1).all() and nz.any(0).any(0).any(1).all(), \
            "the non-zero weights use every lane slot of a chunk, every tap and every chunk"


def test_every_bf16_instance_with_large_cin_runs_a_sparse_case():
    """every bf16 instance that the table runs at Cin >= 256 -- where the decided share of random inputs falls towards the floor --
    also runs a sparse-K case at Cin >= 256 (instances the table reaches only at small Cin keep their high random-input share)"""
    big = {R.instance(R.expected_plan(c)) for c in BF16_CASES if c["Cin"] >= 256}
    sparse = {R.instance(R.expected_plan(c)) for c in BF16_CASES if c["Cin"] >= 256 and c["cls"] == "sparse"}
    assert big == sparse, big - sparse


@pytest.mark.parametrize("kind", R.KINDS)
def test_coefficient_bound_accepts_the_model_and_rejects_wrong_statistics(kind):
    c = R.case(kind, 16, 16, 64, 64, gn=16, Nb=2, cls="gn_edge")
    inp = R.make_inputs(c)
    coef = R.coef_model(inp["x"], inp["gamma"], inp["beta"], 16)
    assert R.check_coef(coef, inp["x"], inp["gamma"], inp["beta"], 16, 8) <= 0.5
    assert R.check_coef(coef.roll(1, 0), inp["x"], inp["gamma"], inp["beta"], 16, 8) >= MARGIN          # another image's statistics
    bad = R.coef_model(inp["x"], inp["gamma"], inp["beta"], 16, eps=0.0)                                   # eps omitted: the zero image
    assert R.check_coef(bad, inp["x"], inp["gamma"], inp["beta"], 16, 8) >= MARGIN
