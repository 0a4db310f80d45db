"""CPU self-check of tests/norm_ref.py (softmax, GroupNorm, RMSNorm): each reference agrees with an independent torch formulation,
an fp32 restatement of each kernel (same sum structure) stays within half the bound on every case of the table (bf16 outputs: half
the bound without its store term before the store, the whole bound after it -- norm_ref's docstring), every kernel mutant
misses the true reference by at least MARGIN x the bound on at least one case, and the bf16 RMSNorm candidates leave at most 1 % of
any case undecided."""
import torch

import norm_ref as R

MARGIN = 10.0


def report(kernel, best):
    for m, (miss, at) in best.items():
        print(f"{kernel} mutant {m}: rejected by {miss:.1f}x at {at}")
    weak = {m: v[0] for m, v in best.items() if not v[0] >= MARGIN}
    assert not weak, f"{kernel}: mutants the bound does not reject by {MARGIN}x: {weak}"


def keep(best, m, miss, at):
    if miss > best[m][0]:
        best[m] = (miss, at)


# ------------------------------------------------------------------------------------------------ softmax
def test_softmax_reference_restatement_and_mutants():
    best = {m: (0.0, None) for m in ("lim+1", "lim-1", "max256", "drop_wave", "pad_unwritten")}
    worst, at = 0.0, None
    for c in R.SOFTMAX_CASES:
        dt, Lq, Lk, lds, ldp, causal, fam = c
        S = R.softmax_inputs(c)
        ref, bound = R.softmax_ref(S, Lq, Lk, ldp, causal, dt)
        assert torch.isfinite(ref).all()
        ind = R.softmax_torch(S, Lq, Lk, causal)
        assert ((ref[:, :Lk] - ind).abs() <= 1e-6 * bound[:, :Lk] + 1e-300).all(), R.softmax_id(c)
        assert (ref[:, Lk:] == 0).all() and (ref.sum(-1) - 1).abs().max() < 1e-12
        r = float(R.ratio((R.softmax_restated(S, Lq, Lk, ldp, causal, dt, rounded=False) - ref).abs(),
                          R.softmax_ref(S, Lq, Lk, ldp, causal, dt, out_term=False)[1]).max())
        assert float(R.ratio((R.softmax_restated(S, Lq, Lk, ldp, causal, dt) - ref).abs(), bound).max()) <= 1.0, R.softmax_id(c)
        if r > worst:
            worst, at = r, R.softmax_id(c)
        assert r <= 0.5, f"{R.softmax_id(c)}: the fp32 restatement reaches {r:.3f} of the bound"
        for m in best:
            out, _ = R.softmax_ref(S, Lq, Lk, ldp, causal, dt, mutant=m)
            keep(best, m, float(R.ratio((out - ref).abs(), bound).max()), R.softmax_id(c))
    print(f"softmax: restatement worst err / bound {worst:.3f} ({at})")
    report("softmax", best)


# ------------------------------------------------------------------------------------------------ GroupNorm
def test_groupnorm_case_table_covers_every_p_with_and_without_idle_lanes():
    seen = {}
    for c in R.GN_CASES:
        vpp = R.gn_geometry(c["P"], c["C"], c["dt"])[0]
        seen.setdefault(c["P"], set()).add(256 % vpp == 0)
    assert set(seen) == {1, 5, 255, 256, 257, 1024, 1025, 2049} and all(v == {True, False} for v in seen.values()), seen
    assert {c["family"] for c in R.GN_CASES} == set(R.GN_FAMILIES) and {c["eps"] for c in R.GN_CASES} == {1e-6, 1e-5}
    assert len(R.GN_CASES) <= 32


def test_groupnorm_reference_restatement_and_mutants():
    names = ("count_padded", "stats_image0", "cpg_32_groups", "pos_block", "no_eps", "idle_lanes")
    best = {m: (0.0, None) for m in names}
    worst, at = 0.0, None
    for c in R.GN_CASES:
        x, gamma, beta, pos = R.gn_inputs(c)
        ref, bound = R.gn_ref(c, x, gamma, beta, pos)
        assert torch.isfinite(ref).all() and (bound > 0).all()
        ind = R.gn_torch(c, x, gamma, beta, pos)
        assert ((ref - ind).abs() <= 1e-6 * bound).all(), f"{R.gn_id(c)}: the reference disagrees with fp64 group_norm"
        r = float(R.ratio((R.gn_restated(c, x, gamma, beta, pos, rounded=False) - ref).abs(),
                          R.gn_ref(c, x, gamma, beta, pos, out_term=False)[1]).max())
        assert float(R.ratio((R.gn_restated(c, x, gamma, beta, pos) - ref).abs(), bound).max()) <= 1.0, R.gn_id(c)
        if r > worst:
            worst, at = r, R.gn_id(c)
        assert r <= 0.5, f"{R.gn_id(c)}: the fp32 restatement reaches {r:.3f} of the bound"
        for m in names:
            if m == "no_eps" and c["family"] != "near_constant":
                continue
            out, _ = R.gn_ref(c, x, gamma, beta, pos, mutant=m)
            keep(best, m, float(R.ratio((out - ref).abs(), bound).max()), R.gn_id(c))
    print(f"GroupNorm: restatement worst err / bound {worst:.3f} ({at})")
    report("GroupNorm", best)


# ------------------------------------------------------------------------------------------------ RMSNorm
def test_rmsnorm_reference_restatement_mutants_and_undecided_share():
    best = {m: (0.0, None) for m in ("no_mid_rounding", "mean_padded", "eps_outside")}
    worst, at, share = 0.0, None, 0.0
    for c in R.RMS_CASES:
        dt, M, H, eps = c
        x, w = R.rms_inputs(c)
        got = R.rms_restated(x, w, eps, dt)
        if dt == "fp32":
            ref, bound = R.rms_ref_fp32(x, w, eps)
            assert ((ref - R.rms_torch(x, w, eps)).abs() <= 1e-6 * bound).all(), R.rms_id(c)
            r = float(R.ratio((got - ref).abs(), bound).max())
            if r > worst:
                worst, at = r, R.rms_id(c)
            assert r <= 0.5, f"{R.rms_id(c)}: the fp32 restatement reaches {r:.3f} of the bound"
            for m in ("mean_padded", "eps_outside"):
                out, _ = R.rms_ref_fp32(x, w, eps, mutant=m)
                keep(best, m, float(R.ratio((out - ref).abs(), bound).max()), R.rms_id(c))
        else:
            cand = R.rms_candidates_bf16(x, w, eps)
            xd = x.double()
            nrm = R._rne_bf16_t(xd * torch.rsqrt(xd.pow(2).mean(-1, keepdim=True) + float(torch.tensor(eps, dtype=torch.float32))))
            centre = R._rne_bf16_t(w.double()[None] * nrm)
            assert (cand == centre[None]).any(0).all(), f"{R.rms_id(c)}: the candidates miss HF's own formulation in fp64"
            und, bad = R.rms_check_bf16(got, cand)
            share = max(share, und)
            assert und <= 0.01, f"{R.rms_id(c)}: {und:.2%} of the elements are undecided"
            assert bad == 0, f"{R.rms_id(c)}: the fp32 restatement stores {bad} values outside the candidates"
            for m in best:   # a decided element that differs is beyond any bound: the miss is infinite
                out = R.rms_candidates_bf16(x, w, eps, mutant=m)[0]
                keep(best, m, float("inf") if R.rms_check_bf16(out, cand)[1] else 0.0, R.rms_id(c))
        if M > 1:
            assert (x[1] == 0).all() and (got[1] == 0).all()
    print(f"RMSNorm fp32: restatement worst err / bound {worst:.3f} ({at}); bf16: largest undecided share {share:.2e}")
    report("RMSNorm", best)
