"""The filtered-scores definition without a GPU (tests/filtered_scores_ref.py): the fp64 reference against HF's own warpers, the share of
rows the reference must skip, the restatement of the kernel's arithmetic against the reference on the whole case table, the mutants it
must expose, and the Python layer's NamedTuple."""
import numpy as np
import pytest
import torch

import filtered_scores_ref as R


@pytest.mark.parametrize("case", list(R.CASES))
def test_reference_skips_at_most_one_row_in_a_hundred(case):
    """The seeds of the case table: no case may lean on ``near`` (8 rows: none of them)."""
    c = R.build(case)
    assert c["near"].sum() * 100 <= len(c["near"]), f"{case}: {int(c['near'].sum())} of {len(c['near'])} rows near the nucleus boundary"


@pytest.mark.parametrize("case", [c for c in R.CASES if not R.CASES[c][4]])
def test_reference_against_hf_warpers(case):
    """TemperatureLogitsWarper -> TopKLogitsWarper -> TopPLogitsWarper -> log_softmax: logprob of the id, entropy and support, on every
    row that is not flagged ``near`` or ``tie`` (HF's unstable sort decides a tie group at the boundary; the engine keeps all of it).
    HF subtracts the maximum in fp64 where the definition, as the sampler, does in fp32: a logit moves by at most eps = 2^-24 times the
    largest |l_i - max| among the survivors, the logprob by at most 2 eps, the entropy by at most eps * sum p |log p + H|; 1e-12 on top
    for the fp64 sums."""
    c = R.build(case)
    top_k, top_p, temperature, _ = c["settings"]
    lp, ent, sup, filt = R.hf_scores(c["z"], c["tok"], top_k, top_p, temperature)
    with np.errstate(invalid="ignore"):
        spread = np.where(np.isfinite(filt), filt.max(-1, keepdims=True) - filt, 0.0).max(-1)
    eps, sens = 2.0 ** -24 * spread, R.entropy_sensitivity(filt)
    rows = [b for b in range(len(lp)) if not (c["near"][b] or c["tie"][b])]
    assert len(rows) >= 5, f"{case}: only {len(rows)} rows left to compare"
    for b in rows:
        want = c["want"][b]
        assert sup[b] == want[3], f"{case} row {R.ROW_KINDS[b]}: HF keeps {sup[b]} tokens, the reference {want[3]}"
        assert abs(ent[b] - want[1]) <= eps[b] * sens[b] + 1e-12, f"{case} row {R.ROW_KINDS[b]}: entropy {ent[b]!r} vs {want[1]!r}"
        if 0 <= c["tok"][b] < c["z"].shape[1]:
            assert R.within(lp[b], want[0], 2 * eps[b] + 1e-12), f"{case} row {R.ROW_KINDS[b]}: logprob {lp[b]!r} vs {want[0]!r}"


def test_reference_properties():
    for case in R.CASES:
        c = R.build(case)
        w, (top_k, top_p, temperature, greedy) = c["want"], c["settings"]
        V = c["z"].shape[1]
        assert (w[:, 2] <= 0).all() and (w[:, 3] >= 1).all() and (w[:, 1] >= -1e-12).all(), case
        assert (w[:, 1] <= np.log(w[:, 3]) + 1e-12).all(), f"{case}: an entropy above log(support)"
        assert np.isnan(w[7, 0]) and np.isfinite(w[7, 1:]).all(), f"{case}: the id outside [0, V)"
        assert np.isfinite(w[0, 0]) and np.isfinite(w[1, 0]), f"{case}: an id inside S with no finite logprob"
        if greedy or ((top_k <= 0 or top_k >= V) and top_p >= 1.0):
            assert (w[:, 2] == 0).all(), f"{case}: nothing is filtered, yet kept_logmass is not exactly 0"
            assert (w[:, 3] == np.isfinite(c["z"]).sum(-1)).all()
        if not greedy and top_p == 0.0:
            assert (w[[0, 1, 2, 3, 6, 7], 3] == 1).all() and w[4, 3] == V, f"{case}: top_p = 0 keeps the maxima alone (a constant row: all of it)"
        if c["kept"][2].sum() > c["survive"][2].sum():
            assert w[2, 0] == -np.inf, f"{case}: an id in K that top-p cut"
        if np.isfinite(c["z"][3]).sum() > c["kept"][3].sum():
            assert w[3, 0] == -np.inf, f"{case}: an id outside K"
        if V > 1:
            assert w[6, 0] == -np.inf, f"{case}: a -inf entry"
    # the rows the issue lists are really there: an id cut by top-p and an id outside K in the default-shaped cases
    for case in ("V16386_k100_p09_t07", "V257_k100_p09", "V18432_k300_p09"):
        c = R.build(case)
        assert c["kept"][2].sum() > c["survive"][2].sum() and np.isfinite(c["z"][3]).sum() > c["kept"][3].sum(), case
        assert c["kept"][5].sum() > c["settings"][0], f"{case}: the tie group does not straddle the top-k threshold"
    z, tok, s = R.nonfinite_case()
    assert np.isnan(R.reference(z, tok, *s)[0]).all()
    z, tok, s = R.merge_case()
    assert R.reference(z, tok, *s)[0][0, 3] == 101, "the tempered row ties at the top-k threshold: 101 kept"


def test_filtered_plus_kept_mass_is_the_tempered_raw_logprob():
    """p_raw(tok) = p_filtered(tok) * (share of the mass that survived): in logarithms the SUM of the two outputs."""
    for case in ("V16386_k100_p09_t07", "V9216_k0_p09_t07", "V1030_k300_t2"):
        c = R.build(case)
        _, _, temperature, _ = c["settings"]
        l = (torch.from_numpy(np.array(c["z"])) / torch.tensor(temperature, dtype=torch.float32)).double()
        raw = torch.log_softmax(l, -1).numpy()
        for b in (0, 1):   # (ids inside S)
            assert abs(c["want"][b, 0] + c["want"][b, 2] - raw[b, c["tok"][b]]) <= 1e-6, (case, b)   # (fp32 subtraction of the maximum)


@pytest.mark.parametrize("case", list(R.CASES))
def test_kernel_arithmetic_against_the_reference(case):
    c = R.build(case)
    got = R.kernel_rows(c["z"], c["tok"], c["settings"]).astype(np.float64)
    ok = R.agrees(got, c["want"], c["near"])
    fin = np.isfinite(c["want"][:, :3])
    print(f"{case}: worst |restatement - fp64| = {np.abs(got[:, :3][fin] - c['want'][:, :3][fin]).max():.2e}")
    for b in range(len(ok)):
        assert ok[b], f"{case} row {R.ROW_KINDS[b]}: {got[b]} against fp64 {c['want'][b]}"


def test_kernel_arithmetic_special_rows():
    z, tok, s = R.nonfinite_case()
    assert np.isnan(R.kernel_rows(z, tok, s)).all()
    z, tok, s = R.merge_case()
    want, near, *_ = R.reference(z, tok, *s)
    assert R.agrees(R.kernel_rows(z, tok, s).astype(np.float64), want, near).all()


# mutant -> the case (or special row) that must expose it
EXPOSED_BY = {
    "ties at the top-k threshold dropped": "V257_k100_p09",
    "temperature applied after top-k": "merge",
    "entropy over K instead of S": "V16386_k100_p09_t07",
    "the maximum not forced to survive": "V1030_k100_p0",
    "kept_logmass normalised by K": "V16386_defaults",
}


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_mutants_fail(mutant):
    where = EXPOSED_BY[mutant]
    if where == "merge":
        z, tok, s = R.merge_case()
        want, near, *_ = R.reference(z, tok, *s)
    else:
        c = R.build(where)
        z, tok, s, want, near = c["z"], c["tok"], c["settings"], c["want"], c["near"]
    assert R.agrees(R.kernel_rows(z, tok, s).astype(np.float64), want, near).all(), "the unmutated restatement must pass here"
    bad = ~R.agrees(R.kernel_rows(z, tok, s, mutant=mutant).astype(np.float64), want, near)
    print(f"{mutant}: {int(bad.sum())} of {len(bad)} rows of {where} fail")
    assert bad.any(), f"the check does not see '{mutant}'"


def test_namedtuple_and_per_frame():
    from ivideogpt_amd import FilteredTokenScores, TokenScores, _lib
    from ivideogpt_amd.engine import _FILTERED_ENTRY, rollout_entry
    assert FilteredTokenScores._fields == R.FIELDS
    # every entry a call with the output can reach has its sibling, and the library exports it
    for kw in (dict(), dict(fanout=True), dict(group_size=2), dict(reuse_kv=True, actions=True), dict(force_sdf=True), dict(frame_outputs=True, actions=True)):
        assert _FILTERED_ENTRY[rollout_entry(token_scores=True, **kw)] in _lib.EXPORTS, kw
    lib = _lib.load()
    assert lib.ivg_debug_counter(b"filtered_scores") >= 0 and lib.ivg_generate_embeds_filtered and lib.ivg_op_filtered_scores
    g = torch.Generator().manual_seed(3)
    x = [torch.randn(2, 50, generator=g) for _ in range(4)]
    fs = FilteredTokenScores(*x)
    lp, en = fs.per_frame()
    want = TokenScores(x[0], x[1], x[2]).per_frame()
    assert lp.shape == (2, 3) and torch.equal(lp, want[0]) and torch.equal(en, want[1])
    with pytest.raises(ValueError):
        FilteredTokenScores(*(t[:, :10] for t in x)).per_frame()
