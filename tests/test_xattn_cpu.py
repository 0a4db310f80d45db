"""CPU self-check of tests/xattn_ref.py: the reference agrees with an independent torch einsum, an fp32 restatement of xattn_kernel
(tile order, online softmax, P rounded to bf16) stays within half the per-row bound on every case of the table, and every kernel
mutant misses the true reference by at least MARGIN x the bound on at least one case."""
import pytest
import torch

import xattn_ref as R

MARGIN = 10.0
MUTANTS = ("natural_order", "no_xor", "drop_last_tile", "no_alpha", "b_mod_F", "scale_C", "head_shift")
INST_IDS = [f"hd{C // nh}-C{C}-nh{nh}" for C, nh in R.INSTANCES]


def applies(mutant, C, nh):
    if mutant == "no_xor":
        return R.key_tile(C // nh) == 32          # the XOR exists only in the 32-key form
    if mutant in ("scale_C", "head_shift"):
        return nh > 1
    return True


@pytest.mark.parametrize("C,nh", R.INSTANCES, ids=INST_IDS)
def test_reference_agrees_with_einsum_and_bounds_the_fp32_restatement(C, nh):
    """every case of the instance: reference within 1e-6 x bound of torch.softmax over an einsum; the fp32 restatement within half
    the bound on every output row (before the bf16 store and without its term; within the whole bound after it: xattn_ref's docstring)
    -- a term missing from the bound shows up here, not on the GPU."""
    worst, at = 0.0, None
    for c in (c for c in R.CASES if c[:2] == (C, nh)):
        q, K, VT = R.make_inputs(c)
        F = c[5]
        ref, bound = R.xattn_ref(q, K, VT, F, nh)
        assert torch.isfinite(ref).all() and (bound > 0).all(), R.case_id(c)
        ind = R.row_error(R.xattn_einsum(q, K, VT, F, nh), ref, nh)
        assert (ind <= 1e-6 * bound).all(), f"{R.case_id(c)}: the reference disagrees with a plain fp64 einsum"
        ratio = float((R.row_error(R.xattn_restated(q, K, VT, F, nh, rounded=False), ref, nh)
                       / R.xattn_ref(q, K, VT, F, nh, out_term=False)[1]).max())
        assert (R.row_error(R.xattn_restated(q, K, VT, F, nh), ref, nh) <= bound).all(), R.case_id(c)
        if ratio > worst:
            worst, at = ratio, R.case_id(c)
        assert ratio <= 0.5, f"{R.case_id(c)}: the fp32 restatement reaches {ratio:.3f} of the bound"
    print(f"xattn hd {C // nh}: restatement worst err / bound {worst:.3f} ({at})")


@pytest.mark.parametrize("C,nh", R.INSTANCES, ids=INST_IDS)
def test_bound_rejects_kernel_mutants(C, nh):
    """needle, ramp and random cases of the instance: each mutant that applies to it is rejected by >= MARGIN x the bound somewhere."""
    best = {m: (0.0, None) for m in MUTANTS if applies(m, C, nh)}
    for c in (c for c in R.CASES if c[:2] == (C, nh) and c[6] in ("needle", "ramp_up", "ramp_down") and c[3] > 64):
        q, K, VT = R.make_inputs(c)
        F = c[5]
        ref, bound = R.xattn_ref(q, K, VT, F, nh)
        for m in best:
            if best[m][0] >= MARGIN:
                continue
            out, _ = R.xattn_ref(q, K, VT, F, nh, mutant=m)
            miss = float((R.row_error(out, ref, nh) / bound).max())
            if miss > best[m][0]:
                best[m] = (miss, R.case_id(c))
    for m, (miss, at) in best.items():
        print(f"xattn hd {C // nh} mutant {m}: rejected by {miss:.1f}x at {at}")
    weak = {m: round(v[0], 2) for m, v in best.items() if not v[0] >= MARGIN}
    assert not weak, f"mutants the bound does not reject by {MARGIN}x: {weak}"


def test_needles_cover_every_position_of_a_key_block():
    """the needle family reaches all 32 positions of a 32-key block in both halves of a 64-key tile, key 0, key kv - 1 and keys of
    the first and last tile -- for every case, over its query rows"""
    for c in (c for c in R.CASES if c[6] == "needle"):
        kv = c[3]
        got = set(R.needle_index(c).flatten().tolist())
        assert set(range(64)) <= got and set(range(kv - 64, kv)) <= got, R.case_id(c)
