"""ivg_kv_extend / ivg_generate_fanout without a GPU: the reference and bound of tests/chunk_attn_ref.py reject the ways
chunk_attn_kernel could be wrong and accept its arithmetic restated in fp32, and the argument checks of the new entries that run
before any launch."""
import ctypes as C

import pytest
import torch

import chunk_attn_ref as R

INVALID = -1


@pytest.mark.parametrize("pos0,T", R.CASES, ids=[f"pos{p}-T{t}" for p, t in R.CASES])
def test_needle_plan_makes_the_edge_keys_decisive(pos0, T):
    """Every wanted key carries a needle in some (trajectory, head) pair of the smallest case the GPU test runs (B = 3, 2 heads), on a
    row that sees it -- except the keys just past a diagonal, which sit on the row that must NOT see them."""
    pairs, last = R.needle_plan(pos0, T, 6)
    keys = {k for p in pairs for _, k in p}
    nk = pos0 + T
    want = {0, pos0, last} | {s for s in range(0, nk, 32)} | {min(s + 31, nk - 1) for s in range(0, nk, 32)} | ({pos0 - 1} if pos0 else set())
    assert want <= keys, f"keys without a needle: {sorted(want - keys)}"
    for p in pairs:
        assert len({t for t, _ in p}) == len(p) and len({k for _, k in p}) == len(p)
        assert all(0 <= t < T and 0 <= k <= pos0 + t + 1 for t, k in p)
    if T > 1:
        assert any(k == pos0 + t + 1 for p in pairs for t, k in p), "no masked needle"
    assert any(k == pos0 + t for p in pairs for t, k in p), "no diagonal needle"


@pytest.mark.parametrize("pos0,T", R.CASES, ids=[f"pos{p}-T{t}" for p, t in R.CASES])
def test_bound_rejects_mutants_and_accepts_the_kernels_arithmetic(pos0, T):
    """With the GPU test's needle inputs and bound, each wrong attention misses the fp64 reference by at least 10x the bound on some
    row: the mask shifted by +1 and by -1, key pos0 - 1 dropped, the chunk's keys roped at t instead of pos0 + t, V read in the P.V
    product's own key order (or its inverse) within a 32-key block.  The fp32 restatement of the kernel (wave split, online softmax,
    bf16 P, merge, bf16 output) stays within the bound on every row, for needle and random inputs."""
    B, heads = 3, 2
    for family in ("needle", "random"):
        inp = R.chunk_inputs(family, B, heads, pos0, T, seed=1000 * pos0 + T)
        ref, tol = R.attention_fp64(inp, B, heads, pos0, T)
        got = R.kernel_arithmetic_fp32(inp, B, heads, pos0, T).double()
        ratio = ((got - ref).abs().amax(-1) / tol).max().item()
        print(f"pos0={pos0} T={T} {family}: fp32 restatement err / bound {ratio:.3f}")
        assert torch.isfinite(got).all() and ratio <= 1, f"{family}: the kernel's own arithmetic misses the bound ({ratio:.3f})"
    perm = R.mfma_key_perm()
    mutants = {"mask -1": dict(shift=-1), "V in MFMA key order": dict(v_perm=perm), "V order undone": dict(v_perm=torch.argsort(perm))}
    if T > 1:
        mutants["mask +1"] = dict(shift=1)      # (T = 1: the only row's next key does not exist)
    if pos0 >= 1:
        mutants[f"key {pos0 - 1} dropped"] = dict(drop=pos0 - 1)
    if pos0 >= 63:   # (at pos0 = 1 the two rotations are one step apart and only the fastest frequencies tell them apart)
        mutants["chunk keys roped at t"] = dict(rope_pos0=0)
    if pos0 + T < 32:
        mutants = {k: v for k, v in mutants.items() if not k.startswith("V ")}   # (no whole 32-key block to permute)
    needle = R.chunk_inputs("needle", B, heads, pos0, T, seed=1000 * pos0 + T)
    ref, tol = R.attention_fp64(needle, B, heads, pos0, T)
    for name, kw in mutants.items():
        mut, _ = R.attention_fp64(needle, B, heads, pos0, T, **kw)
        miss = torch.nan_to_num((mut - ref).abs().amax(-1), nan=float("inf")) / tol   # (mask -1 at pos0 = 0 leaves row 0 empty: NaN is a miss)
        assert miss.max().item() >= 10, f"{name}: misses the reference by only {miss.max().item():.2f}x the bound"


def test_chunk_attn_hook_refuses_what_it_does_not_cover():
    """argument checks of ivg_op_chunk_attn that run before any launch: anything but bf16 at head_dim 64, pos0 < 0, T < 1,
    pos0 + T > Lmax, B or heads <= 0, a misaligned qkv or out."""
    from ivideogpt_amd import _lib
    f = _lib.load().ivg_op_chunk_attn
    x = C.c_void_p(64)
    # (B, T, heads, hd, Lmax, pos0, dtype)
    for args in ((1, 4, 2, 64, 100, 10, 0), (1, 4, 2, 64, 100, 10, 2), (1, 4, 2, 32, 100, 10, 1), (1, 4, 2, 128, 100, 10, 1), (1, 4, 2, 64, 100, -1, 1),
                 (1, 0, 2, 64, 100, 10, 1), (1, 4, 2, 64, 100, 97, 1), (1, 1, 2, 64, 100, 100, 1), (0, 4, 2, 64, 100, 10, 1), (1, 4, 0, 64, 100, 10, 1)):
        assert f(x, x, x, x, None, None, *args, None) == INVALID, args
    assert f(C.c_void_p(72), x, x, x, None, None, 1, 4, 2, 64, 100, 10, 1, None) == INVALID     # qkv not 16-byte aligned
    assert f(x, x, x, C.c_void_p(68), None, None, 1, 4, 2, 64, 100, 10, 1, None) == INVALID     # out not 8-byte aligned


def test_new_entries_refuse_a_null_engine():
    from ivideogpt_amd import _lib
    lib = _lib.load()
    x = C.c_void_p(64)
    assert lib.ivg_kv_extend(None, x, 548, 3, 530, 548, None, 0, 2, None, None) == INVALID
    assert lib.ivg_generate_fanout(None, x, 514, 3, 2, 514, 17, None, 0, 2, None, 100, 1, x, None, None, None, None) == INVALID
    assert lib.ivg_debug_counter(b"kv_extend_chunk_rows") >= 0 and lib.ivg_debug_counter(b"kv_extend_step_rows") >= 0
