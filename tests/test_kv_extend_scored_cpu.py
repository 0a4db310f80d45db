"""ivg_kv_extend_scored without a GPU: the frame window ``extend_frames`` against a walk over the fed positions, the declarations of
the two new entries, the argument checks that run before any launch, and the forced-column rule of token_scores_rows_kernel restated
in fp32 against the ``forced_period`` rule of tests/token_scores_ref.py for a call aligned like a rollout."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import token_scores_ref as TS
from frame_heads_ref import frame_positions

INVALID = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def frames_by_walking(keep, L0, ctx):
    """The frames whose 16th token is among the fed positions [keep, L0 - 1), by looking at every position."""
    q = frame_positions(ctx, 8)
    hits = [q.index(p) for p in range(keep, L0 - 1) if p in q]
    assert hits == list(range(hits[0], hits[0] + len(hits))) if hits else True
    return hits


@pytest.mark.parametrize("ctx", [1, 2])
def test_extend_frames_against_a_walk_over_the_positions(ctx):
    from ivideogpt_amd.transformer import extend_frames
    for keep in range(257 * ctx - 1, 257 * ctx + 41):
        for last in range(keep, keep + 41):          # last = L0 - 1
            hits = frames_by_walking(keep, last + 1, ctx)
            i_first, F = extend_frames(keep, last + 1, ctx)
            assert F == len(hits), f"keep {keep}, L0 {last + 1}: F_out {F}, the walk finds {len(hits)}"
            if hits:
                assert i_first == hits[0], f"keep {keep}, L0 {last + 1}: i_first {i_first}, the walk starts at {hits[0]}"


@pytest.mark.parametrize("ctx", [1, 2])
def test_extend_frames_named_edges(ctx):
    from ivideogpt_amd.transformer import extend_frames
    q = frame_positions(ctx, 4)
    assert extend_frames(q[1], q[1] + 2, ctx) == (1, 1), "keep == q_i: the first fed token is frame i's 16th"
    assert extend_frames(q[1] + 1, q[2] + 2, ctx) == (2, 1), "keep == q_i + 1: frame i was fed before this call"
    assert extend_frames(q[0] - 3, q[1] + 2, ctx) == (0, 2), "L0 - 2 == q_i: the last fed token is frame i's 16th"
    assert extend_frames(q[0] - 3, q[1] + 1, ctx) == (0, 1), "L0 - 2 == q_i - 1: the call ends one short of frame i"
    assert extend_frames(q[0] + 1, q[1] + 1, ctx)[1] == 0
    assert extend_frames(q[0], q[0] + 1, ctx)[1] == 0, "a rewind feeds nothing"
    assert extend_frames(5, 100, ctx) == (0, 0), "inside the context"


def test_both_entries_are_declared_and_listed():
    from ivideogpt_amd import _lib
    with open(os.path.join(ROOT, "include", "ivg.h")) as f:
        header = f.read()
    for name, n_args in (("ivg_kv_extend_scored", 14), ("ivg_op_token_scores_rows", 12)):
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert m, f"{name} is not declared in include/ivg.h"
        args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        assert len(args.split(",")) == n_args, f"{name}: {len(args.split(','))} parameters in the header"
        assert name in _lib.EXPORTS and len(_lib.EXPORTS[name][1]) == n_args, f"{name}: _lib lists another signature"
        assert getattr(_lib.load(), name) is not None


def test_new_entries_refuse_before_any_launch():
    from ivideogpt_amd import _lib
    lib = _lib.load()
    x = C.c_void_p(64)
    assert lib.ivg_kv_extend_scored(None, x, 548, 3, 530, 548, None, 0, 2, None, x, x, x, None) == INVALID
    assert lib.ivg_kv_extend_scored(None, x, 548, 3, 530, 548, None, 0, 2, None, None, None, None, None) == INVALID
    assert lib.ivg_debug_counter(b"kv_extend_frame_rows") >= 0 and lib.ivg_debug_counter(b"kv_extend_scored_rows") >= 0
    f = lib.ivg_op_token_scores_rows
    # (logits, ids, ids_stride, row0, rows, Tc, V, first_forced, period, out, out_ld)
    good = (x, x, 3, 0, 4, 3, 130, 0, 0, x, 3)
    for k, bad in ((0, None), (1, None), (9, None), (3, -1), (4, 0), (5, 0), (6, 0), (6, 256 * 72 + 1), (7, -1), (8, -1)):
        args = list(good)
        args[k] = bad
        assert f(*args, None) == INVALID, f"argument {k} = {bad}"


def forced_rule(keep, ctx, actions=True):
    """(first_forced, period) as the engine passes them to token_scores_rows_kernel: column c scores the token at position
    keep + c + 1, forced when that position is an sdf slot 257 ctx - 1 + 17 i."""
    d = keep + 1 - (257 * ctx - 1)
    return (-d if d <= 0 else (17 - d % 17) % 17), (17 if actions else 0)


def rows_columns(rows, toks, first_forced, period):
    """token_scores_rows_kernel's column loop around the row arithmetic of tests/token_scores_ref.py (fp32)."""
    out = np.full((len(toks), 3), -777.25, dtype=np.float32)
    for c in range(len(toks)):
        if period > 0 and c >= first_forced and (c - first_forced) % period == 0:
            out[c] = 0.0
        else:
            out[c] = TS.kernel_fp32(rows[c], int(toks[c]))
    return out


@pytest.mark.parametrize("ctx,t", [(1, 0), (2, 0), (2, 3)])
def test_forced_columns_are_the_rollouts(ctx, t):
    """A call aligned like a rollout -- keep = L0' - 1 with L0' = 257 ctx + 17 t, so that column c is the rollout's new token c + 1 --
    scores and zeroes the columns ``kernel_columns`` does under forced_period = 17; and the rule by definition for every alignment."""
    rows, toks = TS.column_case()
    keep = 257 * ctx + 17 * t - 1
    first, period = forced_rule(keep, ctx)
    assert (first, period) == (16, 17)
    got, want = rows_columns(rows, toks, first, period), TS.kernel_columns(rows, toks, forced_period=17)
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    assert (got[16] == 0).all() and (got[15] != 0).all() and (got[17] != 0).all()
    for name, kw in TS.COLUMN_MUTANTS.items():
        assert not np.array_equal(got, TS.kernel_columns(rows, toks, forced_period=17, **kw)), f"the comparison does not see: {name}"
    assert np.array_equal(rows_columns(rows, toks, *forced_rule(keep, ctx, actions=False)), TS.kernel_columns(rows, toks, forced_period=0))
    for keep in range(1, 257 * ctx + 60):
        first, period = forced_rule(keep, ctx)
        slots = [c for c in range(80) if keep + c + 1 >= 257 * ctx - 1 and (keep + c + 1 - (257 * ctx - 1)) % 17 == 0]
        assert [c for c in range(80) if c >= first and (c - first) % period == 0] == slots, f"keep {keep}"
