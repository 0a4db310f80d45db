"""Scores of sampled tokens under the distribution they were drawn from (include/ivg.h ivg_generate_filtered; filtered_scores_kernel)
restated in fp64 for tests/test_filtered_scores_cpu.py and tests/test_gpu_filtered_scores.py: the reference, HF's own warpers as the
outside oracle, the case table of the kernel hook, a restatement of the kernel's arithmetic (fp32 rows, fp64 sums in the kernel's
order) and the mutants the CPU test must see fail.  No GPU import.

Definition: ``l = z / temperature`` (fp32); K the top-k kept set (ties at the threshold kept, -inf never; ``top_k <= 0`` or ``>= V``:
every finite entry); S the survivors of the nucleus filter over K (tests/top_p_ref.py ``nucleus``); with ``e_i = exp(l_i - max)``:
``filtered_logprob = (l_tok - max) - log sum_S e`` (-inf outside S), ``filtered_entropy`` of ``e / sum_S e`` over S,
``kept_logmass = log sum_S e - log sum_finite e``, ``support = |S|``.  Greedy: no filter, no temperature.  NaN in all four for a row
that holds a NaN or whose maximum is not finite; a NaN logprob for an id outside [0, V); forced columns exactly 0.

The reference calls ``nucleus(..., tol=1e-9)``: two fp64 summation orders over at most 18,432 terms differ by under 2.1e-12 relative
(n * 2^-53 for n terms of one sign), so a survivor decision farther than 1e-9 from its boundary is the same in every order, with three
orders of magnitude to spare.  The default 1e-5 would flag a large share of full-vocabulary rows (18,432 cumulative masses on [0, 1])."""
import numpy as np
import torch

from token_scores_ref import BOUND, entropy_sensitivity, within  # noqa: F401  (the project's bar for these quantities: 1e-4 absolute)
from top_p_ref import _scaled, nucleus

TOL = 1e-9
PER = 17
FIELDS = ("logprob", "entropy", "kept_logmass", "support")


def _settings(top_k, top_p, temperature, greedy, V):
    if greedy:
        return 0, None, 1.0
    return (0 if (top_k is None or top_k <= 0 or top_k >= V) else int(top_k)), top_p, temperature


def reference(z, tok, top_k, top_p, temperature=1.0, greedy=False, tol=TOL):
    """fp64 scores of rows ``z (B, V)`` float32 at ids ``tok (B)`` -> (out (B, 4) float64, near (B) bool, tie (B) bool, survive (B, V),
    kept (B, V)): ``near`` / ``tie`` as ``nucleus`` reports them at ``tol``."""
    z = torch.from_numpy(np.array(z, dtype=np.float32))
    tok = np.asarray(tok, dtype=np.int64)
    B, V = z.shape
    top_k, top_p, temperature = _settings(top_k, top_p, temperature, greedy, V)
    bad = torch.isnan(z).any(-1) | ~torch.isfinite(_scaled(z, temperature).max(-1).values)
    safe = torch.where(bad[:, None], torch.zeros_like(z), z)   # (a stand-in row: its outputs are overwritten with NaN)
    survive, e, near, tie = nucleus(safe, top_k, top_p, temperature, tol=tol)
    l = _scaled(safe, temperature)
    m = l.max(-1, keepdim=True).values
    d = (l - m).double()                                        # the subtraction in fp32, as the sampler's
    ea = torch.where(l > float("-inf"), torch.exp(d), torch.zeros((), dtype=torch.double))
    w = torch.where(survive, e, torch.zeros((), dtype=torch.double))
    s = w.sum(-1)
    ls = torch.log(s)
    ent = ls - torch.where(w > 0, w * d, torch.zeros((), dtype=torch.double)).sum(-1) / s
    out = np.full((B, 4), np.nan)
    out[:, 1], out[:, 2], out[:, 3] = ent.numpy(), (ls - torch.log(ea.sum(-1))).numpy(), survive.sum(-1).numpy()
    for b in range(B):
        if 0 <= tok[b] < V:
            out[b, 0] = float(d[b, tok[b]] - ls[b]) if bool(survive[b, tok[b]]) else -np.inf
    out[bad.numpy()] = np.nan
    kept = e > 0
    return out, (near & ~bad).numpy(), (tie & ~bad).numpy(), survive.numpy(), kept.numpy()


def reference_columns(rows, toks, top_k, top_p, temperature=1.0, greedy=False, forced_period=0):
    """One trajectory's ``n`` new tokens: ``rows (n, V)`` the row read for new token j = 1 .. n, ``toks (n)`` -> ((n, 4) with the forced
    columns zero, near (n))."""
    out, near, _, _, _ = reference(rows, toks, top_k, top_p, temperature, greedy)
    if forced_period:
        for j in range(1, len(toks) + 1):
            if j % forced_period == 0:
                out[j - 1], near[j - 1] = 0.0, False
    return out, near


def hf_scores(z, tok, top_k, top_p, temperature=1.0):
    """HF's own warpers in the order generate builds them -- TemperatureLogitsWarper (fp32) -> TopKLogitsWarper -> TopPLogitsWarper --
    then log_softmax; the two filters and the softmax run on the fp64 copy of the tempered row, so that HF's cumulative sums are as
    exact as the reference's.  -> (logprob (B) of ``tok``, entropy (B), support (B), the filtered rows (B, V) float64)."""
    from transformers.generation.logits_process import TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper
    s = torch.from_numpy(np.array(z, dtype=np.float32))
    V = s.shape[1]
    if temperature != 1.0:
        s = TemperatureLogitsWarper(float(temperature))(None, s)
    assert s.dtype == torch.float32
    s = s.double()
    if top_k is not None and 0 < top_k < V:
        s = TopKLogitsWarper(int(top_k))(None, s)
    if top_p is not None and top_p < 1.0:
        s = TopPLogitsWarper(float(np.float32(top_p)))(None, s)
    logp = torch.log_softmax(s, -1)
    p = logp.exp()
    ent = -torch.where(p > 0, p * logp, torch.zeros((), dtype=torch.double)).sum(-1)
    tok = torch.from_numpy(np.array(tok, dtype=np.int64)).clamp(0, V - 1)
    return logp.gather(1, tok[:, None])[:, 0].numpy(), ent.numpy(), (s > float("-inf")).sum(-1).numpy(), s.numpy()


# ------------------------------------------------------------------------------------------------ the case table
# name -> (V, top_k, top_p, temperature, greedy, seed).  V: one entry; fewer than a wave; one past a sweep of the workgroup; no multiple of
# anything; the limit of the 36-per-thread instance and one past it; the model's vocabulary; the limit 256 * 72.  top_k: 0 (all), 1, the
# default 100, 300 (beyond the sampler's pre-filter), >= V.  top_p: 1 (none), 0.9, 1e-6 and 0 (the maximum alone).  Seeds: any for which
# the reference flags no row ``near`` (the CPU test asserts it).
CASES = {
    "V1": (1, 100, 0.9, 1.0, False, 1),
    "V5_k1_t07": (5, 1, 1.0, 0.7, False, 2),
    "V5_k0_p09": (5, 0, 0.9, 1.0, False, 3),
    "V257_k100_p09": (257, 100, 0.9, 1.0, False, 4),
    "V1030_k300_t2": (1030, 300, 1.0, 2.0, False, 5),
    "V1030_k100_p0": (1030, 100, 0.0, 1.0, False, 6),
    "V9216_k0_p09_t07": (9216, 0, 0.9, 0.7, False, 7),        # the whole vocabulary kept, then the nucleus: far beyond the sampler's list cap
    "V9217_k100_p1e-6": (9217, 100, 1e-6, 1.0, False, 8),
    "V9217_k1_p09_t2": (9217, 1, 0.9, 2.0, False, 9),
    "V16386_defaults": (16386, 100, 1.0, 1.0, False, 10),      # what every caller of the reference passes
    "V16386_k100_p09_t07": (16386, 100, 0.9, 0.7, False, 11),
    "V16386_k300_p0_t2": (16386, 300, 0.0, 2.0, False, 12),
    "V16386_kV_p09": (16386, 16386, 0.9, 1.0, False, 13),
    "V16386_unfiltered": (16386, 0, 1.0, 1.0, False, 14),      # nothing filtered: kept_logmass exactly 0
    "V16386_greedy": (16386, 100, 0.9, 0.7, True, 15),         # greedy ignores all three settings
    "V18432_k0_p09_t2": (18432, 0, 0.9, 2.0, False, 16),
    "V18432_k20000_p1e-6_t07": (18432, 20000, 1e-6, 0.7, False, 17),
    "V18432_k300_p09": (18432, 300, 0.9, 1.0, False, 18),
    "V1030_greedy": (1030, 0, 1.0, 1.0, True, 19),
}
ROW_KINDS = ("inside_S", "argmax", "cut_by_top_p", "outside_K", "all_equal", "ties_straddle_top_k", "third_minf", "id_out_of_range")
_BUILT = {}


def _rows(V, top_k, seed):
    rng = np.random.default_rng(1000 + seed)
    z = np.empty((len(ROW_KINDS), V), dtype=np.float32)
    z[0] = rng.normal(0, 2.0, V)
    z[1] = rng.normal(0, 1.0, V)
    z[2] = rng.normal(0, 4.0, V)
    z[3] = rng.normal(0, 2.0, V)
    z[4] = np.float32(rng.normal(0, 3) + 0.5)
    z[5] = rng.normal(0, 2.0, V)
    k = top_k if 0 < top_k < V else max(1, V // 2)
    kth = np.sort(z[5])[-k]
    z[5, rng.choice(V, min(V, 7), replace=False)] = kth         # a tie group of up to 8 at the k-th largest value: it straddles the threshold
    z[6] = rng.normal(0, 2.0, V)
    if V > 1:
        z[6, 1::3] = -np.inf
    z[7] = rng.normal(0, 2.0, V)
    return z


def build(name):
    """-> dict(z (8, V) float32, tok (8) int64, want (8, 4) float64, near, tie, survive, kept, settings): the rows of ROW_KINDS, the id of
    each chosen from the reference's own sets -- inside S (its lightest member), the arg-max, in K but cut by top-p, outside K, the last
    id of a constant row, a member of the tie group, a -inf entry, an id outside [0, V).  Where a set is empty (nothing cut, nothing
    outside K) the id falls back to the arg-max.  Computed once, shared, read-only."""
    if name not in _BUILT:
        V, top_k, top_p, temperature, greedy, seed = CASES[name]
        z = _rows(V, top_k, seed)
        _, _, _, survive, kept = reference(z, np.zeros(len(z), dtype=np.int64), top_k, top_p, temperature, greedy)
        amax = z.argmax(-1)
        tok = amax.copy()
        order = np.argsort(z, -1, kind="stable")
        tok[0] = next(i for i in order[0] if survive[0, i])
        cut = kept[2] & ~survive[2]
        if cut.any():
            tok[2] = np.flatnonzero(cut)[-1]
        out = np.isfinite(z[3]) & ~kept[3]
        if out.any():
            tok[3] = np.flatnonzero(out)[0]
        tok[4] = V - 1
        tok[5] = np.flatnonzero(z[5] == np.sort(z[5])[-(top_k if 0 < top_k < V else max(1, V // 2))])[0]
        if V > 1:
            tok[6] = 1
        tok[7] = V if seed % 2 else -1
        want, near, tie, survive, kept = reference(z, tok, top_k, top_p, temperature, greedy)
        d = dict(z=z, tok=tok, want=want, near=near, tie=tie, survive=survive, kept=kept, settings=(top_k, top_p, temperature, greedy))
        for a in d.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _BUILT[name] = d
    return _BUILT[name]


def nonfinite_case():
    """V = 1001 under top_k 100, top_p 0.9, temperature 0.7: a NaN among finite entries, a row of NaN, a +inf, all -inf -> NaN in all four."""
    rng = np.random.default_rng(7)
    z = rng.normal(0, 1, (4, 1001)).astype(np.float32)
    z[0, 500] = np.nan
    z[1] = np.nan
    z[2, 17] = np.inf
    z[3] = -np.inf
    return z, np.array([3, 0, 17, 0], dtype=np.int64), (100, 0.9, 0.7, False)


def merge_case():
    """The row that tells temperature-before-top-k from temperature-after: V = 257, top_k 100, temperature 0.7.  Its 100th and 101st
    largest raw values are neighbouring floats in [0.7, 1) whose quotients by 0.7f round to the SAME float (the quotients' binade
    [1, 1.43) holds fewer floats than [0.7, 1)): the tempered row has a tie at the top-k threshold, which is kept -- 101 survivors --
    where a filter on the raw row keeps 100."""
    t = np.float32(0.7)
    x = np.float32(0.8)
    while np.float32(x / t) != np.float32(np.nextafter(x, np.float32(1)) / t):
        x = np.nextafter(x, np.float32(1))
    rng = np.random.default_rng(3)
    z = np.concatenate([rng.uniform(1.5, 5, 99), [np.nextafter(x, np.float32(1)), x], rng.uniform(-5, 0.5, 156)]).astype(np.float32)
    z = z[rng.permutation(257)][None]
    return z, np.array([int(z[0].argmax())], dtype=np.int64), (100, 1.0, 0.7, False)


# ------------------------------------------------------------------------------------------------ the kernel's arithmetic
def _f2key(x):
    u = np.asarray(x, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def _block_sum(x):
    """(slots, 256) -> the kernel's fp64 block sum: per thread over its slots in ascending order, the xor butterfly inside each wave of
    64, then the four waves in order."""
    t = np.zeros(256)
    for q in range(x.shape[0]):
        t = t + x[q]
    w = t.reshape(4, 64)
    for o in (32, 16, 8, 4, 2, 1):
        w = w + w[:, np.arange(64) ^ o]
    return ((w[0, 0] + w[1, 0]) + w[2, 0]) + w[3, 0]


MUTANTS = ("ties at the top-k threshold dropped", "temperature applied after top-k", "entropy over K instead of S",
           "the maximum not forced to survive", "kept_logmass normalised by K")


def kernel_row(z, tok, top_k, top_p, temperature=1.0, greedy=False, mutant=None):
    """One row through filtered_scores_kernel's arithmetic -> 4 float32: fp32 row, keys, thresholds, fp64 exponentials and sums with
    element i in slot i / 256 of thread i % 256.  The thresholds are found among the row's own values (the kernel bisects the key space
    for the same two numbers).  ``mutant``: one of MUTANTS."""
    assert mutant is None or mutant in MUTANTS
    z = np.asarray(z, dtype=np.float32)
    V = z.shape[0]
    scale = (not greedy) and temperature != 1.0
    with np.errstate(all="ignore"):
        l = (z / np.float32(temperature)).astype(np.float32) if scale else z
        if np.isnan(l).any() or not np.isfinite(l.max()):
            return np.full(4, np.nan, dtype=np.float32)
        mx = l.max()
        slots = -(-V // 256)
        pad = np.full(slots * 256, -np.inf, dtype=np.float32)
        pad[:V] = l
        valid = (np.arange(slots * 256) < V).reshape(slots, 256)
        lt = pad.reshape(slots, 256)
        key = _f2key(lt)
        kept = valid & (lt > -np.inf)
        if not greedy and 0 < top_k < V:
            if mutant == "temperature applied after top-k":
                rkey = _f2key(z)
                thr = np.sort(rkey)[-top_k]
                rk = np.zeros(slots * 256, dtype=np.uint32)
                rk[:V] = rkey
                kept &= rk.reshape(slots, 256) >= thr
            elif mutant == "ties at the top-k threshold dropped":
                keep = np.argsort(-_f2key(l).astype(np.int64), kind="stable")[:top_k]
                only = np.zeros(slots * 256, dtype=bool)
                only[keep] = True
                kept &= only.reshape(slots, 256)
            else:
                kept &= key >= np.sort(_f2key(l))[-top_k]
        ea = np.where(lt > -np.inf, np.exp((lt - mx).astype(np.float32).astype(np.float64)), 0.0)
        total = _block_sum(ea)
        e = np.where(kept, ea, 0.0)
        v = np.where(kept, lt, np.float32(-np.inf))
        tau = np.float32(-np.inf)
        if not greedy and top_p is not None and top_p < 1.0:
            Z = _block_sum(e)
            cut = (1.0 - float(np.float32(top_p))) * Z
            G = lambda c: _block_sum(np.where(v <= c, e, 0.0))
            cand = np.unique(v[kept])
            if not Z > cut:
                tau = np.float32(np.inf) if mutant == "the maximum not forced to survive" else mx
            else:
                lo, hi = 0, len(cand) - 1                        # G(cand[hi]) = Z > cut
                while lo < hi:
                    mid = (lo + hi) // 2
                    if G(cand[mid]) > cut:
                        hi = mid
                    else:
                        lo = mid + 1
                tau = cand[lo]
        S = (v > -np.inf) & (v >= tau)
        H = kept if mutant == "entropy over K instead of S" else S
        s = _block_sum(np.where(S, e, 0.0))
        sh = _block_sum(np.where(H, e, 0.0))
        t = _block_sum(np.where(H & (e > 0), e * (v - mx).astype(np.float32).astype(np.float64), 0.0))
        ls = np.log(s)
        lp = np.nan
        if 0 <= tok < V:
            i = int(tok)
            lp = (np.float64(np.float32(l[i] - mx)) - ls) if S[i // 256, i % 256] else -np.inf
        norm = _block_sum(e) if mutant == "kept_logmass normalised by K" else total
        return np.array([lp, np.log(sh) - t / sh, ls - np.log(norm), S.sum()], dtype=np.float32)


def kernel_rows(z, tok, settings, mutant=None):
    return np.stack([kernel_row(z[b], int(tok[b]), *settings, mutant=mutant) for b in range(len(z))])


def agrees(got, want, near):
    """(B) bool: per row not flagged ``near``, ``support`` exactly the reference's, the three real outputs within BOUND, NaN and
    infinities alike in kind; a ``near`` row agrees by definition."""
    ok = within(got[:, :3], want[:, :3]).all(-1)
    with np.errstate(invalid="ignore"):
        sup = np.where(np.isnan(want[:, 3]), np.isnan(got[:, 3]), got[:, 3] == want[:, 3])
    return near | (ok & sup)
