"""Token log-probabilities and predictive entropy of a rollout (include/ivg.h ivg_generate_scored; token_scores_kernel) restated in
fp64 for tests/test_token_scores_cpu.py and tests/test_gpu_token_scores.py, the case table of the kernel hook, an fp32 restatement of
the kernel's reduction, and the mutants the CPU test must see fail.  No GPU import.

Definition: for the fp32 logits row ``z`` the sampler read (raw: before temperature, top-k, top-p) and the id ``tok`` it wrote,
``logprob = z[tok] - logsumexp(z)``, ``entropy = -sum p log p`` with ``p = softmax(z)`` and 0 for ``p = 0``,
``max_logprob = max(z) - logsumexp(z)``; natural logarithms; NaN in all three when the row's maximum is not finite; forced columns
(new token j with j % 17 == 0 under the forced schedule) are exactly 0."""
import numpy as np

BOUND = 1e-4   # absolute, per output: the bar tests/test_gpu_prefill.py holds token_nll to against fp64 of the same logits
PER = 17


def reference(z, tok):
    """fp64 scores of rows ``z (B, V)`` (any float dtype) at ids ``tok (B)`` -> (B, 3) float64: logprob, entropy, max_logprob."""
    z = np.asarray(z, dtype=np.float64)
    tok = np.asarray(tok, dtype=np.int64)
    out = np.full((z.shape[0], 3), np.nan)
    for b in range(z.shape[0]):
        m = z[b].max()               # NaN when the row holds one
        if not np.isfinite(m):
            continue
        d = z[b] - m
        e = np.exp(d)
        s = e.sum()
        ls = np.log(s)
        nz = e > 0
        out[b, 0] = d[tok[b]] - ls
        out[b, 1] = ls - (e[nz] * d[nz]).sum() / s
        out[b, 2] = -ls
    return out


def reference_columns(rows, toks, forced_period=0):
    """Scores of one trajectory's ``n`` new tokens: ``rows (n, V)`` the row read for new token j = 1 .. n, ``toks (n)`` -> (n, 3) with
    the forced columns zero."""
    out = reference(rows, toks)
    if forced_period:
        for j in range(1, len(toks) + 1):
            if j % forced_period == 0:
                out[j - 1] = 0.0
    return out


def entropy_sensitivity(z):
    """sum_i p_i |log p_i + H| per row, fp64: the first-order change of the entropy under a sup-norm change of the logits
    (dH/dz_i = -p_i (log p_i + H))."""
    z = np.asarray(z, dtype=np.float64)
    m = z.max(-1, keepdims=True)
    d = z - m
    e = np.exp(d)
    s = e.sum(-1, keepdims=True)
    logp = d - np.log(s)
    p = e / s
    with np.errstate(invalid="ignore"):
        plogp = np.where(p > 0, p * logp, 0.0)
        H = -plogp.sum(-1, keepdims=True)
        return np.where(p > 0, p * np.abs(logp + H), 0.0).sum(-1)


def within(got, want, bound=BOUND):
    """Per element: NaN matches NaN, an infinity its like, anything else within ``bound``."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        close = np.abs(got - want) <= bound
    return np.where(np.isnan(want), np.isnan(got), np.where(np.isinf(want), got == want, close))


# ------------------------------------------------------------------------------------------------ the case table
VOCABS = (130, 1001, 16386, 18432)   # below one sweep of the workgroup; odd (4-byte rows); the model's (8-byte rows); the limit 256 * 72
SIGMAS = (0.02, 1.0, 4.0, 12.0)
_CASES = None


def cases():
    """name -> (z (5, V) float32, tok (5) int64): per vocabulary five rows --
    0 N(0, sigma^2), a random id;  1 N(0, sigma'^2) with one spike of +100 (an fp32 sum without max subtraction overflows), id = arg-max;
    2 a constant row (entropy = log V), id = last id;  3 every third entry -inf, id = one of them;  4 every third entry -inf (another
    phase), id = arg-max -- the sigmas rotate so that every vocabulary meets several.  Plus ``nonfinite``: a NaN among finite entries,
    a +inf, all -inf.  Computed once, shared, read-only."""
    global _CASES
    if _CASES is None:
        out = {}
        for vi, V in enumerate(VOCABS):
            rng = np.random.default_rng(100 + V)
            z = np.empty((5, V), dtype=np.float32)
            tok = np.empty(5, dtype=np.int64)
            z[0] = rng.normal(0, SIGMAS[vi], V)
            tok[0] = rng.integers(0, V)
            z[1] = rng.normal(0, SIGMAS[(vi + 1) % 4], V)
            z[1, rng.integers(0, V)] += 100.0
            tok[1] = z[1].argmax()
            z[2] = np.float32(rng.normal(0, 3))
            tok[2] = V - 1
            z[3] = rng.normal(0, SIGMAS[(vi + 2) % 4], V)
            z[3, 0::3] = -np.inf
            tok[3] = 3 * rng.integers(0, V // 3)
            z[4] = rng.normal(0, SIGMAS[(vi + 3) % 4], V)
            z[4, 2::3] = -np.inf
            tok[4] = z[4].argmax()
            out[f"V{V}"] = (z, tok)
        rng = np.random.default_rng(7)
        V = 1001
        z = rng.normal(0, 1, (3, V)).astype(np.float32)
        z[0, 500] = np.nan
        z[1, 17] = np.inf
        z[2] = -np.inf
        out["nonfinite"] = (z, np.array([3, 17, 0], dtype=np.int64))
        for a, b in out.values():
            a.setflags(write=False); b.setflags(write=False)
        _CASES = out
    return _CASES


ROW_KINDS = ("normal", "spike", "constant", "third_minf_id_minf", "third_minf_id_argmax")


def case_rows():
    """(name, z (V), tok) for every finite row of the table: ``V16386/spike`` ..."""
    for name, (z, tok) in cases().items():
        if name == "nonfinite":
            continue
        for r, kind in enumerate(ROW_KINDS):
            yield f"{name}/{kind}", z[r], int(tok[r])


# ------------------------------------------------------------------------------------------------ the kernel's reduction in fp32
def _threads(z):
    """The row as the kernel's 256 threads hold it: element i belongs to thread (i / 4) % 256, in ascending order; -inf past the row."""
    V = z.shape[0]
    groups = -(-V // 4)
    sweeps = -(-groups // 256)
    pad = np.full(sweeps * 256 * 4, -np.inf, dtype=np.float32)
    pad[:V] = z
    return pad.reshape(sweeps, 256, 4).transpose(1, 0, 2).reshape(256, sweeps * 4)


def _block_sum(x):
    """fp32: per thread already summed (256) -> xor butterfly inside each wave of 64, then (w0 + w1) + (w2 + w3)."""
    w = x.astype(np.float32).reshape(4, 64)
    for o in (32, 16, 8, 4, 2, 1):
        w = (w + w[:, np.arange(64) ^ o]).astype(np.float32)
    return np.float32(np.float32(w[0, 0] + w[1, 0]) + np.float32(w[2, 0] + w[3, 0]))


def kernel_fp32(z, tok, subtract_max=True, guard=True):
    """One row through the kernel's arithmetic in numpy float32 (the keyword arguments make the mutants) -> 3 float32."""
    z = np.asarray(z, dtype=np.float32)
    t = _threads(z)
    with np.errstate(all="ignore"):
        m = np.float32(t.max())
        if not np.isfinite(m):
            return np.full(3, np.nan, dtype=np.float32)
        sub = m if subtract_max else np.float32(0)
        s = np.zeros(256, dtype=np.float32)
        acc = np.zeros(256, dtype=np.float32)
        for q in range(t.shape[1]):
            d = (t[:, q] - sub).astype(np.float32)
            e = np.exp(d).astype(np.float32)
            s = (s + e).astype(np.float32)
            term = (e * d).astype(np.float32)
            if guard:
                term = np.where(e != 0, term, np.float32(0))
            acc = (acc + term).astype(np.float32)
        s, acc = _block_sum(s), _block_sum(acc)
        ls = np.float32(np.log(s))
        lp = np.float32(np.float32(z[tok] - sub) - ls) if 0 <= tok < z.shape[0] else np.float32(np.nan)
        ent = np.float32(ls - np.float32(acc / s))
        mlp = np.float32(np.float32(m - sub) - ls)
    return np.array([lp, ent, mlp], dtype=np.float32)


def top_k_filtered(z, k=100):
    """HF's TopKLogitsWarper: everything below the k-th largest logit becomes -inf."""
    z = np.asarray(z, dtype=np.float32).copy()
    if k < z.shape[0]:
        kth = np.sort(z)[-k]
        z[z < kth] = -np.inf
    return z


# mutants of the ROW arithmetic: name -> (function(z, tok) -> 3 values, the case of the table that must expose it)
ROW_MUTANTS = {
    "base-2 logs": (lambda z, tok: (kernel_fp32(z, tok) / np.float32(np.log(2.0))).astype(np.float32), "V16386/normal"),   # bits, not nats
    "no max subtraction": (lambda z, tok: kernel_fp32(z, tok, subtract_max=False), "V16386/spike"),
    "missing p = 0 guard": (lambda z, tok: kernel_fp32(z, tok, guard=False), "V1001/third_minf_id_argmax"),
    "temperature-scaled row": (lambda z, tok: kernel_fp32(np.asarray(z, dtype=np.float32) / np.float32(0.7), tok), "V16386/normal"),
    "entropy of the top-k-filtered row": (lambda z, tok: np.concatenate([kernel_fp32(z, tok)[:1], kernel_fp32(top_k_filtered(z), tok)[1:2],
                                                                          kernel_fp32(z, tok)[2:]]), "V1001/normal"),   # (sigma 1: the 100 kept of 1,001 hold a part of the mass only)
}


def kernel_columns(rows, toks, forced_period=0, shift=0, zero_forced=True):
    """The step loop around the row arithmetic: new token j = 1 .. n writes column j - 1 + ``shift``; forced columns get zeros unless
    ``zero_forced`` is off (the two column mutants).  Columns never written stay at a sentinel."""
    n = len(toks)
    out = np.full((n, 3), -777.25, dtype=np.float32)
    for j in range(1, n + 1):
        c = j - 1 + shift
        if not 0 <= c < n:
            continue
        if forced_period and j % forced_period == 0 and zero_forced:
            out[c] = 0.0
        else:
            out[c] = kernel_fp32(rows[j - 1], int(toks[j - 1]))
    return out


COLUMN_MUTANTS = {
    "the column of token j + 1": dict(shift=1),
    "a forced column not zero": dict(zero_forced=False),
}


def column_case():
    """One trajectory of 18 new tokens over V = 130 under the forced schedule (column 16 is forced, column 17 sampled again)."""
    rng = np.random.default_rng(41)
    rows = rng.normal(0, 2, (18, 130)).astype(np.float32)
    toks = rng.integers(0, 130, 18)
    toks[16] = 129
    return rows, toks
