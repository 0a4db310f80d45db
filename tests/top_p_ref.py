"""fp64 restatement of the engine's sampler with the nucleus filter (include/ivg.h, ivg_set_top_p, steps 1-4).

Per row: 1. logits / temperature (fp32); 2. the top-k kept set, ties at the threshold kept; 3. with e_i = exp(l_i - max) (fp64) over
the kept set, Z = sum e_i and S(i) = sum of e_j over the kept j with l_j <= l_i, token i survives iff S(i) > (1 - top_p) * Z, and the
maximum always survives; 4. the inverse CDF in ascending id order over the survivors (oracle/llama.py sample_from_logits)."""
import torch


def _scaled(logits, temperature):
    l = logits.float()
    if temperature != 1.0:
        l = l / torch.tensor(temperature, dtype=torch.float32)
    return l


def nucleus(logits, top_k, top_p, temperature=1.0, tol=1e-5):
    """logits [B, V] -> (survive [B, V] bool, e [B, V] fp64 kept weights, near [B] bool, tie [B] bool).

    ``near``: a kept token other than the maximum has |S(i) / Z - (1 - top_p)| < tol -- a row whose outcome an fp64 summation
    order (or a logit error of about tol) may change.  ``tie``: the nucleus boundary falls inside a group of tied logits (the
    maximum's included), where HF's unstable sort decides which of them survive and the engine keeps all of them."""
    l = _scaled(logits, temperature)
    B, V = l.shape
    k = V if not top_k else min(int(top_k), V)
    kth = torch.topk(l, k, dim=-1).values[:, -1:]
    kept = (l >= kth) & (l > float("-inf"))
    m = l.max(-1, keepdim=True).values
    e = torch.where(kept, torch.exp((l - m).double()), torch.zeros((), dtype=torch.double))
    none = torch.zeros(B, dtype=torch.bool)
    if top_p is None or top_p >= 1.0:
        return kept, e, none, none
    Z = e.sum(-1, keepdim=True)
    sv, order = torch.sort(l, dim=-1, stable=True)
    cs = torch.cumsum(torch.gather(e, 1, order), -1)
    hi = torch.searchsorted(sv, l.contiguous(), right=True) - 1              # last sorted position with a value <= l_i
    lo = torch.searchsorted(sv, l.contiguous(), right=False)                 # first sorted position of l_i's tie group
    S = torch.gather(cs, 1, hi)                                              # mass of the kept tokens not above l_i
    below = torch.where(lo > 0, torch.gather(cs, 1, (lo - 1).clamp(min=0)), torch.zeros((), dtype=torch.double))
    cut = (1.0 - float(torch.tensor(top_p, dtype=torch.float32))) * Z         # the engine holds top_p as a float
    is_max = l == m
    survive = kept & ((S > cut) | is_max)
    frac, c = S / Z, 1.0 - float(torch.tensor(top_p, dtype=torch.float32))
    near = (kept & ~is_max & ((frac - c).abs() < tol)).any(-1)
    group = hi > lo                                                          # more than one token holds this value
    tie = (kept & group & (below / Z <= c + tol) & ((frac >= c - tol) | is_max)).any(-1)
    return survive, e, near, tie


def sample(logits, top_k, top_p, u, temperature=1.0, tol=1e-5):
    """-> (tokens [B], near [B]): step 4 over the survivors with uniforms u [B] (None: greedy argmax, no filter)."""
    if u is None:
        return torch.argmax(logits, -1), torch.zeros(logits.shape[0], dtype=torch.bool)
    survive, e, near, _ = nucleus(logits, top_k, top_p, temperature, tol)
    w = torch.where(survive, e, torch.zeros((), dtype=torch.double))
    cdf = torch.cumsum(w, -1)
    target = u.double().view(-1, 1) * cdf[:, -1:]
    return (cdf > target).double().argmax(-1), near


def hf_survivors(logits, top_k, top_p, temperature=1.0):
    """The surviving set of HF's own warpers, in the order generate builds them: temperature -> top-k -> top-p."""
    from transformers.generation.logits_process import TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper
    s = logits.float()
    if temperature != 1.0:
        s = TemperatureLogitsWarper(temperature)(None, s)
    if top_k:
        s = TopKLogitsWarper(top_k)(None, s)
    if top_p is not None and top_p < 1.0:
        s = TopPLogitsWarper(top_p)(None, s)
    return s > float("-inf")
