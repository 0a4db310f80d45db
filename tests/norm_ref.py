"""GroupNorm, Llama RMSNorm and the row softmax of csrc/norm.hip in fp64: the contracts of ivg_op_groupnorm, ivg_op_add_rmsnorm and
ivg_op_softmax (include/ivg.h) restated for tests/test_gpu_norm.py and its CPU self-check tests/test_norm_cpu.py.  No GPU import.

Every bound is first order in u = 2^-24 and the output type's rounding (2^-9 relative for a bf16 store, as a term: the doubled sum
then covers the half ulp 2^-8), a sum of named terms each tied to one arithmetic step of the kernel, doubled.  The references take
the stored inputs (bf16 or fp32 values), so the bound has only the kernel's own arithmetic to cover.  Derived, not fitted.

softmax (softmax_kernel), per element.  Row r is query q = r % Lq; it sees columns [0, lim), lim = Lk, or min(Lk, q + Lk - Lq + 1)
when causal.  p_j = exp(s_j - m) / sum.  Columns [lim, ldp) (masked and pad) are written as exact zeros: their bound is 0.
  E_exp = (|s_j - m| + 2) u p_j     the fp32 difference s_j - m (relative u of |s_j - m|, in the exponent) and expf (2 ulp)
  E_sum = (8 + 6 + 2 + 2) u p_j     the row sum: eight strided terms per thread, six wave levels, the 4-wave tree (2 levels); then
                                    inv = 1 / sum and the multiply v * inv
  E_out = 2^-9 p_j                  bf16 output only
  E_tiny = 2^-125                   results below the fp32 normal range may be flushed (expf of a large negative argument)
  bound = 2 (E_exp + E_sum + E_out + E_tiny)

GroupNorm (gn_partial_kernel + gn_apply_kernel), per element: t = x * scale + shift, y = [silu](t) [+ pos[p][c]].
  E_coef = |x| e_scale + e_shift    conv3x3_ref.coef_reference (the same statistics and the same coefficient arithmetic, gn_apply and
                                    gn_coef_kernel share it), with n_lane = ceil(min(P, 1024) / pl_n) fp32 terms per lane,
                                    pl_n = 256 / (C / VEC) pixel lanes, VEC = 8 (bf16), 4 (fp32)
  E_fma  = u |t|                    the fused multiply-add's one rounding
  E_silu                            conv3x3_ref._silu_err on an argument off by E_coef + E_fma (common.h silu_t)
  E_pos  = u |y|                    the fp32 addition of the position row
  E_out  = 2^-9 |y|                 bf16 output only
  bound = 2 (sum of the terms that apply)

RMSNorm (add_rmsnorm_kernel): inv = rsqrt(sum x^2 / H + eps), out = T(w * T(x * inv)) -- the normalised row is rounded to the element
type T before the weight, as HF's LlamaRMSNorm does.
  fp32, per element, relative to |out|:
    E_ss  = (8 + 6 + 2) u           the sum of squares: eight fma per thread, six wave levels, the 4-wave tree -- halved by the root
    E_ms  = 2 u                     ss / H and + eps -- halved by the root
    E_rsq = 2 u                     rsqrtf
    r_inv = (16 + 2) / 2 u + 2 u = 11 u
    E_mul = 2 u                     x * inv and w * nrm
    bound = 2 (r_inv + E_mul) |out| = 26 u |out|
  bf16: two roundings to 8 bits decide the result; a bound in bf16 ulps would accept an omitted intermediate rounding.  Instead the
  candidates: inv anywhere within 2 r_inv of the fp64 value, the fp32 product x * inv off by +-u before it is rounded to bf16, and for
  each resulting nrm the fp32 product w * nrm off by +-u before the final rounding.  Rounding is monotone, so the extremes (and the
  centre) enumerate every value the kernel can produce.  DECIDED element: all candidates agree -- the kernel's bits must equal them.
  UNDECIDED: the kernel's value must be one of the candidates.  Undecided elements may be at most 1 % of a case (a condition the CPU
  self-check asserts for every case from the reference alone).

Mutants restate kernel bugs (keyword `mutant`); tests/test_norm_cpu.py shows each misses the true reference by >= 10x the bound on at
least one case of the table, and that an fp32 restatement of each kernel (same sum structure) stays within half the bound on all.
A bf16 store alone can take the whole of 2 E_out (a value just above a binade's first rounding boundary is off by 2^-8 of itself), so
for bf16 outputs the restatement is held to half of the bound WITHOUT E_out on its value before the store (`out_term=False`,
`rounded=False`), and to the full bound after it: the terms a missing one would hide behind are the fp32 ones.
"""
import numpy as np
import torch
import torch.nn.functional as F

from conv3x3_ref import TINY, _silu_err, coef_reference
from decode_gemm_ref import U, rne_bf16

U_BF16 = 2.0 ** -9


def tdt(dt):
    return torch.bfloat16 if dt == "bf16" else torch.float32


def stored(x, dt):
    """values as the tensor of type dt holds them, as fp32"""
    return x.float().to(tdt(dt)).float()


def _gen(*key):
    import zlib
    return torch.Generator().manual_seed(zlib.crc32("-".join(str(k) for k in key).encode()) % 1000003)


def ratio(err, bound):
    """err / bound with 0 / 0 = 0 and x / 0 = inf; NaN errors count as inf"""
    err = torch.nan_to_num(err, nan=float("inf"), posinf=float("inf"))
    return torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))


# ================================================================================================ softmax
SOFTMAX_SHAPES = [  # (Lq, Lk, lds, ldp, causal)
    (1, 1, 1, 1, 0), (5, 16, 16, 16, 0), (3, 255, 256, 256, 0), (3, 256, 256, 256, 0), (3, 257, 320, 320, 0), (2, 2048, 2048, 2048, 0),
    (4, 100, 128, 192, 0), (33, 33, 64, 64, 1), (64, 64, 64, 64, 1), (7, 40, 64, 64, 1)]
SOFTMAX_FAMILIES = ("randn3", "wide", "dominant")
SOFTMAX_BATCH = 2
SOFTMAX_CASES = [(dt,) + s + (fam,) for dt in ("fp32", "bf16") for s in SOFTMAX_SHAPES for fam in SOFTMAX_FAMILIES]


def softmax_id(c):
    dt, Lq, Lk, lds, ldp, causal, fam = c
    return f"{dt}-Lq{Lq}-Lk{Lk}-lds{lds}-ldp{ldp}-{'causal' if causal else 'full'}-{fam}"


def softmax_limits(rows, Lq, Lk, causal):
    q = torch.arange(rows) % Lq
    return torch.clamp(q + (Lk - Lq) + 1, max=Lk) if causal else torch.full((rows,), Lk)


def softmax_inputs(c):
    """-> S fp32 [rows][lds]; columns [Lk, lds) hold NaN (never read).  dominant: one entry 100 above the rest, cycling per row over the
    first column, the last visible one and every visible multiple of 256."""
    dt, Lq, Lk, lds, ldp, causal, fam = c
    rows = SOFTMAX_BATCH * Lq
    g = _gen("softmax", *c)
    S = torch.randn(rows, lds, generator=g) * 3.0
    if fam == "wide":
        S = (torch.rand(rows, lds, generator=g) * 2.0 - 1.0) * 3e4
    elif fam == "dominant":
        lim = softmax_limits(rows, Lq, Lk, causal)
        for r in range(rows):
            spots = sorted({0, int(lim[r]) - 1} | {j for j in range(256, int(lim[r]), 256)})
            S[r, spots[r % len(spots)]] += 100.0
    S[:, Lk:] = float("nan")
    return S


def softmax_ref(S, Lq, Lk, ldp, causal, dt, mutant=None, out_term=True):
    """S fp32 [rows][lds] -> (P fp64 [rows][ldp], bound [rows][ldp]).  Mutants (evaluated in fp32 where the bug is one of range):
      "lim+1" / "lim-1"   the causal limit off by one
      "max256"            the maximum taken over the first 256 columns only (fp32: the exponentials may overflow)
      "drop_wave"         the partial sum of wave 1 (columns j with (j % 256) // 64 == 1) left out of the row sum
      "pad_unwritten"     columns [Lk, ldp) keep what the buffer held (a sentinel)"""
    rows = S.shape[0]
    lim = softmax_limits(rows, Lq, Lk, causal)
    if mutant in ("lim+1", "lim-1") and causal:
        lim = torch.clamp(lim + (1 if mutant == "lim+1" else -1), max=Lk)
    j = torch.arange(ldp)[None, :]
    vis = j < lim[:, None]
    s = torch.zeros(rows, ldp, dtype=torch.float64)
    n = min(ldp, S.shape[1])
    s[:, :n] = S[:, :n].double()
    s = torch.where(vis, s, torch.full_like(s, -float("inf")))
    if mutant == "max256":
        m = s[:, :256].max(-1, keepdim=True).values
        e = torch.exp((s - m).float()).double()          # fp32 range: overflow to inf as the kernel would
        e = torch.where(vis, e, torch.zeros_like(e))
        p = (e.float() / e.float().sum(-1, keepdim=True)).double()
    else:
        m = s.max(-1, keepdim=True).values
        e = torch.where(vis, torch.exp(s - m), torch.zeros_like(s))
        tot = e.sum(-1, keepdim=True)
        if mutant == "drop_wave":
            tot = torch.where(((j % 256) // 64 == 1), torch.zeros_like(e), e).sum(-1, keepdim=True)
        p = e / tot
    if mutant == "pad_unwritten":
        p = torch.where(j >= Lk, torch.full_like(p, 1536.0), p)
    d = torch.where(vis, (s - m).abs(), torch.zeros_like(s))
    bound = 2.0 * ((d + 2.0) * U * p + (8 + 6 + 2 + 2) * U * p + (U_BF16 * p if dt == "bf16" and out_term else 0.0) + TINY)
    bound = torch.where(vis, bound, torch.zeros_like(bound))
    return p, bound


def softmax_restated(S, Lq, Lk, ldp, causal, dt, rounded=True):
    """softmax_kernel in fp32 with its sum structure: 8 strided terms per thread in order, a butterfly over 64 lanes, the 4-wave tree"""
    rows = S.shape[0]
    lim = softmax_limits(rows, Lq, Lk, causal)
    j = torch.arange(2048)[None, :]
    v = torch.full((rows, 2048), -float("inf"))
    n = min(Lk, S.shape[1])
    v[:, :n] = S[:, :n]
    vis = j < lim[:, None]
    v = torch.where(vis, v, torch.full_like(v, -float("inf")))
    m = v.max(-1, keepdim=True).values
    e = torch.where(vis, torch.exp(v - m), torch.zeros_like(v)).view(rows, 8, 4, 64)
    t = e[:, 0]
    for i in range(1, 8):
        t = t + e[:, i]
    w = 64
    while w > 1:
        w //= 2
        t = t[..., :w] + t[..., w:2 * w]
    t = t[..., 0]
    tot = (t[:, 0] + t[:, 1]) + (t[:, 2] + t[:, 3])
    inv = 1.0 / tot
    out = (e.view(rows, 2048) * inv[:, None])[:, :ldp]
    return stored(out, dt if rounded else "fp32").double()


# ================================================================================================ GroupNorm
def gn_vec(dt):
    return 8 if dt == "bf16" else 4


def gn_geometry(P, C, dt):
    """-> (vpp, pl_n, chunk_px, nchunks, n_lane)"""
    vpp = C // gn_vec(dt)
    pl_n = 256 // vpp
    chunk_px = min(P, 1024)
    return vpp, pl_n, chunk_px, -(-P // chunk_px), -(-chunk_px // pl_n)


GN_N = 2
_GN_SHAPES = [  # (C, groups, dt, (P, P)); C / VEC divides 256 in the first eight, not in the last six
    (32, 32, "fp32", (1, 1025)), (32, 32, "bf16", (5, 2049)), (64, 32, "fp32", (255, 256)), (64, 32, "bf16", (257, 1024)),
    (64, 8, "fp32", (1025, 5)), (512, 32, "bf16", (256, 1)), (1024, 32, "fp32", (257, 2049)), (2048, 32, "bf16", (1024, 255)),
    (96, 32, "bf16", (1, 257)), (160, 32, "fp32", (5, 1025)), (192, 32, "fp32", (255, 2049)), (192, 32, "bf16", (256, 1024)),
    (768, 32, "fp32", (1025, 1)), (768, 32, "bf16", (2049, 256))]
GN_FAMILIES = ("plain", "offset", "near_constant")


def _gn_cases():
    out = []
    for C, groups, dt, Ps in _GN_SHAPES:
        for P in Ps:
            i = len(out)
            out.append(dict(C=C, groups=groups, dt=dt, P=P, family=GN_FAMILIES[i % 3], silu=i % 2, pos=(i // 2) % 2,
                            eps=(1e-6, 1e-5)[(i // 3) % 2]))
    # the cross-attention norms' form at a shape with idle lanes, and a position table past one block on every family
    out.append(dict(C=768, groups=32, dt="bf16", P=257, family="plain", silu=0, pos=1, eps=1e-5))
    out.append(dict(C=64, groups=8, dt="fp32", P=257, family="near_constant", silu=0, pos=1, eps=1e-5))
    return out


GN_CASES = _gn_cases()


def gn_id(c):
    return (f"{c['dt']}-C{c['C']}-g{c['groups']}-P{c['P']}-{c['family']}" + ("-silu" if c["silu"] else "") + ("-pos" if c["pos"] else "")
            + f"-eps{c['eps']:g}")


def gn_inputs(c):
    """-> x [N][P][C] (values of type dt, as fp32), gamma, beta fp32 [C], pos fp32 [P][C] or None.  Statistics differ per image.
    offset: per (image, group) means of +-32 std; near_constant: std 1e-3 of the (image, group) mean, means log-uniform in
    [1e-2, 1] with either sign (at the small end var << eps and eps decides, at the large end E[x^2] - mean^2 cancels to noise)."""
    C, groups, P, dt = c["C"], c["groups"], c["P"], c["dt"]
    g = _gen("gn", gn_id(c))
    cpg = C // groups
    z = torch.randn(GN_N, P, groups, cpg, generator=g)
    sign = torch.where(torch.rand(GN_N, 1, groups, 1, generator=g) < 0.5, -1.0, 1.0)
    if c["family"] == "plain":
        std = torch.tensor([2.0, 0.7]).view(GN_N, 1, 1, 1)
        x = z * std + torch.tensor([0.5, -1.5]).view(GN_N, 1, 1, 1)
    elif c["family"] == "offset":
        std = torch.tensor([1.0, 0.25]).view(GN_N, 1, 1, 1)
        x = (z + 32.0 * sign) * std
    else:
        mean = sign * 10.0 ** (-2.0 * torch.rand(GN_N, 1, groups, 1, generator=g))
        x = mean * (1.0 + 1e-3 * z)
    x = stored(x.reshape(GN_N, P, C), dt)
    gamma = 1.0 + 0.5 * torch.randn(C, generator=g)
    beta = torch.randn(C, generator=g)
    pos = torch.randn(P, C, generator=g) if c["pos"] else None
    return x, gamma, beta, pos


def gn_ref(c, x, gamma, beta, pos, mutant=None, out_term=True):
    """-> (y fp64 [N][P][C], bound).  Mutants:
      "count_padded"   the element count taken as nchunks * chunk_px * cpg
      "stats_image0"   image 0's statistics used for every image
      "cpg_32_groups"  the group of a channel computed as c / (C / 32) (modulo groups)
      "pos_block"      the position row indexed relative to the 256-pixel block
      "no_eps"         eps dropped
      "idle_lanes"     the threads past pl_n * vpp not masked: they add the pixels pl_n, 2 pl_n, ... of a chunk a second time"""
    N, P, C = x.shape
    groups, dt = c["groups"], c["dt"]
    eps = float(np.float32(c["eps"]))
    cpg = C // groups
    vpp, pl_n, chunk_px, nchunks, n_lane = gn_geometry(P, C, dt)
    scale, shift, e_scale, e_shift = coef_reference(x.view(N, P, 1, C), gamma, beta, groups, n_lane, eps=eps)
    if mutant is not None:
        xd = x.double()
        wgt = torch.ones(P, C, dtype=torch.float64)
        if mutant == "idle_lanes":
            extra = 256 - pl_n * vpp
            pin = torch.arange(P) % chunk_px
            again = (pin % pl_n == 0) & (pin >= pl_n)
            wgt[again, :min(C, extra * gn_vec(dt))] += 1.0          # extra = 0: an empty slice
        gidx = torch.arange(C) // cpg
        s1 = (xd * wgt).reshape(N, P, groups, cpg).sum((1, 3))
        s2 = (xd * xd * wgt).reshape(N, P, groups, cpg).sum((1, 3))
        cnt = float(nchunks * chunk_px * cpg) if mutant == "count_padded" else float(P * cpg)
        mean = s1 / cnt
        var = (s2 / cnt - mean * mean).clamp_min(0.0)
        rstd = 1.0 / torch.sqrt(var + (0.0 if mutant == "no_eps" else eps))
        if mutant == "stats_image0":
            mean, rstd = mean[:1].expand(N, -1), rstd[:1].expand(N, -1)
        if mutant == "cpg_32_groups":
            gidx = (torch.arange(C) // max(1, C // 32)) % groups
        scale = gamma.double()[None] * rstd[:, gidx]
        shift = beta.double()[None] - mean[:, gidx] * scale
    xd = x.double()
    t = xd * scale[:, None] + shift[:, None]
    e = xd.abs() * e_scale[:, None] + e_shift[:, None] + U * t.abs()
    if c["silu"]:
        y, e = _silu_err(t, e)
    else:
        y = t
    if pos is not None:
        pp = pos.double()
        if mutant == "pos_block":
            pp = pp[torch.arange(P) % 256]
        y = y + pp[None]
        e = e + U * y.abs()
    if dt == "bf16" and out_term:
        e = e + U_BF16 * y.abs()
    return y, 2.0 * e


def _fma32(a, b, c):
    """fp32 fma of fp32 tensors: the product of two fp32 values is exact in fp64"""
    return (a.double() * b.double() + c.double()).float()


def gn_restated(c, x, gamma, beta, pos, rounded=True):
    """gn_partial + gn_apply in fp32: per-lane sums of n_lane terms in pixel order (sum += f; sq = fma(f, f, sq)), everything after in
    double, the coefficients and y = fma(x, scale, shift) in fp32, the output rounded to the element type"""
    N, P, C = x.shape
    groups, dt = c["groups"], c["dt"]
    cpg = C // groups
    vpp, pl_n, chunk_px, nchunks, n_lane = gn_geometry(P, C, dt)
    a = torch.zeros(N, groups, dtype=torch.float64)
    b = torch.zeros(N, groups, dtype=torch.float64)
    for q in range(nchunks):
        xc = x[:, q * chunk_px:min(P, (q + 1) * chunk_px)]
        pad = n_lane * pl_n - xc.shape[1]
        xc = torch.cat([xc, torch.zeros(N, pad, C)], 1).view(N, n_lane, pl_n, C)
        s = torch.zeros(N, pl_n, C)
        sq = torch.zeros(N, pl_n, C)
        for i in range(n_lane):
            s = s + xc[:, i]
            sq = _fma32(xc[:, i], xc[:, i], sq)
        a += s.double().sum(1).view(N, groups, cpg).sum(-1)
        b += sq.double().sum(1).view(N, groups, cpg).sum(-1)
    cnt = float(P * cpg)
    mean = a / cnt
    var = (b / cnt - mean * mean).clamp_min(0.0)
    rstd = (1.0 / torch.sqrt(var + float(np.float32(c["eps"])))).float()
    gi = torch.arange(C) // cpg
    sc = gamma[None] * rstd[:, gi]
    sh = beta[None] - mean.float()[:, gi] * sc
    y = _fma32(x, sc[:, None].expand_as(x), sh[:, None].expand_as(x))
    if c["silu"]:
        y = y / (1.0 + torch.exp(-y))
    if pos is not None:
        y = y + pos[None]
    return stored(y, dt if rounded else "fp32").double()


# ================================================================================================ RMSNorm
RMS_H = (8, 255, 256, 257, 768, 1024, 2047, 2048)
RMS_CASES = [(dt, M, H, eps) for dt in ("fp32", "bf16") for M in (1, 5) for H in RMS_H for eps in (1e-6, 1e-5)]
RMS_R_INV = ((8 + 6 + 2) + 2) / 2.0 * U + 2.0 * U      # 11 u
RMS_SCALES = (1e-3, 0.0, 1.0, 1e3, 3e-2)                # row scales of an M = 5 case; the second row is all zero


def rms_id(c):
    return f"{c[0]}-M{c[1]}-H{c[2]}-eps{c[3]:g}"


def rms_inputs(c):
    """-> x [M][H] (values of type dt, as fp32), w fp32 [H].  bf16: all elements of a row that share one of the 128 bf16 mantissas sit
    equally close to a rounding boundary of x * inv, so a short row can exceed the 1 % cap on undecided elements by one unlucky
    mantissa; the draw is then repeated with the next salt (a condition on the inputs, checked from the reference alone)."""
    dt, M, H, eps = c
    scales = RMS_SCALES if M > 1 else ((1e-2, 1.0, 1e2)[RMS_H.index(H) % 3],)
    for salt in range(16):
        g = _gen("rms", salt, *c)
        x = stored(torch.randn(M, H, generator=g) * torch.tensor(scales[:M]).view(M, 1), dt)
        w = 1.0 + 0.5 * torch.randn(H, generator=g)
        if dt == "fp32":
            break
        cand = rms_candidates_bf16(x, w, eps)
        if float((cand != cand[:1]).any(0).double().mean()) <= 0.01:
            break
    return x, w


def _rms_inv(x, eps, mutant):
    H = x.shape[1]
    xd = x.double()
    cnt = 256 * -(-H // 256) if mutant == "mean_padded" else H
    ms = (xd * xd).sum(-1, keepdim=True) / cnt
    eps = float(np.float32(eps))
    return 1.0 / (torch.sqrt(ms) + eps) if mutant == "eps_outside" else 1.0 / torch.sqrt(ms + eps)


def rms_ref_fp32(x, w, eps, mutant=None):
    """-> (out fp64, bound).  Mutants: "mean_padded" (mean over 256 * ceil(H / 256)), "eps_outside" (1 / (sqrt(ms) + eps))"""
    out = w.double()[None] * (x.double() * _rms_inv(x, eps, mutant))
    return out, 2.0 * (RMS_R_INV + 2.0 * U) * out.abs()


def _rne_bf16_t(v):
    return torch.from_numpy(rne_bf16(v.numpy()))


def rms_candidates_bf16(x, w, eps, mutant=None):
    """-> candidates fp64 [K][M][H]: every value add_rmsnorm_kernel<bf16> can store (module docstring).  Mutant "no_mid_rounding": the
    normalised row is not rounded to bf16 before the weight (one candidate, from the fp64 inv)."""
    inv = _rms_inv(x, eps, mutant if mutant != "no_mid_rounding" else None)
    xd, wd = x.double(), w.double()[None]
    if mutant is not None:
        nrm = xd * inv if mutant == "no_mid_rounding" else _rne_bf16_t(xd * inv)
        return _rne_bf16_t(wd * nrm)[None]
    out = []
    for di in (-2.0 * RMS_R_INV, 0.0, 2.0 * RMS_R_INV):
        for d1 in (-U, 0.0, U):
            nrm = _rne_bf16_t(xd * (inv * (1.0 + di)) * (1.0 + d1))
            for d2 in (-U, 0.0, U):
                out.append(_rne_bf16_t(wd * nrm * (1.0 + d2)))
    return torch.stack(out)


def rms_check_bf16(got, cand):
    """got fp64 [M][H] (the stored bf16 values) -> (undecided share, elements that equal no candidate)"""
    decided = (cand == cand[:1]).all(0)
    hit = (cand == got[None]).any(0)
    return float((~decided).double().mean()), int((~hit).sum())


def rms_restated(x, w, eps, dt):
    """add_rmsnorm_kernel in fp32 with its sum structure (8 fma per thread, the butterfly, the 4-wave tree)"""
    M, H = x.shape
    f = torch.zeros(M, 2048)
    f[:, :H] = x
    f = f.view(M, 8, 4, 64)
    t = torch.zeros(M, 4, 64)
    for i in range(8):
        t = _fma32(f[:, i], f[:, i], t)
    n = 64
    while n > 1:
        n //= 2
        t = t[..., :n] + t[..., n:2 * n]
    t = t[..., 0]
    ss = (t[:, 0] + t[:, 1]) + (t[:, 2] + t[:, 3])
    inv = torch.rsqrt(ss / float(H) + torch.tensor(eps, dtype=torch.float32))
    nrm = stored(x * inv[:, None], dt)
    return stored(w[None] * nrm, dt).double()


# ================================================================================================ torch formulations (independent)
def softmax_torch(S, Lq, Lk, causal):
    rows = S.shape[0]
    lim = softmax_limits(rows, Lq, Lk, causal)
    s = S[:, :Lk].double().masked_fill(torch.arange(Lk)[None, :] >= lim[:, None], -float("inf"))
    return torch.softmax(s, -1)


def gn_torch(c, x, gamma, beta, pos, dtype=torch.float64):
    y = F.group_norm(x.to(dtype).permute(0, 2, 1), c["groups"], gamma.to(dtype), beta.to(dtype), float(np.float32(c["eps"]))).permute(0, 2, 1)
    if c["silu"]:
        y = F.silu(y)
    return y + pos.to(dtype)[None] if pos is not None else y


def rms_torch(x, w, eps):
    xd = x.double()
    return w.double() * (xd * torch.rsqrt(xd.pow(2).mean(-1, keepdim=True) + float(np.float32(eps))))

