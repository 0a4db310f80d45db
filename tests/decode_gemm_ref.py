"""One decode-step GEMM in fp64: the contract of ivg_op_skinny_policy (include/ivg.h; dgemm3.hip third generation, dgemm.hip second),
restated for tests/test_gpu_decode_gemm.py and its CPU self-check.  No GPU import.

Y = epi(X W^T), X [M][K], W [N][K] (row strides ldx, ldw), for every epilogue the dispatchers accept (flags of csrc/igemm.h):
  0                      plain
  SK_NORM                row scale rs_m = rsqrt(mean_k x_mk^2 + eps) (RMSNorm with its weight folded into W)
  SK_NORM | IG_GLU       W rows packed [16 gate | 16 up] per 32: out = silu(rs g) * (rs u), N_out = N / 2
  IG_RESIDUAL (| SK_NORM) in place: Y = round(Y + v)
  IG_OUT_F32 (| SK_NORM) fp32 output whatever the operand type (the lm_head form)
Kinds: "bf16", "fp32" (operands and output of that type), "x3" (IVG_F32X3: fp32 tensors; dg3_kernel<float, ..., X3> splits both
operands into hi = bf16(x), lo = bf16(x - hi) and forms hi*hi, lo*hi, hi*lo and lo*lo on the bf16 MFMA; dgemm3.hip dg3_split_hi_lo).
The reference multiplies exactly those operands: the stored values for bf16 / fp32, the split pairs for x3, every product exact in
fp64 (8 x 8 and 24 x 24 significant bits), so the bound has only the kernel's fp32 arithmetic to cover.  The row scale always reads
the stored (unsplit) x.

Per-element bound, u = 2^-24, first order, for an output element (m, n) with A = sum_k |x_mk w_nk| (x3: (|hi|+|lo|)(|hi|+|lo|)):
  E_acc = u * n_chain * rs * A      fp32 accumulation.  n_chain from the plan (ivg_op_skinny_plan), not from K: the sequential
                                    roundings of one wave's K slice (lpw lines of 128 bytes: bf16 2 MFMAs per line, x3 4, fp32 8 MFMAs
                                    of 4 fused multiply-adds each = 32 roundings per line), plus the MFMA's internal depth (32 for
                                    the bf16 16x16x32 form, counted once; the f32 form is its own fma chain), plus the fixed-order
                                    combine of the waves' partial tiles (waves additions)
  E_rs  = (n_ss / 2 + 5) u |v|      row scale, v = rs * (x W^T) the scaled value.  The mean of squares: the fp32 sum (a chain of 16
                                    roundings per line of the lane's slice -- squares by fma or v_dot2 -- then the 4 lane groups
                                    and the waves: n_ss = 16 lpw + waves + 2), times 1/K (gen3: a host-rounded inv_k and a multiply;
                                    gen2: a division; 2 either way), + eps (1): n_ss + 3, entering rsqrt at half weight; rsqrtf
                                    (v_rsq_f32, 2) and the multiply by rs (1): n_ss / 2 + 4.5 <= n_ss / 2 + 5
  GLU   out = s(g) u' with s = silu, g = rs * gate, u' = rs * up:
        E = |s'(g)| E_g |u'| + |s(g)| E_u + e_silu |s(g) u'| + u |s(g) u'|
        e_silu = (1 - sigma(g)) (2 |g| + 2) u + 4 u: __expf is exp2 of the rounded -g log2(e) (relative error |g| u from the
                 argument and the constant, 2 u from v_exp_f32), which moves sigma = 1 / (1 + e^-g) by the factor (1 - sigma); then
                 1 + e (1), v_rcp_f32 or the IEEE quotient (2), the multiply (1): common.h silu_t
        s'(g) = sigma (1 + g (1 - sigma))
  residual: pre = r + v, E += u |pre| (the fp32 addition)
  E_out = 2^-8 |pre| (bf16: 8 significant bits, the unit roundoff of the previous test PRs) or 2^-24 |pre| (fp32)
  bound = 2 (E_pre + E_out) with E_pre everything before the final rounding -- twice the first-order estimate.
The constants are derived, not fitted.

Exact rounding (bf16 outputs).  Where the fp64 pre-rounding value lies farther than 2 E_pre from every bf16 rounding boundary (the
midpoints between neighbouring bf16 values), every value the kernel can hold before its store rounds to the same bf16 number: the
stored value must equal RNE(pre) bit for bit.  This catches a truncating or double-rounding store, which the 2 * 2^-8 bound lets pass.

Mutants (keyword `mutant` of reference) restate the kernel bugs the bound must reject; tests/test_decode_gemm_cpu.py shows each
misses the true reference by >= 10x the bound on an input built to expose it.
"""
import numpy as np
import torch

U = 2.0 ** -24
SK_NORM, IG_GLU, IG_RESIDUAL, IG_OUT_F32 = 64, 16, 4, 32
EPS = float(np.float32(1e-6))   # SkinnyArgs::eps as the kernel holds it
KINDS = ("bf16", "fp32", "x3")
PLAN_FIELDS = ("gen", "mf", "fn", "waves", "klw", "ring", "lg", "nburst", "wmax", "wr", "x3")


def plan_dict(p):
    return dict(zip(PLAN_FIELDS, (int(v) for v in p)))


def elem_bytes(kind):
    return 2 if kind == "bf16" else 4


def lines_per_wave(plan):
    """128-byte lines of K one wave reduces: gen3 klw, gen2 lg * nburst"""
    return plan["klw"] if plan["gen"] == 3 else plan["lg"] * plan["nburst"]


def chain_lengths(plan, kind):
    """-> (n_chain, n_ss): fp32 roundings on one output element's accumulation path and on its row's sum of squares"""
    lpw, waves = lines_per_wave(plan), plan["waves"]
    if kind == "fp32":
        n_chain = 32 * lpw + waves
    else:
        n_chain = (4 if kind == "x3" else 2) * lpw + 32 + waves
    return n_chain, 16 * lpw + waves + 2


# ------------------------------------------------------------------------------------------------ rounding
def bf16_split(x):
    """fp32 tensor -> (hi, lo) as fp64: hi = RNE_bf16(x), lo = RNE_bf16(x - hi) (x - hi is exact in fp32)"""
    x = x.float()
    hi = x.to(torch.bfloat16).float()
    lo = (x - hi).to(torch.bfloat16).float()
    return hi.double(), lo.double()


def _bf16_grid(x):
    """-> (ulp, q): x = q * ulp with ulp the bf16 spacing of |x|'s binade (fp64 arrays; q exact)"""
    _, e = np.frexp(x)
    e = np.maximum(e, -125)            # subnormal bf16 spacing 2^-133
    ulp = np.ldexp(1.0, e - 8)
    return ulp, x / ulp


def rne_bf16(x):
    """fp64 array -> the RNE bf16 value (as fp64), one rounding (no detour through fp32)"""
    ulp, q = _bf16_grid(x)
    return np.rint(q) * ulp


def trunc_bf16(x):
    ulp, q = _bf16_grid(x)
    return np.trunc(q) * ulp


def bf16_boundary_distance(x):
    """distance from x to the nearest bf16 rounding boundary (midpoint of two neighbours)"""
    ulp, q = _bf16_grid(x)
    return np.abs(np.abs(q - np.floor(q)) - 0.5) * ulp


def rne_f32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


# ------------------------------------------------------------------------------------------------ the reference
def _sigmoid(g):
    return 1.0 / (1.0 + torch.exp(-g))


def reference(X, W, flags, kind, plan, R=None, eps=EPS, mutant=None):
    """X [M][K], W [N][K]: the stored values (torch, any float type; x3: fp32).  R [M][N_out]: Y's initial values for IG_RESIDUAL.
    plan: plan_dict of ivg_op_skinny_plan (waves and lines per wave drive the chain lengths and the line mutants).
    -> dict(pre, e_pre, bound, out) as fp64 tensors [M][N_out]: the value before the final rounding, its error bound, the bound of
    the stored value and RNE(pre) in the output type.  mutant: None or a tuple (see MUTANTS)."""
    M, K = X.shape
    N = W.shape[0]
    glu, norm = bool(flags & IG_GLU), bool(flags & SK_NORM)
    res, f32out = bool(flags & IG_RESIDUAL), bool(flags & IG_OUT_F32)
    mk = mutant[0] if mutant else None
    x, w = X.double(), W.double()
    epl = 128 // elem_bytes(kind)                          # K elements per 128-byte line
    lpw = lines_per_wave(plan)
    xs = x.clone()                                         # what the kernel stages (the line mutants change it)
    ws = w.clone()
    if mk in ("drop_line", "dup_line"):
        j = (plan["waves"] - 1) * lpw                      # first line of the last wave's slice
        sl = slice(j * epl, (j + 1) * epl)
        if mk == "drop_line":
            xs[:, sl] = 0.0
            ws[:, sl] = 0.0
        else:                                              # line j staged again in place of line j + 1 (ring-slot reuse)
            sl1 = slice((j + 1) * epl, (j + 2) * epl)
            xs[:, sl1] = x[:, sl]
            ws[:, sl1] = w[:, sl]
    if kind == "x3":
        xh, xl = bf16_split(xs)
        wh, wl = bf16_split(ws)
        if mk == "x3_one_bf16":
            P = xh @ wh.T
        else:
            P = xh @ wh.T + xl @ wh.T + xl @ wl.T
            if mk != "x3_drop_hilo":
                P = P + xh @ wl.T
        A = (xh.abs() + xl.abs()) @ (wh.abs() + wl.abs()).T
    else:
        P = xs @ ws.T
        A = x.abs() @ w.abs().T
    n_chain, n_ss = chain_lengths(plan, kind)
    rs = torch.ones(M, 1, dtype=torch.float64)
    if norm:
        ssq = (xs * xs).sum(1, keepdim=True)
        kk = K - 1 if mk == "inv_k_minus1" else K
        rs = 1.0 / torch.sqrt(ssq / kk + (0.0 if mk == "no_eps" else eps))
        if mk == "rs_xor1":
            idx = torch.arange(M) ^ 1
            idx = torch.where(idx < M, idx, torch.arange(M))
            rs = rs[idx]
    v = P * rs                                             # [M][N]
    e_v = U * n_chain * rs * A + ((n_ss / 2 + 5) * U * v.abs() if norm else 0.0)
    if glu:
        nb = N // 32
        gi = (torch.arange(nb)[:, None] * 32 + torch.arange(16)[None, :]).reshape(-1)
        g, u, e_g, e_u = v[:, gi], v[:, gi + 16], e_v[:, gi], e_v[:, gi + 16]
        if mk == "glu_swap":
            g, u = u, g
        if mk == "glu_rs_one":
            u = P[:, gi + 16]                               # rs applied to the gate half only
        sg = _sigmoid(g)
        s = g * sg
        e_silu = (1.0 - sg) * (2.0 * g.abs() + 2.0) * U + 4.0 * U
        y = s * u
        e_pre = (sg * (1.0 + g * (1.0 - sg))).abs() * e_g * u.abs() + s.abs() * e_u + (e_silu + U) * y.abs()
    else:
        y, e_pre = v, e_v
    if res:
        r = R.double()
        if mk == "res_missing":
            pre = y.clone()
        elif mk == "res_twice":
            pre = r + r + y
        else:
            pre = r + y
        e_pre = e_pre + U * pre.abs()
    else:
        pre = y
    if mk == "tail_col_shift":
        n_out = pre.shape[1]
        t0 = (n_out // 16) * 16
        if t0 < n_out - 1:
            pre = pre.clone()
            pre[:, t0:n_out - 1] = pre[:, t0 + 1:n_out]
    out_bf16 = (kind == "bf16") and not f32out
    pn = pre.numpy()
    if out_bf16:
        out = trunc_bf16(pn) if mk == "trunc_store" else rne_bf16(pn)
        e_out = 2.0 ** -8 * pre.abs()
    else:
        out = rne_f32(pn)
        e_out = U * pre.abs()
    return dict(pre=pre, e_pre=e_pre, bound=2.0 * (e_pre + e_out), out=torch.from_numpy(out), out_bf16=out_bf16)


def check(Y, ref):
    """Y: the stored output (any float tensor, [M][N_out], CPU).  -> dict(ratio: max err / bound (inf where a zero bound is missed),
    decided: elements the exact-rounding predicate decides (bf16 outputs), mismatched: decided elements whose bits are not RNE(pre))"""
    y = Y.double().cpu()
    pre, bound = ref["pre"], ref["bound"]
    err = (y - pre).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.inf, 0.0))
    ratio = torch.where(torch.isnan(y), torch.inf, ratio)
    out = dict(ratio=float(ratio.max()) if ratio.numel() else 0.0, decided=0, total=y.numel(), mismatched=0)
    if ref["out_bf16"]:
        dist = torch.from_numpy(bf16_boundary_distance(pre.numpy()))
        dec = dist > 2.0 * ref["e_pre"]
        want = torch.from_numpy(rne_bf16(pre.numpy()))
        out["decided"] = int(dec.sum())
        out["mismatched"] = int((dec & (y != want)).sum())
    return out


MUTANTS = {   # name -> (mutant tuple, kinds it applies to)
    "dropped line (first of the last wave's slice)": (("drop_line",), KINDS),
    "line staged twice in place of its successor": (("dup_line",), KINDS),
    "row scale of row m ^ 1": (("rs_xor1",), KINDS),
    "eps omitted": (("no_eps",), KINDS),
    "1/(K-1) for 1/K": (("inv_k_minus1",), ("fp32", "x3")),
    "gate and up swapped": (("glu_swap",), KINDS),
    "rs on the gate half only": (("glu_rs_one",), KINDS),
    "residual missing": (("res_missing",), KINDS),
    "residual added twice": (("res_twice",), KINDS),
    "last partial N tile: column n from n + 1": (("tail_col_shift",), KINDS),
    "x3 hi*lo cross term dropped": (("x3_drop_hilo",), ("x3",)),
    "x3 as one bf16 product": (("x3_one_bf16",), ("x3",)),
}
