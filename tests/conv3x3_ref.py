"""The LDS-halo 3x3 convolution (csrc/conv3x3.hip, launch_conv3x3) in fp64: the contract tests/test_gpu_conv3x3.py holds every
instance to, its case table, and the kernel mutants of tests/test_conv3x3_cpu.py.  No GPU import.

Y = epi(conv3x3(in(X))) on NHWC tensors, stride 1, zero padding 1; X [Nb][H][W][Cin], W [N][9 Cin] with K ordered (kh, kw, c).
  in:  identity; nearest-x2 upsampling (nine taps over the upsampled grid, or the SUB-PIXEL form: four 2x2 phase convolutions over X
       with the pre-summed weights of packing.pack_subpixel, phase (py, px) writing the pixels (2y + py, 2x + px)); or the fused input
       GroupNorm h = silu(x * scale[c] + shift[c]) with the padding zero AFTER the normalisation.
  epi: + bias[n], + R (in place), SiLU, ReLU, clamp(0, 1), fp32 or element-type output, and the (sum, sum of squares) per (image,
       group) of the values as stored.
Kinds: "bf16", "fp32", "x3" (fp32 tensors; the kernel splits the staged activations into hi = bf16(x), lo = bf16(x - hi), the weights
arrive split by packing.pack_x3, and the bf16 MFMA forms all four partial products).

Operands.  The reference multiplies exactly what the kernel multiplies: the stored values (bf16, fp32), the split pairs (x3; hi + lo
spans at most 24 bits, so (x_hi + x_lo)(w_hi + w_lo) is exact in fp64 like every other product here), the packed sub-pixel weights as
stored.  The bound then has only the kernel's fp32 arithmetic to cover.

Fused input GroupNorm.  (scale, shift) are read back from the table the device wrote (norm.hip gn_coef_kernel); check_coef holds
that table to fp64 statistics of x on its own.  h = silu(t), t = x * scale + shift in fp64; the kernel evaluates fmaf (one rounding,
u |t|) and common.h silu_t, so with s = silu, sigma the logistic function and e_silu of decode_gemm_ref.py
  e_h = |s'(t)| u |t| + e_silu |h| + 2^-125 (1 + |t|),  e_silu = (1 - sigma)(2 |t| + 2) u + 4 u,  s'(t) = sigma (1 + t (1 - sigma)).
(The last term covers results below the fp32 normal range, which v_exp_f32 / v_rcp_f32 may flush: silu(-100) is stored as -0.)
bf16: the kernel rounds h to bf16.  An input is DECIDED when h lies farther than 2 e_h from every bf16 rounding boundary: every value
the kernel can hold rounds to RNE(h), which enters the convolution.  An undecided input enters as RNE(h) too and adds one bf16 ulp of
h times |w| to the bound of every output that reads it.  fp32: the fp32 value the kernel holds is within e_h of h; x3 adds the split's
residual 2^-17 |h|.  Both enter the bound through a second convolution, E_in = conv(e_in, |w|).

Per-element bound, u = 2^-24, first order, A = conv(|x|, |w|) (x3: (|hi| + |lo|) on both sides; GroupNorm: |h|):
  E_acc = u * n_chain * A.  n_chain is the number of fp32 roundings on one accumulator's path, from the kernel's step loop and the
          plan, not from K: with NT = 9 taps (4: sub-pixel form) and `chunks` channel chunks, bf16 issues one 16x16x32 MFMA per (tap,
          chunk) -- NT * chunks, plus the MFMA's internal depth 32 counted once as decode_gemm_ref.py does; x3 two such MFMAs per
          16 channels per tap -- 2 NT chunks + 32; fp32 four 16x16x4 MFMAs of 4 fused multiply-adds per 16-channel chunk per tap --
          16 NT chunks.
  bias, residual: one fp32 addition each, u |v| of its result.
  SiLU epilogue: E = |s'(v)| E_v + e_silu |s(v)| + 2^-125 (1 + |v|).  ReLU and clamp(0, 1) are 1-Lipschitz: E passes through.
  E_out = 2^-8 |pre| (bf16 store) or 2^-24 |pre| (fp32 store); bound = 2 (E_pre + E_out), twice the first-order estimate.
The constants are derived, not fitted.

Exact rounding (bf16 stores): decode_gemm_ref.check's predicate.  Where the value before ReLU / clamp lies farther than 2 E_pre from
every bf16 boundary the stored bits must equal clamp(RNE(value)) (rounding is monotone and 0, 1 are bf16 numbers, so rounding after
the clamp, as the kernel does, gives the same).  An exact zero with a non-zero E_pre is left undecided (decode_gemm_ref's grid has
no binade for it).

Output statistics: (S1, S2) = sums of y and y^2 over an (image, group) of the values AS STORED.  The epilogue adds a lane's FM pixels
in fp32 (FM = 4; 2 for the 16-channel tile), then four row16_sum levels, then everything in double: FM + 4 fp32 roundings on a path,
bound_S1 = 2 u (FM + 4) sum |y|, bound_S2 = 2 u (FM + 4 + 1) sum y^2 (+1: the square inside the fma is exact, but S2's terms also carry
the conversion of the stored value, exact -- the extra unit is slack for the final double sums, 2^-53 per term).
"""
import numpy as np
import torch
import torch.nn.functional as F

from decode_gemm_ref import U, bf16_boundary_distance, bf16_split, rne_bf16, rne_f32, trunc_bf16, _bf16_grid

IG_BIAS_N, IG_RESIDUAL, IG_SILU, IG_OUT_F32, IG_CLAMP01, IG_RELU = 1, 4, 8, 32, 128, 256
KINDS = ("bf16", "fp32", "x3")
KIND_CODE = {"bf16": 0, "fp32": 1, "x3": 2}
PLAN_FIELDS = ("covered", "kind", "bn", "tw", "ups", "gna", "tpb2", "subpix", "tiles_x", "tiles_per_img", "tiles_n", "chunks", "staged",
               "gn_chunks", "lds_bytes")
EPS = float(np.float32(1e-6))
TINY = 2.0 ** -125


def plan_dict(p):
    return dict(zip(PLAN_FIELDS, (int(v) for v in p)))


def tdt(kind):
    return torch.bfloat16 if kind == "bf16" else torch.float32


def instance(plan):
    """the template instance a plan names: (kind, BN, TW, UPS, GNA, TPB2, SUBPIX)"""
    return (KINDS[plan["kind"]], plan["bn"], plan["tw"], plan["ups"], plan["gna"], plan["tpb2"], plan["subpix"])


# every instance launch_conv3x3 can select, written out from its dispatcher (50 of the 54 compiled)
EXPECTED = (
    {(k, bn, tw, 0, 0, 0, 1) for k in KINDS for bn in (64, 128) for tw in (16, 32)}                       # sub-pixel form
    | {("x3", bn, tw, u, g, 0, 0) for bn in (64, 128) for tw in (16, 32) for (u, g) in ((0, 0), (1, 0), (0, 1))}
    | {("bf16", 16, tw, 0, 1, 0, 0) for tw in (16, 32)}                                                    # the decoders' fused tail
    | {(k, bn, tw, 0, 1, 0, 0) for k in ("bf16", "fp32") for bn in (64, 128) for tw in (16, 32)}           # fused input GroupNorm
    | {("bf16", bn, tw, 0, 0, 1, 0) for bn in (64, 128) for tw in (16, 32)}                                # two steps per barrier
    | {(k, bn, tw, 1, 0, 0, 0) for k in ("bf16", "fp32") for bn in (64, 128) for tw in (16, 32)}           # nine-tap upsampling
    | {("fp32", bn, tw, 0, 0, 0, 0) for bn in (64, 128) for tw in (16, 32)})
# compiled but never selected: plain one-step bf16 -- every plain bf16 call takes the two-step branch first
UNREACHABLE = {("bf16", bn, tw, 0, 0, 0, 0) for bn in (64, 128) for tw in (16, 32)}


def expected_plan(c):
    """launch_conv3x3's dispatch restated from its rules for a case of CASES (aligned operands): the fields a test asserts against
    ivg_op_conv3x3_plan before it launches.  None: refused."""
    kind, H, W, Cin, N = c["kind"], c["H"], c["W"], c["Cin"], c["N"]
    ck = 32 if kind == "bf16" else 16
    if Cin % ck or Cin < ck:
        return None
    ups, gna = c["ups"], c["gn"]
    if ups and gna:
        return None
    sub = bool(ups and c["sub"])
    if sub:
        tw = 32 if W >= 32 else W
        sub = tw in (16, 32) and W % tw == 0 and H % (256 // tw) == 0
    Ht, Wt = (H, W) if sub else ((2 * H, 2 * W) if ups else (H, W))
    tw = 32 if Wt >= 32 else Wt
    if tw not in (16, 32) or Wt % tw or Ht % (256 // tw):
        return None
    bn = 128 if N > 64 else (16 if (N <= 16 and gna and kind == "bf16" and not ups) else 64)
    p = dict(covered=1, kind=KIND_CODE[kind], bn=bn, tw=tw, ups=int(bool(ups) and not sub), gna=int(bool(gna)),
             tpb2=int(kind == "bf16" and not ups and not gna), subpix=int(sub), tiles_x=Wt // tw,
             tiles_per_img=(Wt // tw) * (Ht // (256 // tw)), tiles_n=-(-N // bn), chunks=Cin // ck)
    planar = c["planar"] is not None
    es = 2 if kind == "bf16" else 4
    p["staged"] = int(not planar and not (c["flags"] & IG_OUT_F32) and N % bn == 0 and 256 * (bn * es + 16) <= 80 * 1024)
    p["gn_chunks"] = p["tiles_per_img"] * p["tiles_n"] * (4 if sub else 1) if c["stats"] else 0
    return p


def chain_length(plan):
    nt = 4 if plan["subpix"] else 9
    k = plan["kind"]
    return nt * plan["chunks"] + 32 if k == 0 else (2 * nt * plan["chunks"] + 32 if k == 2 else 16 * nt * plan["chunks"])


def stats_chain(plan):
    return (2 if plan["bn"] == 16 else 4) + 4


# ------------------------------------------------------------------------------------------------ fused input GroupNorm
def _sigmoid(t):
    return 1.0 / (1.0 + torch.exp(-t))


def _silu_err(t, e_t):
    """-> (silu(t), error of common.h silu_t evaluated in fp32 on an argument that is off by e_t)"""
    sg = _sigmoid(t)
    s = t * sg
    e_silu = (1.0 - sg) * (2.0 * t.abs() + 2.0) * U + 4.0 * U
    return s, (sg * (1.0 + t * (1.0 - sg))).abs() * e_t + e_silu * s.abs() + TINY * (1.0 + t.abs())


def coef_reference(x, gamma, beta, groups, n_lane, eps=EPS):
    """fp64 GroupNorm coefficients of x [Nb][H][W][C] and the bound of norm.hip's table (gn_coef_kernel on the partial sums of
    gn_partial_kernel or of a convolution epilogue): sums of n_lane fp32 terms per lane (error n_lane u of sum |x| resp. sum x^2), every
    later sum and the mean / variance in double, then rstd, scale = gamma * rstd, shift = beta - (float)mean * scale in fp32 (one
    rounding each).  -> scale, shift, e_scale, e_shift as fp64 [Nb][C]"""
    Nb, H, W, C = x.shape
    cpg = C // groups
    xg = x.double().reshape(Nb, H * W, groups, cpg)
    cnt = H * W * cpg
    m = xg.sum((1, 3)) / cnt
    m2 = (xg * xg).sum((1, 3)) / cnt
    var = (m2 - m * m).clamp_min(0.0)
    d_m = n_lane * U * xg.abs().sum((1, 3)) / cnt
    d_var = n_lane * U * m2 + 2.0 * m.abs() * d_m
    rstd = 1.0 / torch.sqrt(var + eps)
    r_rstd = d_var / (2.0 * (var + eps)) + 2.0 * U            # relative: the statistics, the cast of eps to double's sum and of rstd
    rep = lambda t: t.repeat_interleave(cpg, 1)               # noqa: E731
    g, b = gamma.double()[None], beta.double()[None]
    scale = g * rep(rstd)
    r_scale = rep(r_rstd) + U
    shift = b - rep(m) * scale
    e_shift = (rep(m).abs() * (r_scale + 2.0 * U) + rep(d_m)) * scale.abs() + U * shift.abs() + U * b.abs()
    return scale, shift, r_scale * scale.abs(), e_shift


def check_coef(coef, x, gamma, beta, groups, n_lane):
    """coef: the device table [Nb][C][2].  -> max err / (2 x bound)"""
    sc, sh, e_sc, e_sh = coef_reference(x, gamma, beta, groups, n_lane)
    c = coef.double()
    r1 = ((c[..., 0] - sc).abs() / (2.0 * e_sc).clamp_min(1e-300)).max()
    r2 = ((c[..., 1] - sh).abs() / (2.0 * e_sh).clamp_min(1e-300)).max()
    return float(max(r1, r2)) if torch.isfinite(c).all() else float("inf")


def coef_model(x, gamma, beta, groups, eps=EPS):
    """the table as the device computes it from exact statistics (fp32 coefficients): the CPU tests' stand-in for the device's"""
    Nb, H, W, C = x.shape
    cpg = C // groups
    xg = x.double().reshape(Nb, H * W, groups, cpg)
    m = (xg.sum((1, 3)) / (H * W * cpg)).repeat_interleave(cpg, 1)
    var = ((xg * xg).sum((1, 3)) / (H * W * cpg)).repeat_interleave(cpg, 1) - m * m
    rstd = (1.0 / torch.sqrt(var.clamp_min(0.0) + eps)).float()
    scf = gamma.float()[None] * rstd
    shf = beta.float()[None] - m.float() * scf
    return torch.stack([scf, shf], -1)


# ------------------------------------------------------------------------------------------------ the reference
def _nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def _w4(w, Cin, taps=3):
    """[N][taps^2 Cin] (kh, kw, c) -> [N][Cin][taps][taps]"""
    return w.reshape(w.shape[0], taps, taps, Cin).permute(0, 3, 1, 2).contiguous()


def _conv(xin, w4, plan, ups):
    """xin NCHW fp64 (already normalised), w4 [N][Cin][3][3] or the sub-pixel [4][N][Cin][2][2] -> NCHW fp64"""
    if plan["subpix"]:
        Nb, _, H, W = xin.shape
        xp = F.pad(xin, (1, 1, 1, 1))
        out = xin.new_zeros(Nb, w4.shape[1], 2 * H, 2 * W)
        for py in range(2):
            for px in range(2):
                out[:, :, py::2, px::2] = F.conv2d(xp[:, :, py:py + H + 1, px:px + W + 1], w4[2 * py + px])
        return out
    if ups:
        xin = F.interpolate(xin, scale_factor=2.0, mode="nearest")
    return F.conv2d(xin, w4, padding=1)


def reference(x, w, kind, plan, *, ups=0, w_sub=None, bias=None, res=None, flags=0, coef=None, stats_groups=0, mutant=None):
    """x [Nb][H][W][Cin], w [N][9 Cin], w_sub [4 N][4 Cin] (sub-pixel plans), res [Nb][Ho][Wo][N]: the stored tensors (x3: fp32; the
    weights unsplit, the reference splits them as pack_x3 does).  bias fp32 [N].  coef [Nb][Cin][2] fp32: the fused input GroupNorm's
    table (None: no normalisation).  plan: plan_dict of ivg_op_conv3x3_plan / expected_plan.
    -> dict(pre, e_pre, bound, out [Nb][Ho][Wo][N] fp64; pre_dec: the value the rounding is decided on; out_bf16; undecided_in: share
    of undecided GroupNorm inputs; stats, stats_bound [Nb][groups][2] of `out` -- check_stats recomputes them from the stored tensor)"""
    mk = mutant[0] if mutant else None
    Nb, H, W, Cin = x.shape
    N = w.shape[0]
    sub = bool(plan["subpix"])
    ck = 32 if kind == "bf16" else 16
    nt = 2 if sub else 3
    wsrc = (w_sub.reshape(4, N, 4 * Cin) if sub else w).double()
    if sub and mk == "phase_transposed":
        wsrc = wsrc[[0, 2, 1, 3]]
    wq = wsrc.reshape(-1, nt * nt, Cin).clone()                 # [N or 4 N][tap][c]
    xs = x.double().clone()
    nch = Cin // ck
    if mk == "drop_step":                                       # (tap 1, last chunk) never multiplied
        wq[:, 1, (nch - 1) * ck:] = 0.0
    if mk == "skip_last_chunk":                                 # the tail of the two-chunk unroll
        wq[:, :, (nch - 1) * ck:] = 0.0
    undecided_in = 0.0
    e_in = None
    cf = None
    if coef is not None:
        cf = coef.double()
        if mk == "coef_xor1":
            cf = cf[:, torch.arange(Cin) ^ 1]
        if mk == "coef_next_image":
            cf = cf.roll(-1, 0)
        t = xs * cf[:, None, None, :, 0] + cf[:, None, None, :, 1]
        h, e_h = _silu_err(t, U * t.abs())
        if kind == "bf16":
            hn = h.numpy()
            und = torch.from_numpy(bf16_boundary_distance(hn)) <= 2.0 * e_h
            undecided_in = float(und.double().mean())
            e_in = torch.where(und, torch.from_numpy(_bf16_grid(hn)[0]), torch.zeros_like(h))
            h = torch.from_numpy(rne_bf16(hn))
        else:
            e_in = e_h + (2.0 ** -17 * h.abs() if kind == "x3" else 0.0)
        xs = h
    if mk == "stale_halo":                                      # chunk c staged again in place of chunk c + 1 (the other halo buffer)
        xs[..., ck:2 * ck] = xs[..., :ck]
    xin = _nchw(xs)
    if kind == "x3":
        wh, wl = bf16_split(wq.float())
        if coef is None:
            xh, xl = bf16_split(xin.float())
        else:
            xh, xl = xin, torch.zeros_like(xin)                 # the split of fl(h) is covered by e_in
        wfull, wabs, xfull, xabs = wh + wl, wh.abs() + wl.abs(), xh + xl, xh.abs() + xl.abs()
    else:
        wfull, wabs, xfull, xabs = wq, wq.abs(), xin, xin.abs()

    def to4(wm):
        if sub:
            return wm.reshape(4, N, 2, 2, Cin).permute(0, 1, 4, 2, 3).contiguous()
        return wm.reshape(N, 3, 3, Cin).permute(0, 3, 1, 2).contiguous()

    P = _conv(xfull, to4(wfull), plan, ups)
    if mk == "x3_drop_hilo":
        P = P - _conv(xh, to4(wl), plan, ups)
    if mk == "pad_normalised" and coef is not None:             # out-of-image halo pixels normalised like the rest: silu(shift)
        pv = F.silu(cf[..., 1])
        pv = torch.from_numpy(rne_bf16(pv.numpy())) if kind == "bf16" else pv
        xp = F.pad(xfull, (1, 1, 1, 1))
        border = torch.ones(1, 1, H + 2, W + 2, dtype=torch.float64)
        border[:, :, 1:-1, 1:-1] = 0.0
        P = F.conv2d(xp + border * pv[:, :, None, None], to4(wfull))
    if mk in ("halo_col", "halo_row"):                          # tile 0's last halo column (row) reads its neighbour inside the tile
        tw, th = plan["tw"], 256 // plan["tw"]
        xp = F.pad(xfull, (1, 1, 1, 1))
        if mk == "halo_col":
            xp[:, :, :, tw + 1] = xp[:, :, :, tw]
        else:
            xp[:, :, th + 1, :] = xp[:, :, th, :]
        Pm = F.conv2d(xp, to4(wfull))
        P = P.clone()
        P[:, :, :th, :tw] = Pm[:, :, :th, :tw]
    A = _conv(xabs, to4(wabs), plan, ups)
    e = U * chain_length(plan) * A
    if e_in is not None:
        e = e + _conv(_nchw(e_in), to4(wabs), plan, ups)
    v = P
    if flags & IG_BIAS_N:
        b = bias.double()
        if mk == "bias_shift":                                  # the last, partial N tile reads bias[n + 1]
            n0 = (N - 1) // plan["bn"] * plan["bn"]
            b = b.clone()
            b[n0:N - 1] = bias.double()[n0 + 1:N]
        v = v + b[None, :, None, None]
        e = e + U * v.abs()
    if flags & IG_RESIDUAL:
        r = _nchw(res.double())
        v = v + (0.0 if mk == "res_missing" else (2.0 * r if mk == "res_twice" else r))
        e = e + U * v.abs()
    if flags & IG_SILU:
        v, e = _silu_err(v, e)
    pre_dec = v
    pre = v
    if flags & IG_RELU:
        pre = pre.clamp_min(0.0)
    if flags & IG_CLAMP01:
        pre = pre.clamp(0.0, 1.0)
    out_bf16 = kind == "bf16" and not (flags & IG_OUT_F32)

    def post(t):
        t = t.clamp_min(0.0) if flags & IG_RELU else t
        return t.clamp(0.0, 1.0) if flags & IG_CLAMP01 else t

    pn = pre_dec.numpy()
    if out_bf16:
        out = post(torch.from_numpy(trunc_bf16(pn) if mk == "trunc_store" else rne_bf16(pn)))
        e_out = 2.0 ** -8 * pre.abs()
    else:
        out = post(torch.from_numpy(rne_f32(pn)))
        e_out = U * pre.abs()
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous()         # noqa: E731
    ref = dict(pre=nhwc(pre), pre_dec=nhwc(pre_dec), e_pre=nhwc(e), bound=nhwc(2.0 * (e + e_out)), out=nhwc(out), out_bf16=out_bf16,
               undecided_in=undecided_in, post=post, plan=plan)
    if stats_groups:
        src = ref["pre"] if mk == "stats_before_rounding" else ref["out"]
        ref["stats"], ref["stats_bound"] = group_stats(src, stats_groups, plan)
        if mk == "stats_missing_wave":                          # pixel wave 0 of tile 0's second N tile never reaches the group sum
            cpg, bn = N // stats_groups, plan["bn"]
            g = bn // cpg                                       # the group that straddles channel bn (when bn % cpg != 0)
            tw = plan["tw"]
            rows = 64 // tw
            part = ref["out"][0, :rows, :tw, bn:(g + 1) * cpg]
            ref["stats"][0, g, 0] -= part.sum()
            ref["stats"][0, g, 1] -= (part * part).sum()
    return ref


def group_stats(y, groups, plan):
    """y [Nb][Ho][Wo][N] fp64 as stored -> (S [Nb][groups][2], bound [Nb][groups][2])"""
    Nb, N = y.shape[0], y.shape[-1]
    yg = y.reshape(Nb, -1, groups, N // groups)
    s1, s2, a1 = yg.sum((1, 3)), (yg * yg).sum((1, 3)), yg.abs().sum((1, 3))
    n = stats_chain(plan)
    return torch.stack([s1, s2], -1), torch.stack([2.0 * U * n * a1, 2.0 * U * (n + 1) * s2], -1)


def check(Y, ref):
    """Y: the stored output [Nb][Ho][Wo][N] (CPU).  -> dict(ratio, decided, total, mismatched) as decode_gemm_ref.check"""
    y = Y.double()
    pre, bound = ref["pre"], ref["bound"]
    err = (y - pre).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.inf, 0.0))
    ratio = torch.where(torch.isfinite(y), ratio, torch.inf)
    out = dict(ratio=float(ratio.max()) if ratio.numel() else 0.0, decided=0, total=y.numel(), mismatched=0)
    if ref["out_bf16"]:
        pd = ref["pre_dec"]
        dec = torch.from_numpy(bf16_boundary_distance(pd.numpy())) > 2.0 * ref["e_pre"]
        dec &= (pd != 0) | (ref["e_pre"] == 0)
        want = ref["post"](torch.from_numpy(rne_bf16(pd.numpy())))
        out["decided"] = int(dec.sum())
        out["mismatched"] = int((dec & (y != want)).sum())
    return out


def check_stats(S, Y, groups, plan):
    """S [Nb][groups][2]: the epilogue's statistics summed over their chunks; Y the stored output.  -> max err / bound"""
    want, bound = group_stats(Y.double(), groups, plan)
    err = (S.double() - want).abs()
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.inf, 0.0))
    return float(torch.where(torch.isfinite(S.double()), r, torch.inf).max())


MUTANTS = {   # name -> (mutant tuple, what the exposing case needs)
    "dropped (tap, chunk) step": ("drop_step",),
    "chunk c + 1 read from chunk c's halo buffer": ("stale_halo",),
    "last chunk of an odd count skipped": ("skip_last_chunk",),
    "halo column off by one at a tile edge": ("halo_col",),
    "halo row off by one at a tile edge": ("halo_row",),
    "padding normalised to silu(shift)": ("pad_normalised",),
    "coefficients of channel c ^ 1": ("coef_xor1",),
    "coefficients of the next image": ("coef_next_image",),
    "sub-pixel phase (py, px) transposed": ("phase_transposed",),
    "x3 hi*lo term dropped": ("x3_drop_hilo",),
    "bias of column n + 1 in the last partial N tile": ("bias_shift",),
    "residual missing": ("res_missing",),
    "residual added twice": ("res_twice",),
}
STATS_MUTANTS = {
    "statistics taken before the output rounding": ("stats_before_rounding",),
    "statistics missing one pixel wave of a straddling group": ("stats_missing_wave",),
}


# ------------------------------------------------------------------------------------------------ the case table
def case(kind, H, W, Cin, N, *, ups=0, sub=1, gn=0, stats=0, res=0, flags=IG_BIAS_N, cls="random", Nb=1, planar=None, cap=0, src="partial"):
    """H x W: the INPUT image.  sub: IVG_SUBPIXEL (upsampling cases).  gn: input GroupNorm groups (0: none); src: its statistics from
    "partial" (a pass over x) or "conv" (the epilogue of a preceding convolution).  stats: output statistics groups.  planar: None
    (dense NHWC) or (per, T, t0, out): planar frames [B][T][N][Ho][Wo] written at frame offset t0, `per` images per clip (c_grp), out
    "fp32" | "bf16".  cap: IVG_CONV_CAP."""
    fl = flags | (IG_RESIDUAL if res else 0) | (IG_OUT_F32 if planar and planar[3] == "fp32" else 0)
    return dict(kind=kind, H=H, W=W, Cin=Cin, N=N, ups=ups, sub=sub, gn=gn, stats=stats, res=res, flags=fl, cls=cls, Nb=Nb, planar=planar,
                cap=cap, src=src)


def case_id(c):
    s = f"{c['kind']}-{c['H']}x{c['W']}-C{c['Cin']}-N{c['N']}-{c['cls']}-b{c['Nb']}"
    s += ("-sub" if c["sub"] else "-ups9") if c["ups"] else ""
    s += f"-gn{c['gn']}{c['src'][0]}" if c["gn"] else ""
    s += f"-st{c['stats']}" if c["stats"] else ""
    s += f"-f{c['flags']}" + ("-planar" + c["planar"][3] if c["planar"] else "") + ("-cap" if c["cap"] else "")
    return s


def _cases():
    B, R, C01 = IG_BIAS_N, IG_RELU, IG_CLAMP01
    out = []
    # ---- plain bf16 (two steps per barrier): chunk counts 1, 2, 3, 5, 8, 24; N = 64, 65, 192, 17, 768, 66, 3; non-square images
    out += [case("bf16", 16, 16, 32, 64, Nb=3), case("bf16", 8, 32, 64, 65, res=1), case("bf16", 32, 16, 96, 192, Nb=3, stats=32, res=1),
            case("bf16", 24, 64, 160, 17, cls="scaled", Nb=2), case("bf16", 24, 96, 32, 64, Nb=3, stats=32),
            case("bf16", 16, 96, 256, 66, cls="sparse"), case("bf16", 16, 96, 256, 66), case("bf16", 8, 32, 512, 64, cls="sparse"),
            case("bf16", 8, 32, 512, 64), case("bf16", 16, 16, 768, 64), case("bf16", 16, 16, 768, 64, cls="sparse"),
            case("bf16", 16, 16, 768, 768, cls="sparse", stats=32, res=1), case("bf16", 16, 16, 768, 768, stats=32, res=1),
            case("bf16", 32, 32, 32, 3, Nb=6, planar=(3, 5, 2, "fp32"), flags=B | C01), case("bf16", 16, 16, 64, 3, flags=B | IG_SILU),
            case("bf16", 16, 16, 64, 16, cap=1, Nb=2)]
    # ---- plain fp32 (ReLU: the LPIPS trunk) and x3: chunks of 16 channels
    for k in ("fp32", "x3"):
        f = B | R if k == "fp32" else B
        out += [case(k, 16, 16, 16, 64, Nb=3, flags=f), case(k, 8, 32, 48, 65, res=1, flags=f), case(k, 32, 16, 80, 192, stats=32, flags=f, Nb=2),
                case(k, 24, 64, 128, 16, flags=f, cls="scaled", Nb=2), case(k, 16, 16, 384, 768, stats=32, res=1, cls="scaled"),
                case(k, 16, 96, 32, 3, Nb=6, planar=(3, 4, 1, "fp32"), flags=B | (C01 if k == "fp32" else 0))]
    # ---- upsampling: sub-pixel form (tiles over the input), nine taps under IVG_SUBPIXEL=0, and the untileable 8 x 16 and 8 x 8 inputs
    for k in KINDS:
        c1, c3, c5 = (32, 96, 512) if k == "bf16" else (16, 48, 256)
        out += [case(k, 16, 16, c3, 64, ups=1, Nb=3), case(k, 32, 16, c1, 192, ups=1, stats=32, Nb=2), case(k, 8, 32, 2 * c1, 64, ups=1),
                case(k, 16, 64, c1, 128, ups=1, res=1, stats=32),
                case(k, 8, 8, c3, 64, ups=1, Nb=3), case(k, 16, 8, c1, 192, ups=1, stats=32, res=1), case(k, 8, 16, 2 * c1, 3, ups=1, Nb=2),
                case(k, 16, 16, c1, 128, ups=1, sub=0, res=1, Nb=2)]
        out += [case(k, 16, 16, c5, 128, ups=1, cls="sparse")]
    out += [case("bf16", 16, 16, 512, 128, ups=1), case("bf16", 16, 16, 512, 128, ups=1, sub=0, cls="sparse")]
    # ---- fused input GroupNorm; the production triple (+ output statistics + in-place residual) at 64- and 128-wide tiles, statistics
    # of the input from a pass over it and from a preceding convolution's epilogue (conv1 -> conv2 of a resnet block)
    for k in KINDS:
        c2, c3, c8, c24 = (64, 96, 256, 768) if k == "bf16" else (32, 48, 128, 384)
        g3 = 32 if k == "bf16" else 16
        out += [case(k, 16, 16, c2, 64, gn=32, stats=32, res=1, Nb=3, cls="gn_edge"), case(k, 8, 32, 2 * c2, 64, gn=32, stats=32, res=1, src="conv"),
                case(k, 32, 16, c3, 128, gn=g3, stats=32, res=1, Nb=2, cls="scaled"), case(k, 24, 64, c8, 192, gn=32, stats=32, res=1, src="conv"),
                case(k, 16, 16, c24, 768, gn=32, stats=32, res=1, src="conv", cls="gn_edge"), case(k, 16, 96, c2, 65, gn=32, Nb=2)]
    out += [case("bf16", 24, 64, 256, 192, gn=32, stats=32, res=1, cls="sparse"), case("bf16", 16, 16, 768, 768, gn=32, stats=32, res=1, cls="sparse"),
            case("bf16", 16, 16, 768, 64, gn=32, cls="sparse"), case("bf16", 16, 16, 768, 64, gn=32),
            case("bf16", 16, 16, 128, 128, gn=32, stats=32, res=1, cap=1, Nb=2)]
    # ---- the decoders' fused tail (16-channel tile): planar fp32 / bf16 frames at an offset, with and without clamp; dense N = 16, 3
    out += [case("bf16", 32, 32, 128, 3, gn=32, Nb=6, planar=(3, 5, 2, "fp32"), flags=B | C01, cls="gn_edge"),
            case("bf16", 16, 16, 64, 3, gn=32, Nb=4, planar=(2, 3, 1, "bf16")), case("bf16", 16, 16, 64, 16, gn=32, Nb=2),
            case("bf16", 8, 32, 32, 3, gn=32, Nb=3, flags=B | C01)]
    return out


CASES = _cases()


def make_inputs(c):
    """the seeded tensors of a case as stored: x [Nb][H][W][Cin], w [N][9 Cin], w_sub [4 N][4 Cin] (upsampling), bias, res, gamma, beta"""
    from ivideogpt_amd.packing import pack_subpixel
    kind, H, W, Cin, N, Nb, cls = c["kind"], c["H"], c["W"], c["Cin"], c["N"], c["Nb"], c["cls"]
    g = torch.Generator().manual_seed(H * 7 + W * 3 + Cin + N + len(cls))
    dt = tdt(kind)
    x = torch.randn(Nb, H, W, Cin, generator=g) * 1.3 + 0.2
    w4 = torch.randn(N, Cin, 3, 3, generator=g) / (Cin * 9) ** 0.5
    gamma, beta = 1 + 0.2 * torch.randn(Cin, generator=g), 0.2 * torch.randn(Cin, generator=g)
    if cls == "sparse":
        # Sparse K, in the WEIGHTS: row n is non-zero in every third chunk only, there in one tap and one channel slot, all three varying
        # with (n, chunk), so an output sums about chunks / 3 terms and the union over n uses every tap, chunk and slot
        # (test_conv3x3_cpu.py asserts the union).  This departs from a sparse INPUT with one non-zero channel per chunk: such an input
        # decides 0.94 - 0.96 of the outputs of a plain convolution at Cin 512 / 768 under this bound, but it does not survive a fused
        # input GroupNorm (a zero enters the convolution as silu(shift) != 0), and the fused-GroupNorm instances are the ones that run at
        # Cin >= 256.  Sparse weights reach every instance, so the table uses this one class throughout.
        ck = 32 if kind == "bf16" else 16
        nch = Cin // ck
        n, ch = torch.meshgrid(torch.arange(N), torch.arange(nch), indexing="ij")
        on = ((n + ch) % 3 == 0)
        idx = ((n * 5 + ch) % 9) * Cin + ch * ck + (n * 11 + ch * 7) % ck          # (tap, channel) of the kept element
        keep = torch.zeros(N, 9 * Cin, dtype=torch.bool)
        keep[n[on], idx[on]] = True
        w4 = w4 * keep.reshape(N, 3, 3, Cin).permute(0, 3, 1, 2) * (27.0 * ck) ** 0.5
    if cls in ("scaled", "gn_edge") and Nb >= 2:
        x[1] = 0.0            # an all-zero image
    if cls == "scaled":
        x = x * 2.0 ** (((torch.arange(Cin) * 5) % 17) - 8).float()
    if cls == "gn_edge":
        cpg = Cin // c["gn"]
        x[0, ..., :cpg] = 30.0 + 0.5 * torch.randn(H, W, cpg, generator=g)       # a group whose mean dwarfs its spread
        gamma[cpg:2 * cpg] = 60.0                                                   # pre-activations beyond +-100
        gamma[2 * cpg:3 * cpg] = -60.0
    bias = torch.randn(N, generator=g) * (0.3 if c["flags"] & IG_CLAMP01 else 1.0) + (0.4 if c["flags"] & IG_CLAMP01 else 0.0)
    Ho, Wo = (2 * H, 2 * W) if c["ups"] else (H, W)
    res = torch.randn(Nb, Ho, Wo, N, generator=g).to(dt) if c["res"] else None
    w4 = w4.to(dt)
    d = dict(x=x.to(dt), w=w4.permute(0, 2, 3, 1).reshape(N, -1).contiguous(), bias=bias, res=res, gamma=gamma, beta=beta, w_sub=None)
    if c["ups"]:
        d["w_sub32"] = pack_subpixel(w4.float())
        d["w_sub"] = d["w_sub32"].to(dt)
    return d


def case_reference(c, plan, inp, coef=None, mutant=None):
    if c["gn"] and coef is None:
        coef = coef_model(inp["x"], inp["gamma"], inp["beta"], c["gn"])
    return reference(inp["x"], inp["w"], c["kind"], plan, ups=c["ups"], w_sub=inp["w_sub"], bias=inp["bias"], res=inp["res"], flags=c["flags"],
                     coef=coef, stats_groups=c["stats"], mutant=mutant)
