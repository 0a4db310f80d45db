"""The LDS-halo 3x3 convolution at op level against fp64, per element, at every instance launch_conv3x3 can select (ivg_op_conv3x3:
that kernel alone, with every option of a production launch at once; ivg_op_conv3x3_plan names the instance without launching).

Reference, bound, case table and inputs: tests/conv3x3_ref.py (module docstring: operands, the fused input GroupNorm, the per-element
bound and its derivation, the exact-rounding predicate, the statistics bound).  tests/test_conv3x3_cpu.py shows on the CPU that the
bound rejects each kernel mutant by >= 10x and that the predicates decide enough elements on these very inputs.

Every case asserts its plan against the dispatcher's rules (conv3x3_ref.expected_plan) before it launches, then:
  - every element within its bound, every bf16 element the predicate decides equal to RNE of the fp64 value;
  - the output NaN before and finite after; the guard images before and after it (planar: the frames outside [t0, t0 + per)) untouched;
  - the (scale, shift) table of a fused input GroupNorm within its own bound of fp64 statistics;
  - the epilogue's output statistics within their bound of the sums over the tensor as stored, the entries past the plan's chunks untouched.
"""
import ctypes as C
import time

import pytest
import torch

import conv3x3_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STATS = {}
T0 = time.time()


def lib():
    from ivideogpt_amd import _lib
    return _lib, _lib.load()


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def args_of(L, c, X, W, Y, Rp, bias, **over):
    H, Wd, Cin, N, Nb = c["H"], c["W"], c["Cin"], c["N"], c["Nb"]
    Ho, Wo = (2 * H, 2 * Wd) if c["ups"] else (H, Wd)
    a = L.IvgIgemmArgs()
    a.X, a.W, a.Y, a.R, a.bias = X, W, Y, Rp, bias
    kw = dict(Nimg=Nb, Hin=H, Win=Wd, Cin=Cin, ldx=Cin, Hout=Ho, Wout=Wo, KH=3, KW=3, stride=1, pad=1, ups=c["ups"], N=N, ldw=9 * Cin,
              c_img=Ho * Wo * N, c_pix=N, c_ch=1, c_grp=1, c_grp_stride=0, flags=c["flags"], alpha=1.0, nb0=1, nb1=1, nb2=1)
    if c["planar"]:
        per, T, _, _ = c["planar"]
        kw.update(c_img=N * Ho * Wo, c_pix=1, c_ch=Ho * Wo, c_grp=per, c_grp_stride=T * N * Ho * Wo)
    kw.update(over)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def plan_of(l, a, kind, gn_in, groups, w_x3=None, w_sub=None, w_sub_x3=None):
    out = (C.c_int32 * 15)()
    assert l.ivg_op_conv3x3_plan(C.byref(a), 1 if kind == "bf16" else 0, gn_in, groups, w_x3, w_sub, w_sub_x3, out) == 0
    return R.plan_dict(out)


def identity_conv_statistics(L, l, c, xd):
    """conv1 of a resnet block, reduced to the identity (centre tap = I): h == x bit for bit, and the statistics of h come out of a
    convolution epilogue -- what conv2's fused GroupNorm reads in Run::resnet.  -> (part, chunks per image)"""
    Cin, Nb, H, Wd, g = c["Cin"], c["Nb"], c["H"], c["W"], c["gn"]
    wid = torch.zeros(Cin, 9, Cin, dtype=xd.dtype, device=DEV)
    wid[:, 4] = torch.eye(Cin, dtype=xd.dtype, device=DEV)
    wid = wid.reshape(Cin, 9 * Cin)
    h = torch.full_like(xd, float("nan"))
    c1 = dict(c, N=Cin, ups=0, flags=0, planar=None)
    a = args_of(L, c1, xd.data_ptr(), wid.data_ptr(), h.data_ptr(), None, None)
    bound = ((H * Wd + 255) // 256) * ((Cin + 63) // 64)
    part = torch.full((Nb * bound * g * 2,), float("nan"), dtype=torch.float64, device=DEV)
    rc = l.ivg_op_conv3x3(C.byref(a), 1 if c["kind"] == "bf16" else 0, None, None, 0, 1e-6, None, None, 0, P(part), g, None, None, None, stream())
    torch.cuda.synchronize()
    assert 0 < rc <= bound, rc
    assert torch.equal(h.view(torch.int16 if h.dtype == torch.bfloat16 else torch.int32), xd.view(torch.int16 if h.dtype == torch.bfloat16 else torch.int32))
    return part, rc


def run_case(c, switches):
    from ivideogpt_amd.packing import pack_x3
    L, l = lib()
    switches(IVG_SUBPIXEL="1" if c["sub"] else "0", IVG_CONV_CAP="1" if c["cap"] else None, IVG_CONV3X3=None)
    kind, H, Wd, Cin, N, Nb, flags = c["kind"], c["H"], c["W"], c["Cin"], c["N"], c["Nb"], c["flags"]
    Ho, Wo = (2 * H, 2 * Wd) if c["ups"] else (H, Wd)
    x3 = kind == "x3"
    inp = R.make_inputs(c)
    xd, wd, bd = inp["x"].to(DEV), inp["w"].to(DEV), inp["bias"].to(DEV)
    w3 = pack_x3(wd) if x3 else None
    wsub = inp["w_sub"].to(DEV) if c["ups"] else None
    wsub3 = pack_x3(inp["w_sub32"].to(DEV)) if (c["ups"] and x3) else None
    odt = torch.float32 if (flags & R.IG_OUT_F32 or kind != "bf16") else torch.bfloat16
    # ---- output with guards
    if c["planar"]:
        per, T, t0, _ = c["planar"]
        Bc = Nb // per
        clip = torch.full((Bc, T, N, Ho, Wo), -7.0, device=DEV, dtype=odt)
        clip[:, t0:t0 + per] = float("nan")
        yptr = clip.view(-1)[t0 * N * Ho * Wo:].data_ptr()
    else:
        buf = torch.full((Nb + 2, Ho, Wo, N), float("nan"), device=DEV, dtype=odt)
        if c["res"]:
            buf[1:Nb + 1] = inp["res"].to(DEV)
        yptr = buf[1].data_ptr()
    a = args_of(L, c, xd.data_ptr(), wd.data_ptr(), yptr, yptr if c["res"] else None, bd.data_ptr())
    # ---- the plan, asserted before anything is launched
    plan = plan_of(l, a, kind, 1 if c["gn"] else 0, c["stats"], P(w3), P(wsub), P(wsub3))
    want = R.expected_plan(c)
    assert want is not None and plan["covered"] == 1, (c, plan)
    assert {k: plan[k] for k in want} == want, (c, plan, want)
    assert (82 * 1024 if c["cap"] else 1) <= plan["lds_bytes"] <= 160 * 1024
    # ---- fused input GroupNorm: workspace as ivg_op_gn_conv lays it out
    ws = coef = in_part = None
    in_chunks, n_lane = 0, 0
    if c["gn"]:
        nch = (H * Wd + 1023) // 1024
        off = Nb * nch * c["gn"] * 16
        ws = torch.full((off + Nb * Cin * 8 + 256,), 0xFF, dtype=torch.uint8, device=DEV)
        if c["src"] == "conv":
            in_part, in_chunks = identity_conv_statistics(L, l, c, xd)
            n_lane = 8                                            # FM + 4 fp32 roundings of the epilogue (conv3x3_ref.stats_chain)
        else:
            vpp = Cin // (8 if kind == "bf16" else 4)
            n_lane = -(-min(H * Wd, 1024) // (256 // vpp))        # pixels one lane of gn_partial_kernel adds in fp32
    part = None
    if c["stats"]:
        bound = ((Ho * Wo + 255) // 256) * ((N + 63) // 64)
        part = torch.full((Nb * bound * c["stats"] * 2 + 8,), float("nan"), dtype=torch.float64, device=DEV)
    gd, btd = (inp["gamma"].to(DEV), inp["beta"].to(DEV)) if c["gn"] else (None, None)
    rc = l.ivg_op_conv3x3(C.byref(a), 1 if kind == "bf16" else (2 if x3 else 0), P(gd), P(btd), c["gn"], 1e-6, P(ws), P(in_part), in_chunks,
                          P(part), c["stats"], P(w3), P(wsub), P(wsub3), stream())
    torch.cuda.synchronize()
    assert rc == plan["gn_chunks"], (rc, plan)
    # ---- what was written, and where
    if c["planar"]:
        got = clip[:, t0:t0 + per].reshape(Nb, N, Ho, Wo).permute(0, 2, 3, 1).cpu()
        outside = torch.cat([clip[:, :t0].reshape(-1), clip[:, t0 + per:].reshape(-1)])
        assert (outside.float() == -7.0).all(), "frames outside the written range changed"
    else:
        got = buf[1:Nb + 1].cpu()
        assert torch.isnan(buf[0].float()).all() and torch.isnan(buf[Nb + 1].float()).all(), "guard images were written"
    assert torch.isfinite(got.float()).all(), "an output element was not written"
    ratio_c = 0.0
    if c["gn"]:
        coef = ws[off:off + Nb * Cin * 8].view(torch.float32).view(Nb, Cin, 2).cpu()
        ratio_c = R.check_coef(coef, inp["x"], inp["gamma"], inp["beta"], c["gn"], n_lane)
    ref = R.case_reference(c, plan, inp, coef=coef)
    res = R.check(got, ref)
    ratio_s = 0.0
    if c["stats"]:
        used = Nb * rc * c["stats"] * 2
        assert torch.isnan(part[used:]).all(), "statistics beyond the plan's chunks were written"
        S = part[:used].view(Nb, rc, c["stats"], 2).sum(1).cpu()
        ratio_s = R.check_stats(S, got, c["stats"], plan)
    key = R.instance(plan)
    s = STATS.setdefault(key, dict(ratio=0.0, coef=0.0, stats=0.0, decided=0, total=0, cases=0))
    s["ratio"], s["coef"], s["stats"] = max(s["ratio"], res["ratio"]), max(s["coef"], ratio_c), max(s["stats"], ratio_s)
    s["decided"] += res["decided"]
    s["total"] += res["total"] if ref["out_bf16"] else 0
    s["cases"] += 1
    print(f"CONV3_STAT {R.case_id(c)} {key} ratio {res['ratio']:.3f} coef {ratio_c:.3f} stats {ratio_s:.3f} decided {res['decided']}/{res['total']} "
          f"mismatched {res['mismatched']} undecided_in {ref['undecided_in']:.2e}")
    assert ratio_c <= 1.0, (R.case_id(c), "coefficient table", ratio_c)
    assert res["ratio"] <= 1.0, (R.case_id(c), res)
    assert res["mismatched"] == 0, (R.case_id(c), res)
    assert ratio_s <= 1.0, (R.case_id(c), "statistics", ratio_s)
    if c["gn"]:
        assert ref["undecided_in"] <= 0.01


@pytest.mark.parametrize("c", R.CASES, ids=[R.case_id(c) for c in R.CASES])
def test_case(c, switches):
    run_case(c, switches)


def test_plan_coverage(switches):
    """the plans of the case table, asked of the library, are exactly every instance the dispatcher can select"""
    L, l = lib()
    reached = set()
    for c in R.CASES:
        switches(IVG_SUBPIXEL="1" if c["sub"] else "0", IVG_CONV_CAP="1" if c["cap"] else None, IVG_CONV3X3=None)
        a = args_of(L, c, 4096, 4096, 4096, None, None)
        x3 = C.c_void_p(4096) if c["kind"] == "x3" else None
        sub = C.c_void_p(4096) if c["ups"] else None
        p = plan_of(l, a, c["kind"], 1 if c["gn"] else 0, c["stats"], x3, sub, sub if x3 else None)
        assert p["covered"] == 1, c
        reached.add(R.instance(p))
    assert reached == R.EXPECTED, (R.EXPECTED - reached, reached - R.EXPECTED)
    assert not reached & R.UNREACHABLE
    print(f"CONV3_COVER {len(reached)} of {len(R.EXPECTED)} reachable instances ({len(R.UNREACHABLE)} compiled but shadowed)")


def test_refusals_leave_the_output_untouched(switches):
    """a misaligned X or W, ldx != Cin, Cin % 16 != 0, a 48-wide image, stride 2, and Cin = 0 (the kernel's prologue stages channel
    chunk 0 before it looks at the chunk count, so the plan refuses what the old launcher would have launched out of bounds): covered =
    0, and the op answers IVG_ERR_INVALID without writing (neither the output nor the GroupNorm workspace)"""
    L, l = lib()
    switches(IVG_SUBPIXEL=None, IVG_CONV_CAP=None, IVG_CONV3X3=None)
    for kind in ("bf16", "fp32"):
        dt = R.tdt(kind)
        es = 2 if kind == "bf16" else 4
        Cin, N = 64, 64
        xbuf = torch.randn(16 * 48 * Cin + 64, device=DEV).to(dt)
        wbuf = torch.randn(N * 9 * Cin + 64, device=DEV).to(dt)
        Y = torch.full((16 * 48 * N,), 3.0, device=DEV, dtype=dt)
        ws = torch.full((1 << 16,), 0x5A, dtype=torch.uint8, device=DEV)
        gam = torch.ones(Cin + 8, device=DEV)
        base = R.case(kind, 16, 16, Cin, N)
        good = args_of(L, base, xbuf.data_ptr(), wbuf.data_ptr(), Y.data_ptr(), None, None, flags=0)
        assert plan_of(l, good, kind, 0, 0)["covered"] == 1
        bad = {
            "misaligned X": args_of(L, base, xbuf.data_ptr() + es, wbuf.data_ptr(), Y.data_ptr(), None, None, flags=0),
            "misaligned W": args_of(L, base, xbuf.data_ptr(), wbuf.data_ptr() + es, Y.data_ptr(), None, None, flags=0),
            "ldx != Cin": args_of(L, base, xbuf.data_ptr(), wbuf.data_ptr(), Y.data_ptr(), None, None, flags=0, ldx=Cin + 8),
            "Cin % 16 != 0": args_of(L, base, xbuf.data_ptr(), wbuf.data_ptr(), Y.data_ptr(), None, None, flags=0, Cin=56, ldx=56, ldw=9 * 56),
            "48-wide image": args_of(L, dict(base, W=48), xbuf.data_ptr(), wbuf.data_ptr(), Y.data_ptr(), None, None, flags=0),
            "stride 2": args_of(L, base, xbuf.data_ptr(), wbuf.data_ptr(), Y.data_ptr(), None, None, flags=0, stride=2),
            "Cin == 0": args_of(L, base, xbuf.data_ptr(), wbuf.data_ptr(), Y.data_ptr(), None, None, flags=0, Cin=0, ldx=0, ldw=0),
        }
        for name, a in bad.items():
            for gn in (0, 1):
                assert plan_of(l, a, kind, gn, 0)["covered"] == 0, (kind, name)
                rc = l.ivg_op_conv3x3(C.byref(a), 1 if kind == "bf16" else 0, P(gam) if gn else None, P(gam) if gn else None, 8 if gn else 0, 1e-6,
                                      P(ws) if gn else None, None, 0, None, 0, None, None, None, stream())
                assert rc == -1, (kind, name, rc)
        # split-bf16 weights with bf16 tensors: invalid
        out = (C.c_int32 * 15)()
        assert l.ivg_op_conv3x3_plan(C.byref(good), 1 if kind == "bf16" else 0, 0, 0, P(wbuf), None, None, out) == 0 and out[0] == (-1 if kind == "bf16" else 1)
        assert l.ivg_op_conv3x3_plan(C.byref(good), 3, 0, 0, None, None, None, out) == -1
        torch.cuda.synchronize()
        assert (Y.float() == 3.0).all() and (ws == 0x5A).all()
    switches(IVG_CONV3X3="0")
    assert plan_of(l, good, "fp32", 0, 0)["covered"] == 0


def test_zz_report():
    for key in sorted(STATS):
        s = STATS[key]
        frac = f"{s['decided'] / s['total']:.4f}" if s["total"] else "-"
        print(f"CONV3_WORST {key}: cases {s['cases']}, err/bound {s['ratio']:.3f}, coefficients {s['coef']:.3f}, statistics {s['stats']:.3f}, "
              f"exact-rounding decided {frac}")
    print(f"CONV3_TIME {time.time() - T0:.1f} s since import")
    if sum(s["cases"] for s in STATS.values()) == len(R.CASES):   # the whole table ran: every reachable instance was launched
        assert set(STATS) == R.EXPECTED, R.EXPECTED - set(STATS)
