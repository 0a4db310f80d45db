"""Op-level parity: every hand-written kernel, called through the C ABI (include/ivg.h), against a plain
fp32/fp64 PyTorch-CPU statement of the same op.  Runs on the MI355X only (-m gpu)."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = {"fp32": 2e-5, "bf16": 2e-2}   # relative to the output scale (bf16: inputs rounded once + bf16 output)


def lib():
    from ivideogpt_amd import _lib
    return _lib, _lib.load()


def tdt(name):
    return torch.float32 if name == "fp32" else torch.bfloat16


def code(name):
    return {"fp32": 0, "bf16": 1, "x3": 2}[name]   # x3 = IVG_F32X3: fp32 tensors, split-bf16 arithmetic


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def rel_err(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-12)).item()


def igemm(dt, X, W, Y, R=None, bias=None, halo=None, **kw):
    """halo: True / False -- assert through the plan hook that the LDS-halo 3x3 kernel (conv3x3.hip) resp. the fall-back serves the call"""
    L, l = lib()
    a = L.IvgIgemmArgs()
    a.X, a.W, a.Y, a.R, a.bias = X.data_ptr(), W.data_ptr(), Y.data_ptr(), (R.data_ptr() if R is not None else None), \
        (bias.data_ptr() if bias is not None else None)
    defaults = dict(Nimg=1, Hin=1, Win=1, Cin=0, ldx=0, Hout=1, Wout=1, KH=1, KW=1, stride=1, pad=0, ups=0, N=0, ldw=0,
                    c_img=0, c_pix=0, c_ch=1, c_grp=1, c_grp_stride=0, flags=0, alpha=1.0, nb0=1, nb1=1, nb2=1)
    defaults.update(kw)
    for k, v in defaults.items():
        if k in ("sa", "sw", "sy"):
            continue
        setattr(a, k, v)
    for name in ("sa", "sw", "sy"):
        for i, v in enumerate(kw.get(name, (0, 0, 0))):
            getattr(a, name)[i] = v
    if halo is not None:
        plan = (C.c_int32 * 15)()
        assert l.ivg_op_conv3x3_plan(C.byref(a), code(dt), 0, 0, None, None, None, plan) == 0
        assert (plan[0] == 1) == halo, f"conv3x3 plan covered = {plan[0]}, expected the {'halo kernel' if halo else 'fall-back'}"
    rc = l.ivg_op_igemm(C.byref(a), code(dt), stream())
    assert rc == 0, f"ivg_op_igemm rc={rc}"
    torch.cuda.synchronize()


def q(t, dt):
    """round through the kernel's storage type (so the CPU reference sees the same inputs)"""
    return t.to(tdt(dt)).float()


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("M,N,K", [(300, 200, 256), (128, 128, 64), (1000, 48, 192), (77, 16386, 128)])
def test_gemm_bias_residual(dt, M, N, K):
    g = torch.Generator().manual_seed(M + N + K)
    X, W_, R, b = q(torch.randn(M, K, generator=g), dt), q(torch.randn(N, K, generator=g), dt), q(torch.randn(M, N, generator=g), dt), torch.randn(N, generator=g)
    ref = X.double() @ W_.double().T + b.double() + R.double()
    Xd, Wd, Rd, bd = X.to(DEV, tdt(dt)), W_.to(DEV, tdt(dt)), R.to(DEV, tdt(dt)), b.to(DEV)
    Y = torch.full((M, N), float("nan"), device=DEV, dtype=tdt(dt))
    igemm(dt, Xd, Wd, Y, Rd, bd, Win=M, Wout=M, Cin=K, ldx=K, N=N, ldw=K, c_pix=N, flags=1 | 4)
    assert rel_err(Y.float(), ref) < TOL[dt]


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("mode", ["s1", "s2", "ups", "k1", "patch4"])
def test_conv_modes(dt, mode):
    g = torch.Generator().manual_seed(7)
    Nb, H, Cin, Cout = 3, 16, 64, 128
    x = q(torch.randn(Nb, Cin, H, H, generator=g), dt)
    k = {"s1": 3, "s2": 3, "ups": 3, "k1": 1, "patch4": 4}[mode]
    w = q(torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5, dt)
    b = torch.randn(Cout, generator=g)
    xd = x.double()
    if mode == "s1":
        ref, Ho, stride, pad, ups = F.conv2d(xd, w.double(), b.double(), padding=1), H, 1, 1, 0
    elif mode == "s2":
        ref, Ho, stride, pad, ups = F.conv2d(F.pad(xd, (0, 1, 0, 1)), w.double(), b.double(), stride=2), H // 2, 2, 0, 0
    elif mode == "ups":
        ref, Ho, stride, pad, ups = F.conv2d(F.interpolate(xd, scale_factor=2.0, mode="nearest"), w.double(), b.double(), padding=1), 2 * H, 1, 1, 1
    elif mode == "k1":
        ref, Ho, stride, pad, ups = F.conv2d(xd, w.double(), b.double()), H, 1, 0, 0
    else:
        ref, Ho, stride, pad, ups = F.conv2d(xd, w.double(), b.double(), stride=4), H // 4, 4, 0, 0
    X = x.permute(0, 2, 3, 1).contiguous().to(DEV, tdt(dt))
    Wp = w.permute(0, 2, 3, 1).reshape(Cout, -1).contiguous().to(DEV, tdt(dt))
    Y = torch.full((Nb, Ho, Ho, Cout), float("nan"), device=DEV, dtype=tdt(dt))
    igemm(dt, X, Wp, Y, None, b.to(DEV), halo=mode in ("s1", "ups"), Nimg=Nb, Hin=H, Win=H, Cin=Cin, ldx=Cin, Hout=Ho, Wout=Ho, KH=k, KW=k,
          stride=stride, pad=pad, ups=ups, N=Cout, ldw=k * k * Cin, c_img=Ho * Ho * Cout, c_pix=Cout, flags=1)
    assert rel_err(Y.float().permute(0, 3, 1, 2), ref) < TOL[dt]


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("H,Cin,Cout,ups,res", [(64, 128, 128, 0, 1), (32, 256, 512, 0, 0), (16, 512, 512, 1, 0), (32, 128, 64, 1, 1),
                                                 (128, 64, 128, 0, 0), (16, 64, 192, 0, 1), (16, 96, 128, 0, 0), (32, 32, 64, 0, 1),
                                                 (16, 160, 64, 1, 0), (64, 32, 128, 1, 1)])
def test_conv3x3_halo_kernel(dt, H, Cin, Cout, ups, res):
    """the LDS-halo 3x3 kernel (conv3x3.hip): both tile shapes (16x16 / 8x32), one to sixteen K chunks incl. ODD chunk counts
    (the step loop is unrolled over two chunks, two steps per barrier for bf16: the tail of the last group), several N tiles,
    ragged N (192 = 128 + 64), nearest-x2 upsampling folded into the halo gather, bias + in-place residual"""
    g = torch.Generator().manual_seed(H + Cin + Cout)
    Nb = 3
    x = q(torch.randn(Nb, Cin, H, H, generator=g), dt)
    w = q(torch.randn(Cout, Cin, 3, 3, generator=g) / (Cin * 9) ** 0.5, dt)
    b = torch.randn(Cout, generator=g)
    Ho = 2 * H if ups else H
    xin = F.interpolate(x.double(), scale_factor=2.0, mode="nearest") if ups else x.double()
    ref = F.conv2d(xin, w.double(), b.double(), padding=1)
    r = q(torch.randn(Nb, Cout, Ho, Ho, generator=g), dt) if res else None
    if res:
        ref = ref + r.double()
    X = x.permute(0, 2, 3, 1).contiguous().to(DEV, tdt(dt))
    Wp = w.permute(0, 2, 3, 1).reshape(Cout, -1).contiguous().to(DEV, tdt(dt))
    Y = torch.full((Nb, Ho, Ho, Cout), float("nan"), device=DEV, dtype=tdt(dt))
    if res:
        Y.copy_(r.permute(0, 2, 3, 1))   # in-place residual: R == Y
    bd = b.to(DEV)
    igemm(dt, X, Wp, Y, Y if res else None, bd, halo=True, Nimg=Nb, Hin=H, Win=H, Cin=Cin, ldx=Cin, Hout=Ho, Wout=Ho, KH=3, KW=3, stride=1,
          pad=1, ups=ups, N=Cout, ldw=9 * Cin, c_img=Ho * Ho * Cout, c_pix=Cout, flags=1 | (4 if res else 0))
    assert rel_err(Y.float().permute(0, 3, 1, 2), ref) < TOL[dt]


@pytest.mark.parametrize("dt", ["fp32", "bf16", "x3"])
@pytest.mark.parametrize("H,Cin,Cout,stats", [(16, 512, 512, 1), (32, 256, 256, 1), (32, 128, 64, 0), (16, 160, 64, 1), (64, 32, 128, 0),
                                              (16, 64, 192, 1), (32, 96, 128, 0), (64, 128, 128, 1)])
def test_upsampling_conv_subpixel_form(dt, H, Cin, Cout, stats, switches):
    """Round 6: conv3x3(nearest_x2(x)) as four 2x2 phase convolutions over the low-resolution input with weights pre-summed per
    output-pixel parity (packing.pack_subpixel; diffusers Upsample2D, vae.py:271-284): 2.25 x fewer multiplies.  Against fp64
    ``conv2d(interpolate(x, 2, 'nearest'), w, padding=1)`` on the same inputs: both tile shapes (16 x 16 / 8 x 32 over the INPUT), one to
    sixteen channel chunks incl. odd counts, ragged N (192), one / two / four N tiles, bias; every output pixel written exactly once
    (NaN-filled output); the GroupNorm statistics of the epilogue (per image and group, summed over the 4 x tiles chunks); bf16, fp32
    (f32-input MFMAs) and the split-bf16 arithmetic.  And the nine-tap kernel (IVG_SUBPIXEL=0) gives the same tensor up to the
    rounding of the pre-summed weights."""
    from ivideogpt_amd.packing import pack_subpixel, pack_x3
    L, l = lib()
    x3 = dt == "x3"
    sdt = "fp32" if x3 else dt
    if x3 and Cin % 16:
        pytest.skip("x3 needs Cin % 16 == 0")
    g = torch.Generator().manual_seed(H + Cin + Cout + 5)
    Nb, groups = 3, 32
    x = q(torch.randn(Nb, Cin, H, H, generator=g) * 1.3 + 0.2, sdt)
    w = q(torch.randn(Cout, Cin, 3, 3, generator=g) / (Cin * 9) ** 0.5, sdt)
    b = torch.randn(Cout, generator=g)
    Ho = 2 * H
    ref = F.conv2d(F.interpolate(x.double(), scale_factor=2.0, mode="nearest"), w.double(), b.double(), padding=1)
    X = x.permute(0, 2, 3, 1).contiguous().to(DEV, tdt(sdt))
    Wp = w.permute(0, 2, 3, 1).reshape(Cout, -1).contiguous().to(DEV, tdt(sdt))
    sub32 = pack_subpixel(w)                                   # fp32 [4 Cout, 4 Cin], summed in fp32
    Wsub = sub32.to(DEV, tdt(sdt)).contiguous()
    W3 = pack_x3(Wp) if x3 else None
    Wsub3 = pack_x3(sub32.to(DEV)) if x3 else None
    bd = b.to(DEV)
    outs = []
    for sub in (1, 0):
        switches(IVG_SUBPIXEL=str(sub))
        Y = torch.full((Nb, Ho, Ho, Cout), float("nan"), device=DEV, dtype=tdt(sdt))
        a = L.IvgIgemmArgs()
        a.X, a.W, a.Y, a.R, a.bias = X.data_ptr(), Wp.data_ptr(), Y.data_ptr(), None, bd.data_ptr()
        for k, v in dict(Nimg=Nb, Hin=H, Win=H, Cin=Cin, ldx=Cin, Hout=Ho, Wout=Ho, KH=3, KW=3, stride=1, pad=1, ups=1, N=Cout, ldw=9 * Cin,
                         c_img=Ho * Ho * Cout, c_pix=Cout, c_ch=1, c_grp=1, c_grp_stride=0, flags=1, alpha=1.0, nb0=1, nb1=1, nb2=1).items():
            setattr(a, k, v)
        bound = ((Ho * Ho + 255) // 256) * ((Cout + 63) // 64)
        part = torch.full((Nb * bound * groups * 2,), float("nan"), dtype=torch.float64, device=DEV) if stats and Cout % groups == 0 else None
        n0 = l.ivg_debug_counter(b"conv3x3_subpixel")
        if sub:
            rc = l.ivg_op_conv_subpixel(C.byref(a), code(sdt), P(Wsub), P(W3), P(Wsub3), P(part), groups, stream())
            assert rc >= 0, f"ivg_op_conv_subpixel rc={rc}"
            assert l.ivg_debug_counter(b"conv3x3_subpixel") == n0 + 1
            if part is not None:
                assert 0 < rc <= bound
                torch.cuda.synchronize()
                st = part[:Nb * rc * groups * 2].view(Nb, rc, groups, 2).sum(1).cpu()
                sv = Y.float().permute(0, 3, 1, 2).cpu().double().reshape(Nb, groups, -1)
                assert ((st[..., 0] - sv.sum(-1)).abs() / (sv.abs().sum(-1) + 1e-9)).max().item() < 1e-5
                assert ((st[..., 1] - (sv * sv).sum(-1)).abs() / (sv * sv).sum(-1)).max().item() < 1e-5
        else:
            if x3:
                ws = torch.empty(Nb * (((H * H + 1023) // 1024) * groups * 16 + Cin * 8) + 256, dtype=torch.uint8, device=DEV)
                assert l.ivg_op_conv_x3(C.byref(a), P(W3), groups, None, None, 1e-6, P(ws), stream()) == 0
            else:
                assert l.ivg_op_igemm(C.byref(a), code(sdt), stream()) == 0
            assert l.ivg_debug_counter(b"conv3x3_subpixel") == n0, "IVG_SUBPIXEL=0 must take the nine-tap kernel"
        torch.cuda.synchronize()
        assert torch.isfinite(Y.float()).all(), "an output pixel was not written"
        e = rel_err(Y.float().permute(0, 3, 1, 2), ref)
        assert e < (2e-5 if sdt == "fp32" else TOL["bf16"]), (sub, e)
        outs.append(Y.float())
    d = (outs[0] - outs[1]).abs().max().item() / ref.abs().max().item()
    assert d < (4e-5 if sdt == "fp32" else 2e-2), f"sub-pixel vs nine-tap kernel: {d:.3e}"


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_conv_out_planar_video(dt):
    """Cout = 3 written straight into a planar (B, T, 3, H, W) fp32 clip at frame offsets (decoder tail)."""
    g = torch.Generator().manual_seed(9)
    B, per, T, t0, H, Cin = 2, 3, 5, 2, 16, 64
    x = q(torch.randn(B * per, Cin, H, H, generator=g), dt)
    w = q(torch.randn(3, Cin, 3, 3, generator=g) / (Cin * 9) ** 0.5, dt)
    b = torch.randn(3, generator=g)
    ref = F.conv2d(x.double(), w.double(), b.double(), padding=1).reshape(B, per, 3, H, H)
    X = x.permute(0, 2, 3, 1).contiguous().to(DEV, tdt(dt))
    Wp = w.permute(0, 2, 3, 1).reshape(3, -1).contiguous().to(DEV, tdt(dt))
    clip = torch.full((B, T, 3, H, H), -7.0, device=DEV)
    Yv = clip.view(-1)[t0 * 3 * H * H:]
    igemm(dt, X, Wp, Yv, None, b.to(DEV), halo=True, Nimg=B * per, Hin=H, Win=H, Cin=Cin, ldx=Cin, Hout=H, Wout=H, KH=3, KW=3, stride=1, pad=1,
          N=3, ldw=9 * Cin, c_img=3 * H * H, c_pix=1, c_ch=H * H, c_grp=per, c_grp_stride=T * 3 * H * H, flags=1 | 32)
    assert rel_err(clip[:, t0:t0 + per], ref) < TOL[dt]
    assert (clip[:, :t0] == -7.0).all()


@pytest.mark.parametrize("out32", [1, 0])
@pytest.mark.parametrize("clamp", [1, 0])
def test_fused_decoder_tail_norm_silu_conv_out_clamp_planar(clamp, out32):
    """The decoders' tail as ONE launch (round 5; vae.py:292-294,364-369 + predict.py:73): conv_norm_out -> SiLU -> conv_out (C -> 3)
    [-> clamp(0, 1)] with the normalisation inside the 3x3 kernel's halo staging (its 64-channel instance), written straight into the
    planar (B, T, 3, H, W) clip at a frame offset, float32 or bfloat16 pixels."""
    L, l = lib()
    dt = "bf16"
    g = torch.Generator().manual_seed(21 + clamp)
    B, per, T, t0, H, Cin, groups = 2, 3, 5, 2, 32, 128, 32
    x = q(torch.randn(B * per, Cin, H, H, generator=g) * 1.3 + 0.2, dt)
    w = q(torch.randn(3, Cin, 3, 3, generator=g) / (Cin * 9) ** 0.5 * 3.0, dt)
    b = torch.randn(3, generator=g) * 0.3 + 0.4
    gamma, beta = 1 + 0.2 * torch.randn(Cin, generator=g), 0.2 * torch.randn(Cin, generator=g)
    hn = F.silu(F.group_norm(x.double(), groups, gamma.double(), beta.double(), eps=1e-6))
    hn = q(hn.float(), dt).double()
    ref = F.conv2d(hn, w.double(), b.double(), padding=1)
    if clamp:
        ref = ref.clamp(0, 1)
        assert (ref == 0).any() and (ref == 1).any() and ((ref > 0) & (ref < 1)).any()      # the clamp has something to do on both sides
    ref = ref.reshape(B, per, 3, H, H)
    X = x.permute(0, 2, 3, 1).contiguous().to(DEV, tdt(dt))
    Wp = w.permute(0, 2, 3, 1).reshape(3, -1).contiguous().to(DEV, tdt(dt))
    clip = torch.full((B, T, 3, H, H), -7.0, device=DEV, dtype=torch.float32 if out32 else torch.bfloat16)
    Yv = clip.view(-1)[t0 * 3 * H * H:]
    bd, gd, btd = b.to(DEV), gamma.to(DEV), beta.to(DEV)
    a = L.IvgIgemmArgs()
    a.X, a.W, a.Y, a.R, a.bias = X.data_ptr(), Wp.data_ptr(), Yv.data_ptr(), None, bd.data_ptr()
    for k, v in dict(Nimg=B * per, Hin=H, Win=H, Cin=Cin, ldx=Cin, Hout=H, Wout=H, KH=3, KW=3, stride=1, pad=1, ups=0, N=3, ldw=9 * Cin,
                     c_img=3 * H * H, c_pix=1, c_ch=H * H, c_grp=per, c_grp_stride=T * 3 * H * H, flags=1 | (32 if out32 else 0) | (128 if clamp else 0),
                     alpha=1.0, nb0=1, nb1=1, nb2=1).items():
        setattr(a, k, v)
    ws = torch.empty(B * per * (((H * H + 1023) // 1024) * groups * 16 + Cin * 8) + 256, dtype=torch.uint8, device=DEV)
    assert l.ivg_op_gn_conv(C.byref(a), code(dt), groups, P(gd), P(btd), 1e-6, P(ws), stream()) == 0
    torch.cuda.synchronize()
    got = clip[:, t0:t0 + per].float()
    assert torch.isfinite(got).all()
    assert rel_err(got, ref) < TOL[dt]
    if clamp:
        assert got.min().item() >= 0.0 and got.max().item() <= 1.0
    assert (clip[:, :t0].float() == -7.0).all()


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_batched_attention_gemms(dt):
    """strided batch (b, f, head) with a shared (stride 0) operand, alpha, fp32 scores, K tail (hd = 48), bias along M."""
    g = torch.Generator().manual_seed(11)
    B, Fr, nh, hd, P_, kv = 2, 3, 4, 48, 64, 128
    Cc = nh * hd
    Q = q(torch.randn(B * Fr, P_, Cc, generator=g), dt)
    Kp = q(torch.randn(B, kv, Cc, generator=g), dt)
    ref = torch.einsum("bfphd,bkhd->bfhpk", Q.view(B, Fr, P_, nh, hd).double(), Kp.view(B, kv, nh, hd).double()) * 0.25
    S = torch.full((B, Fr, nh, P_, kv), float("nan"), device=DEV)
    igemm(dt, Q.to(DEV, tdt(dt)), Kp.to(DEV, tdt(dt)), S, Win=P_, Wout=P_, Cin=hd, ldx=Cc, N=kv, ldw=Cc, c_pix=kv, flags=32, alpha=0.25,
          nb0=B, nb1=Fr, nb2=nh, sa=(Fr * P_ * Cc, P_ * Cc, hd), sw=(kv * Cc, 0, hd), sy=(Fr * nh * P_ * kv, nh * P_ * kv, P_ * kv))
    assert rel_err(S, ref) < TOL[dt]
    # V^T[b][c][tok] = Wv[c][:] . x[b][tok][:] + bv[c]   (shared X operand, bias along M)
    Wv, x, bv = q(torch.randn(Cc, Cc, generator=g) / Cc ** 0.5, dt), q(torch.randn(B, kv, Cc, generator=g), dt), torch.randn(Cc, generator=g)
    refv = torch.einsum("ck,btk->bct", Wv.double(), x.double()) + bv.double()[None, :, None]
    VT = torch.full((B, Cc, kv), float("nan"), device=DEV, dtype=tdt(dt))
    igemm(dt, Wv.to(DEV, tdt(dt)), x.to(DEV, tdt(dt)), VT, None, bv.to(DEV), Win=Cc, Wout=Cc, Cin=Cc, ldx=Cc, N=kv, ldw=Cc, c_pix=kv, flags=2,
          nb0=B, sa=(0, 0, 0), sw=(kv * Cc, 0, 0), sy=(Cc * kv, 0, 0))
    assert rel_err(VT.float(), refv) < TOL[dt]


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_glu_epilogue(dt):
    g = torch.Generator().manual_seed(13)
    M, H, I = 200, 128, 256
    x, gate, up = q(torch.randn(M, H, generator=g), dt), q(torch.randn(I, H, generator=g) / H ** 0.5, dt), q(torch.randn(I, H, generator=g) / H ** 0.5, dt)
    ref = F.silu(x.double() @ gate.double().T) * (x.double() @ up.double().T)
    wgu = torch.stack([gate.view(I // 16, 16, H), up.view(I // 16, 16, H)], 1).reshape(2 * I, H).contiguous()
    Y = torch.full((M, I), float("nan"), device=DEV, dtype=tdt(dt))
    igemm(dt, x.to(DEV, tdt(dt)), wgu.to(DEV, tdt(dt)), Y, Win=M, Wout=M, Cin=H, ldx=H, N=2 * I, ldw=H, c_pix=I, flags=16)
    assert rel_err(Y.float(), ref) < TOL[dt]


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("M", [3, 64, 100])
def test_skinny_gemm(dt, M):
    L, l = lib()
    g = torch.Generator().manual_seed(17 + M)
    N, K, I = 200, 512, 128
    x, w = q(torch.randn(M, K, generator=g), dt), q(torch.randn(N, K, generator=g) / K ** 0.5, dt)
    ref = x.double() @ w.double().T
    xd, wd = x.to(DEV, tdt(dt)), w.to(DEV, tdt(dt))
    Y = torch.full((M, N), float("nan"), device=DEV, dtype=tdt(dt))
    assert l.ivg_op_skinny(P(xd), P(wd), P(Y), M, N, K, K, K, N, 0, code(dt), stream()) == 0
    torch.cuda.synchronize()
    assert rel_err(Y.float(), ref) < TOL[dt]
    Yf = torch.full((M, N), float("nan"), device=DEV)
    assert l.ivg_op_skinny(P(xd), P(wd), P(Yf), M, N, K, K, K, N, 32, code(dt), stream()) == 0
    torch.cuda.synchronize()
    assert rel_err(Yf, ref) < 2e-5  # fp32 output: only accumulation-order error
    gate, up = q(torch.randn(I, K, generator=g) / K ** 0.5, dt), q(torch.randn(I, K, generator=g) / K ** 0.5, dt)
    wgu = torch.stack([gate.view(I // 16, 16, K), up.view(I // 16, 16, K)], 1).reshape(2 * I, K).contiguous().to(DEV, tdt(dt))
    refg = F.silu(x.double() @ gate.double().T) * (x.double() @ up.double().T)
    Yg = torch.full((M, I), float("nan"), device=DEV, dtype=tdt(dt))
    assert l.ivg_op_skinny(P(xd), P(wgu), P(Yg), M, 2 * I, K, K, K, I, 16, code(dt), stream()) == 0
    torch.cuda.synchronize()
    assert rel_err(Yg.float(), refg) < TOL[dt]


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("C_,P_,silu,pos", [(64, 256, 1, 0), (128, 4096, 1, 0), (192, 512, 0, 1), (768, 300, 1, 0), (512, 1500, 0, 1)])
def test_groupnorm(dt, C_, P_, silu, pos):
    L, l = lib()
    g = torch.Generator().manual_seed(C_ + P_)
    N = 3
    x = q(torch.randn(N, P_, C_, generator=g) * 2 + 0.5, dt)
    gamma, beta = torch.randn(C_, generator=g), torch.randn(C_, generator=g)
    pe = torch.randn(P_, C_, generator=g) if pos else None
    ref = F.group_norm(x.double().permute(0, 2, 1), 32, gamma.double(), beta.double(), 1e-6).permute(0, 2, 1)
    if silu:
        ref = F.silu(ref)
    if pos:
        ref = ref + pe.double()
    X = x.to(DEV, tdt(dt))
    Y = torch.full_like(X, float("nan"))
    ws = torch.empty(N * 64 * 32 * 2, dtype=torch.float64, device=DEV)
    gd, bd, pd = gamma.to(DEV), beta.to(DEV), (pe.to(DEV) if pos else None)   # keep the device tensors alive across the call
    rc = l.ivg_op_groupnorm(P(X), P(Y), P(ws), P(gd), P(bd), P(pd), N, P_, C_, 32, 1e-6, silu, code(dt), stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert rel_err(Y.float(), ref) < (1e-5 if dt == "fp32" else 1e-2)


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("Lq,Lk,causal", [(256, 512, 0), (514, 514, 1), (64, 2048, 0), (33, 33, 1)])
def test_softmax(dt, Lq, Lk, causal):
    L, l = lib()
    g = torch.Generator().manual_seed(Lq + Lk)
    rows_b = 3
    ld = (Lk + 63) // 64 * 64
    S = torch.randn(rows_b * Lq, ld, generator=g) * 3
    ref = S[:, :Lk].double().view(rows_b, Lq, Lk)
    if causal:
        mask = torch.ones(Lq, Lk, dtype=torch.bool).tril(Lk - Lq)
        ref = ref.masked_fill(~mask, float("-inf"))
    ref = torch.softmax(ref, -1).view(-1, Lk)
    Sd = S.to(DEV)
    Pm = torch.full((rows_b * Lq, ld), float("nan"), device=DEV, dtype=tdt(dt))
    assert l.ivg_op_softmax(P(Sd), P(Pm), rows_b * Lq, Lq, Lk, ld, ld, causal, code(dt), stream()) == 0
    torch.cuda.synchronize()
    assert (Pm[:, Lk:] == 0).all()
    assert (Pm[:, :Lk].float().cpu().double() - ref).abs().max().item() < (1e-6 if dt == "fp32" else 4e-3)


def test_vq_argmin_matches_cdist_argmin():
    """K10 in isolation on the same fp32 z: indices bit-exact vs argmin(torch.cdist) (lowest index on ties)."""
    L, l = lib()
    g = torch.Generator().manual_seed(3)
    for R, n_e, scale in [(1000, 8192, 0.5), (70, 512, 0.4), (4096, 8192, 1.0)]:
        z = torch.randn(R, 64, generator=g) * 0.75
        E = torch.randn(n_e, 64, generator=g) * scale
        ref = torch.argmin(torch.cdist(z, E), dim=1)
        out = torch.full((R,), -1, dtype=torch.int64, device=DEV)
        ee = torch.empty(n_e, device=DEV)
        zd, Ed = z.to(DEV), E.to(DEV)
        assert l.ivg_op_vq_argmin(P(zd), P(Ed), P(ee), P(out), R, n_e, stream()) == 0
        torch.cuda.synchronize()
        bad = (out.cpu() != ref).nonzero().flatten()
        if len(bad):  # audit: every mismatch must be an fp32 near-tie in the fp64 distances
            d = torch.cdist(z[bad].double(), E.double())
            gap = (d.gather(1, out.cpu()[bad, None]) - d.gather(1, ref[bad, None])).abs().squeeze(1)
            assert (gap < 1e-5).all(), f"{len(bad)} mismatches, max fp64 gap {gap.max():.3e}"
        assert len(bad) == 0, f"{len(bad)} near-tie mismatches out of {R} (all within fp32 round-off)"
    # duplicated codes: the lowest index must win
    E = torch.randn(512, 64, generator=g)
    E[300] = E[17]
    z = E[300:301].clone() + 1e-3
    out = torch.full((1,), -1, dtype=torch.int64, device=DEV)
    ee = torch.empty(512, device=DEV)
    zd, Ed = z.to(DEV), E.to(DEV)
    assert l.ivg_op_vq_argmin(P(zd), P(Ed), P(ee), P(out), 1, 512, stream()) == 0
    torch.cuda.synchronize()
    assert out.item() == 17


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_rmsnorm_rows(dt):
    """HF LlamaRMSNorm of the prompt pass: x * rsqrt(mean(x^2) + eps) rounded to the model dtype, then * weight."""
    L, l = lib()
    g = torch.Generator().manual_seed(5)
    M, H = 37, 768
    x, w = q(torch.randn(M, H, generator=g), dt), torch.randn(H, generator=g)
    xf = x.double()
    nrm = q((xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + 1e-6)).float(), dt)
    ref = w.double() * nrm.double()
    X = x.to(DEV, tdt(dt))
    out = torch.full((M, H), float("nan"), device=DEV, dtype=tdt(dt))
    assert l.ivg_op_add_rmsnorm(P(X), P(w.to(DEV)), P(out), M, H, 1e-6, code(dt), stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(X.float().cpu(), x), "the input rows are read only"
    assert rel_err(out.float(), ref) < (1e-5 if dt == "fp32" else 1.5e-2)


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_conv_in_from_video(dt):
    L, l = lib()
    g = torch.Generator().manual_seed(21)
    B, T, t0, per, H, C0 = 2, 5, 2, 3, 32, 64
    vid = torch.rand(B, T, 3, H, H, generator=g)
    w, b = torch.randn(C0, 3, 3, 3, generator=g) / 27 ** 0.5, torch.randn(C0, generator=g)
    ref = F.conv2d(vid[:, t0:t0 + per].reshape(-1, 3, H, H).double(), w.double(), b.double(), padding=1)
    Y = torch.full((B * per, H, H, C0), float("nan"), device=DEV, dtype=tdt(dt))
    vd, wd, bd = vid.to(DEV), w.to(DEV), b.to(DEV)
    assert l.ivg_op_conv_in(P(vd), 0, P(wd), P(bd), P(Y), code(dt), B * per, per, T, t0, H, H, C0, stream()) == 0
    torch.cuda.synchronize()
    assert rel_err(Y.float().permute(0, 3, 1, 2), ref) < (1e-5 if dt == "fp32" else 1e-2)


@pytest.mark.parametrize("case", ["normal", "wide_vocab", "ties_at_threshold", "all_equal", "topk_ge_vocab", "tiny_vocab", "heavy_ties"])
def test_sampler_matches_oracle(case):
    """top-k(100) + softmax + draw: radix-select threshold, ties at the threshold kept (HF masked_fill semantics), explicit
    uniform inverse CDF in ascending id order -- bit-identical tokens to oracle/llama.py sample_from_logits."""
    from oracle.llama import sample_from_logits
    L, l = lib()
    g = torch.Generator().manual_seed(sum(map(ord, case)))
    B, V, k = 64, 8194, 100
    if case == "wide_vocab":
        V = 16386
    if case == "tiny_vocab":
        V, k = 70, 100
    logits = torch.randn(B, V, generator=g) * 3
    if case == "ties_at_threshold":      # 300 copies of the 100-th largest value: all of them stay in the kept set
        kth = torch.topk(logits, k, dim=-1).values[:, -1:]
        idx = torch.randint(0, V, (B, 300), generator=g)
        logits.scatter_(1, idx, kth.expand(B, 300))
    if case == "all_equal":              # every token kept: the general (non-compacted) CDF path
        logits = torch.full((B, V), 1.25)
    if case == "heavy_ties":             # quantised logits: ~2,000 tokens tie at the threshold (> the compaction capacity)
        logits = torch.round(logits)
    if case == "topk_ge_vocab":
        k = V + 5
    logits[1, 7] = float("-inf")
    u = torch.rand(B, generator=g)
    u[0], u[2] = 0.0, 0.99999994
    want = sample_from_logits(logits, k, u)
    lg, ud = logits.to(DEV), u.to(DEV)
    out = torch.full((B,), -7, dtype=torch.int64, device=DEV)
    assert l.ivg_op_sample(P(lg), B, V, k, 1.0, P(ud), P(out), stream()) == 0
    assert torch.equal(out.cpu(), want), (out.cpu() != want).nonzero().flatten().tolist()
    assert l.ivg_op_sample(P(lg), B, V, k, 1.0, None, P(out), stream()) == 0
    assert torch.equal(out.cpu(), sample_from_logits(logits, k, None))


@pytest.mark.parametrize("temperature", [0.7, 1.3, 0.05, 9.0])
@pytest.mark.parametrize("V", [8194, 16386])
def test_sampler_temperature_matches_oracle(temperature, V):
    """``generate(..., temperature=T)`` of the reference (action_model.py:61,89; HF TemperatureLogitsWarper: scores / T in fp32
    BEFORE the top-k filter): token-identical to oracle/llama.py sample_from_logits(temperature=T), greedy unchanged."""
    from oracle.llama import sample_from_logits
    L, l = lib()
    g = torch.Generator().manual_seed(int(temperature * 100) + V)
    B, k = 64, 100
    logits = torch.randn(B, V, generator=g) * 3
    logits[3, 11] = float("-inf")
    u = torch.rand(B, generator=g)
    u[0], u[2] = 0.0, 0.99999994
    want = sample_from_logits(logits, k, u, temperature=temperature)
    assert not torch.equal(want, sample_from_logits(logits, k, u)), "the case must tell the temperatures apart"
    lg, ud = logits.to(DEV), u.to(DEV)
    out = torch.full((B,), -7, dtype=torch.int64, device=DEV)
    assert l.ivg_op_sample(P(lg), B, V, k, temperature, P(ud), P(out), stream()) == 0
    assert torch.equal(out.cpu(), want), (out.cpu() != want).nonzero().flatten().tolist()
    assert l.ivg_op_sample(P(lg), B, V, k, temperature, None, P(out), stream()) == 0
    assert torch.equal(out.cpu(), sample_from_logits(logits, k, None))
    assert l.ivg_op_sample(P(lg), B, V, k, 0.0, P(ud), P(out), stream()) == -1, "temperature must be strictly positive (HF raises)"


def test_sampler_temperature_vs_hf_processor_golden():
    """The sampler kernel against tokens drawn through HF's own TemperatureLogitsWarper -> TopKLogitsWarper -> softmax
    (tests/golden/sampler_temperature.npz; the reference hands temperature / top_k to HF generate)."""
    from helpers import load_golden
    L, l = lib()
    g = load_golden("sampler_temperature.npz")
    B, V, k = int(g["B"]), int(g["V"]), int(g["top_k"])
    gen = torch.Generator().manual_seed(int(g["seed"]))
    lg = (torch.randn(B, V, generator=gen) * 3).to(DEV)
    ud = torch.from_numpy(g["u"]).to(DEV)
    out = torch.full((B,), -7, dtype=torch.int64, device=DEV)
    for T in (0.7, 1.0, 1.3):
        assert l.ivg_op_sample(P(lg), B, V, k, T, P(ud), P(out), stream()) == 0
        assert torch.equal(out.cpu(), torch.from_numpy(g[f"tok_T{T}"])), T


@pytest.mark.parametrize("M", [64, 50, 16])
def test_skinny_gemm_lm_head_shape_with_ragged_vocab(M):
    """lm_head of the released models: 16386 = 256 * 64 + 2 columns -- the two ragged columns are computed by one extra
    workgroup per 16-row tile (tail split); every logit must still be written exactly once."""
    L, l = lib()
    g = torch.Generator().manual_seed(M)
    N, K = 16386, 768
    x, w = q(torch.randn(M, K, generator=g), "bf16"), q(torch.randn(N, K, generator=g) / K ** 0.5, "bf16")
    ref = x.double() @ w.double().T
    xd, wd = x.to(DEV, torch.bfloat16), w.to(DEV, torch.bfloat16)
    Yf = torch.full((M, N), float("nan"), device=DEV)
    assert l.ivg_op_skinny(P(xd), P(wd), P(Yf), M, N, K, K, K, N, 32, code("bf16"), stream()) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(Yf).all() and rel_err(Yf, ref) < 2e-5
    assert rel_err(Yf[:, -2:], ref[:, -2:]) < 2e-5


DECODE_SHAPES = [  # (K, N, flags): every decode-step GEMM of the small (768 / 3072) and medium (1024 / 4096) transformers
    (768, 2304, "norm"), (768, 768, "residual"), (768, 6144, "norm_glu"), (3072, 768, "residual"),
    (1024, 3072, "norm"), (1024, 1024, "residual"), (1024, 8192, "norm_glu"), (4096, 1024, "residual"),
    (768, 16386, "norm_f32"), (128, 384, "norm"), (256, 128, "residual"), (1024, 16386, "norm_f32"),
]


@pytest.mark.parametrize("gen", ["gen3", "gen2", "inflight40"])
@pytest.mark.parametrize("dt", ["bf16", "fp32"])
@pytest.mark.parametrize("K,N,mode", DECODE_SHAPES)
def test_decode_gemm_model_shapes(K, N, mode, dt, gen, switches):
    """The decode-step GEMMs at the shapes the rollouts run (BASELINE configs 2 and 5), with their fused epilogues -- RMSNorm row
    scale, in-place residual, SiLU(gate) * up, fp32 logits -- against fp64, for the third-generation kernel (dgemm3.hip: K over up
    to 16 waves, one barrier; the default), the second (IVG_DG3=0, dgemm.hip: activations as whole lines through LDS) and
    ``inflight40``: the BATCHES-IN-FLIGHT profile exactly as bench.py's lanes launch it -- the engine policy of a 40 KiB LDS budget with
    shared-weight (default cache policy) requests through ivg_op_skinny_policy, whatever generation / plan the dispatcher picks for it:
    the kernel configurations the headline number is produced with."""
    L, l = lib()
    switches(IVG_DG3="0" if gen == "gen2" else None, IVG_DECODE_LDS_KB=None)
    policy = (40, 1) if gen == "inflight40" else (0, 0)
    g2_0 = l.ivg_debug_counter(b"decode_gemm_gen2")
    g = torch.Generator().manual_seed(K + N)
    for M in (64, 37, 128):
        x = q(torch.randn(M, K, generator=g) * 1.7, dt)
        w = q(torch.randn(N, K, generator=g) / K ** 0.5, dt)
        xd = x.to(DEV, tdt(dt))
        flags, ldy, out_dt = 0, N, tdt(dt)
        xs = x.double()
        if "norm" in mode:
            flags |= 64
            xs = xs * torch.rsqrt(xs.pow(2).mean(-1, keepdim=True) + 1e-6)
        if mode == "norm_glu":
            I = N // 2
            gate, up = w[:I], w[I:]
            wd = torch.stack([gate.view(I // 16, 16, K), up.view(I // 16, 16, K)], 1).reshape(N, K).contiguous().to(DEV, tdt(dt))
            ref = F.silu(xs @ gate.double().T) * (xs @ up.double().T)
            flags |= 16
            ldy = I
        else:
            wd = w.to(DEV, tdt(dt))
            ref = xs @ w.double().T
        if mode == "norm_f32":
            flags |= 32
            out_dt = torch.float32
        if mode == "residual":
            r0 = q(torch.randn(M, N, generator=g), dt)
            Y = r0.to(DEV, tdt(dt)).clone()
            ref = ref + r0.double()
            flags |= 4
        else:
            Y = torch.full((M, ldy), float("nan"), device=DEV, dtype=out_dt)
        assert l.ivg_op_skinny_policy(P(xd), P(wd), P(Y), M, N, K, K, K, ldy, flags, code(dt), policy[0], policy[1], stream()) == 0
        torch.cuda.synchronize()
        assert torch.isfinite(Y.float()).all()
        tol = 2e-5 if (dt == "fp32" or mode == "norm_f32") else TOL[dt]
        assert rel_err(Y.float(), ref) < tol, (M, K, N, mode, dt, gen)
    if gen == "inflight40" and K * (2 if dt == "bf16" else 4) in (1536, 6144) and N in (2304, 6144, 768):
        # the small transformer's q/k/v, gate/up, o and down under the lanes' budget: the small-footprint second-generation plans
        assert l.ivg_debug_counter(b"decode_gemm_gen2") - g2_0 == 3, "the 40 KiB budget did not select the second-generation plans"


def test_gemm256_half_width_tile_for_128_output_channels(switches):
    """gemm256l_kernel<128> (round 5): 256 rows x 128 weight rows per workgroup, for the dense 1x1 layers with 128 output channels over
    >= 2^18 pixels (the resnet shortcuts of the top decoder level, 256 -> 128).  Ragged last M tile, bias, in-place residual; and the
    same bits as the implicit GEMM would NOT be expected (other K order) -- compared against fp64."""
    M, N, K = (1 << 18) + 77, 128, 256
    g = torch.Generator().manual_seed(5)
    X = q(torch.randn(M, K, generator=g), "bf16")
    W_ = q(torch.randn(N, K, generator=g) / K ** 0.5, "bf16")
    b = torch.randn(N, generator=g)
    R = q(torch.randn(M, N, generator=g), "bf16")
    ref = X.double() @ W_.double().T + b.double() + R.double()
    Xd, Wd, bd = X.to(DEV, torch.bfloat16), W_.to(DEV, torch.bfloat16), b.to(DEV)
    outs = []
    for g256 in ("1", "0"):
        switches(IVG_GEMM256=g256)
        Y = R.to(DEV, torch.bfloat16).clone()
        igemm("bf16", Xd, Wd, Y, Y, bd, Win=M, Wout=M, Cin=K, ldx=K, N=N, ldw=K, c_pix=N, flags=1 | 4)
        assert rel_err(Y.float(), ref) < TOL["bf16"]
        outs.append(Y)
    assert (outs[0].float() - outs[1].float()).abs().max().item() < 0.1      # two kernels, one result up to bf16 rounding


def test_gemm256_rows_beyond_2gib_run_as_row_ranges():
    """A dense 1x1 layer whose activations exceed the kernel's 32-bit operand offsets (the 256 -> 128 shortcuts of the top decoder level
    at 256 x 256: 14.7 M rows; here 4.2 M rows x 256 channels = 2.15 GB): the launcher splits the rows into ranges of < 2 GiB
    (round 6; such layers fell back to the implicit GEMM before).  Rows on both sides of the range boundary, the first and the ragged
    last tile against fp64; bias + in-place residual."""
    M, N, K = (1 << 22) + 333, 128, 256
    rows_max = ((1 << 31) - 1) // (2 * K) // 256 * 256
    assert 4096 < rows_max < M
    g = torch.Generator(device=DEV).manual_seed(3)
    Xd = torch.randn(M, K, device=DEV, generator=g).to(torch.bfloat16)
    Wd = (torch.randn(N, K, device=DEV, generator=g) / K ** 0.5).to(torch.bfloat16)
    bd = torch.randn(N, device=DEV, generator=g)
    Y = torch.randn(M, N, device=DEV, generator=g).to(torch.bfloat16)
    pick = torch.cat([torch.arange(0, 300), torch.arange(rows_max - 300, rows_max + 300), torch.arange(M - 400, M),
                      torch.randint(0, M, (500,), generator=torch.Generator().manual_seed(1))])
    ref = Xd[pick.to(DEV)].double().cpu() @ Wd.double().cpu().T + bd.double().cpu() + Y[pick.to(DEV)].double().cpu()
    before = Y[rows_max + 100].clone()
    igemm("bf16", Xd, Wd, Y, Y, bd, Win=M, Wout=M, Cin=K, ldx=K, N=N, ldw=K, c_pix=N, flags=1 | 4)
    got = Y[pick.to(DEV)].double().cpu()
    assert torch.isfinite(got).all() and rel_err(got, ref) < TOL["bf16"]
    assert not torch.equal(Y[rows_max + 100], before), "rows of the second range were not written"


@pytest.mark.parametrize("mode", ["plain", "bias_residual_inplace", "glu", "silu", "k_short", "k_odd_steps", "nimg"])
def test_gemm256_large_dense(mode, switches):
    """256 x 256-tile GEMM of the prompt pass (bf16, rows not a multiple of 256): every epilogue against fp64, and bit-for-bit
    agreement is NOT required with the 128 x 128 kernel -- but both must sit inside the same bf16 tolerance.
    Whole-line requests (K steps of 64 elements); k_odd_steps has K = 160, which the tile kernel does not take (K % 64 != 0): the
    same call falls to the generic implicit GEMM and must meet the same bar."""
    g = torch.Generator().manual_seed(len(mode))
    M, N, K = 4900, 512, {"k_short": 64, "k_odd_steps": 96 + 64}.get(mode, 384)   # 2 / 5 / 12 K steps
    dt = "bf16"
    X = q(torch.randn(M, K, generator=g), dt)
    W_ = q(torch.randn(N, K, generator=g) / K ** 0.5, dt)
    Xd, Wd = X.to(DEV, torch.bfloat16), W_.to(DEV, torch.bfloat16)
    kw = dict(Win=M, Wout=M, Cin=K, ldx=K, N=N, ldw=K, c_pix=N)
    if mode == "nimg":                       # a dense 1x1 layer over 49 images of 10 x 10 pixels
        kw.update(Nimg=49, Hin=10, Win=10, Hout=10, Wout=10, c_img=100 * N)
    if mode == "glu":
        I = N // 2
        gate, up = W_[:I], W_[I:]
        wgu = torch.stack([gate.view(I // 16, 16, K), up.view(I // 16, 16, K)], 1).reshape(N, K).contiguous().to(DEV, torch.bfloat16)
        ref = F.silu(X.double() @ gate.double().T) * (X.double() @ up.double().T)
        Y = torch.full((M, I), float("nan"), device=DEV, dtype=torch.bfloat16)
        kw.update(c_pix=I, flags=16)
        igemm(dt, Xd, wgu, Y, **kw)
    elif mode == "bias_residual_inplace":
        b = torch.randn(N, generator=g)
        R = q(torch.randn(M, N, generator=g), dt)
        ref = X.double() @ W_.double().T + b.double() + R.double()
        Y = R.to(DEV, torch.bfloat16).clone()
        igemm(dt, Xd, Wd, Y, Y, b.to(DEV), flags=1 | 4, **kw)   # residual stream updated in place, as o_proj / down_proj do
    else:
        ref = X.double() @ W_.double().T
        if mode == "silu":
            ref = F.silu(ref)
        Y = torch.full((M, N), float("nan"), device=DEV, dtype=torch.bfloat16)
        igemm(dt, Xd, Wd, Y, flags=8 if mode == "silu" else 0, **kw)
    assert torch.isfinite(Y.float()).all()
    e_big = rel_err(Y.float(), ref)
    assert e_big < TOL[dt], f"{mode}: rel err {e_big:.3e}"
    if mode == "plain":                      # the generic kernel on the same operands: same tolerance class
        switches(IVG_GEMM256="0")
        Y2 = torch.full((M, N), float("nan"), device=DEV, dtype=torch.bfloat16)
        igemm(dt, Xd, Wd, Y2, **kw)
        assert rel_err(Y2.float(), ref) < TOL[dt] and (Y2.float() - Y.float()).abs().max().item() <= 2 * TOL[dt] * ref.abs().max().item()


@pytest.mark.parametrize("mode", ["plain", "bias_residual_inplace", "glu", "silu", "k_one_step", "nimg", "narrow_falls_back"])
def test_gemm256_x3_large_dense(mode, switches):
    """256 x 256-tile split-bf16 ("x3") GEMM (round 6: the prompt pass and the dense 1x1 layers of the 1e-3-compliant mode left the
    128 x 128 implicit GEMM): fp32 tensors, both operands split into bf16 (hi, lo) in registers, four partial products, fp32
    accumulate -- against fp64 on the SAME fp32 inputs, 2e-5 relative (2^-17 per operand; the bar of the other x3 kernels).  Rows not a
    multiple of 256, every epilogue, K of one 128-byte step per row pair, a dense 1x1 layer over images; N = 384 is not covered and
    must fall to igemm_kernel<float, ..., X3> with the same bar.  The debug counter shows which kernel ran."""
    L, l = lib()
    g = torch.Generator().manual_seed(7 + len(mode))
    M, N, K = 4900, {"narrow_falls_back": 384}.get(mode, 512), {"k_one_step": 64}.get(mode, 416)
    X = torch.randn(M, K, generator=g) * 1.3 + 0.2
    W_ = torch.randn(N, K, generator=g) / K ** 0.5
    Xd, Wd = X.to(DEV), W_.to(DEV)
    kw = dict(Win=M, Wout=M, Cin=K, ldx=K, N=N, ldw=K, c_pix=N)
    if mode == "nimg":
        kw.update(Nimg=49, Hin=10, Win=10, Hout=10, Wout=10, c_img=100 * N)
    before = l.ivg_debug_counter(b"gemm256x3")
    if mode == "glu":
        I = N // 2
        gate, up = W_[:I], W_[I:]
        wgu = torch.stack([gate.view(I // 16, 16, K), up.view(I // 16, 16, K)], 1).reshape(N, K).contiguous().to(DEV)
        ref = F.silu(X.double() @ gate.double().T) * (X.double() @ up.double().T)
        Y = torch.full((M, I), float("nan"), device=DEV)
        kw.update(c_pix=I, flags=16)
        igemm("x3", Xd, wgu, Y, **kw)
    elif mode == "bias_residual_inplace":
        b = torch.randn(N, generator=g)
        R = torch.randn(M, N, generator=g)
        ref = X.double() @ W_.double().T + b.double() + R.double()
        Y = R.to(DEV).clone()
        igemm("x3", Xd, Wd, Y, Y, b.to(DEV), flags=1 | 4, **kw)
    else:
        ref = X.double() @ W_.double().T
        if mode == "silu":
            ref = F.silu(ref)
        Y = torch.full((M, N), float("nan"), device=DEV)
        igemm("x3", Xd, Wd, Y, flags=8 if mode == "silu" else 0, **kw)
    ran = l.ivg_debug_counter(b"gemm256x3") - before
    assert ran == (0 if mode == "narrow_falls_back" else 1), ran
    assert torch.isfinite(Y).all()
    e = rel_err(Y, ref)
    assert e < 2e-5, f"{mode}: rel err {e:.3e}"
    assert e > 1e-8, "suspiciously exact: is this an f32-input MFMA path?"
    if mode == "plain":   # the implicit GEMM's X3 instance on the same operands: same bar, and the two agree far inside it
        switches(IVG_GEMM256X3="0")
        Y2 = torch.full((M, N), float("nan"), device=DEV)
        igemm("x3", Xd, Wd, Y2, **kw)
        assert l.ivg_debug_counter(b"gemm256x3") - before == 1
        assert rel_err(Y2, ref) < 2e-5 and (Y2 - Y).abs().max().item() < 4e-5 * ref.abs().max().item()


# ------------------------------------------------------------------------------------------------ frame metrics / clip ingest
@pytest.mark.parametrize("gt_dt", ["fp32", "bf16"])
@pytest.mark.parametrize("B,t,T,H,W", [(3, 2, 4, 64, 64), (1, 1, 2, 256, 256), (2, 3, 2, 80, 107), (64, 1, 14, 64, 64)])
def test_frame_metrics_match_the_oracle(B, t, T, H, W, gt_dt):
    """ivg_frame_metrics (per-frame MSE / PSNR / SSIM, mean over frames, best of t) against oracle/metrics.py, the CPU
    restatement of Evaluator.forward (ivideogpt/utils/video_metric.py:63-100), incl. frame offsets into longer clips."""
    from ivideogpt_amd.metrics import frame_metric_rows
    from oracle.metrics import frame_metric_rows as ref_rows
    g = torch.Generator().manual_seed(B * 100 + T + H)
    gt = q(torch.rand(B, T + 2, 3, H, W, generator=g), gt_dt)
    base = gt[:, 2:].repeat(t, 1, 1, 1, 1)
    noise = torch.randn(t * B, T, 3, H, W, generator=g) * torch.linspace(0.01, 0.2, t * B).view(-1, 1, 1, 1, 1)
    pred = torch.cat([torch.rand(t * B, 1, 3, H, W, generator=g), (base + noise).clamp(0, 1)], 1)   # one leading frame to skip
    rows = frame_metric_rows(gt.to(DEV, tdt(gt_dt)), pred.to(DEV), gt_t0=2, pred_t0=1, frames=T).cpu()
    ref = ref_rows(gt[:, 2:], pred[:, 1:])
    assert rows.shape == (B, 3)
    assert ((rows[:, 0] - ref[:, 0]).abs() / ref[:, 0]).max().item() < 1e-4, "mse"
    assert (rows[:, 1] - ref[:, 1]).abs().max().item() < 1e-3, "psnr"
    assert (rows[:, 2] - ref[:, 2]).abs().max().item() < 1e-4, "ssim"


def test_frame_metrics_identical_clips():
    from ivideogpt_amd.metrics import frame_metric_rows
    x = torch.rand(2, 3, 3, 64, 64, device=DEV)
    rows = frame_metric_rows(x, x.clone()).cpu()
    assert rows[:, 0].abs().max().item() == 0.0 and (rows[:, 1] - 80.0).abs().max().item() < 1e-3 and (rows[:, 2] - 1.0).abs().max().item() < 1e-6


@pytest.mark.parametrize("T,H,W,R,crop", [(16, 256, 320, 64, 0), (3, 240, 320, 64, 1), (2, 480, 640, 256, 0), (2, 48, 64, 64, 0),
                                          (1, 64, 64, 64, 0), (2, 131, 97, 64, 1), (1, 720, 960, 64, 0)])
def test_ingest_matches_torch_antialiased_resize(T, H, W, R, crop):
    """ivg_ingest_frames (uint8 (T, H, W, 3) -> / 255 -> optional centre crop -> antialiased bilinear resize -> planar clip) against
    the reference's preprocessing restated with torch on the CPU (inference/utils.py:12-16: images / 255, torchvision resize =
    interpolate(mode='bilinear', antialias=True)); fp32 within 2e-6, bf16 output = the rounded fp32 one."""
    from ivideogpt_amd.data import ingest_frames
    g = torch.Generator().manual_seed(H + W)
    u8 = torch.randint(0, 256, (T, H, W, 3), generator=g, dtype=torch.uint8)
    x = u8.float().permute(0, 3, 1, 2) / 255
    if crop:
        s = min(H, W)
        top, left = int(round((H - s) / 2.0)), int(round((W - s) / 2.0))
        x = x[..., top:top + s, left:left + s]
    ref = x if tuple(x.shape[-2:]) == (R, R) else F.interpolate(x, size=(R, R), mode="bilinear", antialias=True, align_corners=False)
    out = ingest_frames(u8.to(DEV), R, center_crop=bool(crop)).cpu()
    assert out.shape == (T, 3, R, R)
    assert (out - ref).abs().max().item() < 2e-6
    out16 = ingest_frames(u8.to(DEV), R, center_crop=bool(crop), dtype=torch.bfloat16).cpu()
    assert (out16.float() - ref).abs().max().item() < 4e-3


def test_ingest_fractal_sample_matches_reference_clip():
    """BASELINE config 1 input: the frames the reference's NPZParser selects from inference/samples/fractal_sample.npz (seed 0)
    through the device ingest kernel == the clip the REFERENCE's parser produced (tests/golden/fractal_clip_seed0.npz)."""
    import numpy as np
    import os
    from ivideogpt_amd.data import NPZParser
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    ref = torch.from_numpy(np.load(os.path.join(gold, "fractal_clip_seed0.npz"))["clip"])
    np.random.seed(0)
    clip, _ = NPZParser(16, 64, device=DEV).parse(os.path.join(gold, "fractal_sample.npz"), "fractal20220817_data")
    assert clip.shape == (16, 3, 64, 64) and (clip.cpu() - ref).abs().max().item() < 2e-6
    np.random.seed(0)
    host, _ = NPZParser(16, 64).parse(os.path.join(gold, "fractal_sample.npz"), "fractal20220817_data")
    assert torch.equal(host, ref), "host-side parser must reproduce the reference's clip bit for bit"


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("H,Cin,Cout,ups,res,silu", [(64, 128, 128, 0, 1, 1), (32, 256, 512, 0, 0, 1), (16, 512, 512, 1, 0, 0), (32, 128, 64, 1, 1, 1),
                                                      (16, 64, 768, 0, 1, 1), (16, 64, 192, 0, 0, 0)])
def test_conv3x3_epilogue_groupnorm_statistics(dt, H, Cin, Cout, ups, res, silu):
    """The GroupNorm statistics a conv3x3 epilogue reduces for its own output (so the consuming GroupNorm skips its statistics
    pass): conv -> GroupNorm(32 groups)[+ SiLU] from those statistics == torch group_norm of the conv output AS STORED, incl. groups
    that straddle two channel tiles (768 channels: 24 per group, tiles of 128), several spatial tiles, upsampling and the in-place
    residual."""
    L, l = lib()
    g = torch.Generator().manual_seed(H + Cin + Cout + 1)
    Nb, groups = 3, 32
    x = q(torch.randn(Nb, Cin, H, H, generator=g), dt)
    w = q(torch.randn(Cout, Cin, 3, 3, generator=g) / (Cin * 9) ** 0.5, dt)
    b = torch.randn(Cout, generator=g)
    gamma, beta = 1 + 0.2 * torch.randn(Cout, generator=g), 0.2 * torch.randn(Cout, generator=g)
    Ho = 2 * H if ups else H
    r = q(torch.randn(Nb, Cout, Ho, Ho, generator=g), dt) if res else None
    X = x.permute(0, 2, 3, 1).contiguous().to(DEV, tdt(dt))
    Wp = w.permute(0, 2, 3, 1).reshape(Cout, -1).contiguous().to(DEV, tdt(dt))
    Y = torch.full((Nb, Ho, Ho, Cout), float("nan"), device=DEV, dtype=tdt(dt))
    if res:
        Y.copy_(r.permute(0, 2, 3, 1))
    bd = b.to(DEV)
    a = L.IvgIgemmArgs()
    a.X, a.W, a.Y, a.R, a.bias = X.data_ptr(), Wp.data_ptr(), Y.data_ptr(), (Y.data_ptr() if res else None), bd.data_ptr()
    for k, v in dict(Nimg=Nb, Hin=H, Win=H, Cin=Cin, ldx=Cin, Hout=Ho, Wout=Ho, KH=3, KW=3, stride=1, pad=1, ups=ups, N=Cout, ldw=9 * Cin,
                     c_img=Ho * Ho * Cout, c_pix=Cout, c_ch=1, c_grp=1, c_grp_stride=0, flags=1 | (4 if res else 0), alpha=1.0, nb0=1, nb1=1,
                     nb2=1).items():
        setattr(a, k, v)
    bound = ((Ho * Ho + 255) // 256) * ((Cout + 63) // 64)
    part = torch.full((Nb * bound * groups * 2,), float("nan"), dtype=torch.float64, device=DEV)
    out = torch.full((Nb, Ho, Ho, Cout), float("nan"), device=DEV, dtype=tdt(dt))
    gd, btd = gamma.to(DEV), beta.to(DEV)
    chunks = l.ivg_op_conv_gn(C.byref(a), code(dt), P(part), groups, P(gd), P(btd), P(out), 1e-6, silu, stream())
    torch.cuda.synchronize()
    assert 0 < chunks <= bound, chunks
    stored = Y.float().permute(0, 3, 1, 2).cpu().double()          # the conv output as the engine stored it
    ref = F.group_norm(stored, groups, gamma.double(), beta.double(), eps=1e-6)
    if silu:
        ref = F.silu(ref)
    assert torch.isfinite(out.float()).all()
    assert rel_err(out.float().permute(0, 3, 1, 2), ref) < (2e-5 if dt == "fp32" else TOL[dt])
    # the statistics themselves: per (image, group) sums over the chunks
    st = part[:Nb * chunks * groups * 2].view(Nb, chunks, groups, 2).sum(1).cpu()
    cpg = Cout // groups
    sv = stored.reshape(Nb, groups, cpg * Ho * Ho)
    assert ((st[..., 0] - sv.sum(-1)).abs() / (sv.abs().sum(-1) + 1e-9)).max().item() < 1e-5
    assert ((st[..., 1] - (sv * sv).sum(-1)).abs() / (sv * sv).sum(-1)).max().item() < 1e-5


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("H,Cin,Cout,res", [(64, 128, 128, 1), (32, 256, 512, 0), (16, 512, 512, 1), (32, 128, 64, 0), (16, 768, 768, 1),
                                            (16, 64, 192, 0), (32, 32, 128, 1)])
def test_conv3x3_with_fused_input_groupnorm(dt, H, Cin, Cout, res):
    """conv3x3(silu(GroupNorm(x))) with the GroupNorm applied in place on the staged halo chunk (conv3x3.hip, ABL bit 16): against
    torch conv2d(silu(group_norm(x))) in fp64 -- zero padding must stay zero AFTER the normalisation, single- and multi-chunk Cin,
    several spatial tiles (halo rows outside the image on every side), residual."""
    L, l = lib()
    g = torch.Generator().manual_seed(H * 3 + Cin + Cout)
    Nb, groups = 3, 32
    x = q(torch.randn(Nb, Cin, H, H, generator=g) * 1.5 + 0.3, dt)
    w = q(torch.randn(Cout, Cin, 3, 3, generator=g) / (Cin * 9) ** 0.5, dt)
    b = torch.randn(Cout, generator=g)
    gamma, beta = 1 + 0.2 * torch.randn(Cin, generator=g), 0.2 * torch.randn(Cin, generator=g)
    hn = F.silu(F.group_norm(x.double(), groups, gamma.double(), beta.double(), eps=1e-6))
    hn = q(hn.float(), dt).double()                       # the engine rounds the normalised values to the storage type
    ref = F.conv2d(hn, w.double(), b.double(), padding=1)
    r = q(torch.randn(Nb, Cout, H, H, generator=g), dt) if res else None
    if res:
        ref = ref + r.double()
    X = x.permute(0, 2, 3, 1).contiguous().to(DEV, tdt(dt))
    Wp = w.permute(0, 2, 3, 1).reshape(Cout, -1).contiguous().to(DEV, tdt(dt))
    Y = torch.full((Nb, H, H, Cout), float("nan"), device=DEV, dtype=tdt(dt))
    if res:
        Y.copy_(r.permute(0, 2, 3, 1))
    bd, gd, btd = b.to(DEV), gamma.to(DEV), beta.to(DEV)
    a = L.IvgIgemmArgs()
    a.X, a.W, a.Y, a.R, a.bias = X.data_ptr(), Wp.data_ptr(), Y.data_ptr(), (Y.data_ptr() if res else None), bd.data_ptr()
    for k, v in dict(Nimg=Nb, Hin=H, Win=H, Cin=Cin, ldx=Cin, Hout=H, Wout=H, KH=3, KW=3, stride=1, pad=1, ups=0, N=Cout, ldw=9 * Cin,
                     c_img=H * H * Cout, c_pix=Cout, c_ch=1, c_grp=1, c_grp_stride=0, flags=1 | (4 if res else 0), alpha=1.0, nb0=1, nb1=1,
                     nb2=1).items():
        setattr(a, k, v)
    ws = torch.empty(Nb * (((H * H + 1023) // 1024) * groups * 16 + Cin * 8) + 256, dtype=torch.uint8, device=DEV)
    assert l.ivg_op_gn_conv(C.byref(a), code(dt), groups, P(gd), P(btd), 1e-6, P(ws), stream()) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(Y.float()).all()
    assert rel_err(Y.float().permute(0, 3, 1, 2), ref) < (5e-5 if dt == "fp32" else TOL[dt])


@pytest.mark.parametrize("gn", [0, 1])
@pytest.mark.parametrize("H,Cin,Cout,ups,res", [(64, 128, 128, 0, 1), (32, 256, 512, 0, 0), (16, 512, 512, 1, 0), (32, 128, 64, 1, 1),
                                                 (16, 64, 192, 0, 1), (16, 48, 128, 0, 0), (32, 16, 64, 0, 1), (64, 32, 128, 1, 1)])
def test_conv3x3_x3_split_bf16(H, Cin, Cout, ups, res, gn):
    """The split-bf16 ("x3") 3x3 convolution of the 1e-3-compliant decode mode: fp32 tensors in HBM, activations split into bf16
    (hi, lo) pairs inside the halo staging, weights pre-split by packing.pack_x3, two K = 32 bf16 MFMAs per 16 channels, fp32
    accumulate -- against fp64 torch conv2d on the SAME fp32 inputs.  Error bar 2e-5 relative (each operand carries 2^-17; the
    f32-input MFMA path is held to 1e-5 by test_conv3x3_halo_kernel) -- 50x inside the 1e-3 bar on pixels.  Both tile shapes, odd
    chunk counts, one-chunk Cin, ragged N, upsampling, residual, and (gn) GroupNorm + SiLU applied inside the staging before the split."""
    from ivideogpt_amd.packing import pack_x3
    if gn and ups:
        pytest.skip("the upsampling convolutions take un-normalised inputs")
    L, l = lib()
    g = torch.Generator().manual_seed(H + Cin + Cout + 17 * gn)
    Nb, groups = 3, 16 if Cin % 32 else 32
    x = torch.randn(Nb, Cin, H, H, generator=g) * 1.5 + 0.3
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / (Cin * 9) ** 0.5
    b = torch.randn(Cout, generator=g)
    gamma, beta = 1 + 0.2 * torch.randn(Cin, generator=g), 0.2 * torch.randn(Cin, generator=g)
    Ho = 2 * H if ups else H
    xin = x.double()
    if gn:
        xin = F.silu(F.group_norm(xin, groups, gamma.double(), beta.double(), eps=1e-6))
    if ups:
        xin = F.interpolate(xin, scale_factor=2.0, mode="nearest")
    ref = F.conv2d(xin, w.double(), b.double(), padding=1)
    r = torch.randn(Nb, Cout, Ho, Ho, generator=g) if res else None
    if res:
        ref = ref + r.double()
    X = x.permute(0, 2, 3, 1).contiguous().to(DEV)
    Wp = w.permute(0, 2, 3, 1).reshape(Cout, -1).contiguous().to(DEV)
    W3 = pack_x3(Wp)
    assert W3.dtype == torch.bfloat16 and W3.shape == (Cout, 18 * Cin)
    Y = torch.full((Nb, Ho, Ho, Cout), float("nan"), device=DEV)
    if res:
        Y.copy_(r.permute(0, 2, 3, 1))
    bd, gd, btd = b.to(DEV), gamma.to(DEV), beta.to(DEV)
    a = L.IvgIgemmArgs()
    a.X, a.W, a.Y, a.R, a.bias = X.data_ptr(), Wp.data_ptr(), Y.data_ptr(), (Y.data_ptr() if res else None), bd.data_ptr()
    for k, v in dict(Nimg=Nb, Hin=H, Win=H, Cin=Cin, ldx=Cin, Hout=Ho, Wout=Ho, KH=3, KW=3, stride=1, pad=1, ups=ups, N=Cout, ldw=9 * Cin,
                     c_img=Ho * Ho * Cout, c_pix=Cout, c_ch=1, c_grp=1, c_grp_stride=0, flags=1 | (4 if res else 0), alpha=1.0, nb0=1, nb1=1,
                     nb2=1).items():
        setattr(a, k, v)
    ws = torch.empty(Nb * (((H * H + 1023) // 1024) * groups * 16 + Cin * 8) + 256, dtype=torch.uint8, device=DEV)
    rc = l.ivg_op_conv_x3(C.byref(a), P(W3), groups, P(gd) if gn else None, P(btd) if gn else None, 1e-6, P(ws), stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert torch.isfinite(Y).all()
    e = rel_err(Y.permute(0, 3, 1, 2), ref)
    assert e < 2e-5, f"rel err {e:.3e}"
    assert e > 1e-8 or Cin <= 16, "suspiciously exact: is this the f32-input MFMA path?"


@pytest.mark.parametrize("C_,nh,P_,ctx,B,Fr", [(512, 4, 256, 2, 2, 3), (768, 4, 256, 2, 1, 2), (512, 4, 1024, 1, 1, 2), (256, 4, 64, 2, 2, 1),
                                               (128, 4, 64, 1, 1, 2), (512, 1, 256, 1, 5, 1), (768, 1, 256, 1, 3, 1)])
def test_one_pass_cross_attention(C_, nh, P_, ctx, B, Fr):
    """The one-pass attention kernel (head dims 128 / 192 of the 64x64 and 256x256 tokenizers, 64 / 32 of the test models) against
    softmax(q k^T / sqrt(hd)) v in fp64 on the same bf16 inputs (conditional_vae.py:38-55); the last two cases are the diffusers
    Attention of the conditional mid blocks (compressive_vq_model.py:79,136): ONE head of 512 / 768 channels, every
    frame attending to its own 256 tokens (F = 1, B = frames)."""
    _, l = lib()
    torch.manual_seed(3)
    M, kv, hd = B * Fr, ctx * P_, C_ // nh
    q_ = (torch.randn(M, P_, C_) * 1.5).to(torch.bfloat16)
    k_ = (torch.randn(B, kv, C_) * 1.5).to(torch.bfloat16)
    v_ = torch.randn(B, kv, C_).to(torch.bfloat16)
    qd, kd, vtd = q_.to(DEV), k_.to(DEV), v_.transpose(1, 2).contiguous().to(DEV)
    out = torch.full((M, P_, C_), float("nan"), dtype=torch.bfloat16, device=DEV)
    assert l.ivg_op_xattn(P(qd), P(kd), P(vtd), P(out), M, Fr, P_, kv, C_, nh, 1, stream()) == 0
    torch.cuda.synchronize()
    qh = q_.double().view(B, Fr, P_, nh, hd).permute(0, 1, 3, 2, 4)             # B F h P d
    kh = k_.double().view(B, 1, kv, nh, hd).permute(0, 1, 3, 2, 4)              # B 1 h kv d
    vh = v_.double().view(B, 1, kv, nh, hd).permute(0, 1, 3, 2, 4)
    att = torch.softmax(qh @ kh.transpose(-1, -2) / hd ** 0.5, -1) @ vh          # B F h P d
    ref = att.permute(0, 1, 3, 2, 4).reshape(M, P_, C_)
    assert torch.isfinite(out.float()).all()
    assert rel_err(out, ref) < TOL["bf16"]
    # fp32 is not covered: the engine keeps the three-kernel path there
    assert l.ivg_op_xattn(P(qd), P(kd), P(vtd), P(out), M, Fr, P_, kv, C_, nh, 0, stream()) != 0
