"""The I3D detector and FVD on the device (csrc/i3d.hip through the C ABI and ivideogpt_amd/i3d.py) against tests/i3d_ref.py, the
fp64 restatement with seeded He-initialised weights.  Runs on the MI355X only (-m gpu).

Bounds (u = 2^-24).
Convolutions: per element |y - y64| <= gamma_(K + 2) (sum |x w| + |b|) -- the dot-product bound for any summation order plus bias add
and final rounding; y64 is computed in fp64 from the packed fp32 weights and the fp32 input, so the bound covers the kernel's
arithmetic alone.  Max-pool and ReLU are exact.
Front end: a frame value is  2 (hy (hx a + lx b) + ly (hx c + lx d)) - 1  with a .. d in [0, 1].  Each interpolation weight is the exact
rational rounded once (l) or that and one subtraction (h = 1 - l): |l^ - l| <= u l, |h^ - h| <= u (l + h) = u.  A horizontal pair
carries the weights' errors (<= 2u), two products and one sum of values <= 1 (<= 2u): 4u.  The vertical pair carries 4u (a convex
combination of the two), its weights' 2u, two products and one sum, 2u: 8u.  Doubling is exact and doubles the error, the final
subtraction rounds a value <= 1: 17u.  (Fused multiply-adds only remove roundings.)
Head: every input passes through at most 2P (average) + 1 (division) + C + 6 (dot product: lane chain and butterfly) + 1 (bias) +
Tn + 1 (time mean) roundings:  |f - f64| <= gamma_(2P + C + Tn + 12) (mean_t (sum_c mean|x| |w|) + |b|).
End to end: deviation = max over clips of max |f - f64| / max |f64|, at most 8 x the deviation of the same restatement evaluated in
fp32 on the CPU (another summation order, not another arithmetic) and at most 1e-4."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import i3d_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_SD, _DET = {}, {}


def sd_of(div):
    if div not in _SD:
        _SD[div] = R.random_i3d_state_dict(40 + div, width_div=div)
    return _SD[div]


def detector(div, S, max_clips=None):
    from ivideogpt_amd.i3d import I3D
    key = (div, S)
    if key not in _DET:
        _DET[key] = I3D.from_state_dict(sd_of(div), resize=S).to(DEV)
    _DET[key].max_clips = max_clips
    return _DET[key]


def lib():
    from ivideogpt_amd import _lib
    return _lib, _lib.load()


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def geometry(a, dims, k, s):
    for i in range(3):
        a.k[i], a.s[i], a.p[i] = k[i], s[i], R.same_pad(dims[i], k[i], s[i])[0]
    a.D, a.H, a.Wd = dims
    a.Do, a.Ho, a.Wo = (-(-dims[i] // s[i]) for i in range(3))
    return a.Do, a.Ho, a.Wo


def conv3d(x_cl, w, b, k, s, relu=True, Y=None, coff=0, x_off=0, cin=None):
    """ivg_op_conv3d on x_cl (B, D, H, W, ldx): input channels [x_off, x_off + cin), output into channels [coff, coff + Cout) of Y"""
    L, lb = lib()
    n, D, H, W, ldx = x_cl.shape
    cin = ldx if cin is None else cin
    a = L.IvgConv3dArgs()
    do, ho, wo = geometry(a, (D, H, W), k, s)
    if Y is None:
        Y = torch.full((n, do, ho, wo, w.shape[0]), float("nan"), device=DEV)
    a.X, a.W, a.bias, a.Y = x_cl.data_ptr() + 4 * x_off, w.data_ptr(), b.data_ptr(), Y.data_ptr()
    a.n, a.Cin, a.ldx, a.Cout, a.ldy, a.coff, a.relu = n, cin, ldx, w.shape[0], Y.shape[-1], coff, int(relu)
    assert lb.ivg_op_conv3d(C.byref(a), stream()) == 0
    torch.cuda.synchronize()
    return Y


def pool3d(x_cl, k, s):
    L, lb = lib()
    n, D, H, W, c = x_cl.shape
    a = L.IvgPool3dArgs()
    do, ho, wo = geometry(a, (D, H, W), k, s)
    Y = torch.full((n, do, ho, wo, c), float("nan"), device=DEV)
    a.X, a.Y, a.n, a.C, a.ldx, a.ldy, a.coff = x_cl.data_ptr(), Y.data_ptr(), n, c, c, c, 0
    assert lb.ivg_op_pool3d(C.byref(a), stream()) == 0
    torch.cuda.synchronize()
    return Y


def he_conv(g, cout, cin, k):
    K = k[0] * k[1] * k[2] * cin
    return torch.randn(cout, K, generator=g) * (2.0 / K) ** 0.5, 0.1 * torch.randn(cout, generator=g)


def check_conv(y, x_cl, w, b, k, s, relu, what):
    y64, bound = R.conv_oracle(x_cl.cpu(), w.cpu(), b.cpu(), k, s, relu)
    err = (y.cpu().double() - y64).abs()
    ratio = (err / bound.clamp_min(1e-300)).max().item()
    print(f"{what}: max err {err.max().item():.3e}, worst err / bound {ratio:.3f}")
    assert torch.isfinite(y).all() and y.shape == y64.shape, what
    assert (err <= bound).all(), (what, ratio)


@pytest.mark.parametrize("case", range(len(R.CONV_CASES)))
def test_conv3d_within_the_dot_product_bound(case):
    k, s, cin, cout, dims, relu = R.CONV_CASES[case]
    g = torch.Generator().manual_seed(200 + case)
    x = torch.randn(2, *dims, cin, generator=g).to(DEV)
    w, b = (t.to(DEV) for t in he_conv(g, cout, cin, k))
    check_conv(conv3d(x, w, b, k, s, relu), x, w, b, k, s, relu, f"case {case + 1}")


def test_conv3d_writes_only_its_channel_slice_and_reads_a_strided_input():
    g = torch.Generator().manual_seed(300)
    k, s = (3, 3, 3), (1, 1, 1)
    wide = torch.randn(2, 3, 5, 4, 16, generator=g).to(DEV)
    w, b = (t.to(DEV) for t in he_conv(g, 10, 6, k))
    Y = torch.full((2, 3, 5, 4, 24), float("nan"), device=DEV)
    Y[..., 20:] = 7.0
    before = Y.clone().view(torch.int32)
    conv3d(wide, w, b, k, s, True, Y=Y, coff=5, x_off=4, cin=6)
    check_conv(Y[..., 5:15].contiguous(), wide[..., 4:10].contiguous(), w, b, k, s, True, "slice")
    after = Y.view(torch.int32)
    assert torch.equal(after[..., :5], before[..., :5]) and torch.equal(after[..., 15:], before[..., 15:])
    # vector path: 8 of 16 input channels from offset 8, 12 outputs at offset 4 of 24
    w, b = (t.to(DEV) for t in he_conv(g, 12, 8, k))
    Y2 = torch.full((2, 3, 5, 4, 24), float("nan"), device=DEV)
    before = Y2.clone().view(torch.int32)
    conv3d(wide, w, b, k, s, True, Y=Y2, coff=4, x_off=8, cin=8)
    check_conv(Y2[..., 4:16].contiguous(), wide[..., 8:16].contiguous(), w, b, k, s, True, "vector slice")
    after = Y2.view(torch.int32)
    assert torch.equal(after[..., :4], before[..., :4]) and torch.equal(after[..., 16:], before[..., 16:])


@pytest.mark.parametrize("cin,cout", [(6, 10), (16, 70)])
def test_relu_epilogue_is_relu_of_the_plain_result(cin, cout):
    g = torch.Generator().manual_seed(310 + cin)
    k, s = (3, 3, 3), (1, 1, 1)
    x = torch.randn(2, 3, 6, 5, cin, generator=g).to(DEV)
    w, b = (t.to(DEV) for t in he_conv(g, cout, cin, k))
    plain, act = conv3d(x, w, b, k, s, False), conv3d(x, w, b, k, s, True)
    assert (plain < 0).any() and (plain > 0).any()
    assert torch.equal(act.view(torch.int32), F.relu(plain).view(torch.int32))


POOL_CASES = [((1, 3, 3), (1, 2, 2), (2, 7, 9)), ((1, 3, 3), (1, 2, 2), (3, 8, 6)),      # MaxPool3d_2a / 3a
              ((3, 3, 3), (2, 2, 2), (5, 7, 8)), ((3, 3, 3), (2, 2, 2), (4, 6, 5)),      # 4a
              ((2, 2, 2), (2, 2, 2), (3, 5, 4)), ((2, 2, 2), (2, 2, 2), (4, 4, 7)),      # 5a, D = 3
              ((3, 3, 3), (1, 1, 1), (3, 4, 5)), ((3, 3, 3), (1, 1, 1), (2, 7, 2))]      # b3a


@pytest.mark.parametrize("k,s,dims", POOL_CASES)
def test_pool3d_is_bit_exact_with_padded_zeros_in_the_maximum(k, s, dims):
    g = torch.Generator().manual_seed(sum(dims) + k[0])
    x = torch.randn(2, *dims, 13, generator=g) - 0.5       # mostly negative: the padded zeros decide maxima at the borders
    want = R.cl(R.max_pool(R.cf(x), k, s))
    got = pool3d(x.to(DEV), k, s).cpu()
    assert got.shape == want.shape and (want == 0).any()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))


@pytest.mark.parametrize("H,S,dtype", [(64, 224, torch.float32), (64, 64, torch.float32), (256, 224, torch.float32), (64, 224, torch.bfloat16),
                                       (48, 96, torch.float32)])
def test_front_end_against_fp64_interpolate(H, S, dtype):
    _, lb = lib()
    W = H if H != 48 else 40
    v = torch.rand(1, 3, 3, H, W, generator=torch.Generator().manual_seed(H + S)).to(dtype)
    want = R.cl(R.front_end(v.double(), S))                 # (1, 3 frames, S, S, 3)
    out = torch.full((3, S, S, 3), float("nan"), device=DEV)
    vd = v.to(DEV)
    assert lb.ivg_op_i3d_ingest(P(vd), 1 if dtype == torch.bfloat16 else 0, 3, H, W, S, P(out), stream()) == 0
    torch.cuda.synchronize()
    err = (out.cpu().double() - want[0]).abs().max().item()
    print(f"front end {H}x{W} -> {S}: max err {err:.3e} (bound {17 * R.U:.3e})")
    assert err <= 17 * R.U
    if H == S == W:
        assert torch.equal(out.cpu(), (2 * v[0].float() - 1).permute(0, 2, 3, 1))


@pytest.mark.parametrize("D", [2, 3, 4])
def test_head_within_its_bound(D):
    _, lb = lib()
    g = torch.Generator().manual_seed(400 + D)
    n, hw, c, nout = 3, 2, 70, 400
    x = torch.randn(n, D, hw, hw, c, generator=g)
    w, b = torch.randn(nout, c, generator=g) * (2.0 / c) ** 0.5, 0.1 * torch.randn(nout, generator=g)
    out = torch.full((n, nout), float("nan"), device=DEV)
    ws = torch.empty(n * (D - 1) * c, device=DEV)
    assert lb.ivg_op_i3d_head(P(x.to(DEV)), P(w.to(DEV)), P(b.to(DEV)), P(out), n, D, hw * hw, c, nout, P(ws), ws.numel() * 4, stream()) == 0
    torch.cuda.synchronize()
    sd = {"logits.conv3d.weight": w.reshape(nout, c, 1, 1, 1), "logits.conv3d.bias": b}
    want = R.head(sd, R.cf(x.double()))
    mag = R.head({"logits.conv3d.weight": w.abs().reshape(nout, c, 1, 1, 1), "logits.conv3d.bias": b.abs()}, R.cf(x.double().abs()))
    bound = R.gamma(2 * hw * hw + c + (D - 1) + 12) * mag
    err = (out.cpu().double() - want).abs()
    print(f"head D = {D}: worst err / bound {(err / bound).max().item():.3f}")
    assert (err <= bound).all()


@pytest.mark.parametrize("div,S,T,B", [(4, 64, 12, 2), (1, 224, 16, 1)])
def test_every_unit_of_a_forward(div, S, T, B):
    """each unit is fed the fp32 tap of the unit(s) before it: convolutions within the dot-product bound, pools bit-exact"""
    from ivideogpt_amd.packing import pack_i3d
    det = detector(div, S)
    packed = pack_i3d(sd_of(div))
    v = torch.rand(B, T, 3, 64, 64, generator=torch.Generator().manual_seed(500 + div)).to(DEV)
    assert det.num_units() == len(R.UNITS)
    taps = {-1: det.tap(v, -1)[0].cpu()}
    worst = 0.0
    for i, (name, kind, k, s, src) in enumerate(R.UNITS):
        y, got_src = det.tap(v, i)
        assert got_src == src, (name, got_src, src)
        y = taps[i] = y.cpu()
        x = taps[src[0]] if len(src) == 1 else torch.cat([taps[j] for j in src], -1)
        if kind == "pool":
            want = R.cl(R.max_pool(R.cf(x), k, s))
            assert y.shape == want.shape and torch.equal(y.view(torch.int32), want.view(torch.int32)), name
            continue
        y64, bound = R.conv_oracle(x, packed[f"{name}.weight"], packed[f"{name}.bias"], k, s, True)
        assert y.shape == y64.shape and torch.isfinite(y).all(), name
        err = (y.double() - y64).abs()
        worst = max(worst, (err / bound.clamp_min(1e-300)).max().item())
        assert (err <= bound).all(), (name, worst)
        live = {j for (_, _, _, _, sr) in R.UNITS[i + 1:] for j in sr}
        taps = {j: t for j, t in taps.items() if j in live}
    print(f"1/{div} width, S {S}, T {T}: worst err / bound over the convolutions {worst:.3f}")


E2E = [(4, 64, 12, 3, 64), (4, 32, 9, 3, 48), (8, 64, 16, 3, 64), (4, 64, 30, 2, 64), (1, 224, 16, 1, 64)]


@pytest.mark.parametrize("div,S,T,B,H", E2E)
def test_features_end_to_end(div, S, T, B, H):
    sd = sd_of(div)
    v = torch.rand(B, T, 3, H, H, generator=torch.Generator().manual_seed(600 + div + T))
    f64 = R.forward(sd, v, S, torch.float64)
    d32 = R.feature_deviation(R.forward(sd, v, S, torch.float32), f64)
    f = detector(div, S).features(v.to(DEV)).cpu()
    dev = R.feature_deviation(f, f64)
    print(f"1/{div} width, S {S}, T {T}: deviation {dev:.3e}, fp32 CPU restatement {d32:.3e}")
    assert f.shape == (B, 400) and torch.isfinite(f).all()
    assert dev <= 8 * d32 and dev <= 1e-4


def test_chunking_and_repetition_do_not_change_a_bit():
    v = torch.rand(5, 12, 3, 64, 64, generator=torch.Generator().manual_seed(700)).to(DEV)
    runs = [detector(4, 64, max_clips=c).features(v) for c in (1, 2, 5, 5)]
    bf = detector(4, 64, max_clips=2).features(v.bfloat16())
    torch.cuda.synchronize()
    for r in runs[1:]:
        assert torch.equal(r.view(torch.int32), runs[0].view(torch.int32))
    assert torch.equal(bf, detector(4, 64, max_clips=5).features(v.bfloat16().float()))     # a bf16 clip is read exactly


def test_refusals_leave_the_output_untouched():
    L, lb = lib()
    det = detector(8, 64)
    out = torch.full((2, 400), 7.5, device=DEV)
    ws = torch.empty(lb.ivg_i3d_ws_bytes(det._handle, 2, 12, 64, 64), dtype=torch.uint8, device=DEV)
    assert ws.numel() > 0
    ok = torch.rand(2, 12, 3, 64, 64, device=DEV)
    call = lambda h, v, T, ws_bytes: lb.ivg_i3d_features(h, P(v), 0, 2, T, v.shape[3], v.shape[4], P(out), P(ws), ws_bytes, stream())
    assert call(det._handle, ok[:, :8].contiguous(), 8, ws.numel()) == -1                    # T too short
    assert call(None, ok, 12, ws.numel()) == -1                                              # null handle
    assert call(det._handle, ok, 12, lb.ivg_i3d_ws_bytes(det._handle, 1, 12, 64, 64) - 1) == -4   # a short scratch
    from ivideogpt_amd.i3d import I3D
    odd = I3D.from_state_dict(sd_of(8), resize=64)
    odd.resize = 48                                                                          # S not a multiple of 32 (the class refuses it up front)
    odd.to(DEV)
    assert lb.ivg_i3d_ws_bytes(odd._handle, 1, 12, 64, 64) == 0
    assert call(odd._handle, ok, 12, ws.numel()) == -1
    torch.cuda.synchronize()
    assert (out == 7.5).all()
    with pytest.raises(ValueError):
        det.features(ok[:, :8])
    with pytest.raises(ValueError):
        I3D.from_state_dict(sd_of(8), resize=48)
    # a missing and a mis-shaped tensor are named
    from ivideogpt_amd.packing import pack_i3d
    for mutate, word in ((lambda p: p.pop("Mixed_4d.b2a.bias"), "missing"), (lambda p: p.update({"Mixed_4d.b2b.weight": p["Mixed_4d.b2b.weight"][:, :-1].contiguous()}), "columns")):
        packed = pack_i3d(sd_of(8))
        mutate(packed)
        with pytest.raises((L.IvgError, AssertionError)) as e:
            I3D(packed, resize=64).to(DEV)
        assert "Mixed_4d.b2" in str(e.value) and word in str(e.value)
    assert call(det._handle, ok, 12, ws.numel()) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(out).all() and not (out == 7.5).any()


def test_fvd_value_and_ordering():
    from ivideogpt_amd.metrics import Evaluator, FeatureStats, frechet_distance
    sd = sd_of(8)
    ev = Evaluator(i3d=detector(8, 32))
    g = torch.Generator().manual_seed(800)
    base = torch.rand(48, 1, 3, 8, 8, generator=g)
    real = F.interpolate(base.reshape(48, 3, 8, 8), size=32, mode="bilinear").reshape(48, 1, 3, 32, 32).repeat(1, 9, 1, 1, 1)
    real = (real + 0.05 * torch.rand(48, 9, 3, 32, 32, generator=g)).clamp(0, 1)             # smooth clips with a little motion
    noise = torch.randn(48, 9, 3, 32, 32, generator=g)
    gens = {a: (real + a * noise).clamp(0, 1) for a in (0.02, 0.1, 0.5)}

    def ref_stats(x):
        s = FeatureStats()
        s.append_torch(R.forward(sd, x, 32, torch.float64))
        return s.get_mean_cov()

    batched = lambda x: x.reshape(4, 12, *x.shape[1:]).to(DEV)
    mu_r, sig_r = ref_stats(real)
    fvd = {}
    for a, gen in gens.items():
        fvd[a] = ev.compute_fvd_from_raw_data(batched(real), batched(gen))
        mu_g, sig_g = ref_stats(gen)
        want = frechet_distance(mu_g, sig_g, mu_r, sig_r)
        print(f"noise {a}: FVD {fvd[a]:.6g}, from the fp64 features {want:.6g}")
        assert abs(fvd[a] - want) <= 1e-3 * abs(want)
    assert 0 < fvd[0.02] < fvd[0.1] < fvd[0.5]
    same = ev.compute_fvd_from_raw_data(batched(real), batched(real))
    assert abs(same) <= 1e-6 * sig_r.trace()
    with pytest.raises(RuntimeError):
        Evaluator().i3d_features(batched(real)[0])


def test_train_gpt_main_logs_a_finite_fvd():
    import math
    import train_gpt
    logs = train_gpt.main(["--use_fvd", "--i3d_random", "0", "--i3d_width_div", "8", "--i3d_resize", "64", "--batch", "2", "--iters", "2",
                           "--eval_generate_times", "2", "--max_decode_batchsize", "3"])
    assert math.isfinite(logs["eval/fvd"]) and logs["eval/fvd"] >= 0 and math.isfinite(logs["eval/psnr"])
