"""LPIPS on the device (csrc/lpips.hip through the C ABI and its Python mirror) against tests/lpips_ref.py, the fp64 restatement
with seeded random weights.  Runs on the MI355X only (-m gpu).

Bounds.  Convolutions: per element |y - y64| <= gamma_n (sum |x w| + |b|), n = 9 Cin + 2, u = 2^-24 -- the dot-product bound for any
summation order plus bias add and final rounding; y64 is computed in fp64 from the fp32-rounded weights, biases and inputs, so the
bound covers the kernel's arithmetic alone.  (The input layer also scales its input in fp32; its oracle scales the fp32 image in
fp64.)  Max-pool and ReLU are exact.  Head, per image, from the kernel's operation count: a normalised feature carries a relative
error of at most (C / 2 + 3) u (sum of C squares, square root, guard add, division), taken as e1 = gamma_(C + 8); the lin-weighted
sum over a lane's share of pixels and channels is an fp32 chain of at most P C / 256 terms, the rest runs in fp64: e2 =
gamma_(P C / 256 + 12).  With d = n0 - n1:  |v - v64| <= mean_p sum_c lin_c (2 |d| (|n0| + |n1|) e1 + d^2 e2).
End to end: 1e-3 relative (the project's parity bar) and 8 delta, delta = the largest relative deviation of the same restatement
evaluated in fp32 on the CPU from fp64 over the case's inputs."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

import lpips_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SD = R.random_state_dict(20)


def lib():
    from ivideogpt_amd import _lib
    return _lib, _lib.load()


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def metric():
    from ivideogpt_amd.lpips import LPIPS
    return LPIPS.from_state_dict(SD).to(DEV)


def conv_layer(l, x_nhwc, relu=True):
    """layer l >= 1 on the GPU through ivg_op_igemm, the dispatch the trunk uses (conv3x3.hip, else igemm.hip)"""
    L, lb = lib()
    from ivideogpt_amd.packing import pack_lpips
    s, i, cin, cout = R.CONVS[l]
    pk = pack_lpips(SD)
    w, b = pk[f"net.slice{s}.{i}.weight"].to(DEV), pk[f"net.slice{s}.{i}.bias"].to(DEV)
    n, H, W, _ = x_nhwc.shape
    Y = torch.full((n, H, W, cout), float("nan"), device=DEV)
    a = L.IvgIgemmArgs()
    a.X, a.W, a.Y, a.R, a.bias = x_nhwc.data_ptr(), w.data_ptr(), Y.data_ptr(), None, b.data_ptr()
    for k, v in dict(Nimg=n, Hin=H, Win=W, Cin=cin, ldx=cin, Hout=H, Wout=W, KH=3, KW=3, stride=1, pad=1, ups=0, N=cout, ldw=9 * cin,
                     c_img=H * W * cout, c_pix=cout, c_ch=1, c_grp=1, c_grp_stride=0, flags=L.IG_BIAS_N | (L.IG_RELU if relu else 0), alpha=1.0,
                     nb0=1, nb1=1, nb2=1).items():
        setattr(a, k, v)
    assert lb.ivg_op_igemm(C.byref(a), 0, stream()) == 0
    torch.cuda.synchronize()
    return Y


@pytest.mark.parametrize("res,n", [(64, 2), (256, 1), (16, 2)])
def test_every_convolution_within_the_dot_product_bound(res, n):
    L, lb = lib()
    from ivideogpt_amd.packing import pack_lpips
    g = torch.Generator().manual_seed(100 + res)
    x = torch.rand(n, 3, res, res, generator=g)
    ins, _ = R.layer_inputs(SD, x)
    pk = pack_lpips(SD)
    worst = []
    for l, (s, i, cin, cout) in enumerate(R.CONVS):
        w, b = SD[f"net.slice{s}.{i}.weight"], SD[f"net.slice{s}.{i}.bias"]
        if l == 0:
            x64 = R.scale_input(x, torch.float64)
            Y = torch.full((n, res, res, 64), float("nan"), device=DEV)
            xd = x.to(DEV)
            assert lb.ivg_op_lpips_conv_in(P(xd), 0, P(pk["net.slice1.0.weight"].to(DEV)), P(pk["net.slice1.0.bias"].to(DEV)), P(Y), n, res, res,
                                           stream()) == 0
            torch.cuda.synchronize()
        else:
            x32 = ins[l].float()
            x64 = x32.double()
            Y = conv_layer(l, nhwc(x32).to(DEV))
        y64 = F.relu(F.conv2d(x64, w.double(), b.double(), padding=1))
        bound = R.conv_bound(x64, w, b)
        err = (Y.cpu().double().permute(0, 3, 1, 2) - y64).abs()
        ratio = (err / bound.clamp_min(1e-300)).max().item()
        worst.append(ratio)
        print(f"res {res} conv {l + 1:2d} ({cin:3d} -> {cout:3d}, {x64.shape[-1]:3d}^2): max |err| / bound = {ratio:.3f}, max |err| = {err.max().item():.3e}")
    assert all(math.isfinite(r) and r <= 1.0 for r in worst), worst


@pytest.mark.parametrize("n,H,W,Cc", [(3, 64, 64, 64), (2, 16, 32, 128), (2, 8, 8, 512), (1, 2, 2, 512), (1, 256, 256, 64)])
def test_maxpool_is_exact(n, H, W, Cc):
    _, lb = lib()
    g = torch.Generator().manual_seed(7)
    x = torch.randn(n, H, W, Cc, generator=g)
    xd = x.to(DEV)
    Y = torch.full((n, H // 2, W // 2, Cc), float("nan"), device=DEV)
    assert lb.ivg_op_maxpool2(P(xd), P(Y), n, H, W, Cc, stream()) == 0
    torch.cuda.synchronize()
    ref = F.max_pool2d(x.permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1)
    assert torch.equal(Y.cpu().view(torch.int32), ref.contiguous().view(torch.int32))


@pytest.mark.parametrize("l,res", [(1, 64), (5, 16), (9, 8), (12, 4)])     # conv3x3.hip (64, 16) and igemm.hip (8, 4)
def test_relu_epilogue_is_exact(l, res):
    g = torch.Generator().manual_seed(8)
    x = torch.randn(2, res, res, R.CONVS[l][2], generator=g).to(DEV)
    plain, relu = conv_layer(l, x, relu=False), conv_layer(l, x, relu=True)
    assert (plain < 0).any() and torch.equal(relu, torch.relu(plain))


def head_bound(f0, f1, lin, Pn, Cc):
    f0, f1, lin = f0.double(), f1.double(), lin.double().view(1, -1, 1, 1)
    n0 = f0 / (f0.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
    n1 = f1 / (f1.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
    gam = lambda k: k * R.U / (1 - k * R.U)
    d = (n0 - n1).abs()
    return (lin * (2 * d * (n0.abs() + n1.abs()) * gam(Cc + 8) + d * d * gam(Pn * Cc / 256 + 12))).sum(1).mean((1, 2))


def test_head_per_image():
    _, lb = lib()
    g = torch.Generator().manual_seed(30)
    n0, t = 2, 3
    x0 = torch.rand(n0, 3, 64, 64, generator=g)
    x1 = (x0.repeat(t, 1, 1, 1) + 0.2 * torch.randn(t * n0, 3, 64, 64, generator=g)).clamp(0, 1)
    t0 = [v.float() for v in R.taps_of(SD, x0)]
    t1 = [v.float() for v in R.taps_of(SD, x1)]
    for k in range(5):
        Cc, Pn = R.TAP_C[k], (64 >> k) ** 2
        t0[k][0, :, 0, 0] = 0          # an all-zero feature pixel on both sides, and on one side only
        t1[k][0, :, 0, 0] = 0
        t1[k][1, :, -1, -1] = 0
        t1[k][n0] = t0[k][0]           # image n0 of f1 pairs with image 0 of f0: identical inputs
        lin = SD[f"lin{k}.model.1.weight"].reshape(-1)
        f0, f1 = nhwc(t0[k]).to(DEV), nhwc(t1[k]).to(DEV)
        out = torch.full((t * n0,), float("nan"), device=DEV)
        ws = torch.zeros(t * n0 * 128, dtype=torch.uint8, device=DEV)
        assert lb.ivg_op_lpips_head(P(f0), P(f1), P(lin.to(DEV)), n0, t * n0, Pn, Cc, P(out), P(ws), ws.numel(), stream()) == 0
        torch.cuda.synchronize()
        ref = R.head(t0[k].repeat(t, 1, 1, 1), t1[k], lin)
        bound = head_bound(t0[k].repeat(t, 1, 1, 1), t1[k], lin, Pn, Cc)
        err = (out.cpu().double() - ref).abs()
        print(f"tap {k}: values {ref.tolist()}, max |err| / bound = {(err / bound.clamp_min(1e-300)).max().item():.3f}")
        assert torch.isfinite(out).all() and out[n0].item() == 0.0
        assert (err <= bound).all(), (err, bound)


def clips(B, T, t, noise, gt_dt, seed):
    g = torch.Generator().manual_seed(seed)
    Tg, Tp, gt_t0, pr_t0 = T + 2, T + 3, 1, 2
    gt = torch.rand(B, Tg, 3, 64, 64, generator=g).to(gt_dt)
    pred = torch.rand(t * B, Tp, 3, 64, 64, generator=g)
    win = gt[:, gt_t0:gt_t0 + T].float().repeat(t, 1, 1, 1, 1)
    pred[:, pr_t0:pr_t0 + T] = (win + noise * torch.randn(win.shape, generator=g)).clamp(0, 1)
    return gt, pred, gt_t0, pr_t0


@pytest.mark.parametrize("noise", [0.02, 0.1, 0.5])
@pytest.mark.parametrize("gt_dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("t", [1, 3])
def test_rows_end_to_end(t, gt_dt, noise):
    B, T = 4, 3
    gt, pred, gt_t0, pr_t0 = clips(B, T, t, noise, gt_dt, 40 + t)
    m = metric()
    frames, rows = m.frames_and_rows(gt.to(DEV), pred.to(DEV), gt_t0=gt_t0, pred_t0=pr_t0, frames=T)
    f64, r64 = R.clip_lpips(SD, gt, pred, gt_t0, pr_t0, T)
    f32, r32 = R.clip_lpips(SD, gt, pred, gt_t0, pr_t0, T, dt=torch.float32)
    rel = lambda a, b: ((a.double().cpu() - b).abs() / b.abs()).max().item()
    delta = max(rel(f32, f64), rel(r32, r64))
    dev = max(rel(frames, f64), rel(rows, r64))
    print(f"t {t} {gt_dt} noise {noise}: rows {r64.tolist()}; delta (fp32 CPU vs fp64) = {delta:.3e}, GPU vs fp64 = {dev:.3e}, ratio {dev / delta:.2f}")
    assert frames.shape == (t * B, T) and rows.shape == (B,)
    assert dev <= 1e-3, dev
    assert dev <= 8 * delta, (dev, delta)


def test_chunk_invariance_determinism_and_image_count():
    _, lb = lib()
    B, T, t = 4, 3, 3
    gt, pred, gt_t0, pr_t0 = clips(B, T, t, 0.1, torch.float32, 50)
    gt, pred = gt.to(DEV), pred.to(DEV)
    m = metric()
    outs = []
    for cap in (2, 7, None, None):
        c0 = lb.ivg_debug_counter(b"lpips_trunk_images")
        f, r = m.frames_and_rows(gt, pred, gt_t0=gt_t0, pred_t0=pr_t0, frames=T, max_images=cap)
        torch.cuda.synchronize()
        assert lb.ivg_debug_counter(b"lpips_trunk_images") - c0 == B * T * (1 + t), cap
        outs.append((f.clone(), r.clone()))
    for f, r in outs[1:]:
        assert torch.equal(f.view(torch.int32), outs[0][0].view(torch.int32)) and torch.equal(r.view(torch.int32), outs[0][1].view(torch.int32))
    # frames_out = NULL: the per-frame values live in the workspace; same rows
    rows = torch.full((B,), float("nan"), device=DEV)
    nbytes = lb.ivg_lpips_ws_bytes(5, 64, 64) + t * B * T * 4 + 256
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    assert lb.ivg_lpips_rows(m._handle, P(gt), 0, B, T + 2, gt_t0, P(pred), t * B, T + 3, pr_t0, T, 64, 64, None, P(rows), P(ws), nbytes, stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(rows.view(torch.int32), outs[0][1].view(torch.int32))


def test_features_hook_matches_the_oracle_taps():
    _, lb = lib()
    g = torch.Generator().manual_seed(60)
    x = torch.rand(3, 3, 32, 32, generator=g)
    m = metric()
    taps = [torch.full((3, 32 >> k, 32 >> k, R.TAP_C[k]), float("nan"), device=DEV) for k in range(5)]
    arr = (C.c_void_p * 5)(*[t.data_ptr() for t in taps])
    nbytes = lb.ivg_lpips_ws_bytes(2, 32, 32)       # three images through a two-image workspace
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    xd = x.to(DEV)
    assert lb.ivg_op_lpips_features(m._handle, P(xd), 0, 3, 32, 32, arr, P(ws), nbytes, stream()) == 0
    torch.cuda.synchronize()
    ref = R.taps_of(SD, x)
    for k in range(5):
        e = (taps[k].cpu().double().permute(0, 3, 1, 2) - ref[k]).abs().max().item() / ref[k].abs().max().item()
        print(f"tap {k}: max error relative to the tap's scale {e:.3e}")
        assert e < 1e-5


def test_refusals_leave_the_output_untouched():
    L, lb = lib()
    from ivideogpt_amd.packing import pack_lpips
    B, T, t = 2, 2, 2
    gt, pred = torch.rand(B, T, 3, 64, 64, device=DEV), torch.rand(t * B, T, 3, 64, 64, device=DEV)
    m = metric()
    rows = torch.full((B,), float("nan"), device=DEV)
    nbytes = lb.ivg_lpips_ws_bytes(4, 64, 64)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)

    def call(H=64, W=64, n=t * B, nb=nbytes):
        return lb.ivg_lpips_rows(m._handle, P(gt), 0, B, T, 0, P(pred), n, T, 0, T, H, W, None, P(rows), P(ws), nb, stream())
    assert call(H=24) == -1 and call(n=3) == -1
    assert call(nb=lb.ivg_lpips_ws_bytes(1, 64, 64)) == -4 and call(nb=4096) == -4
    pk = {k: v.to(DEV) for k, v in pack_lpips(SD).items() if k != "net.slice5.26.weight"}
    names = [k.encode() for k in pk]
    tab = (L.IvgTensor * len(names))()
    for i, (k, v) in enumerate(pk.items()):
        tab[i].name, tab[i].data, tab[i].dtype, tab[i].ndim = names[i], v.data_ptr(), 0, v.dim()
        for d, s in enumerate(v.shape):
            tab[i].shape[d] = s
    h = C.c_void_p()
    assert lb.ivg_lpips_create(tab, len(names), 0, C.byref(h)) == -2 and not h.value
    torch.cuda.synchronize()
    assert torch.isnan(rows).all()
    with pytest.raises(AssertionError):
        m(gt[..., :24, :], pred[..., :24, :])


def test_evaluator_returns_the_real_fourth_value():
    from ivideogpt_amd.metrics import Evaluator
    B, T, t = 4, 3, 3
    gt, pred, _, _ = clips(B, T, t, 0.1, torch.float32, 70)
    ev = Evaluator(max_batchsize=5, lpips=metric())
    out = ev(gt.to(DEV), pred.to(DEV))
    _, r64 = R.clip_lpips(SD, gt, pred)
    _, r32 = R.clip_lpips(SD, gt, pred, dt=torch.float32)
    delta = ((r32.double() - r64).abs() / r64).max().item()
    got, want = out[3].item(), r64.mean().item()
    print(f"Evaluator lpips {got:.9e} vs oracle {want:.9e}; delta {delta:.3e}")
    assert len(out) == 4 and math.isfinite(got) and abs(got - want) <= min(1e-3, 8 * delta) * want
    r4 = ev.rows4(gt.to(DEV), pred.to(DEV))
    assert r4.shape == (B, 4) and ev.rows(gt.to(DEV), pred.to(DEV)).shape == (B, 3)
    assert ((r4[:, 3].cpu().double() - r64).abs() <= min(1e-3, 8 * delta) * r64).all()
    assert math.isnan(Evaluator()(gt.to(DEV), pred.to(DEV))[3].item())


def test_train_gpt_evaluate_logs_lpips(tmp_path):
    import train_gpt
    from safetensors.torch import save_file
    from ivideogpt_amd import CompressiveVQModel, LlamaForCausalLM, weights as W
    from ivideogpt_amd.metrics import Evaluator
    from ivideogpt_amd.parallel import LocalAccelerator
    vgg, lin = R.torchvision_state_dicts(SD)
    save_file({k: v.contiguous() for k, v in vgg.items()}, str(tmp_path / "vgg16.safetensors"))
    torch.save(lin, str(tmp_path / "vgg.pth"))
    tcfg = W.tokenizer_config(block_out_channels=(64, 128, 128), layers_per_block=1, latent_channels=64, num_vq_embeddings=512, num_dyn_embeddings=512,
                              norm_num_groups=32, mid_block_add_attention=False, context_length=2, resolution=64, max_att_resolution=16)
    lcfg = dict(hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=2, rms_norm_eps=1e-6,
                rope_theta=10000.0, max_position_embeddings=1024, vocab_size=1026)
    tok = CompressiveVQModel(tcfg, W.random_tokenizer_state_dict(tcfg, 81, codebook_std=0.4), encode_dtype="fp32", decode_dtype="fp32").to(DEV)
    llm = LlamaForCausalLM(dict(lcfg), W.random_llama_state_dict(lcfg, 82), dtype="fp32").to(DEV)
    g = torch.Generator().manual_seed(83)
    T, ctx, B, t = 5, 2, 3, 2
    batches = [torch.rand(B, T, 3, 64, 64, generator=g)]
    args = train_gpt.eval_args(context_length=ctx, segment_length=T, eval_generate_times=t, max_generate_batchsize=B, max_decode_batchsize=4,
                               log_gif_interval=1000)
    ev = Evaluator(lpips=(str(tmp_path / "vgg16.safetensors"), str(tmp_path / "vgg.pth")))
    logs = train_gpt.evaluate(args, LocalAccelerator(DEV), tok, llm, batches, ev, 0)
    print(logs)
    assert math.isfinite(logs["eval/lpips"]) and logs["eval/lpips"] > 0
    logs0 = train_gpt.evaluate(args, LocalAccelerator(DEV), tok, llm, batches, Evaluator(), 0)
    assert math.isnan(logs0["eval/lpips"])
