"""Times ``ivg_lpips_rows`` (csrc/lpips.hip) with HIP events, warm, against the same restatement in fp32 through torch-ROCm's own
convolutions on the same GPU -- once with every ground-truth frame through the trunk once (what the engine does), once with the
ground truth repeated t times (what the reference does).  Seeded random weights (tests/lpips_ref.py).  Also a per-layer split of
the engine's trunk (each layer timed alone on the chunk's shape) and the fp32 MFMA fraction: 2 * 9 * Cin * Cout * pixels FLOP of
the twelve MFMA convolutions over the time of the call, against 157.3 TFLOP/s.

    python tools/lpips_bench.py [--repeats 20] [--out profiles/lpips_bench.txt]"""
import argparse
import ctypes as C
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import lpips_ref as R  # noqa: E402

DEV = "cuda:0"
PEAK_F32_MFMA = 157.3e12


def timed(fn, repeats, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return ms[len(ms) // 2], ms[0], ms[-1]


def trunk_flops(H, W):
    fl, h, w = 0.0, H, W
    for l, (_, _, cin, cout) in enumerate(R.CONVS):
        if l in R.POOL_BEFORE:
            h, w = h // 2, w // 2
        fl += 2.0 * 9 * cin * cout * h * w
    return fl


def torch_lpips(sd, gt, pred, B, T, t, repeat_gt, chunk):
    """fp32 restatement on the GPU through torch's convolutions; chunked like the reference's batch_forward"""
    g = gt.reshape(B * T, *gt.shape[2:])
    p = pred.reshape(t * B * T, *pred.shape[2:])
    taps = lambda x: [torch.cat(c) for c in zip(*[R.layer_inputs(sd, x[lo:lo + chunk], torch.float32)[1] for lo in range(0, x.shape[0], chunk)])]
    if repeat_gt:
        g = g.reshape(B, T, *g.shape[1:]).repeat(t, 1, 1, 1, 1).reshape(t * B * T, *g.shape[1:])
    return R.lpips_from_taps(sd, taps(g), taps(p), torch.float32).reshape(t, B, T).mean(-1).min(0).values


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from ivideogpt_amd import _lib
    from ivideogpt_amd.lpips import LPIPS
    from ivideogpt_amd.packing import pack_lpips
    lb = _lib.load()
    sd = R.random_state_dict(0)
    sd_dev = {k: v.to(DEV) for k, v in sd.items()}
    # R.scale_input builds its constants on the CPU: move them once
    R_scale = R.scale_input
    R.scale_input = lambda x, dt: ((x.to(dt) * 2 - 1) - torch.tensor(R.SHIFT, dtype=dt, device=x.device).view(1, 3, 1, 1)) / \
        torch.tensor(R.SCALE, dtype=dt, device=x.device).view(1, 3, 1, 1)
    m = LPIPS.from_state_dict(sd).to(DEV)
    lines = [f"device {torch.cuda.get_device_name(0)}; repeats {a.repeats} (median [min, max] ms), HIP events, 3 warm-up calls per shape"]
    for (B, T, t, res) in ((64, 14, 1, 64), (64, 14, 4, 64), (8, 14, 1, 256)):
        g = torch.Generator().manual_seed(1)
        gt = torch.rand(B, T, 3, res, res, generator=g).to(DEV)
        pred = (gt.repeat(t, 1, 1, 1, 1) + 0.1 * torch.randn(t * B, T, 3, res, res, generator=g).to(DEV)).clamp(0, 1)
        imgs = B * T * (1 + t)
        cap = 1024 if res == 64 else 56
        eng = timed(lambda: m(gt, pred, max_images=cap), a.repeats)
        chunk = 256 if res == 64 else 16
        with torch.no_grad():
            base1 = timed(lambda: torch_lpips(sd_dev, gt, pred, B, T, t, False, chunk), a.repeats)
            baser = timed(lambda: torch_lpips(sd_dev, gt, pred, B, T, t, True, chunk), a.repeats) if t > 1 else base1
            dev = ((m(gt, pred, max_images=cap) - torch_lpips(sd_dev, gt, pred, B, T, t, False, chunk)).abs() /
                   torch_lpips(sd_dev, gt, pred, B, T, t, False, chunk)).max().item()
        mf = (trunk_flops(res, res) - 2.0 * 27 * 64 * res * res) * imgs
        lines.append(f"B {B} T {T} t {t} {res}x{res}: {imgs} images, chunk {cap}: engine {eng[0]:.2f} [{eng[1]:.2f}, {eng[2]:.2f}] ms; "
                     f"torch fp32, ground truth once {base1[0]:.2f} [{base1[1]:.2f}, {base1[2]:.2f}] ms; torch fp32, ground truth repeated "
                     f"{baser[0]:.2f} [{baser[1]:.2f}, {baser[2]:.2f}] ms; engine vs torch max rel. difference {dev:.2e}; "
                     f"fp32 MFMA fraction of the engine call {mf / (eng[0] * 1e-3) / PEAK_F32_MFMA:.3f} ({mf / (eng[0] * 1e-3) / 1e12:.1f} TFLOP/s)")
        # per-layer split: each MFMA convolution alone on `n` images of its shape, through the trunk's own dispatch (ivg_op_igemm)
        n = min(cap, imgs)
        pk = {k: v.to(DEV) for k, v in pack_lpips(sd).items()}
        h = res
        for l, (s, i, cin, cout) in enumerate(R.CONVS):
            if l in R.POOL_BEFORE:
                h //= 2
            if l == 0:
                continue
            X = torch.rand(n, h, h, cin, device=DEV)
            Y = torch.empty(n, h, h, cout, device=DEV)
            args = _lib.IvgIgemmArgs()
            args.X, args.W, args.Y, args.R, args.bias = X.data_ptr(), pk[f"net.slice{s}.{i}.weight"].data_ptr(), Y.data_ptr(), None, pk[f"net.slice{s}.{i}.bias"].data_ptr()
            for k, v in dict(Nimg=n, Hin=h, Win=h, Cin=cin, ldx=cin, Hout=h, Wout=h, KH=3, KW=3, stride=1, pad=1, ups=0, N=cout, ldw=9 * cin,
                             c_img=h * h * cout, c_pix=cout, c_ch=1, c_grp=1, c_grp_stride=0, flags=_lib.IG_BIAS_N | _lib.IG_RELU, alpha=1.0,
                             nb0=1, nb1=1, nb2=1).items():
                setattr(args, k, v)
            st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            ms = timed(lambda: lb.ivg_op_igemm(C.byref(args), 0, st), max(5, a.repeats // 2), warm=2)
            wt = sd_dev[f"net.slice{s}.{i}.weight"]
            Xc = X.permute(0, 3, 1, 2).contiguous()
            tm = timed(lambda: F.conv2d(Xc, wt, sd_dev[f"net.slice{s}.{i}.bias"], padding=1), max(5, a.repeats // 2), warm=2)
            fl = 2.0 * 9 * cin * cout * h * h * n
            lines.append(f"    conv {l + 1:2d} {cin:3d}->{cout:3d} at {h:3d}^2 x {n} images ({'conv3x3.hip' if h >= 16 else 'igemm.hip'}): "
                         f"{ms[0]:.3f} ms = {fl / (ms[0] * 1e-3) / 1e12:.1f} TFLOP/s ({fl / (ms[0] * 1e-3) / PEAK_F32_MFMA:.2f} of peak); torch conv2d {tm[0]:.3f} ms")
        del gt, pred
        torch.cuda.empty_cache()
    R.scale_input = R_scale
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
