"""Times ``I3D.features`` (csrc/i3d.hip) with HIP events, warm, at the eval loop's shape -- full-width detector, clips of 16 frames
of 64 x 64 resized to 224 -- in ms per clip for B = 16 and 64, beside the same clips through the fp32 torch restatement of the tests
(tests/i3d_ref.py) on the same GPU, i.e. through torch-ROCm's own convolutions.  Seeded random weights.  Also where the engine's time
goes: a forward cut after the front end, the stem and each group of Mixed blocks (``ivg_op_i3d_tap`` stops there), differences
of the medians, with the convolution FLOP of the stage against the f32-input MFMA peak (157.3 TFLOP/s).

    python tools/fvd_bench.py [--repeats 10] [--out profiles/fvd_bench.txt]"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import i3d_ref as R  # noqa: E402

DEV = "cuda:0"
PEAK_F32_MFMA = 157.3e12


def timed(fn, repeats, warm=2):
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


def conv_flops(sd, T, S):
    """FLOP of every convolution unit of one clip, by unit index"""
    _, taps = R.forward(sd, torch.zeros(1, T, 3, 8, 8), S, torch.float32, taps=True)   # (one CPU forward, for the shapes)
    fl = {}
    for i, (name, kind, k, s, src) in enumerate(R.UNITS):
        if kind == "conv":
            w = sd[f"{name}.conv3d.weight"]
            fl[i] = 2.0 * w[0].numel() * w.shape[0] * taps[i][0, 0].numel()
    return fl


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--width_div", type=int, default=1)
    ap.add_argument("--skip_torch", action="store_true")
    a = ap.parse_args()
    from ivideogpt_amd.i3d import I3D
    T, H, S, chunk = 16, 64, 224, 8
    sd = R.random_i3d_state_dict(0, width_div=a.width_div)
    det = I3D.from_state_dict(sd, resize=S, max_clips=chunk).to(DEV)
    lines = []

    def say(line):
        lines.append(line)
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    say(f"device {torch.cuda.get_device_name(0)}; I3D width 1/{a.width_div}, clips {T} x {H} x {H} -> {S}, {chunk} clips per pass; "
        f"repeats {a.repeats} (median [min, max]), HIP events, 2 warm-up calls")
    fl = conv_flops(sd, T, S)
    total_fl = sum(fl.values())
    clips = {B: torch.rand(B, T, 3, H, H, generator=torch.Generator().manual_seed(B)).to(DEV) for B in (16, 64)}
    eng = {}
    for B, v in clips.items():
        eng[B] = timed(lambda: det.features(v), a.repeats)
        say(f"B {B}: engine {eng[B][0] / B:.3f} [{eng[B][1] / B:.3f}, {eng[B][2] / B:.3f}] ms per clip = "
            f"{total_fl * B / (eng[B][0] * 1e-3) / 1e12:.1f} TFLOP/s over the convolutions ({total_fl * B / (eng[B][0] * 1e-3) / PEAK_F32_MFMA:.3f} of the f32 MFMA peak; "
            f"{total_fl / 1e9:.1f} GFLOP per clip)")
    # where the time goes: forwards of one chunk cut after a unit
    names = [u[0] for u in R.UNITS]
    cuts = [("front end", -1), ("Conv3d_1a_7x7", 0), ("MaxPool3d_2a .. MaxPool3d_3a", names.index("MaxPool3d_3a_3x3")),
            ("Mixed_3b, 3c, MaxPool3d_4a", names.index("MaxPool3d_4a_3x3")), ("Mixed_4b .. 4f, MaxPool3d_5a", names.index("MaxPool3d_5a_2x2")),
            ("Mixed_5b, 5c", len(names) - 1)]
    v = clips[16][:chunk]
    prev_ms, prev_u = 0.0, -2
    for label, u in cuts:
        ms = timed(lambda: det.tap(v, u), max(3, a.repeats // 2))[0]
        stage_fl = sum(f for i, f in fl.items() if prev_u < i <= u) * chunk
        rate = f", {stage_fl / ((ms - prev_ms) * 1e-3) / 1e12:.1f} TFLOP/s" if stage_fl and ms > prev_ms else ""
        say(f"    up to {label}: {ms / chunk:.3f} ms per clip, the stage {(ms - prev_ms) / chunk:.3f} ms ({stage_fl / chunk / 1e9:.1f} GFLOP per clip{rate})")
        prev_ms, prev_u = ms, u
    if not a.skip_torch:
        sd_dev = {k: t.to(DEV) for k, t in sd.items()}
        with torch.no_grad():
            run = lambda x: torch.cat([R.forward(sd_dev, x[lo:lo + chunk], S, torch.float32) for lo in range(0, x.shape[0], chunk)])
            for B, x in clips.items():
                base = timed(lambda: run(x), max(3, a.repeats // 2))
                dev = R.feature_deviation(det.features(x).cpu(), run(x).double().cpu())
                say(f"B {B}: torch fp32 restatement {base[0] / B:.3f} [{base[1] / B:.3f}, {base[2] / B:.3f}] ms per clip; engine / torch time "
                    f"{eng[B][0] / base[0]:.2f}; engine vs torch feature deviation {dev:.2e}")


if __name__ == "__main__":
    main()
