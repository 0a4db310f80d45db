"""The yardstick of the I3D tests: a torch restatement of the Kinetics-400 Inception-I3D detector as the FVD evaluator calls it
(rescale, resize, return_features), written with library ops only -- ``F.pad`` for the TensorFlow SAME pads, unfolded eval-mode
``F.batch_norm`` (eps 1e-3), ``F.max_pool3d``, ``F.avg_pool3d``, bilinear ``F.interpolate`` -- and run in fp64 (the reference value)
or fp32 (the deviation an fp32 evaluation shows on its own).  It also holds the case tables and the bounds of tests/test_gpu_i3d.py.

Units are numbered in execution order, pools included; a Mixed block is b0, b1a, b1b, b2a, b2b, b3a (the pool), b3b and its output
cat(b0, b1b, b2b, b3b).  Unit -1 is the front end's output."""
import math

import torch
import torch.nn.functional as F

from ivideogpt_amd.weights import random_i3d_state_dict  # noqa: F401  (seeded weights only; the architecture is restated below)

BN_EPS = 1e-3
U = 2.0 ** -24

ARCH = (("Conv3d_1a_7x7", "conv", (7, 7, 7), (2, 2, 2)), ("MaxPool3d_2a_3x3", "pool", (1, 3, 3), (1, 2, 2)),
        ("Conv3d_2b_1x1", "conv", (1, 1, 1), (1, 1, 1)), ("Conv3d_2c_3x3", "conv", (3, 3, 3), (1, 1, 1)),
        ("MaxPool3d_3a_3x3", "pool", (1, 3, 3), (1, 2, 2)), ("Mixed_3b", "mixed"), ("Mixed_3c", "mixed"),
        ("MaxPool3d_4a_3x3", "pool", (3, 3, 3), (2, 2, 2)), ("Mixed_4b", "mixed"), ("Mixed_4c", "mixed"), ("Mixed_4d", "mixed"),
        ("Mixed_4e", "mixed"), ("Mixed_4f", "mixed"), ("MaxPool3d_5a_2x2", "pool", (2, 2, 2), (2, 2, 2)), ("Mixed_5b", "mixed"),
        ("Mixed_5c", "mixed"))
MIXED = (("b0", "conv", (1, 1, 1)), ("b1a", "conv", (1, 1, 1)), ("b1b", "conv", (3, 3, 3)), ("b2a", "conv", (1, 1, 1)),
         ("b2b", "conv", (3, 3, 3)), ("b3a", "pool", (3, 3, 3)), ("b3b", "conv", (1, 1, 1)))
# every (kernel, stride) pair per axis that occurs in the table
KS_PAIRS = ((7, 2), (1, 1), (3, 2), (3, 1), (2, 2))
POOL_SHAPES = (((1, 3, 3), (1, 2, 2)), ((3, 3, 3), (2, 2, 2)), ((2, 2, 2), (2, 2, 2)), ((3, 3, 3), (1, 1, 1)))


def units():
    """[(name, kind, kernel, stride, sources)] in execution order; sources = the units whose concatenated outputs the unit reads"""
    out, src = [], [-1]
    for row in ARCH:
        if row[1] != "mixed":
            out.append((row[0], row[1], row[2], row[3], list(src)))
            src = [len(out) - 1]
            continue
        u = len(out)
        for j, (b, kind, k) in enumerate(MIXED):
            out.append((f"{row[0]}.{b}", kind, k, (1, 1, 1), [u + j - 1] if b in ("b1b", "b2b", "b3b") else list(src)))
        src = [u, u + 2, u + 4, u + 6]
    return out


UNITS = units()


def same_pad(n, k, s):
    """TensorFlow SAME: (front, back) zeros for extent n, kernel k, stride s"""
    pad = max(k - s, 0) if n % s == 0 else max(k - n % s, 0)
    return pad // 2, pad - pad // 2


def pad_same(x, k, s):
    """x (B, C, D, H, W) zero-padded for kernel k, stride s (per axis)"""
    p = [same_pad(x.shape[2 + i], k[i], s[i]) for i in range(3)]
    return F.pad(x, (p[2][0], p[2][1], p[1][0], p[1][1], p[0][0], p[0][1]))


def max_pool(x, k, s):
    return F.max_pool3d(pad_same(x, k, s), k, s)


def unit3d(sd, name, x, k, s):
    dt = x.dtype
    y = F.conv3d(pad_same(x, k, s), sd[f"{name}.conv3d.weight"].to(dt), None, s)
    y = F.batch_norm(y, sd[f"{name}.bn.running_mean"].to(dt), sd[f"{name}.bn.running_var"].to(dt), sd[f"{name}.bn.weight"].to(dt),
                     sd[f"{name}.bn.bias"].to(dt), False, 0.0, BN_EPS)
    return F.relu(y)


def front_end(video, S, dtype=torch.float64):
    """(B, T, 3, H, W) in [0, 1] -> (B, 3, T, S, S): per frame bilinear resize (align_corners False, no antialias), 2 x - 1"""
    B, T, C, H, W = video.shape
    x = F.interpolate(video.to(dtype).reshape(B * T, C, H, W), size=(S, S), mode="bilinear", align_corners=False)
    return (2 * x - 1).reshape(B, T, C, S, S).permute(0, 2, 1, 3, 4).contiguous()


def head(sd, x):
    """(B, C, D, S/32, S/32) -> (B, 400)"""
    dt = x.dtype
    a = F.avg_pool3d(x, (2, x.shape[3], x.shape[4]), stride=1)
    y = F.conv3d(a, sd["logits.conv3d.weight"].to(dt), sd["logits.conv3d.bias"].to(dt))
    return y.mean(dim=(2, 3, 4))


def forward(sd, video, S, dtype=torch.float64, taps=False):
    """-> features (B, 400) [, {unit: activation (B, C, D, H, W)}]"""
    x = front_end(video, S, dtype)
    outs = {-1: x}
    n = len(UNITS)
    final = (n - 7, n - 5, n - 3, n - 1)   # the last block's b0, b1b, b2b, b3b
    for i, (name, kind, k, s, src) in enumerate(UNITS):
        xin = outs[src[0]] if len(src) == 1 else torch.cat([outs[j] for j in src], 1)
        outs[i] = unit3d(sd, name, xin, k, s) if kind == "conv" else max_pool(xin, k, s)
        if not taps:   # keep only what later units read
            live = {j for (_, _, _, _, sr) in UNITS[i + 1:] for j in sr} | set(final)
            outs = {j: v for j, v in outs.items() if j in live}
    f = head(sd, torch.cat([outs[j] for j in final], 1))
    return (f, outs) if taps else f


def cl(x):
    """(B, C, D, H, W) -> channels-last (B, D, H, W, C)"""
    return x.permute(0, 2, 3, 4, 1).contiguous()


def cf(x):
    """channels-last (B, D, H, W, C) -> (B, C, D, H, W)"""
    return x.permute(0, 4, 1, 2, 3).contiguous()


def gamma(n):
    return n * U / (1 - n * U)


def conv_oracle(x_cl32, w_packed, bias, k, s, relu=True):
    """The fp64 value of a packed convolution on fp32 data and its dot-product bound.  x_cl32 (B, D, H, W, Cin) fp32, w_packed
    (Cout, kd kh kw Cin) fp32 with K ordered (kd, kh, kw, c), bias (Cout,) -> (y64, bound) channels-last (B, Do, Ho, Wo, Cout):
    |y - y64| <= gamma_(K + 2) (sum |x w| + |b|) for any summation order (K products and sums, bias add, final rounding); ReLU
    does not increase the error."""
    cin = x_cl32.shape[-1]
    w = w_packed.double().reshape(w_packed.shape[0], k[0], k[1], k[2], cin).permute(0, 4, 1, 2, 3).contiguous()
    x = pad_same(cf(x_cl32.double()), k, s)
    y = F.conv3d(x, w, bias.double(), s)
    mag = F.conv3d(x.abs(), w.abs(), bias.double().abs(), s)
    if relu:
        y = F.relu(y)
    return cl(y), cl(gamma(w_packed.shape[1] + 2) * mag)


# op-level convolution cases of the issue: (kernel, stride, Cin, Cout, (D, H, W), relu)
CONV_CASES = (((7, 7, 7), (2, 2, 2), 3, 64, (9, 18, 18), True),      # odd depth, asymmetric pads
              ((1, 1, 1), (1, 1, 1), 192, 64, (2, 5, 7), True),      # M not a tile multiple
              ((3, 3, 3), (1, 1, 1), 6, 10, (4, 6, 6), True),        # widths no tile divides
              ((3, 3, 3), (1, 1, 1), 192, 384, (2, 3, 3), True),     # K = 5184
              ((1, 1, 1), (1, 1, 1), 832, 384, (2, 2, 2), True),
              ((1, 1, 1), (1, 1, 1), 1024, 400, (1, 1, 1), False),   # the logits shape: bias, no ReLU
              ((7, 7, 7), (2, 2, 2), 3, 16, (8, 16, 16), True),      # stride 2, even sizes
              ((3, 3, 3), (2, 2, 2), 8, 12, (6, 8, 10), True))       # stride 2, even sizes, vector loads


def feature_deviation(f, f64):
    """max over clips of max |f - f64| / max |f64|"""
    return ((f.double() - f64).abs().amax(1) / f64.abs().amax(1)).max().item()
