"""fp64 yardstick of the LPIPS tests: a torch restatement of the four steps (scale -> VGG-16 features[0:30] with five taps ->
per-pixel channel normalisation, lin-weighted squared difference, pixel mean, sum over the taps -> mean over frames, min over
samples), evaluated in a chosen dtype on the CPU, with seeded random weights (He-scaled normal convolutions, small normal biases,
non-negative lin weights) under the state-dict keys of the reference's LPIPS class.  No real weights are needed or committed."""
import torch
import torch.nn.functional as F

# (slice of the reference's wrapper, torchvision features index, Cin, Cout); a 2 x 2 max-pool precedes layers 3, 5, 8, 11 (1-based)
CONVS = ((1, 0, 3, 64), (1, 2, 64, 64), (2, 5, 64, 128), (2, 7, 128, 128), (3, 10, 128, 256), (3, 12, 256, 256), (3, 14, 256, 256),
         (4, 17, 256, 512), (4, 19, 512, 512), (4, 21, 512, 512), (5, 24, 512, 512), (5, 26, 512, 512), (5, 28, 512, 512))
POOL_BEFORE = (2, 4, 7, 10)      # 0-based layer indices whose input is pooled
TAP_AFTER = (1, 3, 6, 9, 12)     # 0-based layer indices whose ReLU output is a tap
TAP_C = (64, 128, 256, 512, 512)
SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)
U = 2.0 ** -24                   # unit roundoff of fp32


def random_state_dict(seed):
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for s, i, cin, cout in CONVS:
        sd[f"net.slice{s}.{i}.weight"] = (torch.randn(cout, cin, 3, 3, generator=g, dtype=torch.float64) * (2.0 / (9 * cin)) ** 0.5).float()
        sd[f"net.slice{s}.{i}.bias"] = (torch.randn(cout, generator=g, dtype=torch.float64) * 0.1).float()
    for k, c in enumerate(TAP_C):
        sd[f"lin{k}.model.1.weight"] = (torch.rand(1, c, 1, 1, generator=g, dtype=torch.float64) * 0.02).float()
    return sd


def torchvision_state_dicts(sd):
    """the same weights as the two files a user has: torchvision's vgg16 (``features.N.*``) and the lpips package's ``vgg.pth``"""
    vgg = {f"features.{i}.{kind}": sd[f"net.slice{s}.{i}.{kind}"] for s, i, _, _ in CONVS for kind in ("weight", "bias")}
    lin = {f"lin{k}.model.1.weight": sd[f"lin{k}.model.1.weight"] for k in range(5)}
    return vgg, lin


def scale_input(x, dt):
    sh = torch.tensor(SHIFT, dtype=dt).view(1, 3, 1, 1)
    sc = torch.tensor(SCALE, dtype=dt).view(1, 3, 1, 1)
    return ((x.to(dt) * 2 - 1) - sh) / sc


def layer_inputs(sd, x, dt=torch.float64):
    """x (n, 3, H, W) in [0, 1] -> list of 13 (conv input NCHW, before the conv; for layer 0 the SCALED image), list of 5 taps (NCHW)"""
    h = scale_input(x, dt)
    ins, taps = [], []
    for l, (s, i, _, _) in enumerate(CONVS):
        if l in POOL_BEFORE:
            h = F.max_pool2d(h, 2, 2)
        ins.append(h)
        h = F.relu(F.conv2d(h, sd[f"net.slice{s}.{i}.weight"].to(dt), sd[f"net.slice{s}.{i}.bias"].to(dt), padding=1))
        if l in TAP_AFTER:
            taps.append(h)
    return ins, taps


def head(f0, f1, lin, dt=torch.float64):
    """f0, f1 (n, C, h, w), lin (C) -> (n,)"""
    f0, f1 = f0.to(dt), f1.to(dt)
    n0 = f0 / (f0.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
    n1 = f1 / (f1.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
    return (((n0 - n1) ** 2) * lin.to(dt).view(1, -1, 1, 1)).sum(1).mean((1, 2))


def taps_of(sd, x, dt=torch.float64, chunk=16):
    """x (n, 3, H, W) -> the five taps (n, C_k, H >> k, W >> k) in dtype dt"""
    parts = [layer_inputs(sd, x[lo:lo + chunk], dt)[1] for lo in range(0, x.shape[0], chunk)]
    return [torch.cat([p[k] for p in parts]) for k in range(5)]


def lpips_from_taps(sd, t0, t1, dt=torch.float64):
    """taps of n0 and n1 = m * n0 images; image i of t1 pairs with image i % n0 of t0 -> (n1,)"""
    m = t1[0].shape[0] // t0[0].shape[0]
    v = 0
    for k in range(5):
        v = v + head(t0[k].repeat(m, 1, 1, 1), t1[k], sd[f"lin{k}.model.1.weight"].reshape(-1), dt)
    return v


def lpips_pairs(sd, x0, x1, dt=torch.float64):
    """x0, x1 (n, 3, H, W) in [0, 1] -> (n,) LPIPS per pair in dtype dt"""
    return lpips_from_taps(sd, taps_of(sd, x0, dt), taps_of(sd, x1, dt), dt)


def clip_lpips(sd, gt, pred, gt_t0=0, pr_t0=0, T=None, dt=torch.float64):
    """gt (B, Tg, 3, H, W), pred (t * B, Tp, 3, H, W) -> (frames (t * B, T), rows (B,)): mean over frames, min over the t samples
    (sample k of trajectory b at row k * B + b).  The features of a ground-truth frame are those of each of its t repeats, so
    they are computed once."""
    B, n = gt.shape[0], pred.shape[0]
    t = n // B
    T = T if T is not None else min(gt.shape[1] - gt_t0, pred.shape[1] - pr_t0)
    g = gt[:, gt_t0:gt_t0 + T].float().reshape(B * T, *gt.shape[2:])
    p = pred[:, pr_t0:pr_t0 + T].reshape(n * T, *pred.shape[2:])
    frames = lpips_from_taps(sd, taps_of(sd, g, dt), taps_of(sd, p, dt), dt).reshape(n, T)
    rows = frames.reshape(t, B, T).mean(-1).min(0).values
    return frames, rows


def conv_bound(x64, w, b):
    """gamma_n * (sum |x w| + |b|) per output element, n = 9 Cin + 2, u = 2^-24: the dot-product bound for any summation order
    plus the bias add and the final rounding.  x64 (n, Cin, H, W) fp64 (values representable in fp32), w fp32, b fp32."""
    n = 9 * w.shape[1] + 2
    gamma = n * U / (1 - n * U)
    mag = F.conv2d(x64.abs(), w.double().abs(), b.double().abs(), padding=1)
    return gamma * mag
