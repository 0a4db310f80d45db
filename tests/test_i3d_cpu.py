"""Host logic of FVD (no GPU): the SAME-pad rule, ``pack_i3d`` (batch-norm fold, K order, prefix stripping, missing keys),
``FeatureStats``, ``frechet_distance`` on both routes, and the ``use_fvd`` branch of ``train_gpt.evaluate`` with a stub detector."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import i3d_ref as R


def test_same_pad_gives_ceil_n_over_s():
    for k, s in R.KS_PAIRS:
        for n in range(1, 21):
            front, back = R.same_pad(n, k, s)
            assert front >= 0 and back >= front and back - front <= 1
            assert (n + front + back - k) // s + 1 == -(-n // s), (n, k, s)
            # the last window reaches the back pad's end exactly (or stays inside the tensor): no tap lies beyond the padding
            assert (-(-n // s) - 1) * s - front + k - 1 <= n - 1 + back


def test_pack_i3d_folds_batch_norm_and_orders_k():
    from ivideogpt_amd.packing import I3D_CONV_UNITS, pack_i3d
    sd = R.random_i3d_state_dict(3, width_div=8)
    packed = pack_i3d(sd)
    assert len(I3D_CONV_UNITS) == 57 and len(packed) == 2 * 57 + 2
    g = torch.Generator().manual_seed(0)
    for name, kind, k, s, _ in R.UNITS:
        if kind != "conv":
            continue
        w = sd[f"{name}.conv3d.weight"]
        cout, cin = w.shape[:2]
        pw, pb = packed[f"{name}.weight"], packed[f"{name}.bias"]
        assert pw.shape == (cout, k[0] * k[1] * k[2] * cin) and pw.dtype == torch.float32 and pw.is_contiguous() and pb.shape == (cout,)
        # folded convolution == convolution + unfolded eval-mode batch norm, in fp64, up to the fp32 rounding of the folded tensors
        x = torch.randn(1, cin, k[0] + 1, k[1] + 1, k[2] + 1, generator=g, dtype=torch.float64)
        ref = F.batch_norm(F.conv3d(x, w.double()), sd[f"{name}.bn.running_mean"].double(), sd[f"{name}.bn.running_var"].double(),
                           sd[f"{name}.bn.weight"].double(), sd[f"{name}.bn.bias"].double(), False, 0.0, 1e-3)
        wf = pw.double().reshape(cout, k[0], k[1], k[2], cin).permute(0, 4, 1, 2, 3)
        got = F.conv3d(x, wf, pb.double())
        mag = F.conv3d(x.abs(), wf.abs(), pb.double().abs())
        assert ((got - ref).abs() <= 2.0 ** -23 * mag).all(), name
    assert torch.equal(packed["logits.weight"], sd["logits.conv3d.weight"].reshape(400, -1))
    assert torch.equal(packed["logits.bias"], sd["logits.conv3d.bias"])
    w = sd["Conv3d_1a_7x7.conv3d.weight"].double()
    scale = sd["Conv3d_1a_7x7.bn.weight"].double() / torch.sqrt(sd["Conv3d_1a_7x7.bn.running_var"].double() + 1e-3)
    assert packed["Conv3d_1a_7x7.weight"][5, ((2 * 7 + 4) * 7 + 6) * 3 + 1] == (w[5, 1, 2, 4, 6] * scale[5]).float()   # K = (kd, kh, kw, c)


def test_pack_i3d_strips_a_prefix_and_lists_missing_keys():
    from ivideogpt_amd.packing import pack_i3d
    sd = R.random_i3d_state_dict(4, width_div=8)
    plain = pack_i3d(sd)
    pre = pack_i3d({"model.i3d." + k: v for k, v in sd.items()})
    assert plain.keys() == pre.keys() and all(torch.equal(plain[k], pre[k]) for k in plain)
    bad = {"model." + k: v for k, v in sd.items() if k not in ("Mixed_4c.b1b.bn.running_var", "logits.conv3d.bias")}
    with pytest.raises(KeyError) as e:
        pack_i3d(bad)
    assert "Mixed_4c.b1b.bn.running_var" in str(e.value) and "logits.conv3d.bias" in str(e.value) and "2 tensors" in str(e.value)


def test_random_state_dict_widths():
    from ivideogpt_amd.weights import i3d_param_shapes
    full = i3d_param_shapes(1)
    assert full["Conv3d_1a_7x7.conv3d.weight"] == (64, 3, 7, 7, 7) and full["Mixed_3b.b0.conv3d.weight"] == (64, 192, 1, 1, 1)
    assert full["Mixed_4b.b0.conv3d.weight"][1] == 480 and full["Mixed_5b.b0.conv3d.weight"][1] == 832
    assert full["Mixed_4f.b1b.conv3d.weight"] == (320, 160, 3, 3, 3) and full["logits.conv3d.weight"] == (400, 1024, 1, 1, 1)
    assert i3d_param_shapes(4)["logits.conv3d.weight"] == (400, 256, 1, 1, 1) and i3d_param_shapes(8)["Mixed_3b.b2a.conv3d.weight"][0] == 2
    sd = R.random_i3d_state_dict(0, 8)
    var = sd["Mixed_3c.b1b.bn.running_var"]
    assert var.min() >= 0.5 and var.max() <= 1.5


def test_reference_forward_runs_in_both_precisions():
    sd = R.random_i3d_state_dict(5, width_div=8)
    v = torch.rand(2, 9, 3, 20, 24, generator=torch.Generator().manual_seed(1))
    f64, taps = R.forward(sd, v, 32, torch.float64, taps=True)
    f32 = R.forward(sd, v, 32, torch.float32)
    assert f64.shape == (2, 400) and f64.dtype == torch.float64 and len(taps) == len(R.UNITS) + 1 == 71
    assert taps[-1].shape == (2, 3, 9, 32, 32) and taps[0].shape[2:] == (5, 16, 16) and taps[len(R.UNITS) - 1].shape[2:] == (2, 1, 1)
    assert R.feature_deviation(f32, f64) < 1e-5


def test_c_abi_plans_the_forward_the_reference_runs():
    """Everything here happens before a launch, so host tensors and no device do: the unit table built from the weight shapes, the
    shape of every tap and the units it reads against the restatement, the scratch size, and the refusals."""
    import ctypes as C
    from ivideogpt_amd import _lib
    from ivideogpt_amd.packing import pack_i3d
    lb = _lib.load()
    sd = R.random_i3d_state_dict(6, width_div=8)
    packed = pack_i3d(sd)

    def create(tensors, resize=64):
        names = [k.encode() for k in tensors]
        table = (_lib.IvgTensor * len(names))()
        for i, (k, v) in enumerate(tensors.items()):
            table[i].name, table[i].data, table[i].dtype, table[i].ndim = names[i], v.data_ptr(), _lib.IVG_F32, v.dim()
            for d, s in enumerate(v.shape):
                table[i].shape[d] = s
        h = C.c_void_p()
        return lb.ivg_i3d_create(table, len(names), 0, resize, C.byref(h)), h

    rc, h = create(packed)
    assert rc == 0 and lb.ivg_i3d_units(h) == len(R.UNITS) == 70
    _, taps = R.forward(sd, torch.rand(1, 12, 3, 16, 16), 64, torch.float32, taps=True)
    dims = (C.c_int64 * 8)()
    for u in range(-1, len(R.UNITS)):
        assert lb.ivg_op_i3d_tap(h, None, 0, 1, 12, 16, 16, u, None, dims, None, 0, None) == 0
        c, d, hh, ww = taps[u].shape[1:]
        assert list(dims[:4]) == [d, hh, ww, c], (u, list(dims))
        assert [s for s in dims[4:8] if s != -2] == ([] if u < 0 else R.UNITS[u][4]), (u, list(dims))
    assert lb.ivg_op_i3d_tap(h, None, 0, 1, 12, 16, 16, 70, None, dims, None, 0, None) == -1
    one, four = lb.ivg_i3d_ws_bytes(h, 1, 12, 16, 16), lb.ivg_i3d_ws_bytes(h, 4, 12, 16, 16)
    assert one > 12 * 64 * 64 * 3 * 4 and four == 4 * (one - 256) + 256
    assert lb.ivg_i3d_ws_bytes(h, 1, 8, 16, 16) == 0 and lb.ivg_i3d_ws_bytes(h, 1, 9, 16, 16) > 0      # two time steps in front of the average pool
    out = torch.full((1, 400), 7.5)
    x = torch.rand(1, 12, 3, 16, 16)
    ws = torch.empty(one, dtype=torch.uint8)
    P = lambda t: C.c_void_p(t.data_ptr())
    assert lb.ivg_i3d_features(h, P(x), 0, 1, 8, 16, 16, P(out), P(ws), one, None) == -1               # T too short
    assert lb.ivg_i3d_features(None, P(x), 0, 1, 12, 16, 16, P(out), P(ws), one, None) == -1           # null handle
    assert lb.ivg_i3d_features(h, P(x), 0, 1, 12, 16, 16, P(out), P(ws), one - 1, None) == -4          # a short scratch
    assert lb.ivg_i3d_features(h, P(x), 3, 1, 12, 16, 16, P(out), P(ws), one, None) == -1              # no such dtype
    assert (out == 7.5).all()
    lb.ivg_i3d_destroy(h)
    rc, h48 = create(packed, resize=48)                                                               # S not a multiple of 32
    assert rc == 0 and lb.ivg_i3d_ws_bytes(h48, 1, 12, 16, 16) == 0
    assert lb.ivg_i3d_features(h48, P(x), 0, 1, 12, 16, 16, P(out), P(ws), one, None) == -1 and (out == 7.5).all()
    lb.ivg_i3d_destroy(h48)
    # a missing tensor and one whose shape does not fit its place are named
    less = {k: v for k, v in packed.items() if k != "Mixed_4d.b2a.bias"}
    rc, _ = create(less)
    assert rc == -2 and "Mixed_4d.b2a.bias" in _lib.last_error()
    bad = dict(packed)
    bad["Mixed_5b.b1b.weight"] = packed["Mixed_5b.b1b.weight"][:, :-1].contiguous()
    rc, _ = create(bad)
    assert rc == -1 and "Mixed_5b.b1b.weight" in _lib.last_error() and "columns" in _lib.last_error()


def test_feature_stats_against_numpy_cov():
    from ivideogpt_amd.metrics import FeatureStats
    rng = np.random.default_rng(0)
    x = rng.normal(size=(37, 12)).astype(np.float32) * 3 + 1
    s = FeatureStats(capture_mean_cov=True)
    s.append(x[:10]); s.append_torch(torch.from_numpy(x[10:30])); s.append(x[30:])
    mean, cov = s.get_mean_cov()
    assert s.num_items == 37
    np.testing.assert_allclose(mean, x.astype(np.float64).mean(0), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(cov, np.cov(x.astype(np.float64), rowvar=False, bias=True), rtol=1e-10, atol=1e-10)


def test_frechet_distance_closed_form_for_diagonal_covariances():
    from ivideogpt_amd.metrics import frechet_distance
    rng = np.random.default_rng(1)
    a, b = rng.uniform(0.1, 2.0, 16), rng.uniform(0.1, 2.0, 16)
    mu_a, mu_b = rng.normal(size=16), rng.normal(size=16)
    want = np.square(mu_a - mu_b).sum() + np.square(np.sqrt(a) - np.sqrt(b)).sum()
    for method in ("scipy", "eig", None):
        assert abs(frechet_distance(mu_a, np.diag(a), mu_b, np.diag(b), method=method) - want) <= 1e-10 * want


def test_frechet_distance_routes_agree_on_singular_covariances():
    """N < d samples: both covariances are singular, as with fewer than 400 clips"""
    from ivideogpt_amd.metrics import FeatureStats, frechet_distance
    rng = np.random.default_rng(2)
    stats = []
    for shift in (0.0, 0.5):
        s = FeatureStats()
        s.append((rng.normal(size=(24, 40)) + shift).astype(np.float32))
        stats.append(s.get_mean_cov())
    (mu_r, sig_r), (mu_g, sig_g) = stats
    a = frechet_distance(mu_g, sig_g, mu_r, sig_r, method="scipy")
    b = frechet_distance(mu_g, sig_g, mu_r, sig_r, method="eig")
    assert math.isfinite(a) and a > 0 and abs(a - b) <= 1e-8 * abs(a), (a, b)


def test_frechet_distance_of_identical_statistics_is_zero():
    from ivideogpt_amd.metrics import FeatureStats, frechet_distance
    rng = np.random.default_rng(3)
    for n in (24, 200):   # singular and full-rank
        s = FeatureStats()
        s.append(rng.normal(size=(n, 40)).astype(np.float32))
        mu, sig = s.get_mean_cov()
        for method in ("scipy", "eig"):
            assert abs(frechet_distance(mu, sig, mu, sig, method=method)) <= 1e-6 * np.trace(sig), (n, method)


class StubDetector:
    """stands where an ``I3D`` goes: (B, T, 3, H, W) -> (B, 6) features, and a log of the chunks it saw"""

    def __init__(self):
        self.calls = []

    def features(self, video, max_clips=None):
        self.calls.append(video.shape[0])
        v = video.float()
        return torch.stack([v.mean((1, 2, 3, 4)), v[:, -1].mean((1, 2, 3)), v[:, :, 0].mean((1, 2, 3)), v.amax((1, 2, 3, 4)),
                            v[:, :, :, ::2].mean((1, 2, 3, 4)), v.std((1, 2, 3, 4))], 1)


def _standins():
    from eval_standins import OracleEvaluator, OracleLM
    from helpers import oracle_llama, oracle_tokenizer
    from ivideogpt_amd import weights as W
    tcfg = W.tokenizer_config(block_out_channels=(32, 32, 64), layers_per_block=1, latent_channels=64, num_vq_embeddings=256,
                              num_dyn_embeddings=256, norm_num_groups=32, mid_block_add_attention=False, context_length=2, resolution=64,
                              max_att_resolution=16)
    lcfg = dict(hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=1, num_key_value_heads=1, rms_norm_eps=1e-6,
                rope_theta=10000.0, max_position_embeddings=1024, vocab_size=514)
    tok = oracle_tokenizer(tcfg, W.random_tokenizer_state_dict(tcfg, 5, codebook_std=0.5), 2)
    gen = torch.Generator().manual_seed(11)
    model = OracleLM(oracle_llama(lcfg, W.random_llama_state_dict(lcfg, 6)), lambda B, n: torch.rand(B, n, generator=gen))
    g = torch.Generator().manual_seed(7)
    batches = [torch.rand(2, 4, 3, 64, 64, generator=g) for _ in range(2)]
    return tok, model, batches, OracleEvaluator


def test_evaluate_logs_fvd_with_a_stub_detector_and_raises_without():
    import train_gpt
    from ivideogpt_amd.metrics import Evaluator, FeatureStats
    from ivideogpt_amd.parallel import LocalAccelerator
    tok, model, batches, OracleEvaluator = _standins()

    class CpuEvaluator(Evaluator):   # the frame metrics of the CPU stand-in, the FVD half of the product
        def __call__(self, video_1, video_2):
            return OracleEvaluator()(video_1, video_2)

    det = StubDetector()
    args = train_gpt.eval_args(context_length=2, segment_length=4, eval_generate_times=2, max_generate_batchsize=4, max_decode_batchsize=3,
                               max_eval_iters=100, log_gif_interval=1000, use_fvd=True)
    logs = train_gpt.evaluate(args, LocalAccelerator("cpu"), tok, model, batches, CpuEvaluator(i3d=det), 0)
    assert math.isfinite(logs["eval/fvd"]) and logs["eval/fvd"] > 0
    # per batch: the 2 real clips in one call, the t * B = 4 generated ones in chunks of max_decode_batchsize
    assert det.calls == [2, 3, 1, 2, 3, 1]
    assert {"eval/eval_loss", "eval/mse", "eval/psnr", "eval/ssim", "eval/lpips"} <= set(logs)

    ev = CpuEvaluator()
    assert ev.i3d is None
    with pytest.raises(NotImplementedError):
        train_gpt.evaluate(args, LocalAccelerator("cpu"), tok, model, batches, ev, 0)
    with pytest.raises(RuntimeError):
        ev.i3d_features(batches[0])
    with pytest.raises(RuntimeError):
        ev.compute_fvd_from_raw_data(torch.stack(batches), torch.stack(batches))
    with pytest.raises(RuntimeError):
        ev.compute_fvd(FeatureStats(), FeatureStats())
    with pytest.raises(ValueError):
        CpuEvaluator(i3d=det).compute_fvd(FeatureStats(), FeatureStats())   # "No data to compute FVD", as the reference
    assert Evaluator(i3d_path="pretrained_models/i3d/i3d_torchscript.pt").i3d is None   # the reference's default path: no such file, no FVD


def test_compute_fvd_from_raw_data_equals_frechet_distance_of_the_features():
    from ivideogpt_amd.metrics import Evaluator, FeatureStats, frechet_distance
    det = StubDetector()
    g = torch.Generator().manual_seed(3)
    real, gen = torch.rand(3, 4, 9, 3, 8, 8, generator=g), torch.rand(3, 4, 9, 3, 8, 8, generator=g) * 0.8
    got = Evaluator(i3d=det).compute_fvd_from_raw_data(real, gen)
    stats = []
    for d in (real, gen):
        s = FeatureStats()
        s.append_torch(det.features(d.reshape(12, 9, 3, 8, 8)))
        stats.append(s.get_mean_cov())
    want = frechet_distance(stats[1][0], stats[1][1], stats[0][0], stats[0][1])
    assert abs(got - want) <= 1e-9 * abs(want) and det.calls[:6] == [4] * 6
