"""Host logic of the LPIPS metric (no GPU): state-dict key mapping, packing round trip, argument refusal through the C ABI (every
refusal happens before a launch, so a null device works), and the unchanged default of ``Evaluator()``."""
import ctypes as C

import pytest
import torch

import lpips_ref as R


def test_key_map_accepts_reference_and_torchvision_names():
    from ivideogpt_amd.packing import lpips_key_map
    sd = R.random_state_dict(1)
    km = lpips_key_map(sd.keys())
    assert len(km) == 31 and all(k == v for k, v in km.items())
    vgg, lin = R.torchvision_state_dicts(sd)
    km2 = lpips_key_map({**vgg, **lin}.keys())
    assert set(km2) == set(km) and km2["net.slice3.12.bias"] == "features.12.bias" and km2["lin4.model.1.weight"] == "lin4.model.1.weight"
    del vgg["features.21.weight"]
    with pytest.raises(KeyError, match="net.slice4.21.weight"):
        lpips_key_map({**vgg, **lin}.keys())


def test_packing_round_trip_and_shape_check():
    from ivideogpt_amd.packing import pack_lpips, unpack_lpips_conv
    sd = R.random_state_dict(2)
    packed = pack_lpips(sd)
    for s, i, cin, cout in R.CONVS:
        w = packed[f"net.slice{s}.{i}.weight"]
        assert w.shape == (cout, 9 * cin) and w.dtype == torch.float32 and w.is_contiguous()
        assert w[5, (1 * 3 + 2) * cin + (cin - 1)] == sd[f"net.slice{s}.{i}.weight"][5, cin - 1, 1, 2]      # K ordered (kh, kw, c)
        assert torch.equal(unpack_lpips_conv(w, cin), sd[f"net.slice{s}.{i}.weight"])
        assert torch.equal(packed[f"net.slice{s}.{i}.bias"], sd[f"net.slice{s}.{i}.bias"])
    for k, c in enumerate(R.TAP_C):
        assert torch.equal(packed[f"lin{k}.model.1.weight"], sd[f"lin{k}.model.1.weight"].reshape(c))
    vgg, lin = R.torchvision_state_dicts(sd)
    p2 = pack_lpips({**vgg, **lin})
    assert all(torch.equal(p2[k], packed[k]) for k in packed)
    bad = dict(sd)
    bad["net.slice2.5.weight"] = torch.zeros(128, 64, 1, 1)
    with pytest.raises(ValueError):
        pack_lpips(bad)


def _table(packed, drop=None, resize=None):
    from ivideogpt_amd import _lib
    keep = {k: v for k, v in packed.items() if k != drop}
    if resize:
        keep[resize] = keep[resize][:-1].contiguous()
    names = [k.encode() for k in keep]
    tab = (_lib.IvgTensor * len(names))()
    for i, (k, v) in enumerate(keep.items()):
        tab[i].name, tab[i].data, tab[i].dtype, tab[i].ndim = names[i], v.data_ptr(), 0, v.dim()
        for d, s in enumerate(v.shape):
            tab[i].shape[d] = s
    return tab, len(names), (names, keep)


def test_abi_refusals_before_any_launch():
    """host tensors stand in for device pointers: every call below must return before touching them"""
    from ivideogpt_amd import _lib
    from ivideogpt_amd.packing import pack_lpips
    l = _lib.load()
    packed = pack_lpips(R.random_state_dict(3))
    h = C.c_void_p()
    tab, n, keep = _table(packed, drop="net.slice4.19.bias")
    assert l.ivg_lpips_create(tab, n, 0, C.byref(h)) == -2 and not h.value and "net.slice4.19.bias" in _lib.last_error()
    tab, n, keep = _table(packed, resize="lin2.model.1.weight")
    assert l.ivg_lpips_create(tab, n, 0, C.byref(h)) == -1 and not h.value and "lin2.model.1.weight" in _lib.last_error()
    tab, n, keep = _table(packed)
    assert l.ivg_lpips_create(tab, n, 0, C.byref(h)) == 0 and h.value
    try:
        B, T, t = 2, 3, 2
        gt, pred = torch.zeros(B, T, 3, 32, 32), torch.zeros(t * B, T, 3, 32, 32)
        rows = torch.full((B,), 7.0)
        ws = torch.zeros(1 << 20, dtype=torch.uint8)
        P = lambda x: C.c_void_p(x.data_ptr())

        def call(H=32, W=32, n_samples=t * B, ws_bytes=ws.numel(), gt_t0=0, dtype=0):
            return l.ivg_lpips_rows(h, P(gt), dtype, B, T, gt_t0, P(pred), n_samples, T, 0, T, H, W, None, P(rows), P(ws), ws_bytes, None)
        assert call(H=24) == -1 and call(W=8) == -1 and call(H=0) == -1
        assert call(n_samples=3) == -1 and call(gt_t0=1) == -1 and call(dtype=2) == -1
        assert l.ivg_lpips_ws_bytes(2, 32, 32) > ws.numel()
        assert call() == -4                                       # 1 MiB does not hold two 32 x 32 images
        assert call(ws_bytes=64) == -4
        assert torch.equal(rows, torch.full((B,), 7.0))
        assert l.ivg_lpips_ws_bytes(0, 32, 32) == 0 and l.ivg_lpips_ws_bytes(4, 64, 64) > 4 * 202 * 4096 * 4
        taps = (C.c_void_p * 5)()
        assert l.ivg_op_lpips_features(h, P(gt), 0, 2, 24, 32, taps, P(ws), ws.numel(), None) == -1
        assert l.ivg_op_lpips_features(h, P(gt), 0, 2, 32, 32, taps, P(ws), 1000, None) == -4
        f = torch.zeros(64)
        assert l.ivg_op_lpips_head(P(f), P(f), P(f), 1, 1, 1, 96, P(rows), P(ws), 1024, None) == -1
        assert l.ivg_op_lpips_head(P(f), P(f), P(f), 1, 4, 1, 64, P(rows), P(ws), 8, None) == -4
        assert l.ivg_op_maxpool2(P(f), P(f), 1, 3, 4, 4, None) == -1
    finally:
        l.ivg_lpips_destroy(h)
    assert l.ivg_debug_counter(b"lpips_trunk_images") == 0


def test_evaluator_default_is_unchanged():
    from ivideogpt_amd.metrics import Evaluator
    ev = Evaluator()
    assert ev.lpips is None and Evaluator(None, 8).max_batchsize == 8
    with pytest.raises(RuntimeError):
        ev.rows4(torch.zeros(1), torch.zeros(1))


def test_oracle_restatement_closed_forms():
    sd = R.random_state_dict(4)
    g = torch.Generator().manual_seed(5)
    x = torch.rand(2, 3, 16, 16, generator=g)
    assert torch.equal(R.lpips_pairs(sd, x, x), torch.zeros(2, dtype=torch.float64))
    gt = torch.rand(2, 2, 3, 16, 16, generator=g)
    pred = torch.rand(4, 2, 3, 16, 16, generator=g)
    frames, rows = R.clip_lpips(sd, gt, pred)
    assert frames.shape == (4, 2) and torch.allclose(rows, torch.minimum(frames[:2].mean(1), frames[2:].mean(1)))
    z = torch.zeros(1, 64, 2, 2, dtype=torch.float64)
    assert R.head(z, z, torch.ones(64)).item() == 0.0
