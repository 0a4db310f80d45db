"""Per-layer, per-head scales of the FP8 K / V cache on the CPU: the calibration's scale rule (tests/kv_scales_ref.py) against brute
force, and the argument checks of set_kv_cache_dtype(scales=...) on a model object that has no weights, no device and no engine."""
import ctypes as C

import numpy as np
import pytest
import torch

import decode_attn8_ref as R8
import kv_scales_ref as KS


def small_cfg(heads=2, hidden=128):
    from ivideogpt_amd import weights as W
    return dict(W.LLAMA_SMALL, hidden_size=hidden, intermediate_size=256, num_hidden_layers=2, num_attention_heads=heads,
                num_key_value_heads=heads)


def bf16_magnitudes(lo_exp=-20, hi_exp=20):
    """every positive bf16 value in [2^lo_exp, 2^hi_exp]"""
    bits = np.arange((127 + lo_exp) << 7, ((127 + hi_exp) << 7) + 1, dtype=np.uint32)
    return (bits << 16).view(np.float32)


@pytest.mark.parametrize("headroom", [0, 1, 3, 8])
def test_scale_rule_equals_brute_force_on_every_bf16_magnitude(headroom):
    """every bf16 magnitude in [2^-20, 2^20] and the edges 447, 448, 449, 0, the smallest normal and 2^126: the rule's scale s is a power
    of two decode_attn8_ref.scale_ok accepts, equals the brute-force search, and -- where the clamp to [2^-126, 2^126] is not active --
    amax / s <= 448 * 2^-h while amax / (s / 2) > 448 * 2^-h."""
    vals = np.concatenate([bf16_magnitudes(), np.array([447.0, 448.0, 449.0, 0.0, 2.0 ** -126, 2.0 ** 126], dtype=np.float32)])
    assert vals.size == 40 * 128 + 1 + 6
    got = KS.scale_from_amax(vals, headroom)
    lim = KS.E4M3_MAX * 2.0 ** -headroom
    for a, s in zip(vals.tolist(), got.tolist()):
        assert R8.scale_ok(s), (a, s)
        assert s == KS.brute_force_scale(a, headroom) == KS.scale_from_amax(a, headroom), (a, s)
        if a == 0.0:
            assert s == 1.0
            continue
        if 2.0 ** -126 < s < 2.0 ** 126:
            assert a / s <= lim and a / (s / 2) > lim, (a, s)
        elif s == 2.0 ** -126:
            assert a / s <= lim, (a, s)      # (clamped from below: more headroom than asked for)
    assert KS.scale_from_amax(448.0) == 1.0 and KS.scale_from_amax(447.0) == 1.0 and KS.scale_from_amax(449.0) == 2.0
    assert KS.scale_from_amax(448.0, 1) == 2.0 and KS.scale_from_amax(0.0, 5) == 1.0
    for bad in (float("nan"), float("inf"), -1.0):
        with pytest.raises(ValueError):
            KS.scale_from_amax(bad)


def good_table(layers=2, heads=2):
    return [[[2.0 ** -3, 2.0 ** 5][:heads], [2.0 ** 2, 2.0 ** -7][:heads]] for _ in range(layers)]


def test_scales_argument_is_checked_before_any_engine_work():
    """set_kv_cache_dtype(scales=...) on a CPU model object: a wrong shape, an entry that is no power of two, scales together with
    k_scale / v_scale, or a model the FP8 cache is not for raise ValueError and leave the model as it was; a good table is kept (with
    either format name), read back by kv_scales, dropped by a later call without scales, and carried by the wrapper and by replica()."""
    from ivideogpt_amd import HeadModelWithAction, LlamaForCausalLM
    m = LlamaForCausalLM(small_cfg(), None, dtype="bf16")
    assert torch.equal(m.kv_scales, torch.ones(2, 2, 2))
    for bad in ([[1.0, 1.0], [1.0, 1.0]], torch.ones(2, 2, 3), torch.ones(3, 2, 2), torch.ones(2, 2), 1.0, "x"):
        with pytest.raises(ValueError, match="shape"):
            m.set_kv_cache_dtype("fp8_e4m3", scales=bad)
    for entry in (3.0, 0.0, -1.0, float("nan"), float("inf"), 0.3, 2.0 ** 127, 2.0 ** -140):
        t = torch.tensor(good_table())
        t[1, 0, 1] = entry
        with pytest.raises(ValueError, match="power of two"):
            m.set_kv_cache_dtype("fp8_e4m3", scales=t)
    for kw in (dict(k_scale=0.5), dict(v_scale=2.0)):
        with pytest.raises(ValueError, match="not both"):
            m.set_kv_cache_dtype("fp8_e4m3", scales=good_table(), **kw)
    for dtype, heads in (("fp32", 2), ("x3", 2), ("bf16", 4)):
        with pytest.raises(ValueError, match="bf16 model with head_dim 64"):
            LlamaForCausalLM(small_cfg(heads), None, dtype=dtype).set_kv_cache_dtype("auto", scales=torch.ones(2, 2, heads))
    assert m._kv == ("auto", 1.0, 1.0), "a refused setting must leave the model as it was"
    with pytest.raises(AttributeError):
        m.kv_scales = torch.ones(2, 2, 2)
    for bad in (-1, 9, 1.5, None):
        with pytest.raises(ValueError, match="headroom"):
            m.calibrate_kv_cache(torch.zeros(1, 4, dtype=torch.int64), headroom=bad)
    with pytest.raises(ValueError, match="bf16 model with head_dim 64"):
        LlamaForCausalLM(small_cfg(), None, dtype="fp32").calibrate_kv_cache(torch.zeros(1, 4, dtype=torch.int64))
    w = HeadModelWithAction(m, 4, 513, 16, 2, 4)
    assert w.set_kv_cache_dtype("fp8_e4m3", scales=good_table()) is w
    assert m._kv[:3] == ("fp8_e4m3", 1.0, 1.0) and torch.equal(m.kv_scales, torch.tensor(good_table())) and torch.equal(w.kv_scales, m.kv_scales)
    assert m.kv_scales.dtype == torch.float32 and m.kv_scales.device.type == "cpu"
    # replica() copies the setting; it needs a device and a weight pack, which this object does not have: stand-ins for both
    m.device = torch.device("cuda", 0)
    m._packed, m._packed_key = {}, m._pack_key()
    r = m.replica()
    assert r._kv == m._kv and torch.equal(r.kv_scales, torch.tensor(good_table()))
    m.set_kv_cache_dtype("auto", scales=torch.tensor(good_table()))
    assert m._kv[0] == "auto" and len(m._kv) == 4
    m.set_kv_cache_dtype("fp8_e4m3")
    assert m._kv == ("fp8_e4m3", 1.0, 1.0) and torch.equal(m.kv_scales, torch.ones(2, 2, 2)), "a call without scales drops the table"
    m.set_kv_cache_dtype("fp8_e4m3", k_scale=0.25, v_scale=8.0)
    assert torch.equal(m.kv_scales, torch.tensor([0.25, 8.0]).view(1, 2, 1).expand(2, 2, 2))
    assert len(r._kv) == 4, "the replica keeps its own setting"


def test_new_entry_points_refuse_bad_arguments_without_an_engine():
    """the C entry points check their arguments before they touch a device: a null engine, and the op hooks' shapes."""
    from ivideogpt_amd import _lib
    lib = _lib.load()
    x = C.c_void_p(16)
    assert lib.ivg_set_kv_scales(None, x) == -1 and lib.ivg_get_kv_scales(None, x) == -1
    assert lib.ivg_kv_calibrate(None, x, 4, 1, 4, None, 0, 1, None) == -1
    assert lib.ivg_kv_calibration_reset(None) == -1 and lib.ivg_kv_calibration_finish(None, 1, None, None) == -1
    for B, heads, L, Lmax in ((0, 2, 4, 16), (2, 0, 4, 16), (2, 2, 17, 16), (2, 2, -1, 16)):
        assert lib.ivg_op_kv_absmax(x, x, B, heads, L, Lmax, x, None) == -1
        assert lib.ivg_op_kv8_pack_heads(x, x, x, x, B, heads, L, Lmax, x, x, None) == -1
    assert lib.ivg_op_kv_absmax(x, x, 2, 2, 4, 16, None, None) == -1
    for B, heads, Lmax, pos, P, G, row0 in ((0, 2, 16, 3, 0, 1, 0), (2, 0, 16, 3, 0, 1, 0), (2, 2, 16, 16, 0, 1, 0), (2, 2, 16, 3, 4, 2, 0),
                                            (2, 2, 16, 3, 0, 0, 0), (2, 2, 16, 3, 0, 2, 1)):
        assert lib.ivg_op_decode_attn8_heads(x, x, x, x, x, x, B, heads, Lmax, pos, P, G, row0, x, x, None) == -1
