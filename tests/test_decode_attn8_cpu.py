"""CPU self-check of tests/decode_attn8_ref.py (the FP8 K / V cache's contract, include/ivg.h ivg_set_kv_format): the store rule against
torch's float8_e4m3fn, the reference against a plain fp64 einsum, every kernel mutant rejected by at least MARGIN x the per-row bound
on inputs built to expose it, and the Python argument checks of kv_cache_dtype / set_kv_cache_dtype (no engine, no GPU)."""
import numpy as np
import pytest
import torch

import decode_attn8_ref as R8

MARGIN = 10.0


def torch_store(x, clamp=True):
    """the issue's reference conversion: torch on the CPU."""
    t = torch.from_numpy(np.asarray(x, dtype=np.float32))
    if clamp:
        t = t.clamp(-448, 448)
    return t.to(torch.float8_e4m3fn).view(torch.uint8).numpy()


# ------------------------------------------------------------------------------------------------ the store rule
def test_decode_table_is_torchs_e4m3fn_over_all_256_codes():
    codes = torch.arange(256, dtype=torch.int32).to(torch.uint8)
    want = codes.view(torch.float8_e4m3fn).float().double().numpy()
    got = R8.e4m3_decode(codes.numpy())
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isnan(got), (codes.numpy() & 0x7F) == 0x7F)
    fin = ~np.isnan(want)
    assert np.array_equal(got[fin], want[fin]) and np.array_equal(np.signbit(got[fin]), np.signbit(want[fin]))
    assert got[0x7E] == 448.0 and got[0x01] == 2.0 ** -9 and got[0x08] == 2.0 ** -6
    # the other dialect (the mutant's decode): torch's float8_e4m3fnuz
    want = codes.view(torch.float8_e4m3fnuz).float().double().numpy()
    got = R8.e4m3_decode(codes.numpy(), fnuz=True)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~np.isnan(want)], want[~np.isnan(want)])


def test_store_rule_round_trips_every_code_and_rounds_like_torch():
    """every finite code is a fixed point; every midpoint of two neighbouring values and both its fp32 neighbours, every bf16 value
    in [-600, 600] and a million random fp32 values round as torch rounds them (RNE, ties to the even code, sign of zero kept)."""
    codes = np.arange(256, dtype=np.uint8)
    fin = (codes & 0x7F) != 0x7F
    vals = R8.e4m3_decode(codes)[fin].astype(np.float32)
    assert np.array_equal(R8.e4m3_encode(vals), codes[fin])
    pos = R8.e4m3_decode(np.arange(0x7F, dtype=np.uint8)).astype(np.float32)
    mid = ((pos[:-1].astype(np.float64) + pos[1:]) / 2).astype(np.float32)
    probe = np.concatenate([mid, np.nextafter(mid, np.float32(0)), np.nextafter(mid, np.float32(np.inf))])
    probe = np.concatenate([probe, -probe])
    assert np.array_equal(R8.e4m3_encode(probe), torch_store(probe))
    bf = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(torch.bfloat16).float().numpy()
    bf = bf[np.isfinite(bf) & (np.abs(bf) <= 600)]
    assert np.array_equal(R8.e4m3_encode(bf), torch_store(bf))
    for scale in (1.0, 0.25, 8.0):
        assert np.array_equal(R8.store8(bf, scale), torch_store(bf / np.float32(scale)))
    rnd = (torch.randn(1 << 20, generator=torch.Generator().manual_seed(1)) * 40).numpy()
    assert np.array_equal(R8.e4m3_encode(rnd), torch_store(rnd))


def test_store_rule_clamps_explicitly_and_keeps_nan():
    edges = np.array([447.9, 448.0, 460.0, 464.0, 470.0, 1e9, np.inf], dtype=np.float32)
    x = np.concatenate([edges, -edges])
    got = R8.e4m3_encode(x)
    assert np.array_equal(got, torch_store(x))
    assert np.array_equal(got, np.array([0x7E] * 7 + [0xFE] * 7, dtype=np.uint8)), "a finite (or infinite) value must saturate to +-448"
    nan = R8.e4m3_encode(np.array([np.nan, -np.nan], dtype=np.float32))
    assert ((nan & 0x7F) == 0x7F).all() and ((torch_store(np.array([np.nan], dtype=np.float32)) & 0x7F) == 0x7F).all()
    # what the clamp is for: the bare conversion turns 470 and beyond into NaN (460 still rounds to 448)
    bare = torch_store(x, clamp=False)
    assert np.array_equal(R8.canon(R8.e4m3_encode(x, clamp=False)), R8.canon(bare))
    assert bare[2] == 0x7E and ((bare[4:7] & 0x7F) == 0x7F).all()


# ------------------------------------------------------------------------------------------------ the reference and its mutants
def independent_fp64(case, heads, pos, P, G, row0, ref, k_scale, v_scale):
    """softmax(q (k_scale K8)^T / 8) (v_scale V8) per trajectory with torch einsum and torch's own e4m3 decode."""
    B = case["qkv"].shape[0]
    dec = lambda c: torch.as_tensor(c).view(torch.float8_e4m3fn).float().double()  # noqa: E731
    K, V = dec(case["K8"]) * k_scale, dec(case["V8"]) * v_scale
    kn, vn = dec(torch.from_numpy(ref["k_new"])) * k_scale, dec(torch.from_numpy(ref["v_new"])) * v_scale
    q = torch.from_numpy(ref["q"])
    out = torch.empty(B, heads, 64, dtype=torch.float64)
    for b in range(B):
        s_ = (b - row0) // G
        Kb = torch.cat([K[s_, :, :P], K[b, :, P:pos], kn[b][:, None]], 1)
        Vb = torch.cat([V[s_, :, :P], V[b, :, P:pos], vn[b][:, None]], 1)
        w = torch.softmax(torch.einsum("hd,hkd->hk", q[b], Kb) / 8.0, -1)
        out[b] = torch.einsum("hk,hkd->hd", w, Vb)
    return out.numpy()


def misses(args, kw, ref, mut):
    got = R8.decode_ref8(*args, **kw, mutant=mut)["out"]
    miss = np.abs(got - ref["out"]).max(-1)
    return np.where(np.isnan(miss), np.inf, miss) / ref["bound"]     # a NaN output misses by any factor


@pytest.mark.parametrize("shared", [False, True], ids=["plain", "shared"])
def test_reference_detects_kernel_mutants(shared):
    """Needle inputs at the kernel's step (512 rows per round), scales 2^-2 / 2^3, unread rows finite: the reference agrees with an
    independent fp64 einsum over torch-decoded bytes to 1e-6 x its bound, and every mutant misses it by >= MARGIN x the bound on at
    least one row -- on the main case (fnuz decode, a scale dropped, a neighbouring row, a prefix row from the own cache row), on a
    saturating case (no clamp) and on a one-key case whose fed v lies in e4m3's subnormal range (the step's own k / v unrounded: with
    a 3-bit mantissa against bf16's 8 the normal range alone gives 7.5 x, a tie in the subnormal range 32 x)."""
    step = R8.STEP
    Lmax, pos = 2 * step + 8, 2 * step + 1
    B, heads = (6, 8) if shared else (2, 8)
    G, row0 = (3, -1) if shared else (1, 0)
    P = step if shared else 0
    ks, vs = 0.25, 8.0
    kw = dict(P=P, G=G, row0=row0, k_scale=ks, v_scale=vs)
    case = R8.make_case8(heads, B, Lmax, pos, P, G, row0, family="needle", seed=8 + shared, poison=False, k_scale=ks, v_scale=vs)
    args = (case["qkv"], case["K8"], case["V8"], case["cos"], case["sin"], heads, pos)
    ref = R8.decode_ref8(*args, **kw)
    assert np.isfinite(ref["out"]).all() and (ref["bound"] > 0).all()
    ind = independent_fp64(case, heads, pos, P, G, row0, ref, ks, vs)
    assert (np.abs(ind - ref["out"]).max(-1) <= 1e-6 * ref["bound"]).all(), "the reference disagrees with a plain fp64 einsum"
    muts = {"rows decoded as fnuz": ("fnuz",), "k_scale dropped": ("no_k_scale",), "v_scale dropped": ("no_v_scale",)}
    for t in (step - 1, step):
        muts[f"key {t} read from row {t + 1}"] = ("key_from", t, t + 1)
    if shared:
        muts[f"shared key P-1 = {P - 1} read from the own row"] = ("prefix_own", P - 1)
    worst = {name: float(misses(args, kw, ref, mut).max()) for name, mut in muts.items()}
    # no clamp: fed k / v beyond the format's range
    sat = R8.make_case8(heads, B, Lmax, pos, P, G, row0, family="random", seed=18 + shared, poison=False, k_scale=ks, v_scale=vs, saturate=True)
    sargs = (sat["qkv"], sat["K8"], sat["V8"], sat["cos"], sat["sin"], heads, pos)
    sref = R8.decode_ref8(*sargs, **kw)
    assert np.isfinite(sref["out"]).all(), "a finite input became NaN under the clamp"
    assert (sref["v_new"][..., :8] & 0x7F == 0x7E).all() and (sref["k_new"] & 0x7F == 0x7E).any()   # (the rotation mixes k's elements)
    worst["no clamp"] = float(misses(sargs, kw, sref, ("no_clamp",)).max())
    # the step's own k / v unrounded: pos = 0 (the fed token is the only key), fed v = 1.5 * 2^-9 * v_scale, a tie between two subnormals
    x = torch.randn(B, 3, heads, 64, generator=torch.Generator().manual_seed(3))
    x[:, 2] = 1.5 * 2.0 ** -9 * vs
    one = dict(P=0, G=1, row0=0, k_scale=ks, v_scale=vs)
    empty = torch.full((B + 1, heads, 8, 64), R8.NAN_CODE, dtype=torch.uint8)
    oargs = (x.view(B, -1).to(torch.bfloat16), empty, empty, case["cos"], case["sin"], heads, 0)
    oref = R8.decode_ref8(*oargs, **one)
    assert np.array_equal(oref["out"], np.full((B, heads, 64), 2.0 ** -8 * vs)), "1.5 * 2^-9 must round to the even code (2^-8)"
    worst["own k / v unrounded"] = float(misses(oargs, one, oref, ("own_unrounded",)).max())
    print(f"kv8 step {step} pos {pos} P {P}: " + ", ".join(f"{k}: {v:.1f}x" for k, v in worst.items()))
    weak = {k: round(v, 2) for k, v in worst.items() if not v >= MARGIN}
    assert not weak, f"mutants the bound does not reject by {MARGIN}x: {weak}"


# ------------------------------------------------------------------------------------------------ the Python argument checks
def small_cfg(heads=2, hidden=128):
    from ivideogpt_amd import weights as W
    return dict(W.LLAMA_SMALL, hidden_size=hidden, intermediate_size=256, num_hidden_layers=2, num_attention_heads=heads,
                num_key_value_heads=heads)


def test_kv_cache_dtype_arguments_are_checked_before_any_engine_work():
    """a wrong name, a wrong model dtype / head_dim or a bad scale is a ValueError from the constructor, from_config and
    set_kv_cache_dtype of a model that has no weights, no device and no engine; good settings are kept and carried by the wrapper."""
    from ivideogpt_amd import HeadModelWithAction, LlamaForCausalLM
    m = LlamaForCausalLM(small_cfg(), None, dtype="bf16")
    assert m._kv == ("auto", 1.0, 1.0)
    assert LlamaForCausalLM(small_cfg(), None, dtype="bf16", kv_cache_dtype="fp8_e4m3")._kv == ("fp8_e4m3", 1.0, 1.0)
    assert LlamaForCausalLM.from_config(small_cfg(), dtype="bf16", kv_cache_dtype="fp8_e4m3")._kv[0] == "fp8_e4m3"
    for name in ("fp8", "e4m3", "fp8_e5m2", "", None, 1):
        with pytest.raises(ValueError, match="kv_cache_dtype"):
            LlamaForCausalLM(small_cfg(), None, dtype="bf16", kv_cache_dtype=name)
        with pytest.raises(ValueError, match="kv_cache_dtype"):
            LlamaForCausalLM.from_config(small_cfg(), dtype="bf16", kv_cache_dtype=name)
        with pytest.raises(ValueError, match="kv_cache_dtype"):
            LlamaForCausalLM.from_pretrained("/nonexistent/checkpoint", kv_cache_dtype=name)
        with pytest.raises(ValueError, match="kv_cache_dtype"):
            m.set_kv_cache_dtype(name)
    for dtype, heads in (("fp32", 2), ("x3", 2), ("bf16", 4), ("bf16", 1)):       # head_dim 64 / 64 / 32 / 128
        with pytest.raises(ValueError, match="bf16 model with head_dim 64"):
            LlamaForCausalLM(small_cfg(heads), None, dtype=dtype, kv_cache_dtype="fp8_e4m3")
        with pytest.raises(ValueError, match="bf16 model with head_dim 64"):
            LlamaForCausalLM(small_cfg(heads), None, dtype=dtype).set_kv_cache_dtype("fp8_e4m3")
        LlamaForCausalLM(small_cfg(heads), None, dtype=dtype).set_kv_cache_dtype("auto")
    for bad in (0.0, -1.0, 3.0, 0.3, float("inf"), float("nan"), 2.0 ** -140, 2.0 ** 127, "x", None):
        for kw in (dict(k_scale=bad), dict(v_scale=bad)):
            with pytest.raises(ValueError, match="power of two"):
                m.set_kv_cache_dtype("fp8_e4m3", **kw)
            with pytest.raises(ValueError, match="power of two"):
                m.set_kv_cache_dtype("auto", **kw)
    assert m._kv == ("auto", 1.0, 1.0), "a refused setting must leave the model as it was"
    w = HeadModelWithAction(m, 4, 513, 16, 2, 4)
    assert w.set_kv_cache_dtype("fp8_e4m3", k_scale=0.25, v_scale=2 ** 3) is w
    assert m._kv == ("fp8_e4m3", 0.25, 8.0)
    assert all(R8.scale_ok(s) for s in (1.0, 0.25, 8.0, 2.0 ** -126, 2.0 ** 126)) and not any(R8.scale_ok(s) for s in (0.0, 3.0, 2.0 ** 127))


def test_set_kv_format_refuses_bad_arguments_without_an_engine():
    """the C entry points check their arguments before they touch a device: a null engine, and the op hooks' scales and positions."""
    import ctypes as C
    from ivideogpt_amd import _lib
    lib = _lib.load()
    assert lib.ivg_set_kv_format(None, 1, 1.0, 1.0) == -1
    x = C.c_void_p(16)
    for ks, vs in ((3.0, 1.0), (1.0, 0.0), (float("nan"), 1.0), (1.0, float("inf")), (-2.0, 1.0)):
        assert lib.ivg_op_decode_attn8(x, x, x, x, x, x, 2, 2, 16, 3, 0, 1, 0, ks, vs, None) == -1, (ks, vs)
        assert lib.ivg_op_kv8_pack(x, x, x, x, 2, 4, 16, ks, vs, None) == -1, (ks, vs)
    for B, heads, Lmax, pos, P, G, row0 in ((0, 2, 16, 3, 0, 1, 0), (2, 0, 16, 3, 0, 1, 0), (2, 2, 16, 16, 0, 1, 0), (2, 2, 16, 3, 4, 2, 0),
                                            (2, 2, 16, 3, 0, 0, 0), (2, 2, 16, 3, 0, 2, 1)):
        assert lib.ivg_op_decode_attn8(x, x, x, x, x, x, B, heads, Lmax, pos, P, G, row0, 1.0, 1.0, None) == -1
    assert lib.ivg_op_kv8_pack(x, x, x, x, 2, 17, 16, 1.0, 1.0, None) == -1
    assert lib.ivg_debug_counter(b"decode_attn8") >= 0
