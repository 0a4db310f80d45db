"""One decode-attention step over the FP8 (e4m3) K / V cache in fp64: the contract of ivg_set_kv_format / ivg_op_decode_attn8 /
ivg_op_kv8_pack (include/ivg.h), restated for tests/test_gpu_decode_attn8.py and its CPU self-check.  No GPU import.

Built on tests/decode_attn_ref.py (imported, not edited): its fp32-exact RoPE forms (the kernel ropes as the bf16 instance of
decode_attn_kernel does, so the same three contractions per half are the candidates), its bf16 case builder and its per-row bound.
Added here: the e4m3 store rule, the step over byte caches with the two scales, and the new kernel's geometry.

Store rule.  byte = e4m3_rne(clamp(x / scale, -448, +448)), x a bf16 value, scale a power of two (the division is exact), OCP e4m3fn
(bias 7, no infinities, 0x7F / 0xFF NaN, largest finite 448): e4m3_encode below, by nearest neighbour in the table of the 127
non-negative finite values, ties to the even code; the clamp lets NaN through (NaN -> a NaN code), so a finite value never becomes
NaN.  tests/test_decode_attn8_cpu.py checks it against torch's float8_e4m3fn.

The step at `pos` (decode_ref8): q and the fed k roped in fp32 (in `form`) and rounded to bf16; the fed k and v rounded to bf16, then
to their e4m3 codes, and USED as decoded from those codes; out = softmax(q (k_scale K8)^T / 8) (v_scale V8) over the group slot's rows
[0, P), the trajectory's own rows [P, pos) and the fed token.

Per-row bound: decode_attn_ref's, unchanged in form, with the bf16 output rounding (u_out = 2^-8):
  bound = 2 (u_out R + (hd + 4) u S (A + R) + E_exp + (ceil((pos+1)/gpb) + gpb + ceil((pos+1)/256) + 8) u A)
with A, R, S, E_exp as defined there over the SCALED keys and values.  Why it carries over: a bf16 x e4m3 product has at most 8 + 4
significant bits and is exact in fp32, so a score is a sum of hd fp32 terms as in the bf16 kernel; k_scale / 8 and v_scale are
powers of two (their products round nothing); the output rounds to bf16.  Only gpb changes: the kernel puts FOUR lanes on a 64-byte
key row (16 bytes each), so gpb = 64 key groups per workgroup and 8 rows in flight per lane make step = 512 rows per fetch round.
Derived, not fitted.
"""
import math

import numpy as np
import torch

import decode_attn_ref as R

HD = 64
LPK, GPB, UNR = 4, 64, 8          # decode_attn8_kernel: lanes per key row, key groups per workgroup, rows in flight per lane
STEP = GPB * UNR                  # key rows per fetch round
E4M3_MAX = 448.0
NAN_CODE = 0x7F


# ------------------------------------------------------------------------------------------------ the formats
def _decode_table(fnuz):
    c = np.arange(256)
    s, e, m = c >> 7, (c >> 3) & 15, (c & 7).astype(np.float64)
    bias = 8 if fnuz else 7
    v = np.where(e == 0, m / 8.0 * 2.0 ** (1 - bias), (1.0 + m / 8.0) * 2.0 ** (e.astype(np.float64) - bias))
    v = np.where(s == 1, -v, v)
    if fnuz:
        v[0x80] = np.nan          # no negative zero: the code is NaN
    else:
        v[0x7F] = v[0xFF] = np.nan
    return v


_FN, _FNUZ = _decode_table(False), _decode_table(True)
_POS = _FN[:0x7F].copy()          # the 127 non-negative finite values, ascending: code == index


def e4m3_decode(codes, fnuz=False):
    """uint8 codes -> float64 values (OCP e4m3fn; fnuz=True: the other FP8 dialect, bias 8 -- a kernel mutant)."""
    return (_FNUZ if fnuz else _FN)[np.asarray(codes, dtype=np.uint8)]


def e4m3_encode(y, clamp=True):
    """float values -> uint8 e4m3fn codes, round to nearest, ties to the even code; clamp: to +-448 first (NaN stays NaN).  Without the
    clamp a magnitude beyond 464 (the midpoint of 448 and the 480 the format has no code for) has no finite code: NaN."""
    y = np.asarray(y, dtype=np.float32)
    nan = np.isnan(y)
    a = np.abs(y).astype(np.float64)
    over = ~nan & (a > 464.0) & (not clamp)
    a = np.where(nan, 0.0, np.minimum(a, E4M3_MAX))
    hi = np.minimum(np.searchsorted(_POS, a, side="left"), 126)
    lo = np.maximum(hi - 1, 0)
    dlo, dhi = a - _POS[lo], _POS[hi] - a
    code = np.where((dhi < dlo) | ((dhi == dlo) & (hi % 2 == 0)), hi, lo).astype(np.uint8)
    code = code | (np.signbit(y).astype(np.uint8) << 7)
    return np.where(nan | over, np.uint8(NAN_CODE), code).astype(np.uint8)


def store8(x, scale, clamp=True):
    """the store rule: bf16 values x (fp32 numpy) -> codes."""
    return e4m3_encode(np.asarray(x, dtype=np.float32) / np.float32(scale), clamp)


def canon(codes):
    """codes with both NaN codes mapped to one (a NaN's sign is not part of the contract)."""
    c = np.asarray(codes, dtype=np.uint8)
    return np.where((c & 0x7F) == 0x7F, np.uint8(NAN_CODE), c)


def scale_ok(s):
    return isinstance(s, float) and math.isfinite(s) and s > 0 and math.frexp(s)[0] == 0.5 and 2.0 ** -126 <= s <= 2.0 ** 126


# ------------------------------------------------------------------------------------------------ the step
def decode_ref8(qkv, K8, V8, cos, sin, heads, pos, P=0, G=1, row0=0, k_scale=1.0, v_scale=1.0, form=("plain", "plain"), mutant=None):
    """qkv (B, 3 * heads * 64) bf16 as fed; K8, V8 (rows, heads, Lmax, 64) uint8 codes of the caches BEFORE the step (NaN codes where
    unread); cos, sin [Lmax][32] fp32.  -> dict(out (B, heads, 64) fp64, bound (B, heads), k_new / v_new (B, heads, 64) uint8 as appended).
    mutant: None or one of
      ("fnuz",)              every code decoded as e4m3fnuz
      ("no_clamp",)          the fed k / v converted without the clamp
      ("own_unrounded",)     the fed k / v used as their bf16 values for this step (the codes appended are the right ones)
      ("no_k_scale",)        k_scale dropped from the scores
      ("no_v_scale",)        v_scale dropped from the output
      ("key_from", t, t2)    key t (its k and v) read from row t2 of the same cache row
      ("prefix_own", t)      key t < P read from the trajectory's own cache row"""
    B = qkv.shape[0]
    mutant = mutant or ("none",)
    q, k, v = R.split_qkv(qkv, heads, HD)
    c, s = cos[pos].numpy(), sin[pos].numpy()
    qr = R.roped(q, c, s, "bf16", form).astype(np.float64)
    k16, v16 = R.roped(k, c, s, "bf16", form), R.to_bf16(v)
    kn8, vn8 = store8(k16, k_scale, mutant[0] != "no_clamp"), store8(v16, v_scale, mutant[0] != "no_clamp")
    fnuz = mutant[0] == "fnuz"
    ks = 1.0 if mutant[0] == "no_k_scale" else k_scale
    vs = 1.0 if mutant[0] == "no_v_scale" else v_scale
    kf, vf = e4m3_decode(kn8, fnuz) * ks, e4m3_decode(vn8, fnuz) * vs
    if mutant[0] == "own_unrounded":
        kf, vf = k16.astype(np.float64) * (ks / k_scale), v16.astype(np.float64) * (vs / v_scale)
    slot = R.slots(B, G, row0)
    t = np.broadcast_to(np.arange(pos), (B, pos)).copy()
    row = np.where(t < P, slot[:, None], np.arange(B)[:, None])
    if mutant[0] == "key_from":
        t[:, mutant[1]] = mutant[2]
    elif mutant[0] == "prefix_own":
        row[:, mutant[1]] = np.arange(B)
    K8n = K8.numpy() if isinstance(K8, torch.Tensor) else K8
    V8n = V8.numpy() if isinstance(V8, torch.Tensor) else V8
    hidx = np.arange(heads)[None, :, None]
    Kb = np.concatenate([e4m3_decode(K8n[row[:, None, :], hidx, t[:, None, :]], fnuz) * ks, kf[:, :, None]], 2)   # (B, heads, pos + 1, 64)
    Vb = np.concatenate([e4m3_decode(V8n[row[:, None, :], hidx, t[:, None, :]], fnuz) * vs, vf[:, :, None]], 2)
    sc = np.einsum("bhd,bhkd->bhk", qr, Kb) / math.sqrt(HD)
    m = sc.max(-1, keepdims=True)
    e = np.exp(sc - m)
    w = e / e.sum(-1, keepdims=True)
    o = np.einsum("bhk,bhkd->bhd", w, Vb)
    av = np.abs(Vb)
    A = np.einsum("bhk,bhkd->bhd", w, av).max(-1)
    Rr = np.abs(o).max(-1)
    S = np.einsum("bhd,bhkd->bhk", np.abs(qr), np.abs(Kb)).max(-1) / math.sqrt(HD)
    Ex = R.U * np.einsum("bhk,bhkd->bhd", w * (np.abs(sc - m) + 2.0), av).max(-1)
    n_acc = -(-(pos + 1) // GPB) + GPB + -(-(pos + 1) // 256) + 8
    bound = 2.0 * (2.0 ** -8 * Rr + (HD + 4) * R.U * S * (A + Rr) + Ex + n_acc * R.U * A)
    return dict(out=o, bound=bound, k_new=kn8, v_new=vn8, q=qr)


# ------------------------------------------------------------------------------------------------ inputs
def make_case8(heads, B, Lmax, pos, P=0, G=1, row0=0, family="random", seed=0, poison=True, k_scale=1.0, v_scale=1.0, saturate=False):
    """decode_attn_ref.make_case for the bf16 kernel at head_dim 64 (its needles sit on 0, pos - 1, pos, 255, 256, 511, 512 and the
    shared edges: STEP - 1 and STEP are among them), its K / V then stored by the rule: -> dict(qkv, K8, V8 uint8 (rows, heads, Lmax,
    64), cos, sin, rows, needles).  Unread elements: NaN codes with poison.  saturate: elements 0..7 of every fed k and v and of every
    fourth readable cache row lie beyond the format's range (+-500 ... +-2000 times the scale; the cache rows hold +-448 there)."""
    case = R.make_case("bf16", HD, heads, B, Lmax, pos, P, G, row0, family=family, seed=seed, poison=poison)
    K, V = case["K"].numpy().copy(), case["V"].numpy().copy()
    qkv = case["qkv"]
    if saturate:
        gen = np.random.default_rng(seed + 1)
        big = lambda n, sc: R.to_bf16((gen.choice([-1.0, 1.0], n) * gen.uniform(500.0, 2000.0, n) * sc).astype(np.float32))  # noqa: E731
        x = qkv.float().view(B, 3, heads, HD).clone()
        x[:, 1, :, :8] = torch.from_numpy(big((B, heads, 8), k_scale) * 0.02)     # (k: large, but the fed score stays comparable)
        x[:, 1, :, :2] = torch.from_numpy(big((B, heads, 2), k_scale))
        x[:, 2, :, :8] = torch.from_numpy(big((B, heads, 8), v_scale))
        qkv = x.view(B, -1).to(torch.bfloat16)
        sel = ~np.isnan(V[:, :, ::4, :8])
        V[:, :, ::4, :8] = np.where(sel, big(V[:, :, ::4, :8].shape, v_scale), np.nan)
    K8, V8 = store8(K, k_scale), store8(V, v_scale)
    return dict(qkv=qkv, K8=torch.from_numpy(K8), V8=torch.from_numpy(V8), cos=case["cos"], sin=case["sin"], rows=case["rows"],
                needles=case["needles"], readable=case["readable"])
