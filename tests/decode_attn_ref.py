"""One decode-attention step in fp64: the contract of ivg_op_shared_decode_attn and ivg_op_decode_attn24 (include/ivg.h), restated for
tests/test_gpu_decode_attn.py and its CPU self-check.  No GPU import.

The step at cache position `pos`: RoPE at `pos` of q and of the fed k (computed in fp32, rounded to the cache type), the fed k / v
appended at row `pos`, and out = softmax(q K^T / sqrt(hd)) V over the keys the trajectory sees -- its group slot's rows [0, P)
(slot = (b - row0) // G, cache row `slot`), its own rows [P, pos) (cache row b) and the fed token.  Three kinds:
  "bf16" / "fp32": decode_attn_kernel, caches and qkv / out of that type;
  "kv24": decode_attn24_kernel, fp32 qkv / out, K / V kept to 24 bits (RNE) in two planes; q stays fp32 after RoPE.

The rotation.  The kernel writes x1 * c - x2 * s and x2 * c + x1 * s in fp32, and the compiler may contract either half into a fused
multiply-add; near a rounding boundary of the cache type the forms round differently.  ROPE_FORMS lists, per half, the plain form and
the two contractions (one product exact, the other rounded first), emulated exactly (TwoSum plus a tie fix, round32 below: never one
fp64 rounding of a sum of two exact products).  A test identifies the form(s) the appended k matches bit for bit and builds q with it.

Per-row bound, for every (b, h), normwise over the head's hd channels (err = max_d |out_d - ref_d|), u = 2^-24:
  E_out   = u_out * R                       output rounding to nearest: u_out = 2^-8 (bf16: 8 significant bits), 2^-24 (fp32,
                                           kv24: the division a / sum)
  E_score = (hd + 4) u * S * (A + R)       score error: a sum of hd fp32 terms (bf16 x bf16 products are exact; fp32 / 24-bit ones
                                           are fma'd: one rounding per term) plus rsqrtf and the scale multiply; a score error
                                           delta_j moves the output by sum_j w_j delta_j (v_jd - out_d) <= max delta (A + R)
  E_exp   = u * max_d sum_j w_j (|s_j - m| + 2) |v_jd|
                                           exp(s_j - m): the fp32 difference (relative u of |s_j - m| in the exponent) and expf
  E_acc   = (ceil((pos+1)/gpb) + gpb + ceil((pos+1)/256) + 8) u * A
                                           the fixed-order weighted sum (one fma chain of ceil((pos+1)/gpb) keys per key group, then gpb
                                           groups added), the row sum (256 thread chains, a wave and a 4-wave tree) and the division
  bound   = 2 (E_out + E_score + E_exp + E_acc)   -- twice the first-order estimate
with A = max_d sum_j w_j |v_jd|, R = max_d |ref_d|, S = max_j sum_i |q_i k_ji| / sqrt(hd), m = max_j s_j, gpb = 256 / (hd / VEC) key
groups per workgroup.  These constants are derived, not fitted.

Mutants (keyword `mutant` of decode_ref) restate the kernel bugs the bound must reject; test_decode_reference_detects_kernel_mutants
shows each misses the true reference by >= 10x the bound on the needle inputs built to expose it.
"""
import math

import numpy as np
import torch

U = 2.0 ** -24
KINDS = ("bf16", "fp32", "kv24")


def vec_of(kind):
    return 8 if kind in ("bf16", "kv24") else 4


def geometry(kind, hd):
    """-> (lpk, gpb, step): lanes per key row, key groups per workgroup, key rows fetched per round (decode_attn_kernel)."""
    lpk = hd // vec_of(kind)
    gpb = 256 // lpk
    return lpk, gpb, gpb * 8


def rope_tables(Lmax, hd, kind):
    """cos / sin [Lmax][hd / 2] fp32 as the engine holds them (fp32 outer product, rounded through the model dtype)."""
    inv = 1.0 / (10000.0 ** (torch.arange(0, hd, 2, dtype=torch.float32) / hd))
    fr = torch.arange(Lmax, dtype=torch.float32)[:, None] * inv[None, :]
    tdt = torch.bfloat16 if kind == "bf16" else torch.float32
    return fr.cos().to(tdt).float(), fr.sin().to(tdt).float()


# ------------------------------------------------------------------------------------------------ exact fp32 arithmetic
def round32(p, q):
    """RN_fp32(p + q) for float64 arrays p, q that hold exact values: TwoSum gives s + e = p + q exactly; RN_fp32(s) is RN_fp32(p + q)
    unless s is itself a midpoint of two fp32 values (fp32 midpoints are fp64 numbers, so no other midpoint can lie between s and
    p + q), in which case the exact sum lies on e's side of it."""
    s = p + q
    bb = s - p
    e = (p - (s - bb)) + (q - bb)
    r = s.astype(np.float32)
    other = np.nextafter(r, np.where(s > r.astype(np.float64), np.float32(np.inf), np.float32(-np.inf)))
    tie = (s != r) & ((r.astype(np.float64) + other.astype(np.float64)) * 0.5 == s) & (e != 0)
    hi, lo = np.maximum(r, other), np.minimum(r, other)
    return np.where(tie, np.where(e > 0, hi, lo), r)


def _r32(x):
    return x.astype(np.float32).astype(np.float64)


# the two halves of the rotation, y1 = x1 c - x2 s and y2 = x2 c + x1 s: "plain" rounds both products, "fma1" keeps the first
# written product exact (fma(x1, c, -(x2 s)) / fma(x2, c, x1 s)), "fma2" the second (fma(-x2, s, x1 c) / fma(x1, s, x2 c))
HALF_FORMS = ("plain", "fma1", "fma2")
ROPE_FORMS = tuple((a, b) for a in HALF_FORMS for b in HALF_FORMS)


def rope_fp32(x1, x2, c, s, form):
    """x1, x2 (..., half), c, s (half,): fp32 values (numpy) -> (y1, y2) fp32, the rotation in `form` (a pair of HALF_FORMS)."""
    a, b = x1.astype(np.float64), x2.astype(np.float64)
    c, s = c.astype(np.float64), s.astype(np.float64)
    ac, bs, bc, as_ = a * c, b * s, b * c, a * s          # exact: products of two fp32 values
    y1 = {"plain": lambda: round32(_r32(ac), -_r32(bs)), "fma1": lambda: round32(ac, -_r32(bs)), "fma2": lambda: round32(-bs, _r32(ac))}
    y2 = {"plain": lambda: round32(_r32(bc), _r32(as_)), "fma1": lambda: round32(bc, _r32(as_)), "fma2": lambda: round32(as_, _r32(bc))}
    return y1[form[0]](), y2[form[1]]()


def to_bf16(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.bfloat16).float().numpy()


def to_f24(x):
    """fp32 -> 24 bits (sign, exponent, 15 mantissa bits), round to nearest even, as f24_round in llama_ops.hip."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7F + ((u >> 8) & 1)) & 0xFFFFFF00
    return u.astype(np.uint32).view(np.float32)


def store_round(x, kind):
    return to_bf16(x) if kind == "bf16" else (to_f24(x) if kind == "kv24" else np.asarray(x, dtype=np.float32))


def roped(x, cos_row, sin_row, kind, form, store=True):
    """x (..., hd) fp32 numpy -> the fp32 rotation in `form`, rounded to the cache type when `store` (q of kv24: not rounded)."""
    half = x.shape[-1] // 2
    y1, y2 = rope_fp32(x[..., :half], x[..., half:], cos_row, sin_row, form)
    y = np.concatenate([y1, y2], -1).astype(np.float32)
    return store_round(y, kind) if store else y


def rope_candidates(x, cos_row, sin_row, kind, store=True):
    return {f: roped(x, cos_row, sin_row, kind, f, store) for f in ROPE_FORMS}


# ------------------------------------------------------------------------------------------------ the step
def split_qkv(qkv, heads, hd):
    """qkv (B, 3 * heads * hd) torch -> q, k, v (B, heads, hd) fp32 numpy."""
    x = qkv.float().numpy().reshape(qkv.shape[0], 3, heads, hd)
    return x[:, 0], x[:, 1], x[:, 2]


def slots(B, G, row0):
    return (np.arange(B) - row0) // G


def decode_ref(qkv, K, V, cos, sin, kind, heads, hd, pos, P=0, G=1, row0=0, form=("plain", "plain"), mutant=None):
    """qkv (B, 3 * heads * hd) as fed; K, V (rows, heads, Lmax, hd) fp32 values of the caches BEFORE the step (poison where unread);
    cos, sin [Lmax][hd / 2] fp32.  -> dict(out (B, heads, hd) fp64, bound (B, heads), k_new / v_new (B, heads, hd) fp32 as appended).
    mutant: None or one of
      ("drop", t)            key t not seen (t = pos: the fed token)
      ("key_from", t, t2)    key t (its k and v) read from row t2 of the same source
      ("v_shift",)           the weight of key t applied to the v of key t + 1 (the last key's own v kept)
      ("rope_pos", p)        RoPE of q and the fed k at position p
      ("scale", x)           scores scaled by x instead of 1 / sqrt(hd)
      ("include_next",)      row pos + 1 of the trajectory's own cache row seen as one more key
      ("prefix_own", t)      key t < P read from the trajectory's own cache row
      ("own_from_slot", t)   key t >= P read from the slot's cache row
      ("slot_no_row0",)      slot = b // G"""
    B = qkv.shape[0]
    mutant = mutant or ("none",)
    q, k, v = split_qkv(qkv, heads, hd)
    rp = mutant[1] if mutant[0] == "rope_pos" else pos
    c, s = cos[rp].numpy(), sin[rp].numpy()
    qr = roped(q, c, s, kind, form, store=kind != "kv24").astype(np.float64)
    kn = roped(k, c, s, kind, form)
    vn = store_round(v, kind)
    slot = (np.arange(B) // G) if mutant[0] == "slot_no_row0" else slots(B, G, row0)
    scale = mutant[1] if mutant[0] == "scale" else 1.0 / math.sqrt(hd)
    # key list: (source, t) per key; source "slot" / "own" / "fed"
    keys = [("slot" if t < P else "own", t) for t in range(pos)] + [("fed", pos)]
    if mutant[0] == "drop":
        keys = [kt for kt in keys if kt[1] != mutant[1]]
    elif mutant[0] == "key_from":
        keys = [(src, mutant[2] if t == mutant[1] else t) if src != "fed" else (src, t) for src, t in keys]
    elif mutant[0] == "include_next":
        keys.append(("own", pos + 1))
    elif mutant[0] == "prefix_own":
        keys = [("own", t) if t == mutant[1] else (src, t) for src, t in keys]
    elif mutant[0] == "own_from_slot":
        keys = [("slot", t) if t == mutant[1] else (src, t) for src, t in keys]
    vkeys = keys[1:] + keys[-1:] if mutant[0] == "v_shift" else keys
    Kn = K.numpy() if isinstance(K, torch.Tensor) else K
    Vn = V.numpy() if isinstance(V, torch.Tensor) else V

    def gather(X, new, ks, b0, b1):
        code = np.array([{"slot": 0, "own": 1, "fed": 2}[src] for src, _ in ks])
        ts = np.array([0 if src == "fed" else t for src, t in ks])
        r = np.where(code[None, :] == 0, slot[b0:b1, None], np.arange(b0, b1)[:, None])
        g = X.transpose(0, 2, 1, 3)[r, ts[None, :]].transpose(0, 2, 1, 3).astype(np.float64)   # (nb, heads, n, hd)
        g[:, :, code == 2] = new[b0:b1, :, None]
        return g
    out = np.empty((B, heads, hd))
    bound = np.empty((B, heads))
    n = len(keys)
    chunk = max(1, int(4e6 // max(1, heads * n * hd)))
    _, gpb, _ = geometry(kind, hd)
    u_out = 2.0 ** -8 if kind == "bf16" else U
    n_acc = -(-(pos + 1) // gpb) + gpb + -(-(pos + 1) // 256) + 8
    for b0 in range(0, B, chunk):
        b1 = min(B, b0 + chunk)
        Kb, Vb = gather(Kn, kn, keys, b0, b1), gather(Vn, vn, vkeys, b0, b1)
        qb = qr[b0:b1]
        sc = np.einsum("bhd,bhkd->bhk", qb, Kb) * scale
        m = sc.max(-1, keepdims=True)
        e = np.exp(sc - m)
        w = e / e.sum(-1, keepdims=True)
        o = np.einsum("bhk,bhkd->bhd", w, Vb)
        av = np.abs(Vb)
        A = np.einsum("bhk,bhkd->bhd", w, av).max(-1)
        R = np.abs(o).max(-1)
        S = np.einsum("bhd,bhkd->bhk", np.abs(qb), np.abs(Kb)).max(-1) / math.sqrt(hd)
        Ex = U * np.einsum("bhk,bhkd->bhd", w * (np.abs(sc - m) + 2.0), av).max(-1)
        bound[b0:b1] = 2.0 * (u_out * R + (hd + 4) * U * S * (A + R) + Ex + n_acc * U * A)
        out[b0:b1] = o
    return dict(out=out, bound=bound, k_new=kn, v_new=vn, q=qr)


# ------------------------------------------------------------------------------------------------ inputs
def needle_positions(pos, step, P=0, shared=False):
    """key rows a needle is planted in: 0, pos - 1, the fed token (pos), the round edges step - 1, step, 2 step - 1, 2 step below pos,
    and in SHARED mode P - 1 and P."""
    c = [0, pos - 1, pos, step - 1, step, 2 * step - 1, 2 * step]
    if shared:
        c += [P - 1, P]
    return sorted({t for t in c if 0 <= t <= pos})


def make_case(kind, hd, heads, B, Lmax, pos, P=0, G=1, row0=0, family="random", seed=0, poison=True):
    """-> dict(qkv, K, V, cos, sin, rows, needles).  K / V (rows, heads, Lmax, hd) fp32 values already in the cache type; rows =
    max(B, slots) + 1 (the last row is nobody's).  Unread elements: NaN with poison, else finite random values plus, in the needle
    family, a trap needle at row pos + 1 (a step that reads it is wrong).  Unread means: rows [pos, Lmax) of every cache row; rows
    [0, P) of rows that are no group's slot; rows [P, pos) of rows >= B.
    needle: each (slot, h) gets one needle row t* (needle_positions, cycled), k = lambda * (its roped q) in the cache (or the fed raw
    k = lambda * raw q), v = 3 * randn; q is shared by the trajectories of a group, lambda puts about half the softmax mass on the needle."""
    gen = torch.Generator().manual_seed(seed)
    tdt = torch.bfloat16 if kind == "bf16" else torch.float32
    cos, sin = rope_tables(Lmax, hd, kind)
    _, _, step = geometry(kind, hd)
    sl = slots(B, G, row0)
    rows = max(B, int(sl.max()) + 1) + 1
    shape = (rows, heads, Lmax, hd)
    K = torch.full(shape, float("nan"))
    V = torch.full(shape, float("nan"))
    if not poison:
        K.normal_(generator=gen)
        V.normal_(generator=gen)
    readable = torch.zeros(rows, Lmax, dtype=torch.bool)
    readable[torch.as_tensor(np.unique(sl)), :P] = True
    readable[:B, P:pos] = True
    n_read = int(readable.sum()) * heads * hd
    kr = torch.from_numpy(store_round((torch.randn(n_read, generator=gen) * 1.2).numpy(), kind))
    vr = torch.from_numpy(store_round(torch.randn(n_read, generator=gen).numpy(), kind))
    sel = readable[:, None, :, None].expand(shape)
    K[sel] = kr
    V[sel] = vr
    qkv = torch.randn(B, 3 * heads * hd, generator=gen, dtype=torch.float64) * 1.5
    needles = None
    c, s = cos[pos].numpy(), sin[pos].numpy()
    if family == "needle":
        qkv = qkv.view(B, 3, heads, hd)
        qg = torch.randn(int(sl.max()) + 1, heads, hd, generator=gen, dtype=torch.float64)
        qg = 4.0 * qg / qg.norm(dim=-1, keepdim=True)
        qkv[:, 0] = qg[torch.as_tensor(sl)]
        qkv = qkv.view(B, -1)
    qkv = qkv.to(tdt)
    if kind == "bf16":
        qkv = condition_q(qkv, heads, hd, c, s)
    if family == "needle":
        lam = (math.log(pos + 1) + 8.0 / hd) * math.sqrt(hd) / 16.0     # needle score ~ ln(number of keys) + the others' mean lift
        tl = needle_positions(pos, step, P, shared=G > 1)
        q, _, _ = split_qkv(qkv, heads, hd)
        qr = roped(q, c, s, kind, ("plain", "plain"), store=kind != "kv24")
        x = qkv.float().view(B, 3, heads, hd).clone()
        needles = np.empty((B, heads), dtype=np.int64)
        for b in range(B):
            for h in range(heads):
                t = tl[(int(sl[b]) * heads + h) % len(tl)]
                needles[b, h] = t
                vv = 3.0 * torch.randn(hd, generator=gen)
                kk = torch.from_numpy(store_round(lam * qr[b, h], kind))
                if t == pos:
                    x[b, 1, h] = lam * x[b, 0, h]
                    x[b, 2, h] = vv
                elif t < P:
                    K[sl[b], h, t] = kk
                    V[sl[b], h, t] = torch.from_numpy(store_round(vv.numpy(), kind))
                else:
                    K[b, h, t] = kk
                    V[b, h, t] = torch.from_numpy(store_round(vv.numpy(), kind))
                if not poison and pos + 1 < Lmax:
                    K[b, h, pos + 1] = kk        # trap: only a step that reads row pos + 1 sees it
        qkv = x.view(B, -1).to(tdt)
    if not poison:   # (poison is NaN in every type; the values read were rounded when drawn)
        K = torch.from_numpy(store_round(K.numpy(), kind))
        V = torch.from_numpy(store_round(V.numpy(), kind))
    return dict(qkv=qkv, K=K, V=V, cos=cos, sin=sin, rows=rows, needles=needles, readable=readable)


def condition_q(qkv, heads, hd, c, s):
    """bf16: nudge raw q pairs whose roped value rounds differently under the rotation forms (about 2^-16 of them) by one bf16 ulp
    until every form gives the same q -- so q does not depend on which form the kernel uses (the fed k still identifies it)."""
    x = qkv.float().numpy().reshape(qkv.shape[0], 3, heads, hd).copy()
    half = hd // 2
    for _ in range(8):
        cand = rope_candidates(x[:, 0], c, s, "bf16")
        first = cand[ROPE_FORMS[0]]
        bad = np.zeros(first.shape, dtype=bool)
        for f in ROPE_FORMS[1:]:
            bad |= cand[f] != first
        bad = bad[..., :half] | bad[..., half:]
        if not bad.any():
            break
        for part in (slice(0, half), slice(half, hd)):
            y = x[:, 0, :, part]
            y[bad] = to_bf16(y[bad] * (1.0 + 2.0 ** -7))
    return torch.from_numpy(x.reshape(qkv.shape)).to(torch.bfloat16)


# ------------------------------------------------------------------------------------------------ 24-bit planes
def kv24_planes(X, poison_mask=None):
    """(rows, heads, Lmax, 64) fp32 values already on 24 bits -> (rows, heads, Lmax * 192) uint8: [Lmax][64] upper 16 bits |
    [Lmax][64] next byte.  NaN elements become 0xFF bytes (decoded: NaN)."""
    rows, heads, Lmax, hd = X.shape
    u = X.numpy().view(np.uint32)
    hi = (u >> 16).astype(np.uint16)
    lo = ((u >> 8) & 0xFF).astype(np.uint8)
    nan = np.isnan(X.numpy())
    hi[nan] = 0xFFFF
    lo[nan] = 0xFF
    out = np.concatenate([hi.view(np.uint8).reshape(rows, heads, Lmax * hd * 2), lo.reshape(rows, heads, Lmax * hd)], -1)
    return torch.from_numpy(np.ascontiguousarray(out))


def kv24_values(planes, Lmax, hd=64):
    """inverse of kv24_planes (any bytes): (rows, heads, Lmax * 192) uint8 -> (rows, heads, Lmax, 64) fp32."""
    p = planes.numpy()
    rows, heads = p.shape[:2]
    hi = np.ascontiguousarray(p[..., :Lmax * hd * 2]).view(np.uint16).reshape(rows, heads, Lmax, hd).astype(np.uint32)
    lo = p[..., Lmax * hd * 2:].reshape(rows, heads, Lmax, hd).astype(np.uint32)
    return torch.from_numpy(((hi << 16) | (lo << 8)).view(np.float32))
