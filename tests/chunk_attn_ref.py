"""Reference, inputs and bound for the attention of ivg_kv_extend's chunk pass (chunk_attn_kernel, llama_ops.hip; hook
ivg_op_chunk_attn): T query rows per (trajectory, head) at positions pos0 .. pos0 + T - 1 against a cache that already holds roped
K / V rows [0, pos0) and receives rows [pos0, pos0 + T) from the same call.

Reference: softmax(q k^T / 8, key j visible to row t iff j <= pos0 + t) v in fp64, from the bf16-rounded roped q and k.
Bound, per query row, the one tests/test_gpu_prefill.py derives for the same arithmetic (P rounded to bf16 for P.V while the row sum
keeps the fp32 P, output rounded to bf16, fp32 scores and accumulations):
    max_d |out - ref| <= 2^-8 (max_d sum_j w_j |v_jd| + max_d |ref_d|)
The kernel's split of the key range over four waves and their merge rescale fp32 partial sums by exp(m_w - M) <= 1: a few fp32
roundings, three orders of magnitude below the bf16 terms the bound is made of.

"Needle" inputs make single keys decisive, spread over the (trajectory, head) pairs of a case because a chunk has only T query rows:
key pos0 - 1 (the last kept row), key pos0 (the first appended one), key 0, the diagonal, the key just past the diagonal (masked: it
must NOT dominate), the first and last key of every 32-key block (hence of every 64-key tile and of every wave's share), a key of the
last partial tile."""
import torch

from test_gpu_prefill import rope_tables

HD = 64
CASES = [(0, 17), (1, 1), (63, 2), (64, 16), (514, 17), (530, 17), (530, 33), (100, 65), (783, 17)]   # (pos0, T); Lmax = 800
LMAX = 800


def rope_exact_at(x, cos, sin, pos):
    """x (B, T, heads, hd) at positions pos (T,) -> (the rotation in fp64, the scale of its terms |x1 c| + |x2 s|)."""
    x = x.double()
    half = x.shape[-1] // 2
    c, s = cos[pos][:, None, :].double(), sin[pos][:, None, :].double()
    a, b = x[..., :half], x[..., half:]
    return torch.cat([a * c - b * s, b * c + a * s], -1), torch.cat([(a * c).abs() + (b * s).abs()] * 2, -1)


def rope_rounded_at(x, cos, sin, pos):
    """the fp32 rotation at positions pos rounded to x's dtype (what rope_kv64_kernel stores, up to FMA contraction)."""
    xf = x.float()
    half = x.shape[-1] // 2
    c, s = cos[pos][:, None, :], sin[pos][:, None, :]
    a, b = xf[..., :half], xf[..., half:]
    return torch.cat([a * c - b * s, b * c + a * s], -1).to(x.dtype)


def needle_plan(pos0, T, slots):
    """-> (pairs, last): pairs[s] = [(t, key), ...] for (trajectory, head) pair s, unique rows and unique keys within a pair; every wanted
    key is decisive for some row of some pair.  last: the key of the last partial tile that carries a needle."""
    nk = pos0 + T
    pairs = [[] for _ in range(slots)]
    used_t = [set() for _ in range(slots)]
    used_k = [set() for _ in range(slots)]

    def place(key, rows):
        for s in range(slots):
            if key in used_k[s]:
                continue
            for t in rows:
                if 0 <= t < T and t not in used_t[s]:
                    used_t[s].add(t); used_k[s].add(key); pairs[s].append((t, key))
                    return True
        return False

    def visible_rows(key):   # rows that see `key`, late rows first (they also cross the most tiles)
        return [t for t in range(T - 1, -1, -1) if pos0 + t >= key]

    wanted = [pos0 - 1, pos0, 0]
    t0 = (nk - 1) // 64 * 64
    last = t0 + (nk - 1 - t0) // 2
    wanted.append(last)
    for s in range(0, nk, 32):
        wanted += [s, min(s + 31, nk - 1)]
    for key in wanted:
        if 0 <= key < nk:
            assert any(key in used_k[s] for s in range(slots)) or place(key, visible_rows(key)), f"no room for key {key}"
    for t in dict.fromkeys((0, T // 2, 14, 15, 16, 30, 31, T - 2)):     # the key just past the diagonal: masked
        if 0 <= t < T - 1:
            place(pos0 + t + 1, [t])
    for t in dict.fromkeys((0, 1, T // 2, 15, 16, 31, 32, T - 1)):      # the diagonal
        if 0 <= t < T:
            place(pos0 + t, [t])
    return pairs, last


def chunk_inputs(family, B, heads, pos0, T, seed):
    """-> dict(qkv (B * T, 3 * heads * 64) bf16 pre-RoPE, k_past / v_past (B, heads, pos0, 64) bf16 as the cache holds them, cos, sin,
    pairs).  'needle': the wanted ROPED q / k are built first and the chunk's rotated back, so that after the kernel's RoPE each needle
    pair scores ~32 against <~10 for every other key of its row."""
    tdt = torch.bfloat16
    gen = torch.Generator().manual_seed(seed)
    cos, sin = rope_tables(LMAX, HD, tdt)
    pos = pos0 + torch.arange(T)
    if family == "random":
        return dict(qkv=torch.randn(B * T, 3 * heads * HD, generator=gen).to(tdt), k_past=torch.randn(B, heads, pos0, HD, generator=gen).to(tdt),
                    v_past=torch.randn(B, heads, pos0, HD, generator=gen).to(tdt), cos=cos, sin=sin, pairs=None)
    nk = pos0 + T
    qr = torch.randn(B, T, heads, HD, generator=gen, dtype=torch.float64) * 0.05
    kr = torch.randn(B, nk, heads, HD, generator=gen, dtype=torch.float64)
    v = torch.randn(B, nk, heads, HD, generator=gen, dtype=torch.float64)
    pairs, _ = needle_plan(pos0, T, B * heads)
    for s, plist in enumerate(pairs):
        b, h = divmod(s, heads)
        u = torch.randn(len(plist), HD, generator=gen, dtype=torch.float64)
        u = 16.0 * u / u.norm(dim=-1, keepdim=True)
        for i, (t, key) in enumerate(plist):
            qr[b, t, h] = u[i]
            kr[b, key, h] = u[i]
    c, s_ = cos[pos][:, None, :].double(), sin[pos][:, None, :].double()
    n = c * c + s_ * s_

    def unrope(y):
        a, b = y[..., :HD // 2], y[..., HD // 2:]
        return torch.cat([(a * c + b * s_) / n, (b * c - a * s_) / n], -1)
    qkv = torch.stack([unrope(qr), unrope(kr[:, pos0:]), v[:, pos0:]], 2).to(tdt)
    return dict(qkv=qkv.reshape(B * T, 3 * heads * HD), k_past=kr[:, :pos0].permute(0, 2, 1, 3).to(tdt).contiguous(),
                v_past=v[:, :pos0].permute(0, 2, 1, 3).to(tdt).contiguous(), cos=cos, sin=sin, pairs=pairs)


def roped_operands(inp, B, heads, pos0, T, rope_pos0=None):
    """-> q (B, heads, T, 64), K, V (B, heads, pos0 + T, 64) as bf16 tensors: what the attention kernel reads after RoPE + append.
    rope_pos0: the position the CHUNK's keys are roped at (mutant: 0 instead of pos0)."""
    t = inp["qkv"].view(B, T, 3, heads, HD)
    pos = pos0 + torch.arange(T)
    kpos = pos if rope_pos0 is None else rope_pos0 + torch.arange(T)
    q = rope_rounded_at(t[:, :, 0], inp["cos"], inp["sin"], pos).permute(0, 2, 1, 3)
    k = rope_rounded_at(t[:, :, 1], inp["cos"], inp["sin"], kpos).permute(0, 2, 1, 3)
    v = t[:, :, 2].permute(0, 2, 1, 3)
    return q, torch.cat([inp["k_past"], k], 2), torch.cat([inp["v_past"], v], 2)


def attention_fp64(inp, B, heads, pos0, T, shift=0, drop=None, rope_pos0=None, v_perm=None):
    """-> (out (B, heads, T, 64) fp64, tolerance per row (B, heads, T)).  Mutants for the sensitivity check: shift (key j visible to row t
    iff j <= pos0 + t + shift), drop (a key nobody sees), rope_pos0 (chunk keys roped from there), v_perm (key order of V within 32-key
    blocks)."""
    q, K, V = (x.double() for x in roped_operands(inp, B, heads, pos0, T, rope_pos0))
    nk = pos0 + T
    if v_perm is not None:
        nb = nk // 32 * 32
        V = V.clone()
        V[:, :, :nb] = V[:, :, :nb].reshape(B, heads, -1, 32, HD)[:, :, :, v_perm].reshape(B, heads, nb, HD)
    s = torch.einsum("bhqd,bhkd->bhqk", q, K) / 8.0
    vis = torch.arange(nk)[None, :] <= (pos0 + torch.arange(T))[:, None] + shift
    if drop is not None:
        vis[:, drop] = False
    s = s.masked_fill(~vis, float("-inf"))
    w = torch.softmax(s, -1)
    out = w @ V
    tol = 2.0 ** -8 * ((w @ V.abs()).amax(-1) + out.abs().amax(-1))
    return out, tol


def mfma_key_perm():
    """The key order chunk_attn_kernel's P.V product enumerates a 32-key step in: element 8 lg + j is key (j // 4) * 16 + 4 lg + j % 4."""
    return torch.tensor([((p % 8) // 4) * 16 + (p // 8) * 4 + p % 4 for p in range(32)])


def kernel_arithmetic_fp32(inp, B, heads, pos0, T):
    """chunk_attn_kernel restated in fp32 torch: query tiles of 32 rows (16 when T <= 16), the tile's keys [0, nk) in 64-key tiles dealt
    to four waves (tile kt to wave kt % 4), per wave an online softmax in fp32 with P rounded to bf16 for P.V and the row sum on the
    fp32 P, masked scores by select, the waves merged in the order 0 .. 3, the output rounded to bf16.  -> (B, heads, T, 64) bf16."""
    q, K, V = (x.float() for x in roped_operands(inp, B, heads, pos0, T))
    QT = 32 if T > 16 else 16
    out = torch.empty(B, heads, T, HD)
    ninf = float("-inf")
    for t0 in range(0, T, QT):
        rows = torch.arange(t0, min(t0 + QT, T))
        nk = pos0 + min(T, t0 + QT)
        qt = q[:, :, rows]
        R = len(rows)
        m = torch.full((4, B, heads, R), ninf)
        l = torch.zeros(4, B, heads, R)
        o = torch.zeros(4, B, heads, R, HD)
        for kt in range((nk + 63) // 64):
            w = kt % 4
            keys = torch.arange(kt * 64, min(kt * 64 + 64, nk))
            s = torch.einsum("bhqd,bhkd->bhqk", qt, K[:, :, keys]) * 0.125
            vis = keys[None, :] <= (pos0 + rows)[:, None]
            s = torch.where(vis, s, torch.tensor(ninf))
            mn = torch.maximum(m[w], s.amax(-1))
            ms = torch.where(mn == ninf, torch.zeros(()), mn)
            alpha = torch.exp(m[w] - ms)
            p = torch.exp(s - ms[..., None])
            l[w] = l[w] * alpha + p.sum(-1)
            o[w] = o[w] * alpha[..., None] + p.bfloat16().float() @ V[:, :, keys]
            m[w] = mn
        M = m.amax(0)
        sc = torch.exp(m - M)
        L = torch.zeros(B, heads, R)
        acc = torch.zeros(B, heads, R, HD)
        for w in range(4):
            L = L + l[w] * sc[w]
            acc = acc + o[w] * sc[w][..., None]
        out[:, :, rows] = acc / L[..., None]
    return out.bfloat16()
