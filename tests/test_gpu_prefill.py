"""The prompt pass at op level against fp64: RoPE + K / V append (rope_kv64_kernel, rope_kv_kernel), the one-pass causal attention
(flash_prefill_kernel) through ivg_op_prefill_attn, and the row-chunked cross-entropy of the eval forward (ce_rows_kernel /
ce_reduce_kernel behind Run::prefill's 4096-row lm_head chunks).

The whole-model tests see these kernels only through logits, where one wrong key out of ~700 near-uniform ones moves nothing
beyond bf16 noise.  Here every query row is held to its own bound, and "needle" inputs make single keys decisive: the diagonal key,
the key just past it (which must stay masked), the first / last key of every 32- and 64-key block, a key of the last partial tile.
test_needle_reference_detects_kernel_mutants (CPU) shows that the attention bound rejects a mask shifted either way, a V^T tile read
in the wrong key order and a dropped key of the last tile.

Attention bound, per query row (b, h, q), normwise over the 64 channels:
    max_d |out - ref| <= 2^-8 * (max_d sum_j w_j |v_jd| + max_d |ref_d|)
ref = softmax(q k^T / 8, causal) v in fp64 from the bf16-rounded roped q and k.  The kernel rounds P to bf16 for the P.V product
(relative 2^-9 per weight, while the row sum keeps the fp32 P: at most 2^-9 sum_j w_j |v_jd|) and rounds the output to bf16
(2^-9 |ref_d|); the scores and both accumulations are fp32 (bf16 x bf16 products are exact there).  The bound is twice that.
"""
import ctypes as C

import pytest
import torch

DEV = "cuda:0"
gpu = pytest.mark.gpu


def rup(x, a):
    return (x + a - 1) // a * a


def rope_tables(Lmax, hd, tdt):
    """cos / sin [Lmax][hd / 2] as the engine holds them (packing.py pack_llama: fp32 outer product, rounded through the model dtype)."""
    inv = 1.0 / (10000.0 ** (torch.arange(0, hd, 2, dtype=torch.float32) / hd))
    fr = torch.arange(Lmax, dtype=torch.float32)[:, None] * inv[None, :]
    return fr.cos().to(tdt).float(), fr.sin().to(tdt).float()


def rope_exact(x, cos, sin):
    """x (B, L, heads, hd) at positions 0 .. L-1 -> (the rotation in fp64, the scale of its terms |x1 c| + |x2 s|)."""
    x = x.double()
    L, half = x.shape[1], x.shape[-1] // 2
    c, s = cos[:L, None, :].double(), sin[:L, None, :].double()
    a, b = x[..., :half], x[..., half:]
    return torch.cat([a * c - b * s, b * c + a * s], -1), torch.cat([(a * c).abs() + (b * s).abs()] * 2, -1)


def rope_rounded(x, cos, sin):
    """the fp32 rotation rounded to x's dtype (what the kernels store; they may contract it into FMAs: one rounding apart)."""
    xf = x.float()
    L, half = x.shape[1], x.shape[-1] // 2
    c, s = cos[:L, None, :], sin[:L, None, :]
    a, b = xf[..., :half], xf[..., half:]
    return torch.cat([a * c - b * s, b * c + a * s], -1).to(x.dtype)


def split_qkv(qkv, B, L, heads, hd):
    t = qkv.view(B, L, 3, heads, hd)
    return t[:, :, 0], t[:, :, 1], t[:, :, 2]


def prefill_attn(qkv, kc, vc, vt, out, cos, sin, B, L, heads, hd, Lmax, tdt):
    from ivideogpt_amd import _lib
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = _lib.load().ivg_op_prefill_attn(p(qkv), p(kc), p(vc), p(vt), p(out), p(cos), p(sin), B, L, heads, hd, Lmax,
                                          1 if tdt == torch.bfloat16 else 0, st)
    torch.cuda.synchronize()
    return rc


def nan_buffers(B, heads, hd, Lmax, L, tdt):
    kc = torch.full((B, heads, Lmax, hd), float("nan"), dtype=tdt, device=DEV)
    vt = torch.full((B, heads, hd, rup(L, 64)), float("nan"), dtype=tdt, device=DEV)
    return kc, kc.clone(), vt


def aligned_copy(qkv, misalign):
    """qkv on the device; misalign: 8 bytes off 16-byte alignment (the launcher then takes the scalar kernel at hd = 64)."""
    if not misalign:
        return qkv.to(DEV).contiguous()
    es = qkv.element_size()
    base = torch.empty(qkv.numel() + 16 // es, dtype=qkv.dtype, device=DEV)
    off = (-(base.data_ptr() // es) + 8 // es) % (16 // es)
    t = base[off:off + qkv.numel()].view(qkv.shape)
    t.copy_(qkv)
    assert t.data_ptr() % 16 == 8
    return t


# ------------------------------------------------------------------------------------------------ (a) RoPE + K / V append
APPEND_PATHS = {   # name: (dtype, head_dim, heads, misaligned qkv)
    "rope_kv64-bf16": (torch.bfloat16, 64, 12, False),
    "rope_kv64-fp32": (torch.float32, 64, 12, False),
    "scalar-hd32-bf16": (torch.bfloat16, 32, 12, False),
    "scalar-hd128-bf16": (torch.bfloat16, 128, 6, False),
    "scalar-hd32-fp32": (torch.float32, 32, 12, False),
    "scalar-hd128-fp32": (torch.float32, 128, 6, False),
    "scalar-hd64-misaligned-bf16": (torch.bfloat16, 64, 12, True),
}


def check_append(qkv0, qkv1, kc, vc, vt, cos, sin, B, L, heads, hd, Lmax):
    """qkv0: the input (CPU), qkv1 / kc / vc / vt: the device buffers after the call (kc / vc / vt NaN-filled before it)."""
    tdt = qkv0.dtype
    ulp = 2.0 ** -7 if tdt == torch.bfloat16 else 2.0 ** -23
    q0, k0, v0 = split_qkv(qkv0, B, L, heads, hd)
    q1, k1, v1 = split_qkv(qkv1.cpu(), B, L, heads, hd)
    for name, x0, got in (("q (in place)", q0, q1), ("kc rows [0, L)", k0, kc[:, :, :L].cpu().permute(0, 2, 1, 3))):
        ex, scale = rope_exact(x0, cos, sin)
        err = (got.double() - ex).abs()
        bound = ulp * ex.abs() + 2.0 ** -22 * scale   # one rounding to the storage type + the fp32 rotation's own error
        print(f"{tdt} hd={hd} L={L} {name}: worst err / bound {(err / bound).max().item():.3f}")
        assert torch.isfinite(got).all() and (err <= bound).all(), \
            f"{name}: {(err > bound).sum().item()} elements beyond one rounding, worst excess {(err - bound).max().item():.3e}"
    assert torch.equal(v1, v0), "v in qkv must not change"
    assert torch.equal(vc[:, :, :L].cpu(), v0.permute(0, 2, 1, 3)), "vc rows [0, L) must equal v bit for bit"
    assert torch.isnan(kc[:, :, L:]).all() and torch.isnan(vc[:, :, L:]).all(), "cache rows >= L must not be written"
    vtc = vt.cpu()
    assert torch.equal(vtc[..., :L], v0.permute(0, 2, 3, 1)), "vt[bh][d][l] must equal v bit for bit for l < L"
    pad = vtc[..., L:]
    bits = pad.view(torch.int16 if tdt == torch.bfloat16 else torch.int32)
    assert (bits == 0).all(), f"V^T padding [L, rup(L, 64)) must be +0: {(bits != 0).sum().item()} of {bits.numel()} elements are not"


@gpu
@pytest.mark.parametrize("L", [1, 65, 751])
@pytest.mark.parametrize("path", list(APPEND_PATHS))
def test_rope_kv_append_vs_fp64(path, L):
    """ivg_op_prefill_attn without out = launch_rope_kv of one prefill layer, on the vectorised head-dim-64 kernel (bf16: 64 rows per
    workgroup, fp32: 32), the scalar kernel (head dims 32 / 128) and the scalar kernel at head dim 64 (qkv 8 bytes off 16-byte
    alignment).  Into NaN-filled kc / vc / vt: q roped in place and kc rows [0, L) within one rounding of the rotation; vc rows and V^T
    columns [0, L) bit-exact; V^T columns [L, rup(L, 64)) +0 -- the one-pass attention multiplies them by P = 0 -- and cache rows >= L
    untouched.
    Found by this test: the scalar kernel (and the fp32 vectorised one past rup(L, 32)) left the V^T padding as it was; the engine only
    got away with it because its vt is zeroed once at creation.  launch_rope_kv now zeroes [L, ldvt) on every prompt path."""
    tdt, hd, heads, mis = APPEND_PATHS[path]
    B, Lmax = 3, 800
    gen = torch.Generator().manual_seed(L * 7 + hd)
    qkv0 = (torch.randn(B * L, 3 * heads * hd, generator=gen) * 1.5).to(tdt)
    cos, sin = rope_tables(Lmax, hd, tdt)
    cd, sd = cos.to(DEV), sin.to(DEV)
    qkv = aligned_copy(qkv0, mis)
    kc, vc, vt = nan_buffers(B, heads, hd, Lmax, L, tdt)
    assert prefill_attn(qkv, kc, vc, vt, None, cd, sd, B, L, heads, hd, Lmax, tdt) == 0
    check_append(qkv0.view(B, L, -1), qkv, kc, vc, vt, cos, sin, B, L, heads, hd, Lmax)
    if mis:   # the scalar kernel agrees with rope_kv64 on the same input: within one bf16 ulp for the rotations, bit-exact for the copies
        qa = aligned_copy(qkv0, False)
        ka, va, vta = nan_buffers(B, heads, hd, Lmax, L, tdt)
        assert prefill_attn(qa, ka, va, vta, None, cd, sd, B, L, heads, hd, Lmax, tdt) == 0
        for a, b in ((qkv, qa), (kc[:, :, :L], ka[:, :, :L])):
            d = (a.float() - b.float()).abs()
            assert (d <= 2.0 ** -7 * torch.maximum(a.float().abs(), b.float().abs())).all(), f"scalar vs rope_kv64: max diff {d.max().item():.3e}"
        assert torch.equal(vc[:, :, :L], va[:, :, :L]) and torch.equal(vt, vta)


def test_prefill_hook_refuses_what_it_does_not_cover():
    """argument checks of ivg_op_prefill_attn that run before any launch (no GPU needed): L outside [1, Lmax], odd head_dim, B <= 0,
    an unknown dtype; with out: the one-pass kernel covers bf16 at head_dim 64 only and needs vt."""
    from ivideogpt_amd import _lib
    f = _lib.load().ivg_op_prefill_attn
    x = C.c_void_p(16)
    for args in ((1, 0, 12, 64, 10, 1), (1, 11, 12, 64, 10, 1), (0, 4, 12, 64, 10, 1), (1, 4, 12, 63, 10, 1), (1, 4, 12, 64, 10, 2)):
        assert f(x, x, x, x, None, None, None, *args, None) == -1, args
    assert f(x, x, x, x, x, None, None, 1, 4, 12, 64, 10, 0, None) == -1          # fp32 attention: not covered
    assert f(x, x, x, None, x, None, None, 1, 4, 12, 64, 10, 1, None) == -1       # out without vt
    assert f(C.c_void_p(24), x, x, x, x, None, None, 1, 4, 12, 64, 10, 1, None) == -1   # qkv not 16-byte aligned


# ------------------------------------------------------------------------------------------------ (b) one-pass attention
def needle_pairs(L):
    """(query, key) pairs whose score dominates the query's row (unique queries, unique keys), and the key of the last partial
    64-key tile that carries one: the diagonal key; the key just past the diagonal (masked: it must NOT dominate); the first and last
    key of every 32-key block (hence of every 64-key block); a key inside the last tile."""
    used_q, used_k, pairs = set(), set(), []

    def add(q, k):
        if 0 <= k < L and 0 <= q < L and q not in used_q and k not in used_k:
            used_q.add(q); used_k.add(k); pairs.append((q, k))
            return True
        return False

    def add_key(k):   # a free query at or after k, preferably in a later tile
        return k in used_k or any(add(q, k) for q in list(range(k + 37, L)) + list(range(k, min(k + 37, L))))

    for q in (0, 1, 5, 31, 32, 40, 63, 64, 100, 200, L // 2, L - 1):
        add(q, q)
    for q in (2, 33, 62, 70, L - 2):
        add(q, q + 1)
    for s in range(0, L, 32):
        add_key(s)
        add_key(min(s + 31, L - 1))
    t0 = (L - 1) // 64 * 64
    last = t0 + (L - 1 - t0) // 2
    assert add_key(last)
    return pairs, last


def attn_inputs(family, B, L, heads, Lmax, seed):
    """-> qkv (B * L, 3 * heads * 64) bf16 (pre-RoPE, what the hook is fed), cos, sin.  'needle': the wanted ROPED q / k are built
    first and rotated back, so after the kernel's RoPE (and bf16 rounding) each needle pair scores ~32 against <~10 for every other
    key of its row."""
    hd, tdt = 64, torch.bfloat16
    gen = torch.Generator().manual_seed(seed)
    cos, sin = rope_tables(Lmax, hd, tdt)
    if family == "random":
        return torch.randn(B * L, 3 * heads * hd, generator=gen).to(tdt), cos, sin
    qr = torch.randn(B, L, heads, hd, generator=gen, dtype=torch.float64) * 0.05
    kr = torch.randn(B, L, heads, hd, generator=gen, dtype=torch.float64)
    v = torch.randn(B, L, heads, hd, generator=gen, dtype=torch.float64)
    pairs, _ = needle_pairs(L)
    u = torch.randn(B, len(pairs), heads, hd, generator=gen, dtype=torch.float64)
    u = 16.0 * u / u.norm(dim=-1, keepdim=True)
    for i, (q, k) in enumerate(pairs):
        qr[:, q] = u[:, i]
        kr[:, k] = u[:, i]
    c, s = cos[:L, None, :].double(), sin[:L, None, :].double()
    n = c * c + s * s

    def unrope(y):
        a, b = y[..., :hd // 2], y[..., hd // 2:]
        return torch.cat([(a * c + b * s) / n, (b * c - a * s) / n], -1)
    qkv = torch.stack([unrope(qr), unrope(kr), v], 2).to(tdt)
    return qkv.reshape(B * L, 3 * heads * hd), cos, sin


def attention_fp64(qkv, cos, sin, B, L, heads, shift=0, v_perm=None, drop=None):
    """softmax(q k^T / 8, causal) v in fp64 from the bf16-rounded roped q, k -> (out (B, heads, L, 64), tolerance per row (B, heads, L)).
    Mutants for the sensitivity check: shift (key j visible to query i iff j <= i + shift), v_perm (key order of V within 32-key
    blocks), drop (a key nobody sees)."""
    q, k, v = split_qkv(qkv, B, L, heads, 64)
    q = rope_rounded(q, cos, sin).double().permute(0, 2, 1, 3)
    k = rope_rounded(k, cos, sin).double().permute(0, 2, 1, 3)
    v = v.double().permute(0, 2, 1, 3)
    if v_perm is not None:
        nb = L // 32 * 32
        v = v.clone()
        v[:, :, :nb] = v[:, :, :nb].reshape(B, heads, -1, 32, 64)[:, :, :, v_perm].reshape(B, heads, nb, 64)
    s = torch.einsum("bhqd,bhkd->bhqk", q, k) / 8.0
    i = torch.arange(L)
    vis = i[None, :] <= i[:, None] + shift
    if drop is not None:
        vis[:, drop] = False
    s = s.masked_fill(~vis, float("-inf"))
    w = torch.softmax(s, -1)
    out = w @ v
    tol = 2.0 ** -8 * ((w @ v.abs()).amax(-1) + out.abs().amax(-1))
    return out, tol


ATTN_CASES = [(B, heads, L, 1024) for L in (1, 2, 63, 64, 65, 127, 257, 514, 751) for heads in (12, 16) for B in (1, 3)]
ATTN_CASES += [(3, 12, 751, 751), (2, 16, 127, 127), (32, 16, 257, 300)]   # L = Lmax (the kr < Lmax clamp); B * heads = 512


@gpu
@pytest.mark.parametrize("family", ["random", "needle"])
@pytest.mark.parametrize("B,heads,L,Lmax", ATTN_CASES, ids=[f"B{c[0]}-h{c[1]}-L{c[2]}-Lmax{c[3]}" for c in ATTN_CASES])
def test_flash_prefill_vs_fp64(B, heads, L, Lmax, family):
    """ivg_op_prefill_attn with out (rope_kv64 + flash_prefill_kernel, bf16, head_dim 64) against softmax(q k^T / 8, causal) v in fp64,
    every query row within its own bound (module docstring).  kc rows past L stay NaN, so a mask that worked by arithmetic instead of
    select would poison whole rows; L = Lmax not a multiple of 64 runs the key-row clamp of the last tile."""
    qkv0, cos, sin = attn_inputs(family, B, L, heads, Lmax, seed=1000 * B + 10 * heads + L)
    ref, tol = attention_fp64(qkv0, cos, sin, B, L, heads)
    qkv = qkv0.to(DEV)
    kc, vc, vt = nan_buffers(B, heads, 64, Lmax, L, torch.bfloat16)
    out = torch.full((B * L, heads * 64), float("nan"), dtype=torch.bfloat16, device=DEV)
    assert prefill_attn(qkv, kc, vc, vt, out, cos.to(DEV), sin.to(DEV), B, L, heads, 64, Lmax, torch.bfloat16) == 0
    got = out.cpu().double().view(B, L, heads, 64).permute(0, 2, 1, 3)
    assert torch.isfinite(got).all(), f"{(~torch.isfinite(got)).any(-1).sum().item()} rows are not finite"
    err = (got - ref).abs().amax(-1)
    ratio = err / tol
    worst = divmod(int(ratio.argmax()), L)
    msg = (f"{family}: worst row (b*heads+h, q) = {worst}: err {err.flatten()[ratio.argmax()].item():.3e} vs bound "
           f"{tol.flatten()[ratio.argmax()].item():.3e} (err / bound {ratio.max().item():.3f}); {(ratio > 1).sum().item()} rows beyond")
    print(msg)
    assert (ratio <= 1).all(), msg


# ------------------------------------------------------------------------------------------------ (c) the bound can fail
def vt_tile_perm():
    """VtTile (llama_ops.hip): position lg * 8 + half * 4 + r of a staged 32-key block holds key half * 16 + lg * 4 + r."""
    return torch.tensor([((p // 4) % 2) * 16 + (p // 8) * 4 + p % 4 for p in range(32)])


@pytest.mark.parametrize("L", [63, 64, 65, 127, 257, 514, 751])
def test_needle_reference_detects_kernel_mutants(L):
    """CPU: with test_flash_prefill_vs_fp64's needle inputs and bound, each of these wrong attentions misses the true reference by at
    least 10x the bound on some row -- so that test fails on any of them: the causal mask shifted by -1 (diagonal dropped) and by +1
    (next key seen), V read in the VtTile key order of a 32-key block or in its inverse, one key of the last partial tile dropped."""
    B, heads, Lmax = 1, 12, 1024
    qkv, cos, sin = attn_inputs("needle", B, L, heads, Lmax, seed=1000 * B + 10 * heads + L)
    ref, tol = attention_fp64(qkv, cos, sin, B, L, heads)
    perm = vt_tile_perm()
    _, last = needle_pairs(L)
    mutants = {"mask -1": dict(shift=-1), "mask +1": dict(shift=1), "VtTile order": dict(v_perm=perm),
               "VtTile order undone": dict(v_perm=torch.argsort(perm)), f"key {last} dropped": dict(drop=last)}
    for name, kw in mutants.items():
        mut, _ = attention_fp64(qkv, cos, sin, B, L, heads, **kw)
        miss = torch.nan_to_num((mut - ref).abs().amax(-1), nan=0.0) / tol   # (mask -1 leaves row 0 empty: not counted)
        assert miss.max().item() >= 10, f"{name}: misses the reference by only {miss.max().item():.2f}x the bound"


# ------------------------------------------------------------------------------------------------ cross-entropy row chunks
@gpu
@pytest.mark.parametrize("B,dtype", [(6, "fp32"), (6, "bf16"), (12, "bf16")])
def test_eval_cross_entropy_across_row_chunks_vs_fp64(B, dtype):
    """The fused cross-entropy of the eval forward runs the lm_head over chunks of 4096 rows of the B * L = B * 751 positions (two
    chunks at B = 6, the boundary inside trajectory 5; three at B = 12).  2-layer small Llama at the released vocabulary (16386);
    labels -100 on the 257-token prompt, one label >= vocab (ignored, as ce_rows_kernel documents) and -100 exactly at the target of
    a chunk's last row (flat index 4096 at B = 6, 8192 at B = 12; at B = 12 the target of row 4095 is a real one).
    token_nll within 1e-4 of fp64 cross_entropy(ignore_index=-100) of the SAME engine's logits (which isolates the CE kernels from
    model error), 0 at every row's last position; per-trajectory sums / valid-target counts of ce_reduce_kernel against fp64 sums
    (counts exact), and the public loss / sample_loss."""
    from ivideogpt_amd import LlamaForCausalLM, weights as W
    cfg = dict(W.LLAMA_SMALL, num_hidden_layers=2)
    V, L = cfg["vocab_size"], 751
    assert B * L > 4096
    m = LlamaForCausalLM(cfg, W.random_llama_state_dict(cfg, 51), dtype=dtype).to(DEV)
    gen = torch.Generator().manual_seed(B)
    ids = torch.randint(0, V, (B, L), generator=gen)
    labels = ids.clone()
    labels[:, :257] = -100
    flat = labels.view(-1)
    flat[4096 if B == 6 else 8192] = -100
    if B == 12:
        assert flat[4096] >= 0
    labels[2, 600] = V + 3
    ids, labels = ids.to(DEV), labels.to(DEV)
    nll = torch.full((B, L), float("nan"), device=DEV)
    rows = torch.full((B, 2), float("nan"), device=DEV)
    m._ensure(B).eval_forward(ids, labels, nll, rows)
    torch.cuda.synchronize()
    tgt = labels[:, 1:].clone()
    tgt[tgt >= V] = -100
    lg = m.logits(ids)
    ref = torch.nn.functional.cross_entropy(lg[:, :-1].double().reshape(-1, V), tgt.reshape(-1), ignore_index=-100,
                                            reduction="none").view(B, L - 1)
    del lg
    err = (nll[:, :-1].double() - ref).abs()
    print(f"B={B} {dtype}: token_nll max |err| vs fp64 {err.max().item():.3e}; ce_reduce sums vs fp64 of token_nll "
          f"{((rows[:, 0].double() - nll[:, :-1].double().sum(1)).abs() / rows[:, 0].double().abs()).max().item():.3e} relative")
    assert torch.isfinite(nll).all() and err.max().item() < 1e-4, \
        f"token_nll vs fp64: max {err.max().item():.3e} at (b, l) = {divmod(int(err.argmax()), L - 1)}"
    assert (nll[:, -1] == 0).all() and (nll[:, :-1][tgt < 0] == 0).all()
    cnt = (tgt >= 0).sum(1).double()
    assert torch.equal(rows[:, 1].double(), cnt), (rows[:, 1], cnt)
    own = nll[:, :-1].double().sum(1)
    assert ((rows[:, 0].double() - own).abs() <= 1e-5 * own.abs()).all(), (rows[:, 0], own)
    assert ((rows[:, 0].double() - ref.sum(1)).abs() <= 1e-4 * cnt + 1e-5 * own.abs()).all()
    out = m(input_ids=ids, labels=labels)
    assert (out.sample_loss.double() - ref.sum(1) / cnt).abs().max().item() < 1e-4
    assert abs(out.loss.item() - (ref.sum() / cnt.sum()).item()) < 1e-4
