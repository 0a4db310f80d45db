"""The tokenizer's one-pass attention (csrc/llama_ops.hip, xattn_kernel through ivg_op_xattn) in fp64: the contract
tests/test_gpu_xattn.py holds all six instances to, its case table, input families and the kernel mutants of
tests/test_xattn_cpu.py.  No GPU import.

  q   [M][P][C]   frame m = b * F + f; head h reads channels [h * hd, (h + 1) * hd), hd = C / nh
  Kp  [B][kv][C]  projected keys of trajectory b (shared by its F frames)
  VpT [B][C][kv]  projected values, transposed
  out [M][P][C] = softmax(q K^T / sqrt(hd)) V per (frame, head), no mask.  bf16 only.
Instances: hd 32, 64, 128, 192 stage 64-key tiles (KT = 64), hd 512 and 768 32-key tiles (KT = 32; VtTile<32>, the XOR-swizzled
form).  The kernel walks the kv / KT tiles with an online softmax: running max mx, p = expf(s - mx) summed in fp32 and ROUNDED TO
BF16 for the P.V MFMA, o and the row sum rescaled by alpha = expf(mx_old - mx_new) per tile, out = o / sum.

Per-row bound, for every (frame, head, query row), normwise over the head's hd channels (err = max_d |out_d - ref_d|), u = 2^-24.
The reference is fp64 on the same bf16 inputs.  With w_j the softmax weights, s_j the scores, m = max_j s_j,
A = max_d sum_j w_j |v_jd|, R = max_d |ref_d|, S = max_j sum_i |q_i k_ji| / sqrt(hd), nt = kv / KT:
  E_out   = 2^-9 R                            the bf16 store (as a term; the doubled sum covers the half ulp 2^-8)
  E_p     = 2^-9 A                            p rounded to bf16 for the P.V product while the row sum keeps the fp32 p: each weight
                                              is off by 2^-9 of itself relative to the normaliser
  E_score = (hd + 4) u S (A + R)              a chain of hd fp32 accumulations (bf16 x bf16 products are exact), the fp32 scale
                                              1 / sqrtf(hd) and its multiply; a score error delta_j moves the output by
                                              sum_j w_j delta_j (v_jd - out_d) <= max delta (A + R).  At hd = 768 this term is
                                              comparable to the bf16 ones.
  E_exp   = u max_d sum_j w_j (|s_j - m| + 2) |v_jd|
                                              expf(s_j - mx) and the alphas that later carry it to the final max: the exponents'
                                              magnitudes telescope to |s_j - m| (relative u each, in the exponent); + 2 for expf
  E_acc   = (kv + 3 nt + kv / 4 + 4 nt + 2 + 2) u A
                                              the P.V MFMA chain over all kv keys; per tile the rescale of o (expf of alpha: 2, the
                                              multiply: 1); the row sum: KT / 4 additions per lane and tile (kv / 4 in all), per
                                              tile alpha (2) and lsum * alpha + ps (2), two cross-lane additions; 1 / sum and o * inv
  bound   = 2 (E_out + E_p + E_score + E_exp + E_acc)
Derived, not fitted.

Mutants (keyword `mutant` of xattn_ref) restate kernel bugs; tests/test_xattn_cpu.py shows each misses the true reference by >= 10x
the bound on at least one case, and that an fp32 restatement of the kernel (tile order, online softmax, P rounded to bf16) stays
within half the bound on every case.  The bf16 store alone can take the whole of 2 E_out (a value just above a binade's first
rounding boundary is off by 2^-8 of itself), so the restatement is held to half of the bound WITHOUT E_out on its value before the
store (`out_term=False`, `rounded=False`) and to the full bound after it.
"""
import math
import zlib

import torch

U = 2.0 ** -24
U_BF16 = 2.0 ** -9
INSTANCES = [(128, 4), (256, 4), (512, 4), (768, 4), (512, 1), (768, 1)]     # (C, nh): hd 32, 64, 128, 192, 512, 768
SHAPES = [(64, 64, 3, 1), (128, 192, 2, 3), (64, 320, 2, 3), (128, 320, 3, 1)]   # (P, kv, B, F); the first is the engine's self-attention form
FAMILIES = ("random", "needle", "ramp_up", "ramp_down", "large", "flat")
CASES = [(C, nh) + s + (fam,) for C, nh in INSTANCES for s in SHAPES for fam in FAMILIES]


def case_id(c):
    C, nh, P, kv, B, F, fam = c
    return f"hd{C // nh}-C{C}-nh{nh}-P{P}-kv{kv}-B{B}-F{F}-{fam}"


def key_tile(hd):
    return 32 if hd >= 512 else 64


def bf16(x):
    return x.float().to(torch.bfloat16).float()


def needle_keys(kv):
    """key indices a needle lands on: all 64 positions of the first 64-key tile (= every position of a 32-key block in both halves,
    and both 32-key tiles of the KT = 32 form), and all of the last 64 keys (the last tile; kv - 1 is the last key overall)"""
    return sorted(set(range(64)) | set(range(kv - 64, kv)))


def needle_index(c):
    """-> [M][nh][P] the needle key of every query row"""
    C, nh, P, kv, B, F, fam = c
    keys = torch.tensor(needle_keys(kv))
    m, h, i = torch.meshgrid(torch.arange(B * F), torch.arange(nh), torch.arange(P), indexing="ij")
    return keys[(i + 64 * (m // F) + 5 * h + 17 * (m % F)) % len(keys)]


def make_inputs(c):
    """-> q [M][P][C], Kp [B][kv][C], VpT [B][C][kv] as fp32 tensors of bf16 values (family: module docstring of the test)."""
    C, nh, P, kv, B, F, fam = c
    hd, M = C // nh, B * F
    g = torch.Generator().manual_seed(zlib.crc32(case_id(c).encode()) % 1000003)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)   # noqa: E731
    V = 3.0 * rn(B, kv, nh, hd)
    rs = math.sqrt(math.sqrt(hd))                                       # |q| = |k| = a * hd^(1/4) * ... gives scores of order a^2
    if fam in ("random", "large"):
        a = math.sqrt(2.0) if fam == "random" else 10.0
        q, K = a * rn(M, P, nh, hd), a * rn(B, kv, nh, hd)
    elif fam == "flat":
        q = rn(M, P, nh, hd)
        K = rn(B, 1, nh, hd).expand(B, kv, nh, hd).clone()
    elif fam in ("ramp_up", "ramp_down"):
        d = rn(B, 1, nh, hd)
        d = d / d.norm(dim=-1, keepdim=True) * rs
        t = torch.linspace(-8.0, 8.0, kv, dtype=torch.float64).view(1, kv, 1, 1)
        K = d * (t if fam == "ramp_up" else -t)
        rho = 0.5 + torch.rand(M, P, nh, 1, generator=g, dtype=torch.float64)
        q = (rho * d.repeat_interleave(F, 0)) + 0.05 * rn(M, P, nh, hd)
    else:   # needle: unit-direction keys of norm kappa; q = rho * (its needle key's direction): score T on the needle, T cos(theta) elsewhere
        K = rn(B, kv, nh, hd)
        K = K / K.norm(dim=-1, keepdim=True)
        T = math.log(kv) + 0.5 * (math.log(kv) ** 2) / hd              # exp(T) ~ sum of the others' exp(T cos), cos ~ N(0, 1 / hd)
        idx = needle_index(c)                                           # [M][nh][P]
        Kb = K.repeat_interleave(F, 0)                                  # [M][kv][nh][hd]
        pick = torch.gather(Kb.permute(0, 2, 1, 3), 2, idx[..., None].expand(M, nh, P, hd))   # [M][nh][P][hd]
        kappa = math.sqrt(T) * rs
        q = (kappa * pick).permute(0, 2, 1, 3)
        K = kappa * K
    q, K, V = bf16(q.reshape(M, P, C)), bf16(K.reshape(B, kv, C)), bf16(V.reshape(B, kv, C))
    return q, K, V.transpose(1, 2).contiguous()


def _v_permutation(kv, hd, kind):
    """index [hd][kv]: the key whose V the weight of key j meets, per channel d, under a staging bug of VtTile"""
    j = torch.arange(kv)
    blk, r32 = j // 32 * 32, j % 32
    half, lg, r = r32 // 16, (r32 % 16) // 4, r32 % 4
    if kind == "natural_order":       # tile staged in natural key order, read as if permuted: position lg * 8 + half * 4 + r
        return (blk + lg * 8 + half * 4 + r)[None, :].expand(hd, kv)
    x = (torch.arange(hd)[:, None] >> 1) & 3          # "no_xor": staged with the XOR key of the row, read without it
    return blk[None] + half[None] * 16 + (lg[None] ^ x) * 4 + r[None]


def xattn_ref(q, Kp, VpT, F, nh, mutant=None, out_term=True):
    """-> (out fp64 [M][P][C], bound [M][nh][P]).  Mutants:
      "natural_order"   V^T tile read in natural key order, without the permutation inside every 32-key block
      "no_xor"          the 32-key form read without its XOR swizzle (KT = 32 instances only)
      "drop_last_tile"  the last key tile not visited
      "no_alpha"        o not rescaled by alpha when the running max moves (the row sum is)
      "b_mod_F"         trajectory b = m % F
      "scale_C"         scores scaled by 1 / sqrt(C)
      "head_shift"      head h reads the K / V channels of head (h + 1) % nh"""
    M, P, C = q.shape
    B, kv, _ = Kp.shape
    hd = C // nh
    KT = key_tile(hd)
    nt = kv // KT
    bidx = torch.arange(M) % F if mutant == "b_mod_F" else torch.arange(M) // F
    bidx = bidx.clamp(max=B - 1)
    qh = q.double().view(M, P, nh, hd).permute(0, 2, 1, 3)                    # M nh P hd
    Kh = Kp.double().view(B, kv, nh, hd).permute(0, 2, 1, 3)                  # B nh kv hd
    Vh = VpT.double().view(B, nh, hd, kv).transpose(2, 3)                     # B nh kv hd
    if mutant == "head_shift":
        Kh, Vh = Kh.roll(-1, 1), Vh.roll(-1, 1)
    Kh, Vh = Kh[bidx], Vh[bidx]
    scale = 1.0 / math.sqrt(C if mutant == "scale_C" else hd)
    s = torch.einsum("mhpd,mhkd->mhpk", qh, Kh) * scale
    if mutant == "drop_last_tile":
        s, Kh, Vh = s[..., :kv - KT], Kh[:, :, :kv - KT], Vh[:, :, :kv - KT]
    m = s.max(-1, keepdim=True).values
    e = torch.exp(s - m)
    w = e / e.sum(-1, keepdim=True)
    if mutant == "no_alpha":   # a tile's p are taken against the running max of its time and never brought to the final one
        run = torch.cummax(s.view(M, nh, P, -1, KT).max(-1).values, -1).values          # M nh P nt
        w = torch.exp(s - run.repeat_interleave(KT, -1)) / e.sum(-1, keepdim=True)
    if mutant in ("natural_order", "no_xor"):
        perm = _v_permutation(Vh.shape[2], hd, mutant)                                   # hd kv
        Vp = torch.gather(Vh.transpose(2, 3), 3, perm[None, None].expand(M, nh, hd, -1)).transpose(2, 3)
        o = torch.einsum("mhpk,mhkd->mhpd", w, Vp)
    else:
        o = torch.einsum("mhpk,mhkd->mhpd", w, Vh)
    av = Vh.abs()
    A = torch.einsum("mhpk,mhkd->mhpd", w, av).max(-1).values
    R = o.abs().max(-1).values
    S = torch.einsum("mhpd,mhkd->mhpk", qh.abs(), Kh.abs()).max(-1).values / math.sqrt(hd)
    Ex = U * torch.einsum("mhpk,mhkd->mhpd", w * ((s - m).abs() + 2.0), av).max(-1).values
    n_acc = kv + 3 * nt + kv // 4 + 4 * nt + 2 + 2
    bound = 2.0 * ((U_BF16 * R if out_term else 0.0) + U_BF16 * A + (hd + 4) * U * S * (A + R) + Ex + n_acc * U * A)
    return o.permute(0, 2, 1, 3).reshape(M, P, C), bound


def row_error(got, ref, nh):
    """[M][P][C] x 2 -> max_d |got - ref| per (frame, head, row): [M][nh][P]"""
    M, P, C = ref.shape
    return (got.double() - ref).abs().view(M, P, nh, C // nh).max(-1).values.permute(0, 2, 1)


def xattn_restated(q, Kp, VpT, F, nh, rounded=True):
    """xattn_kernel in fp32: the key tiles in order, the online softmax with the running max, p summed in fp32 and rounded to bf16
    for the P.V product, o and the row sum rescaled by alpha, the final o * (1 / sum) rounded to bf16."""
    M, P, C = q.shape
    B, kv, _ = Kp.shape
    hd = C // nh
    KT = key_tile(hd)
    bidx = torch.arange(M) // F
    qh = q.view(M, P, nh, hd).permute(0, 2, 1, 3)
    Kh = Kp.view(B, kv, nh, hd).permute(0, 2, 1, 3)[bidx]
    Vh = VpT.view(B, nh, hd, kv).transpose(2, 3)[bidx]
    scale = torch.tensor(1.0 / math.sqrt(hd), dtype=torch.float32)
    o = torch.zeros(M, nh, P, hd)
    mx = torch.full((M, nh, P, 1), -float("inf"))
    ls = torch.zeros(M, nh, P, 1)
    for t in range(kv // KT):
        sc = torch.einsum("mhpd,mhkd->mhpk", qh, Kh[:, :, t * KT:(t + 1) * KT]) * scale
        mn = torch.maximum(mx, sc.max(-1, keepdim=True).values)
        alpha = torch.exp(mx - mn)
        mx = mn
        pe = torch.exp(sc - mn)
        ls = ls * alpha + pe.sum(-1, keepdim=True)
        o = o * alpha + torch.einsum("mhpk,mhkd->mhpd", bf16(pe), Vh[:, :, t * KT:(t + 1) * KT])
    o = o * (1.0 / ls)
    return (bf16(o) if rounded else o).permute(0, 2, 1, 3).reshape(M, P, C)


def xattn_einsum(q, Kp, VpT, F, nh):
    """independent formulation: torch.softmax over a per-trajectory einsum"""
    M, P, C = q.shape
    B, kv, _ = Kp.shape
    hd = C // nh
    out = torch.empty(M, P, C, dtype=torch.float64)
    for m in range(M):
        b = m // F
        for h in range(nh):
            ch = slice(h * hd, (h + 1) * hd)
            w = torch.softmax(q[m, :, ch].double() @ Kp[b, :, ch].double().T / math.sqrt(hd), -1)
            out[m, :, ch] = w @ VpT[b, ch].double().T
    return out
