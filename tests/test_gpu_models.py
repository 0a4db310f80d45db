"""Model-level parity on the MI355X (-m gpu): the HIP engine, through the Python mirror of the reference API
(which only calls the C ABI), against (a) the committed golden vectors = outputs of the REFERENCE classes and
(b) the CPU oracle on the same seeded inputs.

Bars (BASELINE.json north_star): VQ code indices bit-exact; decoded pixels and logits within 1e-3 (fp32
engine mode, absolute); the bf16 engine mode is compared with a bf16-sized tolerance that is written in each test.
"""
import json

import numpy as np
import pytest
import torch

from helpers import llama_fixture, oracle_llama, oracle_tokenizer, tokenizer_fixture, vq_near_tie_audit

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def make_tok(cfg, sd, ctx, enc="fp32", dec="fp32"):
    from ivideogpt_amd import CompressiveVQModel
    m = CompressiveVQModel(cfg, sd, encode_dtype=enc, decode_dtype=dec).to(DEV)
    if ctx != cfg["context_length"]:
        m.set_context_length(ctx)
    return m


def audit_indices(ids, ref_ids, what):
    bad = int((ids != ref_ids).sum())
    assert bad == 0, f"{what}: {bad} / {ref_ids.size} token ids differ from the reference"


@pytest.mark.parametrize("name", ["tok_mini64_ctx2.npz", "tok_mini64_ctx1.npz", "tok_mini256_ctx2.npz"])
def test_tokenize_bit_exact_and_detokenize_1e3(name):
    cfg, sd, ctx, px, g = tokenizer_fixture(name)
    m = make_tok(cfg, sd, ctx)
    ids, labels = m.tokenize(px.to(DEV), ctx)
    audit_indices(ids.cpu().numpy(), g["indices"], "tokenize")
    assert np.array_equal(labels.cpu().numpy(), g["labels"])
    pre = m.encode_context(px.to(DEV), ctx)
    assert torch.equal(pre, ids[:, :257 * ctx]), "encode_context must equal tokenize(...)[:, :257*ctx]"
    s = int(g["subsample"])
    rec = m.detokenize(torch.from_numpy(g["indices"]).to(DEV), ctx).cpu().numpy()[..., ::s, ::s]
    err = np.abs(rec - g["recon"]).max()
    assert err < 1e-3, f"decoded pixels: max abs err {err:.2e} vs reference"
    rec2 = m.detokenize(torch.from_numpy(g["indices_perturbed"]).to(DEV), ctx).cpu().numpy()[..., ::s, ::s]
    err2 = np.abs(rec2 - g["recon_perturbed"]).max()
    assert err2 < 1e-3, f"decoded pixels (perturbed / clamped ids): max abs err {err2:.2e}"


def test_groupnorm_apply_fused_and_separate_agree(monkeypatch):
    """The tokenizer with GroupNorm + SiLU applied inside the conv3x3 staging (default) and as a separate pass (IVG_GN_APPLY_FUSE=0):
    fp32 ids identical and equal to the reference's, fp32 pixels within 1e-3 of the reference either way."""
    cfg, sd, ctx, px, g = tokenizer_fixture("tok_mini64_ctx2.npz")
    out = {}
    monkeypatch.setenv("IVG_DEV", "1")   # the A/B switches are honoured only in development mode (csrc/switches.h)
    for fuse in ("1", "0"):
        monkeypatch.setenv("IVG_GN_APPLY_FUSE", fuse)
        m = make_tok(cfg, sd, ctx)
        ids, _ = m.tokenize(px.to(DEV), ctx)
        rec = m.detokenize(torch.from_numpy(g["indices"]).to(DEV), ctx)
        sub = int(g["subsample"])
        out[fuse] = (ids.cpu().numpy(), rec.cpu().numpy()[..., ::sub, ::sub])
        audit_indices(out[fuse][0], g["indices"], f"tokenize (IVG_GN_APPLY_FUSE={fuse})")
        assert np.abs(out[fuse][1] - g["recon"]).max() < 1e-3, f"IVG_GN_APPLY_FUSE={fuse}"
    assert np.array_equal(out["1"][0], out["0"][0])


def test_detokenize_bf16_mode_close():
    """bf16 decode path (the throughput mode).  bf16 storage cannot meet 1e-3 against an fp32 reference (bf16 eps is
    3.9e-3), so the bar is the reference's own bf16 path: the oracle under torch.autocast(bfloat16) -- how the reference
    runs detokenize in vp/ivideogpt_interface.py:180 and mbrl/video_predictor.py:269.  The engine's deviation from the
    fp32 reference must not exceed 1.5x the autocast oracle's (max and mean), and stay below 0.15 / 0.02 absolute."""
    cfg, sd, ctx, px, g = tokenizer_fixture("tok_mini64_ctx2.npz")
    m = make_tok(cfg, sd, ctx, dec="bf16")
    rec = m.detokenize(torch.from_numpy(g["indices"]).to(DEV), ctx).cpu().numpy()
    d = np.abs(rec - g["recon"])
    ora = oracle_tokenizer(cfg, sd, ctx)
    with torch.autocast("cpu", dtype=torch.bfloat16):
        auto = ora.detokenize(torch.from_numpy(g["indices"]), ctx).float().numpy()
    da = np.abs(auto - g["recon"])
    msg = f"bf16 decode: engine max {d.max():.3e} mean {d.mean():.3e}; reference-style autocast max {da.max():.3e} mean {da.mean():.3e}"
    print(msg)
    assert d.max() < max(1.5 * da.max(), 2e-2) and d.mean() < max(1.5 * da.mean(), 2e-3), msg
    assert d.max() < 0.15 and d.mean() < 0.02, msg


def test_detokenize_cache_paths():
    """return_cache / cache=... (mbrl/video_predictor.py:320-321): cached == uncached, also for F > 1."""
    cfg, sd, ctx, px, g = tokenizer_fixture("tok_mini64_ctx2.npz")
    m = make_tok(cfg, sd, ctx)
    ids = torch.from_numpy(g["indices"]).to(DEV)
    full = m.detokenize(ids, ctx)
    one = ids[:, :257 * ctx + 16]
    r1, cache = m.detokenize(one, ctx, return_cache=True)
    assert torch.equal(r1, full[:, :ctx + 1])
    r2 = m.detokenize(ids, ctx, cache=cache)
    assert torch.equal(r2, full)


def test_tokenize_batch_invariance_and_determinism():
    """rows of a batched call == the single-trajectory calls (what makes the multi-GPU batch shard exact)."""
    cfg, sd, ctx, px, g = tokenizer_fixture("tok_mini64_ctx2.npz")
    m = make_tok(cfg, sd, ctx)
    big = px.repeat(3, 1, 1, 1, 1)[:5].to(DEV)
    ids, _ = m.tokenize(big, ctx)
    ids_again, _ = m.tokenize(big, ctx)
    assert torch.equal(ids, ids_again)
    for b in range(5):
        one, _ = m.tokenize(big[b:b + 1], ctx)
        assert torch.equal(one[0], ids[b])
    rec = m.detokenize(ids, ctx)
    for b in (0, 4):
        assert torch.equal(m.detokenize(ids[b:b + 1], ctx)[0], rec[b])


def test_api_errors_mirror_reference():
    cfg, sd, ctx, px, g = tokenizer_fixture("tok_mini64_ctx2.npz")
    m = make_tok(cfg, sd, ctx)
    with pytest.raises(AssertionError):
        m.tokenize(px.to(DEV), ctx - 1)            # context_length mismatch (compressive_vq_model.py:166)
    with pytest.raises(AssertionError):
        m.detokenize(torch.zeros(1, 520, dtype=torch.int64), ctx)   # (L + 1 - 257*ctx) % 17 != 0 (:230)


# ------------------------------------------------------------------------------------------------ transformer
def make_llm(cfg, sd, dtype="fp32", lds_kb=0):
    from ivideogpt_amd import LlamaForCausalLM
    return LlamaForCausalLM(cfg, sd, dtype=dtype, decode_lds_kb=lds_kb).to(DEV)


# The two launch profiles of an engine (include/ivg.h, ivg_config.decode_lds_kb): 0 = one batch alone (a whole CU's LDS per decode-GEMM
# workgroup, third-generation kernel, non-temporal weights + warm-up) and 40 KiB = BATCHES IN FLIGHT -- the profile bench.py's lanes run
# and the headline number is produced with (second-generation 4-wave plans with another K partition / summation order, default-policy
# weight requests, no warm-up).  Every decode-path parity test below runs under both (round-5 review: "the arithmetic that produces
# the headline number is compared only with itself").
PROFILES = pytest.mark.parametrize("lds_kb", [0, 40], ids=["one_batch", "batches_in_flight"])


class ran_generation:
    """``with ran_generation(lds_kb, width): ...``: asserts WHICH decode-GEMM generation produced the tokens checked inside -- under the
    batches-in-flight budget the released widths' q/k/v, gate/up and down GEMMs must have left dgemm3.hip for the small-footprint plans
    of dgemm.hip (ivg_debug_counter)."""

    def __init__(self, lds_kb, released_width=True):
        self.kb, self.released = lds_kb, released_width

    def __enter__(self):
        from ivideogpt_amd import _lib
        self.l = _lib.load()
        self.g2, self.g3 = self.l.ivg_debug_counter(b"decode_gemm_gen2"), self.l.ivg_debug_counter(b"decode_gemm_gen3")
        return self

    def __exit__(self, *exc):
        if exc[0] is not None:
            return False
        d2 = self.l.ivg_debug_counter(b"decode_gemm_gen2") - self.g2
        d3 = self.l.ivg_debug_counter(b"decode_gemm_gen3") - self.g3
        assert d2 + d3 > 0, "no decode GEMM ran"
        if self.kb and self.released:
            assert d2 > 3 * d3, f"batches-in-flight budget: {d2} second-generation vs {d3} third-generation launches -- the small-footprint plans did not run"
        if not self.kb and self.released:
            assert d3 > d2, f"one-batch profile: {d3} third-generation vs {d2} second-generation launches"
        return False


@PROFILES
@pytest.mark.parametrize("name", ["llama_tiny_ctx2_free.npz", "llama_tiny_ctx1_free.npz"])
def test_llama_logits_and_greedy_rollout(name, lds_kb):
    cfg, sd, g = llama_fixture(name)
    m = make_llm(cfg, sd, lds_kb=lds_kb)
    lg = m.logits(torch.from_numpy(g["teacher_ids"]).to(DEV)).cpu().numpy()
    e1 = np.abs(lg[:, -2:] - g["teacher_logits_last"]).max()
    e2 = np.abs(lg[:, ::37, ::101] - g["teacher_logits_sub"]).max()
    assert max(e1, e2) < 1e-3, f"teacher-forced logits: max abs err {max(e1, e2):.2e}"
    prompt = torch.from_numpy(g["prompt"]).to(DEV)
    out = m.generate(prompt, do_sample=False, max_new_tokens=g["greedy"].shape[1] - prompt.shape[1]).cpu().numpy()
    assert np.array_equal(out, g["greedy"]), f"{(out != g['greedy']).sum()} greedy tokens differ from HF generate"


@PROFILES
@pytest.mark.parametrize("name", ["llama_tiny_ctx2_act.npz", "llama_tiny_ctx1_act.npz"])
def test_action_conditioned_greedy_matches_reference(name, lds_kb):
    from ivideogpt_amd import HeadModelWithAction, LlamaForCausalLM
    cfg, sd, g = llama_fixture(name)
    ctx, adim = int(g["ctx"]), int(g["action_dim"])
    prompt, action = torch.from_numpy(g["prompt"]).to(DEV), torch.from_numpy(g["action"]).to(DEV)
    head = HeadModelWithAction(LlamaForCausalLM(cfg, None, dtype="fp32", decode_lds_kb=lds_kb), adim, 257 * ctx - 1, 16, ctx, action.shape[1])
    head.load_state_dict(sd, strict=True)
    head.to(DEV)
    n_new = g["greedy"].shape[1] - prompt.shape[1]
    out = head.generate(prompt, do_sample=False, max_new_tokens=n_new, action=action).cpu().numpy()
    assert np.array_equal(out, g["greedy"]), f"{(out != g['greedy']).sum()} tokens differ from HeadModelWithAction.generate"
    # teacher-forced logits of the finished sequence vs the reference's HeadModelWithAction.forward (action_model.py:154-185)
    lg = head.logits(torch.from_numpy(g["greedy"]).to(DEV), action).cpu().numpy()
    err = max(np.abs(lg[:, -2:] - g["forward_logits_last"]).max(), np.abs(lg[:, ::37, ::101] - g["forward_logits_sub"]).max())
    assert err < 1e-3, f"forward logits with actions: max abs err {err:.2e}"


@PROFILES
def test_sampled_rollout_matches_oracle_with_same_uniforms(lds_kb):
    from oracle.llama import generate_cached
    cfg, sd, g = llama_fixture("llama_tiny_ctx2_free.npz")
    m = make_llm(cfg, sd, lds_kb=lds_kb)
    prompt = torch.from_numpy(g["prompt"])
    n_new = 50
    u = torch.rand(prompt.shape[0], n_new, generator=torch.Generator().manual_seed(1))
    out = m.generate(prompt.to(DEV), do_sample=True, top_k=100, max_new_tokens=n_new, uniforms=u.to(DEV)).cpu()
    ref = generate_cached(oracle_llama(cfg, sd), prompt, n_new, top_k=100, uniforms=u)
    assert torch.equal(out, ref), f"{(out != ref).sum().item()} sampled tokens differ"


def test_llama_bf16_mode_close():
    """bf16 transformer (throughput mode): bar = the same model evaluated in bf16 by plain PyTorch on the CPU (weights
    and activations in bfloat16, as HF runs it): engine deviation from the fp32 reference <= 1.5x that, and < 0.25 abs
    at a logit scale of ~12."""
    cfg, sd, g = llama_fixture("llama_tiny_ctx2_free.npz")
    m = make_llm(cfg, sd, "bf16")
    ids = torch.from_numpy(g["teacher_ids"])
    lg = m.logits(ids.to(DEV)).cpu().numpy()
    e = np.abs(lg[:, -2:] - g["teacher_logits_last"]).max()
    sd16 = {k: v.to(torch.bfloat16) for k, v in sd.items()}
    ora16 = oracle_llama(cfg, sd16)
    ora16.cos, ora16.sin = ora16.cos.to(torch.bfloat16), ora16.sin.to(torch.bfloat16)
    ref16 = ora16.logits(ids)[:, -2:].float().numpy()
    e16 = np.abs(ref16 - g["teacher_logits_last"]).max()
    msg = f"bf16 logits: engine max abs err {e:.3e}; torch-bf16 reference max abs err {e16:.3e}"
    print(msg)
    assert e < max(1.5 * e16, 5e-2) and e < 0.25, msg


def test_generate_graph_replay_equals_eager(monkeypatch):
    """the captured per-token hipGraph must give the same tokens as eager launches"""
    cfg, sd, g = llama_fixture("llama_tiny_ctx1_free.npz")
    prompt = torch.from_numpy(g["prompt"]).to(DEV)
    a = make_llm(cfg, sd).generate(prompt, do_sample=False, max_new_tokens=40)
    monkeypatch.setenv("IVG_GRAPH", "1")
    b = make_llm(cfg, sd).generate(prompt, do_sample=False, max_new_tokens=40)
    assert torch.equal(a, b)


def test_generate_batch_of_40_rows_matches_oracle():
    """B = 40 rows (2.5 row tiles: ragged last tile of every decode GEMM), sampled with explicit uniforms: rows match the oracle."""
    from oracle.llama import generate_cached
    cfg, sd, g = llama_fixture("llama_tiny_ctx1_free.npz")
    gen = torch.Generator().manual_seed(9)
    prompt = torch.randint(0, 8192, (40, 257), generator=gen)
    prompt[:, -1] = cfg["vocab_size"] - 1
    u = torch.rand(40, 36, generator=gen)
    a = make_llm(cfg, sd).generate(prompt.to(DEV), do_sample=True, top_k=100, max_new_tokens=36, uniforms=u.to(DEV)).cpu()
    rows = [0, 15, 16, 31, 32, 39]
    ref = generate_cached(oracle_llama(cfg, sd), prompt[rows], 36, top_k=100, uniforms=u[rows])
    assert torch.equal(a[rows], ref)


@pytest.mark.parametrize("temperature", [0.7, 1.3])
def test_generate_with_temperature_matches_oracle(temperature):
    """``generate(..., temperature=T)`` (the argument the reference forwards to HF: inference/predict.py:61,
    action_model.py:61,89,104): sampled rollouts equal the oracle's at the same uniforms, differ from T = 1, and the engine goes back
    to T = 1 on the next call; action-conditioned path included."""
    from oracle.llama import generate_cached
    cfg, sd, g = llama_fixture("llama_tiny_ctx1_free.npz")
    gen = torch.Generator().manual_seed(int(temperature * 10))
    prompt = torch.randint(0, 8192, (6, 257), generator=gen)
    prompt[:, -1] = cfg["vocab_size"] - 1
    u = torch.rand(6, 50, generator=gen)
    llm = make_llm(cfg, sd)
    ref1 = generate_cached(oracle_llama(cfg, sd), prompt, 50, top_k=100, uniforms=u)
    refT = generate_cached(oracle_llama(cfg, sd), prompt, 50, top_k=100, uniforms=u, temperature=temperature)
    assert not torch.equal(ref1, refT)
    outT = llm.generate(prompt.to(DEV), do_sample=True, temperature=temperature, top_k=100, max_new_tokens=50, uniforms=u.to(DEV)).cpu()
    assert torch.equal(outT, refT), f"temperature {temperature}: {(outT != refT).sum().item()} tokens differ"
    out1 = llm.generate(prompt.to(DEV), do_sample=True, top_k=100, max_new_tokens=50, uniforms=u.to(DEV)).cpu()
    assert torch.equal(out1, ref1), "temperature back at 1.0"
    with pytest.raises(ValueError):
        llm.generate(prompt.to(DEV), do_sample=True, temperature=0.0, top_k=100, max_new_tokens=4)


@PROFILES
@pytest.mark.parametrize("width", ["small", "medium"])
def test_fp32_decode_rows_do_not_depend_on_batch_mates(width, lds_kb):
    """fp32 (parity) mode at the released widths: a trajectory's sampled tokens in a 64-row batch equal those of its 16-row
    shard and of the row alone.  The decode GEMMs' K partition is a function of (K, N, dtype) only; a tile the batch size asks
    for that the wave count cannot hold is clamped, never answered by falling back to the first-generation kernel (different
    summation order) for some batch sizes only (fp32 lm_head / q,k,v at M = 64 vs M <= 32)."""
    from ivideogpt_amd import weights as W
    cfg = dict(W.LLAMA_SMALL if width == "small" else W.LLAMA_MEDIUM)
    cfg["num_hidden_layers"] = 2
    sd = W.random_llama_state_dict(cfg, 47)
    g = torch.Generator().manual_seed(11)
    prompt = torch.randint(0, 16384, (64, 40), generator=g)
    u = torch.rand(64, 20, generator=g)
    m = make_llm(cfg, sd, lds_kb=lds_kb)
    with ran_generation(lds_kb, released_width=(width == "small")):
        full = m.generate(prompt.to(DEV), do_sample=True, top_k=100, max_new_tokens=20, uniforms=u.to(DEV)).cpu()
    for rows in (slice(0, 16), slice(16, 48), slice(63, 64), slice(5, 6)):
        part = m.generate(prompt[rows].to(DEV), do_sample=True, top_k=100, max_new_tokens=20, uniforms=u[rows].to(DEV)).cpu()
        assert torch.equal(part, full[rows]), f"{width}: rows {rows} differ between the 64-row batch and the shard"


# ------------------------------------------------------------------------------------------------ full width
def test_full_width_64_tokenizer_vs_oracle():
    """ctx_vae64 shapes (114 M parameters), one trajectory: HIP fp32 vs the CPU oracle run here."""
    from ivideogpt_amd import weights as W
    cfg = W.tokenizer_config(**W.CTX_VAE64)                        # 8192 + 8192 codes: the released vocabulary
    sd = W.random_tokenizer_state_dict(cfg, 31, codebook_std=0.4)
    px = torch.randint(0, 256, (1, 4, 3, 64, 64), generator=torch.Generator().manual_seed(2)).float() / 255
    ora = oracle_tokenizer(cfg, sd, 2)
    ids_ref, _ = ora.tokenize(px, 2)
    m = make_tok(cfg, sd, 2)
    ids, _ = m.tokenize(px.to(DEV), 2)
    vq_near_tie_audit(ora, px, 2, ids, ids_ref, what="ctx_vae64 full width, N(0, 0.4) codebooks")   # SURVEY 7 (iii); tests/test_gpu_vocab.py has the 16-clip runs
    err = (m.detokenize(ids, 2).cpu() - ora.detokenize(ids.cpu(), 2)).abs().max().item()
    assert err < 1e-3, f"full-width decode max abs err {err:.2e}"


@PROFILES
def test_full_width_llama_small_logits_vs_oracle(lds_kb):
    """12-layer small Llama at full width: teacher-forced logits (prompt pass) AND the logits the DECODE path leaves -- the same 300
    tokens fed as a 280-token prompt plus 20 forced single-token steps is not expressible through generate, so the decode path is held
    to the oracle through its tokens: a greedy and a sampled continuation of 24 tokens, near-ties of the inverse CDF excepted."""
    from oracle.llama import generate_cached
    from helpers import assert_sampled_rollout_matches
    from ivideogpt_amd import weights as W
    cfg = dict(W.LLAMA_SMALL)
    sd = W.random_llama_state_dict(cfg, 41)
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(0, 16386, (2, 300), generator=g)
    ora = oracle_llama(cfg, sd)
    ref = ora.logits(ids)
    m = make_llm(cfg, sd, lds_kb=lds_kb)
    lg = m.logits(ids.to(DEV)).cpu()
    err = (lg - ref).abs().max().item()
    assert err < 1e-3, f"12-layer logits max abs err {err:.2e} (scale {ref.abs().max():.1f})"
    n_new = 24
    u = torch.rand(2, n_new, generator=g)
    with ran_generation(lds_kb):
        out_g = m.generate(ids.to(DEV), do_sample=False, max_new_tokens=n_new).cpu()
        out_s = m.generate(ids.to(DEV), do_sample=True, top_k=100, max_new_tokens=n_new, uniforms=u.to(DEV)).cpu()
    assert torch.equal(out_g, generate_cached(ora, ids, n_new)), "greedy continuation differs from the oracle"
    assert_sampled_rollout_matches(out_s, generate_cached(ora, ids, n_new, top_k=100, uniforms=u), ora, u, 100, ids.shape[1], what=f"small, lds_kb={lds_kb}")


@pytest.mark.parametrize("L", [300, 64, 65, 514])
def test_flash_prefill_matches_three_kernel_path(monkeypatch, L):
    """bf16 prompt attention in one kernel (online softmax) vs score GEMM + row softmax + P.V GEMM: both are bf16 schedules
    of the same attention, so against the fp32 CPU oracle the one-pass kernel may not be worse than 1.25x the three-kernel
    path (+1e-2), and the two agree with each other within bf16 noise; ragged prompt lengths (tail tiles) included."""
    from ivideogpt_amd import weights as W
    cfg = dict(W.LLAMA_SMALL)
    cfg["num_hidden_layers"] = 4                      # head_dim 64 as the released models; 4 layers keep the CPU oracle quick
    sd = W.random_llama_state_dict(cfg, 43)
    ids = torch.randint(0, cfg["vocab_size"], (3, L), generator=torch.Generator().manual_seed(L))
    ref = oracle_llama(cfg, sd).logits(ids)
    monkeypatch.setenv("IVG_DEV", "1")
    monkeypatch.setenv("IVG_FLASH_PREFILL", "0")
    lg3 = make_llm(cfg, sd, "bf16").logits(ids.to(DEV)).cpu()
    monkeypatch.setenv("IVG_FLASH_PREFILL", "1")
    lgf = make_llm(cfg, sd, "bf16").logits(ids.to(DEV)).cpu()
    e3, ef, d = (lg3 - ref).abs().max().item(), (lgf - ref).abs().max().item(), (lgf - lg3).abs().max().item()
    msg = f"L={L}: max abs err vs fp32 oracle: three-kernel {e3:.3e}, one-pass {ef:.3e}; between them {d:.3e} (logit scale {ref.abs().max():.1f})"
    print(msg)
    assert torch.isfinite(lgf).all() and ef <= 1.25 * e3 + 1e-2 and d <= 2 * e3 + 1e-2, msg


def test_full_width_256_tokenizer_vs_oracle():
    """ctx_vae256 shapes (310 M parameters, five levels up to 768 channels, 256 x 256 frames), one trajectory with two context
    frames and one future frame: HIP fp32 vs the CPU oracle run here -- ids bit-exact, decoded pixels within 1e-3."""
    from ivideogpt_amd import weights as W
    cfg = W.tokenizer_config(**W.CTX_VAE256)                       # 8192 + 8192 codes: the released vocabulary
    sd = W.random_tokenizer_state_dict(cfg, 33, codebook_std=0.4)
    px = torch.randint(0, 256, (1, 3, 3, 256, 256), generator=torch.Generator().manual_seed(4)).float() / 255
    ora = oracle_tokenizer(cfg, sd, 2)
    ids_ref, _ = ora.tokenize(px, 2)
    m = make_tok(cfg, sd, 2)
    ids, _ = m.tokenize(px.to(DEV), 2)
    vq_near_tie_audit(ora, px, 2, ids, ids_ref, what="ctx_vae256 full width, N(0, 0.4) codebooks")
    ids_ref = ids.cpu()
    err = (m.detokenize(ids, 2).cpu() - ora.detokenize(ids_ref, 2)).abs().max().item()
    assert err < 1e-3, f"256x256 full-width decode max abs err {err:.2e}"
    # the benchmarked arithmetic (bf16 decode) at this width: finite and close to the fp32 decode (bf16-sized tolerance)
    m16 = make_tok(cfg, sd, 2, dec="bf16")
    d16 = m16.detokenize(ids, 2).cpu()
    assert torch.isfinite(d16).all()
    ref = ora.detokenize(ids_ref, 2)
    rel = (d16 - ref).abs().mean().item() / ref.abs().mean().item()
    assert rel < 3e-2, f"bf16 decode mean relative deviation {rel:.3e}"


@PROFILES
def test_full_width_llama_medium_logits_vs_oracle(lds_kb):
    """config_medium (24 layers, hidden 1024, 16 heads; 436 M parameters): teacher-forced logits vs the CPU oracle."""
    from ivideogpt_amd import weights as W
    cfg = dict(W.LLAMA_MEDIUM)
    sd = W.random_llama_state_dict(cfg, 45)
    ids = torch.randint(0, cfg["vocab_size"], (1, 160), generator=torch.Generator().manual_seed(7))
    ref = oracle_llama(cfg, sd).logits(ids)
    lg = make_llm(cfg, sd, lds_kb=lds_kb).logits(ids.to(DEV)).cpu()
    err = (lg - ref).abs().max().item()
    assert err < 1e-3, f"24-layer logits max abs err {err:.2e} (scale {ref.abs().max():.1f})"


# ------------------------------------------------------------------------------------------------ the reference's own bf16 path
def test_bf16_mode_against_reference_autocast_vectors():
    """tests/golden/bf16_mini64_ctx2.npz holds what the REFERENCE classes produce under ``torch.autocast(dtype=bfloat16)`` -- the
    way vp/ivideogpt_interface.py:180 and mbrl/video_predictor.py:269 run them -- for the tokens / ids of the fp32 fixtures.  The
    engine's bf16 mode (the benchmarked arithmetic) against those vectors, absolute tolerances:
      decoded pixels  max |d| < 0.15, mean |d| < 0.012   (the reference's autocast path itself sits 7.7e-2 / 7.9e-3 from its fp32 path)
      logits          max |d| < 0.30 at a logit scale of 12  (autocast is 0.17 from fp32, HF with bf16 weights 0.98)
    and the engine may not be further from the fp32 reference than the reference's own bf16 paths are."""
    from helpers import load_golden
    gb = load_golden("bf16_mini64_ctx2.npz")
    cfg, sd, ctx, px, g = tokenizer_fixture("tok_mini64_ctx2.npz")
    m = make_tok(cfg, sd, ctx, dec="bf16")
    rec = m.detokenize(torch.from_numpy(g["indices"]).to(DEV), ctx).cpu().numpy()
    d = np.abs(rec - gb["pixels_autocast"])
    d32 = np.abs(rec - g["recon"])
    ref_dev = gb["autocast_pixel_dev"]
    msg = (f"bf16 decode vs reference autocast: max {d.max():.3e} mean {d.mean():.3e}; vs reference fp32: max {d32.max():.3e} mean "
           f"{d32.mean():.3e} (reference autocast vs its fp32: max {ref_dev[0]:.3e} mean {ref_dev[1]:.3e})")
    print(msg)
    assert d.max() < 0.15 and d.mean() < 0.012, msg
    assert d32.max() <= 1.25 * ref_dev[0] and d32.mean() <= 1.25 * ref_dev[1], msg
    lcfg, lsd, gl = llama_fixture("llama_tiny_ctx2_free.npz")
    lg = make_llm(lcfg, lsd, "bf16").logits(torch.from_numpy(gl["teacher_ids"]).to(DEV)).cpu().numpy()
    e_ac = max(np.abs(lg[:, -2:] - gb["logits_autocast_last"]).max(), np.abs(lg[:, ::37, ::101] - gb["logits_autocast_sub"]).max())
    e_32 = max(np.abs(lg[:, -2:] - gl["teacher_logits_last"]).max(), np.abs(lg[:, ::37, ::101] - gl["teacher_logits_sub"]).max())
    msg = (f"bf16 logits vs reference autocast: max {e_ac:.3e}; vs reference fp32: {e_32:.3e} (reference autocast vs fp32 {gb['logits_dev'][0]:.3e}, "
           f"HF bf16 weights vs fp32 {gb['logits_dev'][1]:.3e})")
    print(msg)
    assert e_ac < 0.30 and e_32 <= 1.25 * gb["logits_dev"][0], msg


# ------------------------------------------------------------------------------------------------ eval forward (labels -> loss)
def test_eval_forward_matches_reference_loss():
    """``model(input_ids, labels[, action])`` of the eval loop (train_gpt.py:356-376) against the REFERENCE's numbers
    (tests/golden/llama_tiny_ctx2_eval.npz): HF shifted cross-entropy of LlamaForCausalLM; HeadModelWithAction.forward with
    reward head and action reconstruction (loss = CE + 0.5 * MSE, reward_pred (B, F, 1)) -- computed without a logits tensor."""
    from helpers import load_golden
    from ivideogpt_amd import HeadModelWithAction, LlamaForCausalLM, weights as W
    g = load_golden("llama_tiny_ctx2_eval.npz")
    cfg = json.loads(str(g["config"]))
    seed, adim, ctx, F = int(g["seed"]), int(g["action_dim"]), int(g["ctx"]), int(g["n_future"])
    ids, labels = torch.from_numpy(g["ids"]).to(DEV), torch.from_numpy(g["labels"]).to(DEV)
    free = LlamaForCausalLM(cfg, W.random_llama_state_dict(cfg, seed), dtype="fp32").to(DEV)
    out = free(input_ids=ids, labels=labels)
    assert abs(out.loss.item() - float(g["loss_free"])) < 1e-3, (out.loss.item(), float(g["loss_free"]))
    # per-position losses against the logits path of the same engine
    lg = free.logits(ids)
    nll = torch.nn.functional.cross_entropy(lg[:, :-1].reshape(-1, lg.shape[-1]), labels[:, 1:].reshape(-1), ignore_index=-100,
                                            reduction="none").view(ids.shape[0], -1)
    assert (out.token_nll[:, :-1] - nll).abs().max().item() < 1e-4 and out.token_nll[:, -1].abs().max().item() == 0
    assert (out.sample_perplexity - torch.exp(out.sample_loss)).abs().max().item() < 1e-3
    sda = W.random_llama_state_dict(cfg, seed + 1, action_dim=adim, reward_prediction=True, action_recon=True)
    head = HeadModelWithAction(LlamaForCausalLM(cfg, None, dtype="fp32"), adim, 257 * ctx - 1, 16, ctx, ctx + F, reward_prediction=True,
                               action_recon=float(g["action_recon_weight"]))
    head.load_state_dict(sda, strict=True)
    head.to(DEV)
    action = torch.from_numpy(g["action"]).to(DEV)
    x, reward_pred = head(input_ids=ids, labels=labels, action=action)
    assert abs(x.loss.item() - float(g["loss_act"])) < 1e-3, (x.loss.item(), float(g["loss_act"]))
    assert abs(head.action_recon_loss.item() - float(g["action_recon_loss"])) < 1e-4
    assert reward_pred.shape == g["reward_pred"].shape and np.abs(reward_pred.cpu().numpy() - g["reward_pred"]).max() < 1e-3


def test_eval_forward_full_width_loss_vs_oracle():
    """12-layer small Llama, L = 751 (2 context + 14 future frames), 3 trajectories: loss / per-sample loss vs the oracle's
    eval_forward.  The 2253 rows fit in ONE 4096-row lm_head chunk of the fused cross-entropy: several chunks are exercised by
    tests/test_gpu_prefill.py test_eval_cross_entropy_across_row_chunks_vs_fp64."""
    from oracle.llama import eval_forward
    from ivideogpt_amd import weights as W
    cfg = dict(W.LLAMA_SMALL)
    sd = W.random_llama_state_dict(cfg, 47)
    g = torch.Generator().manual_seed(11)
    ids = torch.randint(0, cfg["vocab_size"], (3, 751), generator=g)
    labels = ids.clone()
    labels[:, :514] = -100
    ref = eval_forward(oracle_llama(cfg, sd), ids, labels)
    out = make_llm(cfg, sd)(input_ids=ids.to(DEV), labels=labels.to(DEV))
    assert abs(out.loss.item() - ref["loss"].item()) < 1e-3
    assert (out.sample_loss.cpu() - ref["sample_loss"]).abs().max().item() < 1e-3
    assert (out.token_nll.cpu() - ref["token_nll"]).abs().max().item() < 2e-3


# ------------------------------------------------------------------------------------------------ BASELINE config 5: medium decode path
@PROFILES
def test_medium_llama_decode_path_vs_oracle(lds_kb):
    """ivideogpt-oxe-64-act-free-medium (24 layers, hidden 1024, 16 heads, intermediate 4096): the DECODE path -- skinny / decode
    GEMMs at K = 1024 / 4096, decode attention with 16 heads -- through ``generate`` from a 514-token prompt, 2 rows, 48 new
    tokens, greedy and sampled with explicit uniforms, fp32 mode: token-identical to oracle.llama.generate_cached."""
    from oracle.llama import generate_cached
    from ivideogpt_amd import weights as W
    cfg = dict(W.LLAMA_MEDIUM)
    sd = W.random_llama_state_dict(cfg, 49)
    g = torch.Generator().manual_seed(13)
    prompt = torch.randint(0, 8192, (2, 514), generator=g)
    prompt[:, 256] = cfg["vocab_size"] - 2
    prompt[:, -1] = cfg["vocab_size"] - 1
    n_new = 48
    u = torch.rand(2, n_new, generator=g)
    ora = oracle_llama(cfg, sd)
    m = make_llm(cfg, sd, lds_kb=lds_kb)
    with ran_generation(lds_kb, released_width=False):   # (medium: o-proj / gate-up sit on the second generation under either budget)
        out_g = m.generate(prompt.to(DEV), do_sample=False, max_new_tokens=n_new).cpu()
    ref_g = generate_cached(ora, prompt, n_new)
    assert torch.equal(out_g, ref_g), f"greedy: {(out_g != ref_g).sum().item()} of {2 * n_new} tokens differ from the oracle"
    out_s = m.generate(prompt.to(DEV), do_sample=True, top_k=100, max_new_tokens=n_new, uniforms=u.to(DEV)).cpu()
    ref_s = generate_cached(ora, prompt, n_new, top_k=100, uniforms=u)
    assert torch.equal(out_s, ref_s), f"sampled: {(out_s != ref_s).sum().item()} of {2 * n_new} tokens differ from the oracle"


def test_sampler_survives_nan_logits():
    """A row of NaN (or -inf) logits must decide an in-range token (0) instead of writing a garbage id / gathering an embedding
    out of bounds inside a replayed graph."""
    import ctypes as C
    from ivideogpt_amd import _lib
    l = _lib.load()
    B, V = 4, 16386
    lg = torch.randn(B, V, device=DEV)
    lg[1] = float("nan")
    lg[2] = float("-inf")
    u = torch.rand(B, device=DEV)
    out = torch.full((B,), -7, dtype=torch.int64, device=DEV)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for uni in (u, None):
        assert l.ivg_op_sample(C.c_void_p(lg.data_ptr()), B, V, 100, 1.0, C.c_void_p(uni.data_ptr()) if uni is not None else None,
                               C.c_void_p(out.data_ptr()), st) == 0
        o = out.cpu()
        assert ((o >= 0) & (o < V)).all(), o.tolist()
        assert o[1].item() == 0 and o[2].item() == 0
