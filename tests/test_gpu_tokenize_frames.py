"""Tokens of observed frames against the encoder's kept context (include/ivg.h ivg_enc_cache_create, ivg_encode_context_cached,
ivg_tokenize_frames, ivg_enc_cache_select; CompressiveVQModel.encode_context(return_cache=True) / tokenize_frames / EncodeCache) on the
MI355X: the ids against the indices the reference's own classes wrote into the golden fixtures (0 differing ids, fp32 encoder), frame
and batch independence, the strided output, which trunks ran (ivg_debug_counter), select, the context length, every refusal through the
C ABI, and the bf16 encoder against its own tokenize."""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import tokenizer_fixture

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
OK, INVALID, CAPACITY = 0, -1, -4
SENT = -4242
FIXTURES = ["tok_mini64_ctx2", "tok_mini64_ctx1", "tok_mini256_ctx2"]


def lib():
    from ivideogpt_amd import _lib
    return _lib.load()


def _p(t):
    from ivideogpt_amd.engine import _ptr
    return _ptr(t)


def counters():
    return tuple(lib().ivg_debug_counter(n) for n in (b"enc_plain_images", b"enc_cond_images", b"enc_kv_projections"))


_models = {}


def model_of(name, dtype="fp32"):
    """(tokenizer on the GPU, ctx, pixels (B, T, 3, H, W) on the GPU, golden arrays), built once per fixture and encode dtype."""
    from ivideogpt_amd import CompressiveVQModel
    if (name, dtype) not in _models:
        cfg, sd, ctx, px, g = tokenizer_fixture(name + ".npz")
        tok = CompressiveVQModel(cfg, sd, encode_dtype=dtype, decode_dtype="fp32").to(DEV)
        if ctx != cfg["context_length"]:
            tok.set_context_length(ctx)
        _models[(name, dtype)] = (tok, ctx, px.to(DEV), g)
    return _models[(name, dtype)]


def cols(ctx, i):
    from ivideogpt_amd.vq_model import frame_token_columns
    return frame_token_columns(ctx, i)


# ------------------------------------------------------------------------------------------------ against the reference
@pytest.mark.parametrize("name", FIXTURES)
def test_ids_equal_the_reference_indices(name):
    tok, ctx, px, g = model_of(name)
    ref = torch.from_numpy(g["indices"]).to(DEV)
    F = px.shape[1] - ctx
    sdf = tok.num_vq_embeddings + tok.num_dyn_embeddings + 1
    plain = tok.encode_context(px, ctx)
    ids0, cache = tok.encode_context(px, ctx, return_cache=True)
    assert torch.equal(ids0, plain), "encode_context(return_cache=True) returned other ids"
    assert torch.equal(ids0, ref[:, :257 * ctx])
    for n in sorted({1, F}):
        ids = tok.tokenize_frames(px[:, ctx:ctx + n], cache)
        assert ids.shape == (px.shape[0], 17 * n) and ids.dtype == torch.int64
        for i in range(n):
            a, b = cols(ctx, i)
            diff = (ids[:, 17 * i:17 * i + 16] != ref[:, a:b]).sum().item()
            print(f"{name}: n = {n}, frame {i}: {diff} differing ids of {ids.shape[0] * 16}")
            assert diff == 0
        assert (ids[:, 16::17] == sdf).all(), "sdf columns"


def test_frames_are_independent():
    tok, ctx, px, g = model_of("tok_mini64_ctx2")
    _, cache = tok.encode_context(px, ctx, return_cache=True)
    both = tok.tokenize_frames(px[:, ctx:ctx + 2], cache)
    one = [tok.tokenize_frames(px[:, ctx + i:ctx + i + 1], cache) for i in range(2)]
    assert torch.equal(both, torch.cat(one, 1)), "two calls of n = 1 differ from one call of n = 2"
    swapped = tok.tokenize_frames(px[:, [ctx + 1, ctx]], cache)
    assert torch.equal(swapped[:, :17], both[:, 17:]) and torch.equal(swapped[:, 17:], both[:, :17]), "a frame's ids depend on its position"


def test_rows_do_not_depend_on_the_batch():
    tok, ctx, px, g = model_of("tok_mini64_ctx2")
    px5 = px.repeat(3, 1, 1, 1, 1)[:5].contiguous()
    ids5, cache5 = tok.encode_context(px5, ctx, return_cache=True)
    dyn5 = tok.tokenize_frames(px5[:, ctx:], cache5)
    for b in range(5):
        ids1, cache1 = tok.encode_context(px5[b:b + 1], ctx, return_cache=True)
        assert torch.equal(ids1, ids5[b:b + 1])
        assert torch.equal(tok.tokenize_frames(px5[b:b + 1, ctx:], cache1), dyn5[b:b + 1]), f"row {b} differs from its B = 1 call"


def raw_tokenize_frames(eng, frames, cache, n=None, B=None, stride_extra=3, dtype=None):
    """ivg_tokenize_frames through the C ABI into a sentinel-filled (B, 17 n + stride_extra) matrix -> (status, matrix)."""
    from ivideogpt_amd.packing import dtype_code
    rows, nn = frames.shape[0], (frames.shape[1] if n is None else n)
    out = torch.full((rows, 17 * max(nn, 1) + stride_extra), SENT, dtype=torch.int64, device=DEV)
    with eng.stream() as s:
        rc = eng.lib.ivg_tokenize_frames(eng.h, _p(frames), dtype_code(frames.dtype) if dtype is None else dtype, rows if B is None else B, nn, cache,
                                         _p(out), out.stride(0), s)
    torch.cuda.synchronize()
    return rc, out


def test_strided_output_and_counters():
    tok, ctx, px, g = model_of("tok_mini64_ctx2")
    ids0, cache = tok.encode_context(px, ctx, return_cache=True)
    dense = tok.tokenize_frames(px[:, ctx:], cache)
    B, n = px.shape[0], px.shape[1] - ctx
    c0 = counters()
    rc, out = raw_tokenize_frames(tok._engine, px[:, ctx:].contiguous(), cache.handle)
    c1 = counters()
    assert rc == OK
    assert torch.equal(out[:, :17 * n], dense) and (out[:, 17 * n:] == SENT).all(), "columns >= 17 n were touched"
    assert (c1[0] - c0[0], c1[1] - c0[1], c1[2] - c0[2]) == (0, B * n, 0), "tokenize_frames ran the plain encoder or a projection"
    # the fill: ctx images per row through the plain trunk, one projection per site; the plain entry: no projection at all
    from ivideogpt_amd.weights import cross_attention_sites
    sites = len(cross_attention_sites(tok.config)[0])
    c0 = counters()
    tok.encode_context(px, ctx, return_cache=True)
    c1 = counters()
    assert (c1[0] - c0[0], c1[1] - c0[1], c1[2] - c0[2]) == (B * ctx, 0, sites)
    tok.encode_context(px, ctx)
    c2 = counters()
    assert (c2[0] - c1[0], c2[1] - c1[1], c2[2] - c1[2]) == (B * ctx, 0, 0), "ivg_encode_context launches what it launched before"


def test_select_gathers_rows_and_leaves_the_source():
    tok, ctx, px, g = model_of("tok_mini64_ctx2")
    tok._ensure(5, px.shape[1])             # room for the four rows below
    _, cache = tok.encode_context(px, ctx, return_cache=True)
    frames = px[:, ctx:]
    dyn = tok.tokenize_frames(frames, cache)
    parents = [1, 1, 0, 1]  # a duplicate, growth from 2 rows to 4; [1, 1] below drops row 0
    for p in (parents, [1, 1]):
        sel = cache.select(p)
        assert sel.B == len(p)
        assert torch.equal(tok.tokenize_frames(frames[p].contiguous(), sel), dyn[p]), f"parents {p}"
    assert torch.equal(tok.tokenize_frames(frames, cache), dyn), "the source cache changed"
    with pytest.raises(ValueError):
        cache.select([0, 2])
    with pytest.raises(ValueError):
        cache.select(list(range(2)) * 40)   # more rows than the engine's batch


def test_context_length():
    from ivideogpt_amd import CompressiveVQModel
    cfg, sd, ctx, px, g = tokenizer_fixture("tok_mini64_ctx2.npz")
    tok = CompressiveVQModel(cfg, sd, encode_dtype="fp32", decode_dtype="fp32").to(DEV)
    px = px.to(DEV)
    tok.set_context_length(1)
    clip = px[:, 1:]                        # one context frame, two future frames
    full, _ = tok.tokenize(clip, 1)
    ids0, cache = tok.encode_context(clip, 1, return_cache=True)
    dyn = tok.tokenize_frames(clip[:, 1:], cache)
    assert torch.equal(ids0, full[:, :257])
    assert torch.equal(dyn[:, :-1], full[:, 257:]), "ctx-2 model under set_context_length(1)"
    tok.set_context_length(2)
    with pytest.raises(AssertionError):
        tok.tokenize_frames(clip[:, 1:], cache)
    rc, out = raw_tokenize_frames(tok._engine, clip[:, 1:].contiguous(), cache.handle)
    assert rc == INVALID and (out == SENT).all(), "a cache filled under another context length was accepted"
    assert b"context length" in lib().ivg_last_error(tok._engine.h)


def test_refusals():
    from ivideogpt_amd import CompressiveVQModel, LlamaForCausalLM, weights as W
    tok, ctx, px, g = model_of("tok_mini64_ctx2")
    ids0, cache = tok.encode_context(px, ctx, return_cache=True)
    eng = tok._engine
    frames = px[:, ctx:].contiguous()
    good = tok.tokenize_frames(frames, cache)
    B = px.shape[0]

    def refused(status, what, *a, engine=eng, **k):
        rc, out = raw_tokenize_frames(engine, *a, **k)
        assert rc == status, f"{what}: status {rc}, expected {status}: {engine.lib.ivg_last_error(engine.h)}"
        assert (out == SENT).all(), f"{what}: a refused call wrote ids"
        assert engine.lib.ivg_last_error(engine.h), f"{what}: no text in ivg_last_error"

    refused(INVALID, "null cache", frames, None)
    empty = eng.enc_cache_create(B)
    refused(INVALID, "unfilled cache", frames, empty)
    eng.enc_cache_destroy(empty)
    other = CompressiveVQModel(tok.config, tok._sd, encode_dtype="fp32", decode_dtype="fp32").to(DEV)
    _, foreign = other.encode_context(px, ctx, return_cache=True)
    refused(INVALID, "cache of another engine", frames, foreign.handle)
    refused(INVALID, "another B", frames[:1].contiguous(), cache.handle)
    refused(INVALID, "n = 0", frames, cache.handle, n=0)
    refused(INVALID, "bad dtype", frames, cache.handle, dtype=7)
    refused(CAPACITY, "B above max_batch", frames.repeat(eng.max_batch, 1, 1, 1, 1)[:eng.max_batch + 1].contiguous(), cache.handle)
    refused(CAPACITY, "n above max_frames - ctx", frames.repeat(1, eng.max_frames, 1, 1, 1)[:, :eng.max_frames - ctx + 1].contiguous(), cache.handle)
    tok.set_context_length(1)
    try:
        refused(INVALID, "another context length", frames, cache.handle)
    finally:
        tok.set_context_length(ctx)
    # an engine without a tokenizer: the transformer's
    lcfg = dict(W.LLAMA_SMALL, hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=2)
    llm = LlamaForCausalLM(lcfg, W.random_llama_state_dict(lcfg, 5), dtype="fp32").to(DEV)
    leng = llm._ensure(2, 4)
    refused(INVALID, "engine without a tokenizer", frames, cache.handle, engine=leng)
    h = C.c_void_p()
    assert leng.lib.ivg_enc_cache_create(leng.h, 2, C.byref(h)) == INVALID
    assert eng.lib.ivg_enc_cache_create(eng.h, eng.max_batch + 1, C.byref(h)) == CAPACITY
    # ivg_enc_cache_select: the refusals of ivg_cache_select
    p = np.array([0, 2], dtype=np.int32)
    assert eng.lib.ivg_enc_cache_select(eng.h, cache.handle, p.ctypes.data_as(C.c_void_p), 2, C.byref(h), None) == INVALID
    p = np.zeros(eng.max_batch + 1, dtype=np.int32)
    assert eng.lib.ivg_enc_cache_select(eng.h, cache.handle, p.ctypes.data_as(C.c_void_p), int(p.size), C.byref(h), None) == CAPACITY
    assert eng.lib.ivg_enc_cache_select(eng.h, None, p.ctypes.data_as(C.c_void_p), 1, C.byref(h), None) == INVALID
    # ivg_encode_context_cached: a cache of another B
    sink = torch.full((1, 257 * ctx), SENT, dtype=torch.int64, device=DEV)
    with eng.stream() as s:
        rc = eng.lib.ivg_encode_context_cached(eng.h, _p(px[:1].contiguous()), 0, 1, px.shape[1], _p(sink), sink.stride(0), cache.handle, s)
    torch.cuda.synchronize()
    assert rc == INVALID and (sink == SENT).all()
    # and a good call afterwards gives the ids it gave before
    assert torch.equal(tok.tokenize_frames(frames, cache), good)


def test_refill_after_an_engine_rebuild():
    from ivideogpt_amd import CompressiveVQModel
    cfg, sd, ctx, px, g = tokenizer_fixture("tok_mini64_ctx2.npz")
    tok = CompressiveVQModel(cfg, sd, encode_dtype="fp32", decode_dtype="fp32").to(DEV)
    px = px.to(DEV)
    _, cache = tok.encode_context(px[:, :ctx], ctx, return_cache=True)
    first = tok._engine
    dyn = tok.tokenize_frames(px[:, ctx:ctx + 1], cache)
    tok.tokenize(px.repeat(2, 1, 1, 1, 1), ctx)        # a larger batch: the engine is rebuilt, the cache's projections are gone
    assert tok._engine is not first
    assert torch.equal(tok.tokenize_frames(px[:, ctx:ctx + 1], cache), dyn), "the cache was not filled again from its context pixels"
    assert cache.engine is tok._engine


def test_bf16_encoder_equals_its_own_tokenize():
    """A bf16 encoder's ids are promised equal to tokenize's only where both calls dispatch the same kernels (include/ivg.h): bf16 1x1
    convolutions and dense GEMMs leave the implicit-GEMM kernel for the 256 x 256-tile one when their output width is a multiple of
    256 at >= 4096 rows, or a multiple of 128 at >= 2^18 rows.  The mini model's widths are 64 and 128 (block_out_channels 64, 128, 128;
    latent and codebook width 64): never a multiple of 256, and its widest GEMM sees at most 4 images x 1024 pixels = 4096 < 2^18 rows
    here -- so every GEMM stays on the implicit-GEMM kernel in tokenize (B * F = 4 images) and in tokenize_frames (2 or 4), whose
    summation order per output element does not depend on the row count."""
    tok, ctx, px, g = model_of("tok_mini64_ctx2", "bf16")
    full, _ = tok.tokenize(px, ctx)
    ids0, cache = tok.encode_context(px, ctx, return_cache=True)
    assert torch.equal(ids0, full[:, :257 * ctx])
    dyn = tok.tokenize_frames(px[:, ctx:], cache)
    assert torch.equal(dyn[:, :-1], full[:, 257 * ctx:])
    one = tok.tokenize_frames(px[:, ctx:ctx + 1], cache)
    assert torch.equal(one, dyn[:, :17])
