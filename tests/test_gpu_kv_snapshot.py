"""Saving and restoring the kept K / V cache (include/ivg.h ivg_kv_snapshot_create / _restore; launch_kv_snapshot over
kv_gather_rows_kernel) on the MI355X: the copy byte for byte against numpy through ivg_op_kv_snapshot, a round trip
through the engine in every cache format and both launch profiles against a model that never left, ``parents`` against
``select_kept_cache``, the embeddings path, another engine over the same weights, the refusals, and sessions of one
``VideoPredictor`` interleaved with each other and with rollouts.  Every check is an equality.  Tiny model throughout, as
tests/test_gpu_frame_heads.py (hidden 128, 2 layers, 2 heads of 64, L0 = 514)."""

import ctypes as C

import numpy as np
import pytest
import torch

from test_gpu_frame_heads import DEV, FLAVOURS, PER_HEAD, PROFILES, make_head, three_rows
from test_gpu_kv_select import CASES, HEADS, LAYERS, LMAX, continue_scored, first_step, hashed_buffer
from test_gpu_track import episode, extend_rows, predictors

pytestmark = pytest.mark.gpu
OK, INVALID, CAPACITY = 0, -1, -4
POISON = 0xA5


def lib():
    from ivideogpt_amd import _lib
    return _lib.load()


def counters():
    return lib().ivg_debug_counter(b"kv_snapshot_rows_saved"), lib().ivg_debug_counter(b"kv_snapshot_rows_restored")


# ------------------------------------------------------------------------------------------------ 1. the copy, byte for byte
def blocks_of(buf, chunk, ra, rb):
    return buf.reshape(LAYERS * 2, chunk, HEADS, LMAX * (ra + rb))


def compact(buf, chunk, ra, rb, length, B):
    """[layers * 2][B][heads]{length * ra | length * rb} of a buffer laid out as the cache is."""
    b = blocks_of(buf, chunk, ra, rb)
    return np.concatenate([b[:, :B, :, :length * ra], b[:, :B, :, LMAX * ra:LMAX * ra + length * rb]], axis=3).reshape(-1)


def restored(dst, src, chunk, ra, rb, length, parents):
    """Rows < n, positions < length of both planes of dst come from row parents[i] of src; every other byte of dst stays."""
    s, want = blocks_of(src, chunk, ra, rb), blocks_of(dst, chunk, ra, rb).copy()
    for i, p in enumerate(parents):
        want[:, i, :, :length * ra] = s[:, p, :, :length * ra]
        if rb:
            want[:, i, :, LMAX * ra:LMAX * ra + length * rb] = s[:, p, :, LMAX * ra:LMAX * ra + length * rb]
    return want.reshape(-1)


def op_snapshot(buf, chunk, ra, rb, length, B, dense, dense_bytes, parents, direction):
    p = np.ascontiguousarray(parents, dtype=np.int32) if parents is not None else None
    rc = lib().ivg_op_kv_snapshot(C.c_void_p(buf.data_ptr()), LAYERS, chunk, HEADS, LMAX, ra, rb, length, B, C.c_void_p(dense.data_ptr()), dense_bytes,
                                  p.ctypes.data_as(C.c_void_p) if p is not None else None, int(p.size) if p is not None else 0, direction, None)
    torch.cuda.synchronize()
    return rc


def other_hash(chunk, ra, rb):
    return (hashed_buffer(chunk, ra, rb)[::-1] ^ np.uint8(0x3C)).copy()


@pytest.mark.parametrize("ra,rb", [(16, 0), (128, 64), (64, 0)], ids=["fp32_hd4", "planes24", "fp8"])
def test_copy_is_byte_exact_both_ways(ra, rb):
    chunk, slack = 8, 256
    src, dst0 = hashed_buffer(chunk, ra, rb), other_hash(chunk, ra, rb)
    assert not np.array_equal(src, dst0)
    src_dev = torch.from_numpy(src).to(DEV)
    for length in (1, 17, 40):
        for name, (B, parents) in CASES.items():
            size = LAYERS * 2 * B * HEADS * length * (ra + rb)
            dense = torch.full((size + slack,), POISON, dtype=torch.uint8, device=DEV)
            s0, r0 = counters()
            assert op_snapshot(src_dev, chunk, ra, rb, length, B, dense, size, None, 0) == OK, name
            assert counters() == (s0 + B, r0), f"{name}: rows saved"
            got = dense.cpu().numpy()
            want = compact(src, chunk, ra, rb, length, B)
            assert want.size == size and np.array_equal(got[:size], want), f"{name}, len {length}: {(got[:size] != want).sum()} bytes of the image differ"
            assert (got[size:] == POISON).all(), f"{name}, len {length}: the save wrote behind the image"
            assert np.array_equal(src_dev.cpu().numpy(), src), "the save changed its source"
            dst = torch.from_numpy(dst0).to(DEV)
            assert op_snapshot(dst, chunk, ra, rb, length, B, dense, size, parents, 1) == OK, name
            assert counters() == (s0 + B, r0 + len(parents)), f"{name}: rows restored"
            got, want = dst.cpu().numpy(), restored(dst0, src, chunk, ra, rb, length, parents)
            assert np.array_equal(got, want), f"{name}, len {length}: {(got != want).sum()} bytes differ after the restore"
            assert np.array_equal(dense.cpu().numpy()[:size], compact(src, chunk, ra, rb, length, B)), "the restore changed the image"
    # refusals, nothing launched: an image that does not fit, more rows than the chunk, a parent outside the image
    B, length = 3, 17
    size = LAYERS * 2 * B * HEADS * length * (ra + rb)
    dense = torch.full((size,), POISON, dtype=torch.uint8, device=DEV)
    dst = torch.from_numpy(dst0).to(DEV)
    c0 = counters()
    assert op_snapshot(src_dev, chunk, ra, rb, length, B, dense, size - 16, None, 0) == CAPACITY
    assert op_snapshot(dst, chunk, ra, rb, length, B, dense, size - 16, [0, 1], 1) == CAPACITY
    assert op_snapshot(dst, chunk, ra, rb, length, B, dense, size, [0] * 9, 1) == CAPACITY
    assert op_snapshot(dst, chunk, ra, rb, length, B, dense, size, [0, 3], 1) == INVALID
    assert op_snapshot(dst, chunk, ra, rb, length, B, dense, size, [0, -1], 1) == INVALID
    assert op_snapshot(dst, chunk, ra, rb, length, B, dense, size, None, 1) == INVALID
    assert (dense.cpu().numpy() == POISON).all() and np.array_equal(dst.cpu().numpy(), dst0) and counters() == c0


def test_copy_at_the_limit_of_the_move_table():
    """chunk 128, B = n = 128: every entry of the uint8 move table in use, a seeded resampling with duplicates."""
    chunk, ra, rb, length, B = 128, 128, 64, 17, 128
    src, dst0 = hashed_buffer(chunk, ra, rb), other_hash(chunk, ra, rb)
    size = LAYERS * 2 * B * HEADS * length * (ra + rb)
    dense = torch.full((size + 256,), POISON, dtype=torch.uint8, device=DEV)
    parents = np.random.default_rng(5).integers(0, 128, 128).tolist()
    s0, r0 = counters()
    assert op_snapshot(torch.from_numpy(src).to(DEV), chunk, ra, rb, length, B, dense, size, None, 0) == OK
    got = dense.cpu().numpy()
    assert np.array_equal(got[:size], compact(src, chunk, ra, rb, length, B)) and (got[size:] == POISON).all()
    dst = torch.from_numpy(dst0).to(DEV)
    assert op_snapshot(dst, chunk, ra, rb, length, B, dense, size, parents, 1) == OK
    assert counters() == (s0 + 128, r0 + 128)
    assert np.array_equal(dst.cpu().numpy(), restored(dst0, src, chunk, ra, rb, length, parents))


# ------------------------------------------------------------------------------------------------ 2. round trip through the engine
def two_frames(head, grown, table, v):
    """17 + 17 tokens on the kept cache: tokens, frame rewards, frame hidden states and token scores."""
    return head.generate(grown, do_sample=True, top_k=100, max_new_tokens=33, action=table, uniforms=v.contiguous(), reuse_cache=True,
                         return_reward="frames", output_frame_hidden_states=True, output_token_scores=True)


def assert_same(got, want, what):
    for a, b, name in zip(got, want, ("tokens", "frame rewards", "frame hidden states", "token scores")):
        if isinstance(a, tuple):
            for x, y in zip(a, b):
                assert torch.equal(x, y), f"{what}: {name} differ"
        else:
            assert torch.equal(a, b), f"{what}: {name} differ ({(a != b).sum().item()} elements)"


def detour(head, ids, table, uni):
    """Another call that overwrites the kept cache: other prompts, two rows."""
    other = ids[[1, 0]].clone()
    other[:, 7:90] = ids[[0, 2], 7:90]
    head.generate(other.contiguous(), do_sample=True, top_k=100, max_new_tokens=17, action=table[[2, 0]].contiguous(), uniforms=uni[:2, 3:20].contiguous())


def kv_bytes(dtype, kv):
    return 3 if dtype == "x3" else 1 if kv is not None else 2 if dtype == "bf16" else 4


@PROFILES
@pytest.mark.parametrize("flavour", list(FLAVOURS))
def test_round_trip_equals_the_run_that_never_left(flavour, lds_kb):
    dtype, kv = FLAVOURS[flavour]
    head, twin = make_head(dtype, lds_kb, kv=kv), make_head(dtype, lds_kb, kv=kv)
    ids, table, uni = three_rows()
    table = torch.cat([table, table[:, :1]], 1).contiguous()   # one row more, for the forced sdf behind the frame calls' last frame: the kept
    u0, v = uni[:, :17].contiguous(), uni[:, 17:51].contiguous()   # cache's action table has the shape every later call presents
    for m in (head, twin):
        m.llm._ensure(6, 8)   # (room for the fan-out's six candidates and the frame calls' forced-sdf action row: no engine is rebuilt below)
    grown = first_step(head, ids, table, u0)
    assert torch.equal(first_step(twin, ids, table, u0), grown)
    s0, r0 = counters()
    kept = head.save_kept_cache()
    assert (kept.rows, kept.length, kept.from_embeds, kept.act_T, kept.ctx) == (3, 530, False, table.shape[1], 2)
    assert kept.nbytes == 2 * 2 * 3 * 2 * 530 * 64 * kv_bytes(dtype, kv) + 3 * 531 * 8 + 3 * table.shape[1] * table.shape[2] * 4
    assert counters() == (s0 + 3, r0)
    detour(head, ids, table, uni)
    head.restore_kept_cache(kept)
    assert counters() == (s0 + 3, r0 + 3)
    want = two_frames(twin, grown, table, v)
    assert_same(two_frames(head, grown, table, v), want, "continue after save / detour / restore")
    # restore again, then extend and fan out: against the same calls on the model that never left
    full = want[0][:, :548].contiguous()                                    # the 16 tokens of the next frame and its forced sdf
    g = torch.Generator().manual_seed(37)
    table6 = torch.randn(6, table.shape[1], table.shape[2], generator=g).to(DEV)
    uni6 = torch.rand(6, 17, generator=g).to(DEV)

    def extend_and_fan(m):
        nll = m.extend_kept_cache(full, action=table, keep=530, return_nll=True)
        return (nll,) + tuple(m.fan_out(full, 2, action=table6.clone(), do_sample=True, max_new_tokens=16, uniforms=uni6, return_reward="frames",
                                        output_frame_hidden_states=True, output_token_scores=True))

    first_step(twin, ids, table, u0)
    ref = extend_and_fan(twin)
    detour(head, ids, table, uni)
    head.restore_kept_cache(kept)
    got = extend_and_fan(head)
    assert torch.equal(got[0], ref[0]), "token NLLs of the extend after a restore differ"
    assert_same(got[1:], ref[1:], "fan-out after restore and extend")
    kept.close()


# ------------------------------------------------------------------------------------------------ 3. parents
@pytest.mark.parametrize("parents", [[2, 2, 0], [1, 2, 0, 1], [1]], ids=["duplicate_and_drop", "grow", "one_row"])
def test_restore_with_parents_equals_select(parents):
    head, twin = make_head("bf16"), make_head("bf16")
    ids, table, uni = three_rows()
    u0 = uni[:, :17].contiguous()
    v = torch.rand(len(parents), 17, generator=torch.Generator().manual_seed(3)).to(DEV)
    for m in (head, twin):
        m.llm._ensure(4, table.shape[1])
    idx = torch.tensor(parents, device=DEV)
    grown = first_step(twin, ids, table, u0)
    twin.select_kept_cache(parents)
    want = continue_scored(twin, grown[idx].contiguous(), table[idx].contiguous(), v)
    assert torch.equal(first_step(head, ids, table, u0), grown)
    with head.save_kept_cache() as kept:
        for round_ in range(2):                                              # the snapshot is const: a second restore gives the same again
            detour(head, ids, table, uni)
            head.restore_kept_cache(kept, parents if round_ == 0 else idx)   # (a device tensor is brought to the host)
            out, rew, sc = continue_scored(head, grown[idx].contiguous(), table[idx].contiguous(), v)
            assert torch.equal(out, want[0]) and torch.equal(rew, want[1]), f"restore {round_}: the continue differs from select + continue"
            for a, b in zip(sc, want[2]):
                assert torch.equal(a, b)
        # the guard still guards: ungathered rows are refused, and the refusal leaves the restored cache usable
        if parents != [1]:
            head.restore_kept_cache(kept, parents)
            with pytest.raises(AssertionError, match="different prefix"):
                continue_scored(head, grown[:len(parents)].contiguous() if len(parents) <= 3 else grown[[0, 1, 2, 0]].contiguous(),
                                table[idx].contiguous(), v)
            out, _, _ = continue_scored(head, grown[idx].contiguous(), table[idx].contiguous(), v)
            assert torch.equal(out, want[0])
        with pytest.raises(ValueError):
            head.restore_kept_cache(kept, [0, 3])


# ------------------------------------------------------------------------------------------------ 4. the embeddings path
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_embeds_path_round_trip(dtype):
    head, twin = make_head(dtype), make_head(dtype)
    ids, _, uni = three_rows()
    u0, v = uni[:, :17].contiguous(), uni[:, 17:34].contiguous()

    def first(m):
        sdf = torch.full((3, 1), m.token_for_sdf, dtype=torch.int64, device=DEV)
        emb = m.get_input_embeddings(ids)
        new = m.llm.generate(inputs_embeds=emb, do_sample=True, top_k=100, max_new_tokens=17, uniforms=u0, use_cache=True)
        assert not m.llm.last_generate_reused_cache
        return torch.cat([emb, m.get_input_embeddings(torch.cat([new[:, :-1], sdf], 1))], 1)

    def step(m, emb):
        r = m.llm.generate(inputs_embeds=emb, do_sample=True, top_k=100, max_new_tokens=17, uniforms=v, use_cache=True, return_dict_in_generate=True,
                           output_hidden_states=True)
        return r.sequences, r.hidden_states[-1][-1]

    grown = first(twin)
    want = step(twin, grown)
    assert twin.llm.last_generate_reused_cache
    assert torch.equal(first(head), grown)
    kept = head.save_kept_cache()
    assert kept.from_embeds and kept.rows == 3 and kept.length == 530 and kept.act_T == 0
    other = head.get_input_embeddings(ids[[1, 0]].contiguous())
    head.llm.generate(inputs_embeds=other, do_sample=True, top_k=100, max_new_tokens=17, uniforms=u0[:2].contiguous(), use_cache=True)
    head.restore_kept_cache(kept)
    seq, hid = step(head, grown)
    assert head.llm.last_generate_reused_cache is True, "the restored embeddings snapshot was not recognised: the prompt was prefilled again"
    assert torch.equal(seq, want[0]) and torch.equal(hid, want[1])
    # into a replica that never ran an embeds call (its embeddings snapshot is allocated by the restore), gathered by parents
    rep = head.replica()
    rep.restore_kept_cache(kept, [2, 0])
    r = rep.llm.generate(inputs_embeds=grown[[2, 0]].contiguous(), do_sample=True, top_k=100, max_new_tokens=17, uniforms=v[[2, 0]].contiguous(), use_cache=True)
    assert rep.llm.last_generate_reused_cache is True and torch.equal(r, want[0][[2, 0]])
    kept.close()


# ------------------------------------------------------------------------------------------------ 5. another engine, the same weights
@pytest.mark.parametrize("flavour", ["bf16", "bf16_fp8_per_head", "x3"])
def test_restore_into_a_replica_and_a_rebuilt_engine(flavour):
    dtype, kv = FLAVOURS[flavour]
    head = make_head(dtype, kv=kv)
    ids, table, uni = three_rows()
    u0, v = uni[:, :17].contiguous(), uni[:, 17:34].contiguous()
    grown = first_step(head, ids, table, u0)
    kept = head.save_kept_cache()
    want = continue_scored(head, grown, table, v)
    rep = head.replica()
    assert rep.llm._engine is None
    rep.restore_kept_cache(kept)
    assert rep.llm._engine is not None and rep.llm._engine is not head.llm._engine
    out, rew, sc = continue_scored(rep, grown, table, v)
    assert torch.equal(out, want[0]) and torch.equal(rew, want[1]) and all(torch.equal(a, b) for a, b in zip(sc, want[2])), "continue in the replica"
    # the engine the model rebuilds for a larger batch: five rows out of the three saved ones
    old = head.llm._engine
    assert old.max_batch == 3
    parents = [0, 1, 2, 2, 1]
    idx = torch.tensor(parents, device=DEV)
    head.restore_kept_cache(kept, parents)
    assert head.llm._engine is not old and head.llm._engine.max_batch == 5
    out, rew, sc = continue_scored(head, grown[idx].contiguous(), table[idx].contiguous(), v[idx].contiguous())
    assert torch.equal(out, want[0][idx]) and torch.equal(rew, want[1][idx]) and all(torch.equal(a, b[idx]) for a, b in zip(sc, want[2])), \
        "continue in the rebuilt engine"
    kept.close()


# ------------------------------------------------------------------------------------------------ 6. refusals
def raw_restore(eng, kept, parents, n=None):
    p = np.ascontiguousarray(parents, dtype=np.int32) if parents is not None else None
    with eng.stream() as s:
        rc = eng.lib.ivg_kv_snapshot_restore(eng.h, kept.h if kept is not None else None, p.ctypes.data_as(C.c_void_p) if p is not None else None,
                                             (len(parents) if n is None else n) if parents is not None else 0, s)
    torch.cuda.synchronize()
    return rc


def raw_create(eng, out):
    with eng.stream() as s:
        rc = eng.lib.ivg_kv_snapshot_create(eng.h, C.byref(out) if out is not None else None, s)
    torch.cuda.synchronize()
    return rc


def test_refusals_leave_the_kept_cache_usable():
    ids, table, uni = three_rows()
    u0, v = uni[:, :17].contiguous(), uni[:, 17:34].contiguous()
    head = make_head()
    eng = head.llm._ensure(3, table.shape[1])
    c0 = counters()
    slot = C.c_void_p(0x1234)
    assert raw_create(eng, slot) == INVALID and slot.value == 0x1234, "a fresh engine holds no kept cache"
    with pytest.raises(ValueError, match="no kept cache"):
        head.save_kept_cache()
    grown = first_step(head, ids, table, u0)
    want, wrew, _ = continue_scored(head, grown, table, v)
    first_step(head, ids, table, u0)
    kept = head.save_kept_cache()
    saved = counters()
    assert saved == (c0[0] + 3, c0[1])
    assert raw_create(eng, None) == INVALID, "a null out"
    stranger = make_head()                                                 # the same config and values, other tensors in HBM
    seng = stranger.llm._ensure(3, table.shape[1])
    first_step(stranger, ids, table, u0)
    for what, status, e, args in (("a parent out of range", INVALID, eng, (kept, [0, 3, 1])), ("a negative parent", INVALID, eng, (kept, [0, -1, 1])),
                                  ("n = 0 with parents", INVALID, eng, (kept, [0], 0)), ("a null snapshot", INVALID, eng, (None, [0, 1, 2])),
                                  ("n above the chunk", CAPACITY, eng, (kept, [0, 1, 2, 0])), ("other weights", INVALID, seng, (kept, None))):
        m = stranger if e is seng else head
        assert torch.equal(first_step(m, ids, table, u0), grown)
        assert raw_restore(e, *args) == status, what
        out, rew, _ = continue_scored(m, grown, table, v)
        assert torch.equal(out, want) and torch.equal(rew, wrew), f"{what}: the continue after the refused restore differs"
    with pytest.raises(ValueError, match="other weights"):
        stranger.restore_kept_cache(kept)
    assert counters() == saved, "a refused restore moved rows"
    # no kept cache after a shared-context call
    twice = ids[:1].repeat(2, 1)
    head.generate(twice, do_sample=True, max_new_tokens=17, action=table[:2].contiguous(), uniforms=u0[:2].contiguous(), shared_context=2)
    assert raw_create(eng, slot) == INVALID and slot.value == 0x1234, "a shared-context cache is never kept"
    # a snapshot longer than a max_seq-limited engine over the same weights holds
    short = head.replica()
    short.llm._max_seq = 520
    short.generate(ids, do_sample=False, max_new_tokens=1, action=table)
    assert raw_restore(short.llm._engine, kept, None) == CAPACITY
    with pytest.raises(ValueError, match="exceed the KV cache"):
        short.restore_kept_cache(kept)
    short.extend_kept_cache(ids, action=table, keep=513)                   # its own kept cache is what it was
    kept.close()
    # the format or a scale changed since the save (bf16: the FP8 cache is available)
    head = make_head("bf16")
    grown = first_step(head, ids, table, u0)
    native = head.save_kept_cache()
    head.set_kv_cache_dtype("fp8_e4m3")
    eng = head.llm._engine
    g8 = first_step(head, ids, table, u0)
    want8 = continue_scored(head, g8, table, v)[0]
    assert torch.equal(first_step(head, ids, table, u0), g8)
    fp8 = head.save_kept_cache()
    assert raw_restore(eng, native, None) == INVALID, "a native snapshot into the FP8 cache"
    assert torch.equal(continue_scored(head, g8, table, v)[0], want8)
    for what, setting in (("a uniform scale", dict(k_scale=2.0)), ("a scale table", dict(scales=PER_HEAD)), ("the format", None)):
        head.set_kv_cache_dtype("fp8_e4m3", **setting) if setting is not None else head.set_kv_cache_dtype("auto")
        g2 = first_step(head, ids, table, u0)
        w2 = continue_scored(head, g2, table, v)[0]
        assert torch.equal(first_step(head, ids, table, u0), g2)
        assert raw_restore(eng, fp8, None) == INVALID, what
        with pytest.raises(ValueError):
            head.restore_kept_cache(fp8)
        assert torch.equal(continue_scored(head, g2, table, v)[0], w2), f"{what}: the continue after the refused restore differs"
    head.restore_kept_cache(native)                                        # back in the native format: accepted
    assert torch.equal(continue_scored(head, grown, table, v)[0][:, :531], grown)
    native.close(), fp8.close()


# ------------------------------------------------------------------------------------------------ 7. sessions of one predictor
def session(trk, frames, acts, plans, k, uni):
    """observe, plan, observe -> the two surprises and the plan's outputs, as a generator: one ``next`` per call."""
    s1 = trk.observe(frames[0], acts[0])
    yield
    plan = trk.plan(plans, samples=k, return_uncertainty=True, uniforms=uni)
    yield
    s2 = trk.observe(frames[1], acts[1])
    yield (s1, *plan, s2)


def run(gen):
    for last in gen:
        pass
    return last


@pytest.mark.parametrize("llm_dtype", ["fp32", "bf16"])
def test_sessions_and_rollouts_interleave(tmp_path, llm_dtype):
    shared, alone_a, alone_b = predictors(tmp_path, llm_dtype, n=3)
    for vp in (shared, alone_a, alone_b):
        vp.model.llm._ensure(8, 40)   # (every engine as large as anything below needs: no rebuild, whose prompt pass has other bits)
    k, horizon = 2, 2
    g = torch.Generator().manual_seed(12)
    eps = {"a": episode(2, 2, seed=8), "b": episode(3, 2, seed=9)}
    plans = {n: torch.randn(e[0].shape[0] * k, horizon, 4, generator=g) for n, e in eps.items()}
    unis = {n: torch.rand(e[0].shape[0] * k, 17 * horizon - 1, generator=g).to(DEV) for n, e in eps.items()}
    want = {n: run(session(vp.track(eps[n][0]), eps[n][1], eps[n][2], plans[n], k, unis[n])) for n, vp in (("a", alone_a), ("b", alone_b))}
    saved0 = counters()
    a, b = shared.track(eps["a"][0]), shared.track(eps["b"][0])
    assert a.suspended and not b.suspended and shared._active is b
    ga, gb = (session(t, eps[n][1], eps[n][2], plans[n], k, unis[n]) for n, t in (("a", a), ("b", b)))
    r0 = extend_rows()
    next(ga), next(gb)                                                       # observe, observe
    shared.rollout_actions(eps["b"][0], torch.randn(3, 2, 4, generator=g))
    assert shared._active is None and a.suspended and b.suspended
    next(ga), next(gb)                                                       # plan, plan
    shared.rollout(eps["a"][0], lambda o, t: torch.zeros(o.shape[0], 4), 2)
    got = {"b": next(gb), "a": next(ga)}                                     # observe, observe
    assert extend_rows() - r0 == 2 * (2 + 3) * 17, "only the observes extend a kept cache: no session was established again"
    assert a.restore_fallbacks == 0 and b.restore_fallbacks == 0 and a.reanchors == 0 and b.reanchors == 0
    assert counters()[0] > saved0[0] and counters()[1] > saved0[1]
    names = ("surprise 1", "observations", "actions", "rewards", "uncertainty", "surprise 2")
    for n in ("a", "b"):
        for x, y, what in zip(got[n], want[n], names):
            assert torch.equal(x, y), f"session {n}: {what} differ from the session run alone"
    # a call past the predictor still ends the session's claim: refused by the verification, as ever
    shared._activate(a)
    shared.model.generate(b.tokens, do_sample=False, max_new_tokens=1, action=b.table)
    with pytest.raises(ValueError):
        a.observe(eps["a"][1][0], eps["a"][2][0])
    # new weights: the snapshot is refused and the session pays the prompt pass, once
    shared._activate(b)
    shared._suspend_active()
    shared.model.load_state_dict(shared.model.state_dict())
    shared.model.llm._ensure(8, 40)
    b.select([0, 1, 2])
    assert b.restore_fallbacks == 1 and not b.suspended and shared._active is b
    # a call past the predictor that leaves NO kept cache: the next rollout still runs (nothing to save), the session starts afresh
    shared.model.generate(b.tokens[:1, :257 * 2].repeat(2, 1), do_sample=True, max_new_tokens=17, action=b.table[:2].contiguous(), shared_context=2)
    shared.rollout_actions(eps["b"][0], torch.randn(3, 2, 4, generator=g))
    assert b.suspended and shared._active is None
    b.select([0, 1, 2])
    assert b.restore_fallbacks == 2 and shared._active is b


def test_plan_grows_the_engine_by_restore(tmp_path):
    small, large = predictors(tmp_path, "bf16", n=2)
    large.model.llm._ensure(6, 40)
    B, k, horizon = 2, 3, 2
    obs, (f1,), (a1,) = episode(B, 1)
    g = torch.Generator().manual_seed(3)
    plans = torch.randn(B * k, horizon, 4, generator=g)
    uni = torch.rand(B * k, 17 * horizon - 1, generator=g).to(DEV)
    want_trk = large.track(obs)
    s_want = want_trk.observe(f1, a1)
    want = want_trk.plan(plans, samples=k, return_uncertainty=True, uniforms=uni)
    trk = small.track(obs, grow="restore")
    assert trk.grow == "restore" and small.model.llm._engine.max_batch == B
    assert torch.equal(trk.observe(f1, a1), s_want)
    r0, c0 = extend_rows(), counters()
    got = trk.plan(plans, samples=k, return_uncertainty=True, uniforms=uni)
    assert small.model.llm._engine.max_batch == B * k
    assert counters() == (c0[0] + B, c0[1] + B) and extend_rows() == r0, "the kept cache came into the larger engine by a copy"
    for x, y, what in zip(got, want, ("observations", "actions", "rewards", "uncertainty")):
        assert torch.equal(x, y), f"{what} differ from the plan of a predictor that was large enough from the start"
