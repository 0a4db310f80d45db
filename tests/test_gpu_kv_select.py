"""Resampling trajectories on the kept K / V cache (include/ivg.h ivg_kv_select / ivg_cache_select; kv_gather_rows_kernel, DESIGN.md
3.6) on the MI355X: the kernel byte for byte against a numpy gather through ivg_op_kv_select, a continue after a select against rows
of the run without it bit for bit (every cache format, both launch profiles, truncation and growth), the on-device guard after a
select, the refusals through the C ABI, the embeddings path, the detokenizer cache and ``VideoPredictor.rollout(select=...)``.
Tiny model throughout, as tests/test_gpu_frame_heads.py (hidden 128, 2 layers, 2 heads of 64, L0 = 514)."""

import ctypes as C

import numpy as np
import pytest
import torch

from test_gpu_frame_heads import DEV, FLAVOURS, PER_HEAD, PROFILES, Dealer, make_head, three_rows

pytestmark = pytest.mark.gpu
OK, INVALID, CAPACITY = 0, -1, -4


def lib():
    from ivideogpt_amd import _lib
    return _lib.load()


def counters():
    return lib().ivg_debug_counter(b"kv_select_direct"), lib().ivg_debug_counter(b"kv_select_staged")


def moves_of(parents, n):
    """(direct, staged) rows of a select by the rule of the header, worked out here without the library's planner."""
    direct = staged = 0
    for i in range(n):
        s = parents[i]
        if s == i:
            continue
        if s >= n or parents[s] == s:
            direct += 1
        else:
            staged += 1
    return direct, staged


# ------------------------------------------------------------------------------------------------ 1. the kernel, byte for byte
LAYERS, HEADS, LMAX = 2, 2, 40
CASES = {   # name: (B_old, parents)
    "identity": (5, [0, 1, 2, 3, 4]),
    "swap": (2, [1, 0]),
    "3-cycle": (3, [1, 2, 0]),
    "all the same row": (4, [2, 2, 2, 2]),
    "drop": (6, [0, 2, 4]),
    "grow": (3, [0, 1, 2, 0, 1, 2, 1]),
    "mixed": (6, [1, 0, 2, 2, 5, 5]),
}


def hashed_buffer(chunk, ra, rb):
    n = LAYERS * 2 * chunk * HEADS * LMAX * (ra + rb)
    a = np.arange(n, dtype=np.uint64)
    return ((a * np.uint64(2654435761) + (a >> np.uint64(7))) >> np.uint64(11)).astype(np.uint8)


def gathered(snap, chunk, ra, rb, length, parents):
    """The rule: rows < n, positions < length of both planes come from row parents[i] of the snapshot; every other byte stays."""
    blocks = snap.reshape(LAYERS * 2, chunk, HEADS, LMAX * (ra + rb))
    want = blocks.copy()
    for i, p in enumerate(parents):
        want[:, i, :, :length * ra] = blocks[:, p, :, :length * ra]
        if rb:
            want[:, i, :, LMAX * ra:LMAX * ra + length * rb] = blocks[:, p, :, LMAX * ra:LMAX * ra + length * rb]
    return want.reshape(-1)


def op_select(buf, chunk, ra, rb, length, B_old, parents, scratch):
    p = np.ascontiguousarray(parents, dtype=np.int32)
    rc = lib().ivg_op_kv_select(C.c_void_p(buf.data_ptr()), LAYERS, chunk, HEADS, LMAX, ra, rb, length, B_old, p.ctypes.data_as(C.c_void_p), int(p.size),
                                C.c_void_p(scratch.data_ptr()) if scratch is not None else None, scratch.numel() if scratch is not None else 0, None)
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("ra,rb", [(16, 0), (128, 64), (64, 0)], ids=["fp32_hd4", "planes24", "fp8"])
def test_kernel_is_a_byte_exact_gather(ra, rb):
    chunk = 8
    snap = hashed_buffer(chunk, ra, rb)
    scratch = torch.empty(LAYERS * 2 * chunk * HEADS * LMAX * (ra + rb), dtype=torch.uint8, device=DEV)
    for length in (1, 17, 40):
        for name, (B_old, parents) in CASES.items():
            buf = torch.from_numpy(snap).to(DEV)
            d0, s0 = counters()
            assert op_select(buf, chunk, ra, rb, length, B_old, parents, scratch) == OK, name
            d1, s1 = counters()
            assert (d1 - d0, s1 - s0) == moves_of(parents, len(parents)), f"{name}: counters"
            got, want = buf.cpu().numpy(), gathered(snap, chunk, ra, rb, length, parents)
            assert np.array_equal(got, want), f"{name}, len {length}: {(got != want).sum()} bytes differ from the gather of the snapshot"
    assert moves_of(CASES["identity"][1], 5) == (0, 0) and moves_of(CASES["mixed"][1], 6) == (2, 2) and moves_of(CASES["3-cycle"][1], 3) == (0, 3)


def test_kernel_at_the_limit_of_the_move_table():
    """chunk 128, n = 128: every entry of the uint8 move table in use (a seeded resampling with duplicates, then a full cyclic shift)."""
    chunk, ra, rb, length = 128, 128, 64, 17
    snap = hashed_buffer(chunk, ra, rb)
    scratch = torch.empty(LAYERS * 2 * chunk * HEADS * LMAX * (ra + rb), dtype=torch.uint8, device=DEV)
    rng = np.random.default_rng(5)
    for parents in (rng.integers(0, 128, 128).tolist(), [(i + 1) % 128 for i in range(128)]):
        buf = torch.from_numpy(snap).to(DEV)
        d0, s0 = counters()
        assert op_select(buf, chunk, ra, rb, length, 128, parents, scratch) == OK
        d1, s1 = counters()
        assert (d1 - d0, s1 - s0) == moves_of(parents, 128)
        assert np.array_equal(buf.cpu().numpy(), gathered(snap, chunk, ra, rb, length, parents))
    assert moves_of([(i + 1) % 128 for i in range(128)], 128) == (0, 128)


def test_slab_groups_small_scratch_and_stable_parents():
    from ivideogpt_amd.transformer import stable_parents
    chunk, ra, rb, length = 8, 128, 64, 17
    B_old, parents = CASES["mixed"]
    snap = hashed_buffer(chunk, ra, rb)
    want = gathered(snap, chunk, ra, rb, length, parents)
    per_slab = moves_of(parents, len(parents))[1] * HEADS * length * (ra + rb)      # one slab's staged rows
    # room for one slab and a half: the four slabs go in four groups
    buf = torch.from_numpy(snap).to(DEV)
    assert op_select(buf, chunk, ra, rb, length, B_old, parents, torch.empty(per_slab * 3 // 2, dtype=torch.uint8, device=DEV)) == OK
    assert np.array_equal(buf.cpu().numpy(), want)
    # room for two: two groups
    buf = torch.from_numpy(snap).to(DEV)
    assert op_select(buf, chunk, ra, rb, length, B_old, parents, torch.empty(per_slab * 2, dtype=torch.uint8, device=DEV)) == OK
    assert np.array_equal(buf.cpu().numpy(), want)
    # not even one slab: refused with nothing written
    buf = torch.from_numpy(snap).to(DEV)
    d0, s0 = counters()
    assert op_select(buf, chunk, ra, rb, length, B_old, parents, torch.empty(per_slab - 16, dtype=torch.uint8, device=DEV)) == CAPACITY
    assert op_select(buf, chunk, ra, rb, length, B_old, parents, None) == CAPACITY
    assert np.array_equal(buf.cpu().numpy(), snap) and counters() == (d0, s0)
    # bad arguments: refused with nothing written
    assert op_select(buf, chunk, ra, rb, length, B_old, [0, 6], None) == INVALID
    assert op_select(buf, chunk, ra, rb, length, B_old, [0] * 9, None) == CAPACITY
    assert np.array_equal(buf.cpu().numpy(), snap)
    # a resampling arranged by stable_parents moves every row in place: no scratch at all
    for raw in ([5, 5, 1, 1, 3, 0], [4, 4, 4, 2, 2, 0, 1], [3, 3]):
        arranged, _ = stable_parents(raw, 6)
        buf = torch.from_numpy(snap).to(DEV)
        d0, s0 = counters()
        assert op_select(buf, chunk, ra, rb, length, 6, arranged.tolist(), None) == OK
        d1, s1 = counters()
        assert s1 == s0 and d1 - d0 == moves_of(arranged.tolist(), len(raw))[0]
        assert np.array_equal(buf.cpu().numpy(), gathered(snap, chunk, ra, rb, length, arranged.tolist()))


# ------------------------------------------------------------------------------------------------ 2. continue after a select
def first_step(head, ids, table, u0):
    """The 17-token call that leaves the kept cache: -> the grown prompt (B, 531), ending with the forced sdf."""
    return head.generate(ids, do_sample=True, top_k=100, max_new_tokens=17, action=table, uniforms=u0).contiguous()


def continue_scored(head, grown, table, u):
    return head.generate(grown, do_sample=True, top_k=100, max_new_tokens=17, action=table, uniforms=u.contiguous(), return_reward=True, reuse_cache=True,
                         output_token_scores=True)


def assert_children_equal_parents(head, ids, table, u0, parents, v):
    """Child i of a select (uniforms v[i]) against row parents[i] of a run WITHOUT select whose continue gave that row v[i]: the k-th
    child of every parent is checked against reference run k."""
    B, n = ids.shape[0], len(parents)
    rounds, seen = {}, {}
    for i, p in enumerate(parents):
        rounds.setdefault(seen.get(p, 0), []).append(i)
        seen[p] = seen.get(p, 0) + 1
    refs = {}
    for k, children in rounds.items():
        w = torch.full((B, 17), 0.5, device=DEV)
        for i in children:
            w[parents[i]] = v[i]
        grown = first_step(head, ids, table, u0)
        out, rew, sc = continue_scored(head, grown, table, w)
        for i in children:
            refs[i] = (out[parents[i]], rew[parents[i]], [s[parents[i]] for s in sc])
    grown = first_step(head, ids, table, u0)
    d0, s0 = counters()
    head.select_kept_cache(parents)
    d1, s1 = counters()
    assert (d1 - d0, s1 - s0) == moves_of(parents, n)
    idx = torch.tensor(parents, device=DEV)
    out, rew, sc = continue_scored(head, grown[idx].contiguous(), table[idx].contiguous(), v)
    assert out.shape == (n, 531 + 17)
    for i in range(n):
        ro, rr, rs = refs[i]
        assert torch.equal(out[i], ro), f"child {i} of row {parents[i]}: {(out[i] != ro).sum().item()} tokens differ"
        assert torch.equal(rew[i], rr), f"child {i}: reward {rew[i].item()!r} != {rr.item()!r}"
        for a, b, what in zip(sc, rs, ("logprob", "entropy", "max_logprob")):
            assert torch.equal(a[i], b), f"child {i}: {what} differs by {(a[i] - b).abs().max().item():.3e}"


@PROFILES
@pytest.mark.parametrize("flavour", list(FLAVOURS))
def test_continue_after_select_equals_unselected_rows_bitwise(flavour, lds_kb):
    dtype, kv = FLAVOURS[flavour]
    head = make_head(dtype, lds_kb, kv=kv)
    ids, table, uni = three_rows()
    assert_children_equal_parents(head, ids, table, uni[:, :17].contiguous(), [2, 2, 0], uni[:, 17:34].contiguous())


@pytest.mark.parametrize("parents", [[2, 0], [1, 2, 0, 1]], ids=["truncate", "grow"])
def test_continue_after_truncation_and_growth(parents):
    head = make_head("bf16")
    ids, table, uni = three_rows()
    head.llm._ensure(4, table.shape[1])   # room for a fourth trajectory: the cache chunk is the largest batch the engine was built for
    v = torch.rand(len(parents), 17, generator=torch.Generator().manual_seed(3)).to(DEV)
    assert_children_equal_parents(head, ids, table, uni[:, :17].contiguous(), parents, v)


# ------------------------------------------------------------------------------------------------ 3. the guard still guards
def test_guard_after_select():
    head = make_head()
    ids, table, uni = three_rows()
    u0, v = uni[:, :17].contiguous(), uni[:, 17:34].contiguous()
    parents = [2, 2, 0]
    idx = torch.tensor(parents, device=DEV)
    grown = first_step(head, ids, table, u0)
    head.select_kept_cache(parents)
    with pytest.raises(AssertionError, match="different prefix"):     # rows 0 and 2 are no longer what the original prompt says
        continue_scored(head, grown, table, v)
    with pytest.raises(AssertionError, match="different prefix"):     # the right tokens under the ungathered action table
        continue_scored(head, grown[idx].contiguous(), table, v)
    half = grown[idx].contiguous()
    half[1] = grown[1]                                                 # one row not gathered
    with pytest.raises(AssertionError, match="different prefix"):
        continue_scored(head, half, table[idx].contiguous(), v)
    out, _, _ = continue_scored(head, grown[idx].contiguous(), table[idx].contiguous(), v)   # the refusals left the selected cache usable
    assert out.shape == (3, 548) and torch.equal(out[:, :531], grown[idx])
    with pytest.raises(ValueError):
        head.select_kept_cache([0, 3])
    with pytest.raises(ValueError):
        head.select_kept_cache([0, 1, 2, 0])                          # a fourth row in an engine built for three


# ------------------------------------------------------------------------------------------------ 4. refusals (C ABI)
def raw_select(eng, parents, n=None):
    p = np.ascontiguousarray(parents, dtype=np.int32)
    with eng.stream() as s:
        rc = eng.lib.ivg_kv_select(eng.h, p.ctypes.data_as(C.c_void_p), len(parents) if n is None else n, s)
    torch.cuda.synchronize()
    return rc


def test_refusals_leave_the_kept_cache_usable():
    ids, table, uni = three_rows()
    u0, v = uni[:, :17].contiguous(), uni[:, 17:34].contiguous()
    head = make_head()
    eng = head.llm._ensure(3, table.shape[1])
    d0, s0 = counters()
    assert raw_select(eng, [0, 1, 2]) == INVALID, "a fresh engine holds no kept cache"
    grown = first_step(head, ids, table, u0)
    want, wrew, _ = continue_scored(head, grown, table, v)
    for what, status, args in (("an index out of range", INVALID, ([0, 3, 1],)), ("a negative index", INVALID, ([0, -1, 1],)), ("n = 0", INVALID, ([0], 0)),
                               ("n above the chunk", CAPACITY, ([0, 1, 2, 0],))):
        grown2 = first_step(head, ids, table, u0)
        assert torch.equal(grown2, grown)
        assert raw_select(eng, *args) == status, what
        out, rew, _ = continue_scored(head, grown, table, v)
        assert torch.equal(out, want) and torch.equal(rew, wrew), f"{what}: the continue after the refused select differs"
    assert raw_select(eng, [0, 1, 2]) == OK and counters() == (d0, s0), "the identity is accepted and moves nothing"
    # no kept cache: a shared-context call, a change of the format
    twice = ids[:1].repeat(2, 1)
    head.generate(twice, do_sample=True, max_new_tokens=17, action=table[:2].contiguous(), uniforms=u0[:2].contiguous(), shared_context=2)
    assert raw_select(eng, [1, 0]) == INVALID, "a shared-context cache is never kept"
    first_step(head, ids, table, u0)
    assert raw_select(eng, [0, 1, 2]) == OK
    from ivideogpt_amd import _lib
    eng.set_kv_format(_lib.IVG_KV_NATIVE)
    assert raw_select(eng, [0, 1, 2]) == INVALID, "ivg_set_kv_format invalidates the kept cache"
    # ... of the scales, a calibration pass (bf16 engines)
    head = make_head("bf16")
    eng = head.llm._ensure(3, table.shape[1])
    first_step(head, ids, table, u0)
    eng.set_kv_scales(PER_HEAD)
    assert raw_select(eng, [0, 1, 2]) == INVALID, "ivg_set_kv_scales invalidates the kept cache"
    first_step(head, ids, table, u0)
    eng.kv_calibrate(ids, actions=table, ctx=2)
    assert raw_select(eng, [0, 1, 2]) == INVALID, "ivg_kv_calibrate invalidates the kept cache"
    assert counters() == (d0, s0), "a refused select moved rows"


# ------------------------------------------------------------------------------------------------ 5. the embeddings path
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_embeds_path_after_select(dtype):
    head = make_head(dtype)
    llm = head.llm
    ids, _, uni = three_rows()
    u0, v = uni[:, :17].contiguous(), uni[:, 17:34].contiguous()
    sdf = torch.full((3, 1), head.token_for_sdf, dtype=torch.int64, device=DEV)
    parents = [2, 2, 0]
    idx = torch.tensor(parents, device=DEV)

    def first():
        emb = head.get_input_embeddings(ids)
        new = llm.generate(inputs_embeds=emb, do_sample=True, top_k=100, max_new_tokens=17, uniforms=u0, use_cache=True)
        assert not llm.last_generate_reused_cache
        return torch.cat([emb, head.get_input_embeddings(torch.cat([new[:, :-1], sdf], 1))], 1)

    def step(emb, u):
        r = llm.generate(inputs_embeds=emb, do_sample=True, top_k=100, max_new_tokens=17, uniforms=u.contiguous(), use_cache=True,
                         return_dict_in_generate=True, output_hidden_states=True, output_token_scores=True)
        return r.sequences, r.hidden_states[-1][-1], r.token_scores

    refs = []
    for w in (torch.stack([v[2], v[2], v[0]]), torch.stack([v[2], v[2], v[1]])):   # row 0 gets v[2]; row 2 gets v[0], then v[1]
        grown = first()
        seq, hid, sc = step(grown, w)
        assert llm.last_generate_reused_cache
        refs.append((seq, hid, sc))
    grown = first()
    llm.select_kept_cache(idx)                                                       # (a device tensor: brought to the host)
    seq, hid, sc = step(grown[idx].contiguous(), v)
    assert llm.last_generate_reused_cache is True, "the gathered embeddings were not recognised: the prompt was prefilled again"
    for i, (run, row) in enumerate(((0, 2), (1, 2), (0, 0))):
        rseq, rhid, rsc = refs[run]
        assert torch.equal(seq[i], rseq[row]) and torch.equal(hid[i], rhid[row]), f"child {i}"
        for a, b in zip(sc, rsc):
            assert torch.equal(a[i], b[row]), f"child {i}: token scores"
    # ungathered embeddings after a select: no reuse (and still the right tokens: the prompt is prefilled)
    grown = first()
    llm.select_kept_cache(parents)
    step(grown, v)
    assert llm.last_generate_reused_cache is False


# ------------------------------------------------------------------------------------------------ 6. the detokenizer cache
@pytest.mark.parametrize("decode_dtype", ["fp32", "bf16"])
def test_detokenizer_cache_select(decode_dtype):
    from ivideogpt_amd import CompressiveVQModel, weights as W
    cfg = W.tokenizer_config(block_out_channels=(64, 64, 64), layers_per_block=1, latent_channels=64, num_vq_embeddings=64, num_dyn_embeddings=64,
                             mid_block_add_attention=False, context_length=2, resolution=64, max_att_resolution=16)
    tok = CompressiveVQModel(cfg, W.random_tokenizer_state_dict(cfg, 3, codebook_std=0.4), encode_dtype="fp32", decode_dtype=decode_dtype).to(DEV)
    px = torch.rand(3, 4, 3, 64, 64, generator=torch.Generator().manual_seed(2)).to(DEV)
    ids, _ = tok.tokenize(px, 2)
    odt = torch.float32 if decode_dtype == "fp32" else torch.bfloat16
    _, cache = tok.detokenize(ids, 2, return_cache=True, out_dtype=odt)
    base = tok.detokenize(ids, 2, cache=cache, out_dtype=odt)
    for parents in ([2, 2, 0], np.array([1, 0]), torch.tensor([0, 1, 2], device=DEV)):
        idx = torch.as_tensor(parents).to(DEV).long()
        sel = cache.select(parents)
        assert sel.B == len(idx) and sel.handle.value != cache.handle.value
        got = tok.detokenize(ids[idx].contiguous(), 2, cache=sel, out_dtype=odt)
        assert torch.equal(got, base[idx]), f"parents {parents}: frames differ from the rows of the call on the original cache"
    assert torch.equal(tok.detokenize(ids, 2, cache=cache, out_dtype=odt), base), "the source cache changed"
    with pytest.raises(ValueError):
        cache.select([0, 3])
    with pytest.raises(ValueError):
        cache.select([0, 1, 2, 0])            # four rows in an engine built for three
    eng = tok._engine
    empty = eng.cache_create(3)
    with pytest.raises(AssertionError, match="empty"):
        eng.cache_select(empty, [0, 1])


# ------------------------------------------------------------------------------------------------ 7. VideoPredictor.rollout(select=...)
def test_rollout_with_select(tmp_path):
    from helpers import world_model_files
    from mbrl.video_predictor import VideoPredictor
    args, *_ = world_model_files(tmp_path, False)
    args.update(encode_dtype="fp32", decode_dtype="fp32", llm_dtype="fp32")
    vp = VideoPredictor("cuda", args)
    g = torch.Generator().manual_seed(8)
    obs = torch.randint(0, 256, (3, 9, 64, 64), generator=g).float()
    acts = torch.randn(3, 3, 4, generator=g)
    table = torch.rand(3, 51, generator=g).to(DEV)
    llm = vp.model.llm
    horizon = 3

    def run(select, rows=None, **kw):
        # the policy replays the plain run's actions of the trajectory each row descends from (rows: its genealogy, kept by `select`)
        llm._uniforms = Dealer(table)
        return vp.rollout(obs, lambda o, t: acts[rows() if rows else torch.arange(3), t], horizon, select=select, **kw)

    plain = run(None, return_uncertainty=True)
    assert vp.steps_with_kept_cache == horizon - 1
    seen = []
    ident = run(lambda t, o, r, u: seen.append((t, tuple(o.shape), tuple(r.shape), tuple(u.shape))) or (None if t == 0 else [0, 1, 2]), return_uncertainty=True)
    assert vp.steps_with_kept_cache == horizon - 1
    assert seen == [(t, (3, 9, 64, 64), (3, 1), (3, 1)) for t in range(horizon)]
    for a, b in zip(ident, plain):
        assert torch.equal(a, b), "select returning None / the identity changed the rollout"
    # after step 0: trajectory 1 is dropped, trajectory 2 duplicated (survivors stay in their rows); after step 1: a permutation
    lineage = [torch.arange(3)]

    def select(t, o, r, u):
        assert u is None and o.shape[0] == 3
        p = {0: [0, 2, 2], 1: [1, 0, 2]}.get(t)
        if p is not None:
            lineage[0] = lineage[0][torch.tensor(p)]
        return p

    d0, s0 = counters()
    obss, actions, rewards = run(select, rows=lambda: lineage[0])
    d1, s1 = counters()
    assert vp.steps_with_kept_cache == horizon - 1, "a step after a select did not run on the kept cache"
    assert (d1 - d0, s1 - s0) == (1, 2), "[0, 2, 2] moves one row in place, [1, 0, 2] two through scratch"
    assert obss.shape == (3, horizon + 1, 9, 64, 64) and actions.shape == (3, horizon + 1, 4) and rewards.shape == (3, horizon + 1, 1)
    po, pa, pr = plain[:3]
    first = torch.tensor([0, 2, 2])[torch.tensor([1, 0, 2])]      # the original trajectory each final row descends from: [2, 0, 2]
    assert lineage[0].tolist() == first.tolist() == [2, 0, 2]
    # up to the first resampling (the dummy step and imagined step 0) every final row IS its ancestor of the plain run
    assert torch.equal(obss[:, :2], po[first][:, :2]) and torch.equal(rewards[:, :2], pr[first][:, :2]) and torch.equal(actions[:, :2], pa[first][:, :2])
    # rows 0 and 2 are the two children of trajectory 2: one history up to step 0, different draws afterwards
    assert torch.equal(obss[0, :2], obss[2, :2]) and not torch.equal(obss[0, 2], obss[2, 2])
    # final row 1 descends from trajectory 0, which kept its row and its column of uniforms through step 1: still the plain run there
    assert torch.equal(obss[1, :3], po[0, :3]) and torch.equal(rewards[1, :3], pr[0, :3])
    # final row 2 is trajectory 2 in its own row with its own uniforms throughout: the whole plain trajectory
    assert torch.equal(obss[2], po[2]) and torch.equal(rewards[2], pr[2]) and torch.equal(actions[2], pa[2])
    assert torch.isfinite(obss).all() and torch.isfinite(rewards).all()
    del llm._uniforms
