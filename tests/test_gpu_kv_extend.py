"""Extending the kept K / V cache with given tokens and fanning candidates out of it (include/ivg.h ivg_kv_extend,
ivg_generate_fanout; chunk_attn_kernel) on the MI355X: the chunk kernel per query row against fp64 through
ivg_op_chunk_attn (reference, needles and bound: tests/chunk_attn_ref.py), the step-wise route bit for bit against the rollout that
sampled the same tokens (every cache format, both launch profiles), the rewind, the chunk pass's NLL against the fp32 oracle with
ivg_eval_forward as the yardstick, the guard and every refusal through the C ABI, select / extend after an extend, the fan-out bit
for bit against ivg_kv_select + ivg_generate_scored on the kept cache, and the Python entries.
Tiny model throughout, as tests/test_gpu_frame_heads.py (hidden 128, 2 layers, 2 heads of 64, L0 = 514)."""
import ctypes as C

import pytest
import torch

import chunk_attn_ref as R
import frame_heads_ref as FR
from test_gpu_frame_heads import DEV, FLAVOURS, PROFILES, make_head, three_rows
from test_gpu_prefill import prefill_attn

pytestmark = pytest.mark.gpu
OK, INVALID, CAPACITY = 0, -1, -4
SENT = -777.25
CTX = 2


def lib():
    from ivideogpt_amd import _lib
    return _lib.load()


def counters():
    return lib().ivg_debug_counter(b"kv_extend_chunk_rows"), lib().ivg_debug_counter(b"kv_extend_step_rows")


def _p(t):
    from ivideogpt_amd.engine import _ptr
    return _ptr(t)


# ------------------------------------------------------------------------------------------------ 1. the kernel against fp64
def chunk_attn(qkv, kc, vc, out, cos, sin, B, T, heads, pos0, Lmax=R.LMAX, hd=64):
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib().ivg_op_chunk_attn(_p(qkv), _p(kc), _p(vc), _p(out), _p(cos), _p(sin), B, T, heads, hd, Lmax, pos0, 1, st)
    torch.cuda.synchronize()
    return rc


def cache_buffers(inp, B, heads, pos0):
    """kc / vc (B, heads, Lmax, 64) bf16: the given rows in [0, pos0), NaN from pos0 on."""
    kc = torch.full((B, heads, R.LMAX, 64), float("nan"), dtype=torch.bfloat16, device=DEV)
    vc = kc.clone()
    kc[:, :, :pos0] = inp["k_past"].to(DEV)
    vc[:, :, :pos0] = inp["v_past"].to(DEV)
    return kc, vc


@pytest.mark.parametrize("family", ["random", "needle"])
@pytest.mark.parametrize("heads", [2, 12])
@pytest.mark.parametrize("pos0,T", R.CASES, ids=[f"pos{p}-T{t}" for p, t in R.CASES])
def test_chunk_attn_vs_fp64(pos0, T, heads, family):
    """Every query row within its own bound of the fp64 reference; cache rows [0, pos0) and >= pos0 + T bit-unchanged (the latter NaN:
    a mask by arithmetic, or a V row past the chunk reaching the P.V product, would poison whole rows); the appended rows within one
    rounding of the fp64 rotation at positions pos0 + t (K, and q in place) and bit-equal (V); the same bits when run twice; at
    pos0 = 0 flash_prefill_kernel on the same input is within the same bound."""
    B = 3
    inp = R.chunk_inputs(family, B, heads, pos0, T, seed=1000 * pos0 + 10 * heads + T)
    ref, tol = R.attention_fp64(inp, B, heads, pos0, T)
    cos, sin = inp["cos"].to(DEV), inp["sin"].to(DEV)
    runs = []
    for _ in range(2):
        qkv = inp["qkv"].to(DEV)
        kc, vc = cache_buffers(inp, B, heads, pos0)
        out = torch.full((B * T, heads * 64), float("nan"), dtype=torch.bfloat16, device=DEV)
        assert chunk_attn(qkv, kc, vc, out, cos, sin, B, T, heads, pos0) == OK
        runs.append((qkv, kc, vc, out))
    qkv, kc, vc, out = runs[0]
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16)), "two runs of one case differ"
    got = out.cpu().double().view(B, T, heads, 64).permute(0, 2, 1, 3)
    assert torch.isfinite(got).all(), f"{(~torch.isfinite(got)).any(-1).sum().item()} rows are not finite"
    err = (got - ref).abs().amax(-1)
    ratio = err / tol
    worst = divmod(int(ratio.argmax()), T)
    msg = (f"{family}: worst row (b*heads+h, t) = {worst}: err {err.flatten()[ratio.argmax()].item():.3e} vs bound "
           f"{tol.flatten()[ratio.argmax()].item():.3e} (err / bound {ratio.max().item():.3f}); {(ratio > 1).sum().item()} rows beyond")
    print(msg)
    assert (ratio <= 1).all(), msg
    # the cache: kept rows and rows past the chunk untouched, the chunk's rows appended
    assert torch.equal(kc[:, :, :pos0].cpu().view(torch.int16), inp["k_past"].view(torch.int16)), "kc rows [0, pos0) changed"
    assert torch.equal(vc[:, :, :pos0].cpu().view(torch.int16), inp["v_past"].view(torch.int16)), "vc rows [0, pos0) changed"
    assert torch.isnan(kc[:, :, pos0 + T:]).all() and torch.isnan(vc[:, :, pos0 + T:]).all(), "cache rows >= pos0 + T must not be written"
    t0 = inp["qkv"].view(B, T, 3, heads, 64)
    t1 = qkv.cpu().view(B, T, 3, heads, 64)
    pos = pos0 + torch.arange(T)
    for name, x0, gotx in (("q (in place)", t0[:, :, 0], t1[:, :, 0]), ("kc rows [pos0, pos0 + T)", t0[:, :, 1], kc[:, :, pos0:pos0 + T].cpu().permute(0, 2, 1, 3))):
        ex, scale = R.rope_exact_at(x0, inp["cos"], inp["sin"], pos)
        e = (gotx.double() - ex).abs()
        bound = 2.0 ** -7 * ex.abs() + 2.0 ** -22 * scale   # one rounding to bf16 + the fp32 rotation's own error (check_append's bound)
        assert torch.isfinite(gotx).all() and (e <= bound).all(), f"{name}: {(e > bound).sum().item()} elements beyond one rounding"
    assert torch.equal(t1[:, :, 2], t0[:, :, 2]), "v in qkv must not change"
    assert torch.equal(vc[:, :, pos0:pos0 + T].cpu(), t0[:, :, 2].permute(0, 2, 1, 3)), "vc rows [pos0, pos0 + T) must equal v bit for bit"
    if pos0 == 0:
        qkv2 = inp["qkv"].to(DEV)
        kc2 = torch.full((B, heads, R.LMAX, 64), float("nan"), dtype=torch.bfloat16, device=DEV)
        vt2 = torch.full((B, heads, 64, 64), float("nan"), dtype=torch.bfloat16, device=DEV)
        out2 = torch.full_like(out, float("nan"))
        assert prefill_attn(qkv2, kc2, kc2.clone(), vt2, out2, cos, sin, B, T, heads, 64, R.LMAX, torch.bfloat16) == 0
        got2 = out2.cpu().double().view(B, T, heads, 64).permute(0, 2, 1, 3)
        r2 = ((got2 - ref).abs().amax(-1) / tol).max().item()
        print(f"flash_prefill on the same input: err / bound {r2:.3f}")
        assert r2 <= 1


# ------------------------------------------------------------------------------------------------ model-level helpers (C ABI)
def engine_of(head, B, act_T):
    return head.llm._ensure(B, act_T)


def scored(eng, prompt, n_new, actions, uni, kept=0, group=1, fan=False, hid_dtype=None, expect=OK):
    """ivg_generate_scored (fan: ivg_generate_fanout with `group` candidates per prompt row) with frame rewards, token scores and,
    with hid_dtype, frame hidden states -> (ids (B, L0 + n_new), rewards (B, F), hidden (B, F, H) or None, scores (B, n_new, 3))."""
    L0 = prompt.shape[1]
    B = prompt.shape[0] * group if fan else prompt.shape[0]
    F = n_new // 17
    ids = torch.full((B, L0 + n_new), -12345, dtype=torch.int64, device=DEV)
    fr = torch.full((B, F), SENT, dtype=torch.float32, device=DEV)
    hid = torch.full((B, F, 128), SENT, dtype=hid_dtype, device=DEV) if hid_dtype is not None else None
    ts = torch.full((B, n_new, 3), SENT, dtype=torch.float32, device=DEV)
    act_T = actions.shape[1] if actions is not None else 0
    with eng.stream() as s:
        if fan:
            rc = eng.lib.ivg_generate_fanout(eng.h, _p(prompt), prompt.stride(0), prompt.shape[0], group, L0, n_new, _p(actions), act_T, CTX, _p(uni), 100, 0,
                                             _p(ids), _p(fr), _p(hid), _p(ts), s)
        else:
            rc = eng.lib.ivg_generate_scored(eng.h, _p(prompt), prompt.stride(0), B, L0, n_new, _p(actions), act_T, CTX, _p(uni), 100, group, kept, 0,
                                             _p(ids), _p(fr), _p(hid), _p(ts), s)
    torch.cuda.synchronize()
    assert rc == expect, f"status {rc}, expected {expect}: {eng.lib.ivg_last_error(eng.h)}"
    if rc != OK:
        assert (ids == -12345).all() and (fr == SENT).all() and (ts == SENT).all() and (hid is None or (hid == SENT).all()), "a refused call wrote an output"
    return ids, fr, hid, ts


def extend(eng, prompt, keep, actions, nll=None, B=None, L0=None, ctx=CTX):
    act_T = actions.shape[1] if actions is not None else 0
    with eng.stream() as s:
        rc = eng.lib.ivg_kv_extend(eng.h, _p(prompt), prompt.stride(0), B or prompt.shape[0], keep, L0 or prompt.shape[1], _p(actions), act_T, ctx, _p(nll), s)
    torch.cuda.synchronize()
    return rc


def assert_same(a, b, what):
    for x, y, name in zip(a, b, ("tokens", "frame rewards", "frame hidden states", "token scores")):
        if x is None:
            continue
        assert torch.equal(x, y), f"{what}: {name} differ ({(x != y).sum().item()} elements)"


# ------------------------------------------------------------------------------------------------ 2. route (b) is exact; the rewind
@PROFILES
@pytest.mark.parametrize("flavour", list(FLAVOURS))
def test_stepwise_extend_equals_the_rollout_that_sampled_the_tokens(flavour, lds_kb, switches):
    """R1 = one 51-token call.  R2 = a 17-token call with the same first uniforms, then ivg_kv_extend with R1's next 17 tokens as given
    ones (keep_len 530, L0 548), then a 17-token continue on R1's uniform columns 34 ..: the decode steps with given inputs append
    bit for bit what R1's own steps appended, so R2's tokens, frame rewards and token scores equal R1's columns bit for bit.  Then the
    rewind: back to 530 kept positions (nothing launched, the counters stay) and a continue that reproduces R1's tokens [531, 548)."""
    dtype, kv = FLAVOURS[flavour]
    if flavour == "bf16":
        switches(IVG_KV_EXTEND_CHUNK="0")
    head = make_head(dtype, lds_kb, kv=kv)
    ids, table, uni = three_rows()
    eng = engine_of(head, 3, table.shape[1])
    r1 = scored(eng, ids, 51, table, uni)
    a = scored(eng, ids, 17, table, uni[:, :17].contiguous())
    assert_same((a[0], a[1], None, a[3]), (r1[0][:, :531], r1[1][:, :1], None, r1[3][:, :17]), "first 17 tokens")
    full = r1[0][:, :548].contiguous()
    c0 = counters()
    assert extend(eng, full, 530, table) == OK, eng.lib.ivg_last_error(eng.h)
    assert counters() == (c0[0], c0[1] + 3 * 17), "3 x 17 rows through the decode steps, none through the chunk pass"
    b = scored(eng, full, 17, table, uni[:, 34:51].contiguous(), kept=1)
    assert_same((b[0], b[1], None, b[3]), (r1[0], r1[1][:, 2:3], None, r1[3][:, 34:51]), "continue after the extend")
    # rewind: the cache now holds 564 positions; keep 530 of them
    c0 = counters()
    assert extend(eng, r1[0][:, :531].contiguous(), 530, table) == OK, eng.lib.ivg_last_error(eng.h)
    assert counters() == c0, "a rewind launches nothing"
    c = scored(eng, r1[0][:, :531].contiguous(), 17, table, uni[:, 17:34].contiguous(), kept=1)
    assert torch.equal(c[0], r1[0][:, :548]), "continue after the rewind: tokens [531, 548) differ from R1's"
    assert torch.equal(c[3], r1[3][:, 17:34]) and torch.equal(c[1], r1[1][:, 1:2])


# ------------------------------------------------------------------------------------------------ 3. route (a) at model level
def oracle_nll(ref, full, table, lo, hi):
    """-log softmax(z_p)[full[:, p + 1]] for p in [lo, hi) from the fp32 CPU oracle's teacher-forced logits."""
    logits, _ = FR.teacher_forced(ref["sd"], ref["cfg"], full.cpu(), table.cpu(), CTX)
    lp = torch.log_softmax(logits[:, lo:hi].double(), -1)
    return -lp.gather(-1, full.cpu()[:, lo + 1:hi + 1, None]).squeeze(-1)


def test_chunk_pass_nll_vs_oracle(switches):
    """bf16.  The NLL of the 17 given tokens from the chunk pass, and ivg_eval_forward's token_nll at the same positions, both against
    the fp32 oracle: max |nll_a - oracle| <= 2 max |nll_evalforward - oracle| + 1e-3 (both are bf16 through the same GEMMs; they differ
    in the attention kernel and in which kept rows came from decode steps; 1e-3 is the project's parity bar).  Precondition: on the
    oracle, shifting the action rows by one slot moves some NLL by more than ten times that tolerance, so a wrong slot or row fails.
    The step-wise route on the same engine and inputs agrees within the same tolerance; the extended cache is then continued."""
    ref = FR.fixture_reference()
    head = make_head("bf16")
    ids, table, uni = three_rows()
    table = (table * 3.0).contiguous()
    eng = engine_of(head, 3, table.shape[1])
    r1 = scored(eng, ids, 51, table, uni)
    full = r1[0][:, :548].contiguous()
    want = oracle_nll(ref, full, table, 530, 547)
    # yardstick: the eval forward over the whole row
    nll_all = torch.zeros(3, 548, device=DEV)
    rows = torch.zeros(3, 2, device=DEV)
    eng.eval_forward(full, full, nll_all, rows, actions=table, ctx=CTX)
    torch.cuda.synchronize()
    e_ef = (nll_all[:, 530:547].cpu().double() - want).abs().max().item()
    tol = 2 * e_ef + 1e-3
    shifted = oracle_nll(ref, full, torch.roll(table, 1, 1), 530, 547)
    moved = (shifted - want).abs().max().item()
    assert moved > 10 * tol, f"precondition: a shifted action row moves the oracle's NLL by only {moved:.3e} (tolerance {tol:.3e})"
    got = {}
    for route, env in (("chunk", None), ("steps", "0")):
        switches(IVG_KV_EXTEND_CHUNK=env)
        scored(eng, ids, 17, table, uni[:, :17].contiguous())
        nll = torch.full((3, 17), SENT, device=DEV)
        c0 = counters()
        assert extend(eng, full, 530, table, nll) == OK, eng.lib.ivg_last_error(eng.h)
        assert counters() == ((c0[0] + 51, c0[1]) if route == "chunk" else (c0[0], c0[1] + 51)), f"{route}: the wrong route ran"
        got[route] = nll.cpu().double()
        out = scored(eng, full, 17, table, uni[:, 34:51].contiguous(), kept=1)
        assert torch.equal(out[0][:, :548], full)
    e_a, e_b = (got["chunk"] - want).abs().max().item(), (got["steps"] - want).abs().max().item()
    e_ab = (got["chunk"] - got["steps"]).abs().max().item()
    print(f"NLL vs fp32 oracle: chunk pass {e_a:.3e}, decode steps {e_b:.3e}, eval forward {e_ef:.3e}; chunk vs steps {e_ab:.3e}; tolerance {tol:.3e}; "
          f"shifted action row moves the oracle by {moved:.3e}")
    assert e_a <= tol, f"chunk pass NLL misses the oracle by {e_a:.3e} (eval forward: {e_ef:.3e})"
    assert e_ab <= tol, f"chunk pass and decode steps differ by {e_ab:.3e}"


# ------------------------------------------------------------------------------------------------ 4. guard and refusals
def test_refusals_leave_outputs_and_kept_cache_untouched():
    head, twin = make_head(), make_head()
    ids, table, uni = three_rows()
    eng, teng = engine_of(head, 3, table.shape[1]), engine_of(twin, 3, table.shape[1])
    u0, v = uni[:, :17].contiguous(), uni[:, 17:34].contiguous()
    nll = torch.full((3, 64), SENT, device=DEV)
    assert extend(eng, ids, 500, table, nll) == INVALID and (nll == SENT).all(), "a fresh engine holds no kept cache"
    emb = torch.empty(3, 514, 128, device=DEV)
    eng.embed_tokens(ids, emb)
    eng.generate_embeds(emb, 3, torch.empty(3, 3, dtype=torch.int64, device=DEV))
    assert extend(eng, ids, 500, None, nll, ctx=1) == INVALID and (nll == SENT).all(), "a cache built from embeddings is out of scope"
    grown = scored(eng, ids, 17, table, u0)[0].contiguous()            # (3, 531); the kept cache holds 530 positions
    want = scored(teng, scored(teng, ids, 17, table, u0)[0].contiguous(), 17, table, v, kept=1)
    full = want[0].contiguous()                                          # (3, 548)
    other = full.clone(); other[1, 520] = (other[1, 520] + 1) % 100
    act2 = table.clone(); act2[2, 1, 0] += 1.0                           # the row baked into the cached slot at position 513
    wide = torch.zeros(3, 5000, dtype=torch.int64, device=DEV); wide[:, :531] = grown
    cases = {
        "another B": (INVALID, dict(prompt=full[:2].contiguous(), keep=530, actions=table[:2].contiguous())),
        "keep_len 0": (INVALID, dict(prompt=full, keep=0, actions=table)),
        "keep_len above the kept length": (INVALID, dict(prompt=full, keep=531, actions=table)),
        "keep_len above L0 - 1": (INVALID, dict(prompt=full, keep=530, actions=table, L0=530)),
        "another token": (INVALID, dict(prompt=other, keep=530, actions=table)),
        "another cached action row": (INVALID, dict(prompt=full, keep=530, actions=act2)),
        "built with actions, extended without": (INVALID, dict(prompt=full, keep=530, actions=None)),
        "another context length": (INVALID, dict(prompt=full, keep=530, actions=table, ctx=1)),
        "another action-table shape": (INVALID, dict(prompt=full, keep=530, actions=table[:, :4].contiguous())),
        "action table too short for the slots": (INVALID, dict(prompt=full, keep=530, actions=table[:, :2].contiguous())),
        "beyond the cache": (CAPACITY, dict(prompt=wide, keep=530, actions=table)),
    }
    c0 = counters()
    for what, (status, kw) in cases.items():
        rc = extend(eng, kw["prompt"], kw["keep"], kw["actions"], nll, L0=kw.get("L0"), ctx=kw.get("ctx", CTX))
        assert rc == status, f"{what}: status {rc}, expected {status}"
        assert (nll == SENT).all(), f"{what}: the output was written"
        assert counters() == c0
        got = scored(eng, grown, 17, table, v, kept=1)                  # the refusal left the kept cache usable: same bits as the twin
        assert_same(got, want, f"continue after the refusal of {what}")
        scored(eng, ids, 17, table, u0)                                 # (the kept cache of 530 positions again)
    # after a successful extend the OLD prompt is refused, the extended one accepted
    assert extend(eng, full, 530, table) == OK
    scored(eng, grown, 17, table, v, kept=1, expect=INVALID)
    scored(eng, full, 17, table, uni[:, 34:51].contiguous(), kept=1)


# ------------------------------------------------------------------------------------------------ 5. second-order state
def test_select_and_extend_after_an_extend():
    head = make_head()
    ids, table, _ = three_rows()
    uni = torch.rand(3, 52, generator=torch.Generator().manual_seed(29)).to(DEV)
    eng = engine_of(head, 3, table.shape[1])
    r1 = scored(eng, ids, 52, table, uni)                               # the decode steps are exact on this engine: R1 is the yardstick
    full, longer = r1[0][:, :548].contiguous(), r1[0][:, :565].contiguous()
    # extend, select, continue: children 0 and 1 of row 2, child 2 of row 0, each on its parent's uniforms
    scored(eng, ids, 17, table, uni[:, :17].contiguous())
    assert extend(eng, full, 530, table) == OK
    parents = torch.tensor([2, 2, 0], device=DEV)
    head.select_kept_cache([2, 2, 0])
    out = scored(eng, full[parents].contiguous(), 17, table[parents].contiguous(), uni[parents, 34:51].contiguous(), kept=1)
    assert torch.equal(out[0], r1[0][parents, :565]) and torch.equal(out[3], r1[3][parents, 34:51])
    # extend, extend, continue
    scored(eng, ids, 17, table, uni[:, :17].contiguous())
    assert extend(eng, full, 530, table) == OK
    nll = torch.full((3, 17), SENT, device=DEV)
    assert extend(eng, longer, 547, table, nll) == OK
    assert torch.isfinite(nll).all() and (nll != SENT).all()
    # R1 SAMPLED the tokens at positions 548 .. 563 (score columns 34 .. 49) and reported their log-probabilities from the same fp32
    # logits rows: the same quantity from two fp32 kernels (each within 1e-4 of fp64, the bar of tests/test_gpu_prefill.py's CE test)
    d = (nll[:, :16] + r1[3][:, 34:50, 0]).abs().max().item()
    print(f"NLL of the given tokens vs the rollout's own log-probabilities: {d:.3e}")
    assert d <= 2e-4, "NLL of a given token differs from the log-probability the rollout reported for it"
    out = scored(eng, longer, 1, table, uni[:, 51:52].contiguous(), kept=1)
    assert torch.equal(out[0], r1[0]), "the token decided after two extends differs from R1's"


# ------------------------------------------------------------------------------------------------ 6. fan-out
@PROFILES
@pytest.mark.parametrize("flavour", list(FLAVOURS))
def test_fanout_equals_select_then_scored_bitwise(flavour, lds_kb):
    """3 kept histories x 2 candidates from the kept cache against the route that exists without the entry: grow the kept cache to 6
    rows with ivg_kv_select and run ivg_generate_scored on it -- the shared-context attention reads the same bytes in the same order.
    Afterwards the kept cache is what it was: a continue of the 3 histories equals that of an engine that never fanned out, and a
    second fan-out gives the same bits."""
    dtype, kv = FLAVOURS[flavour]
    head, twin = make_head(dtype, lds_kb, kv=kv), make_head(dtype, lds_kb, kv=kv)
    ids, table, uni = three_rows()
    eng, teng = engine_of(head, 6, table.shape[1]), engine_of(twin, 6, table.shape[1])
    hdt = head.llm.torch_dtype
    u0, v = uni[:, :17].contiguous(), uni[:, 17:34].contiguous()
    g = torch.Generator().manual_seed(31)
    parents = torch.tensor([0, 0, 1, 1, 2, 2], device=DEV)
    table6 = torch.randn(6, table.shape[1], table.shape[2], generator=g).to(DEV)
    table6[:, :2] = table[parents, :2]                                   # (the row of the cached slot: the select route compares it)
    uni6 = torch.rand(6, 17, generator=g).to(DEV)
    grown = scored(eng, ids, 17, table, u0)[0].contiguous()
    fan = scored(eng, grown, 17, table6, uni6, group=2, fan=True, hid_dtype=hdt)
    assert fan[0].shape == (6, 548) and torch.equal(fan[0][:, :531], grown[parents])
    again = scored(eng, grown, 17, table6, uni6, group=2, fan=True, hid_dtype=hdt)
    assert_same(again, fan, "second fan-out")
    cont = scored(eng, grown, 17, table, v, kept=1, hid_dtype=hdt)       # the kept cache of the 3 histories is still there
    # the twin: never fans out
    tg = scored(teng, ids, 17, table, u0)[0].contiguous()
    assert torch.equal(tg, grown)
    assert_same(cont, scored(teng, tg, 17, table, v, kept=1, hid_dtype=hdt), "continue after the fan-outs")
    scored(teng, ids, 17, table, u0)
    twin.select_kept_cache([0, 0, 1, 1, 2, 2])
    sel = scored(teng, grown[parents].contiguous(), 17, table6, uni6, kept=1, hid_dtype=hdt)
    assert_same(fan, sel, "fan-out vs select + scored")


def test_fanout_refusals():
    head = make_head()
    ids, table, uni = three_rows()
    eng = engine_of(head, 6, table.shape[1])
    table6, uni6 = table.repeat_interleave(2, 0).contiguous(), uni[:, :17].repeat_interleave(2, 0).contiguous()
    scored(eng, ids, 17, table6, uni6, group=2, fan=True, expect=INVALID)            # a fresh engine: no kept cache
    grown = scored(eng, ids, 17, table, uni[:, :17].contiguous())[0].contiguous()
    other = grown.clone(); other[2, 7] = (other[2, 7] + 1) % 100
    scored(eng, other, 17, table6, uni6, group=2, fan=True, expect=INVALID)          # another token
    scored(eng, grown[:2].contiguous(), 17, table6[:4].contiguous(), uni6[:4].contiguous(), group=2, fan=True, expect=INVALID)   # another number of histories
    scored(eng, ids, 17, table6, uni6, group=2, fan=True, expect=INVALID)            # another length
    t9, u9 = table.repeat_interleave(3, 0).contiguous(), uni[:, :17].repeat_interleave(3, 0).contiguous()
    scored(eng, grown, 17, t9, u9, group=3, fan=True, expect=CAPACITY)               # 9 candidates, a cache chunk of 6
    scored(eng, grown, 1000, table6, None, group=2, fan=True, expect=CAPACITY)       # beyond the cache length
    out = scored(eng, grown, 17, table6, uni6, group=2, fan=True)                    # the refusals left the kept cache usable
    assert torch.equal(out[0][:, :531], grown.repeat_interleave(2, 0))
    scored(eng, grown, 17, table, uni[:, 17:34].contiguous(), kept=1)


# ------------------------------------------------------------------------------------------------ 7. Python
def test_python_entries_match_the_c_level():
    head, twin = make_head(), make_head()
    ids, table, uni = three_rows()
    eng, teng = engine_of(head, 6, table.shape[1]), engine_of(twin, 6, table.shape[1])
    u0 = uni[:, :17].contiguous()
    with pytest.raises(ValueError):
        make_head().extend_kept_cache(ids, action=table, keep=500)
    with pytest.raises(ValueError):
        make_head().fan_out(ids, 2, action=table.repeat_interleave(2, 0), max_new_tokens=16)
    r1 = scored(teng, ids, 51, table, uni)
    full = r1[0][:, :548].contiguous()
    # extend
    scored(teng, ids, 17, table, u0)
    want = torch.full((3, 17), SENT, device=DEV)
    assert extend(teng, full, 530, table, want) == OK
    grown = head.generate(ids, do_sample=True, max_new_tokens=17, action=table, uniforms=u0)
    assert head.extend_kept_cache(full, action=table, keep=530) is None
    head.generate(ids, do_sample=True, max_new_tokens=17, action=table, uniforms=u0)
    nll = head.extend_kept_cache(full, action=table, keep=530, return_nll=True)
    assert nll.shape == (3, 17) and torch.equal(nll, want)
    assert head.extend_kept_cache(grown, action=table, keep=530, return_nll=True).shape == (3, 0)      # rewind
    with pytest.raises(ValueError, match="different prefix"):
        head.extend_kept_cache(full.roll(1, 0), action=table, keep=530)
    with pytest.raises(ValueError):
        head.extend_kept_cache(full, action=table)
    # fan out of the rewound cache: rows b * 2 + k
    g = torch.Generator().manual_seed(37)
    table6 = torch.randn(6, table.shape[1], table.shape[2], generator=g).to(DEV)
    uni6 = torch.rand(6, 17, generator=g).to(DEV)
    scored(teng, ids, 17, table, u0)
    want = scored(teng, grown, 17, table6, uni6, group=2, fan=True, hid_dtype=torch.float32)
    out, fr, fh, sc = head.fan_out(grown, 2, action=table6, do_sample=True, max_new_tokens=16, uniforms=uni6, return_reward="frames",
                                   output_frame_hidden_states=True, output_token_scores=True)
    assert torch.equal(out, want[0][:, :547]) and torch.equal(fr, want[1]) and torch.equal(fh, want[2])
    for k, t in enumerate(sc):
        assert torch.equal(t, want[3][:, :16, k])
    plain = head.fan_out(grown, 2, action=table6, do_sample=True, max_new_tokens=17, uniforms=uni6)
    assert torch.equal(plain, want[0])
    with pytest.raises(ValueError):
        head.fan_out(grown, 3, action=table6.repeat(2, 1, 1)[:9], max_new_tokens=17)     # 9 candidates, an engine built for 6
    with pytest.raises(ValueError):
        head.fan_out(ids, 2, action=table6, max_new_tokens=17)                            # not what the kept cache holds
    cont = head.generate(grown, do_sample=True, max_new_tokens=17, action=table, uniforms=uni[:, 17:34].contiguous(), reuse_cache=True)
    assert torch.equal(cont, full[:, :548])
