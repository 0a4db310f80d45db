"""Scores of sampled tokens under the filtered (temperature / top-k / top-p) distribution (include/ivg.h ivg_generate_filtered;
filtered_scores_kernel inside the decode steps) on the MI355X: the kernel through ivg_op_filtered_scores against the fp64 reference of
tests/filtered_scores_ref.py on its whole case table, the in-engine scores against the teacher-forced oracle, the exact statements (the
drawn token is in the set, forced columns, kept_logmass 0 without a filter), bit for bit against the step-by-step route, row orders of
shared contexts and fan-outs, the untouched off path, the refusals through the C ABI with guarded buffers, and ``VideoPredictor``'s
``return_proposal_logprob``.  The tiny model and the rows of tests/test_gpu_token_scores.py: B = 3, L0 = 514, 51 new tokens."""
import ctypes as C

import numpy as np
import pytest
import torch

import filtered_scores_ref as R
import frame_heads_ref as FR
import test_gpu_token_scores as T

pytestmark = pytest.mark.gpu
DEV = T.DEV
OK, INVALID, CAPACITY = 0, -1, -4
L0, FORCED, SAMPLED = T.L0, T.FORCED, T.SAMPLED
COUNTERS = (b"filtered_scores", b"token_scores", b"frame_heads", b"decode_gemm_gen2", b"decode_gemm_gen3", b"decode_attn8", b"decode_attn24")


def counter(name=b"filtered_scores"):
    return T.lib().ivg_debug_counter(name)


def counters():
    return [counter(n) for n in COUNTERS]


def stack(fs):
    """FilteredTokenScores -> (B, n, 4) float64 numpy"""
    return torch.stack(list(fs), -1).double().cpu().numpy()


# ------------------------------------------------------------------------------------------------ 1. the kernel against fp64
def op_filtered(z, tok, settings):
    from ivideogpt_amd.engine import _ptr
    top_k, top_p, temperature, greedy = settings
    B, V = z.shape
    zd, td = torch.from_numpy(np.array(z)).to(DEV), torch.from_numpy(np.array(tok)).to(DEV)
    out = T.Guarded(B * 4, torch.float32, T.SENT_F)
    rc = T.lib().ivg_op_filtered_scores(_ptr(zd), _ptr(td), B, V, int(top_k), C.c_float(temperature), C.c_float(top_p), int(greedy), _ptr(out.view),
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == OK and out.guards_intact(), "a guard word around `out` was overwritten"
    return out.view.view(B, 4).cpu().numpy().astype(np.float64)


@pytest.mark.parametrize("case", list(R.CASES))
def test_kernel_against_fp64(case):
    """Every row of the table: ``support`` exactly the reference's on rows not flagged ``near``, the three real outputs within 1e-4
    absolute, NaN and infinities alike in kind."""
    c = R.build(case)
    got = op_filtered(c["z"], c["tok"], c["settings"])
    want = c["want"]
    fin = np.isfinite(want[:, :3])
    print(f"{case}: worst |kernel - fp64| = {np.abs(got[:, :3][fin] - want[:, :3][fin]).max():.2e}; support {got[:, 3].astype(int).tolist()}, "
          f"{int(c['near'].sum())} rows near")
    assert c["near"].sum() * 100 <= len(want)
    ok = R.agrees(got, want, c["near"])
    for b in range(len(ok)):
        assert ok[b], f"{case} row {R.ROW_KINDS[b]}: {got[b]} against fp64 {want[b]}"
    again = op_filtered(c["z"], c["tok"], c["settings"])
    assert np.array_equal(got, again, equal_nan=True), "two launches on the same rows differ"
    if not c["settings"][3] and (c["settings"][0] <= 0 or c["settings"][0] >= c["z"].shape[1]) and c["settings"][1] >= 1.0:
        assert (got[:, 2] == 0).all(), "nothing is filtered, yet kept_logmass is not exactly 0"


def test_kernel_special_rows_and_refusals():
    from ivideogpt_amd.engine import _ptr
    z, tok, s = R.nonfinite_case()
    assert np.isnan(op_filtered(z, tok, s)).all(), "a NaN, a +inf or a row of -inf: NaN in all four"
    z, tok, s = R.merge_case()
    want, near, *_ = R.reference(z, tok, *s)
    got = op_filtered(z, tok, s)
    assert got[0, 3] == 101 and R.agrees(got, want, near).all(), "the tie the temperature division makes at the top-k threshold is kept"
    # greedy ignores the three settings: the bits of the call with none of them
    c = R.build("V16386_greedy")
    assert np.array_equal(op_filtered(c["z"], c["tok"], c["settings"]), op_filtered(c["z"], c["tok"], (0, 1.0, 1.0, True)), equal_nan=True)
    zd, td = torch.zeros(1, 8, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV)
    out = T.Guarded(4, torch.float32, T.SENT_F)
    for V, top_p, temperature in ((0, 0.9, 1.0), (256 * 72 + 1, 0.9, 1.0), (8, 1.5, 1.0), (8, -0.1, 1.0), (8, 0.9, 0.0), (8, 0.9, float("nan"))):
        rc = T.lib().ivg_op_filtered_scores(_ptr(zd), _ptr(td), 1, V, 100, C.c_float(temperature), C.c_float(top_p), 0, _ptr(out.view), None)
        assert rc == INVALID and out.untouched(), (V, top_p, temperature)


# ------------------------------------------------------------------------------------------------ 2. in the engine against the oracle
def oracle_filtered(tokens, table, n, top_k, top_p, temperature, greedy=False, tol=1e-4, start=L0):
    """The teacher-forced oracle over the finished rows, whose new tokens begin at column ``start``: -> (reference (B, n, 4) with the
    forced columns zero, near (B, n) at ``tol`` -- a column whose survivor set a logit error of about ``tol`` may change, as
    tests/test_gpu_top_p.py counts them --, entropy sensitivity of the filtered rows (B, n), the tempered raw log-probability of the
    produced tokens (B, n))."""
    ref = FR.fixture_reference()
    logits, _ = FR.teacher_forced(ref["sd"], ref["cfg"], tokens.cpu(), table.cpu(), int(ref["g"]["ctx"]))
    rows = logits[:, start - 1:start - 1 + n].numpy()
    new = tokens[:, start:start + n].cpu().numpy()
    want, near, sens, raw = [], [], [], []
    for b in range(rows.shape[0]):
        w, _ = R.reference_columns(rows[b], new[b], top_k, top_p, temperature, greedy, R.PER)
        _, nr, _, survive, _ = R.reference(rows[b], new[b], top_k, top_p, temperature, greedy, tol=tol)
        l = torch.from_numpy(rows[b]) if greedy or temperature == 1.0 else torch.from_numpy(rows[b]) / torch.tensor(temperature, dtype=torch.float32)
        filt = np.where(survive, l.double().numpy(), -np.inf)
        want.append(w); near.append(nr); sens.append(R.entropy_sensitivity(filt))
        raw.append(torch.log_softmax(l.double(), -1).gather(1, torch.from_numpy(new[b])[:, None])[:, 0].numpy())
    return np.stack(want), np.stack(near), np.stack(sens), np.stack(raw)


@T.PROFILES
def test_filtered_scores_match_the_teacher_forced_oracle(lds_kb):
    """Sampled with uniforms and actions under top_k 100, top_p 0.9, temperature 0.7, fp32: per column against the fp64 reference on the
    oracle's logits of the same tokens, with the bounds of tests/test_gpu_token_scores.py (a 1e-3 logits parity: 2e-3 on the two
    log-quantities, 1e-3 * sum p |log p + H| + 1e-4 on the entropy) and ``support`` exact, on the columns whose survivor set a logit
    error of 1e-4 cannot change; the exact statements on every column."""
    head = T.make_head(lds_kb=lds_kb)
    ids, table, uni = T.three_rows()
    kw = dict(do_sample=True, top_k=100, top_p=0.9, temperature=0.7, max_new_tokens=51, action=table, uniforms=uni)
    c0, t0 = counter(), counter(b"token_scores")
    out, fs = head.generate(ids, output_filtered_scores=True, **kw)
    assert counter() - c0 == 51 and counter(b"token_scores") == t0, "one launch per step that ran the sampler, and none of token_scores_kernel"
    assert type(fs).__name__ == "FilteredTokenScores" and fs._fields == R.FIELDS
    assert all(t.shape == (3, 51) and t.dtype == torch.float32 for t in fs)
    assert torch.equal(out, head.generate(ids, **kw)), "the call with filtered scores decides other tokens than the plain one"
    got = stack(fs)
    # exact: the drawn token is in the set the kernel computes; forced columns
    assert np.isfinite(got[:, SAMPLED, 0]).all() and (got[:, SAMPLED, 3] >= 1).all(), "a sampled token outside the kernel's survivor set"
    assert (got[:, FORCED] == 0).all(), "a forced column is not exactly 0"
    assert (got[..., 0] <= 0).all() and (got[..., 2] <= 0).all() and (got[:, SAMPLED, 3] <= 100).all()
    want, near, sens, raw = oracle_filtered(out, table, 51, 100, 0.9, 0.7)
    cols = np.array(SAMPLED)
    use = ~near[:, cols]
    print(f"lds_kb {lds_kb}: {int(use.sum())} of {use.size} sampled columns compared ({int((~use).sum())} within 1e-4 of the nucleus boundary)")
    assert use.sum() * 2 >= use.size
    d = np.abs(got - want)[:, cols]
    e_bound = 1e-3 * sens[:, cols] + 1e-4
    print(f"|d logprob| {d[..., 0][use].max():.2e}, |d kept_logmass| {d[..., 2][use].max():.2e} (bound 2e-3); |d entropy| {d[..., 1][use].max():.2e} "
          f"(largest ratio {(d[..., 1] / e_bound)[use].max():.3f}); support differs on {int((d[..., 3][use] != 0).sum())}")
    assert d[..., 0][use].max() <= 2e-3 and d[..., 2][use].max() <= 2e-3
    assert (d[..., 1] <= e_bound)[use].all()
    assert (d[..., 3][use] == 0).all(), "support differs from the reference away from the boundary"
    # p_raw = p_filtered * kept share, against the oracle's tempered log-softmax (on every sampled column: the sum does not depend on S)
    dr = np.abs(got[:, cols, 0] + got[:, cols, 2] - raw[:, cols]).max()
    print(f"|filtered_logprob + kept_logmass - tempered raw logprob (oracle)| = {dr:.2e}")
    assert dr <= 2e-3
    flp, fen = fs.per_frame()
    assert flp.shape == fen.shape == (3, 3)
    for i in range(3):
        assert np.abs(flp[:, i].double().cpu().numpy() - got[:, 17 * i:17 * i + 16, 0].sum(-1)).max() < 1e-4
        assert np.abs(fen[:, i].double().cpu().numpy() - got[:, 17 * i:17 * i + 16, 1].mean(-1)).max() < 1e-5


def test_against_token_scores_of_the_same_rows():
    """Both kernels read the same row in the same call.  temperature 1: filtered_logprob + kept_logmass is TokenScores.logprob within
    1e-4.  Without any filter (top_k 0, top_p 1) the first two outputs are TokenScores' within 1e-4 and kept_logmass is exactly 0;
    greedy likewise, whatever the settings."""
    head = T.make_head()
    ids, table, uni = T.three_rows(5)
    out, ts, fs = head.generate(ids, do_sample=True, top_k=100, top_p=0.9, max_new_tokens=51, action=table, uniforms=uni, output_token_scores=True,
                                output_filtered_scores=True)
    s = np.array(SAMPLED)
    d = (fs.logprob + fs.kept_logmass - ts.logprob)[:, s].abs().max().item()
    print(f"top_k 100, top_p 0.9: |filtered_logprob + kept_logmass - logprob| = {d:.2e}")
    assert d <= R.BOUND and (fs.kept_logmass[:, s] < 0).all() and (fs.logprob[:, s] >= ts.logprob[:, s] - R.BOUND).all()
    V = FR.fixture_reference()["cfg"]["vocab_size"]
    for kw in (dict(do_sample=True, top_k=0, top_p=1.0, uniforms=uni), dict(do_sample=False, top_k=100, top_p=0.9, temperature=0.7)):
        out, ts, fs = head.generate(ids, max_new_tokens=51, action=table, output_token_scores=True, output_filtered_scores=True, **kw)
        d0, d1 = (fs.logprob - ts.logprob).abs().max().item(), (fs.entropy - ts.entropy).abs().max().item()
        print(f"{'sampled, no filter' if kw['do_sample'] else 'greedy'}: |d logprob| {d0:.2e}, |d entropy| {d1:.2e}")
        assert d0 <= R.BOUND and d1 <= R.BOUND
        assert (fs.kept_logmass == 0).all() and (fs.support[:, s] == V).all() and (fs.support[:, FORCED] == 0).all()


# ------------------------------------------------------------------------------------------------ 3. bitwise: one call == step by step
def test_one_call_equals_three_kept_cache_calls_bitwise():
    head = T.make_head()
    ids, table, uni = T.three_rows()
    kw = dict(do_sample=True, top_k=100, top_p=0.9, temperature=0.7, action=table, output_filtered_scores=True)
    out, fs = head.generate(ids, max_new_tokens=51, uniforms=uni, **kw)
    again, fs2 = head.generate(ids, max_new_tokens=51, uniforms=uni, **kw)
    assert torch.equal(again, out) and all(torch.equal(a, b) for a, b in zip(fs, fs2)), "two identical calls differ (eager / replayed graph)"
    tokens, steps = ids, []
    c0 = counter()
    for t in range(3):
        tokens, s = head.generate(tokens, max_new_tokens=17, uniforms=uni[:, 17 * t:17 * t + 17].contiguous(), reuse_cache=t > 0, **kw)
        steps.append(s)
    assert counter() - c0 == 17 + 18 + 18, "a kept-cache call runs the sampler once more, for j = 0, which writes nothing"
    assert torch.equal(out, tokens)
    for k, name in enumerate(fs._fields):
        whole, parts = fs[k], torch.cat([s[k] for s in steps], 1)
        assert torch.equal(whole, parts), f"{name} differs between one call and three kept-cache calls"
        assert (whole[:, FORCED] == 0).all() and torch.isfinite(whole).all()


# ------------------------------------------------------------------------------------------------ 4. row orders
def test_shared_context_and_fan_out_row_orders():
    ref = FR.fixture_reference()
    prompt = torch.from_numpy(ref["g"]["prompt"]).to(DEV)
    g = torch.Generator().manual_seed(13)
    ids = prompt.repeat(2, 1)                                             # rows k * 2 + b: sample k of prompt b
    table = torch.randn(4, ref["table"].shape[1], ref["table"].shape[2], generator=g).to(DEV)
    uni = torch.rand(4, 50, generator=g).to(DEV)
    head = T.make_head()
    kw = dict(do_sample=True, top_k=100, top_p=0.9, max_new_tokens=50, action=table, uniforms=uni, output_filtered_scores=True)
    plain, pf = head.generate(ids, **kw)
    c0 = counter()
    shared, sf = head.generate(ids, shared_context=2, **kw)
    assert counter() - c0 == 51, "a shared-context call runs the sampler once more, for j = 0"
    # (the prompt's last position goes through the decode-step kernels there: the same tokens up to near-ties of the sampler)
    print(f"shared context: {int((shared == plain).all(1).sum())} of 4 rows decide the plain call's tokens")
    want, near, sens, _ = oracle_filtered(shared, table, 50, 100, 0.9, 1.0)
    got = stack(sf)
    cols = np.array([c for c in SAMPLED if c < 50])
    use = ~near[:, cols]
    d = np.abs(got - want)[:, cols]
    assert d[..., 0][use].max() <= 2e-3 and d[..., 2][use].max() <= 2e-3 and (d[..., 3][use] == 0).all(), "a row of the shared call is not the caller's row"
    assert np.isfinite(got[:, cols, 0]).all() and (got[:, [16, 33]] == 0).all()
    # fan_out: rows b * k + j, and the kept cache is what it was
    head = T.make_head()
    head.llm._ensure(6, 32)
    ids3, table3, uni3 = T.three_rows()
    grown = head.generate(ids3, do_sample=True, max_new_tokens=17, action=table3, uniforms=uni3[:, :17].contiguous())
    g = torch.Generator().manual_seed(37)
    table6 = torch.randn(6, table3.shape[1], table3.shape[2], generator=g).to(DEV)
    uni6 = torch.rand(6, 16, generator=g).to(DEV)
    fkw = dict(action=table6, do_sample=True, top_k=100, top_p=0.9, max_new_tokens=16, uniforms=uni6)
    c0 = counter()
    cand, ff = head.fan_out(grown, 2, output_filtered_scores=True, **fkw)
    assert counter() - c0 == 17
    assert torch.equal(cand, head.fan_out(grown, 2, **fkw)) and torch.equal(cand[:, :531], grown.repeat_interleave(2, 0))
    _, ff2 = head.fan_out(grown, 2, output_filtered_scores=True, **fkw)
    assert all(torch.equal(a, b) for a, b in zip(ff, ff2)), "a second fan-out gave other scores: the kept cache changed"
    assert ff.logprob.shape == (6, 16) and torch.isfinite(ff.logprob).all() and (ff.support >= 1).all()
    # candidate b * 2 + j continues row b under its own actions: the oracle over its finished row (the sdf slot inside the kept prefix
    # carries the kept trajectory's action, the later ones the candidate's)
    tb = table6.clone()
    tb[:, :2] = table3.repeat_interleave(2, 0)[:, :2]
    want, near, sens, _ = oracle_filtered(cand, tb, 16, 100, 0.9, 1.0, start=531)
    got, use = stack(ff), ~near
    d = np.abs(got - want)
    print(f"fan_out: {int(use.sum())} of {use.size} columns compared; |d logprob| {d[..., 0][use].max():.2e}, |d kept_logmass| {d[..., 2][use].max():.2e}")
    assert d[..., 0][use].max() <= 2e-3 and d[..., 2][use].max() <= 2e-3 and (d[..., 3][use] == 0).all(), "fan_out rows are not b * k + j"
    cont = head.generate(grown, do_sample=True, max_new_tokens=17, action=table3, uniforms=uni3[:, 17:34].contiguous(), reuse_cache=True)
    assert cont.shape == (3, 548), "the kept cache no longer continues after the fan-outs"


# ------------------------------------------------------------------------------------------------ 5. the off path, refusals (C ABI)
def raw(eng, entry, prompt, B, L0_, n_new, actions, ids, ts, fs, uniforms=None, group=1, kept=0, fr=None, top_k=100):
    """ivg_generate_scored / ivg_generate_filtered (``fs`` is passed to the latter only)"""
    from ivideogpt_amd.engine import _ptr
    act_T = actions.shape[1] if actions is not None else 0
    tail = (_ptr(fs),) if entry == "ivg_generate_filtered" else ()
    with eng.stream() as s:
        rc = getattr(eng.lib, entry)(eng.h, _ptr(prompt), prompt.stride(0), B, L0_, n_new, _ptr(actions), act_T, 2, _ptr(uniforms), top_k,
                                     group, kept, 0, _ptr(ids), _ptr(fr), None, _ptr(ts), *tail, s)
    torch.cuda.synchronize()
    return rc


def test_off_path_and_refusals():
    ref = FR.fixture_reference()
    prompt, table = torch.from_numpy(ref["g"]["prompt"]).to(DEV), ref["table"].to(DEV)
    uni = torch.rand(2, 20, generator=torch.Generator().manual_seed(3)).to(DEV)
    head = T.make_head()
    eng = head.llm._ensure(2, 32)
    eng.set_temperature(1.0).set_top_p(0.9)
    runs = {}
    for entry in ("ivg_generate_scored", "ivg_generate_filtered"):
        ids, ts = T.Guarded(2 * (L0 + 20), torch.int64, T.SENT_I), T.Guarded(2 * 20 * 3, torch.float32, T.SENT_F)
        c0 = counters()
        assert raw(eng, entry, prompt, 2, L0, 20, table, ids.view, ts.view, None, uniforms=uni) == OK
        runs[entry] = (ids.view.clone(), ts.view.clone(), [a - b for a, b in zip(counters(), c0)])
        assert ids.guards_intact() and ts.guards_intact()
    a, b = runs["ivg_generate_scored"], runs["ivg_generate_filtered"]
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)), "without the new output the entries differ"
    assert a[2] == b[2] and b[2][0] == 0 and b[2][1] == 20, f"debug counters {dict(zip(COUNTERS, a[2]))} against {dict(zip(COUNTERS, b[2]))}"
    # with it: the same ids and TokenScores bits, exactly n_new columns of four
    ids, ts, fs = T.Guarded(2 * (L0 + 20), torch.int64, T.SENT_I), T.Guarded(2 * 20 * 3, torch.float32, T.SENT_F), T.Guarded(2 * 20 * 4, torch.float32, T.SENT_F)
    c0 = counters()
    assert raw(eng, "ivg_generate_filtered", prompt, 2, L0, 20, table, ids.view, ts.view, fs.view, uniforms=uni) == OK
    d = [x - y for x, y in zip(counters(), c0)]
    assert d[0] == 20 and d[1:] == a[2][1:], "the new output changed another counter"
    assert torch.equal(ids.view, a[0]) and torch.equal(ts.view.view(torch.int32), a[1].view(torch.int32))
    assert fs.guards_intact() and fs.filled() and (fs.view.view(2, 20, 4)[:, 16] == 0).all() and (fs.view.view(2, 20, 4)[:, :16, 3] >= 1).all()
    # refusals: by status and text, before anything is written
    big = T.Guarded(2 * 600 * 4, torch.float32, T.SENT_F)
    out = T.Guarded(2 * 1100, torch.int64, T.SENT_I)
    frw = T.Guarded(2 * 64, torch.float32, T.SENT_F)
    cases = {
        "beyond the cache": (CAPACITY, "exceeds the KV cache", dict(n_new=511, actions=table)),
        "a frame output with an unforced schedule": (INVALID, "forced-sdf schedule", dict(n_new=17, actions=None, fr=frw.view)),
        "a kept cache of another length": (INVALID, "generate_continue: the KV cache holds", dict(n_new=17, actions=table, kept=1)),
        "a kept cache with groups": (INVALID, "group_size must be 1", dict(n_new=17, actions=table, kept=1, group=2)),
    }
    c0 = counters()
    for what, (status, text, kw) in cases.items():
        rc = raw(eng, "ivg_generate_filtered", prompt, 2, kw.get("L0_", L0), kw["n_new"], kw["actions"], out.view, None, big.view,
                 kept=kw.get("kept", 0), group=kw.get("group", 1), fr=kw.get("fr"))
        msg = eng.lib.ivg_last_error(eng.h).decode()
        assert rc == status and text in msg, f"{what}: status {rc} ({msg!r}), expected {status} with {text!r}"
        assert out.untouched() and big.untouched() and frw.untouched(), f"{what}: an output was written"
    assert counters() == c0
    # the Python layer: the embeds-level call and generate_without_action carry the output too
    ids3, table3, uni3 = T.three_rows(23)
    e = head.llm.generate(inputs_embeds=head.get_input_embeddings(ids3), do_sample=True, max_new_tokens=17, uniforms=uni3[:, :17].contiguous(),
                          use_cache=False, return_dict_in_generate=True, output_filtered_scores=True)
    assert not hasattr(e, "token_scores") and e.filtered_scores.logprob.shape == (3, 17) and torch.isfinite(e.filtered_scores.logprob).all()
    assert (e.filtered_scores.support >= 1).all(), "the embeds path forces no column"
    seq, ef = head.llm.generate(inputs_embeds=head.get_input_embeddings(ids3), do_sample=True, max_new_tokens=17, uniforms=uni3[:, :17].contiguous(),
                                use_cache=False, output_filtered_scores=True)
    assert torch.equal(seq, e.sequences) and torch.equal(ef.logprob, e.filtered_scores.logprob)
    w = head.generate_without_action(ids3, do_sample=True, max_new_tokens=50, uniforms=uni3[:, :50].contiguous())
    w2, wf = head.generate_without_action(ids3, do_sample=True, max_new_tokens=50, uniforms=uni3[:, :50].contiguous(), output_filtered_scores=True)
    assert torch.equal(w2, w) and (wf.support[:, [16, 33]] == 0).all() and (wf.support[:, :16] >= 1).all()
    o17, r17 = head.generate(ids3, do_sample=True, max_new_tokens=17, action=table3, uniforms=uni3[:, :17].contiguous(), return_reward=True)
    s17 = head.generate(ids3, do_sample=True, max_new_tokens=17, action=table3, uniforms=uni3[:, :17].contiguous(), return_reward=True,
                        output_filtered_scores=True)
    assert len(s17) == 3 and torch.equal(s17[0], o17) and torch.equal(s17[1], r17) and type(s17[2]).__name__ == "FilteredTokenScores"


# ------------------------------------------------------------------------------------------------ 6. MBRL
def test_proposal_logprob_of_rollout_actions_and_plan(tmp_path):
    from helpers import world_model_files
    from mbrl.video_predictor import VideoPredictor
    args, *_ = world_model_files(tmp_path, False)
    args.update(encode_dtype="fp32", decode_dtype="fp32", llm_dtype="fp32")
    vp = VideoPredictor("cuda", args)
    g = torch.Generator().manual_seed(8)
    obs = torch.randint(0, 256, (2, 9, 64, 64), generator=g).float()
    acts = torch.randn(4, 3, 4, generator=g)
    uni = torch.rand(4, 50, generator=g).to(DEV)
    o0, a0, r0 = vp.rollout_actions(obs, acts, samples=2, uniforms=uni)
    o1, a1, r1, u1, p1 = vp.rollout_actions(obs, acts, samples=2, uniforms=uni, return_uncertainty=True, return_proposal_logprob=True)
    o2, a2, r2, p2 = vp.rollout_actions(obs, acts, samples=2, uniforms=uni, return_proposal_logprob=True)
    assert torch.equal(o1, o0) and torch.equal(r1, r0) and torch.equal(o2, o0), "return_proposal_logprob changed the rollout"
    assert p1.shape == (4, 4, 1) and p1.dtype == torch.float32 and torch.equal(p1, p2) and u1.shape == (4, 4, 1)
    assert (p1[:, 0] == 0).all() and (p1[:, 1:] < 0).all() and torch.isfinite(p1).all()
    # equality with per_frame() of the underlying call
    from ivideogpt_amd.transformer import _from_group_major, _to_group_major
    ctx, model = vp.context_length, vp.model
    stack_ = list(torch.chunk(obs.to(DEV) / 255., 3, dim=1))
    prompt = vp.tokenizer.encode_context(torch.stack(stack_[-ctx:], dim=1), ctx)
    table = torch.cat([acts.new_zeros(4, ctx - 1, 4), acts], 1).to(DEV)
    tokens, hidden, fs = model.generate(prompt.repeat(2, 1), do_sample=True, temperature=1.0, top_k=100, max_new_tokens=50,
                                        action=_from_group_major(table.contiguous(), 2, 2), uniforms=_from_group_major(uni.contiguous(), 2, 2),
                                        output_frame_hidden_states=True, shared_context=2, output_filtered_scores=True)
    assert torch.equal(p1[:, 1:, 0], _to_group_major(fs.per_frame()[0], 2, 2).float())
    # plan
    trk = vp.track(obs)
    plans = torch.randn(6, 2, 4, generator=g)
    pu = torch.rand(6, 33, generator=g).to(DEV)
    obss, actions, rewards, unc, prop = trk.plan(plans, samples=3, return_uncertainty=True, uniforms=pu, return_proposal_logprob=True)
    base = trk.plan(plans, samples=3, uniforms=pu)
    assert torch.equal(obss, base[0]) and torch.equal(rewards, base[2])
    assert prop.shape == unc.shape == (6, 3, 1) and (prop[:, 0] == 0).all() and (prop[:, 1:] < 0).all() and torch.isfinite(prop).all()
    tb = trk.table.repeat_interleave(3, 0)
    tb[:, trk.steps + ctx - 1:trk.steps + ctx - 1 + 2] = plans.to(DEV)
    _, _, ff = model.fan_out(trk.tokens, 3, action=tb, max_new_tokens=33, uniforms=pu, output_frame_hidden_states=True, output_filtered_scores=True)
    assert torch.equal(prop[:, 1:, 0], ff.per_frame()[0].float())
