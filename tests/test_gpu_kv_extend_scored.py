"""Frame rewards, hidden states and token scores from extending the kept K / V cache (include/ivg.h ivg_kv_extend_scored;
frame_rows_heads_kernel, token_scores_rows_kernel) on the MI355X: the score row kernel against its contract through
ivg_op_token_scores_rows, the decode-step route bit for bit against the rollout that sampled the same tokens (every cache format, both
launch profiles), the frame window's edges with guarded buffers, the chunk pass against the fp32 oracle with ivg_eval_forward /
ivg_logits as the yardstick, the untouched off path and every refusal, and the Python entries up to ``TrackedEpisode.observe``.
Tiny model throughout, as tests/test_gpu_frame_heads.py (hidden 128, 2 layers, 2 heads of 64, L0 = 514, ctx 2, B = 3)."""
import ctypes as C

import numpy as np
import pytest
import torch

import frame_heads_ref as FR
import token_scores_ref as TS
from test_gpu_frame_heads import DEV, FLAVOURS, PROFILES, SENT_F, Guarded, make_head, three_rows
from test_gpu_kv_extend import CTX, SENT, _p, assert_same, engine_of, extend, lib, scored

pytestmark = pytest.mark.gpu
OK, INVALID, MISSING, CAPACITY = 0, -1, -2, -4
H = 128
SENT_H = -768.0   # (a sentinel bf16 holds exactly)
Q = FR.frame_positions(CTX, 3)   # 529, 546, 563: the 16th tokens of the three predicted frames


def counters():
    return tuple(lib().ivg_debug_counter(n) for n in (b"kv_extend_chunk_rows", b"kv_extend_step_rows", b"kv_extend_frame_rows",
                                                      b"kv_extend_scored_rows", b"frame_heads", b"token_scores"))


def extend_scored(eng, prompt, keep, actions, nll=None, ts=None, fr=None, fh=None, B=None, L0=None, ctx=CTX):
    act_T = actions.shape[1] if actions is not None else 0
    with eng.stream() as s:
        rc = eng.lib.ivg_kv_extend_scored(eng.h, _p(prompt), prompt.stride(0), B or prompt.shape[0], keep, L0 or prompt.shape[1], _p(actions), act_T, ctx,
                                          _p(nll), _p(ts), _p(fr), _p(fh), s)
    torch.cuda.synchronize()
    return rc


def bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------ 1. the row kernel against its contract
def scores_rows(z, ids, ids_stride, row0, rows, Tc, V, first_forced, period, out, out_ld):
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib().ivg_op_token_scores_rows(_p(z), _p(ids), ids_stride, row0, rows, Tc, V, first_forced, period, _p(out), out_ld, st)
    torch.cuda.synchronize()
    return rc


def scores_step_kernel(z, tok):
    out = torch.full((z.shape[0], 3), SENT, device=DEV)
    assert lib().ivg_op_token_scores(_p(z), _p(tok), z.shape[0], z.shape[1], _p(out), C.c_void_p(torch.cuda.current_stream().cuda_stream)) == OK
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("name", [f"V{v}" for v in TS.VOCABS] + ["nonfinite"])
def test_score_rows_kernel_contract(name):
    """The chunk rows are rows r = row0 .. row0 + rows - 1 of (B, Tc = 3) rows with row0 = 1, so that row0 != 0 and every column
    occurs: each written entry holds token_scores_kernel's bits for the same logits row and id and is within BOUND of fp64; a forced
    column is three zeros; nothing but out[b * out_ld + c] is written (sentinels around and between)."""
    z_np, tok_np = TS.cases()[name]
    n, V = z_np.shape
    if name == "nonfinite":   # plus a row whose id is outside [0, V)
        z_np, tok_np = np.concatenate([z_np, np.ones((1, V), dtype=np.float32)]), np.concatenate([tok_np, [V]])
        n += 1
    z, tok = torch.from_numpy(np.array(z_np)).to(DEV), torch.from_numpy(np.array(tok_np)).to(DEV)
    want = scores_step_kernel(z, tok)
    ref = TS.reference(z_np[:, :V], np.clip(tok_np, 0, V - 1))
    if name == "nonfinite":
        ref[-1, 0] = np.nan
    assert TS.within(want.cpu().numpy(), ref).all()
    Tc, row0, ids_stride, out_ld = 3, 1, 7, 5
    B = (row0 + n + Tc - 1) // Tc
    where = [divmod(row0 + i, Tc) for i in range(n)]
    ids = torch.full((B, ids_stride), -5, dtype=torch.int64, device=DEV)
    for i, (b, c) in enumerate(where):
        ids[b, c] = tok[i]
    for first, period in ((0, 0), (2, 17), (1, 1), (0, 3)):
        out = Guarded(B * out_ld * 3, torch.float32, SENT_F)
        assert scores_rows(z, ids, ids_stride, row0, n, Tc, V, first, period, out.view, out_ld) == OK
        assert out.guards_intact()
        got = out.view.view(B, out_ld, 3)
        written = torch.zeros(B, out_ld, dtype=torch.bool, device=DEV)
        for i, (b, c) in enumerate(where):
            written[b, c] = True
            if period > 0 and c >= first and (c - first) % period == 0:
                assert (got[b, c] == 0).all(), f"({first}, {period}): forced column {c} of row {b} is not three zeros"
            else:
                assert torch.equal(bits(got[b, c]), bits(want[i])), f"({first}, {period}): row {i} -> ({b}, {c}) differs from token_scores_kernel"
                assert TS.within(got[b, c].cpu().numpy(), ref[i]).all()
        assert (got[~written] == SENT_F).all(), f"({first}, {period}): an entry outside the chunk's rows was written"


# ------------------------------------------------------------------------------------------------ 2. the step route is exact
@PROFILES
@pytest.mark.parametrize("flavour", list(FLAVOURS))
def test_step_route_equals_the_rollout_that_sampled_the_tokens(flavour, lds_kb, switches):
    """R1 = one 51-token ivg_generate_scored call with rewards, hidden states and scores.  R2 = a 17-token call, then
    ivg_kv_extend_scored(keep_len 530, L0 548) with R1's tokens: its scores are R1's columns 17 .. 33 (column 16 forced: zeros), its
    frame is R1's frame 1, its NLL ivg_kv_extend's -- bit for bit -- and a 17-token continue reproduces R1's last 17 tokens."""
    dtype, kv = FLAVOURS[flavour]
    if flavour == "bf16":
        switches(IVG_KV_EXTEND_CHUNK="0")
    head = make_head(dtype, lds_kb, kv=kv)
    hdt = head.llm.torch_dtype
    ids, table, uni = three_rows()
    eng = engine_of(head, 3, table.shape[1])
    r1 = scored(eng, ids, 51, table, uni, hid_dtype=hdt)
    full = r1[0][:, :548].contiguous()
    u0 = uni[:, :17].contiguous()
    scored(eng, ids, 17, table, u0)
    nll0 = torch.full((3, 17), SENT, device=DEV)
    assert extend(eng, full, 530, table, nll0) == OK
    scored(eng, ids, 17, table, u0)
    nll, ts, fr = torch.full((3, 17), SENT, device=DEV), torch.full((3, 17, 3), SENT, device=DEV), torch.full((3, 1), SENT, device=DEV)
    fh = torch.full((3, 1, H), SENT, dtype=hdt, device=DEV)
    c0 = counters()
    assert extend_scored(eng, full, 530, table, nll, ts, fr, fh) == OK, eng.lib.ivg_last_error(eng.h)
    c1 = counters()
    assert (c1[0] - c0[0], c1[1] - c0[1]) == (0, 51), "3 x 17 rows through the decode steps"
    assert (c1[2] - c0[2], c1[3] - c0[3]) == (3, 51), "3 frame rows, 51 scored rows"
    assert torch.equal(ts, r1[3][:, 17:34]), f"{(ts != r1[3][:, 17:34]).sum().item()} score entries differ from R1's columns 17 .. 33"
    assert (ts[:, 16] == 0).all() and (ts[:, :16, 0] < 0).all()
    assert torch.equal(fr, r1[1][:, 1:2]), "the frame reward is not R1's frame 1"
    assert torch.equal(fh, r1[2][:, 1:2]), "the frame hidden state is not R1's frame 1"
    assert torch.equal(nll, nll0), "token_nll differs from ivg_kv_extend's"
    b = scored(eng, full, 17, table, uni[:, 34:51].contiguous(), kept=1, hid_dtype=hdt)
    assert_same(b, (r1[0], r1[1][:, 2:3], r1[2][:, 2:3], r1[3][:, 34:51]), "continue after the scored extend")


# ------------------------------------------------------------------------------------------------ 3. the frame window's edges
@pytest.mark.parametrize("dtype", ["fp32", "bf16"], ids=["fp32_steps", "bf16_chunk"])
def test_frame_window_edges(dtype):
    """F_out and which of R1's frames lands in column 0, with guarded buffers: on the fp32 step route the frames are R1's bit for
    bit; on the bf16 chunk route (another attention kernel) each column is nearer to its R1 frame than to any other."""
    head = make_head(dtype)
    hdt = head.llm.torch_dtype
    ids, table, uni = three_rows()
    eng = engine_of(head, 3, table.shape[1])
    r1 = scored(eng, ids, 51, table, uni, hid_dtype=hdt)
    u0 = uni[:, :17].contiguous()
    chunk = dtype == "bf16"

    def run(keep, L0, F_cap):
        scored(eng, ids, 17, table, u0)                                      # the kept cache of 530 positions
        fr, fh = Guarded(3 * F_cap, torch.float32, SENT_F), Guarded(3 * F_cap * H, hdt, SENT_H)
        T = L0 - 1 - keep
        ts, nll = Guarded(3 * max(T, 1) * 3, torch.float32, SENT_F), Guarded(3 * max(T, 1), torch.float32, SENT_F)
        c0 = counters()
        assert extend_scored(eng, r1[0][:, :L0].contiguous(), keep, table, nll.view, ts.view, fr.view, fh.view) == OK, eng.lib.ivg_last_error(eng.h)
        c1 = counters()
        for g in (fr, fh, ts, nll):
            assert g.guards_intact()
        assert (c1[0] - c0[0], c1[1] - c0[1]) == ((3 * T, 0) if chunk else (0, 3 * T)), "the wrong route ran"
        assert c1[3] - c0[3] == 3 * T and c1[4:] == c0[4:]
        return fr, fh, ts, nll, c1[2] - c0[2]

    def check_frames(fr, fh, first, F):
        got_r, got_h = fr.view.view(3, F), fh.view.view(3, F, H)
        for k in range(F):
            if chunk:
                d = (got_h[:, k, None].float() - r1[2].float()).abs().amax(-1)     # (3, 3): to each of R1's frames
                assert (d.argmin(1) == first + k).all(), f"column {k} is not R1's frame {first + k}: distances {d.tolist()}"
                assert torch.isfinite(got_r[:, k]).all()
            else:
                assert torch.equal(got_h[:, k], r1[2][:, first + k]) and torch.equal(got_r[:, k], r1[1][:, first + k]), f"column {k} is not R1's frame {first + k}"

    # T = 1: the one fed token is q_0
    assert Q[0] == 529
    fr, fh, ts, nll, rows = run(529, 531, 1)
    assert rows == 3 and fr.filled() and fh.filled() and ts.filled() and nll.filled()
    check_frames(fr, fh, 0, 1)
    # ends one short of q_1: no frame, nothing written, no frame row counted; the scores and the NLL are there
    fr, fh, ts, nll, rows = run(530, 547, 1)
    assert rows == 0 and fr.untouched() and fh.untouched() and ts.filled() and nll.filled()
    # frames 0, 1, 2
    fr, fh, ts, nll, rows = run(529, 565, 3)
    assert rows == 9 and fr.filled() and fh.filled() and ts.filled()
    check_frames(fr, fh, 0, 3)
    assert (ts.view.view(3, 35, 3)[:, [0, 17, 34]] == 0).all(), "the columns whose target is an sdf slot (530, 547, 564) are zeros"
    # a rewind with outputs given writes nothing
    fr, fh, ts, nll, rows = run(530, 531, 1)
    assert rows == 0 and fr.untouched() and fh.untouched() and ts.untouched() and nll.untouched()
    out = scored(eng, r1[0][:, :531].contiguous(), 17, table, uni[:, 17:34].contiguous(), kept=1)
    assert torch.equal(out[0][:, :531], r1[0][:, :531])


# ------------------------------------------------------------------------------------------------ 4. the chunk pass against the oracle
def test_chunk_pass_vs_oracle(switches):
    """bf16, keep_len 530, L0 548.  frame_hidden, frame_rewards, logprob and entropy against the fp32 oracle's teacher-forced pass
    (log-softmax and entropy of its logits in fp64): max |got - oracle| <= 2 e_ef + 1e-3, the bar of test_chunk_pass_nll_vs_oracle,
    with e_ef the deviation at the same positions of ivg_eval_forward's hidden (hidden, reward) or of ivg_logits' rows reduced in fp64
    (scores).  Preconditions on the oracle alone: the hidden rows at q_1 - 1 and q_1 + 1 differ from row q_1, and a one-slot shift of
    the action table moves some output, by more than ten times that tolerance.  The step route on the same engine agrees within the
    same tolerance; reward_linear(frame_hidden) in fp64 is within H eps sum |w h| of frame_rewards; the extended cache continues."""
    ref = FR.fixture_reference()
    head = make_head("bf16")
    ids, table, uni = three_rows()
    table = (table * 3.0).contiguous()
    eng = engine_of(head, 3, table.shape[1])
    r1 = scored(eng, ids, 51, table, uni)
    full = r1[0][:, :548].contiguous()
    w, bias = ref["sd"]["reward_linear.weight"].double()[0], ref["sd"]["reward_linear.bias"].double()[0]
    tgt = full.cpu()[:, 531:548, None]

    def oracle(tab):
        logits, hid = FR.teacher_forced(ref["sd"], ref["cfg"], full.cpu(), tab.cpu(), CTX)
        return hid.double(), reduce64(logits[:, 530:547])

    def reduce64(rows):
        lp = torch.log_softmax(rows.double(), -1)
        return lp.gather(-1, tgt).squeeze(-1)[:, :16], -(lp.exp() * lp).sum(-1)[:, :16]    # (column 16 is forced: not scored)

    hid_o, (lp_o, en_o) = oracle(table)
    want = dict(hidden=hid_o[:, Q[1]], reward=hid_o[:, Q[1]] @ w + bias, logprob=lp_o, entropy=en_o)
    # the yardstick: the prompt pass over the whole row
    nll_all, rows2 = torch.zeros(3, 548, device=DEV), torch.zeros(3, 2, device=DEV)
    hid_ef = torch.zeros(3, 548, H, dtype=torch.bfloat16, device=DEV)
    eng.eval_forward(full, full, nll_all, rows2, actions=table, ctx=CTX, hidden=hid_ef)
    lg = torch.zeros(3, 548, ref["cfg"]["vocab_size"], device=DEV)
    eng.logits(full, lg, actions=table, ctx=CTX)
    torch.cuda.synchronize()
    h_ef = hid_ef[:, Q[1]].cpu().double()
    lp_ef, en_ef = reduce64(lg[:, 530:547].cpu())
    yard = dict(hidden=h_ef, reward=h_ef @ w + bias, logprob=lp_ef, entropy=en_ef)
    e_ef = {k: (yard[k] - want[k]).abs().max().item() for k in want}
    tol = {k: 2 * e_ef[k] + 1e-3 for k in want}
    for d in (-1, 1):
        gap = (hid_o[:, Q[1] + d] - hid_o[:, Q[1]]).abs().max().item()
        assert gap > 10 * tol["hidden"], f"precondition: the oracle's hidden row at q_1 {d:+d} differs from row q_1 by only {gap:.3e} (tolerance {tol['hidden']:.3e})"
    hid_s, (lp_s, en_s) = oracle(torch.roll(table, 1, 1))
    moved = dict(hidden=(hid_s[:, Q[1]] - want["hidden"]).abs().max().item(), reward=((hid_s[:, Q[1]] @ w + bias) - want["reward"]).abs().max().item(),
                 logprob=(lp_s - lp_o).abs().max().item(), entropy=(en_s - en_o).abs().max().item())
    assert any(moved[k] > 10 * tol[k] for k in want), f"precondition: a shifted action row moves the oracle by only {moved} (tolerances {tol})"
    got = {}
    for route, env in (("chunk", None), ("steps", "0")):
        switches(IVG_KV_EXTEND_CHUNK=env)
        scored(eng, ids, 17, table, uni[:, :17].contiguous())
        ts, fr = torch.full((3, 17, 3), SENT, device=DEV), torch.full((3, 1), SENT, device=DEV)
        fh = torch.full((3, 1, H), SENT, dtype=torch.bfloat16, device=DEV)
        c0 = counters()
        assert extend_scored(eng, full, 530, table, None, ts, fr, fh) == OK, eng.lib.ivg_last_error(eng.h)
        c1 = counters()
        assert (c1[0] - c0[0], c1[1] - c0[1]) == ((51, 0) if route == "chunk" else (0, 51)), f"{route}: the wrong route ran"
        assert (c1[2] - c0[2], c1[3] - c0[3]) == (3, 51)
        assert (ts[:, 16] == 0).all()
        got[route] = dict(hidden=fh[:, 0].cpu().double(), reward=fr[:, 0].cpu().double(), logprob=ts[:, :16, 0].cpu().double(),
                          entropy=ts[:, :16, 1].cpu().double())
        terms = fh[:, 0].cpu().double() * w
        bound = H * torch.finfo(torch.bfloat16).eps * terms.abs().sum(-1)
        d = (fr[:, 0].cpu().double() - (terms.sum(-1) + bias)).abs()
        print(f"{route}: max |frame_rewards - fp64 reward_linear(frame_hidden)| = {d.max().item():.3e}, smallest bound {bound.min().item():.3e}")
        assert (d <= bound).all(), f"{route}: frame_rewards is not reward_linear of frame_hidden"
        out = scored(eng, full, 17, table, uni[:, 34:51].contiguous(), kept=1)
        assert torch.equal(out[0][:, :548], full)
    e_a = {k: (got["chunk"][k] - want[k]).abs().max().item() for k in want}
    e_b = {k: (got["steps"][k] - want[k]).abs().max().item() for k in want}
    e_ab = {k: (got["chunk"][k] - got["steps"][k]).abs().max().item() for k in want}
    for k in want:
        print(f"{k}: chunk pass vs oracle e_a {e_a[k]:.3e}, decode steps {e_b[k]:.3e}, yardstick e_ef {e_ef[k]:.3e}; chunk vs steps {e_ab[k]:.3e}; "
              f"tolerance {tol[k]:.3e}; a shifted action row moves the oracle by {moved[k]:.3e}")
    for k in want:
        assert e_a[k] <= tol[k], f"chunk pass {k} misses the oracle by {e_a[k]:.3e} (yardstick {e_ef[k]:.3e})"
        assert e_ab[k] <= tol[k], f"chunk pass and decode steps differ in {k} by {e_ab[k]:.3e}"


# ------------------------------------------------------------------------------------------------ 5. nothing else moved
@pytest.mark.parametrize("dtype", ["fp32", "bf16"], ids=["fp32_steps", "bf16_chunk"])
def test_all_outputs_null_is_kv_extend(dtype):
    head = make_head(dtype)
    ids, table, uni = three_rows()
    eng = engine_of(head, 3, table.shape[1])
    r1 = scored(eng, ids, 51, table, uni)
    full, u0, v = r1[0][:, :548].contiguous(), uni[:, :17].contiguous(), uni[:, 34:51].contiguous()
    outs = []
    for entry in (extend, extend_scored):
        scored(eng, ids, 17, table, u0)
        nll = torch.full((3, 17), SENT, device=DEV)
        c0 = counters()
        assert entry(eng, full, 530, table, nll) == OK
        c1 = counters()
        outs.append((nll, tuple(a - b for a, b in zip(c1, c0)), scored(eng, full, 17, table, v, kept=1)))
    assert torch.equal(outs[0][0], outs[1][0]), "token_nll differs between the two entries"
    assert outs[0][1] == outs[1][1] and outs[1][1][2:] == (0, 0, 0, 0), f"counters: {outs[0][1]} vs {outs[1][1]}"
    assert sum(outs[1][1][:2]) == 51
    assert_same(outs[1][2], outs[0][2], "continue after the entry with all outputs NULL")


def test_missing_heads_are_refused():
    ids, table, uni = three_rows()
    u0 = uni[:, :17].contiguous()
    # no reward head
    bare = make_head(reward=False)
    eng = engine_of(bare, 3, table.shape[1])
    grown = scored_no_reward(eng, ids, table, u0)
    full = torch.cat([grown, grown[:, 514:531]], 1).contiguous()
    fr, fh, ts = Guarded(3, torch.float32, SENT_F), Guarded(3 * H, torch.float32, SENT_F), Guarded(3 * 17 * 3, torch.float32, SENT_F)
    c0 = counters()
    assert extend_scored(eng, full, 530, table, None, ts.view, fr.view, fh.view) == MISSING
    assert "reward_linear is not loaded" in eng.lib.ivg_last_error(eng.h).decode()
    assert fr.untouched() and fh.untouched() and ts.untouched() and counters() == c0
    assert extend_scored(eng, full, 530, table, None, ts.view, None, fh.view) == OK, "hidden states and scores need no reward head"
    assert fh.filled() and ts.filled() and fr.untouched()
    # no final norm in the weight table
    head = make_head()
    head.llm._packed_weights().pop("llm.norm")
    eng = engine_of(head, 3, table.shape[1])
    grown = scored(eng, ids, 17, table, u0)[0]
    full = torch.cat([grown, grown[:, 514:531]], 1).contiguous()
    fr, fh = Guarded(3, torch.float32, SENT_F), Guarded(3 * H, torch.float32, SENT_F)
    c0 = counters()
    assert extend_scored(eng, full, 530, table, None, None, fr.view, fh.view) == MISSING
    assert "'llm.norm' is not in the weight table" in eng.lib.ivg_last_error(eng.h).decode()
    assert fr.untouched() and fh.untouched() and counters() == c0
    assert extend_scored(eng, full, 530, table, None, None, fr.view, None) == OK and fr.filled(), "rewards need no 'llm.norm' entry (it is folded into the head)"


def scored_no_reward(eng, ids, table, u0):
    """A 17-token rollout on an engine without a reward head -> (3, 531); keeps 530 positions."""
    out = torch.full((3, 531), -12345, dtype=torch.int64, device=DEV)
    with eng.stream() as s:
        rc = eng.lib.ivg_generate_scored(eng.h, _p(ids), ids.stride(0), 3, 514, 17, _p(table), table.shape[1], CTX, _p(u0), 100, 1, 0, 0, _p(out), None, None,
                                         None, s)
    torch.cuda.synchronize()
    assert rc == OK
    return out


def test_kv_extends_refusals_come_through_with_outputs_untouched():
    head, twin = make_head(), make_head()
    ids, table, uni = three_rows()
    eng, teng = engine_of(head, 3, table.shape[1]), engine_of(twin, 3, table.shape[1])
    u0, v = uni[:, :17].contiguous(), uni[:, 17:34].contiguous()
    nll, ts = torch.full((3, 64), SENT, device=DEV), torch.full((3, 64, 3), SENT, device=DEV)
    fr, fh = torch.full((3, 4), SENT, device=DEV), torch.full((3, 4, H), SENT, device=DEV)

    def call(prompt, keep, actions, **kw):
        rc = extend_scored(eng, prompt, keep, actions, nll, ts, fr, fh, **kw)
        assert all((t == SENT).all() for t in (nll, ts, fr, fh)) or rc == OK, "a refused call wrote an output"
        return rc

    assert call(ids, 500, table) == INVALID, "a fresh engine holds no kept cache"
    assert eng.lib.ivg_last_error(eng.h).decode().startswith("kv_extend_scored: ")
    emb = torch.empty(3, 514, H, device=DEV)
    eng.embed_tokens(ids, emb)
    eng.generate_embeds(emb, 3, torch.empty(3, 3, dtype=torch.int64, device=DEV))
    assert call(ids, 500, None, ctx=1) == INVALID, "a cache built from embeddings is out of scope"
    grown = scored(eng, ids, 17, table, u0)[0].contiguous()
    want = scored(teng, scored(teng, ids, 17, table, u0)[0].contiguous(), 17, table, v, kept=1)
    full = want[0].contiguous()
    other = full.clone(); other[1, 520] = (other[1, 520] + 1) % 100
    act2 = table.clone(); act2[2, 1, 0] += 1.0
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
        rc = call(kw["prompt"], kw["keep"], kw["actions"], L0=kw.get("L0"), ctx=kw.get("ctx", CTX))
        assert rc == status, f"{what}: status {rc}, expected {status}"
        assert counters()[:4] == c0[:4]
        got = scored(eng, grown, 17, table, v, kept=1)
        assert_same(got, want, f"continue after the refusal of {what}")
        scored(eng, ids, 17, table, u0)


# ------------------------------------------------------------------------------------------------ 6. Python
def test_python_extend_kept_cache_matches_the_c_level():
    from ivideogpt_amd import ExtendOutputs, TokenScores
    head, twin = make_head(), make_head()
    ids, table, uni = three_rows()
    teng = engine_of(twin, 3, table.shape[1])
    u0 = uni[:, :17].contiguous()
    r1 = scored(teng, ids, 51, table, uni)
    full = r1[0][:, :548].contiguous()
    scored(teng, ids, 17, table, u0)
    nll, ts, fr = torch.full((3, 17), SENT, device=DEV), torch.full((3, 17, 3), SENT, device=DEV), torch.full((3, 1), SENT, device=DEV)
    fh = torch.full((3, 1, H), SENT, device=DEV)
    assert extend_scored(teng, full, 530, table, nll, ts, fr, fh) == OK

    def fresh():
        head.generate(ids, do_sample=True, max_new_tokens=17, action=table, uniforms=u0)

    fresh()
    assert head.extend_kept_cache(full, action=table, keep=530) is None
    fresh()
    assert torch.equal(head.extend_kept_cache(full, action=table, keep=530, return_nll=True), nll)
    for kw, field, want in ((dict(return_reward="frames"), "frame_rewards", fr), (dict(output_frame_hidden_states=True), "frame_hidden", fh),
                            (dict(output_token_scores=True), "token_scores", ts)):
        fresh()
        out = head.extend_kept_cache(full, action=table, keep=530, **kw)
        assert isinstance(out, ExtendOutputs) and [f for f in out._fields if getattr(out, f) is not None] == [field]
        if field == "token_scores":
            assert isinstance(out.token_scores, TokenScores) and all(torch.equal(t, want[:, :, k]) for k, t in enumerate(out.token_scores))
        else:
            assert torch.equal(getattr(out, field), want)
    fresh()
    out = head.extend_kept_cache(full, action=table, keep=530, return_nll=True, return_reward="frames", output_frame_hidden_states=True,
                                 output_token_scores=True)
    assert torch.equal(out.token_nll, nll) and torch.equal(out.frame_rewards, fr) and torch.equal(out.frame_hidden, fh)
    assert all(torch.equal(t, ts[:, :, k]) for k, t in enumerate(out.token_scores))
    out = head.extend_kept_cache(full[:, :531].contiguous(), action=table, keep=530, return_reward="frames", output_token_scores=True)   # rewind
    assert out.frame_rewards.shape == (3, 0) and out.token_scores.logprob.shape == (3, 0) and out.token_nll is None
    with pytest.raises(ValueError, match="reward_prediction"):
        make_head(reward=False).extend_kept_cache(full, action=table, keep=530, return_reward="frames")
    with pytest.raises(ValueError):
        head.extend_kept_cache(full, action=table, keep=530, return_reward=True)


def test_observe_returns_the_models_view_of_the_frame(tmp_path):
    from mbrl.video_predictor import Observation, symexp
    from test_gpu_track import episode, predictors
    vp, plain, by_hand = predictors(tmp_path, "bf16", n=3)
    obs, (f1,), (a1,) = episode(2, 1)
    trk, trk0 = vp.track(obs), plain.track(obs)
    o = trk.observe(f1, a1, return_outputs=True)
    s0 = trk0.observe(f1, a1)
    assert isinstance(o, Observation) and s0.shape == (2,)
    assert torch.equal(o.surprise, s0), "the surprise differs from the default call's on an identical session"
    assert o.reward.shape == (2, 1) and o.hidden.shape[0] == 2 and o.hidden.dim() == 2 and o.entropy.shape == (2,)
    assert torch.isfinite(o.entropy).all() and (o.entropy > 0).all()
    # by hand: the same extend on a third model object taken through the same calls
    model = by_hand.model
    ids0 = trk0.tokens[:, :257 * 2].contiguous()
    table0 = torch.zeros_like(trk.table)
    model.generate(ids0, do_sample=False, max_new_tokens=1, action=table0)
    model.extend_kept_cache(ids0, action=table0, keep=ids0.shape[1] - 1)
    out = model.extend_kept_cache(trk.tokens, action=trk.table, keep=ids0.shape[1] - 1, output_frame_hidden_states=True, output_token_scores=True)
    assert out.frame_hidden.shape[1] == 1 and torch.equal(o.hidden, out.frame_hidden[:, 0])
    assert torch.equal(o.entropy, out.token_scores.per_frame()[1][:, 0])
    r = vp.model.reward_linear(o.hidden)
    assert torch.equal(o.reward, (symexp(r) if vp.symlog else r).float())
    trk.select([1, 0])
    assert trk.observe(f1[[1, 0]], a1[[1, 0]]).shape == (2,)
