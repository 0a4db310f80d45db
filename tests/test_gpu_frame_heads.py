"""Per-frame rewards and hidden states from one rollout call (include/ivg.h ivg_generate_frames; frame_heads_kernel inside the decode
steps) on the MI355X: against the REFERENCE's own per-step vectors (tests/golden/llama_tiny_ctx2_mbrl.npz) and the teacher-forced
oracle of tests/frame_heads_ref.py, bit for bit against the step-by-step route and today's ``reward_out``, the frame count and the
refusals through the C ABI with guarded buffers, the second cache chunk, the untouched off path, and ``VideoPredictor.rollout_actions``
against ``rollout``.  Tiny model throughout (hidden 128, 2 layers, 2 heads of 64, L0 = 514)."""

import numpy as np
import pytest
import torch

import frame_heads_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PROFILES = pytest.mark.parametrize("lds_kb", [0, 40], ids=["one_batch", "batches_in_flight"])   # as tests/test_gpu_models.py
OK, INVALID, MISSING, CAPACITY = 0, -1, -2, -4


def counter():
    from ivideogpt_amd import _lib
    return _lib.load().ivg_debug_counter(b"frame_heads")


def make_head(dtype="fp32", lds_kb=0, reward=True, kv=None):
    """The fixture's model (seeded weights the reference vectors were made with) under the wrapper; 3 future frames."""
    from ivideogpt_amd import HeadModelWithAction, LlamaForCausalLM, weights as W
    ref = R.fixture_reference()
    cfg, g = ref["cfg"], ref["g"]
    adim, ctx = int(g["action_dim"]), int(g["ctx"])
    sd = W.random_llama_state_dict(cfg, int(g["seed"]), action_dim=adim, reward_prediction=reward)
    head = HeadModelWithAction(LlamaForCausalLM(cfg, None, dtype=dtype, decode_lds_kb=lds_kb), adim, 257 * ctx - 1, 16, ctx, ctx + 3,
                               reward_prediction=reward)
    head.load_state_dict(sd, strict=True)
    head.to(DEV)
    if kv is not None:
        head.set_kv_cache_dtype("fp8_e4m3", **kv)
    return head


def fixture_inputs():
    ref = R.fixture_reference()
    return ref, torch.from_numpy(ref["g"]["prompt"]).to(DEV), ref["table"].to(DEV)


def three_rows(seed=7):
    """B = 3 prompts (the fixture's two and a splice of them), an action table and a (3, 51) table of uniforms."""
    ref, prompt, _ = fixture_inputs()
    third = prompt[1].clone()
    third[5:200] = prompt[0, 5:200]
    g = torch.Generator().manual_seed(seed)
    table = torch.randn(3, ref["table"].shape[1], ref["table"].shape[2], generator=g).to(DEV)
    uni = torch.rand(3, 51, generator=g).to(DEV)
    return torch.cat([prompt, third[None]], 0), table, uni


# ------------------------------------------------------------------------------------------------ 1. the reference's own vectors
@PROFILES
def test_frames_match_reference_vectors(lds_kb):
    """One 51-token call (``max_new_tokens=50``) gives, per frame, the 16 tokens of the reference's step and its reward within 1e-3
    (the bar of test_mbrl_step_matches_reference_vectors); the same through ``shared_context=2``, row by row against a plain run."""
    ref, prompt, table = fixture_inputs()
    g = ref["g"]
    head = make_head(lds_kb=lds_kb)
    c0 = counter()
    out, rew = head.generate(prompt, do_sample=False, max_new_tokens=50, action=table, return_reward="frames")
    assert out.shape == (2, 514 + 50) and rew.shape == (2, 3) and rew.dtype == torch.float32
    assert counter() - c0 == 3, "three steps of the call fed a frame's 16th token"
    out, rew = out.cpu().numpy(), rew.cpu().numpy()
    for t in range(3):
        assert np.array_equal(out[:, 514 + 17 * t:514 + 17 * t + 16], g["step_tokens"][t]), f"frame {t}: tokens differ from the reference"
        err = np.abs(rew[:, t] - g["step_rewards"][t]).max()
        print(f"frame {t}: reward vs reference {err:.2e}")
        assert err < 1e-3, f"frame {t}: reward differs from the reference"
    assert (out[:, 514 + 16] == ref["cfg"]["vocab_size"] - 1).all() and (out[:, 514 + 33] == ref["cfg"]["vocab_size"] - 1).all()
    # shared context: the prompt of row 0 twice, each row its own actions
    twice = prompt[:1].repeat(2, 1)
    c0 = counter()
    plain, prew = head.generate(twice, do_sample=False, max_new_tokens=50, action=table, return_reward="frames")
    shared, srew = head.generate(twice, do_sample=False, max_new_tokens=50, action=table, return_reward="frames", shared_context=2)
    assert counter() - c0 == 6
    assert torch.equal(plain[0], torch.from_numpy(out[0]).to(DEV)), "row 0 of the repeated prompt is the fixture's row 0"
    assert torch.equal(shared, plain), "shared-context tokens differ from the plain run"
    err = (srew - prew).abs().max().item()
    print(f"shared vs plain rewards {err:.2e}")
    assert err < 1e-3
    assert np.abs(srew[0].cpu().numpy() - g["step_rewards"][:, 0]).max() < 1e-3


# ------------------------------------------------------------------------------------------------ 2. one call == step by step
PER_HEAD = [[[1.0, 0.5], [2.0, 1.0]], [[0.25, 1.0], [1.0, 4.0]]]   # (layers, k|v, heads) powers of two
FLAVOURS = {"fp32": ("fp32", None), "bf16": ("bf16", None), "bf16_fp8": ("bf16", dict(k_scale=1.0, v_scale=1.0)),
            "bf16_fp8_per_head": ("bf16", dict(scales=PER_HEAD)), "x3": ("x3", None)}


@PROFILES
@pytest.mark.parametrize("flavour", list(FLAVOURS))
def test_one_call_equals_step_by_step_bitwise(flavour, lds_kb):
    """Sampled, B = 3: the tokens of one 51-token call equal those of three 17-token calls on the kept cache fed columns 17 t .. 17 t + 16
    of the same uniforms, and the frame rewards equal the three ``return_reward=True`` values BIT FOR BIT: both routes feed the same
    tokens through the same decode-step kernels over the same cache contents."""
    dtype, kv = FLAVOURS[flavour]
    head = make_head(dtype, lds_kb, kv=kv)
    ids, table, uni = three_rows()
    c0 = counter()
    out, rew = head.generate(ids, do_sample=True, top_k=100, max_new_tokens=50, action=table, uniforms=uni, return_reward="frames")
    assert counter() - c0 == 3
    tokens, steps = ids, []
    for t in range(3):
        tokens, r = head.generate(tokens, do_sample=True, top_k=100, max_new_tokens=17, action=table,
                                  uniforms=uni[:, 17 * t:17 * t + 17].contiguous(), return_reward=True, reuse_cache=t > 0)
        steps.append(r)
    assert counter() - c0 == 3, "the step-wise calls do not run the frame kernel"
    assert torch.equal(out, tokens[:, :-1]), f"{(out != tokens[:, :-1]).sum().item()} tokens differ between one call and three"
    steps = torch.stack(steps, 1)
    print(f"{flavour}: max |one call - step by step| = {(rew - steps).abs().max().item():.3e}")
    assert torch.equal(rew, steps), "frame rewards differ from the step-wise reward_out values"


# ------------------------------------------------------------------------------------------------ 3. today's reward_out
@pytest.mark.parametrize("n_new", [17, 34])
def test_last_frame_is_todays_reward_out(n_new):
    head = make_head()
    ids, table, uni = three_rows(11)
    u = uni[:, :n_new].contiguous()
    old, r = head.generate(ids, do_sample=True, max_new_tokens=n_new, action=table, uniforms=u, return_reward=True)
    new, rew = head.generate(ids, do_sample=True, max_new_tokens=n_new - 1, action=table, uniforms=u, return_reward="frames")
    assert rew.shape == (3, n_new // 17)
    assert torch.equal(new, old[:, :-1])
    assert torch.equal(rew[:, -1], r), "frame_rewards[:, F_out - 1] is not reward_out of the same call"


# ------------------------------------------------------------------------------------------------ 4. hidden states
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_frame_hidden_states(dtype):
    """``reward_linear(frame_hidden)`` in fp64 equals ``frame_rewards`` within the rounding of one dot product of H terms
    (H x eps x sum |w h|); the fp32 rows are within 1e-3 of the teacher-forced oracle's ``hid`` rows."""
    ref, prompt, table = fixture_inputs()
    head = make_head(dtype)
    out, rew, hid = head.generate(prompt, do_sample=False, max_new_tokens=50, action=table, return_reward="frames", output_frame_hidden_states=True)
    H = ref["cfg"]["hidden_size"]
    assert hid.shape == (2, 3, H) and hid.dtype == (torch.float32 if dtype == "fp32" else torch.bfloat16)
    only = head.generate(prompt, do_sample=False, max_new_tokens=50, action=table, output_frame_hidden_states=True)
    assert len(only) == 2 and torch.equal(only[0], out) and torch.equal(only[1], hid)
    w, b = ref["sd"]["reward_linear.weight"].double()[0], ref["sd"]["reward_linear.bias"].double()[0]
    terms = hid.double().cpu() * w
    dot = terms.sum(-1) + b
    eps = torch.finfo(hid.dtype).eps
    bound = H * eps * terms.abs().sum(-1)
    d = (rew.double().cpu() - dot).abs()
    print(f"{dtype}: max |rewards - fp64 reward_linear(hidden)| = {d.max().item():.3e}, smallest bound {bound.min().item():.3e}")
    assert (d <= bound).all()
    if dtype == "fp32":
        assert torch.equal(out.cpu(), ref["ids"][:, :out.shape[1]]), "greedy tokens are the fixture's"
        err = (hid.cpu() - ref["frame_hidden"]).abs().max().item()
        print(f"fp32 frame_hidden vs oracle {err:.2e}")
        assert err < 1e-3


def test_generate_without_action_frame_hidden():
    ref, prompt, _ = fixture_inputs()
    head = make_head()
    uni = torch.rand(2, 50, generator=torch.Generator().manual_seed(3)).to(DEV)
    plain = head.generate_without_action(prompt, do_sample=True, max_new_tokens=50, uniforms=uni)
    c0 = counter()
    out, hid = head.generate_without_action(prompt, do_sample=True, max_new_tokens=50, uniforms=uni, output_frame_hidden_states=True)
    assert counter() - c0 == 3
    assert hid.shape == (2, 3, ref["cfg"]["hidden_size"]) and torch.isfinite(hid).all()
    assert torch.equal(out, plain)


# ------------------------------------------------------------------------------------------------ 5. count, edges, refusals (C ABI)
SENT_F, SENT_I, GUARD = -777.25, -12345, 64


class Guarded:
    """A device buffer of ``n`` elements with GUARD sentinel elements on both sides, all filled with the sentinel."""

    def __init__(self, n, dtype, sentinel):
        self.n, self.sent = n, sentinel
        self.buf = torch.full((n + 2 * GUARD,), sentinel, dtype=dtype, device=DEV)
        self.view = self.buf[GUARD:GUARD + n]

    def guards_intact(self):
        return bool((self.buf[:GUARD] == self.sent).all() and (self.buf[GUARD + self.n:] == self.sent).all())

    def untouched(self):
        return bool((self.buf == self.sent).all())

    def filled(self):
        return bool((self.view != self.sent).all())


def raw_frames(eng, prompt, B, L0, n_new, actions, ctx, ids, fr, fh, uniforms=None, group=1, kept=0, force=0):
    from ivideogpt_amd.engine import _ptr
    act_T = actions.shape[1] if actions is not None else 0
    with eng.stream() as s:
        rc = eng.lib.ivg_generate_frames(eng.h, _ptr(prompt), prompt.stride(0), B, L0, n_new, _ptr(actions), act_T, ctx, _ptr(uniforms), 100,
                                         group, kept, force, _ptr(ids), _ptr(fr), _ptr(fh), s)
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("n_new,frames", [(17, 1), (33, 1), (34, 2)])
def test_frame_count_and_nothing_written_beyond(n_new, frames):
    ref, prompt, table = fixture_inputs()
    head = make_head()
    eng = head.llm._ensure(2, table.shape[1])
    H = ref["cfg"]["hidden_size"]
    ids, fr, fh = Guarded(2 * (514 + n_new), torch.int64, SENT_I), Guarded(2 * frames, torch.float32, SENT_F), Guarded(2 * frames * H, torch.float32, SENT_F)
    c0 = counter()
    assert raw_frames(eng, prompt, 2, 514, n_new, table, 2, ids.view, fr.view, fh.view) == OK
    assert counter() - c0 == frames
    for b in (ids, fr, fh):
        assert b.guards_intact() and b.filled()
    # the rows are those of the Python call (which reads the same entry) and, with both outputs NULL, of ivg_generate
    ids2 = Guarded(2 * (514 + n_new), torch.int64, SENT_I)
    c0 = counter()
    assert raw_frames(eng, prompt, 2, 514, n_new, table, 2, ids2.view, None, None) == OK
    assert counter() == c0, "a call without frame outputs must not run the frame kernel"
    plain = head.generate(prompt, do_sample=False, max_new_tokens=n_new, action=table)
    assert torch.equal(ids2.view.view(2, -1), plain) and torch.equal(ids.view.view(2, -1), plain)
    want = ref["frame_rewards"][:, :frames]
    assert (fr.view.view(2, frames).cpu() - want).abs().max().item() < 1e-3


def test_refusals_leave_outputs_and_kept_cache_untouched():
    ref, prompt, table = fixture_inputs()
    head = make_head()
    eng = head.llm._ensure(2, table.shape[1])
    first = head.generate(prompt, do_sample=False, max_new_tokens=17, action=table)          # keeps the cache of 514 + 16 positions
    grown = first.contiguous()                                                                 # (B, 531): ends with the forced sdf
    ids, fr, fh = Guarded(2 * 1100, torch.int64, SENT_I), Guarded(2 * 64, torch.float32, SENT_F), Guarded(2 * 64 * 128, torch.float32, SENT_F)
    other = grown.clone()
    other[0, 520] = (other[0, 520] + 1) % 100
    long_prompt = torch.cat([prompt, prompt[:, :1]], 1).contiguous()                           # L0 = 515
    cases = {
        "n_new = 16": (INVALID, dict(prompt=prompt, L0=514, n_new=16, actions=table)),
        "unforced schedule": (INVALID, dict(prompt=prompt, L0=514, n_new=17, actions=None)),
        "(L0 - 257 ctx) % 17 != 0": (INVALID, dict(prompt=long_prompt, L0=515, n_new=17, actions=table)),
        "the same without actions": (INVALID, dict(prompt=long_prompt, L0=515, n_new=17, actions=None, force=1)),
        "kept cache with a group": (INVALID, dict(prompt=grown, L0=531, n_new=17, actions=table, kept=1, group=2)),
        "cache built from another prefix": (INVALID, dict(prompt=other, L0=531, n_new=17, actions=table, kept=1)),
        "cache of another length": (INVALID, dict(prompt=prompt, L0=514, n_new=17, actions=table, kept=1)),
        "beyond the cache": (CAPACITY, dict(prompt=prompt, L0=514, n_new=511, actions=table)),
    }
    c0 = counter()
    for what, (status, kw) in cases.items():
        rc = raw_frames(eng, kw["prompt"], 2, kw["L0"], kw["n_new"], kw["actions"], 2, ids.view, fr.view, fh.view, group=kw.get("group", 1),
                        kept=kw.get("kept", 0), force=kw.get("force", 0))
        assert rc == status, f"{what}: status {rc}, expected {status}"
        assert ids.untouched() and fr.untouched() and fh.untouched(), f"{what}: an output was written"
    assert counter() == c0
    # the kept cache is still the first call's: the continuation is accepted (verified on the device) and gives the greedy tokens
    assert raw_frames(eng, grown, 2, 531, 17, table, 2, ids.view[:2 * 548], fr.view[:2], None, kept=1) == OK
    cont = ids.view[:2 * 548].view(2, 548)
    assert torch.equal(cont[:, 531:547].cpu(), torch.from_numpy(ref["g"]["step_tokens"][1]))
    assert (fr.view[:2].cpu() - ref["frame_rewards"][:, 1]).abs().max().item() < 1e-3, "frame 0 of the continuation is step 1 of the fixture"
    # rewards without a head
    bare = make_head(reward=False)
    beng = bare.llm._ensure(2, table.shape[1])
    fr2, ids3 = Guarded(2, torch.float32, SENT_F), Guarded(2 * 531, torch.int64, SENT_I)
    assert raw_frames(beng, prompt, 2, 514, 17, table, 2, ids3.view, fr2.view, None) == MISSING
    assert fr2.untouched() and ids3.untouched()
    assert raw_frames(beng, prompt, 2, 514, 17, table, 2, ids3.view, None, None) == OK     # (hidden states and tokens need no reward head)


# ------------------------------------------------------------------------------------------------ 6. the second cache chunk
def test_rows_of_the_second_chunk():
    """B = 130 > the 128-row cache chunk: rows 126 .. 129 (two of each chunk) equal the same rows run alone as a batch of 4."""
    ref, prompt, _ = fixture_inputs()
    g = torch.Generator().manual_seed(19)
    V = ref["cfg"]["vocab_size"]
    ids = prompt[torch.arange(130) % 2].clone()
    ids[:, 5:200] = torch.randint(0, V - 2, (130, 195), generator=g).to(DEV)
    table = torch.randn(130, 3, 4, generator=g).to(DEV)
    head = make_head()
    c0 = counter()
    out, rew, hid = head.generate(ids, do_sample=False, max_new_tokens=16, action=table, return_reward="frames", output_frame_hidden_states=True)
    assert counter() - c0 == 2, "one hit per chunk"
    assert out.shape == (130, 530) and rew.shape == (130, 1) and hid.shape == (130, 1, 128)
    sel = slice(126, 130)
    o4, r4, h4 = head.generate(ids[sel].contiguous(), do_sample=False, max_new_tokens=16, action=table[sel].contiguous(), return_reward="frames",
                               output_frame_hidden_states=True)
    assert torch.equal(out[sel], o4), "tokens of rows 126..129 differ from the batch of 4"
    dr, dh = (rew[sel] - r4).abs().max().item(), (hid[sel] - h4).abs().max().item()
    print(f"rows 126..129 vs alone: rewards {dr:.3e}, hidden {dh:.3e}")
    assert torch.equal(rew[sel], r4) and torch.equal(hid[sel], h4)


# ------------------------------------------------------------------------------------------------ 7. the off path
def test_plain_generate_after_a_frames_call_is_unchanged():
    ids, table, uni = three_rows(23)
    u = uni[:, :50].contiguous()
    fresh = make_head().generate(ids, do_sample=True, max_new_tokens=50, action=table, uniforms=u)
    head = make_head()
    head.generate(ids, do_sample=True, max_new_tokens=50, action=table, uniforms=uni, return_reward="frames", output_frame_hidden_states=True)
    c0 = counter()
    again, r = head.generate(ids, do_sample=True, max_new_tokens=50, action=table, uniforms=u, return_reward=True)
    assert counter() == c0, "a plain generate ran the frame kernel"
    assert torch.equal(again, fresh) and r.shape == (3,)


# ------------------------------------------------------------------------------------------------ 8. VideoPredictor.rollout_actions
class Dealer:
    """Stands in for ``LlamaForCausalLM._uniforms``: deals consecutive columns of one table, so that ``rollout`` (17 per step) and
    ``rollout_actions`` (17 * horizon - 1 at once) draw the same numbers for the same new tokens."""

    def __init__(self, table):
        self.table, self.col = table, 0

    def __call__(self, B, n, do_sample, generator):
        u = self.table[:B, self.col:self.col + n].contiguous()
        self.col += n
        return u


def test_rollout_actions_matches_rollout(tmp_path):
    """Open loop against closed loop with a policy that replays the same actions, both drawing from one table of uniforms: actions
    and rewards EQUAL (``rollout_actions`` applies ``reward_linear`` to the frame hidden states, ``rollout``'s own arithmetic),
    observations within 1e-3, the fp32 pixel bar (one whole-clip decode against the step-wise cached one).  ``samples=2`` against
    the two candidates run alone: same actions; rewards and observations within 1e-3 -- a shared context feeds the prompt's last
    position through the decode-step kernels instead of the prompt pass (include/ivg.h ivg_generate_shared: identical up to that
    rounding), so the two are not bit-comparable; measured 1.9e-6 on the rewards, 0 on the observations."""
    from helpers import world_model_files
    from mbrl.video_predictor import VideoPredictor
    args, *_ = world_model_files(tmp_path, False)
    args.update(encode_dtype="fp32", decode_dtype="fp32", llm_dtype="fp32")
    vp = VideoPredictor("cuda", args)
    g = torch.Generator().manual_seed(8)
    obs = torch.randint(0, 256, (2, 9, 64, 64), generator=g).float()
    acts = torch.randn(2, 3, 4, generator=g)
    table = torch.rand(4, 51, generator=g).to(DEV)
    llm = vp.model.llm
    llm._uniforms = Dealer(table)
    o1, a1, r1 = vp.rollout(obs, lambda o, t: acts[:, t], 3)
    llm._uniforms = Dealer(table)
    c0 = counter()
    o2, a2, r2 = vp.rollout_actions(obs, acts)
    assert counter() - c0 == 3
    assert o2.shape == o1.shape == (2, 4, 9, 64, 64) and a2.shape == a1.shape and r2.shape == r1.shape == (2, 4, 1)
    assert torch.equal(a2, a1)
    dr, do = (r2 - r1).abs().max().item(), (o2 - o1).abs().max().item()
    print(f"rollout_actions vs rollout: rewards {dr:.3e}, observations {do:.3e}")
    assert torch.equal(r2, r1), f"rewards differ by {dr:.3e}"
    assert do < 1e-3
    # samples = 2: rows b * 2 + k are candidate k of observation b; equal to the two candidates run as calls of their own
    acts4 = torch.randn(4, 3, 4, generator=g)
    del llm._uniforms
    o4, a4, r4 = vp.rollout_actions(obs, acts4, samples=2, uniforms=table[:, :50])
    assert o4.shape == (4, 4, 9, 64, 64) and r4.shape == (4, 4, 1)
    for k in range(2):
        ok, ak, rk = vp.rollout_actions(obs, acts4[k::2], uniforms=table[k::2, :50])
        assert torch.equal(a4[k::2], ak)
        dr, do = (r4[k::2] - rk).abs().max().item(), (o4[k::2] - ok).abs().max().item()
        print(f"candidate {k}: shared vs alone: rewards {dr:.3e}, observations {do:.3e}")
        assert dr < 1e-3 and do < 1e-3
