"""CPU self-check of tests/frame_heads_ref.py (the contract of include/ivg.h ivg_generate_frames) against the REFERENCE's own per-step
outputs (tests/golden/llama_tiny_ctx2_mbrl.npz), the frame count against a literal walk of the step loop, and the argument checks of
``HeadModelWithAction.generate`` that need no GPU."""
import numpy as np
import pytest
import torch

import frame_heads_ref as R


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
def test_reference_reproduces_the_fixture(dtype):
    """The teacher-forced pass alone gives the reference's ``step_rewards`` (measured: 2.4e-6 in fp32, 7.8e-7 in fp64) and decides
    greedily every one of its 96 ``step_tokens``, with a top-2 logit margin (measured 3.5e-3) above the 1e-3 logits bar: the greedy
    tokens of the fixture are decided, not near-ties."""
    ref = R.fixture_reference(dtype=dtype)
    g = ref["g"]
    err = np.abs(ref["frame_rewards"].double().numpy().T - g["step_rewards"]).max()   # fixture: (steps, B)
    print(f"rewards vs fixture ({dtype}): {err:.2e}")
    assert err < 1e-5
    toks, margin = R.greedy_margin_and_tokens(ref)
    print(f"smallest top-2 margin ({dtype}): {margin:.2e}")
    assert np.array_equal(toks, g["step_tokens"])
    assert margin > 1e-3


def test_frame_count_is_n_new_over_17():
    for n_new in range(16, 53):
        assert R.frames_out(n_new) == R.frames_by_walking_the_step_loop(n_new) == n_new // 17, n_new
    assert [R.frames_out(n) for n in (16, 17, 33, 34, 50, 51)] == [0, 1, 1, 2, 2, 3]
    assert R.frame_positions(2, 3) == [529, 546, 563]


def _cpu_head(reward=True):
    from helpers import llama_fixture
    from ivideogpt_amd import HeadModelWithAction, LlamaForCausalLM
    cfg, _, g = llama_fixture("llama_tiny_ctx2_mbrl.npz")
    ctx = int(g["ctx"])
    return HeadModelWithAction(LlamaForCausalLM(cfg, None, dtype="fp32"), int(g["action_dim"]), 257 * ctx - 1, 16, ctx, ctx + 4,
                               reward_prediction=reward), g


@pytest.mark.parametrize("bad", [17, 49, 51, 15, 0])
def test_generate_refuses_a_length_without_whole_frames(bad):
    head, g = _cpu_head()
    prompt, table = torch.from_numpy(g["prompt"]), R.fixture_action_table(g)
    with pytest.raises(ValueError, match="17"):
        head.generate(prompt, do_sample=False, max_new_tokens=bad, action=table, return_reward="frames")
    with pytest.raises(ValueError, match="17"):
        head.generate(prompt, do_sample=False, max_new_tokens=bad, action=table, output_frame_hidden_states=True)
    with pytest.raises(ValueError, match="17"):
        head.generate_without_action(prompt, do_sample=False, max_new_tokens=bad, output_frame_hidden_states=True)


def test_generate_refuses_other_bad_frame_arguments():
    head, g = _cpu_head()
    prompt, table = torch.from_numpy(g["prompt"]), R.fixture_action_table(g)
    with pytest.raises(ValueError, match="frames"):
        head.generate(prompt, do_sample=False, max_new_tokens=50, action=table, return_reward="every")
    with pytest.raises(ValueError, match="return_reward"):
        head.generate(prompt, do_sample=False, max_new_tokens=50, action=table, return_reward=True, output_frame_hidden_states=True)
    bare, _ = _cpu_head(reward=False)
    with pytest.raises(ValueError, match="reward_prediction"):
        bare.generate(prompt, do_sample=False, max_new_tokens=50, action=table, return_reward="frames")


def test_binding_table_has_the_entry():
    from ivideogpt_amd import _lib
    res, args = _lib.EXPORTS["ivg_generate_frames"]
    assert len(args) == 18   # engine, prompt, stride, B, L0, n_new, actions, act_T, ctx, uniforms, top_k, group, kept, force, ids, rewards, hidden, stream
