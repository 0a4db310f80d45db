"""CPU checks of the token scores (include/ivg.h ivg_generate_scored): the fp32 restatement of token_scores_kernel's reduction against
the fp64 reference of tests/token_scores_ref.py on every case of the table, mutants that must each miss the bound on a named case, the
definition against HF's own ``compute_transition_scores`` offline, the binding tables, and the no-fallback error without a GPU."""
import os
import re

import numpy as np
import pytest
import torch

import token_scores_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTPUTS = ("logprob", "entropy", "max_logprob")


def _row_errors(fn):
    """case name -> per-output pass flags of ``fn(z, tok)`` against the fp64 reference under the bound."""
    res = {}
    for name, z, tok in R.case_rows():
        want = R.reference(z[None], [tok])[0]
        res[name] = (R.within(fn(z, tok), want), fn(z, tok), want)
    return res


def test_fp32_restatement_passes_every_case():
    """Measured: worst |fp32 - fp64| 1.5e-6 over the table (V up to 18,432, sigma up to 12, spike and -inf rows)."""
    worst = 0.0
    for name, (ok, got, want) in _row_errors(R.kernel_fp32).items():
        fin = np.isfinite(want)
        if fin.any():
            worst = max(worst, float(np.abs(got[fin] - want[fin]).max()))
        for k, out in enumerate(OUTPUTS):
            assert ok[k], f"{name}: {out} {got[k]!r} against fp64 {want[k]!r}"
    print(f"worst |fp32 restatement - fp64| = {worst:.2e}")
    z, tok = R.cases()["nonfinite"]
    for b in range(z.shape[0]):
        assert np.isnan(R.kernel_fp32(z[b], int(tok[b]))).all() and np.isnan(R.reference(z[b:b + 1], tok[b:b + 1])).all(), f"nonfinite row {b}"


def test_reference_knows_its_closed_forms():
    """A constant row: entropy = log V, logprob = max_logprob = -log V; a -inf id: logprob = -inf; greedy: logprob == max_logprob."""
    for name, (z, tok) in R.cases().items():
        if name == "nonfinite":
            continue
        V = z.shape[1]
        ref = R.reference(z, tok)
        assert abs(ref[2, 1] - np.log(V)) < 1e-12 and abs(ref[2, 0] + np.log(V)) < 1e-12 and abs(ref[2, 2] + np.log(V)) < 1e-12, name
        assert ref[3, 0] == -np.inf, name
        assert ref[1, 0] == ref[1, 2] and ref[4, 0] == ref[4, 2], name
        assert (ref[:, 1] >= 0).all() and (ref[:, 1] <= np.log(V) + 1e-12).all(), name
        assert abs(ref[4, 1] - R.reference(z[4:5, np.isfinite(z[4])], [0])[0, 1]) < 1e-12, f"{name}: -inf entries carry no entropy"


@pytest.mark.parametrize("mutant", list(R.ROW_MUTANTS))
def test_row_mutants_miss_the_bound(mutant):
    fn, case = R.ROW_MUTANTS[mutant]
    res = _row_errors(fn)
    failing = [n for n, (ok, _, _) in res.items() if not ok.all()]
    print(f"{mutant}: misses the bound on {len(failing)} of {len(res)} cases")
    ok, got, want = res[case]
    assert not ok.all(), f"the mutant '{mutant}' passes case {case}: {got!r} against {want!r}"


@pytest.mark.parametrize("mutant", list(R.COLUMN_MUTANTS))
def test_column_mutants_miss_the_bound(mutant):
    rows, toks = R.column_case()
    want = R.reference_columns(rows, toks, R.PER)
    good = R.kernel_columns(rows, toks, R.PER)
    assert R.within(good, want).all() and (good[16] == 0).all(), "the step loop itself must pass case columns/V130"
    got = R.kernel_columns(rows, toks, R.PER, **R.COLUMN_MUTANTS[mutant])
    assert not R.within(got, want).all(), f"the mutant '{mutant}' passes case columns/V130"


def test_reference_logprob_is_hf_transition_score():
    """A seeded 2-layer random HF LlamaForCausalLM, ``generate(output_logits=True)`` sampled with temperature 0.7 and top-k 100:
    ``compute_transition_scores(sequences, logits, normalize_logits=True)`` is the reference's logprob on HF's logits within 1e-5
    (HF's ``logits`` are the raw rows, before the temperature and the filter)."""
    import transformers
    torch.manual_seed(0)
    cfg = transformers.LlamaConfig(vocab_size=300, hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=2,
                                   num_key_value_heads=2, max_position_embeddings=64)
    model = transformers.LlamaForCausalLM(cfg).eval()
    prompt = torch.randint(0, 300, (3, 5))
    out = model.generate(prompt, do_sample=True, temperature=0.7, top_k=100, max_new_tokens=12, output_logits=True, return_dict_in_generate=True,
                         pad_token_id=0)
    hf = model.compute_transition_scores(out.sequences, out.logits, normalize_logits=True).double().numpy()   # (B, 12)
    new = out.sequences[:, prompt.shape[1]:].numpy()
    worst = 0.0
    for j, z in enumerate(out.logits):
        ref = R.reference(z.float().numpy(), new[:, j])
        worst = max(worst, float(np.abs(ref[:, 0] - hf[:, j]).max()))
    print(f"reference logprob vs HF transition scores: {worst:.2e}")
    assert worst < 1e-5


def _header_params(name):
    text = open(os.path.join(ROOT, "include", "ivg.h")).read()
    m = re.search(r"\bint " + name + r"\((.*?)\);", text, re.S)
    assert m, f"{name} is not declared in include/ivg.h"
    return [p for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",") if p.strip()]


def test_header_bindings_and_engine_agree():
    from ivideogpt_amd import _lib
    from ivideogpt_amd.engine import Engine
    for name, base, extra in (("ivg_generate_scored", "ivg_generate_frames", 1), ("ivg_generate_embeds_scored", "ivg_generate_embeds", 1),
                              ("ivg_op_token_scores", None, 0)):
        params = _header_params(name)
        res, args = _lib.EXPORTS[name]
        assert len(args) == len(params), f"{name}: {len(params)} parameters in the header, {len(args)} in _lib.EXPORTS"
        if base:
            assert len(args) == len(_lib.EXPORTS[base][1]) + extra and len(params) == len(_header_params(base)) + extra
            assert "token_scores_out" in params[-2]
    assert len(_lib.EXPORTS["ivg_generate_scored"][1]) == 19 and len(_lib.EXPORTS["ivg_op_token_scores"][1]) == 6
    assert callable(Engine.rollout) and "token_scores" in Engine.generate_embeds.__code__.co_varnames
    assert "token_scores" in Engine.rollout.__code__.co_varnames


def test_per_frame_sums_and_means_the_sampled_columns():
    from ivideogpt_amd import TokenScores
    g = torch.Generator().manual_seed(2)
    lp, en = -torch.rand(2, 50, generator=g), torch.rand(2, 50, generator=g)
    lp[:, 16::17] = 0
    en[:, 16::17] = 0
    flp, fen = TokenScores(lp, en, lp.clone()).per_frame()
    assert flp.shape == fen.shape == (2, 3)
    want_lp = torch.stack([lp[:, 17 * i:17 * i + 16].double().sum(1) for i in range(3)], 1)
    want_en = torch.stack([en[:, 17 * i:17 * i + 16].double().mean(1) for i in range(3)], 1)
    assert (flp.double() - want_lp).abs().max() < 1e-5 and (fen.double() - want_en).abs().max() < 1e-6
    one = TokenScores(lp[:, 17:34], en[:, 17:34], lp[:, 17:34]).per_frame()      # a 17-token step: the same bits as frame 1 of the long call
    assert torch.equal(one[0][:, 0], flp[:, 1]) and torch.equal(one[1][:, 0], fen[:, 1])


def test_without_a_gpu_token_scores_raise_the_no_fallback_error():
    """``output_token_scores=True`` is an argument the models know (no TypeError) and, as every product path, fails loudly without a
    GPU: there is no eager fallback."""
    from helpers import llama_fixture
    from ivideogpt_amd import HeadModelWithAction, LlamaForCausalLM
    import frame_heads_ref as F
    cfg, _, g = llama_fixture("llama_tiny_ctx2_mbrl.npz")
    ctx = int(g["ctx"])
    sd = F.fixture_state_dict(cfg, g)
    head = HeadModelWithAction(LlamaForCausalLM(cfg, None, dtype="fp32"), int(g["action_dim"]), 257 * ctx - 1, 16, ctx, ctx + 3, reward_prediction=True)
    head.load_state_dict(sd, strict=True)
    prompt, table = torch.from_numpy(g["prompt"]), F.fixture_action_table(g)
    for kw in (dict(), dict(return_reward="frames"), dict(output_frame_hidden_states=True)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            head.generate(prompt, do_sample=False, max_new_tokens=50, action=table, output_token_scores=True, **kw)
    with pytest.raises(RuntimeError, match="no CPU path"):
        head.generate_without_action(prompt, do_sample=False, max_new_tokens=50, output_token_scores=True)
    with pytest.raises(RuntimeError, match="no CPU path"):
        head.llm.generate(prompt, do_sample=False, max_new_tokens=5, output_token_scores=True)
    with pytest.raises(ValueError, match="17"):
        head.generate(prompt, do_sample=False, max_new_tokens=50, action=table, output_token_scores=True, return_reward=True)
