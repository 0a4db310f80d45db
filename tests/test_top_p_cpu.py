"""Nucleus (top-p) sampling without a GPU: the fp64 restatement of the engine's contract (tests/top_p_ref.py) against HF's own
warpers, and the argument checks of every generate entry, which run before any engine work."""
import math

import pytest
import torch

from top_p_ref import hf_survivors, nucleus, sample


@pytest.mark.parametrize("temperature", [1.0, 0.7])
@pytest.mark.parametrize("top_p", [0.0, 0.3, 0.9, 0.999, 1.0])
@pytest.mark.parametrize("top_k", [1, 100, 1000, None])
@pytest.mark.parametrize("V", [70, 8194, 16386])
def test_restatement_equals_hf_warpers(V, top_k, top_p, temperature):
    """Temperature -> TopK -> TopP of the installed transformers keep exactly the restatement's survivors, except on rows where the
    nucleus boundary is near a kept token's cumulative mass or falls inside a group of tied logits.  HF's fp32 cumsum errs in
    proportion to the mass summed up to the boundary, 1 - top_p, so "near" is 1e-5 of that (at least 1e-5 of 0.01)."""
    pytest.importorskip("transformers")
    g = torch.Generator().manual_seed(V * 7 + (top_k or 0) + int(top_p * 1000) + int(temperature * 10))
    B = 16
    logits = torch.randn(B, V, generator=g) * 3
    logits[1, 7] = float("-inf")
    logits[2] = torch.round(logits[2])          # heavy ties
    want = hf_survivors(logits, top_k, top_p, temperature)
    got, _, near, tie = nucleus(logits, top_k, top_p, temperature, tol=1e-5 * max(1.0 - top_p, 0.01))
    skip = near | tie
    assert (~skip).sum() >= B // 2, f"{int(skip.sum())} of {B} rows flagged"
    bad = [b for b in range(B) if not skip[b] and not torch.equal(got[b], want[b])]
    assert not bad, f"rows {bad} differ from HF's warpers"
    if top_p == 0.0:
        assert (got.sum(-1)[~tie] == 1).all(), "top_p = 0 keeps the maximum alone (no ties)"


def test_restatement_top_p_one_is_the_oracle_sampler():
    from oracle.llama import sample_from_logits
    g = torch.Generator().manual_seed(3)
    logits = torch.randn(32, 8194, generator=g) * 3
    u = torch.rand(32, generator=g)
    for k in (100, 1000):
        tok, near = sample(logits, k, 1.0, u)
        assert torch.equal(tok, sample_from_logits(logits, k, u)) and not near.any()


def test_restatement_ties_at_the_boundary_are_kept():
    """four tokens tied at the nucleus boundary: all of them survive (HF's sort would pick some)."""
    logits = torch.tensor([[5.0, 1.0, 1.0, 0.0, 1.0, 1.0, -2.0]])
    e = torch.exp(logits.double() - 5.0)
    p = float(1.0 - (e[0, 3] + e[0, 6] + 2 * e[0, 1]) / e.sum())   # the boundary in the middle of the tied group
    keep, _, near, tie = nucleus(logits, None, p)
    assert keep[0].tolist() == [True, True, True, False, True, True, False] and tie[0]


class _NoEngine:
    """stands in for the engine: any use fails the test (validation has to happen first)"""
    def __getattr__(self, name):
        raise AssertionError(f"engine touched ({name}) before top_p was validated")


@pytest.mark.parametrize("bad", [1.5, -0.1, math.nan])
def test_generate_rejects_invalid_top_p_before_any_engine_work(bad):
    from ivideogpt_amd import HeadModelWithAction, LlamaForCausalLM
    from ivideogpt_amd import weights as W
    cfg = dict(W.LLAMA_SMALL, hidden_size=64, intermediate_size=128, num_hidden_layers=1, num_attention_heads=2, num_key_value_heads=2)
    m = LlamaForCausalLM(cfg, None, dtype="fp32")
    m._ensure = lambda *a, **k: _NoEngine()
    ids = torch.zeros(2, 514, dtype=torch.int64)
    with pytest.raises(ValueError, match="top_p"):
        m.generate(ids, do_sample=True, top_k=100, max_new_tokens=4, top_p=bad)
    with pytest.raises(ValueError, match="top_p"):
        m.generate(ids, do_sample=True, max_new_tokens=4, top_p=bad, shared_context=2)
    with pytest.raises(ValueError, match="top_p"):
        m.generate(inputs_embeds=torch.zeros(2, 3, 64), do_sample=True, max_new_tokens=4, top_p=bad)
    head = HeadModelWithAction(m, 4, 513, 16, 2, 5)
    with pytest.raises(ValueError, match="top_p"):
        head.generate(ids, do_sample=True, max_new_tokens=16, action=torch.zeros(2, 5, 4), top_p=bad)
    with pytest.raises(ValueError, match="top_p"):
        head.generate_without_action(ids, do_sample=True, max_new_tokens=16, top_p=bad)


def test_top_p_argument_values():
    """as HF's TopPLogitsWarper: float(top_p) in [0, 1], checked only when sampling; NaN refused as well"""
    import numpy as np
    from ivideogpt_amd.transformer import _top_p_of
    assert _top_p_of(None, True) == 1.0 and _top_p_of(1, True) == 1.0 and _top_p_of(0, True) == 0.0
    assert _top_p_of(0.9, True) == 0.9
    assert _top_p_of(np.float32(0.5), True) == 0.5 and _top_p_of(torch.tensor(0.25), True) == 0.25 and _top_p_of("0.75", True) == 0.75
    assert _top_p_of(0.9, False) == 1.0, "greedy: no warper runs, top_p has no effect"
    assert _top_p_of(1.5, False) == 1.0, "greedy: HF never builds the warper, so it does not check the value either"
    for bad in (2, -0.5, math.nan, "x"):
        with pytest.raises(ValueError):
            _top_p_of(bad, True)


def test_predict_cli_top_p_flag():
    from inference.predict import parse_args
    base = ["--pretrained_model_name_or_path", "x", "--input_path", "y", "--dataset_name", "z"]
    assert parse_args(base).top_p is None, "absent by default: the reference's command line is unchanged"
    assert parse_args(base + ["--top_p", "0.9"]).top_p == 0.9
