"""Saving and restoring the kept K / V cache (include/ivg.h ivg_kv_snapshot_*), the parts that need no GPU: the life cycle of
``KeptCache`` and what ``save_kept_cache`` / ``restore_kept_cache`` hand the engine, with a stub engine; the order in which
``VideoPredictor`` suspends and resumes its sessions, with stub sessions; the refusals of the C entries that come before any device work."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch


class StubLib:
    """What ``KeptCache`` calls: info (rows 3, length 530, 4096 bytes, from ids, act_T 4, ctx 2, native, device 0) and destroy."""

    def __init__(self):
        self.destroyed = []

    def ivg_kv_snapshot_info(self, h, out):
        for i, v in enumerate((3, 530, 4096, 0, 4, 2, 0, 0)):
            out[i] = v
        return 0

    def ivg_kv_snapshot_destroy(self, h):
        self.destroyed.append(h)


def kept_cache(lib=None):
    from ivideogpt_amd import KeptCache
    return KeptCache(lib or StubLib(), object())


def test_kept_cache_life_cycle():
    lib = StubLib()
    k = kept_cache(lib)
    h = k.h
    assert (k.rows, k.length, k.nbytes, k.from_embeds, k.act_T, k.ctx) == (3, 530, 4096, False, 4, 2) and not k.closed
    k.close()
    assert k.closed and lib.destroyed == [h]
    k.close()
    assert lib.destroyed == [h], "close() is idempotent"
    with kept_cache(lib) as k2:
        assert not k2.closed
    assert k2.closed and len(lib.destroyed) == 2
    k3 = kept_cache(lib)
    del k3
    assert len(lib.destroyed) == 3, "garbage collection releases the snapshot"


class StubEngine:
    max_batch, max_frames = 4, 32

    def __init__(self):
        self.calls, self.fail = [], None

    def kv_snapshot(self):
        self.calls.append(("snapshot",))
        return kept_cache()

    def kv_restore(self, kept, parents):
        if self.fail:
            raise self.fail
        self.calls.append(("restore", kept, parents))

    def close(self):
        pass


def stub_model():
    from ivideogpt_amd import HeadModelWithAction, LlamaForCausalLM, weights as W
    cfg = dict(W.LLAMA_SMALL, hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2, vocab_size=130)
    head = HeadModelWithAction(LlamaForCausalLM(cfg, None, dtype="fp32"), 4, 513, 16, 2, 5, reward_prediction=True)
    return head


def test_model_methods_hand_the_engine_normalized_parents():
    from ivideogpt_amd import _lib
    head = stub_model()
    with pytest.raises(ValueError, match="no kept cache"):
        head.save_kept_cache()
    eng = head.llm._engine = StubEngine()
    kept = head.save_kept_cache()
    assert eng.calls == [("snapshot",)] and kept.weights_version == head.llm._pack_key()
    assert head.restore_kept_cache(kept) is head and eng.calls[-1] == ("restore", kept, None)
    for parents in ([2, 2, 0], np.array([2, 2, 0], dtype=np.int64), torch.tensor([2, 2, 0])):
        head.llm.restore_kept_cache(kept, parents)
        p = eng.calls[-1][2]
        assert isinstance(p, np.ndarray) and p.dtype == np.int32 and p.tolist() == [2, 2, 0]
    head.restore_kept_cache(kept, [0, 1, 2, 0])
    assert eng.calls[-1][2].tolist() == [0, 1, 2, 0], "more rows than the snapshot has, within the engine's batch"
    n = len(eng.calls)
    for bad in ([0, 3], [-1], [], [[0, 1]], [0.5]):
        with pytest.raises(ValueError):
            head.restore_kept_cache(kept, bad)
    assert len(eng.calls) == n, "bad parents never reach the engine"
    # the engine's refusals become ValueError with the engine's text
    for err in (AssertionError("kv_snapshot_restore: libivg error -1: the snapshot was taken over other weights"), _lib.IvgError("error -4: rows exceed the KV-cache chunk")):
        eng.fail = err
        with pytest.raises(ValueError, match="restore_kept_cache: .*(other weights|KV-cache chunk)"):
            head.restore_kept_cache(kept)
    eng.fail = None
    # more rows than a cache chunk ever holds: the engine refuses, the model builds nothing
    eng.fail = _lib.IvgError("error -4: 129 rows exceed the KV-cache chunk")
    with pytest.raises(ValueError, match="129 rows"):
        head.restore_kept_cache(kept, [0] * 129)
    assert head.llm._engine is eng
    eng.fail = None
    # new weights: refused before the engine is asked
    other = stub_model()
    other.llm._engine = StubEngine()
    other.llm._sd_version += 1
    with pytest.raises(ValueError, match="other weights"):
        other.restore_kept_cache(kept)
    assert other.llm._engine.calls == []
    kept.close()
    with pytest.raises(ValueError, match="closed"):
        head.restore_kept_cache(kept)
    head.llm._engine = None


class StubSession:
    def __init__(self, name, log, predictor):
        self.name, self.log, self.p = name, log, predictor

    def suspend(self):
        self.log.append(("suspend", self.name))
        if self.p._active is self:
            self.p._active = None

    def resume(self):
        self.log.append(("resume", self.name))
        self.p._active = self


class Touched(Exception):
    """The first thing a rollout does to the models."""


class StubTokenizer:
    def __init__(self, log):
        self.log = log

    def encode_context(self, *a, **k):
        self.log.append(("model",))
        raise Touched


def test_predictor_arbitration_order():
    from mbrl.video_predictor import VideoPredictor
    log = []
    model = SimpleNamespace(llm=SimpleNamespace(_max_seq=0, _cfg={"max_position_embeddings": 1024}), action_dim=4)
    vp = VideoPredictor.from_models(StubTokenizer(log), model, device="cpu")
    a, b = StubSession("a", log, vp), StubSession("b", log, vp)
    assert vp._active is None
    vp._activate(a)
    assert log == [("resume", "a")] and vp._active is a
    vp._activate(a)
    assert log == [("resume", "a")], "the active session is neither suspended nor resumed again"
    vp._activate(b)
    assert log[1:] == [("suspend", "a"), ("resume", "b")] and vp._active is b, "the previous session is suspended first, then this one resumes"
    del log[:]
    obs = torch.zeros(1, 9, 8, 8)
    with pytest.raises(Touched):
        vp.rollout_actions(obs, torch.zeros(1, 2, 4))
    assert log == [("suspend", "b"), ("model",)] and vp._active is None, "a rollout suspends the active session before it touches the model"
    del log[:]
    with pytest.raises(Touched):
        vp.rollout(obs, lambda o, t: torch.zeros(1, 4), 1)
    assert log == [("model",)], "nobody is active: nothing to suspend"
    vp._activate(a)
    del log[:]
    with pytest.raises(Touched):
        vp.rollout(obs, lambda o, t: torch.zeros(1, 4), 1)
    assert log == [("suspend", "a"), ("model",)]
    vp._activate(b)
    del log[:]
    with pytest.raises(Touched):
        vp.track(obs.expand(1, 9, 8, 8))
    assert log[:2] == [("suspend", "b"), ("model",)], "track suspends the active session before the new one is anchored"
    with pytest.raises(ValueError, match="grow"):
        vp.track(obs, grow="sometimes")
    # two predictors do not share their arbitration
    other = VideoPredictor.from_models(StubTokenizer(log), model, device="cpu")
    vp._activate(a)
    assert other._active is None


def test_c_entries_refuse_before_any_device_work():
    from ivideogpt_amd import _lib
    lib = _lib.load()
    for name in ("ivg_kv_snapshot_create", "ivg_kv_snapshot_restore", "ivg_kv_snapshot_destroy", "ivg_kv_snapshot_info", "ivg_op_kv_snapshot"):
        assert name in _lib.EXPORTS and getattr(lib, name)
    out = C.c_void_p(0x1234)
    assert lib.ivg_kv_snapshot_create(None, C.byref(out), None) == -1 and out.value == 0x1234, "a null engine: *out is not written"
    assert lib.ivg_kv_snapshot_restore(None, None, None, 0, None) == -1
    info = (C.c_int64 * _lib.IVG_KV_SNAPSHOT_INFO_INTS)(*([7] * _lib.IVG_KV_SNAPSHOT_INFO_INTS))
    assert lib.ivg_kv_snapshot_info(None, info) == -1 and list(info) == [7] * 8
    lib.ivg_kv_snapshot_destroy(None)
    assert lib.ivg_op_kv_snapshot(None, 2, 8, 2, 40, 16, 0, 1, 1, None, 0, None, 0, 0, None) == -1
    assert lib.ivg_debug_counter(b"kv_snapshot_rows_saved") >= 0 and lib.ivg_debug_counter(b"kv_snapshot_rows_restored") >= 0
