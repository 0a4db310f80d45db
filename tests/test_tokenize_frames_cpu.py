"""Host-side halves of the encoder context cache and the closed loop that need no GPU: where a frame's tokens sit in a ``tokenize`` row,
argument errors of ``EncodeCache.select`` before any engine call, no CPU fallback, and the new C entries in the library."""
from types import SimpleNamespace

import pytest
import torch


class NoEngine:
    """Stands where an Engine would: any use is a failure of the test."""
    h = object()

    def __getattr__(self, name):
        raise AssertionError(f"the engine was called ({name})")


@pytest.mark.parametrize("ctx", [1, 2])
def test_frame_token_columns_follow_the_reference_layout(ctx):
    """compressive_vq_model.py:205-215: per context frame 256 tokens and a separator slot (scf, the last one sdf), then per future frame
    16 dyn tokens and sdf, the row's last sdf cut off.  Built here with tags instead of tokens: (frame, j) for dyn token j of a frame."""
    from ivideogpt_amd.vq_model import CTX_TOKENS, DYN_TOKENS, frame_token_columns
    F = 3
    row = []
    for c in range(ctx):
        row += [("ctx", c, j) for j in range(256)] + ["sdf" if c == ctx - 1 else "scf"]
    for f in range(F):
        row += [("dyn", f, j) for j in range(16)] + ["sdf"]
    row = row[:-1]
    assert len(row) == CTX_TOKENS * ctx - 1 + DYN_TOKENS * F
    for f in range(F):
        a, b = frame_token_columns(ctx, f)
        assert b - a == 16 and row[a:b] == [("dyn", f, j) for j in range(16)]
        assert row[a - 1] == "sdf" and (f == F - 1 or row[b] == "sdf")
    # what tokenize_frames returns for frames 0 .. n - 1 is row[first(0) : first(0) + 17 n - 1] plus the next slot's sdf
    a0 = frame_token_columns(ctx, 0)[0]
    assert a0 == 257 * ctx and frame_token_columns(ctx, 2)[1] == a0 + 17 * 3 - 1


@pytest.mark.parametrize("bad", [[], [0, 2], [-1], [0.5], [True], [[0, 1]], "ab"])
def test_encode_cache_select_argument_errors_come_before_the_engine(bad):
    from ivideogpt_amd.vq_model import EncodeCache
    cache = EncodeCache(NoEngine(), 2, 2, torch.zeros(2, 2, 3, 8, 8), handle=object())
    with pytest.raises(ValueError):
        cache.select(bad)
    cache.handle = None   # (nothing to release)


def test_no_cpu_fallback(tmp_path):
    from helpers import world_model_files
    from ivideogpt_amd import CompressiveVQModel
    from ivideogpt_amd.vq_model import EncodeCache
    from mbrl.video_predictor import VideoPredictor
    args, tcfg, tsd, *_ = world_model_files(tmp_path, False)
    tok = CompressiveVQModel(tcfg, tsd)
    px = torch.zeros(1, 3, 3, 64, 64)
    with pytest.raises(RuntimeError, match="MI355X"):
        tok.encode_context(px, 2, return_cache=True)
    cache = EncodeCache(NoEngine(), 1, 2, px[:, :2], handle=None)
    with pytest.raises(RuntimeError, match="MI355X"):
        tok.tokenize_frames(px[:, 2:], cache)
    with pytest.raises(AssertionError):
        tok.tokenize_frames(px[:, 2:], object())
    vp = VideoPredictor("cpu", SimpleNamespace(**args))
    with pytest.raises(RuntimeError, match="MI355X"):
        vp.track(torch.zeros(1, 9, 64, 64))


def test_library_exports_the_encoder_cache_entries():
    from ivideogpt_amd import _lib
    lib = _lib.load()
    for name in ("ivg_enc_cache_create", "ivg_enc_cache_destroy", "ivg_encode_context_cached", "ivg_tokenize_frames", "ivg_enc_cache_select"):
        assert name in _lib.EXPORTS and getattr(lib, name)
    for name in (b"enc_plain_images", b"enc_cond_images", b"enc_kv_projections"):
        assert lib.ivg_debug_counter(name) >= 0
