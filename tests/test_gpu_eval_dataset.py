"""Evaluation on a test set of npz episodes, on the device: ``ivg_ingest_clips`` (the batched ingest kernel) against
``ivg_ingest_frames`` clip by clip and against torch, its refusals, ``EvalDataLoader(device='cuda')`` against the host path, and
``train_gpt.evaluate`` / ``train_gpt.main`` fed by the loader."""
import ctypes as C
import json
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CLIPS = [(1, 48, 64), (5, 64, 48), (8, 33, 21), (11, 32, 32)]   # (frames, H, W): padding from one frame, padding, odd row length, truncation + no resize
T_OUT, R_OUT = 8, 32


def torch_restatement(u8, size, crop):
    x = u8.float().permute(0, 3, 1, 2) / 255
    if crop:
        H, W = x.shape[-2:]
        s = min(H, W)
        top, left = int(round((H - s) / 2.0)), int(round((W - s) / 2.0))
        x = x[..., top:top + s, left:left + s]
    return x if tuple(x.shape[-2:]) == (size, size) else F.interpolate(x, size=(size, size), mode="bilinear", antialias=True, align_corners=False)


def segment(u8, T):
    """frames [0, T) of a clip, the last one repeated when it is shorter (EvalDataset.get_segment)"""
    return torch.cat([u8[:T], u8[-1:].expand(max(T - len(u8), 0), -1, -1, -1)], 0)


@pytest.fixture(scope="module")
def staged():
    """the four clips at 16-byte-aligned offsets of one staging tensor (the first at 16); 16 bytes in front, the gaps and 5 guard
    bytes behind the last clip hold 255"""
    g = torch.Generator().manual_seed(7)
    clips = [torch.randint(0, 256, (n, H, W, 3), generator=g, dtype=torch.uint8) for n, H, W in CLIPS]
    table, end = [], 16
    for c in clips:
        off = -(-end // 16) * 16
        table.append((off, c.shape[0], c.shape[1], c.shape[2]))
        end = off + c.numel()
    staging = torch.full((end + 5,), 255, dtype=torch.uint8)
    for c, (off, *_) in zip(clips, table):
        staging[off:off + c.numel()] = c.reshape(-1)
    assert any(off % 64 for off, *_ in table) and all(off % 16 == 0 for off, *_ in table)
    return clips, table, staging.to(DEV)


@pytest.mark.parametrize("crop", [0, 1])
def test_ingest_clips_equals_ingest_frames_clip_by_clip(staged, crop):
    from ivideogpt_amd.data import ingest_clips, ingest_frames
    clips, table, staging = staged
    out = ingest_clips(staging, table, T_OUT, R_OUT, center_crop=bool(crop))
    out16 = ingest_clips(staging, table, T_OUT, R_OUT, center_crop=bool(crop), dtype=torch.bfloat16)
    assert out.shape == out16.shape == (4, T_OUT, 3, R_OUT, R_OUT) and out.dtype == torch.float32 and out16.dtype == torch.bfloat16
    for b, c in enumerate(clips):
        seg = segment(c, T_OUT)
        one = ingest_frames(seg.to(DEV), R_OUT, center_crop=bool(crop))
        one16 = ingest_frames(seg.to(DEV), R_OUT, center_crop=bool(crop), dtype=torch.bfloat16)
        assert torch.equal(out[b], one), f"clip {b} fp32: {(out[b] != one).sum().item()} values differ from ingest_frames"
        assert torch.equal(out16[b], one16), f"clip {b} bf16: {(out16[b] != one16).sum().item()} values differ from ingest_frames"
        ref = torch_restatement(seg, R_OUT, crop)
        e32, e16 = (out[b].cpu() - ref).abs().max().item(), (out16[b].float().cpu() - ref).abs().max().item()
        print(f"crop {crop} clip {b} {tuple(c.shape)}: fp32 err {e32:.3e}, bf16 err {e16:.3e}")
        assert e32 < 2e-6 and e16 < 4e-3


def test_ingest_clips_refusals_leave_the_output_untouched(staged):
    from ivideogpt_amd import _lib
    lib = _lib.load()
    clips, table, staging = staged
    out = torch.full((4, T_OUT, 3, R_OUT, R_OUT), -7.0, device=DEV)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(tab, B=None, T=T_OUT, nbytes=None, R=R_OUT):
        arr = (_lib.IvgClipDesc * len(tab))(*[_lib.IvgClipDesc(*t) for t in tab])
        return lib.ivg_ingest_clips(C.c_void_p(staging.data_ptr()), staging.numel() if nbytes is None else nbytes, arr, len(tab) if B is None else B, T, 0,
                                    C.c_void_p(out.data_ptr()), _lib.IVG_F32, R, st)

    def with_clip(b, **kv):
        off, n, H, W = table[b]
        d = dict(offset=off, frames=n, H=H, W=W)
        d.update(kv)
        return table[:b] + [(d["offset"], d["frames"], d["H"], d["W"])] + table[b + 1:]

    last = len(table) - 1
    end = table[last][0] + clips[last].numel()
    refused = {
        "B = 0": call(table, B=0), "B < 0": call(table, B=-1), "T = 0": call(table, T=0), "T < 0": call(table, T=-3),
        "frames = 0": call(with_clip(1, frames=0)), "H = 0": call(with_clip(2, H=0)), "W = 0": call(with_clip(0, W=0)),
        "offset not a multiple of 16": call(with_clip(3, offset=table[3][0] + 8)), "offset < 0": call(with_clip(0, offset=-16)),
        "clip past the end of the staging buffer": call(table, nbytes=end - 1),
        "one frame too many for the buffer": call(with_clip(last, frames=table[last][1] + 1)),
        "downscale beyond the kernel's taps": call(table, R=1),        # 64 / 1: what ivg_ingest_frames refuses too
    }
    assert lib.ivg_ingest_frames(C.c_void_p(staging.data_ptr()), 1, 48, 64, 0, C.c_void_p(out.data_ptr()), _lib.IVG_F32, 1, st) == -1
    torch.cuda.synchronize()
    assert {k: v for k, v in refused.items() if v != -1} == {}, "IVG_ERR_INVALID expected"
    assert bool((out == -7.0).all()), "a refused call wrote to the output"
    assert call(table, nbytes=end) == 0                               # the same batch with exactly enough bytes is accepted
    torch.cuda.synchronize()
    assert bool((out != -7.0).all())


def write_episodes(root, shapes, key, action_dim=4, seed=3, int64_at=()):
    rng = np.random.default_rng(seed)
    os.makedirs(root, exist_ok=True)
    for i, (n, H, W) in enumerate(shapes):
        rgb = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
        np.savez_compressed(os.path.join(root, f"ep_{i:03d}.npz"), **{key: rgb.astype(np.int64) if i in int64_at else rgb},
                            action=rng.normal(size=(n, action_dim)).astype(np.float32))


def test_device_loader_matches_the_host_path(tmp_path):
    """two batches, the second short; episode 1 is shorter than T (padded on the device), episode 0 stores int64 frames, episode 2 has
    another frame size; then a seeded vp2 run, whose random starts must be the host path's"""
    from ivideogpt_amd.data import EvalDataLoader
    write_episodes(tmp_path / "bair", [(9, 40, 52), (4, 40, 52), (7, 37, 45)], "aux1_image", int64_at=(0,))
    kw = dict(batch_size=2, load_action=True, root=str(tmp_path / "bair"))
    host = list(EvalDataLoader("bair_robot_pushing", 6, 32, **kw))
    runs = {}
    for workers in (1, 4):
        dl = EvalDataLoader("bair_robot_pushing", 6, 32, num_workers=workers, device=DEV, **kw)
        assert len(dl) == 2
        runs[workers] = [list(dl), list(dl)]                   # iterated twice
    torch.cuda.synchronize()
    first = runs[1][0]
    assert [b[0].shape for b in first] == [(2, 6, 3, 32, 32), (1, 6, 3, 32, 32)]
    for (frames, actions), (hf, ha) in zip(first, host):
        assert frames.is_cuda and actions.is_cuda and frames.dtype == torch.float32
        err = (frames.cpu() - hf).abs().max().item()
        print(f"device loader vs host path: {err:.3e}")
        assert err < 2e-6 and torch.equal(actions.cpu(), ha)
    for other in (runs[1][1], runs[4][0], runs[4][1]):
        for (f0, a0), (f1, a1) in zip(first, other):
            assert torch.equal(f0, f1) and torch.equal(a0, a1), "the loader's output depends on the iteration or on the number of readers"
    write_episodes(tmp_path / "vp2" / "validation", [(12, 24, 24)] * 4, "image", seed=4)
    np.random.seed(21)
    assert len({int(np.random.randint(12 - 5 + 1)) for _ in range(4)}) > 1, "the seed should exercise different starts"
    np.random.seed(21)
    host = list(EvalDataLoader("vp2_robosuite", 5, 16, batch_size=3, root=str(tmp_path / "vp2")))
    np.random.seed(21)
    dev = list(EvalDataLoader("vp2_robosuite", 5, 16, batch_size=3, num_workers=4, device=DEV, root=str(tmp_path / "vp2")))
    assert len(dev) == len(host) == 2
    assert all((d.cpu() - h).abs().max().item() < 2e-6 for d, h in zip(dev, host))


def test_evaluate_over_the_loader_equals_evaluate_over_its_batches(tmp_path):
    import train_gpt
    from test_gpu_evaluate import LLM_CFG, TOK_CFG
    from ivideogpt_amd import CompressiveVQModel, LlamaForCausalLM, weights as W
    from ivideogpt_amd.data import EvalDataLoader
    from ivideogpt_amd.metrics import Evaluator
    from ivideogpt_amd.parallel import LocalAccelerator
    write_episodes(tmp_path, [(7, 48, 64), (3, 48, 64), (5, 64, 64)], "aux1_image", seed=5)
    tcfg = W.tokenizer_config(**TOK_CFG)
    tok = CompressiveVQModel(tcfg, W.random_tokenizer_state_dict(tcfg, 81, codebook_std=0.4), encode_dtype="fp32", decode_dtype="fp32").to(DEV)
    llm = LlamaForCausalLM(dict(LLM_CFG), W.random_llama_state_dict(LLM_CFG, 82), dtype="fp32").to(DEV)
    args = train_gpt.eval_args(context_length=2, segment_length=5, eval_generate_times=2, max_generate_batchsize=2, log_gif_interval=1000)
    loader = EvalDataLoader("bair_robot_pushing", 5, 64, batch_size=2, num_workers=2, device=DEV, root=str(tmp_path))
    batches = [b.clone() for b in loader]
    torch.manual_seed(1234)
    from_list = train_gpt.evaluate(args, LocalAccelerator(DEV), tok, llm, batches, Evaluator(), 0)
    torch.manual_seed(1234)
    from_loader = train_gpt.evaluate(args, LocalAccelerator(DEV), tok, llm, loader, Evaluator(), 0)
    print("list", from_list, "\nloader", from_loader)
    assert from_list.keys() == from_loader.keys() and math.isfinite(from_list["eval/eval_loss"]) and 0 < from_list["eval/ssim"] <= 1
    for k, v in from_list.items():
        assert from_loader[k] == v or (math.isnan(v) and math.isnan(from_loader[k])), k


def test_eval_cli_on_a_directory_of_episodes(tmp_path, capsys, monkeypatch):
    """``train_gpt.main`` with the dataset flags (seeded random weights, full width): 3 episodes in batches of 2 at world 1"""
    import train_gpt
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "IVG_FORCE_COLLECTIVE"):
        monkeypatch.delenv(k, raising=False)
    write_episodes(tmp_path, [(6, 64, 64), (2, 48, 64), (4, 64, 64)], "aux1_image", seed=6)
    import random
    py_state, np_state = random.getstate(), np.random.get_state()           # --seed seeds the process-wide generators: put them back
    with torch.random.fork_rng(devices=[0]):
        logs = train_gpt.main(["--use_eval_dataset", "--dataset_name", "bair_robot_pushing", "--dataset_root", str(tmp_path), "--segment_length", "4",
                               "--per_device_eval_batch_size", "2", "--dataloader_num_workers", "2", "--eval_generate_times", "1",
                               "--use_frame_metrics", "--seed", "0"])
    random.setstate(py_state)
    np.random.set_state(np_state)
    line = json.loads([l for l in capsys.readouterr().out.splitlines() if l.startswith("{")][-1])
    assert line["eval/samples"] == 3 and line["eval/batches"] == 2
    assert math.isfinite(line["eval/eval_loss"]) and 0 < line["eval/ssim"] <= 1 and line["eval/psnr"] > 0
    assert logs["eval/eval_loss"] == line["eval/eval_loss"]
