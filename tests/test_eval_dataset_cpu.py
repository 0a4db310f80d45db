"""``ivideogpt_amd.data.EvalDataset`` / ``EvalDataLoader`` / ``shard_batches`` on the host: the reference's test-set loader
(ivideogpt/data/simple_dataloader.py:467-552) and what ``accelerator.prepare`` does to it, against independent restatements."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def write_episodes(root, shapes, key="image", action_dim=4, dtype=np.uint8, seed=0, action_rows=None):
    """shapes: [(frames, H, W)] -> files ep_000.npz ... (written in reverse, so sorting is the dataset's doing); -> the arrays"""
    rng = np.random.default_rng(seed)
    eps = []
    for i, (n, H, W) in enumerate(shapes):
        rgb = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8).astype(dtype)
        act = rng.normal(size=(n if action_rows is None else action_rows(n), action_dim)).astype(np.float32)
        eps.append((rgb, act))
    os.makedirs(root, exist_ok=True)
    for i in reversed(range(len(eps))):
        np.savez(os.path.join(root, f"ep_{i:03d}.npz"), **{key: eps[i][0], "action": eps[i][1]})
    return eps


def restate(rgb, size, crop):
    """/ 255 -> torchvision centre crop -> antialiased bilinear resize, written out independently of the package"""
    x = torch.from_numpy(rgb.astype(np.float32)).permute(0, 3, 1, 2) / 255
    if crop:
        H, W = x.shape[-2:]
        s = min(H, W)
        top, left = int(round((H - s) / 2.0)), int(round((W - s) / 2.0))
        x = x[..., top:top + s, left:left + s]
    return x if tuple(x.shape[-2:]) == (size, size) else F.interpolate(x, size=(size, size), mode="bilinear", antialias=True, align_corners=False)


def test_short_episode_repeats_last_frame_and_action_and_bair_starts_at_zero(tmp_path):
    from ivideogpt_amd.data import EvalDataset
    eps = write_episodes(tmp_path, [(3, 20, 24), (12, 20, 24)], key="aux1_image")
    ds = EvalDataset("bair_robot_pushing", 8, image_size=16, load_action=True, root=str(tmp_path))
    assert len(ds) == 2 and ds.display_key == "aux1_image"
    np.random.seed(5)
    state = np.random.get_state()[1].copy()
    frames, actions = ds[0]
    assert frames.shape == (8, 3, 16, 16) and frames.dtype == torch.float32 and actions.shape == (8, 4) and actions.dtype == torch.float32
    ref = restate(eps[0][0], 16, False)
    assert torch.equal(frames[:3], ref) and all(torch.equal(frames[t], ref[2]) for t in range(3, 8))
    assert torch.equal(actions[:3], torch.from_numpy(eps[0][1])) and all(torch.equal(actions[t], actions[2]) for t in range(3, 8))
    frames, actions = ds[1]                                   # a longer episode: frames [0, 8)
    assert torch.equal(frames, restate(eps[1][0][:8], 16, False)) and torch.equal(actions, torch.from_numpy(eps[1][1][:8]))
    assert np.array_equal(np.random.get_state()[1], state), "a fixed start draws nothing"


@pytest.mark.parametrize("name,sub", [("vp2_robosuite", ("validation",)), ("vp2_robodesk", ("task_a", "validation_0"))])
def test_vp2_start_is_the_seeded_draw_with_the_reference_bound(tmp_path, name, sub):
    from ivideogpt_amd.data import EvalDataset
    eps = write_episodes(os.path.join(tmp_path, *sub), [(15, 16, 16), (4, 16, 16)])
    write_episodes(os.path.join(tmp_path, "training"), [(5, 16, 16)], seed=9)        # not under the reference's sub-pattern
    ds = EvalDataset(name, 6, image_size=16, load_action=True, root=str(tmp_path))
    assert len(ds) == 2
    np.random.seed(11)
    got = [ds[0], ds[1], ds[0]]
    np.random.seed(11)
    starts = [np.random.randint(max(n - 6 + 1, 1)) for n in (15, 4, 15)]
    assert starts[1] == 0 and starts[0] > 0 and starts[2] != starts[0]     # the seed exercises non-zero starts; a short episode has one
    for (frames, actions), start, (rgb, act) in zip(got, starts, (eps[0], eps[1], eps[0])):
        seg, rows = rgb[start:start + 6], act[start:start + 6]
        seg = np.concatenate([seg, np.repeat(seg[-1:], 6 - len(seg), 0)], 0)
        rows = np.concatenate([rows, np.repeat(rows[-1:], 6 - len(rows), 0)], 0)
        assert torch.equal(frames, restate(seg, 16, False)) and torch.equal(actions, torch.from_numpy(rows))


def test_robonet_zero_action_row_and_centre_crop(tmp_path):
    from ivideogpt_amd.data import EvalDataset
    # one action row less than frames, 5-d; H - s odd on one axis (torchvision rounds half to even: (33 - 21) / 2 = 6, (26 - 21) / 2 = 2.5 -> 2)
    eps = write_episodes(tmp_path, [(6, 33, 21), (6, 21, 26)], action_dim=5, action_rows=lambda n: n - 1)
    ds = EvalDataset("tfds_robonet", 6, image_size=16, load_action=True, root=str(tmp_path))
    for i in range(2):
        frames, actions = ds[i]
        assert actions.shape == (6, 5)
        assert torch.equal(actions[:5], torch.from_numpy(eps[i][1])) and torch.equal(actions[5], torch.zeros(5))
        assert torch.equal(frames, restate(eps[i][0], 16, True))
        assert not torch.equal(frames, restate(eps[i][0], 16, False))
    plain = EvalDataset("bair_robot_pushing", 6, image_size=16, root=str(tmp_path))      # the crop is tfds_robonet's alone
    plain.display_key = "image"
    assert torch.equal(plain[0], restate(eps[0][0], 16, False))


def test_file_order_empty_directory_unknown_name_and_yaml(tmp_path):
    from ivideogpt_amd.data import EvalDataset
    write_episodes(tmp_path / "bair", [(2, 8, 8)] * 3, key="aux1_image")
    ds = EvalDataset("bair_robot_pushing", 2, image_size=8, root=str(tmp_path / "bair"))
    assert [os.path.basename(f) for f in ds.filenames] == ["ep_000.npz", "ep_001.npz", "ep_002.npz"]
    os.makedirs(tmp_path / "empty")
    with pytest.raises(ValueError, match="No test episodes found in tfds_robonet"):
        EvalDataset("tfds_robonet", 2, root=str(tmp_path / "empty"))
    with pytest.raises(NotImplementedError):
        EvalDataset("no_such_dataset", 2, root=str(tmp_path / "bair"))
    with pytest.raises(NotImplementedError):
        EvalDataset("fractal20220817_data", 2)                    # no test-set entry in the yaml for it (reference :497-498)
    assert len(EvalDataset("fractal20220817_data", 2, image_size=8, root=str(tmp_path / "bair"))) == 3   # root= accepts any known name
    yml = tmp_path / "DATASET.yaml"
    yml.write_text(f"bair_test_dataset: {tmp_path / 'bair'}\nrobonet_test_dataset: {tmp_path / 'empty'}\n")
    assert len(EvalDataset("bair_robot_pushing", 2, image_size=8, dataset_yaml=str(yml))) == 3
    with pytest.raises(ValueError):
        EvalDataset("tfds_robonet", 2, dataset_yaml=str(yml))


def test_int64_frames_and_the_real_format_episode(tmp_path):
    from ivideogpt_amd.data import EvalDataset, episode_header
    eps = write_episodes(tmp_path / "b", [(5, 12, 12)], key="aux1_image", dtype=np.int64)
    ds = EvalDataset("bair_robot_pushing", 4, image_size=8, root=str(tmp_path / "b"))
    assert torch.equal(ds[0], restate(eps[0][0][:4], 8, False))
    assert episode_header(ds.filenames[0], "aux1_image") == ((5, 12, 12, 3), np.dtype(np.int64))
    # tests/golden/fractal_sample.npz: an episode as the reference's converter writes it (22 x 256 x 320 x 3 uint8, compressed)
    assert episode_header(os.path.join(GOLDEN, "fractal_sample.npz"), "image") == ((22, 256, 320, 3), np.dtype(np.uint8))
    os.symlink(os.path.join(GOLDEN, "fractal_sample.npz"), tmp_path / "fractal_sample.npz")
    real = EvalDataset("fractal20220817_data", 24, image_size=64, root=str(tmp_path))
    rgb = np.load(os.path.join(GOLDEN, "fractal_sample.npz"))["image"]
    clip = real[0]
    assert torch.equal(clip[:22], restate(rgb, 64, False)) and torch.equal(clip[23], clip[21])


@pytest.mark.parametrize("world", [1, 2, 3])
@pytest.mark.parametrize("bs", [1, 2, 3])
@pytest.mark.parametrize("n", [1, 2, 5, 7, 8])
def test_shard_batches_is_accelerates_batch_sampler_shard(n, bs, world):
    from accelerate.data_loader import BatchSamplerShard
    from torch.utils.data import BatchSampler, SequentialSampler
    from ivideogpt_amd.data import shard_batches
    for rank in range(world):
        ref = list(BatchSamplerShard(BatchSampler(SequentialSampler(range(n)), bs, False), world, rank))   # split_batches=False, even_batches=True
        assert shard_batches(n, bs, rank, world) == ref, (n, bs, world, rank)


def test_shard_batches_documented_example():
    from ivideogpt_amd.data import shard_batches
    assert [shard_batches(7, 2, r, 3) for r in range(3)] == [[[0, 1], [6, 0]], [[2, 3], [1, 2]], [[4, 5], [3, 4]]]


def test_host_loader_batches_and_shards(tmp_path):
    from ivideogpt_amd.data import EvalDataLoader, shard_batches
    eps = write_episodes(tmp_path, [(4, 10, 12)] * 7, key="aux1_image")
    clips = [restate(rgb[:3], 8, False) for rgb, _ in eps]
    acts = [torch.from_numpy(a[:3]) for _, a in eps]
    one = EvalDataLoader("bair_robot_pushing", 3, 8, batch_size=2, num_workers=4, load_action=True, root=str(tmp_path), unused_reference_kwarg=1)
    assert len(one) == 4
    got = list(one)
    assert [b[0].shape[0] for b in got] == [2, 2, 2, 1], "world 1 keeps the short last batch (drop_last=False)"
    for k, (frames, actions) in enumerate(got):
        assert frames.shape[1:] == (3, 3, 8, 8) and actions.shape[1:] == (3, 4)
        assert torch.equal(frames, torch.stack(clips[2 * k:2 * k + 2])) and torch.equal(actions, torch.stack(acts[2 * k:2 * k + 2]))
    for world in (2, 3):
        counts = []
        for rank in range(world):
            dl = EvalDataLoader("bair_robot_pushing", 3, 8, batch_size=2, rank=rank, world=world, root=str(tmp_path))   # frames alone
            want = shard_batches(7, 2, rank, world)
            got = list(dl)
            assert len(dl) == len(got) == len(want)
            for frames, idxs in zip(got, want):
                assert torch.is_tensor(frames) and torch.equal(frames, torch.stack([clips[i] for i in idxs]))
            counts.append(len(got))
        assert len(set(counts)) == 1, "every rank sees the same number of (full) batches"
