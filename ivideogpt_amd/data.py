"""Clip ingest for the prediction path (host-side plumbing): the reference's per-episode ``.npz`` format and the
preprocessing of inference/utils.py:12-39.

  * episode file: one uint8 / int ``[T, H, W, 3]`` array under the dataset's display key (``image`` unless the table below
    names another) and a float ``[T, A]`` array ``action`` (datasets/oxe_data_converter.py:57-59, inference/samples/*.npz);
  * ``NPZParser.parse`` -> float ``[segment_length, 3, res, res]`` in [0, 1]: a strided window of the episode, /255, then
    torchvision's tensor ``resize`` WITHOUT centre crop (the aspect ratio is squashed, inference/utils.py:12-16) -- for tensors
    that is ``interpolate(mode='bilinear', antialias=True, align_corners=False)``, restated here (torchvision is not a
    dependency).  The window start is drawn from ``np.random.randint`` with the reference's bound (utils.py:23), so a seeded
    run picks the same frames;
  * ``EvalDataset`` / ``EvalDataLoader`` (ivideogpt/data/simple_dataloader.py:467-552): a directory of such files as a test set, in
    the batches ``accelerator.prepare`` hands the reference's eval loop (``shard_batches``); on the device a batch is staged as
    stored and preprocessed by one ``ivg_ingest_clips`` launch.
"""
import numpy as np
import torch
import torch.nn.functional as F

# dataset -> (frame stride at the dataset's native rate, key of the RGB stream in the episode file); everything is resampled
# relative to fractal20220817_data (3 Hz-equivalent stride), as the reference's table does
DATASETS = {
    "fractal20220817_data": (3, "image"), "kuka": (10, "image"), "bridge": (5, "image"), "taco_play": (15, "rgb_static"),
    "jaco_play": (10, "image"), "berkeley_cable_routing": (10, "image"), "roboturk": (10, "front_rgb"),
    "viola": (20, "agentview_rgb"), "toto": (30, "image"), "language_table": (10, "rgb"),
    "columbia_cairlab_pusht_real": (10, "image"),
    "stanford_kuka_multimodal_dataset_converted_externally_to_rlds": (20, "image"),
    "stanford_hydra_dataset_converted_externally_to_rlds": (10, "image"),
    "austin_buds_dataset_converted_externally_to_rlds": (20, "image"),
    "nyu_franka_play_dataset_converted_externally_to_rlds": (3, "image"),
    "maniskill_dataset_converted_externally_to_rlds": (20, "image"),
    "furniture_bench_dataset_converted_externally_to_rlds": (10, "image"),
    "ucsd_kitchen_dataset_converted_externally_to_rlds": (2, "image"),
    "ucsd_pick_and_place_dataset_converted_externally_to_rlds": (3, "image"),
    "austin_sailor_dataset_converted_externally_to_rlds": (20, "image"), "bc_z": (10, "image"),
    "utokyo_pr2_opening_fridge_converted_externally_to_rlds": (10, "image"),
    "utokyo_pr2_tabletop_manipulation_converted_externally_to_rlds": (10, "image"),
    "utokyo_xarm_pick_and_place_converted_externally_to_rlds": (10, "image"),
    "utokyo_xarm_bimanual_converted_externally_to_rlds": (10, "image"), "robo_net": (1, "image"),
    "kaist_nonprehensile_converted_externally_to_rlds": (10, "image"),
    "stanford_mask_vit_converted_externally_to_rlds": (1, "image"),
    "dlr_sara_pour_converted_externally_to_rlds": (10, "image"),
    "dlr_sara_grid_clamp_converted_externally_to_rlds": (10, "image"),
    "dlr_edan_shared_control_converted_externally_to_rlds": (5, "image"),
    "asu_table_top_converted_externally_to_rlds": (12.5, "image"),
    "iamlab_cmu_pickup_insert_converted_externally_to_rlds": (20, "image"), "uiuc_d3field1": (1, "image_1"),
    "uiuc_d3field2": (1, "image_2"), "uiuc_d3field3": (1, "image_3"), "uiuc_d3field4": (1, "image_4"),
    "utaustin_mutex": (20, "image"), "berkeley_fanuc_manipulation": (10, "image"), "cmu_playing_with_food": (10, "image"),
    "cmu_play_fusion": (5, "image"), "cmu_stretch": (10, "image"), "bair_robot_pushing": (1, "aux1_image"),
    "tfds_robonet": (1, "image"), "stanford_robocook_converted_externally_to_rlds1": (1, "image_1"),
    "stanford_robocook_converted_externally_to_rlds2": (1, "image_2"),
    "stanford_robocook_converted_externally_to_rlds3": (1, "image_3"),
    "stanford_robocook_converted_externally_to_rlds4": (1, "image_4"),
}
REFERENCE_STRIDE = DATASETS["fractal20220817_data"][0]
# names only the reference's dataloader tables know (simple_dataloader.py:18-98: get_base_stepsize / get_display_key), same columns.
# Kept beside DATASETS, which stays the parser's table entry for entry (inference/utils.py): oracle/pin checks that one against the
# reference key by key and refuses names the parser does not have.
DATALOADER_DATASETS = {
    "vp2_robodesk": (1, "image"), "vp2_robosuite": (1, "image"), "berkeley_autolab_ur5": (1, "hand_image"),
    "berkeley_mvp_converted_externally_to_rlds": (1, "hand_image"), "berkeley_rpt_converted_externally_to_rlds": (1, "hand_image"),
}


def known_dataset(dataset_name):
    return dataset_name in DATASETS or dataset_name in DATALOADER_DATASETS


def get_display_key(dataset_name):
    """simple_dataloader.py:73-98: the key of the RGB stream in an episode file, ``image`` for names no table has."""
    return DATASETS.get(dataset_name, DATALOADER_DATASETS.get(dataset_name, (1, "image")))[1]


def resize_frames(images, size):
    """images float [T, 3, H, W] -> [T, 3, size, size], antialiased bilinear (== torchvision F.resize on tensors)."""
    if tuple(images.shape[-2:]) == (size, size):
        return images
    return F.interpolate(images, size=(size, size), mode="bilinear", antialias=True, align_corners=False)


def ingest_frames(frames_u8, size, center_crop=False, dtype=torch.float32):
    """uint8 frames [T, H, W, 3] ON THE GPU -> [T, 3, size, size] in [0, 1] (``dtype`` float32 / bfloat16): / 255, optional
    centre crop to the short side, antialiased bilinear resize -- one HIP kernel (libivg ``ivg_ingest_frames``) reading the
    interleaved rows as they are stored; the device-side form of ``resize_frames(frames / 255, size)``."""
    import ctypes as C
    from . import _lib
    from .packing import dtype_code
    if not frames_u8.is_cuda or frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4 or frames_u8.shape[-1] != 3:
        raise AssertionError("ingest_frames: uint8 [T, H, W, 3] tensor on the GPU expected")
    src = frames_u8.contiguous()
    T, H, W, _ = src.shape
    out = torch.empty(T, 3, size, size, dtype=dtype, device=src.device)
    st = C.c_void_p(torch.cuda.current_stream(src.device).cuda_stream)
    _lib.check(_lib.load().ivg_ingest_frames(C.c_void_p(src.data_ptr()), T, H, W, int(bool(center_crop)), C.c_void_p(out.data_ptr()),
                                             dtype_code(dtype), int(size), st), None, "ingest_frames")
    return out


def ingest_clips(staging_u8, clips, segment_length, size, center_crop=False, dtype=torch.float32):
    """The batched form of ``ingest_frames`` (libivg ``ivg_ingest_clips``): ``staging_u8`` is a flat uint8 tensor ON THE GPU that holds
    B clips, ``clips`` a sequence of ``(offset, frames, H, W)`` -- clip b is ``frames`` stored ``[H, W, 3]`` frames from byte ``offset``
    (a multiple of 16) on.  -> ``[B, segment_length, 3, size, size]``; output frame t of clip b is, bit for bit, what ``ingest_frames``
    gives for stored frame ``min(t, frames - 1)``: longer clips are truncated, shorter ones repeat their last frame.  One launch on
    the current stream, nothing synchronises the host; a bad clip raises before anything is launched."""
    import ctypes as C
    from . import _lib
    from .packing import dtype_code
    if not staging_u8.is_cuda or staging_u8.dtype != torch.uint8 or staging_u8.dim() != 1 or not staging_u8.is_contiguous():
        raise AssertionError("ingest_clips: flat uint8 tensor on the GPU expected")
    table = (_lib.IvgClipDesc * max(len(clips), 1))(*[_lib.IvgClipDesc(int(o), int(f), int(h), int(w)) for o, f, h, w in clips])
    out = torch.empty(len(clips), max(segment_length, 0), 3, size, size, dtype=dtype, device=staging_u8.device)
    st = C.c_void_p(torch.cuda.current_stream(staging_u8.device).cuda_stream)
    _lib.check(_lib.load().ivg_ingest_clips(C.c_void_p(staging_u8.data_ptr()), staging_u8.numel(), table, len(clips), int(segment_length),
                                            int(bool(center_crop)), C.c_void_p(out.data_ptr()), dtype_code(dtype), int(size), st), None, "ingest_clips")
    return out


def frame_stride(dataset_name):
    native = DATASETS.get(dataset_name, (1, "image"))[0]
    return max(1, round(native / REFERENCE_STRIDE))


def pick_window(n_frames, length, stride):
    """-> slice of `length` frames every `stride`; the stride shrinks when the episode is too short, the start is random."""
    if stride * length > n_frames:
        stride = max(1, n_frames // length)
    span = stride * length
    first = np.random.randint(max(n_frames - span + 1, 1))
    return slice(first, first + span, stride)


class NPZParser:
    """Same constructor / ``parse`` contract as the reference's parser (inference/utils.py:18-39)."""

    def __init__(self, segment_length, image_size=64, device=None):
        """device=None: host preprocessing with the reference's exact arithmetic (what predict.py does before ``.to(device)``);
        device='cuda': the window's uint8 frames are uploaded as stored and preprocessed by the HIP ingest kernel."""
        self.segment_length, self.image_size, self.device = segment_length, image_size, device

    def parse(self, npz_file, dataset_name, load_action=False):
        episode = np.load(npz_file)
        rgb = episode[DATASETS.get(dataset_name, (1, "image"))[1]]
        window = pick_window(len(rgb), self.segment_length, frame_stride(dataset_name))
        if self.device is not None:
            frames = ingest_frames(torch.from_numpy(np.ascontiguousarray(rgb[window])).to(self.device), self.image_size)
            actions = torch.from_numpy(np.asarray(episode["action"][window])).float().to(self.device) if load_action else None
            return frames, actions      # both on self.device
        frames = torch.from_numpy(np.ascontiguousarray(rgb[window])).float().permute(0, 3, 1, 2)   # T,H,W,C -> T,C,H,W
        frames = resize_frames(frames / 255, self.image_size)
        actions = torch.from_numpy(np.asarray(episode["action"][window])).float() if load_action else None
        return frames, actions


# ------------------------------------------------------------------------------------------------ evaluation on a test set of episodes
# dataset -> (key of its directory in DATASET.yaml, glob pattern under that directory): simple_dataloader.py:480-499
EVAL_SETS = {
    "bair_robot_pushing": ("bair_test_dataset", ("*.npz",)), "tfds_robonet": ("robonet_test_dataset", ("*.npz",)),
    "vp2_robodesk": ("robodesk_dataset", ("*", "validation*", "*.npz")), "vp2_robosuite": ("robosuite_dataset", ("validation", "*.npz")),
}
STAGING_ALIGN = 16        # a clip starts at a multiple of this in the staging buffer (ivg_ingest_clips)
MAX_LOADER_THREADS = 16


def shard_batches(n_items, batch_size, rank, world):
    """The index batches rank ``rank`` of ``world`` sees -- what ``accelerator.prepare`` makes of the reference's eval loader
    (``DataLoader(batch_size, shuffle=False, drop_last=False)``): accelerate's ``BatchSamplerShard(split_batches=False,
    even_batches=True)``.  The items in order, followed by the items of the first ``world`` batches over again (repeated until they
    fill ``world`` batches), are cut into batches of ``batch_size``; the batch count is rounded up to a multiple of ``world`` and rank
    r takes batches r, r + world, ...  So every rank gets the same number of full batches, and the tail wraps around to the first
    samples: 7 items, batch 2, world 3 -> [[0, 1], [6, 0]], [[2, 3], [1, 2]], [[4, 5], [3, 4]].  The wrapped duplicates enter the
    eval means, as they do in the reference, whose loop calls ``accelerator.gather`` and not ``gather_for_metrics``
    (train_gpt.py:376, 476-479).  (accelerate applies the same rule when asked for one process, 7 items -> [.., [6, 0]], but
    ``prepare`` leaves a one-process loader alone: ``EvalDataLoader`` keeps the short last batch at world 1.)"""
    if n_items <= 0:
        return []
    n_batches = -(-n_items // batch_size)
    wrap = list(range(min(n_items, world * batch_size)))
    while len(wrap) < world * batch_size:
        wrap += wrap
    total = -(-n_batches // world) * world
    seq = list(range(n_items)) + wrap[:total * batch_size - n_items]
    return [seq[k * batch_size:(k + 1) * batch_size] for k in range(rank, total, world)]


def episode_header(npz_file, key):
    """-> (shape, dtype) of array ``key`` of an episode file, from the member's header alone (nothing is decompressed)."""
    import zipfile
    from numpy.lib import format as npf
    with zipfile.ZipFile(npz_file) as z, z.open(key + ".npy") as f:
        version = npf.read_magic(f)
        read = {(1, 0): npf.read_array_header_1_0, (2, 0): npf.read_array_header_2_0}.get(version)
        if read is not None:
            shape, _, dtype = read(f)
            return shape, dtype
    a = np.load(npz_file)[key]
    return a.shape, a.dtype


class EvalDataset:
    """The reference's ``EvalDataset`` (ivideogpt/data/simple_dataloader.py:467-546): one test episode per ``.npz`` file, sorted by
    name; item i is the segment ``[start, start + segment_length)`` of episode i (``start`` 0, random for the ``vp2`` sets), a short
    episode repeating its last frame and action, preprocessed as ``/ 255 -> centre crop (tfds_robonet only) -> resize``.
    ``root=DIR`` names the directory directly instead of looking it up in ``dataset_yaml``."""

    def __init__(self, dataset_name, segment_length, image_size=256, load_action=False, root=None, dataset_yaml="DATASET.yaml"):
        import glob
        import os
        self.image_size, self.dataset_name, self.segment_length, self.load_action = image_size, dataset_name, segment_length, load_action
        if root is not None:
            if not known_dataset(dataset_name):
                raise NotImplementedError(dataset_name)
            pattern = EVAL_SETS.get(dataset_name, (None, ("*.npz",)))[1]
        elif dataset_name in EVAL_SETS:
            import yaml
            key, pattern = EVAL_SETS[dataset_name]
            with open(dataset_yaml) as f:
                root = yaml.load(f, Loader=yaml.FullLoader)[key]
        else:
            raise NotImplementedError(dataset_name)
        self.filenames = sorted(glob.glob(os.path.join(root, *pattern)))
        self.size = len(self.filenames)
        self.display_key = get_display_key(dataset_name)
        self.center_crop = dataset_name == "tfds_robonet"
        self.random_start = "vp2" in dataset_name
        if self.size == 0:
            raise ValueError(f"[EvalDataset] No test episodes found in {dataset_name}")
        print(f"[EvalDataset] Find {self.size} test episodes in {dataset_name}")

    def __len__(self):
        return self.size

    def draw_start(self, n_frames):
        """First frame of the segment of an episode of ``n_frames`` (:513-516); the vp2 draw advances ``np.random``."""
        return int(np.random.randint(max(n_frames - self.segment_length + 1, 1))) if self.random_start else 0

    def load_actions(self, episode):
        """The ``action`` rows the segment is cut from; tfds_robonet stores one row less than frames: a zero row is appended (:532-534)."""
        action = np.asarray(episode["action"])
        if self.dataset_name == "tfds_robonet":
            action = np.append(action, np.zeros((1, 5), dtype=np.int64), axis=0)
        return action

    def cut(self, rows, start):
        """rows [start, start + segment_length) of an array, the last one repeated when the array ends early (:517-526)."""
        T = self.segment_length
        part = np.asarray(rows[start:start + T])
        if len(part) < T:
            part = np.concatenate([part, np.repeat(part[-1:], T - len(part), axis=0)], axis=0)
        return part

    def get_segment(self, episode, action=None, start=None):
        if start is None:
            start = self.draw_start(len(episode))
        return self.cut(episode, start), (self.cut(action, start) if action is not None else None)

    def data_augmentation(self, images):
        """float [T, 3, H, W] in [0, 255] -> [T, 3, size, size] in [0, 1] (:506-510; torchvision's center_crop offsets)."""
        images = images / 255
        if self.center_crop:
            H, W = images.shape[-2:]
            s = min(H, W)
            top, left = int(round((H - s) / 2.0)), int(round((W - s) / 2.0))
            images = images[..., top:top + s, left:left + s]
        return resize_frames(images, self.image_size)

    def __getitem__(self, item):
        """The host path, with the reference's arithmetic: float32 [T, 3, size, size] (and [T, A] float32 with ``load_action``)."""
        episode = np.load(self.filenames[item])
        images, actions = self.get_segment(episode[self.display_key], self.load_actions(episode) if self.load_action else None)
        images = torch.from_numpy(np.ascontiguousarray(images, dtype=np.uint8)).float().permute(0, 3, 1, 2)   # T,H,W,C -> T,C,H,W
        images = self.data_augmentation(images)
        if self.load_action:
            return images, torch.from_numpy(np.ascontiguousarray(actions)).float()
        return images


class _StagingSlot:
    """One batch's episodes as stored (uint8, interleaved RGB), clip after clip at STAGING_ALIGN-byte boundaries: a pinned host buffer
    the reader threads fill, its device mirror, and the event of the copy that last read the host side."""

    def __init__(self, device, stream):
        self.device, self.stream, self.host, self.dev, self.copied = device, stream, None, None, torch.cuda.Event()

    def reserve(self, nbytes):
        """-> the host side as a numpy array of at least ``nbytes``; call only after ``copied`` has completed."""
        if self.host is None or self.host.numel() < nbytes:
            cap = nbytes + nbytes // 4
            self.host = torch.empty(cap, dtype=torch.uint8, pin_memory=True)
            with torch.cuda.stream(self.stream):     # the device side belongs to the stream that copies into and reads it
                self.dev = torch.empty(cap, dtype=torch.uint8, device=self.device)
        return self.host.numpy()


class EvalDataLoader:
    """The reference's ``EvalDataLoader`` (simple_dataloader.py:549-552) as ``accelerator.prepare`` hands it to the eval loop: an
    iterable with ``len()`` over batches in file order, ``pixel_values [B, T, 3, R, R]`` float32 in [0, 1] or ``(pixel_values,
    actions [B, T, A])``.  At world 1 the last batch is short (``drop_last=False``); with more ranks see ``shard_batches``.

    ``device=None``: ``EvalDataset.__getitem__`` results stacked on the host (the reference's arithmetic).
    ``device='cuda'``: ``min(num_workers, 16)`` threads read and decompress the episodes and copy ONLY the frames a segment needs, as
    stored, into a slot of a pinned staging buffer (a short episode is not padded on the host); a batch then takes one asynchronous
    host-to-device copy on a side stream, one ``ivg_ingest_clips`` launch (/ 255, crop, resize, repetition of the last frame) and
    one small copy for the actions.  Two batches are in flight (two slots); a slot is refilled only after the copy that read it has
    completed (an event per slot), and the consumer's stream waits on the batch's event, never the host.  The random ``vp2`` starts
    are drawn in the iterating thread in file order (the episode length comes from the file's header), so a seeded run does not
    depend on the timing of the readers."""

    def __init__(self, dataset_name, segment_length, image_size, batch_size=2, num_workers=1, load_action=False, device=None, rank=0,
                 world=1, root=None, dataset_yaml="DATASET.yaml", **dummy_args):
        self.dataset = EvalDataset(dataset_name, segment_length, image_size, load_action, root=root, dataset_yaml=dataset_yaml)
        self.batch_size, self.num_workers = batch_size, max(1, min(int(num_workers), MAX_LOADER_THREADS))
        self.device = torch.device(device) if device is not None else None
        n = len(self.dataset)
        self.batches = [list(range(lo, min(lo + batch_size, n))) for lo in range(0, n, batch_size)] if world == 1 \
            else shard_batches(n, batch_size, rank, world)
        self.wait_s = 0.0       # host time the last iteration spent waiting for readers (tools/eval_dataset_bench.py)

    def __len__(self):
        return len(self.batches)

    def __iter__(self):
        return self._host_batches() if self.device is None else self._device_batches()

    def _host_batches(self):
        for idxs in self.batches:
            items = [self.dataset[i] for i in idxs]
            if self.dataset.load_action:
                yield torch.stack([f for f, _ in items]), torch.stack([a for _, a in items])
            else:
                yield torch.stack(items)

    def _read_into(self, dst, item, start, shape):
        """Reader thread: frames [start, start + shape[0]) of episode ``item`` -> ``dst`` (a view of the pinned slot), narrowed to
        uint8 on the way; -> the segment's actions (host, padded) or None."""
        ds = self.dataset
        episode = np.load(ds.filenames[item])
        rgb = episode[ds.display_key]
        assert rgb.shape[1:] == shape[1:] and start + shape[0] <= len(rgb), f"{ds.filenames[item]}: header and array disagree"
        np.copyto(dst.reshape(shape), rgb[start:start + shape[0]], casting="unsafe")
        return ds.cut(ds.load_actions(episode), start).astype(np.float32) if ds.load_action else None

    def _submit(self, pool, slot, idxs):
        """Iterating thread: lay batch ``idxs`` out in ``slot`` and hand its episodes to the readers."""
        ds, T = self.dataset, self.dataset.segment_length
        plan, total = [], 0
        for i in idxs:
            shape, dtype = episode_header(ds.filenames[i], ds.display_key)
            if len(shape) != 4 or shape[-1] != 3 or dtype.kind not in "ui":
                raise ValueError(f"{ds.filenames[i]}: [T, H, W, 3] integer frames expected under {ds.display_key!r}, found {shape} {dtype}")
            start = ds.draw_start(shape[0])
            kept = (min(T, shape[0] - start),) + tuple(shape[1:])
            plan.append((i, start, kept, total))
            total = -(-(total + int(np.prod(kept))) // STAGING_ALIGN) * STAGING_ALIGN
        slot.copied.synchronize()           # the copy that last read this slot's host side
        host = slot.reserve(total)
        reads = [pool.submit(self._read_into, host[off:off + int(np.prod(kept))], i, start, kept) for i, start, kept, off in plan]
        return slot, total, [(off, kept[0], kept[1], kept[2]) for _, _, kept, off in plan], reads

    def _launch(self, side, job):
        import time
        slot, total, clips, reads = job
        t0 = time.perf_counter()
        actions = [r.result() for r in reads]
        self.wait_s += time.perf_counter() - t0
        ds = self.dataset
        with torch.cuda.stream(side):
            slot.dev[:total].copy_(slot.host[:total], non_blocking=True)
            slot.copied.record(side)
            frames = ingest_clips(slot.dev[:total], clips, ds.segment_length, ds.image_size, center_crop=ds.center_crop)
            acts = torch.from_numpy(np.stack(actions)).pin_memory().to(self.device, non_blocking=True) if ds.load_action else None
            ready = torch.cuda.Event()
            ready.record(side)
        return frames, acts, ready

    def _device_batches(self):
        from collections import deque
        from concurrent.futures import ThreadPoolExecutor
        self.wait_s = 0.0
        side = torch.cuda.Stream(device=self.device)
        slots = [_StagingSlot(self.device, side) for _ in range(2)]
        pool = ThreadPoolExecutor(max_workers=self.num_workers)
        jobs = deque()
        try:
            for k, idxs in enumerate(self.batches[:2]):
                jobs.append(self._submit(pool, slots[k], idxs))
            for k in range(len(self.batches)):
                frames, acts, ready = self._launch(side, jobs.popleft())
                if k + 2 < len(self.batches):
                    jobs.append(self._submit(pool, slots[k % 2], self.batches[k + 2]))
                consumer = torch.cuda.current_stream(self.device)
                consumer.wait_event(ready)
                for t in (frames, acts):
                    if t is not None:
                        t.record_stream(consumer)
                yield (frames, acts) if self.dataset.load_action else frames
        finally:
            pool.shutdown(wait=True, cancel_futures=True)
            side.synchronize()      # the slots' buffers go away with this generator
