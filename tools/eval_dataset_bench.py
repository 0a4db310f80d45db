"""What evaluating from a directory of npz episodes costs (``ivideogpt_amd.data.EvalDataLoader(device='cuda')``), measured on synthetic
episodes of the two real shapes, written to a temporary directory with ``np.savez_compressed`` (smooth images plus a little noise, so
that inflating them is real work):

    robonet-like   22 x 256 x 320 x 3 uint8, no actions read, centre crop + resize to 64   (``tfds_robonet``)
    bair-like      30 x 64 x 64 x 3 uint8 with 4-d actions, nothing resized                (``bair_robot_pushing``)

  1. the loader alone: clips per second over a whole pass (host clock, ending in a device synchronise) with 1, 4 and 16 reader threads;
  2. ``train_gpt.evaluate`` (full-width tokenizer and action-conditioned transformer, seeded random weights, bf16, frame metrics, one
     sample per trajectory) over the bair-like set: time per batch fed by the loader against the SAME batches preloaded on the device
     (the path that existed before the loader: the baseline), alternating the two; and the host time the loop spends blocked in the
     loader's ``next()``.

    python tools/eval_dataset_bench.py [--episodes 64] [--repeats 3] [--out profiles/eval_dataset.txt]"""
import argparse
import os
import sys
import tempfile
import time
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
DEV = "cuda:0"


def write_episodes(root, n, frames, H, W, key, action_dim, seed):
    """smooth random fields (an 8 x 10 grid of colours, bilinearly enlarged, drifting over time) + noise of +-2 levels"""
    rng = np.random.default_rng(seed)
    os.makedirs(root, exist_ok=True)
    for i in range(n):
        coarse = torch.from_numpy(rng.uniform(0, 255, (1, 3, frames // 4 + 2, 8, 10)).astype(np.float32))
        field = torch.nn.functional.interpolate(coarse, size=(frames, H, W), mode="trilinear", align_corners=True)[0]
        rgb = (field.permute(1, 2, 3, 0).numpy() + rng.integers(-2, 3, (frames, H, W, 3))).clip(0, 255).astype(np.uint8)
        arrays = {key: rgb}
        if action_dim:
            arrays["action"] = rng.normal(size=(frames, action_dim)).astype(np.float32)
        np.savez_compressed(os.path.join(root, f"ep_{i:04d}.npz"), **arrays)
    return sum(os.path.getsize(os.path.join(root, f)) for f in os.listdir(root)) / n


def loader_pass(loader):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = 0
    for batch in loader:
        n += (batch[0] if isinstance(batch, tuple) else batch).shape[0]
    torch.cuda.synchronize()
    return n / (time.perf_counter() - t0)


class TimedNext:
    """iterates ``inner``; ``calls`` holds the host time spent inside each of its ``next()`` calls (the last one ends the iteration)"""

    def __init__(self, inner):
        self.inner, self.calls = inner, []

    def __iter__(self):
        it = iter(self.inner)
        while True:
            t0 = time.perf_counter()
            try:
                batch = next(it)
            except StopIteration:
                return
            finally:
                self.calls.append(time.perf_counter() - t0)
            yield batch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--episodes", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import train_gpt
    from ivideogpt_amd import CompressiveVQModel, weights as W
    from ivideogpt_amd.data import EvalDataLoader
    from ivideogpt_amd.metrics import Evaluator
    from ivideogpt_amd.parallel import LocalAccelerator
    lines = []

    def say(line):
        lines.append(line)
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    med = lambda v: sorted(v)[len(v) // 2]
    with tempfile.TemporaryDirectory() as tmp:
        sets = {"robonet-like": ("tfds_robonet", os.path.join(tmp, "robonet"), (22, 256, 320), "image", 0),
                "bair-like": ("bair_robot_pushing", os.path.join(tmp, "bair"), (30, 64, 64), "aux1_image", 4)}
        say(f"device {torch.cuda.get_device_name(0)}; {a.episodes} synthetic episodes per set (np.savez_compressed), segment 16 frames -> 64 x 64, "
            f"batch {a.batch}; {a.repeats} repeats after one warm pass, median [min, max]; host clock around a pass that ends in a device synchronise")
        for label, (name, root, (n, height, width), key, adim) in sets.items():
            size = write_episodes(root, a.episodes, n, height, width, key, adim, seed=len(label))
            say(f"{label}: {n} x {height} x {width} x 3 uint8, {size / 1e6:.2f} MB per file ({n * height * width * 3 / size:.1f} x compressed), "
                f"{16 * height * width * 3 / 1e6:.2f} MB of frames staged per clip")
            for workers in (1, 4, 16):
                dl = EvalDataLoader(name, 16, 64, batch_size=a.batch, num_workers=workers, load_action=bool(adim), device=DEV, root=root)
                loader_pass(dl)
                rates = [loader_pass(dl) for _ in range(a.repeats)]
                say(f"    loader alone, {workers:2d} reader threads: {med(rates):8.1f} [{min(rates):.1f}, {max(rates):.1f}] clips/s "
                    f"({1e3 * a.batch / med(rates):.2f} ms per batch)")

        # ---- evaluate: the loader against the same batches preloaded on the device
        name, root = sets["bair-like"][:2]
        dev = torch.device(DEV)
        tcfg = W.tokenizer_config(**W.CTX_VAE64)
        tok = CompressiveVQModel(tcfg, W.random_tokenizer_state_dict(tcfg, 0, codebook_std=0.4)).to(dev)
        flags = SimpleNamespace(pretrained_transformer_path=None, pretrained_model_name_or_path=None, action_conditioned=True, action_dim=4,
                                reward_prediction=False, context_length=2, segment_length=16)
        model = train_gpt.build_eval_model(flags, tok.num_vq_embeddings + tok.num_dyn_embeddings + 2, dev)
        args = train_gpt.eval_args(context_length=2, segment_length=16, eval_generate_times=1, action_conditioned=True, log_gif_interval=10 ** 9)
        loader = EvalDataLoader(name, 16, 64, batch_size=a.batch, num_workers=4, load_action=True, device=DEV, root=root)
        preloaded = [(f.clone(), x.clone()) for f, x in loader]
        n_batches = len(preloaded)

        def run(batches):
            torch.manual_seed(0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            logs = train_gpt.evaluate(args, LocalAccelerator(dev), tok, model, batches, Evaluator(), 0)
            torch.cuda.synchronize()
            return 1e3 * (time.perf_counter() - t0) / n_batches, logs

        run(preloaded)
        base, fed, blocked, first, waited, same = [], [], [], [], [], True
        for _ in range(a.repeats):
            ms0, logs0 = run(preloaded)
            timed = TimedNext(loader)
            ms1, logs1 = run(timed)
            base.append(ms0); fed.append(ms1); blocked.append(1e3 * sum(timed.calls) / n_batches); first.append(1e3 * timed.calls[0])
            waited.append(1e3 * loader.wait_s / n_batches)
            same = same and all(logs0[k] == logs1[k] or (logs0[k] != logs0[k] and logs1[k] != logs1[k]) for k in logs0)
        say(f"evaluate, bair-like, {n_batches} batches of {a.batch}, action-conditioned, 4 reader threads (ms per batch, whole loop incl. the final gathers):")
        say(f"    batches preloaded on the device (baseline): {med(base):8.2f} [{min(base):.2f}, {max(base):.2f}]")
        say(f"    batches from the loader:                    {med(fed):8.2f} [{min(fed):.2f}, {max(fed):.2f}]   ({med(fed) / med(base):.3f} x the baseline)")
        say(f"    host time blocked in the loader's next():   {med(blocked):8.2f} [{min(blocked):.2f}, {max(blocked):.2f}]   "
            f"({100 * med(blocked) / med(fed):.1f} % of the loop; of it waiting for reader threads {med(waited):.2f})")
        say(f"    the first next() of a pass, which nothing overlaps: {med(first):.2f} ms [{min(first):.2f}, {max(first):.2f}]")
        say(f"    eval logs of the two runs identical: {same}")


if __name__ == "__main__":
    main()
