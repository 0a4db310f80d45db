"""What setting the kept K / V cache aside and bringing it back costs (ivg_kv_snapshot_create / _restore; launch_kv_snapshot over
kv_gather_rows_kernel), against the only route a caller had before: a prompt pass over the whole tracked row.  Development tool;
bench.py is the contract and does not know the feature.  Prints a text report (profiles/kv_snapshot.txt is one).

    python tools/kv_snapshot_bench.py [--out REPORT] [--rounds N]     the measurement, in a child process under a time limit
    python tools/kv_snapshot_bench.py --arm run [--rounds N]          the measurement itself

BASELINE config 2's transformer (Llama-small, bf16, seeded weights) under the action wrapper, B = 16 and 64, a kept cache of 513 (the
context alone) and 717 (twelve frames later) positions.  Arms ALTERNATE round by round in one process, HIP events around each, medians.
  (a) save                ``save_kept_cache``: hipMalloc of the snapshot and the copy out (the hipFree of ``close`` is not timed)
  (b) restore             ``restore_kept_cache`` of every row, after another call overwrote the kept cache
  (c) save + restore      both, back to back
  (d) prompt pass         what ``TrackedEpisode._establish`` does, the route without the entries: ``generate`` of ONE token over the
                          tracked tokens, then the rewind in front of the last sdf slot
  (e) select, all staged  ``select_kept_cache`` with a cyclic shift: every row out to scratch and back in, the same bytes moved twice
GB/s: the snapshot's bytes over the time, each byte read once and written once ((c) and (e): twice the bytes)."""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CTX, BATCHES, FRAMES = 2, (16, 64), (0, 12)
LIMIT_S = 900


def timed(f):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    r = f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), r


def line(name, ts, nbytes):
    m = statistics.median(ts)
    rate = f"{nbytes / m / 1e6:8.0f} GB/s" if nbytes else ""
    return f"  {name:<34s}{m:8.3f} ms (min {min(ts):.3f}, max {max(ts):.3f})   {rate}", m


def arm_run(rounds):
    import torch
    from kv_extend_bench import inputs, make_world
    frames = max(FRAMES) + 3
    head, cfg = make_world(frames)
    print(f"# {torch.cuda.get_device_name(0)}, Llama-small bf16 (12 layers, 12 heads of 64), median of {rounds} alternating rounds (HIP events)")
    for B in BATCHES:
        prompt, table, gen = inputs(cfg, frames, B)
        head.llm._ensure(B, table.shape[1])
        for k in FRAMES:
            keep = 257 * CTX + 17 * k - 1
            if k:
                u = torch.rand(B, 17 * k, generator=gen).to("cuda:0")
                tokens = head.generate(prompt, do_sample=True, top_k=100, max_new_tokens=17 * k, action=table, uniforms=u).contiguous()
            else:
                tokens = prompt

            def establish():
                head.generate(tokens, do_sample=False, max_new_tokens=1, action=table)
                head.extend_kept_cache(tokens, action=table, keep=keep)

            def overwrite():
                head.generate(prompt[:2].contiguous(), do_sample=False, max_new_tokens=1, action=table[:2].contiguous())

            def both():
                kept = head.save_kept_cache()
                head.restore_kept_cache(kept)
                return kept

            shift = [(i + 1) % B for i in range(B)]
            ta, tb, tc, td, te = [], [], [], [], []
            nbytes = 0
            for r in range(rounds + 2):          # two warm-up rounds
                establish()
                a_ms, kept = timed(head.save_kept_cache)
                nbytes = kept.nbytes
                overwrite()
                b_ms, _ = timed(lambda: head.restore_kept_cache(kept))
                head.extend_kept_cache(tokens, action=table, keep=keep)      # (verified on the device: the restored rows are the tracked ones)
                kept.close()
                c_ms, kept = timed(both)
                kept.close()
                d_ms, _ = timed(establish)
                e_ms, _ = timed(lambda: head.select_kept_cache(shift))
                if r >= 2:
                    ta.append(a_ms); tb.append(b_ms); tc.append(c_ms); td.append(d_ms); te.append(e_ms)
            print(f"B = {B}, kept cache {keep} positions: snapshot of {nbytes / 1e6:.1f} MB")
            la, ma = line("(a) save", ta, nbytes)
            lb, mb = line("(b) restore", tb, nbytes)
            lc, mc = line("(c) save + restore", tc, 2 * nbytes)
            ld, md = line("(d) prompt pass (_establish)", td, 0)
            le, me = line("(e) select, every row staged", te, 2 * nbytes)
            for text in (la, lb, lc, ld, le):
                print(text)
            print(f"      restore is {md / mb:.2f} x {'faster' if mb < md else 'SLOWER'} than the prompt pass; save + restore {md / (ma + mb):.2f} x "
                  f"{'faster' if ma + mb < md else 'SLOWER'}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arm", choices=("run",))
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.arm == "run":
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        return arm_run(a.rounds)
    # (this process never opens the GPU; nothing more is started after a child that failed or ran out of time)
    r = subprocess.run(["timeout", "-k", "10", str(LIMIT_S), sys.executable, os.path.abspath(__file__), "--arm", "run", "--rounds", str(a.rounds)],
                       cwd=ROOT, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-4000:] + r.stderr[-4000:])
        raise SystemExit(f"the measurement failed with exit status {r.returncode}")
    text = f"# python tools/kv_snapshot_bench.py --rounds {a.rounds}\n" + r.stdout
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
