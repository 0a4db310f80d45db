"""What the filtered scores cost (ivg_generate_filtered; filtered_scores_kernel, one more launch per decode step).  Development tool;
bench.py is the contract and does not know the feature.  Prints a text report (profiles/filtered_scores.txt is one).

    python tools/filtered_scores_bench.py [--out REPORT] [--dir SCRATCH]     both arms, each a child process under its own time limit
    python tools/filtered_scores_bench.py --arm kernel                       the launches alone (run under rocprofv3 --kernel-trace to time them)
    python tools/filtered_scores_bench.py --summarize TRACE.csv              us per launch from the kernel trace of that run
    python tools/filtered_scores_bench.py --arm rollout [--rounds N]         the rollout with and without the output

  kernel   ivg_op_filtered_scores on B = 64 rows of V = 16,386 logits (N(0, 3^2), seeded) under each of SETTINGS, one after the other:
           WARM untimed launches, then TIMED; the time of a launch is the kernel's own, from the trace (the hook allocates its step state
           and synchronises around the launch).  The trace lists the launches in order, so launch i belongs to setting i // (WARM + TIMED).
  rollout  BASELINE config 2's transformer (Llama-small, bf16, seeded weights), B = 64, 514 prompt tokens, 237 new ones, sampled with
           top-k 100 (top_p 1 and top_p 0.9): ``generate`` with and without ``output_filtered_scores`` ALTERNATING round by round in one
           process, HIP events around each call, median per arm.  The call without the output launches what the parent commit launches
           (tests/test_gpu_filtered_scores.py: same ids, same counters), so its time is the parent's for the same call.
The driver starts nothing more after a step that fails or runs out of time."""
import argparse
import ctypes as C
import glob
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARM, TIMED = 10, 40
B, V = 64, 16386
# (name, top_k, temperature, top_p, greedy)
SETTINGS = (("top_k 100", 100, 1.0, 1.0, 0), ("top_k 100, top_p 0.9, temperature 0.7", 100, 0.7, 0.9, 0), ("top_k 0 (all), top_p 0.9", 0, 1.0, 0.9, 0),
            ("greedy", 100, 1.0, 1.0, 1))
KERNEL_LIMIT_S, ROLLOUT_LIMIT_S = 240, 420


def arm_kernel():
    import torch
    from ivideogpt_amd import _lib
    l = _lib.load()
    g = torch.Generator().manual_seed(0)
    lg = (torch.randn(B, V, generator=g) * 3).cuda()
    ids = torch.randint(0, V, (B,), generator=g).cuda()
    out = torch.zeros(B, 4, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for name, top_k, temperature, top_p, greedy in SETTINGS:
        for _ in range(WARM + TIMED):
            assert l.ivg_op_filtered_scores(C.c_void_p(lg.data_ptr()), C.c_void_p(ids.data_ptr()), B, V, top_k, C.c_float(temperature), C.c_float(top_p),
                                            greedy, C.c_void_p(out.data_ptr()), st) == 0
        torch.cuda.synchronize()
        print("ok", name, out[0].tolist())


def summarize(path):
    import csv
    rows = [r for r in csv.DictReader(open(path)) if "filtered_scores_kernel" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    per = WARM + TIMED
    assert len(rows) == per * len(SETTINGS), f"{len(rows)} filtered_scores_kernel launches in {path}, expected {per * len(SETTINGS)}"
    lines = [f"filtered_scores_kernel alone, B = {B}, V = {V} ({TIMED} launches after {WARM} warm-up per setting, kernel trace):"]
    for i, s in enumerate(SETTINGS):
        us = sorted((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows[i * per + WARM:(i + 1) * per])
        lines.append(f"  {s[0]:42s} median {statistics.median(us):7.2f} us  min {us[0]:.2f}  max {us[-1]:.2f}")
    return "\n".join(lines)


def arm_rollout(rounds):
    import torch
    from ivideogpt_amd import LlamaForCausalLM, weights as W
    dev = torch.device("cuda:0")
    cfg = dict(W.LLAMA_SMALL)
    m = LlamaForCausalLM(cfg, W.random_llama_state_dict(cfg, 0), dtype="bf16").to(dev)
    gen = torch.Generator().manual_seed(1)
    L0, n_new = 514, 17 * 14 - 1
    prompt = torch.randint(0, 8192, (B, L0), generator=gen)
    prompt[:, 256], prompt[:, -1] = cfg["vocab_size"] - 2, cfg["vocab_size"] - 1
    prompt = prompt.to(dev)
    u = torch.rand(B, n_new, generator=gen).to(dev)

    def roll(top_p, filtered):
        return m.generate(prompt, do_sample=True, top_k=100, top_p=top_p, max_new_tokens=n_new, uniforms=u, output_filtered_scores=filtered)

    def timed(top_p, filtered):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        roll(top_p, filtered)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    print(f"rollout on {torch.cuda.get_device_name(0)}, Llama-small bf16, B = {B}, {L0} + {n_new} tokens, top-k 100, median of {rounds} alternating rounds "
          f"(HIP events):")
    for top_p in (None, 0.9):
        plain, (scored, fs) = roll(top_p, False), roll(top_p, True)     # warm both arms (engine, workspace, both sets of step graphs)
        assert torch.equal(plain, scored), "the rollout with filtered scores decides other tokens"
        assert torch.isfinite(fs.logprob).all() and (fs.support >= 1).all(), "a drawn token outside the kernel's survivor set"
        roll(top_p, False), roll(top_p, True)
        t = {False: [], True: []}
        for _ in range(rounds):
            for arm in (False, True):
                t[arm].append(timed(top_p, arm))
        med = {k: statistics.median(v) for k, v in t.items()}
        print(f" top_p {top_p if top_p is not None else 1.0}:")
        for arm, name in ((False, "without the output"), (True, "with the output   ")):
            print(f"  {name} {med[arm]:8.2f} ms (min {min(t[arm]):.2f}, max {max(t[arm]):.2f})")
        d = med[True] - med[False]
        print(f"  difference {d:+.3f} ms per rollout = {1e3 * d / n_new:+.2f} us per decode step ({100 * d / med[False]:+.2f} %); "
              f"mean filtered logprob {fs.logprob.mean().item():.3f}, mean kept log-mass {fs.kept_logmass.mean().item():.3f}, "
              f"mean support {fs.support.mean().item():.1f}")


def child(cmd, limit, log):
    """One step in a process of its own under a time limit -> its output; raises when it failed or ran out of time."""
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, cwd=ROOT, capture_output=True, text=True)
    log.append(f"$ {' '.join(os.path.relpath(c, ROOT) if os.path.isabs(c) and c.startswith(ROOT) else c for c in cmd)}   (exit {r.returncode})")
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-4000:] + r.stderr[-4000:])
        raise SystemExit(f"step failed with exit status {r.returncode}: nothing more is started")
    return r.stdout


def driver(a):
    me = os.path.abspath(__file__)      # (this process never opens the GPU: each arm is a child of its own)
    os.makedirs(a.dir, exist_ok=True)
    log = []
    out = [f"# tools/filtered_scores_bench.py --rounds {a.rounds}: GPU_MAX_HW_QUEUES={os.environ.get('GPU_MAX_HW_QUEUES', '(unset)')}"]
    child(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", a.dir, "-o", "filtered_scores", "--", sys.executable, me, "--arm", "kernel"],
          KERNEL_LIMIT_S, log)
    traces = sorted(glob.glob(os.path.join(a.dir, "**", "*kernel_trace.csv"), recursive=True), key=os.path.getmtime)
    assert traces, f"no kernel trace under {a.dir}"
    out.append(summarize(traces[-1]))
    out.append(child([sys.executable, me, "--arm", "rollout", "--rounds", str(a.rounds)], ROLLOUT_LIMIT_S, log).rstrip())
    text = "\n".join(out)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arm", choices=("kernel", "rollout"))
    ap.add_argument("--summarize", default="")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--dir", default=os.path.join(ROOT, "build", "filtered_scores_trace"))
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.summarize:
        print(summarize(a.summarize))
    elif a.arm == "kernel":
        arm_kernel()
    elif a.arm == "rollout":
        arm_rollout(a.rounds)
    else:
        driver(a)


if __name__ == "__main__":
    main()
