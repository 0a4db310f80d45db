"""What the frame heads and token scores of an observed frame cost on top of extending the kept K / V cache (ivg_kv_extend_scored;
frame_rows_heads_kernel, token_scores_rows_kernel), and what a caller paid for them before.  Development tool; bench.py is the
contract and does not know the feature.  Prints a text report (profiles/kv_extend_heads.txt is one).

    python tools/kv_extend_heads_bench.py [--out REPORT] [--rounds N]     the measurement, in a child process under a time limit
    python tools/kv_extend_heads_bench.py --arm run [--rounds N]          the measurement itself

The protocol of tools/kv_extend_bench.py: BASELINE config 2's transformer (Llama-small, bf16, seeded weights) under the action
wrapper, B = 64, the chunk pass; arms ALTERNATE round by round in one process, HIP events around each, medians; the kept cache is
rebuilt by an untimed call before every timed arm.  At a kept cache of 514 + 17 k - 1 positions (k = 1, 13: 530 and 734), 17 given
tokens appended:
  (a0) extend alone        ivg_kv_extend without an output: no lm_head pass
  (a)  extend + NLL        ivg_kv_extend with token_nll_out
  (b)  extend + all four   ivg_kv_extend_scored with token_nll, token_scores, frame_rewards and frame_hidden
  (c)  eval forward        what a caller had to ADD to (a) for the hidden states before: ivg_eval_forward(hidden=...) over the whole row
                           (its token_nll comes with it; scores needed ivg_logits over the row on top -- not timed, (B, L, V) fp32)"""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, ROOT)

LIMIT_S = 600


def arm_run(rounds):
    import torch
    from kv_extend_bench import B, CTX, KS, inputs, make_world, set_route, timed
    from ivideogpt_amd import _lib
    frames = max(KS) + 3
    head, cfg = make_world(frames)
    prompt, table, gen = inputs(cfg, frames, B)
    lib = _lib.load()
    set_route(True)
    H = cfg["hidden_size"]
    print(f"# {torch.cuda.get_device_name(0)}, Llama-small bf16 (12 layers, 12 heads of 64), B = {B}, 17 given tokens, chunk pass, "
          f"median of {rounds} alternating rounds (HIP events)")
    for k in KS:
        n0 = 17 * k
        u = torch.rand(B, n0 + 17, generator=gen).to("cuda:0")
        full = head.generate(prompt, do_sample=True, top_k=100, max_new_tokens=n0 + 17, action=table, uniforms=u)[:, :257 * CTX + n0 + 17].contiguous()
        keep, L = 257 * CTX + n0 - 1, full.shape[1]
        eng = head.llm._engine
        nll_all = torch.zeros(B, L, device="cuda:0")
        rows2 = torch.zeros(B, 2, device="cuda:0")
        hid_all = torch.zeros(B, L, H, dtype=torch.bfloat16, device="cuda:0")

        def first():
            return head.generate(prompt, do_sample=True, top_k=100, max_new_tokens=n0, action=table, uniforms=u[:, :n0].contiguous())

        arms = {
            "(a0) extend alone": lambda: head.extend_kept_cache(full, action=table, keep=keep),
            "(a)  extend + NLL": lambda: head.extend_kept_cache(full, action=table, keep=keep, return_nll=True),
            "(b)  extend + NLL, scores, frame heads": lambda: head.extend_kept_cache(full, action=table, keep=keep, return_nll=True, return_reward="frames",
                                                                                   output_frame_hidden_states=True, output_token_scores=True),
            "(c)  eval forward over the whole row": lambda: eng.eval_forward(full, full, nll_all, rows2, actions=table, ctx=CTX, hidden=hid_all),
        }
        ts = {name: [] for name in arms}
        out = {}
        for r in range(rounds + 2):          # two warm-up rounds (workspace, one-time kernel set-up of every shape)
            for name, f in arms.items():
                first()
                c0 = lib.ivg_debug_counter(b"kv_extend_chunk_rows")
                ms, out[name] = timed(f)
                assert name.startswith("(c)") or lib.ivg_debug_counter(b"kv_extend_chunk_rows") - c0 == B * 17
                if r >= 2:
                    ts[name].append(ms)
        med = {name: statistics.median(v) for name, v in ts.items()}
        print(f"k = {k:2d}: kept cache {keep} positions, extended to {keep + 17}; the whole row is {L} tokens")
        for name, v in ts.items():
            print(f"  {name:<42s}{med[name]:8.3f} ms (min {min(v):.3f}, max {max(v):.3f})")
        a0, a, b, c = (med[n] for n in arms)
        o = out["(b)  extend + NLL, scores, frame heads"]
        q = keep + 16   # the frame's 16th token
        print(f"      (b) - (a) = {b - a:+.3f} ms; (a)'s own lm_head pass (a) - (a0) = {a - a0:+.3f} ms; (c) = {c:.3f} ms = {c / max(b - a, 1e-6):.0f} x (b) - (a)")
        print(f"      max |frame_hidden - eval forward's hidden row {q}| = {(o.frame_hidden[:, 0].float() - hid_all[:, q].float()).abs().max().item():.3e}; "
              f"max |NLL + logprob| over the 16 scored columns = {(o.token_nll[:, :16] + o.token_scores.logprob[:, :16]).abs().max().item():.3e}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arm", choices=("run",))
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.arm == "run":
        return arm_run(a.rounds)
    # (this process never opens the GPU; nothing more is started after a child that failed or ran out of time)
    r = subprocess.run(["timeout", "-k", "10", str(LIMIT_S), sys.executable, os.path.abspath(__file__), "--arm", "run", "--rounds", str(a.rounds)],
                       cwd=ROOT, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-4000:] + r.stderr[-4000:])
        raise SystemExit(f"the measurement failed with exit status {r.returncode}")
    text = f"# python tools/kv_extend_heads_bench.py --rounds {a.rounds}\n" + r.stdout
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
