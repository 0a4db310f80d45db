"""What resampling on the kept K / V cache buys (ivg_kv_select; kv_gather_rows_kernel).  Development tool; bench.py is the contract and does
not know the feature.  Prints a text report (profiles/kv_select.txt is one).

    python tools/kv_select_bench.py [--out REPORT] [--rounds N]     the measurement, in a child process under a time limit
    python tools/kv_select_bench.py --arm run [--rounds N]          the measurement itself

BASELINE config 2's transformer (Llama-small, bf16, seeded weights) under the action wrapper, B = 64 trajectories, sampled with top-k 100.
For k = 1, 6, 13 imagined frames the engine keeps the cache of a 514 + 17 k token prompt; then half of the trajectories survive and each
survivor is duplicated over a dropped one (``stable_parents``: survivors keep their rows).  Arms, ALTERNATING round by round in one
process, HIP events around each, medians:
  (a) select + continue   ``select_kept_cache(parents)``, then the 17-token ``generate(reuse_cache=True)`` on the gathered prompt and actions
  (b) re-prefill          the same rows through a fresh ``generate`` of 17 tokens on the gathered grown prompt: the prompt pass a caller
                          pays without the feature (that code path is untouched by it)
  (c) select alone        a full cyclic shift of the 64 rows, every row through scratch -- the worst case: cache bytes gathered per second
Before every timed (a) and (c) the kept cache is rebuilt by the untimed first call."""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, CTX, KS = 64, 2, (1, 6, 13)
LIMIT_S = 900


def arm_run(rounds):
    import numpy as np
    import torch
    from ivideogpt_amd import HeadModelWithAction, LlamaForCausalLM, weights as W
    from ivideogpt_amd.transformer import stable_parents
    dev = torch.device("cuda:0")
    cfg = dict(W.LLAMA_SMALL)
    frames = max(KS) + 2
    head = HeadModelWithAction(LlamaForCausalLM(cfg, None, dtype="bf16"), 4, 257 * CTX - 1, 16, CTX, CTX + frames, reward_prediction=True)
    head.load_state_dict(W.random_llama_state_dict(cfg, 2, action_dim=4, reward_prediction=True), strict=True)
    head.to(dev)
    gen = torch.Generator().manual_seed(1)
    L0 = 257 * CTX
    prompt = torch.randint(0, 8192, (B, L0), generator=gen)
    prompt[:, 256], prompt[:, -1] = cfg["vocab_size"] - 2, cfg["vocab_size"] - 1
    prompt = prompt.to(dev)
    table = torch.randn(B, CTX + frames, 4, generator=gen).to(dev)
    rng = np.random.default_rng(3)
    alive = np.sort(rng.permutation(B)[:B // 2])
    parents, _ = stable_parents(np.repeat(alive, 2), B)      # every survivor twice: once in its own row, once over a dropped row
    assert int((parents == torch.arange(B)).sum()) == B // 2
    idx = parents.to(dev)
    shift = [(i + 1) % B for i in range(B)]
    lc = head.llm._cfg
    hd = lc["hidden_size"] // lc["num_attention_heads"]
    print(f"# {torch.cuda.get_device_name(0)}, Llama-small bf16 (12 layers, 12 heads of 64), B = {B}, top-k 100, median of {rounds} alternating rounds (HIP events)")
    print(f"# parents: {B // 2} survivors in place, {B // 2} rows copied in place from a survivor (0 staged); cyclic shift: {B} rows staged")

    def timed(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        r = f()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), r

    for k in KS:
        n0 = 17 * k
        u0 = torch.rand(B, n0, generator=gen).to(dev)
        v = torch.rand(B, 17, generator=gen).to(dev)

        def first():
            return head.generate(prompt, do_sample=True, top_k=100, max_new_tokens=n0, action=table, uniforms=u0)

        def arm_a(grown):
            head.select_kept_cache(parents)
            return head.generate(grown[idx], do_sample=True, top_k=100, max_new_tokens=17, action=table[idx], uniforms=v, reuse_cache=True)

        def arm_b(grown):
            return head.generate(grown[idx], do_sample=True, top_k=100, max_new_tokens=17, action=table[idx], uniforms=v)

        grown = first()
        ta, tb, tc = [], [], []
        for r in range(rounds + 2):          # two warm-up rounds (workspace, one-time kernel set-up of every shape)
            first()
            a_ms, out_a = timed(lambda: arm_a(grown))
            b_ms, out_b = timed(lambda: arm_b(grown))
            first()
            c_ms, _ = timed(lambda: head.select_kept_cache(shift))
            if r >= 2:
                ta.append(a_ms); tb.append(b_ms); tc.append(c_ms)
        same = (out_a[:, -17:] == out_b[:, -17:]).float().mean().item()
        ma, mb, mc = statistics.median(ta), statistics.median(tb), statistics.median(tc)
        kept = L0 + n0 - 1                                        # positions the kept cache holds
        payload = B * lc["num_hidden_layers"] * 2 * lc["num_attention_heads"] * kept * hd * 2
        print(f"k = {k:2d}: grown prompt {L0 + n0} tokens, kept cache {kept} positions")
        print(f"  (a) select + 17-token continue {ma:8.3f} ms (min {min(ta):.3f}, max {max(ta):.3f})   {B / ma * 1e3:7.0f} imagined steps/s")
        print(f"  (b) re-prefill + 17 tokens     {mb:8.3f} ms (min {min(tb):.3f}, max {max(tb):.3f})   {B / mb * 1e3:7.0f} imagined steps/s")
        print(f"      (a) is {mb / ma:.2f} x {'faster' if ma < mb else 'SLOWER'} than (b); {100 * same:.0f} % of the 17 new tokens equal "
              f"(random weights, near-flat distributions: the prompt's last position goes through the decode kernels in (a), the prompt pass in (b), "
              f"and the first flipped near-tie changes what follows; tests/test_gpu_kv_select.py holds (a) to the unselected kept-cache run bit for bit)")
        print(f"  (c) select alone, cyclic shift {mc:8.3f} ms (min {min(tc):.3f}, max {max(tc):.3f})   {payload / 1e6:.1f} MB of K / V rows gathered "
              f"= {payload / mc / 1e6:.1f} GB/s (each byte read twice and written twice: through scratch)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arm", choices=("run",))
    ap.add_argument("--rounds", type=int, default=20)
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
    text = f"# python tools/kv_select_bench.py --rounds {a.rounds}\n" + r.stdout
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
