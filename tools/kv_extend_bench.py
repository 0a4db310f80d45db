"""What extending the kept K / V cache with given tokens, and fanning candidates out of it, buy (ivg_kv_extend, ivg_generate_fanout;
chunk_attn_kernel).  Development tool; bench.py is the contract and does not know the feature.  Prints a text report
(profiles/kv_extend.txt is one).

    python tools/kv_extend_bench.py [--out REPORT] [--rounds N]     the measurement, in a child process under a time limit
    python tools/kv_extend_bench.py --arm run [--rounds N]          the measurement itself
    python tools/kv_extend_bench.py --arm trace --route chunk|steps one warm extend, then 10 more: under a kernel trace, launches per call

BASELINE config 2's transformer (Llama-small, bf16, seeded weights) under the action wrapper, B = 64, sampled with top-k 100.  Arms
ALTERNATE round by round in one process, HIP events around each, medians.  Before every timed arm that needs one, the kept cache is rebuilt
by an untimed call.
Extend, at a kept cache of 514 + 17 k - 1 positions (k = 1, 13): 17 given tokens appended
  (a) chunk pass          ivg_kv_extend, one pass over the 64 x 17 rows (chunk_attn_kernel)
  (b) decode steps        the same call under IVG_KV_EXTEND_CHUNK=0: 17 decode steps with given inputs
  (c) prompt pass         what a caller has without the entry: ivg_generate of ONE token over the whole grown prompt (its prompt pass
                          rebuilds the cache; the one sampler step is part of it)
Fan-out, 8 histories x 16 candidates, 17 new tokens:
  (d) fan-out             ivg_generate_fanout from the kept cache
  (e) shared context      ivg_generate_shared on the same prompts: one prompt pass per history (an action-conditioned shared prompt is the
                          context alone, 514 tokens; the kept cache is rewound to 513 positions for this comparison)
  (f) select + continue   ivg_kv_select growing the kept cache to 128 rows, then ivg_generate_continue on the repeated prompt rows
  (d) and (f) again from a kept cache of 530 positions, where (e) does not apply."""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, CTX, KS = 64, 2, (1, 13)
GROUPS, CAND = 8, 16
LIMIT_S = 900


def make_world(frames):
    import torch
    from ivideogpt_amd import HeadModelWithAction, LlamaForCausalLM, weights as W
    cfg = dict(W.LLAMA_SMALL)
    head = HeadModelWithAction(LlamaForCausalLM(cfg, None, dtype="bf16"), 4, 257 * CTX - 1, 16, CTX, CTX + frames, reward_prediction=True)
    head.load_state_dict(W.random_llama_state_dict(cfg, 2, action_dim=4, reward_prediction=True), strict=True)
    head.to(torch.device("cuda:0"))
    return head, cfg


def set_route(chunk):
    from ivideogpt_amd import _lib
    os.environ["IVG_DEV"] = "1"
    os.environ["IVG_KV_EXTEND_CHUNK"] = "1" if chunk else "0"
    _lib.reload_switches()


def inputs(cfg, frames, rows):
    import torch
    gen = torch.Generator().manual_seed(1)
    prompt = torch.randint(0, 8192, (rows, 257 * CTX), generator=gen)
    prompt[:, 256], prompt[:, -1] = cfg["vocab_size"] - 2, cfg["vocab_size"] - 1
    return prompt.to("cuda:0"), torch.randn(rows, CTX + frames, 4, generator=gen).to("cuda:0"), gen


def timed(f):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    r = f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), r


def line(name, ts, unit_rows):
    m = statistics.median(ts)
    return f"  {name:<34s}{m:8.3f} ms (min {min(ts):.3f}, max {max(ts):.3f})   {unit_rows / m * 1e3:9.0f} rows/s", m


def arm_run(rounds):
    import torch
    from ivideogpt_amd import _lib
    frames = max(KS) + 3
    head, cfg = make_world(frames)
    prompt, table, gen = inputs(cfg, frames, B)
    print(f"# {torch.cuda.get_device_name(0)}, Llama-small bf16 (12 layers, 12 heads of 64), top-k 100, median of {rounds} alternating rounds (HIP events)")
    print(f"# extend: B = {B}, 17 given tokens")
    lib = _lib.load()
    for k in KS:
        n0 = 17 * k
        u = torch.rand(B, n0 + 17, generator=gen).to("cuda:0")
        full = head.generate(prompt, do_sample=True, top_k=100, max_new_tokens=n0 + 17, action=table, uniforms=u)[:, :257 * CTX + n0 + 17].contiguous()
        keep = 257 * CTX + n0 - 1

        def first():
            return head.generate(prompt, do_sample=True, top_k=100, max_new_tokens=n0, action=table, uniforms=u[:, :n0].contiguous())

        def ext():
            return head.extend_kept_cache(full, action=table, keep=keep, return_nll=True)

        def prefill():
            return head.generate(full, do_sample=True, top_k=100, max_new_tokens=1, action=table, uniforms=u[:, :1].contiguous())

        ta, tb, tc = [], [], []
        for r in range(rounds + 2):          # two warm-up rounds (workspace, one-time kernel set-up of every shape)
            set_route(True); first()
            c0 = lib.ivg_debug_counter(b"kv_extend_chunk_rows")
            a_ms, nll_a = timed(ext)
            assert lib.ivg_debug_counter(b"kv_extend_chunk_rows") - c0 == B * 17
            set_route(False); first()
            c0 = lib.ivg_debug_counter(b"kv_extend_step_rows")
            b_ms, nll_b = timed(ext)
            assert lib.ivg_debug_counter(b"kv_extend_step_rows") - c0 == B * 17
            c_ms, _ = timed(prefill)
            if r >= 2:
                ta.append(a_ms); tb.append(b_ms); tc.append(c_ms)
        set_route(True)
        print(f"k = {k:2d}: kept cache {keep} positions, extended to {keep + 17}")
        la, ma = line("(a) extend, chunk pass", ta, B)
        lb, mb = line("(b) extend, 17 decode steps", tb, B)
        lc, mc = line("(c) prompt pass over the whole row", tc, B)
        print(la); print(lb); print(lc)
        print(f"      (a) is {mb / ma:.2f} x {'faster' if ma < mb else 'SLOWER'} than (b) and {mc / ma:.2f} x {'faster' if ma < mc else 'SLOWER'} than (c); "
              f"max |NLL (a) - NLL (b)| = {(nll_a - nll_b).abs().max().item():.3e} (mean NLL {nll_b.mean().item():.3f})")
    # ---- fan-out
    n = GROUPS * CAND
    head.llm._ensure(n, table.shape[1])
    hp, ht = prompt[:GROUPS].contiguous(), table[:GROUPS].contiguous()
    gt = torch.randn(n, table.shape[1], 4, generator=gen).to("cuda:0")
    gu = torch.rand(n, 17, generator=gen).to("cuda:0")
    u0 = torch.rand(GROUPS, 17, generator=gen).to("cuda:0")
    par = [g for g in range(GROUPS) for _ in range(CAND)]
    idx = torch.tensor(par, device="cuda:0")
    print(f"# fan-out: {GROUPS} histories x {CAND} candidates, 17 new tokens")
    for kept in (513, 530):
        def first():
            grown = head.generate(hp, do_sample=True, top_k=100, max_new_tokens=17, action=ht, uniforms=u0)
            if kept == 513:
                head.extend_kept_cache(hp, action=ht, keep=513)       # rewind to the context alone
                return hp
            return grown.contiguous()

        base = first()
        gt2 = gt.clone()
        gt2[:, :CTX] = ht[idx, :CTX]                                  # (the select route compares the row of the slot cached at 513)
        rep = base[idx].contiguous()

        def fan():
            return head.fan_out(base, CAND, action=gt2, do_sample=True, top_k=100, max_new_tokens=17, uniforms=gu)

        def shared():   # rows k * GROUPS + g, the public order of shared_context
            perm = torch.arange(n, device="cuda:0").view(GROUPS, CAND).t().reshape(-1)
            return head.generate(base.repeat(CAND, 1), do_sample=True, top_k=100, max_new_tokens=17, action=gt2[perm].contiguous(),
                                 uniforms=gu[perm].contiguous(), shared_context=CAND)

        def select_continue():
            head.select_kept_cache(par)
            return head.generate(rep, do_sample=True, top_k=100, max_new_tokens=17, action=gt2, uniforms=gu, reuse_cache=True)

        td, te, tf = [], [], []
        for r in range(rounds + 2):
            first()
            d_ms, out_d = timed(fan)
            e_ms = timed(shared)[0] if kept == 513 else None
            first()
            f_ms, out_f = timed(select_continue)
            if r >= 2:
                td.append(d_ms); tf.append(f_ms)
                if e_ms is not None:
                    te.append(e_ms)
        print(f"kept cache {kept} positions x {GROUPS} rows: fan-out == select + continue bit for bit: {bool(torch.equal(out_d, out_f))}")
        ld, md = line("(d) fan-out from the kept cache", td, n)
        print(ld)
        if te:
            le, me = line("(e) shared context (prompt pass)", te, n)
            print(le)
        lf, mf = line("(f) select to 128 rows + continue", tf, n)
        print(lf)
        print(f"      (d) is {mf / md:.2f} x {'faster' if md < mf else 'SLOWER'} than (f)" + (f" and {me / md:.2f} x {'faster' if md < me else 'SLOWER'} than (e)" if te else ""))


def arm_trace(route):
    """One warm extend, then 10 more of one route: `rocprofv3 --kernel-trace --stats -- python tools/kv_extend_bench.py --arm trace --route R`
    counts the launches (divide what the 17-token generate and the extends share out by running both routes)."""
    import torch
    head, cfg = make_world(4)
    prompt, table, gen = inputs(cfg, 4, B)
    u = torch.rand(B, 34, generator=gen).to("cuda:0")
    full = head.generate(prompt, do_sample=True, top_k=100, max_new_tokens=34, action=table, uniforms=u)[:, :548].contiguous()
    set_route(route == "chunk")
    head.generate(prompt, do_sample=True, top_k=100, max_new_tokens=17, action=table, uniforms=u[:, :17].contiguous())   # keeps 530 positions
    short = full[:, :531].contiguous()
    for _ in range(11):
        head.extend_kept_cache(full, action=table, keep=530)      # 530 -> 547
        head.extend_kept_cache(short, action=table, keep=530)     # rewind
    torch.cuda.synchronize()
    print(f"route {route}: 11 extends of {B} x 17 rows (each after a rewind, which launches one comparison)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arm", choices=("run", "trace"))
    ap.add_argument("--route", choices=("chunk", "steps"), default="chunk")
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.arm == "run":
        return arm_run(a.rounds)
    if a.arm == "trace":
        return arm_trace(a.route)
    # (this process never opens the GPU; nothing more is started after a child that failed or ran out of time)
    r = subprocess.run(["timeout", "-k", "10", str(LIMIT_S), sys.executable, os.path.abspath(__file__), "--arm", "run", "--rounds", str(a.rounds)],
                       cwd=ROOT, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-4000:] + r.stderr[-4000:])
        raise SystemExit(f"the measurement failed with exit status {r.returncode}")
    text = f"# python tools/kv_extend_bench.py --rounds {a.rounds}\n" + r.stdout
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
