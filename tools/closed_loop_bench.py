"""What the encoder's context cache buys a closed loop (ivg_tokenize_frames, EncodeCache, VideoPredictor.track): the observation of one
control step -- the new frame's tokens onto the transformer's kept cache -- three ways, and the whole step with a plan.  Development
tool; bench.py is the contract and does not know the feature.  Prints a text report (profiles/closed_loop.txt is one).

    python tools/closed_loop_bench.py [--out REPORT] [--rounds N]     the measurement, in a child process under a time limit
    python tools/closed_loop_bench.py --arm run [--rounds N]          the measurement itself

BASELINE config 2's models with seeded weights: the full-width ctx_vae64 tokenizer (fp32 encoder, bf16 decoder) and Llama-small in
bf16 under the action wrapper with a reward head, ctx = 2, 64 x 64 frames.  B = 16 and B = 64 tracked histories, after 0 and after 12
observed frames.  Arms ALTERNATE round by round in one process, HIP events around each, medians; two warm-up rounds.  After every
timed arm the session and the kept cache are put back (an untimed rewind), so every arm starts from the same state.
  (1) tracked       TrackedEpisode.observe: tokenize_frames against the encoder cache + extend_kept_cache
  (2) re-encode     tokenize(cat(context, frame)) + extend_kept_cache: the best a caller has without the encoder cache (the plain
                    encoder over the ctx context frames and the K / V projections again at every step)
  (3) from scratch  that tokenize + a prompt pass over the whole grown row (generate of one token)
The ids of (1) and (2) are compared (an fp32 encoder: equal bit for bit).
Whole step: observe + plan with 16 candidates of 4 frames per history (one fan_out, one detokenize), at 8 histories -- the K / V cache
holds 128 trajectories per chunk, which bounds histories x candidates."""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CTX, BATCHES, AT_STEPS = 2, (16, 64), (0, 12)
PLAN_B, CAND, HORIZON = 8, 16, 4
LIMIT_S = 900


def make_predictor():
    import torch
    from ivideogpt_amd import CompressiveVQModel, HeadModelWithAction, LlamaForCausalLM, weights as W
    from mbrl.video_predictor import VideoPredictor
    dev = torch.device("cuda:0")
    tcfg = W.tokenizer_config(**W.CTX_VAE64)
    tok = CompressiveVQModel(tcfg, W.random_tokenizer_state_dict(tcfg, seed=0, codebook_std=0.4), encode_dtype="fp32", decode_dtype="bf16").to(dev)
    cfg = dict(W.LLAMA_SMALL)
    head = HeadModelWithAction(LlamaForCausalLM(cfg, None, dtype="bf16"), 4, 257 * CTX - 1, 16, CTX, 32, reward_prediction=True)
    head.load_state_dict(W.random_llama_state_dict(cfg, 2, action_dim=4, reward_prediction=True), strict=True)
    head.to(dev)
    return VideoPredictor.from_models(tok, head, context_length=CTX, symlog=True, device=dev)


def timed(f):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    r = f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), r


def line(name, ts):
    m = statistics.median(ts)
    return f"  {name:<46s}{m:8.3f} ms (min {min(ts):.3f}, max {max(ts):.3f})", m


class Snapshot:
    """The session's host state, and the rewind that makes the kept cache match it again."""

    def __init__(self, trk):
        self.trk, self.state = trk, (trk.tokens, trk.table, trk.steps, list(trk.stack))

    def restore(self):
        t = self.trk
        t.tokens, t.table, t.steps, t.stack = self.state[0], self.state[1], self.state[2], list(self.state[3])
        t.p.model.extend_kept_cache(t.tokens, action=t.table, keep=t.tokens.shape[1] - 1)


def measure_observe(vp, B, at_steps, rounds, gen):
    import torch
    dev, tok, model = vp.device, vp.tokenizer, vp.model
    obs = torch.randint(0, 256, (B, 9, 64, 64), generator=gen).float()
    trk = vp.track(obs)
    for _ in range(at_steps):
        trk.observe(torch.randint(0, 256, (B, 3, 64, 64), generator=gen).float(), torch.randn(B, 4, generator=gen))
    frame = torch.randint(0, 256, (B, 3, 64, 64), generator=gen).float().to(dev)
    action = torch.randn(B, 4, generator=gen).to(dev)
    ctx_px = trk.enc_cache.pixels                       # the frames the session is anchored at
    snap = Snapshot(trk)
    sdf = torch.full((B, 1), model.token_for_sdf, dtype=torch.int64, device=dev)
    table = trk.table.clone()
    table[:, trk.steps + CTX - 1] = action
    L = trk.tokens.shape[1]

    def tracked():
        return trk.observe(frame, action)

    def reencode_ids():
        clip = torch.cat([ctx_px, frame[:, None] / 255.], 1)
        return torch.cat([trk.tokens, tok.tokenize(clip, CTX)[0][:, 257 * CTX:], sdf], 1)

    def reencode():
        return model.extend_kept_cache(reencode_ids(), action=table, keep=L - 1, return_nll=True)[:, :16].sum(1)

    def scratch():
        return model.generate(reencode_ids(), do_sample=False, max_new_tokens=1, action=table)

    t1, t2, t3 = [], [], []
    for r in range(rounds + 2):                         # two warm-up rounds (workspaces, one-time kernel set-up of every shape)
        a_ms, s1 = timed(tracked)
        ids1 = trk.tokens
        snap.restore()
        b_ms, s2 = timed(reencode)
        snap.restore()
        c_ms, _ = timed(scratch)
        snap.restore()
        if r >= 2:
            t1.append(a_ms); t2.append(b_ms); t3.append(c_ms)
    same = bool(torch.equal(ids1, reencode_ids())) and bool(torch.equal(s1, s2))
    print(f"B = {B}, {at_steps} frames observed before (kept cache {L - 1} positions): ids and surprise of (1) == (2) bit for bit: {same}")
    l1, m1 = line("(1) tokenize_frames + extend_kept_cache", t1)
    l2, m2 = line("(2) tokenize(context + frame) + extend", t2)
    l3, m3 = line("(3) tokenize(context + frame) + prompt pass", t3)
    print(l1); print(l2); print(l3)
    print(f"      (1) is {m2 / m1:.2f} x {'faster' if m1 < m2 else 'SLOWER'} than (2) and {m3 / m1:.2f} x {'faster' if m1 < m3 else 'SLOWER'} than (3)")
    return m1, m2, m3


def measure_step(vp, rounds, gen):
    import torch
    B = PLAN_B
    obs = torch.randint(0, 256, (B, 9, 64, 64), generator=gen).float()
    trk = vp.track(obs)
    frame = torch.randint(0, 256, (B, 3, 64, 64), generator=gen).float().to(vp.device)
    action = torch.randn(B, 4, generator=gen).to(vp.device)
    plans = torch.randn(B * CAND, HORIZON, 4, generator=gen).to(vp.device)
    uni = torch.rand(B * CAND, 17 * HORIZON - 1, generator=gen).to(vp.device)
    trk.plan(plans, samples=CAND, uniforms=uni)         # (the engine grows to the candidates' rows once, outside the timed window)
    snap = Snapshot(trk)

    def step():
        s = trk.observe(frame, action)
        return s, trk.plan(plans, samples=CAND, uniforms=uni)

    def plan_only():
        return trk.plan(plans, samples=CAND, uniforms=uni)

    ta, tb = [], []
    for r in range(rounds + 2):
        a_ms, _ = timed(step)
        snap.restore()
        b_ms, _ = timed(plan_only)
        if r >= 2:
            ta.append(a_ms); tb.append(b_ms)
    print(f"# whole control step: {B} histories, observe + plan of {CAND} candidates x {HORIZON} frames (fan_out, {B * CAND} rows; detokenize of {B * CAND * HORIZON} frames)")
    print(line("observe + plan", ta)[0])
    print(line("plan alone (one frame earlier)", tb)[0])


def arm_run(rounds):
    import torch
    vp = make_predictor()
    gen = torch.Generator().manual_seed(1)
    print(f"# {torch.cuda.get_device_name(0)}, ctx_vae64 full width (fp32 encoder, bf16 decoder) + Llama-small bf16, ctx {CTX}, 64 x 64 frames; "
          f"median of {rounds} alternating rounds (HIP events)")
    print("# the observation of one control step: one new frame per history onto the kept cache")
    worst = None
    for B in BATCHES:
        for k in AT_STEPS:
            m1, m2, _ = measure_observe(vp, B, k, rounds, gen)
            worst = m2 / m1 if worst is None else min(worst, m2 / m1)
    print(f"# (1) against (2), the smallest ratio over the four cases: {worst:.2f} x")
    measure_step(vp, rounds, gen)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arm", choices=("run",))
    ap.add_argument("--rounds", type=int, default=10)
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
    text = f"# python tools/closed_loop_bench.py --rounds {a.rounds}\n" + r.stdout
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
