"""The FP8 (e4m3) K / V cache against the untouched bf16 cache, same process, same GPU (development tool; bench.py is the contract and
does not know the format).  BASELINE config 2's transformer: Llama-small at released width with seeded weights, B = 64 trajectories,
514 prompt tokens, 237 new ones.  Prints a text report (profiles/kv8.txt is one).

  speed     one batch in flight, then four (replicas on their own streams and host threads, the batches-in-flight LDS budget): the two
            formats ALTERNATE round by round; per format the median over --rounds rounds of
              * the rollout (HIP events, one lane; host clock around the four joined lanes) and ms per decode step
                ((rollout - a rollout of one new token) / 236 for one lane; rollout / 237 per lane for four);
              * from the kernels' own stamps, in rounds of their own: us per attention launch and ivg_profile_attn_fit's line
                (fixed us per launch, streaming GB/s over the bytes of the format).
  accuracy  the golden clip (tests/golden/fractal_clip_seed0.npz) through a seeded released-width tokenizer as the prompt:
              * teacher-forced prefix + ONE decode step (generate_embeds: a prefill of 530 rows, then the grown prompt with reuse, so the
                last row goes through the decode-step kernels over the cache): hidden state of that step against the fp32 CPU oracle,
                for the FP8-cache engine and, beside it, the bf16-cache engine;
              * greedy and sampled rollouts: token agreement with the bf16-cache engine, first diverging step;
              * pixels after detokenize of both rollouts.
            Seeded weights give near-uniform attention and bounded activations: they understate what outliers in trained K / V do
            to an 8-bit format.  No pass bar: the op-level contract (tests/test_gpu_decode_attn8.py) is the bar.
  --calibrate  one more accuracy column (profiles/kv8_scales.txt): the same prefix + one decode step on a RESCALED twin of the model
            (per layer q_proj rows of head 0 x 2^-10, k_proj rows of head 0 x 2^10, v_proj rows of head 1 x 2^-12, o_proj columns of
            head 1 x 2^12: the same function, as tests/test_gpu_kv_scales.py checks) with the FP8 cache at scale 1 against the per-layer,
            per-head scales calibrate_kv_cache finds on the prefix, and the original model beside it.
"""
import argparse
import os
import statistics
import sys
import threading
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ivideogpt_amd import CompressiveVQModel, LlamaForCausalLM, _lib, weights as W  # noqa: E402

FORMATS = ("auto", "fp8_e4m3")
med = statistics.median


def timed(fn, stream=None):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record(stream)
    fn()
    e1.record(stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def stamps(model, fn):
    """one profiled call -> (us per attention launch, fixed us, GB/s, launches)."""
    eng = model._engine
    eng.profile_enable(_lib.IVG_K_DECODE_ATTN, True)
    fn()
    st = eng.profile_read(_lib.IVG_K_DECODE_ATTN)
    fixed, gbps = eng.profile_attn_fit()
    eng.profile_enable(_lib.IVG_K_DECODE_ATTN, False)
    return 1e3 * st["total_ms"] / max(1, st["launches"]), fixed, gbps, st["launches"]


def speed_one_lane(m, prompt, u, n_new, rounds, out):
    roll = lambda n: m.generate(prompt, do_sample=True, top_k=100, max_new_tokens=n, uniforms=u[:, :n])  # noqa: E731
    t = {f: dict(full=[], one=[], us=[], fixed=[], gbps=[]) for f in FORMATS}
    for f in FORMATS:   # warm every shape and both formats (engine, workspace, one-time kernel attributes)
        m.set_kv_cache_dtype(f)
        roll(n_new), roll(1)
    for _ in range(rounds):
        for f in FORMATS:
            m.set_kv_cache_dtype(f)
            t[f]["full"].append(timed(lambda: roll(n_new)))
            t[f]["one"].append(timed(lambda: roll(1)))
    for _ in range(rounds):
        for f in FORMATS:
            m.set_kv_cache_dtype(f)
            us, fixed, gbps, n = stamps(m, lambda: roll(n_new))
            t[f]["us"].append(us), t[f]["fixed"].append(fixed), t[f]["gbps"].append(gbps)
            t[f]["launches"] = n
    out.append(f"one batch in flight (B = {prompt.shape[0]}, {prompt.shape[1]} + {n_new} tokens, median of {rounds} alternating rounds):")
    for f in FORMATS:
        r = t[f]
        step = (med(r["full"]) - med(r["one"])) / (n_new - 1)
        out.append(f"  {f:9s} rollout {med(r['full']):8.2f} ms (min {min(r['full']):.2f}, max {max(r['full']):.2f})   prefill + 1 token {med(r['one']):7.2f} ms   "
                   f"{step:.4f} ms per decode step")
        out.append(f"  {f:9s} attention: {med(r['us']):6.2f} us per launch over {r['launches']} launches (min {min(r['us']):.2f}, max {max(r['us']):.2f});  "
                   f"fit: fixed {med(r['fixed']):.2f} us + bytes / {med(r['gbps']):.0f} GB/s")
    return t


def speed_lanes(m, prompt, u, n_new, rounds, n_lanes, out):
    dev = prompt.device
    models = [m] + [m.replica() for _ in range(n_lanes - 1)]
    streams = [torch.cuda.Stream(device=dev) for _ in range(n_lanes)]
    for x in models:
        x.set_decode_lds_kb(LlamaForCausalLM.BATCHES_IN_FLIGHT_LDS_KB)

    def round_(profile=False):
        res = [None] * n_lanes

        def body(i):
            torch.cuda.set_device(dev)
            with torch.cuda.stream(streams[i]):
                fn = lambda: models[i].generate(prompt, do_sample=True, top_k=100, max_new_tokens=n_new, uniforms=u)  # noqa: E731
                res[i] = stamps(models[i], fn) if profile else fn()
                streams[i].synchronize()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ths = [threading.Thread(target=body, args=(i,)) for i in range(n_lanes)]
        [th.start() for th in ths], [th.join() for th in ths]
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, res

    t = {f: dict(ms=[], us=[], fixed=[], gbps=[]) for f in FORMATS}
    for f in FORMATS:
        [x.set_kv_cache_dtype(f) for x in models]
        round_(), round_()
    for _ in range(rounds):
        for f in FORMATS:
            [x.set_kv_cache_dtype(f) for x in models]
            t[f]["ms"].append(round_()[0])
    for _ in range(rounds):
        for f in FORMATS:
            [x.set_kv_cache_dtype(f) for x in models]
            res = round_(profile=True)[1]
            t[f]["us"].append(med([r[0] for r in res])), t[f]["fixed"].append(med([r[1] for r in res])), t[f]["gbps"].append(med([r[2] for r in res]))
    out.append(f"{n_lanes} batches in flight (each B = {prompt.shape[0]}, decode_lds_kb {LlamaForCausalLM.BATCHES_IN_FLIGHT_LDS_KB}; host clock around the joined "
               f"lanes, median of {rounds} alternating rounds):")
    for f in FORMATS:
        r = t[f]
        out.append(f"  {f:9s} {n_lanes} rollouts {med(r['ms']):8.2f} ms (min {min(r['ms']):.2f}, max {max(r['ms']):.2f})   {med(r['ms']) / n_new:.4f} ms per decode step of "
                   f"a lane   {med(r['ms']) / n_new / n_lanes:.4f} ms per step and batch")
        out.append(f"  {f:9s} attention (per lane, the others running): {med(r['us']):6.2f} us per launch;  fit: fixed {med(r['fixed']):.2f} us + bytes / "
                   f"{med(r['gbps']):.0f} GB/s")
    for x in models:
        x.set_decode_lds_kb(0)
        x.set_kv_cache_dtype("auto")
    return t


def accuracy(m, cfg, sd, dev, out, n_new):
    from oracle.llama import LlamaRef
    clip = torch.from_numpy(np.load(os.path.join(ROOT, "tests", "golden", "fractal_clip_seed0.npz"))["clip"])[None]   # (1, 16, 3, 64, 64)
    tcfg = W.tokenizer_config(**W.CTX_VAE64)
    tok = CompressiveVQModel(tcfg, W.random_tokenizer_state_dict(tcfg, 0, 0.4), encode_dtype="fp32", decode_dtype="bf16").to(dev)
    ctx = tcfg["context_length"]
    ids, _ = tok.tokenize(clip.to(dev), ctx)                       # the clip's own tokens: 257 * ctx - 1 + 17 * 14
    ids = ids.cpu()
    # ---- teacher-forced prefix + one decode step
    L = 257 * ctx + 16                                             # two context frames + the first predicted one (530 rows), then its sdf
    seq = torch.cat([ids[:, :L], torch.full((1, 1), cfg["vocab_size"] - 1, dtype=torch.int64)], 1)
    ora = LlamaRef(sd, cfg["num_hidden_layers"], cfg["num_attention_heads"], cfg["rms_norm_eps"], cfg["rope_theta"], cfg["max_position_embeddings"])
    ref = ora.forward_embeds(ora.embed(seq), return_hidden=True)[2][:, -1].double()
    emb = m.get_input_embeddings()(seq.to(dev))
    out.append(f"teacher-forced prefix of {L} golden-clip tokens + one decode step: hidden state (post final norm) against the fp32 CPU oracle "
               f"(|oracle| max {ref.abs().max():.3f}, rms {ref.pow(2).mean().sqrt():.3f}):")
    for f in FORMATS:
        m.set_kv_cache_dtype(f)
        m.generate(inputs_embeds=emb[:, :L], do_sample=False, max_new_tokens=1)
        r = m.generate(inputs_embeds=emb, do_sample=False, max_new_tokens=1, return_dict_in_generate=True, output_hidden_states=True)
        assert m.last_generate_reused_cache, "the decode step did not run over the kept cache"
        d = (r.hidden_states[-1][-1][:, 0].double().cpu() - ref).abs()
        out.append(f"  {f:9s} max abs deviation {d.max():.4e}   rms {d.pow(2).mean().sqrt():.4e}")
    # ---- rollouts from the clip's context
    B = 8
    prompt = ids[:, :257 * ctx].repeat(B, 1).to(dev)
    u = torch.rand(B, n_new, generator=torch.Generator().manual_seed(2)).to(dev)
    roll = {}
    for f in FORMATS:
        m.set_kv_cache_dtype(f)
        roll[f] = (m.generate(prompt[:1], do_sample=False, max_new_tokens=n_new), m.generate(prompt, do_sample=True, top_k=100, max_new_tokens=n_new, uniforms=u))
    L0 = prompt.shape[1]
    for k, name in ((0, "greedy (1 row)"), (1, f"sampled (top-k 100, {B} rows, one uniform table)")):
        a, b = roll["auto"][k][:, L0:].cpu(), roll["fp8_e4m3"][k][:, L0:].cpu()
        first = [int((a[i] != b[i]).nonzero()[0]) + 1 if (a[i] != b[i]).any() else None for i in range(a.shape[0])]
        out.append(f"rollout of {n_new} tokens, {name}: {(a == b).float().mean():.4f} of the tokens equal the bf16-cache engine's; first diverging new token per row: {first}")
    px = {f: tok.detokenize(roll[f][1], ctx).float().clamp(0, 1).cpu() for f in FORMATS}
    d = (px["auto"][:, ctx:] - px["fp8_e4m3"][:, ctx:]).abs()
    same = (roll["auto"][1] == roll["fp8_e4m3"][1]).all(1).cpu()
    out.append(f"pixels of the {B} sampled rollouts after detokenize (predicted frames, clamped to [0, 1]): mean abs deviation {d.mean():.4e}, max {d.max():.4e} "
               f"({int(same.sum())} of {B} rows have identical tokens; a row that diverged is another sample, not a perturbed one)")
    m.set_kv_cache_dtype("auto")


def rescaled_twin(sd, layers):
    tw = {k: v.clone() for k, v in sd.items()}
    for l in range(layers):
        pre = f"model.layers.{l}.self_attn."
        tw[pre + "q_proj.weight"][0:64] *= 2.0 ** -10
        tw[pre + "k_proj.weight"][0:64] *= 2.0 ** 10
        tw[pre + "v_proj.weight"][64:128] *= 2.0 ** -12
        tw[pre + "o_proj.weight"][:, 64:128] *= 2.0 ** 12
    return tw


def calibrate_column(m, cfg, sd, dev, out):
    from oracle.llama import LlamaRef
    clip = torch.from_numpy(np.load(os.path.join(ROOT, "tests", "golden", "fractal_clip_seed0.npz"))["clip"])[None]
    tcfg = W.tokenizer_config(**W.CTX_VAE64)
    tok = CompressiveVQModel(tcfg, W.random_tokenizer_state_dict(tcfg, 0, 0.4), encode_dtype="fp32", decode_dtype="bf16").to(dev)
    ctx = tcfg["context_length"]
    ids = tok.tokenize(clip.to(dev), ctx)[0].cpu()
    L = 257 * ctx + 16
    seq = torch.cat([ids[:, :L], torch.full((1, 1), cfg["vocab_size"] - 1, dtype=torch.int64)], 1)
    ora = LlamaRef(sd, cfg["num_hidden_layers"], cfg["num_attention_heads"], cfg["rms_norm_eps"], cfg["rope_theta"], cfg["max_position_embeddings"])
    ref = ora.forward_embeds(ora.embed(seq), return_hidden=True)[2][:, -1].double()
    twin = LlamaForCausalLM(cfg, rescaled_twin(sd, cfg["num_hidden_layers"]), dtype="bf16").to(dev)
    out.append(f"--calibrate: teacher-forced prefix of {L} golden-clip tokens + one decode step, hidden state against the fp32 CPU oracle of the original "
               f"model; scales calibrated on the {L + 1} tokens (headroom 1):")
    for name, model in (("original", m), ("rescaled twin", twin)):
        emb = model.get_input_embeddings()(seq.to(dev))
        model.set_kv_cache_dtype("auto")
        tab = model.calibrate_kv_cache(seq.to(dev))
        lg = torch.log2(tab)
        for what, kw in (("bf16 cache", dict(name="auto")), ("fp8, scale 1", dict(name="fp8_e4m3")), ("fp8, calibrated", dict(name="fp8_e4m3", scales=tab))):
            model.set_kv_cache_dtype(**kw)
            model.generate(inputs_embeds=emb[:, :L], do_sample=False, max_new_tokens=1)
            r = model.generate(inputs_embeds=emb, do_sample=False, max_new_tokens=1, return_dict_in_generate=True, output_hidden_states=True)
            assert model.last_generate_reused_cache, "the decode step did not run over the kept cache"
            d = (r.hidden_states[-1][-1][:, 0].double().cpu() - ref).abs()
            out.append(f"  {name:13s} {what:15s} max abs deviation {d.max():.4e}   rms {d.pow(2).mean().sqrt():.4e}")
        out.append(f"  {name:13s} log2 of the calibrated scales: K min {int(lg[:, 0].min())} max {int(lg[:, 0].max())} (head 0: {int(lg[:, 0, 0].min())} .. {int(lg[:, 0, 0].max())});  "
                   f"V min {int(lg[:, 1].min())} max {int(lg[:, 1].max())} (head 1: {int(lg[:, 1, 1].min())} .. {int(lg[:, 1, 1].max())})")
        model.set_kv_cache_dtype("auto")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--lanes", type=int, default=4)
    ap.add_argument("--skip", default="", help="comma list of speed1, speed4, accuracy")
    ap.add_argument("--calibrate", action="store_true", help="add the calibrated-scales accuracy column (rescaled twin of the model)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert a.rounds >= 1
    dev = torch.device("cuda:0")
    cfg = dict(W.LLAMA_SMALL)
    sd = W.random_llama_state_dict(cfg, 0)
    m = LlamaForCausalLM(cfg, sd, dtype="bf16").to(dev)
    gen = torch.Generator().manual_seed(1)
    L0, n_new = 514, 17 * 14 - 1
    prompt = torch.randint(0, 8192, (a.batch, L0), generator=gen)
    prompt[:, 256], prompt[:, -1] = cfg["vocab_size"] - 2, cfg["vocab_size"] - 1
    prompt = prompt.to(dev)
    u = torch.rand(a.batch, n_new, generator=gen).to(dev)
    out = [f"# tools/kv8_bench.py --batch {a.batch} --rounds {a.rounds} --lanes {a.lanes}: Llama-small (12 x 768, head_dim 64) bf16, seeded weights; "
           f"K / V cache bf16 (\"auto\") against FP8 e4m3 (scales 1.0)", f"# {torch.cuda.get_device_name(0)}, GPU_MAX_HW_QUEUES={os.environ.get('GPU_MAX_HW_QUEUES', '(unset)')}"]
    skip = set(a.skip.split(","))
    if "speed1" not in skip:
        speed_one_lane(m, prompt, u, n_new, a.rounds, out)
    if "speed4" not in skip:
        speed_lanes(m, prompt, u, n_new, a.rounds, a.lanes, out)
    if "accuracy" not in skip:
        accuracy(m, cfg, sd, dev, out, n_new)
    if a.calibrate:
        calibrate_column(m, cfg, sd, dev, out)
    text = "\n".join(out)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
