"""Evaluation half of the reference's ``train_gpt.py`` on the MI355X engine (the training loop is out of scope):

    get_tokenizer             /root/reference/train_gpt.py:128-149
    generate_multiple_times   :152-191   t samples per trajectory, chunked by ``max_generate_batchsize``
    batch_forward             :194-195   chunked detokenize
    evaluate                  :321-512   full-clip tokenize -> ``model(**input).loss`` -> gather -> t x B repeated generation ->
                                         chunked detokenize -> clamp -> best-of-t frame metrics -> gather -> eval logs

Same names, arguments and op sequence as the reference, so the loop reads like the original; what differs:
  * ``accelerator`` is any object with ``device / num_processes / is_main_process / is_local_main_process / gather / unwrap_model /
    log`` -- ``ivideogpt_amd.parallel.LocalAccelerator`` (torch.distributed over RCCL, no ``accelerate`` dependency) or HF's
    ``Accelerator`` itself;
  * FVD needs the I3D detector's weights, which do not ship: ``args.use_fvd`` with an ``Evaluator(i3d=...)`` computes the features
    of the real and of all t * B generated clips on the device (ivideogpt_amd/i3d.py), gathers them and logs ``eval/fvd``
    (:341-355, :456-470, :495-497); without a detector it raises.  The LPIPS column needs the VGG-16 / LPIPS weights: with
    ``--lpips_vgg_path`` and ``--lpips_lin_path`` (``Evaluator(lpips=...)``) ``eval/lpips`` is computed on the device and
    gathered like the other three, without them it is NaN;
  * ``--use_eval_dataset`` feeds the loop from ``ivideogpt_amd.data.EvalDataLoader`` (the reference's ``EvalDataLoader`` after
    ``accelerator.prepare``, train_gpt.py:102-113) instead of synthetic clips;
  * GIF dumps (``imageio``) are not written; the ``eval/mse`` fallback of that branch is kept (:447-449).
The only collectives are the all-gathers of per-sample loss / metric rows (train_gpt.py:376, 476-479).
"""
import argparse
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def get_tokenizer(args):
    """train_gpt.py:128-149 (``ctx_vqgan`` only, as the reference: the plain ``vqgan`` branch raises there too).
    -> (tokenizer, size of the transformer's vocabulary: static + dynamic codes, + 2 with the frame-separator tokens)."""
    from ivideogpt_amd import CompressiveVQModel
    if args.vqgan_type != "ctx_vqgan":
        raise NotImplementedError(f"vqgan_type {args.vqgan_type!r}: only the compressive tokenizer is on the path")
    tok = CompressiveVQModel.from_pretrained(args.pretrained_model_name_or_path, subfolder=None, low_cpu_mem_usage=False).eval()
    had = tok.context_length
    if had != args.context_length:
        print(f"[Warning] pretrained context length of vq_model mismatch, change from {had} to {args.context_length}")
        tok.set_context_length(args.context_length)
    n_codes = tok.num_vq_embeddings + tok.num_dyn_embeddings
    return tok, n_codes + (2 if args.special_token else 0)


def generate_multiple_times(gen_times, accelerator, model, gen_input, actions, gen_kwargs, max_batch_size=None, verbose=False,
                            reward_prediction=False):
    """train_gpt.py:152-191: ``gen_times`` samples of every prompt row; one ``generate`` call carries ``max_batch_size // B`` copies
    of the B prompts (``max_batch_size`` None: one copy), so ``gen_times`` must be a multiple of that and ``max_batch_size`` of B
    (AssertionError otherwise, as the reference).  -> tokens [t * B, L], sample k of trajectory b at row k * B + b (the layout
    ``Evaluator`` expects); with ``reward_prediction`` also the rewards, concatenated the same way."""
    B = gen_input.shape[0]
    cap = B if max_batch_size is None or max_batch_size == 0 else max_batch_size
    copies, rest = divmod(cap, B)
    assert rest == 0, f"max_batch_size {cap} is not a multiple of the batch {B}"
    calls, rest = divmod(gen_times, copies)
    assert rest == 0, f"gen_times {gen_times} is not a multiple of the {copies} copies one call carries"
    net = accelerator.unwrap_model(model)
    prompts = gen_input.repeat(copies, 1)
    extra = dict(gen_kwargs, pad_token_id=50256)
    if actions is not None:
        extra["action"] = actions.repeat(copies, 1, 1)
    if reward_prediction:
        extra["return_reward"] = True
    if copies > 1 and getattr(net, "supports_shared_context", False):
        extra["shared_context"] = copies   # rows k * B + b repeat prompt b: prefilled once, its K / V rows kept once (ivg_generate_shared)
    tokens, rewards = [], []
    for _ in range(calls):
        out = net.generate(prompts, **extra)
        if reward_prediction:
            tokens.append(out[0]); rewards.append(out[1])
        else:
            tokens.append(out)
    tokens = torch.cat(tokens, dim=0)
    return (tokens, torch.cat(rewards, dim=0)) if reward_prediction else tokens


def batch_forward(batch_size, input, forward, verbose=False):
    """train_gpt.py:194-195: ``forward`` over consecutive slices of ``batch_size`` rows, results concatenated."""
    pieces = [forward(input[lo: lo + batch_size]) for lo in range(0, input.shape[0], batch_size)]
    return torch.cat(pieces, dim=0)


def _prompt_and_budget(args, tokens):
    """The context part of a tokenized clip and the number of tokens a rollout adds (train_gpt.py:392-403): 256 tokens per context
    frame and 16 per predicted frame, one more of each with the frame-separator tokens (the last separator is not generated)."""
    sep = 1 if args.special_token else 0
    n_future = args.segment_length - args.context_length
    return tokens[:, :args.context_length * (256 + sep)], (16 + sep) * n_future - sep


@torch.no_grad()
def evaluate(args, accelerator, tokenizer, model, eval_dataloader, evaluator, completed_steps):
    """train_gpt.py:321-512.  ``eval_dataloader`` yields ``pixel_values [B, T, 3, H, W]`` in [0, 1] (or ``(pixel_values, actions)``
    when ``args.action_conditioned``).  Returns the eval logs on the main process, None elsewhere."""
    use_fvd = getattr(args, "use_fvd", False)
    scorer = accelerator.unwrap_model(evaluator) if use_fvd else None
    if use_fvd and getattr(scorer, "i3d", None) is None:
        raise NotImplementedError("FVD needs the I3D detector weights, which do not ship with the reference: Evaluator(i3d=...)")
    tok, net = accelerator.unwrap_model(tokenizer), accelerator.unwrap_model(model)
    dev, ctx = accelerator.device, args.context_length
    rows = {k: [] for k in ("loss", "mse", "psnr", "ssim", "lpips")}   # per-sample values, gathered over the ranks batch by batch

    def keep(name, value, n):
        rows[name].append(accelerator.gather(value.repeat(n)))

    from ivideogpt_amd.metrics import FeatureStats
    real_feats, gen_feats = FeatureStats(capture_mean_cov=True), FeatureStats(capture_mean_cov=True)

    def keep_features(stats, clips):
        # :341-355 / :456-470: detector features chunked by max_decode_batchsize, gathered, accumulated on the main process
        chunk = args.max_decode_batchsize
        feats = batch_forward(chunk, clips, scorer.i3d_features) if chunk is not None and clips.shape[0] > chunk else scorer.i3d_features(clips)
        feats = accelerator.gather(feats)
        if accelerator.is_main_process:
            stats.append_torch(feats)

    for it, batch in enumerate(eval_dataloader):
        if it == args.max_eval_iters:
            break
        frames, actions = batch if args.action_conditioned else (batch, None)
        frames = frames.to(dev, non_blocking=True)
        actions = actions.to(dev, non_blocking=True) if actions is not None else None
        n = frames.shape[0]
        if use_fvd:
            keep_features(real_feats, frames)

        # teacher-forced loss over the whole clip (:356-376)
        tokens, labels = tok.tokenize(frames, ctx)
        fwd = dict(input_ids=tokens, labels=labels)
        if actions is not None:
            fwd["action"] = actions
        out = net(**fwd)
        keep("loss", (out[0] if args.reward_prediction else out).loss, n)

        # rollout from the context frames, t samples per trajectory, decoded back to pixels (:390-430)
        show = it % args.log_gif_interval == 0 and accelerator.is_main_process
        recon = None
        if show or args.use_frame_metrics or use_fvd:
            prompt, budget = _prompt_and_budget(args, tokens)
            sampled = generate_multiple_times(args.eval_generate_times, accelerator, model, prompt, actions,
                                              gen_kwargs=dict(do_sample=True, temperature=1.0, top_k=100, max_new_tokens=budget),
                                              max_batch_size=args.max_generate_batchsize, reward_prediction=args.reward_prediction)
            sampled = sampled[0] if args.reward_prediction else sampled       # prompt included
            if args.eval_generate_times > 1 and getattr(tok, "supports_shared_context", False):
                decode = lambda ids: tok.detokenize(ids, ctx, shared_context="auto")   # the samples of a clip share its context: decoded once per clip
            else:
                decode = lambda ids: tok.detokenize(ids, ctx)
            chunk = args.max_decode_batchsize
            recon = batch_forward(chunk, sampled, decode) if chunk is not None and sampled.shape[0] > chunk else decode(sampled)
            recon = recon.clamp(0.0, 1.0)

        if use_fvd:
            keep_features(gen_feats, recon)

        if args.use_frame_metrics:
            # the ground truth is clamped too: resized frames overshoot 1.0 by an ulp (:470-471)
            for name, value in zip(("mse", "psnr", "ssim", "lpips"), evaluator(frames.clamp(0.0, 1.0), recon)):
                keep(name, value, n)
        elif show:   # no metric pass: the plain pixel MSE of the shown batch stands in for eval/mse (:447-449), not gathered
            assert recon.shape[0] == n, "the fallback compares one sample per trajectory"
            rows["mse"].append(((frames.float() - recon) ** 2).mean().repeat(n))

    if not accelerator.is_main_process:
        return None
    mean = lambda name: torch.cat(rows[name], 0).mean().item() if rows[name] else float("nan")
    eval_loss = mean("loss")
    try:
        perplexity = math.exp(eval_loss)
    except OverflowError:
        perplexity = float("inf")
    eval_logs = {"eval/eval_loss": eval_loss, "eval/perplexity": perplexity, "eval/mse": mean("mse")}
    if args.use_frame_metrics:
        eval_logs.update({f"eval/{k}": mean(k) for k in ("psnr", "ssim", "lpips")})
    if use_fvd:
        eval_logs["eval/fvd"] = scorer.compute_fvd(real_feats, gen_feats)
    accelerator.log(eval_logs, step=completed_steps)
    return eval_logs


def eval_args(**overrides):
    """The subset of the reference's ``parse_args`` the eval loop reads, with its defaults (train_gpt.py:198-318)."""
    d = dict(action_conditioned=False, reward_prediction=False, use_fvd=False, use_frame_metrics=True, special_token=True, context_length=2,
             segment_length=16, eval_generate_times=1, max_generate_batchsize=None, max_decode_batchsize=None, max_eval_iters=100,
             log_gif_interval=10, vqgan_type="ctx_vqgan", pretrained_model_name_or_path=None, output_dir="eval-out")
    d.update(overrides)
    return argparse.Namespace(**d)


def build_eval_model(a, vocab, dev):
    """The transformer of a ``--use_eval_dataset`` run, built as inference/predict.py builds it (reference train_gpt.py:597-616): the
    checkpoint of ``--pretrained_transformer_path`` (a directory with config.json + model.safetensors), else ``transformer/`` under
    ``--pretrained_model_name_or_path``, else seeded random weights; with ``--action_conditioned`` a ``HeadModelWithAction`` with the
    reference's prelude ((256 + 1) * context - 1) and token counts (16 per predicted frame)."""
    from ivideogpt_amd import HeadModelWithAction, LlamaForCausalLM, weights as W
    if a.pretrained_transformer_path:
        cfg, state = W.load_transformer_checkpoint(a.pretrained_transformer_path, None)
    elif a.pretrained_model_name_or_path:
        cfg, state = W.load_transformer_checkpoint(a.pretrained_model_name_or_path, "transformer")
    else:
        cfg, state = dict(W.LLAMA_SMALL), None
    assert cfg["vocab_size"] == vocab, f"the transformer's vocabulary ({cfg['vocab_size']}) is not the tokenizer's ({vocab})"   # predict.py:113
    if not a.action_conditioned:
        if state is None:
            state = W.random_llama_state_dict(cfg, 0)
        W.validate_state_dict(state, W.llama_param_shapes(cfg), "transformer")
        return LlamaForCausalLM(cfg, state).to(dev)
    if state is None:
        state = W.random_llama_state_dict(cfg, 0, action_dim=a.action_dim, reward_prediction=a.reward_prediction)
    model = HeadModelWithAction(LlamaForCausalLM.from_config(cfg), action_dim=a.action_dim, prelude_tokens_num=(256 + 1) * a.context_length - 1,
                                tokens_num_per_dyna=16, context=a.context_length, segment_length=a.segment_length,
                                reward_prediction=a.reward_prediction).to(dev)
    model.load_state_dict(state, strict=True)
    return model


def main(argv=None):
    """``python train_gpt.py --eval_only``-style entry; every rank evaluates its shard of the batches, rank 0 prints the logs as one
    JSON line.  Default: synthetic clips and seeded random weights.  ``--use_eval_dataset``: the test set of ``--dataset_name`` (a
    directory of per-episode ``.npz`` files, ``--dataset_root`` or the entry of ``--dataset_yaml``) through
    ``ivideogpt_amd.data.EvalDataLoader(device='cuda')``, the reference's flag names (train_gpt.py:198-318); the line then also
    carries ``eval/samples`` (rows that entered the means, over all ranks, wrapped duplicates included) and ``eval/batches``
    (iterations per rank)."""
    import json
    from ivideogpt_amd import CompressiveVQModel, LlamaForCausalLM, parallel, weights as W
    from ivideogpt_amd.metrics import Evaluator
    ap = argparse.ArgumentParser()
    ap.add_argument("--pretrained_model_name_or_path", default=None, help="checkpoint directory (tokenizer/ + transformer/); default: seeded random weights")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--segment_length", type=int, default=16)
    ap.add_argument("--context_length", type=int, default=2)
    ap.add_argument("--eval_generate_times", type=int, default=2)
    ap.add_argument("--max_generate_batchsize", type=int, default=None)
    ap.add_argument("--max_decode_batchsize", type=int, default=None)
    ap.add_argument("--lpips_vgg_path", default=None, help="torchvision vgg16 weights (features.N.* keys; .pth or .safetensors)")
    ap.add_argument("--lpips_lin_path", default=None, help="the lpips package's vgg.pth (lin{k}.model.1.weight); both paths: eval/lpips is real")
    ap.add_argument("--use_fvd", action="store_true", help="log eval/fvd (needs --i3d_path or --i3d_random)")
    ap.add_argument("--i3d_path", default=None, help="the I3D detector: the torchscript file of the reference, or a state-dict file")
    ap.add_argument("--i3d_random", type=int, default=None, metavar="SEED", help="seeded random I3D weights (synthetic runs)")
    ap.add_argument("--i3d_width_div", type=int, default=1, help="with --i3d_random: divide every width of the detector (quick runs)")
    ap.add_argument("--i3d_resize", type=int, default=224, help="side the detector resizes frames to (a multiple of 32)")
    ap.add_argument("--use_eval_dataset", action="store_true", help="evaluate on the test episodes of --dataset_name instead of synthetic clips")
    ap.add_argument("--dataset_name", default=None, help="bair_robot_pushing, tfds_robonet, vp2_robodesk, vp2_robosuite (any known name with --dataset_root)")
    ap.add_argument("--dataset_root", default=None, help="directory of the test episodes (*.npz); default: the entry of --dataset_yaml")
    ap.add_argument("--dataset_yaml", default="DATASET.yaml", help="the reference's DATASET.yaml (bair_test_dataset, robonet_test_dataset, ...)")
    ap.add_argument("--resolution", type=int, default=None, help="frame side; default (and only accepted value): the tokenizer's")
    ap.add_argument("--per_device_eval_batch_size", type=int, default=None, help="default: --batch")
    ap.add_argument("--dataloader_num_workers", type=int, default=4, help="reader threads of the loader (at most 16)")
    ap.add_argument("--max_eval_iters", type=int, default=100)
    ap.add_argument("--action_conditioned", action="store_true", help="HeadModelWithAction checkpoint + the episodes' actions")
    ap.add_argument("--action_dim", type=int, default=4)
    ap.add_argument("--reward_prediction", action="store_true")
    ap.add_argument("--use_frame_metrics", action="store_true", help="with --use_eval_dataset: log mse / psnr / ssim / lpips (the synthetic run always does)")
    ap.add_argument("--pretrained_transformer_path", default=None, help="directory of the transformer checkpoint (config.json + model.safetensors)")
    ap.add_argument("--seed", type=int, default=None, help="seeds python / numpy / torch (+ rank, as accelerate's device_specific set_seed)")
    a = ap.parse_args(argv)
    if bool(a.lpips_vgg_path) != bool(a.lpips_lin_path):
        ap.error("--lpips_vgg_path and --lpips_lin_path go together")
    if a.use_eval_dataset and not a.dataset_name:
        ap.error("--use_eval_dataset needs --dataset_name")
    if a.use_eval_dataset and not a.use_frame_metrics and not a.use_fvd and a.eval_generate_times != 1:
        ap.error("without --use_frame_metrics the loop compares one sample per trajectory (its eval/mse fallback): --eval_generate_times 1")
    rank, world, local = parallel.init_from_env()
    dev = torch.device("cuda", local)
    torch.cuda.set_device(dev)
    if a.seed is not None:
        import random
        import numpy as np
        for seeder in (random.seed, np.random.seed, torch.manual_seed, torch.cuda.manual_seed_all):
            seeder(a.seed + rank)
    if a.pretrained_model_name_or_path:
        tok = CompressiveVQModel.from_pretrained(a.pretrained_model_name_or_path, subfolder="tokenizer").to(dev)
    else:
        tcfg = W.tokenizer_config(**W.CTX_VAE64)
        tok = CompressiveVQModel(tcfg, W.random_tokenizer_state_dict(tcfg, 0, codebook_std=0.4)).to(dev)
    if a.context_length != tok.context_length:
        tok.set_context_length(a.context_length)
    res = tok.config["resolution"]
    args = eval_args(context_length=a.context_length, segment_length=a.segment_length, eval_generate_times=a.eval_generate_times,
                     max_generate_batchsize=a.max_generate_batchsize, max_decode_batchsize=a.max_decode_batchsize, use_fvd=a.use_fvd)
    if a.use_eval_dataset:
        from ivideogpt_amd.data import EvalDataLoader
        if a.resolution not in (None, res):
            ap.error(f"--resolution {a.resolution}: the tokenizer works at {res}")
        llm = build_eval_model(a, tok.num_vq_embeddings + tok.num_dyn_embeddings + 2, dev)
        batches = EvalDataLoader(a.dataset_name, a.segment_length, res, batch_size=a.per_device_eval_batch_size or a.batch,
                                 num_workers=a.dataloader_num_workers, load_action=a.action_conditioned, device=dev, rank=rank, world=world,
                                 root=a.dataset_root, dataset_yaml=a.dataset_yaml)
        vars(args).update(action_conditioned=a.action_conditioned, reward_prediction=a.reward_prediction, use_frame_metrics=a.use_frame_metrics,
                          max_eval_iters=a.max_eval_iters)
    else:
        if a.pretrained_model_name_or_path:
            llm = LlamaForCausalLM.from_pretrained(a.pretrained_model_name_or_path, subfolder="transformer").to(dev)
        else:
            llm = LlamaForCausalLM(dict(W.LLAMA_SMALL), W.random_llama_state_dict(dict(W.LLAMA_SMALL), 0)).to(dev)
        g = torch.Generator().manual_seed(1234)
        batches = [torch.rand(a.batch, a.segment_length, 3, res, res, generator=g) for _ in range(a.iters * world)][rank::world]
    i3d = a.i3d_path
    if a.i3d_random is not None:
        from ivideogpt_amd.i3d import I3D
        i3d = I3D.from_state_dict(W.random_i3d_state_dict(a.i3d_random, a.i3d_width_div), resize=a.i3d_resize)
    elif i3d is not None:
        from ivideogpt_amd.i3d import I3D
        i3d = I3D.from_file(i3d, resize=a.i3d_resize)
    evaluator = Evaluator(lpips=(a.lpips_vgg_path, a.lpips_lin_path) if a.lpips_vgg_path else None, i3d=i3d)
    logs = evaluate(args, parallel.LocalAccelerator(dev), tok, llm, batches, evaluator, 0)
    if logs is not None:
        if a.use_eval_dataset:
            seen = batches.batches[:a.max_eval_iters] if a.max_eval_iters >= 0 else batches.batches
            logs["eval/samples"] = sum(len(b) for b in seen) * world     # with more than one rank every batch is full (data.shard_batches)
            logs["eval/batches"] = len(seen)
        print(json.dumps(logs))
    return logs


if __name__ == "__main__":
    main()
