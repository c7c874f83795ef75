"""Sparsified fine-tuning ("unlearning") of a pre-trained DDPM on one contributor coalition, then the
model-behaviour score - global (FID / IS / precision / recall, `--model_behavior global`) or local (per generated image
MSE / NRMSE / SSIM against the full model's image and the diffusion loss, `--model_behavior local`) - and one jsonl row.

Entry point kept from the reference (unconditional_generation/unlearn.py): same flags for the sFT path
(`--method gd` / `ga`), for influence unlearning (`--method iu`, `--iu_ratio`: :509-546 through
`gad.InfluenceUnlearner`) and for LoRA unlearning (`--method lora` / `lora_u`, `--lora_rank`, `--lora_dropout`: :404-424,
629-634, 748-749 through `gad.get_peft_model` / `gad.merge_and_unload`), same coalition semantics (the by_class quirk of :331 included), same jsonl keys
(:277,834-837,960-968).  The cycle itself is `gad.coalition.CoalitionEngine`: fused training steps,
EMA weights, 64-image preview, fused-batch DDIM sampling and the Frechet score on the MI355X.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

_HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

import src.constants as constants  # noqa: E402
from src.datasets import (create_dataset, remove_data_by_datamodel, remove_data_by_loo,  # noqa: E402
                          remove_data_by_shapley, remove_data_by_uniform, remove_data_for_aoi)
from src.diffusion_utils import (build_pipeline, dataset_config, generate_images, load_ckpt_model,  # noqa: E402
                                 local_behavior_row)
from src.utils import save_image_grid  # noqa: E402


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Training DDPM")
    p.add_argument("--load", type=str, default=None, help="directory of the pre-trained (pruned) model")
    p.add_argument("--dataset", type=str, default="mnist", choices=constants.DATASET + ["toy2"])
    p.add_argument("--excluded_class", type=str, default=None)
    p.add_argument("--removal_dist", type=str, default=None,
                   choices=["uniform", "datamodel", "shapley", "loo", "add_one_in"])
    p.add_argument("--datamodel_alpha", type=float, default=0.5)
    p.add_argument("--removal_seed", type=int, default=0)
    p.add_argument("--method", type=str, required=True, choices=constants.METHOD)
    p.add_argument("--iu_ratio", type=float, default=0.5)
    p.add_argument("--ga_ratio", type=float, default=1.0)
    p.add_argument("--gd_steps", type=int, default=4000)
    p.add_argument("--lora_rank", type=int, default=16)
    p.add_argument("--lora_dropout", type=float, default=0.05)
    p.add_argument("--opt_seed", type=int, default=42)
    p.add_argument("--outdir", type=str, default=constants.OUTDIR)
    p.add_argument("--gradient_accumulation_steps", type=int, default=1)
    p.add_argument("--db", type=str, required=True)
    p.add_argument("--reference_dir", type=str, default=None)
    p.add_argument("--batch_size", type=int, default=32)
    p.add_argument("--n_samples", type=int, default=10240)
    p.add_argument("--pruning_ratio", type=float, default=0.3)
    p.add_argument("--pruner", type=str, default="magnitude",
                   choices=["taylor", "random", "magnitude", "reinit", "diff-pruning"])
    p.add_argument("--thr", type=float, default=0.05)
    p.add_argument("--mixed_precision", type=str, default="no", choices=["no", "fp16", "bf16"])
    p.add_argument("--precompute_stage", type=str, default=None, choices=[None, "save", "reuse"])
    p.add_argument("--use_8bit_optimizer", default=False, action="store_true")
    p.add_argument("--ema_inv_gamma", type=float, default=1.0)
    p.add_argument("--ema_power", type=float, default=3 / 4)
    p.add_argument("--ema_max_decay", type=float, default=0.9999)
    p.add_argument("--model_behavior", type=str, default=None, choices=[None, "global", "local"])
    p.add_argument("--use_ema", default=False, action="store_true")
    p.add_argument("--exp_name", type=str, default=None)
    p.add_argument("--n_noises", type=int, default=50)
    p.add_argument("--num_inference_steps", type=int, default=100)
    p.add_argument("--num_train_steps", type=int, default=1000)
    p.add_argument("--trained_steps", type=int, default=None)
    p.add_argument("--device", type=str, default="cuda:0")
    return p.parse_args(argv)


def coalition(args, dataset):
    d = args.removal_dist
    if d == "uniform":
        return remove_data_by_uniform(dataset, seed=args.removal_seed, by_class=True)   # TypeError, as :323-325
    if d == "datamodel":
        return remove_data_by_datamodel(dataset, alpha=args.datamodel_alpha, seed=args.removal_seed, by_class=True)
    if d == "shapley":
        # `if args.dataset == "cifar100" or "celeba":` is always true in the reference (:331) -> always by class
        return remove_data_by_shapley(dataset, seed=args.removal_seed, by_class=True)
    if d == "loo":
        return remove_data_by_loo(dataset, args.removal_seed)
    if d == "add_one_in":
        return remove_data_for_aoi(dataset, args.removal_seed)
    return np.arange(len(dataset)), np.array([], dtype=int)


def iu_counts(args, remaining_labels, removed_labels):
    """(forget_count, retain_count) of get_grad (Wfisher.py:113-120).  `--removal_dist shapley` sets args.by_class = True in the
    reference (:331-335), so it counts the DISTINCT LABELS a loader shows, not its images.  For every other --removal_dist the
    reference never sets args.by_class and dies with AttributeError; here those count images (the `else` branch)."""
    if args.removal_dist == "shapley":
        return int(torch.unique(removed_labels).numel()), int(torch.unique(remaining_labels).numel())
    return int(removed_labels.numel()), int(remaining_labels.numel())


def influence_unlearn(args, backend, config, dataset, model, ema_model, scheduler, remaining_idx, removed_idx):
    """Influence unlearning (:509-546): the removed and the remaining set's size-weighted gradient sums, their normalised
    difference pushed through the WoodFisher inverse-Hessian approximation over a fresh shuffle of the remaining loader, one
    parameter perturbation and ONE EMA step.  Returns len(remaining loader), the reference's `training_steps` (:392)."""
    device = args.device
    n_t = scheduler.config.num_train_timesteps
    unlearner = backend.InfluenceUnlearner(model, scheduler)

    def loader_of(idx):
        return backend.DeviceLoader(dataset, idx, config["batch_size"], device)

    def draws(loader):
        for image, _ in loader:
            noise = torch.randn_like(image)
            yield image, noise, backend.antithetic_timesteps(n_t, image.shape[0], device)

    remaining = loader_of(remaining_idx)
    removed = loader_of(removed_idx) if len(removed_idx) else None          # no loader over nothing: count 0, gradient 0
    no_labels = torch.empty(0, dtype=torch.long)
    forget_count, retain_count = iu_counts(args, remaining.labels, removed.labels if removed is not None else no_labels)
    print("Calculating gradients with removed dataset....")
    forget_grad = unlearner.gradient_sum(draws(removed) if removed is not None else ())
    print("Calculating gradients with remaining dataset...")
    retain_grad = unlearner.gradient_sum(draws(remaining))
    retain_grad.mul_(forget_count / ((forget_count + retain_count) * retain_count))     # weight normalisation, 1^T w = 1 (:528)
    forget_grad.div_(forget_count + retain_count)                                       # 1 / N of equation (1) (:531)
    delta_w = unlearner.woodfisher(draws(remaining), retain_count, forget_grad.sub_(retain_grad))
    print("Applying perturbation...")
    unlearner.apply(delta_w, args.iu_ratio)
    ema_model.step(model.parameters())
    return len(remaining)


LORA_ALPHA, LORAPLUS_LR_RATIO = 32, 16          # fixed by the reference whatever the rank (:413, :423)


def lora_unlearn(args, backend, config, dataset, model, ema_model, scheduler, remaining_idx):
    """LoRA unlearning (:404-424, 548-642, 748-749): the gd loop body over the LoRA matrices of to_q / to_k / to_v alone (base frozen),
    LoRA+ Adam (B at 16 x the A matrices' rate, one clip norm over all of them), then ONE merge.
    The reference merges a deep copy of the model after every step and hands it to `ema_model.step`; every merged parameter is
    frozen, so that step copies instead of averaging and the shadows are the merged weights of the last step.  Here: merge once
    after the loop, copy into the shadows and advance the EMA's step counter by the steps taken - the same end state without
    streaming the whole model per step.  -> the model with the LoRA layers merged and removed"""
    device = args.device
    model = backend.get_peft_model(model, backend.LoraConfig(r=args.lora_rank, target_modules=["to_q", "to_v", "to_k"],
                                                               lora_alpha=LORA_ALPHA, lora_dropout=args.lora_dropout))
    params, groups = backend.lora_parameters(model, LORAPLUS_LR_RATIO)
    # create_loraplus_optimizer passes lr alone: Adam's defaults, no weight decay
    trainer = backend.FusedTrainer(model, scheduler, None, lr=config["optimizer_config"]["kwargs"].get("lr", 1e-4), weight_decay=0.0,
                                   adamw=config["optimizer_config"]["class_name"] == "AdamW", max_grad_norm=1.0, params=params,
                                   groups=groups)
    loader = backend.DeviceLoader(dataset, remaining_idx, config["batch_size"], device)
    n_t = scheduler.config.num_train_timesteps
    model.train()
    steps = 0
    while steps < args.gd_steps:
        for image, _ in loader:
            noise = torch.randn_like(image)
            ts = backend.antithetic_timesteps(n_t, image.shape[0], device)
            trainer.step(image, noise, ts)
            steps += 1
            if steps == args.gd_steps:
                break
    model = backend.merge_and_unload(model)
    with torch.no_grad():
        for s, p in zip(ema_model.shadow_params, model.parameters()):
            s.copy_(p.detach())
    ema_model.optimization_step += steps
    ema_model.cur_decay_value = ema_model.get_decay(ema_model.optimization_step)
    return model


def main(args, backend=None):
    if backend is None:
        import gad as backend
    lora = args.method in ("lora", "lora_u")
    if args.method not in ("gd", "gd_u", "ga", "ga_u", "iu", "lora", "lora_u"):
        raise NotImplementedError(f"method={args.method}: the engine implements the sFT family (gd/ga), influence unlearning (iu) and "
                                  "LoRA unlearning (lora); esd / retrain / prune_fine_tune are not unlearn.py methods here")
    if lora:
        if args.load is None:
            raise NotImplementedError(f"method={args.method} without --load: LoRA unlearning from a fresh model is not implemented - like the "
                                      "sFT family and influence unlearning it adapts a pre-trained (pruned) checkpoint; pass its directory")
        if args.use_8bit_optimizer:
            raise NotImplementedError("--use_8bit_optimizer: bitsandbytes' Adam8bit (reference :446) is not built here; LoRA unlearning "
                                      "runs fp32 LoRA+ Adam")
        if args.gradient_accumulation_steps != 1:
            raise NotImplementedError(f"--gradient_accumulation_steps={args.gradient_accumulation_steps}: only 1 is implemented "
                                      "(the reference's default)")
        if args.dataset == "imagenette":
            raise NotImplementedError("--dataset imagenette: the reference's unlearn.py leaves this branch dead (label_tokenizer and "
                                      "text_encoder are undefined at :576-577); LoRA unlearning covers the unconditional U-Nets")
    if hasattr(backend, "set_operand_precision"):      # --mixed_precision fp16|bf16 -> bf16 operands, fp32 everything else
        backend.set_operand_precision(args.mixed_precision)
    device = torch.device(args.device)
    args.device = device
    info = dict(vars(args))
    config = dataset_config(args.dataset)
    dataset = create_dataset(dataset_name=args.dataset, train=True)
    remaining_idx, removed_idx = coalition(args, dataset)
    if args.method in ("ga", "ga_u"):
        remaining_idx, removed_idx = removed_idx, remaining_idx
    backend.seed_everything(args.opt_seed)

    model, ema_model, _, _ = load_ckpt_model(args, args.load, backend)
    model.to(device)
    ema_model.to(device)
    scheduler = backend.DDPMScheduler(**config["scheduler_config"])
    if args.method == "iu":
        t0 = time.time()
        steps_goal = influence_unlearn(args, backend, config, dataset, model, ema_model, scheduler, remaining_idx, removed_idx)
    elif lora:
        t0 = time.time()
        steps_goal = args.gd_steps
        model = lora_unlearn(args, backend, config, dataset, model, ema_model, scheduler, remaining_idx)
    else:
        okw = dict(config["optimizer_config"]["kwargs"])
        if args.use_8bit_optimizer:
            # :429-477 bnb.optim.Adam8bit whatever class_name says: the config's decay (KeyError where the config has none, :459) on
            # every parameter whose name lacks "bias", none on the rest
            trainer = backend.FusedTrainer(model, scheduler, ema_model, lr=okw.get("lr", 1e-4),
                                           weight_decay=config["optimizer_config"]["kwargs"]["weight_decay"], max_grad_norm=1.0,
                                           loss_sign=-1.0 if args.method.startswith("ga") else 1.0, optim_bits=8,
                                           no_decay=["bias" in n for n, _ in model.named_parameters()])
        else:
            trainer = backend.FusedTrainer(model, scheduler, ema_model, lr=okw.get("lr", 1e-4),
                                           weight_decay=okw.get("weight_decay", 0.0),
                                           adamw=config["optimizer_config"]["class_name"] == "AdamW", max_grad_norm=1.0,
                                           loss_sign=-1.0 if args.method.startswith("ga") else 1.0)
        loader = backend.DeviceLoader(dataset, remaining_idx, config["batch_size"], device)
        n_t = scheduler.config.num_train_timesteps
        steps_goal = args.gd_steps if args.method.startswith("gd") else int(config["training_steps"]["ga"] // args.ga_ratio)

        t0 = time.time()
        steps = 0
        while steps < steps_goal:
            for image, _ in loader:
                noise = torch.randn_like(image)
                ts = backend.antithetic_timesteps(n_t, image.shape[0], device)
                trainer.step(image, noise, ts)
                steps += 1
                if steps == steps_goal:
                    break
    if device.type == "cuda":
        torch.cuda.synchronize(device)
    total_steps_time = time.time() - t0

    ema_model.store(model.parameters())           # the EMA is used for inference (:751-753)
    ema_model.copy_to(model.parameters())
    model.eval()
    pipeline, _, _ = build_pipeline(args, model, backend)
    sample_outdir = os.path.join(args.outdir, args.dataset, args.method, "samples",
                                 f"{args.removal_dist}/{args.removal_dist}_seed={args.removal_seed}")
    preview = pipeline(batch_size=config["n_samples"], num_inference_steps=args.num_inference_steps,
                       output_type="numpy").images
    save_image_grid(torch.from_numpy(np.asarray(preview)).permute(0, 3, 1, 2),
                    os.path.join(sample_outdir, f"prutirb_ratio_{args.iu_ratio}_steps_{steps_goal:0>8}.png"),
                    nrow=int(np.sqrt(config["n_samples"])))

    t1 = time.time()
    if args.model_behavior == "global":
        print(f"Generating {args.n_samples}...")
        images = generate_images(args, pipeline)
        if args.dataset == "celeba":                               # entropy, cluster_count, cluster_proportions (:787-803)
            decode = getattr(pipeline, "decoder", None)        # GAD_VQVAE_WEIGHTS: decoded samples against decoded reference latents
            info.update(backend.diversity_against_dataset(images, dataset, device, num_cluster=20,
                                                          **({} if decode is None else {"decode": decode})))
            print(f"entropy: {info['entropy']}")
        elif hasattr(backend, "global_scores_against_dataset"):      # fid_value, is, precision, recall (:807-837)
            info.update(backend.global_scores_against_dataset(images, dataset, device, args.batch_size))
        else:
            info["fid_value"] = backend.fid_against_dataset(images, dataset, device, args.batch_size)
        print("; ".join(f"{k}: {info[k]}" for k in ("fid_value", "precision", "recall", "is") if k in info))
    elif args.model_behavior == "local":                           # :839-958
        full_model_dir = os.path.join(args.outdir, args.dataset, "retrain", "models", "full")
        print(f"Loading full model checkpoint from {full_model_dir}")
        method, trained_steps = args.method, args.trained_steps
        args.method, args.trained_steps = "retrain", None
        try:
            full_model, full_ema_model, _, _ = load_ckpt_model(args, full_model_dir, backend)
        finally:
            args.method, args.trained_steps = method, trained_steps
        full_model.to(device)
        if args.use_ema:
            full_ema_model.to(device)
            full_ema_model.copy_to(full_model.parameters())
        full_model.eval()
        full_pipeline, _, _ = build_pipeline(args, full_model, backend)
        info.update(local_behavior_row(args, full_pipeline, pipeline, sample_outdir, backend))
        print("; ".join(f"{k}: {info[k]}" for k in ("avg_mse", "avg_nrmse", "avg_ssim", "avg_total_loss")))
    info.update(total_steps_time=total_steps_time, trained_steps=steps_goal,
                remaining_idx=np.asarray(remaining_idx).tolist(), removed_idx=np.asarray(removed_idx).tolist(),
                device=str(device), total_sampling_time=time.time() - t1)
    with open(args.db, "a+") as f:
        f.write(json.dumps(info, default=str) + "\n")
    print(f"Results saved to the database at {args.db}")
    return True


if __name__ == "__main__":
    if main(parse_args()):
        print("Unlearning is done!")
