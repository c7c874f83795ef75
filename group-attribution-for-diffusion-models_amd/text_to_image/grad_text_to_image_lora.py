"""Projected per-sample LoRA gradients (TRAK / D-TRAK / Journey-TRAK features) of a Stable-Diffusion U-Net.

Entry point kept from the reference (text_to_image/grad_text_to_image_lora.py): flags and defaults (:76-251), output directory
`{output_dir}/{dataset}/gradients/{source}` (:266-274), LoRA loaded from `--lora_dir` / `--lora_steps` (:313-333), the three
sources (:335-545), projector seed 42 / normal entries / `max_batch_size = --train_batch_size` (:562-569), the behaviours of
`--f` (:589-727), the average over `--num_timesteps` selected timesteps or `--num_journey_noises` draws (:732-815) and the
file names `emb_f=..._num_timesteps=..._proj_dim=....pt` / `emb_f=..._num_journey_points=..._num_journey_noises=..._proj_dim=....pt`
with `group.csv` beside them.

The features come from gad.trak.lora_gradient_features: with `--mixed_precision fp16|bf16` (bf16 activations) all per-sample
gradients of a batch of `--train_batch_size` rows come from ONE forward / backward (gad_hgemm_tn_seg), as vmap(grad(f)) gives them
in the reference; with fp32 activations one row per backward.

Deliberate deviations: the frozen VAE / CLIP encoders are hub-fetched and outside the hot path, so `train` reads
`{train_data_dir}/latent_cache.pt` as train_text_to_image_lora.py here does (`--synthetic_cache` writes a seeded stand-in) and
the prompt arrives as embeddings (`--prompt_embeds`, else the text encoder GAD_SD_TEXT_WEIGHTS + GAD_CLIP_BPE name, gad/text.py,
else a seeded stand-in); generated and journey latents come from
gad.StableDiffusionLatentPipeline (DDIM, or PLMS with `--sampler pndm`: num_inference_steps + 1 callbacks, which the journey
points index as they come) with a per-step callback; noise is drawn per block of `--train_batch_size` rows as one
[rows][k] draw from a device generator seeded with `--seed` (the reference: one draw per batch per timestep from the global
generator); the row index of R is the offset in the flat gradient buffer (gad/trak.py)."""
import argparse
import json
import os
import sys

import numpy as np
import pandas as pd
import torch

_HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

from src.ddpm_config import PromptConfig  # noqa: E402


def parse_args(argv=None):
    """grad_text_to_image_lora.py:76-251"""
    p = argparse.ArgumentParser(description="Per-sample LoRA gradient features of a text-to-image U-Net")
    p.add_argument("--pretrained_model_name_or_path", type=str, default="lambdalabs/miniSD-diffusers")
    p.add_argument("--revision", type=str, default=None)                   # hub models only: accepted, not used
    p.add_argument("--variant", type=str, default=None)
    p.add_argument("--source", type=str, default="train", choices=["train", "generated", "generated_journey"])
    p.add_argument("--train_data_dir", type=str, default=None)
    p.add_argument("--image_column", type=str, default="image")
    p.add_argument("--caption_column", type=str, default="text")
    p.add_argument("--output_dir", type=str, default=None)
    p.add_argument("--cache_dir", type=str, default=None)
    p.add_argument("--seed", type=int, default=42, help="A seed for reproducible training.")
    p.add_argument("--num_images", type=int, default=50, help="number of generated images")
    p.add_argument("--generation_seed", type=int, default=42, help="seed for image generation")
    p.add_argument("--num_journey_points", type=int, default=50)
    p.add_argument("--num_journey_noises", type=int, default=1)
    p.add_argument("--resolution", type=int, default=256)
    p.add_argument("--center_crop", default=False, action="store_true")
    p.add_argument("--random_flip", default=False, action="store_true")
    p.add_argument("--train_batch_size", type=int, default=16)
    p.add_argument("--dataloader_num_workers", type=int, default=0)
    p.add_argument("--cls_key", type=str, default="style")
    p.add_argument("--cls", type=str, default="post_impressionism")
    p.add_argument("--lora_dir", type=str, default=None)
    p.add_argument("--lora_steps", type=int, default=None)
    p.add_argument("--num_timesteps", type=int, default=100, help="number of timesteps to select for computing gradients")
    p.add_argument("--proj_dim", type=int, default=32768, help="dimension size for projected gradients")
    p.add_argument("--f", type=str, required=True, help="loss function for computing gradients")
    # additions of this tree
    p.add_argument("--mixed_precision", type=str, default="fp16", choices=["no", "fp16", "bf16"],
                   help="fp16 / bf16: bf16 activations (the reference casts the frozen weights to fp16); no: fp32")
    p.add_argument("--timesteps_per_backward", type=int, default=None, help="timesteps of a row per forward / backward")
    p.add_argument("--num_inference_steps", type=int, default=100, help="the reference generates with 100 steps")
    p.add_argument("--sampler", type=str, default="ddim", choices=["ddim", "pndm"], help="ddim (default) or pndm: the PLMS sampler SD-1.x repositories ship, num_inference_steps + 1 U-Net calls")
    p.add_argument("--prompt_embeds", type=str, default=None, help=".pt with cond / uncond [77, D] text embeddings")
    p.add_argument("--unet_weights", type=str, default=None, help="local state_dict of the base U-Net (optional)")
    p.add_argument("--unet_overrides", type=str, default=None, help="json dict of UNet2DConditionModel kwargs (tests)")
    p.add_argument("--synthetic_cache", action="store_true", help="create a seeded stand-in latent cache if missing")
    p.add_argument("--device", type=str, default="cuda:0")
    args = p.parse_args(argv)
    if args.train_data_dir is None:
        raise ValueError("Need a training folder.")
    return args


def dataset_name(args):
    """:264-268"""
    name = "artbench" if "artbench" in args.train_data_dir else args.train_data_dir
    if args.cls is not None and args.cls_key is not None:
        name += f"_{args.cls}"
    return name


def output_directory(args):
    """:270-274"""
    return os.path.join(args.output_dir, dataset_name(args), "gradients", args.source)


def output_filename(args):
    """:774,814"""
    if args.source == "generated_journey":
        return (f"emb_f={args.f}_num_journey_points={args.num_journey_points}_num_journey_noises={args.num_journey_noises}"
                f"_proj_dim={args.proj_dim}.pt")
    return f"emb_f={args.f}_num_timesteps={args.num_timesteps}_proj_dim={args.proj_dim}.pt"


def lora_weight_name(args):
    """:316-319"""
    return "pytorch_lora_weights" + (f"_{args.lora_steps}" if args.lora_steps is not None else "") + ".safetensors"


def journey_points(num_inference_steps, num_journey_points):
    """:517-521"""
    return np.arange(start=1, stop=num_inference_steps, step=num_inference_steps // num_journey_points)


def prompt_embeddings(args, ctx_dim):
    """(cond, uncond) [1][77][D]: `--prompt_embeds`, or the seeded stand-in for CLIP-text(prompt) compute_model_behaviors.py uses"""
    if "artbench" not in dataset_name(args):
        raise NotImplementedError(dataset_name(args))                     # :453-456
    assert args.cls is not None
    prompt = PromptConfig.artbench_config[args.cls]
    from gad.text import prompt_context
    pe = torch.load(args.prompt_embeds, map_location="cpu", weights_only=False) if args.prompt_embeds else None
    cond, uncond, _ = prompt_context(prompt, pe, ctx_dim, torch.device(args.device))   # GAD_SD_TEXT_WEIGHTS: the text encoder itself
    return cond.unsqueeze(0), uncond.unsqueeze(0)


def main(args, backend=None):
    if backend is None:
        import gad as backend
    from gad import trak
    from text_to_image.train_text_to_image_lora import synthetic_cache
    if args.output_dir is None:
        raise ValueError("Need an output folder.")
    args.dataset = dataset_name(args)
    out_dir = output_directory(args)
    os.makedirs(out_dir, exist_ok=True)
    if args.seed is not None:
        backend.seed_everything(args.seed)
    device = torch.device(args.device)
    backend.set_operand_precision(args.mixed_precision)
    try:
        ucfg = json.loads(args.unet_overrides) if args.unet_overrides else {}
        unet = backend.UNet2DConditionModel(**ucfg)
        if args.unet_weights:
            unet.load_state_dict(torch.load(args.unet_weights, map_location="cpu", weights_only=False))
        unet.to(device)
        for p in unet.parameters():                                       # :297-299
            p.requires_grad_(False)
        unet.load_attn_procs(args.lora_dir, weight_name=lora_weight_name(args))
        print(f"LoRA weights loaded from {os.path.join(args.lora_dir, lora_weight_name(args))}")
        for n, p in unet.named_parameters():                              # :331-333
            if "lora_layer" in n:
                p.requires_grad_(True)
        sched = backend.DDPMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", num_train_timesteps=1000)

        if args.source == "train":
            cache_path = os.path.join(args.train_data_dir, "latent_cache.pt")
            if not os.path.exists(cache_path):
                if not args.synthetic_cache:
                    raise FileNotFoundError(f"{cache_path} not found (pass --synthetic_cache for a seeded stand-in)")
                synthetic_cache(cache_path, res=args.resolution, ctx_dim=unet.config.cross_attention_dim)
            cache = torch.load(cache_path, map_location="cpu", weights_only=False)
            keep = np.arange(len(cache["latents"]))
            if args.cls is not None and args.cls_key is not None:         # :347-351
                keep = keep[np.array(cache[args.cls_key]) == args.cls]
            latents = cache["latents"][keep].float()
            text = cache["text_emb"].float()
            contexts = text[keep] if text.shape[0] == len(cache["latents"]) else text.expand(len(keep), -1, -1)
            pd.DataFrame({"index": list(range(len(keep))), "artist": np.array(cache["artist"])[keep],
                          "filename": np.array(cache["filename"])[keep]}).to_csv(os.path.join(out_dir, "group.csv"), index=False)
            timesteps = torch.tensor(list(range(0, 1000, 1000 // args.num_timesteps)))                 # :780
        else:
            cond, uncond = prompt_embeddings(args, unet.config.cross_attention_dim)
            pipe = backend.StableDiffusionLatentPipeline(unet, backend.sd_scheduler(args.sampler))
            gen = torch.Generator(device=device).manual_seed(args.generation_seed)                      # :487-488
            step_idx, ts, lats, image_idx = [], [], [], []
            for i in range(args.num_images):
                steps = []
                pipe(cond.to(device), uncond.to(device), num_inference_steps=args.num_inference_steps, generator=gen,
                     height=args.resolution, width=args.resolution,
                     callback=lambda s, t, lat: steps.append((s, int(t), lat.detach().cpu())))
                if args.source == "generated":                            # the final latent only (:508-513)
                    picks = [len(steps) - 1]
                else:
                    picks = journey_points(len(steps), args.num_journey_points)
                for j in picks:
                    step_idx.append(steps[j][0])
                    ts.append(steps[j][1])
                    lats.append(steps[j][2])
                    image_idx.append(i)
            pd.DataFrame({"generated_image_idx": image_idx, "step_idx": step_idx}).to_csv(os.path.join(out_dir, "group.csv"), index=True)
            latents = torch.cat(lats).float()
            contexts = cond.expand(latents.shape[0], -1, -1)
            if args.source == "generated_journey":                        # the row's own t, num_journey_noises draws (:734-772)
                timesteps = torch.tensor(ts).view(-1, 1).expand(-1, args.num_journey_noises)
            else:
                timesteps = torch.tensor(list(range(0, 1000, 1000 // args.num_timesteps)))

        lora_params, gflat = trak.lora_flat_gradient(unet)
        print(f"Number of trainable LoRA parameters: {sum(p.numel() for p in lora_params)}")
        projector = trak.Projector(grad_dim=gflat.numel(), proj_dim=args.proj_dim, seed=42, proj_type=trak.ProjectionType.normal,
                                   device=device, max_batch_size=args.train_batch_size)
        embs = trak.lora_gradient_features(unet, sched, latents, contexts, timesteps, args.f, projector, seed=args.seed,
                                           samples_per_backward=args.train_batch_size,
                                           timesteps_per_backward=args.timesteps_per_backward)
    finally:
        backend.set_operand_precision("no")
    path = os.path.join(out_dir, output_filename(args))
    torch.save(embs, path)
    return path


if __name__ == "__main__":
    main(parse_args())
    print("Done!")
