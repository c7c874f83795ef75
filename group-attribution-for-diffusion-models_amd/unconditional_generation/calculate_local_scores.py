"""Local model behaviours of a removal model against the full model: per seed s = 0..n_samples-1 both models generate an
image from the same noise; the row records MSE / NRMSE / SSIM of the pair and the removal model's diffusion loss on the full
model's image, plus their averages.

Entry point kept from the reference (unconditional_generation/calculate_local_scores.py:71-388): same flags, the same default
directory grammar for the removal model (:246-263), `remaining_idx` / `removed_idx` from the removal checkpoint (:290-291),
`--use_ema` (:36-40), the full model's images saved under `{outdir}/{dataset}/local_scores/[ema_]generated_samples` (:265-271,
343-346), row = vars(args) + `generated_image_{s}_{mse,nrmse,ssim,diffusion_loss}` + `avg_*` (:335-384).  The computation is
the engine's (`gad.local_model_behaviors`: wide-launch generation, one fp64 metrics launch, ~1000-row loss launches).
`--precompute_stage reuse` is this port's CelebA latent mode, as in calculate_global_scores.py."""
import argparse
import json
import os
import sys

import numpy as np
import torch

_HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

import src.constants as constants  # noqa: E402
from src.diffusion_utils import build_pipeline, load_ckpt_model, local_behavior_row  # noqa: E402


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="calculate local model behaviors")
    p.add_argument("--removal_model_dir", type=str, default=None)
    p.add_argument("--removal_model_steps", type=int, default=None)
    p.add_argument("--full_model_dir", type=str, required=True)
    p.add_argument("--full_model_steps", type=int, default=None)
    p.add_argument("--outdir", type=str, default=constants.OUTDIR)
    p.add_argument("--dataset", type=str, choices=constants.DATASET + ["toy2"], default="cifar")
    p.add_argument("--excluded_class", type=int, default=None)
    p.add_argument("--removal_dist", type=str, default=None)
    p.add_argument("--datamodel_alpha", type=float, default=0.5)
    p.add_argument("--removal_seed", type=int, default=0)
    p.add_argument("--method", type=str, choices=constants.METHOD)
    p.add_argument("--pruning_ratio", type=float, default=0.3)
    p.add_argument("--pruner", type=str, default="magnitude", choices=["taylor", "random", "magnitude", "reinit", "diff-pruning"])
    p.add_argument("--thr", type=float, default=0.05)
    p.add_argument("--db", type=str, required=True)
    p.add_argument("--exp_name", type=str, default=None)
    p.add_argument("--n_samples", type=int, default=100)
    p.add_argument("--n_noises", type=int, default=50)
    p.add_argument("--num_inference_steps", type=int, default=100)
    p.add_argument("--device", type=str, default="cuda:0")
    p.add_argument("--use_ema", action="store_true", default=False)
    p.add_argument("--precompute_stage", type=str, default=None, choices=[None, "save", "reuse"])   # celeba latent mode
    return p.parse_args(argv)


def removal_directory(args):
    """:247-255"""
    d = "full"
    if args.excluded_class is not None:
        d = f"excluded_{args.excluded_class}"
    if args.removal_dist is not None:
        d = f"{args.removal_dist}/{args.removal_dist}"
        if args.removal_dist == "datamodel":
            d += f"_alpha={args.datamodel_alpha}"
        d += f"_seed={args.removal_seed}"
    return d


def _load(args, loaddir, method, steps, device, backend):
    """Newest (or the `steps`) checkpoint of a directory as (model in eval mode on the device, index lists); the architecture
    is the registry's for `retrain` / `gd_u` and the pruned one otherwise (:222-243)."""
    keep = args.method, getattr(args, "trained_steps", None)
    args.method, args.trained_steps = method, steps
    try:
        model, ema_model, remaining_idx, removed_idx = load_ckpt_model(args, loaddir, backend)
    finally:
        args.method, args.trained_steps = keep
    model.to(device)
    if args.use_ema:
        ema_model.to(device)
        ema_model.copy_to(model.parameters())
    model.eval()
    return model, remaining_idx, removed_idx


def main(args, backend=None):
    if backend is None:
        import gad as backend
    if args.method is None:
        raise ValueError("--method is needed: it names the removal model's directory and architecture")
    device = torch.device(args.device)
    if args.removal_model_dir is None:
        args.removal_model_dir = os.path.join(args.outdir, args.dataset, args.method, "models", removal_directory(args))
    sample_outdir = os.path.join(args.outdir, args.dataset, "local_scores",
                                 "ema_generated_samples" if args.use_ema else "generated_samples")
    os.makedirs(sample_outdir, exist_ok=True)
    print("Loading full model checkpoint...")
    full_model, _, _ = _load(args, args.full_model_dir, "retrain", args.full_model_steps, device, backend)
    print("Loading removal model checkpoint...")
    removal_model, remaining_idx, removed_idx = _load(args, args.removal_model_dir, args.method, args.removal_model_steps,
                                                      device, backend)
    info = {k: v for k, v in vars(args).items() if k != "trained_steps"}
    info["remaining_idx"] = np.asarray(remaining_idx).tolist()
    info["removed_idx"] = np.asarray(removed_idx).tolist()
    full_pipeline, _, _ = build_pipeline(args, full_model, backend)
    removal_pipeline, _, _ = build_pipeline(args, removal_model, backend)
    info.update(local_behavior_row(args, full_pipeline, removal_pipeline, sample_outdir, backend))
    with open(args.db, "a+") as f:
        f.write(json.dumps(info, default=str) + "\n")
    print(f"Results saved to the database at {args.db}")
    return True


if __name__ == "__main__":
    main(parse_args())
