"""TRAK / D-TRAK gradient features (entry point kept from the reference src/attributions/methods/d_trak_grad.py).

Same flags, defaults and output path grammar; the float32 np.memmap [n_samples][projector_dim] is written where the
reference writes it.  The features come from gad.trak: one fused forward / backward per image over its k (noisy, t) rows
and the HIP random projector in place of trak's CudaProjector.

Deliberate deviation: rows are written in dataset order (row r = r-th remaining training image, or the r-th sample
image in sorted file order); the reference writes them in the order of a shuffled DataLoader.

--calculate_gen_grad (Journey-TRAK, reference :450-494) generates --n_samples ancestral DDPM trajectories with
gad.trak.journey_latents (one fused gad_ddpm_step launch per step, variance noise keyed by (opt_seed, sample): a rerun is
bit-identical, where the reference draws that noise from an unseeded generator) and writes the features of their latents
to the gen_ path.  Not ported (refused by name): --calculate_gen_grad together with --sample_dir, the celeba / imagenette
latent pipelines, and the behaviours ssim / fid / nrmse / is."""
import argparse
import os
import sys

import numpy as np
import torch

_HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

import src.constants as constants  # noqa: E402
from src.datasets import (create_dataset, remove_data_by_class, remove_data_by_datamodel,  # noqa: E402
                          remove_data_by_shapley, remove_data_by_uniform)

IMAGE_EXTENSIONS = {"jpg", "jpeg", "png", "bmp", "webp", "tiff"}


def parse_args(argv=None):
    """d_trak_grad.py:34-181"""
    parser = argparse.ArgumentParser(description="Calculating gradient for D-TRAK and TRAK.")
    parser.add_argument("--opt_seed", type=int, help="random seed for model training or unlearning", default=42)
    parser.add_argument("--load", type=str, help="directory path for loading pre-trained model", default=None)
    parser.add_argument("--dataset", type=str, help="dataset for training or unlearning", choices=constants.DATASET,
                        default=None)
    parser.add_argument("--device", type=str, help="device of training", default="cuda:0")
    parser.add_argument("--outdir", type=str, help="output parent directory", default=constants.OUTDIR)
    parser.add_argument("--excluded_class", type=int, help="dataset class to exclude for class-wise data removal",
                        default=None)
    parser.add_argument("--method", type=str, help="training or unlearning method", choices=constants.METHOD, required=True)
    parser.add_argument("--removal_dist", type=str, help="distribution for removing data", default=None)
    parser.add_argument("--datamodel_alpha", type=float,
                        help="proportion of full dataset to keep in the datamodel distribution", default=0.5)
    parser.add_argument("--removal_seed", type=int, help="random seed for sampling from the removal distribution", default=0)
    parser.add_argument("--num_inference_steps", type=int, default=100,
                        help="number of diffusion steps for generating images")
    parser.add_argument("--num_train_steps", type=int, default=1000, help="number of diffusion steps during training")
    parser.add_argument("--mixed_precision", type=str, default="no", choices=["no", "fp16", "bf16"],
                        help="Whether to use mixed precision (the features are computed in fp32).")
    parser.add_argument("--model_behavior", type=str,
                        choices=["loss", "mean", "mean-squared-l2-norm", "l1-norm", "l2-norm", "linf-norm", "ssim", "fid",
                                 "nrmse", "is"],
                        default=None, required=True, help="Specification for D-TRAK model behavior.")
    parser.add_argument("--model_behavior_value", type=float, default=None,
                        help="Model output for a pre-calculated model behavior e.g. FID, SSIM, IS.")
    parser.add_argument("--t_strategy", type=str, choices=["uniform", "cumulative"], help="strategy for sampling time steps")
    parser.add_argument("--k_partition", type=int, default=None, help="Partition for embeddings across time steps.")
    parser.add_argument("--projector_dim", type=int, default=1024, help="Dimension for TRAK projector")
    parser.add_argument("--sample_dir", type=str, default=None, help="filepath of sample (generated) images ")
    parser.add_argument("--calculate_gen_grad", help="whether to generate validation set and calculate phi",
                        action="store_true", default=False)
    parser.add_argument("--n_samples", type=int, help="number of generated images to consider for local model behaviors",
                        default=None)
    return parser.parse_args(argv)


def removal_directory(args):
    """d_trak_grad.py:277-284"""
    removal_dir = "full"
    if args.excluded_class is not None:
        removal_dir = f"excluded_{args.excluded_class}"
    if args.removal_dist is not None:
        removal_dir = f"{args.removal_dist}/{args.removal_dist}"
        if args.removal_dist == "datamodel":
            removal_dir += f"_alpha={args.datamodel_alpha}"
        removal_dir += f"_seed={args.removal_seed}"
    return removal_dir


def feature_tag(args):
    return f"f={args.model_behavior}_t={args.t_strategy}_k={args.k_partition}_d={args.projector_dim}"


def save_path(args):
    """Where the memmap goes (d_trak_grad.py:333-378)."""
    if args.sample_dir is not None:
        return os.path.join(args.sample_dir, "d_trak", f"reference_{feature_tag(args)}")
    prefix = "gen" if args.calculate_gen_grad else "train"
    return os.path.join(args.outdir, args.dataset, "d_trak", removal_directory(args), f"{prefix}_{feature_tag(args)}")


def model_directory(args):
    return os.path.join(args.outdir, args.dataset, args.method, "models", removal_directory(args))


def remaining_indices(args, dataset):
    """d_trak_grad.py:295-324"""
    if args.excluded_class is not None:
        return remove_data_by_class(dataset, excluded_class=[args.excluded_class])[0]
    if args.removal_dist is None:
        return np.arange(len(dataset))
    if args.removal_dist == "uniform":
        return remove_data_by_uniform(dataset, seed=args.removal_seed)[0]
    if args.removal_dist == "datamodel":
        return remove_data_by_datamodel(dataset, alpha=args.datamodel_alpha, seed=args.removal_seed)[0]
    if args.removal_dist == "shapley":
        # the reference's `args.dataset == "cifar100" or "celeba"` is always true: by class for every dataset
        return remove_data_by_shapley(dataset, seed=args.removal_seed, by_class=True)[0]
    raise NotImplementedError(f"--removal_dist {args.removal_dist}")


def sample_files(sample_dir):
    return sorted(f for f in os.listdir(sample_dir) if f.split(".")[-1] in IMAGE_EXTENSIONS)


def load_sample_images(sample_dir):
    """Sample images as [N][C][H][W] in [-1, 1] (ToTensor + Normalize(0.5, 0.5)), sorted by file name."""
    from PIL import Image
    imgs = []
    for f in sample_files(sample_dir):
        with Image.open(os.path.join(sample_dir, f)) as im:
            imgs.append(torch.from_numpy(np.asarray(im.convert("RGB"), dtype=np.float32) / 255.0).permute(2, 0, 1))
    return torch.stack(imgs) * 2 - 1


def main(args, backend=None):
    """Compute and save the projected gradient features (d_trak_grad.py:184-696)."""
    if backend is None:
        import gad as backend
    from gad.trak import (Projector, ProjectionType, gradient_features, journey_gradient_features, journey_latents,
                          selected_timesteps)
    from src.diffusion_utils import build_model, dataset_config
    from src.utils import get_max_steps

    if args.calculate_gen_grad and args.sample_dir is not None:
        raise NotImplementedError("--calculate_gen_grad with --sample_dir: calculate_gen_grad generates its own validation "
                                  "set (the combination is meaningless in the reference)")
    if args.dataset in ("celeba", "imagenette"):
        raise NotImplementedError(f"--dataset {args.dataset}: the latent (VQ-VAE / LDM) gradient features are not ported")
    if args.calculate_gen_grad:
        for flag in ("n_samples", "k_partition", "t_strategy"):
            if getattr(args, flag) is None:
                raise ValueError(f"--calculate_gen_grad requires --{flag}")
        if args.n_samples < 1:
            raise ValueError(f"--n_samples {args.n_samples}: must be >= 1")
    if args.t_strategy is None or args.k_partition is None:
        raise ValueError("--t_strategy and --k_partition are required")
    device = torch.device(args.device)
    config = dataset_config(args.dataset)
    batch_size = 8                                                     # config["batch_size"] = 8 (:326)

    train_dataset = None if args.calculate_gen_grad else create_dataset(dataset_name=args.dataset, train=True)
    if args.calculate_gen_grad:
        images, n_samples = None, args.n_samples                       # the validation set is generated below
    elif args.sample_dir is None:
        n_samples = len(train_dataset)
        backend.seed_everything(args.opt_seed)                         # the training transform's random flips
        images = torch.stack([torch.as_tensor(train_dataset[int(i)][0]) for i in remaining_indices(args, train_dataset)])
    else:
        images = load_sample_images(args.sample_dir)
        n_samples = len(images)
    out_path = save_path(args)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)

    model_outdir = model_directory(args)
    steps = get_max_steps(model_outdir)
    if steps is None:
        raise FileNotFoundError(f"no ckpt_steps_*.pt under {model_outdir}")
    ckpt = torch.load(os.path.join(model_outdir, f"ckpt_steps_{steps:0>8}.pt"), map_location="cpu", weights_only=False)
    model = build_model(args, config, backend)
    model.load_state_dict(ckpt["unet"])
    model.to(device)
    _, gflat = model.flatten_parameters()
    scheduler = backend.DDPMScheduler(**config["scheduler_config"])
    if scheduler.config.prediction_type != "epsilon":
        raise NotImplementedError(f"prediction_type={scheduler.config.prediction_type}")

    projector = Projector(grad_dim=gflat.numel(), proj_dim=args.projector_dim, seed=args.opt_seed,
                          proj_type=ProjectionType.normal, device=device, max_batch_size=32)
    dstore_keys = np.memmap(out_path, dtype=np.float32, mode="w+", shape=(n_samples, args.projector_dim))
    timesteps = selected_timesteps(args.t_strategy, args.k_partition, scheduler.config.num_train_timesteps)
    if args.calculate_gen_grad:                                        # Journey-TRAK (d_trak_grad.py:450-494, :729-731)
        latents = journey_latents(model, scheduler, n_samples, args.k_partition, opt_seed=args.opt_seed, device=device)
        journey_gradient_features(model, scheduler, latents, args.model_behavior, timesteps, projector, opt_seed=args.opt_seed,
                                  batch_size=batch_size, out=dstore_keys, k_partition=args.k_partition)
    else:
        gradient_features(model, scheduler, images, args.model_behavior, timesteps, projector, opt_seed=args.opt_seed,
                          batch_size=batch_size, out=dstore_keys)
    dstore_keys.flush()
    print(f"saved {n_samples if images is None else len(images)} x {args.projector_dim} features to {out_path}")
    return out_path


if __name__ == "__main__":
    main(parse_args())
