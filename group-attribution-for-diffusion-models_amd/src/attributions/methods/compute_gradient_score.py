"""Scores from projected gradient features: D-TRAK, TRAK, Journey-TRAK, relative / renormalized IF, vanilla gradient
(entry point kept from the reference src/attributions/methods/compute_gradient_score.py).

Host linear algebra in fp64 (a [d][d] kernel, d = 1024 by default: milliseconds, not a device kernel).  The features
are the float32 memmaps d_trak_grad.py writes, at the same paths."""
import os

import numpy as np

import src.constants as constants
from src.datasets import create_dataset

IMAGE_EXTENSIONS = {"jpg", "jpeg", "png", "bmp", "webp", "tiff"}
RIDGE = 5e-1


def trak_kernel_inverse(train_phi):
    """(phi^T phi + 0.5 I)^-1 in fp64 (compute_gradient_score.py:101-103)"""
    phi = np.asarray(train_phi, dtype=np.float64)
    kernel = phi.T @ phi + RIDGE * np.eye(phi.shape[1])
    return np.linalg.inv(kernel)


def gradient_scores(train_phi, val_phi, gradient_type, kernel=None):
    """[n_val][n_train] scores (compute_gradient_score.py:106-120)"""
    train_phi = np.asarray(train_phi, dtype=np.float64)
    val_phi = np.asarray(val_phi, dtype=np.float64)
    if gradient_type == "vanilla_gradient":
        train_n = train_phi / np.linalg.norm(train_phi, axis=1, keepdims=True)
        val_n = val_phi / np.linalg.norm(val_phi, axis=1, keepdims=True)
        return val_n @ train_n.T
    if kernel is None:
        kernel = trak_kernel_inverse(train_phi)
    proj = train_phi @ kernel                                      # [n_train][d]
    if gradient_type == "relative_if":
        magnitude = np.linalg.norm(proj.T, axis=0)
    elif gradient_type == "renormalized_if":
        magnitude = np.linalg.norm(train_phi.T, axis=0)
    else:
        magnitude = 1.0
    return val_phi @ proj.T / magnitude


def aggregate_by_class(scores, dataset, by="mean"):
    """Per-class mean (or max) of sample scores (reference src/attributions/methods/attribution_utils.py:15-48)."""
    if scores.ndim == 1:
        scores = scores.reshape(1, -1)
    n = scores.shape[0]
    labels_raw = [entry[1] for entry in dataset] if not hasattr(dataset, "targets") else list(dataset.targets)
    value_to_number = {v: i for i, v in enumerate(sorted(set(labels_raw)))}
    labels = np.array([value_to_number[v] for v in labels_raw])
    num_labels = len(np.unique(labels))
    result = np.zeros((n, num_labels))
    for i in range(num_labels):
        mask = labels == i
        if by == "mean":
            result[:, i] = scores[:, mask].sum(axis=1) / np.sum(mask)
        elif by == "max":
            result[:, i] = np.max(scores[:, mask])
    return result


def _n_images(sample_dir):
    return len([f for f in os.listdir(sample_dir) if f.split(".")[-1] in IMAGE_EXTENSIONS])


def compute_gradient_scores(args, retraining=False, training_seeds=None):
    """Compute scores for D-TRAK, TRAK, and influence function (compute_gradient_score.py:13-136)."""
    dataset = create_dataset(dataset_name=args.dataset, train=True)
    model_behavior = "mean-squared-l2-norm" if args.gradient_type == "d_trak" else "loss"
    t_strategy = "uniform"
    tag = f"f={model_behavior}_t={t_strategy}_k={args.k_partition}_d={args.projector_dim}"
    if args.gradient_type == "journey_trak":
        # the generation gradients of d_trak_grad.py --calculate_gen_grad (:26-33, :42): sample_size rows, no --sample_dir;
        # train side, kernel, formula and aggregation are trak's
        val_grad_path = os.path.join(constants.OUTDIR, args.dataset, "d_trak", "full", f"gen_{tag}")
        have = os.path.getsize(val_grad_path) // (4 * args.projector_dim)
        if args.sample_size is None or have < args.sample_size:
            raise ValueError(f"journey_trak: {val_grad_path} holds {have} rows of {args.projector_dim} features, "
                             f"sample_size={args.sample_size} asked for")
        n_val = args.sample_size
    else:
        val_grad_path = os.path.join(args.sample_dir, "d_trak", f"reference_{tag}")
        n_val = _n_images(args.sample_dir)
    val_phi = np.memmap(val_grad_path, dtype=np.float32, mode="r", shape=(n_val, args.projector_dim))
    val_phi = val_phi[: args.sample_size]

    if retraining:
        scores = np.zeros(len(dataset))
        for seed in training_seeds:
            removal_dir = f"{args.removal_dist}/{args.removal_dist}_seed={seed}"
            # the reference reads "d_track" here (a typo of d_trak): kept so its artefacts load
            train_grad_path = os.path.join(constants.OUTDIR, args.dataset, "d_track", removal_dir,
                                           f"train_f={args.trak_behavior}_t={args.t_strategy}_k={args.k_partition}"
                                           f"_d={args.projector_dim}")
            train_phi = np.memmap(train_grad_path, dtype=np.float32, mode="r", shape=(len(dataset), args.projector_dim))
            scores = scores + gradient_scores(train_phi, val_phi, "trak") / len(training_seeds)
    else:
        train_grad_dir = os.path.join(constants.OUTDIR, args.dataset, "d_trak", "full")
        train_grad_path = os.path.join(train_grad_dir, f"train_{tag}")
        kernel_path = os.path.join(train_grad_dir, f"kernel_train_{tag}.npy")
        train_phi = np.memmap(train_grad_path, dtype=np.float32, mode="r", shape=(len(dataset), args.projector_dim))
        kernel = None
        if args.gradient_type != "vanilla_gradient":
            if os.path.isfile(kernel_path):
                kernel = np.load(kernel_path)
            else:
                kernel = trak_kernel_inverse(train_phi)
                np.save(kernel_path, kernel)
        scores = gradient_scores(train_phi, val_phi, args.gradient_type, kernel)

    # Using the average as coefficients
    if args.model_behavior_key not in ["ssim", "nrmse", "diffusion_loss"]:
        coeff = np.mean(scores, axis=0)
    else:
        coeff = scores
    if args.by_class:
        coeff = aggregate_by_class(coeff, dataset, args.by)
    else:
        coeff = scores                    # as in the reference: without by_class the raw [n_val][n_train] scores
    return coeff
