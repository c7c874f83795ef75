"""TRAK-related baselines for the text-to-image experiment (entry point kept from the reference text_to_image/traks.py).

Reads the feature files grad_text_to_image_lora.py writes under `{output_dir}/gradients/{train,generated,generated_journey}` and
computes, per training image, gradient similarity, TRAK, relative / renormalised influence, Journey-TRAK and D-TRAK, aggregates
them per group (avg / max for grad_sim, sum for the others) and saves the `.npy` arrays and stable-sorted rank files under
`{output_dir}/baselines` with the reference's names.

Deliberate deviations: the ridge system (Phi^T Phi + lam I) X = Phi^T is SOLVED (torch.linalg.solve; rocSOLVER on the device)
instead of inverted and multiplied; `--device`, `--train_data_dir` (where `{cls}_{group}s.csv` lies; default as the reference,
under DATASET_DIR) and `--num_journey_points` / `--num_journey_noises` (the reference hard-codes 50 / 1 in the file name) are
additions."""
import argparse
import os
import sys

import numpy as np
import pandas as pd
import torch

_HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

import src.constants as constants  # noqa: E402


def parse_args(argv=None):
    """traks.py:14-63"""
    p = argparse.ArgumentParser(description="Run TRAK-related methods.")
    p.add_argument("--output_dir", type=str, default=None, help="output parent directory", required=True)
    p.add_argument("--num_timesteps", type=int, help="number of timesteps for computing the gradients", default=100)
    p.add_argument("--proj_dim", type=int, help="projection dimension for the gradients", default=32768)
    p.add_argument("--dataset", type=str, choices=["artbench"], default="artbench", help="dataset")
    p.add_argument("--cls", type=str, default="post_impressionism", help="class of images in the dataset")
    p.add_argument("--group", type=str, default="artist", choices=["artist", "filename"], help="unit for how to group images")
    p.add_argument("--lam", type=float, help="factor to stablize kernel matrix inversion", default=5e-1)
    p.add_argument("--num_journey_points", type=int, default=50)
    p.add_argument("--num_journey_noises", type=int, default=1)
    p.add_argument("--train_data_dir", type=str, default=None, help="directory of {cls}_{group}s.csv")
    p.add_argument("--device", type=str, default="cuda")
    args = p.parse_args(argv)
    args.gradient_dir = os.path.join(args.output_dir, "gradients")
    return args


def sample_scores(train, train_dtrak, gen, gen_dtrak, journey, lam):
    """traks.py:131-188: name -> per-training-image score (float tensors on the features' device)"""
    out = {}
    sim = gen @ train.T
    sim = sim / (gen.norm(dim=-1, keepdim=True) @ train.norm(dim=-1, keepdim=True).T)
    out["grad_sim"] = sim.mean(dim=0)

    def ridge(phi):                                               # (Phi^T Phi + lam I)^-1 Phi^T: [proj_dim][train_size]
        k = phi.T @ phi
        k.diagonal().add_(lam)
        return torch.linalg.solve(k, phi.T)

    x = ridge(train)
    influence = gen @ x
    out["trak"] = influence.mean(dim=0)
    out["relative_influence"] = (influence / x.norm(dim=0)).mean(dim=0)
    out["renorm_influence"] = (influence / train.norm(dim=-1)).mean(dim=0)
    out["journey_trak"] = (journey @ x).mean(dim=0)
    out["dtrak"] = (gen_dtrak @ ridge(train_dtrak)).mean(dim=0)
    return out


def group_scores(sample, group_indices):
    """traks.py:190-207: [num_groups][1] arrays; avg / max for grad_sim, sum for the others"""
    out = {}
    for method, attrs in sample.items():
        if method == "grad_sim":
            out[f"avg_{method}"] = np.array([[attrs[idx].mean()] for idx in group_indices], dtype=np.float64)
            out[f"max_{method}"] = np.array([[attrs[idx].max()] for idx in group_indices], dtype=np.float64)
        else:
            out[method] = np.array([[attrs[idx].sum()] for idx in group_indices], dtype=np.float64)
    return out


def main(args):
    if args.dataset != "artbench":
        raise ValueError(args.dataset)
    data_dir = args.train_data_dir or os.path.join(constants.DATASET_DIR, "artbench-10-imagefolder-split", "train")
    group_df = pd.read_csv(os.path.join(data_dir, f"{args.cls}_{args.group}s.csv"))
    suffix = f"num_timesteps={args.num_timesteps}_proj_dim={args.proj_dim}.pt"
    dev = torch.device(args.device)

    def load(*parts):
        return torch.load(os.path.join(args.gradient_dir, *parts), map_location="cpu", weights_only=False).to(dev, torch.float32)

    train = load("train", f"emb_f=loss_{suffix}")
    train_dtrak = load("train", f"emb_f=mean-squared-l2-norm_{suffix}")
    gen = load("generated", f"emb_f=loss_{suffix}")
    gen_dtrak = load("generated", f"emb_f=mean-squared-l2-norm_{suffix}")
    journey = load("generated_journey", f"emb_f=loss_num_journey_points={args.num_journey_points}"
                                        f"_num_journey_noises={args.num_journey_noises}_proj_dim={args.proj_dim}.pt")
    train_df = pd.read_csv(os.path.join(args.gradient_dir, "train", "group.csv"))
    names = train_df[args.group].to_numpy()
    group_indices = [np.where(names == group_df.iloc[i].item())[0] for i in group_df.index]

    sample = {k: v.cpu().numpy() for k, v in sample_scores(train, train_dtrak, gen, gen_dtrak, journey, args.lam).items()}
    output = group_scores(sample, group_indices)
    output_dir = os.path.join(args.output_dir, "baselines")
    os.makedirs(output_dir, exist_ok=True)
    for name, arr in output.items():
        assert arr.shape == (len(group_indices), 1)
        np.save(os.path.join(output_dir, f"{args.group}_{name}.npy"), arr)
        rank = np.argsort(-arr.mean(axis=-1), kind="stable")
        np.save(os.path.join(output_dir, f"all_generated_images_{args.group}_rank_{name}.npy"), rank)
    return output_dir


if __name__ == "__main__":
    main(parse_args())
    print("Done!")
