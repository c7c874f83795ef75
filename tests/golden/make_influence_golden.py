"""Golden vector for influence unlearning by RUNNING THE REFERENCE'S OWN FUNCTIONS on CPU (build container only):
  src/unlearn/Wfisher.py   get_grad (:37-122), woodfisher_diff (:125-207)
loaded from the reference by path, called in the order and with the two weightings of unconditional_generation/unlearn.py:518-541
(removed loader, then remaining loader; retain_grad *= f / ((f + r) r); forget_grad /= f + r; woodfisher_diff(N = r)), with
args.by_class = True as `--removal_dist shapley` sets it (:331-335).  Nothing of the reference's is defined here: the model, the
scheduler stand-in (tests/influence_ref.py) and the loaders (lists of (image, label) batches) are its inputs.  While it runs,
every torch.randn_like / torch.randint draw it makes is recorded, so the test side can replay the same noise and timesteps.
Run:  python tests/golden/make_influence_golden.py   ->  tests/golden/influence.npz
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))

from influence_ref import ToyEps, ToyScheduler  # noqa: E402

N_IMAGES, N_LABELS, BATCH = 40, 5, 8
REMOVED_LABELS = (0, 1)


def main():
    spec = importlib.util.spec_from_file_location("ref_wfisher", os.path.join(REF, "src", "unlearn", "Wfisher.py"))
    W = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(W)

    torch.manual_seed(20240)
    model = ToyEps()
    with torch.no_grad():
        for p in model.parameters():
            p.mul_(1.5)                                   # away from the initialisation's small outputs
    scheduler = ToyScheduler()
    g = torch.Generator().manual_seed(7)
    images = torch.randn(N_IMAGES, 3, 8, 8, generator=g).clamp_(-1, 1)
    labels = torch.arange(N_IMAGES) % N_LABELS
    removed_idx = torch.nonzero(torch.isin(labels, torch.tensor(REMOVED_LABELS))).flatten()
    remaining_idx = torch.nonzero(~torch.isin(labels, torch.tensor(REMOVED_LABELS))).flatten()

    def shuffled(idx):                                    # one epoch of a shuffled loader: index batches of BATCH
        return idx[torch.randperm(len(idx), generator=g)].view(-1, BATCH)
    removed_batches, remaining_batches, wf_batches = shuffled(removed_idx), shuffled(remaining_idx), shuffled(remaining_idx)

    def loader(batches):
        return [(images[b], labels[b]) for b in batches]

    noise, half_t = [], []
    randn_like, randint = torch.randn_like, torch.randint

    def rec_randn_like(x, *a, **k):
        out = randn_like(x, *a, **k)
        noise.append(out.clone())
        return out

    def rec_randint(*a, **k):
        out = randint(*a, **k)
        half_t.append(out.clone())
        return out

    args = types.SimpleNamespace(dataset="toy", precompute_stage=None, by_class=True)
    pipeline = types.SimpleNamespace(unet=model, device=torch.device("cpu"), scheduler=scheduler)
    torch.randn_like, torch.randint = rec_randn_like, rec_randint
    try:
        forget_count, forget_grad = W.get_grad(args, loader(removed_batches), pipeline)
        retain_count, retain_grad = W.get_grad(args, loader(remaining_batches), pipeline)
        retain_grad *= forget_count / ((forget_count + retain_count) * retain_count)
        forget_grad /= forget_count + retain_count
        delta_w = W.woodfisher_diff(args, retain_count, loader(wf_batches), pipeline, forget_grad - retain_grad)
    finally:
        torch.randn_like, torch.randint = randn_like, randint
    n_batches = len(removed_batches) + len(remaining_batches) + len(wf_batches)
    assert len(noise) == len(half_t) == n_batches
    out = {f"weight.{k}": v.numpy() for k, v in model.state_dict().items()}
    out.update(images=images.numpy(), labels=labels.numpy(), removed_batches=removed_batches.numpy(),
               remaining_batches=remaining_batches.numpy(), wf_batches=wf_batches.numpy(),
               noise=torch.stack(noise).numpy(), half_timesteps=torch.stack(half_t).numpy(),
               forget_count=np.int64(forget_count), retain_count=np.int64(retain_count),
               forget_grad=forget_grad.detach().numpy(), retain_grad=retain_grad.detach().numpy(), delta_w=delta_w.detach().numpy())
    path = os.path.join(OUT, "influence.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, P = {delta_w.numel()}, counts ({forget_count}, {retain_count}), "
          f"|delta_w| = {delta_w.norm():.6e}, |F - R| = {(forget_grad - retain_grad).norm():.6e}")


if __name__ == "__main__":
    main()
