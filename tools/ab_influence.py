"""The WoodFisher iteration of influence unlearning, gad_wf_dots + gad_wf_update (csrc/influence.hip), against the plain torch
expression sequence of the reference (src/unlearn/Wfisher.py:203-205: two torch.dot, two scaled subtractions) on the same
vectors, at the CIFAR U-Net's flat parameter count and at the pruned (ratio 0.3) model's; and the whole IU phase of one toy
coalition.  Bytes are the algorithm's: 3 + 2 reads and 2 writes of fp32 = 28 B per parameter per iteration (12 B for the dots
sweep alone, 16 B for the update alone); GB/s = those bytes over the measured time.

Method: device events around `ITERS` back-to-back iterations, after a warm-up of the same shape; `ROUNDS` rounds with the two
versions alternating inside each round; median and min .. max over the rounds are reported.  N is 1e12 in the timed loops so
that the coefficients are ~0 and the vectors keep their magnitudes over thousands of iterations; one iteration with N = 3 from
a common start compares the two versions' results.

Run by hand on the GPU, each step in a process of its own under a time limit:
    timeout -k 10 300 python tools/ab_influence.py --step kernels --out profiles/influence.txt && \\
    timeout -k 10 300 python tools/ab_influence.py --step phase --out profiles/influence.txt
Each step appends its report to --out (the `kernels` step starts the file)."""
import argparse
import os
import statistics
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "group-attribution-for-diffusion-models_amd"))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

dev = torch.device("cuda:0")
ITERS, ROUNDS, WARM = 50, 5, 10
PRUNED = dict(block_out_channels=[96, 192, 192, 192])            # unconditional_generation/prune.py at --pruning_ratio 0.3
LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def flat_count(overrides):
    import gad
    from src.ddpm_config import DDPMConfig
    net = gad.UNet2DModel(**dict(DDPMConfig.cifar_config["unet_config"], **overrides)).to(dev)
    flat, _ = net.flatten_parameters()
    return flat.numel(), sum(p.numel() for p in net.parameters())


def window(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e-3


def alternate(fns):
    """{name: [seconds per call, one per round]} with the versions alternating inside each round"""
    for fn in fns.values():
        window(fn, WARM)
    out = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, fn in fns.items():
            out[k].append(window(fn, ITERS))
    return out


def report(name, ts, nbytes):
    med = statistics.median(ts)
    say(f"  {name:34s} {med * 1e6:9.1f} us  ({min(ts) * 1e6:.1f} .. {max(ts) * 1e6:.1f})   {nbytes / med / 1e9:8.1f} GB/s of {nbytes / 1e6:.0f} MB")
    return med


def kernels_step():
    from gad import ops
    say("WoodFisher iteration: gad_wf_dots + gad_wf_update against the torch expression sequence")
    say(f"device: {torch.cuda.get_device_name(0)}; {ITERS} iterations per window after {WARM} warm-up, {ROUNDS} alternating rounds; "
        "median (min .. max)")
    for label, overrides in (("CIFAR U-Net", {}), ("CIFAR U-Net pruned at ratio 0.3", PRUNED)):
        P, logical = flat_count(overrides)
        torch.cuda.empty_cache()
        gen = torch.Generator(device=dev).manual_seed(0)
        o, k, g = (torch.randn(P, device=dev, generator=gen) / P ** 0.5 for _ in range(3))
        dots = torch.zeros(2, dtype=torch.float64, device=dev)
        N = 1e12

        def gad_iter():
            ops.wf_dots_raw(o, k, g, dots)
            ops.wf_update_raw(o, k, dots, N)

        def torch_iter():
            tmp = torch.dot(o, g)
            k.sub_((torch.dot(k, g) / (N + tmp)) * o)
            o.sub_((tmp / (N + tmp)) * o)
        ops.wf_dots_raw(o, k, g, dots)                               # the stream's workspace is allocated outside the windows
        torch.cuda.synchronize()
        say(f"\n{label}: P = {P} flat (slot-padded; {logical} parameters)")
        ts = alternate({"gad": gad_iter, "torch": torch_iter, "dots": lambda: ops.wf_dots_raw(o, k, g, dots),
                        "update": lambda: ops.wf_update_raw(o, k, dots, N)})
        t_gad = report("gad_wf_dots + gad_wf_update", ts["gad"], 28 * P)
        t_torch = report("torch: 2 dot, 2 scaled subtractions", ts["torch"], 28 * P)
        report("gad_wf_dots alone (12 B/param)", ts["dots"], 12 * P)
        report("gad_wf_update alone (16 B/param)", ts["update"], 16 * P)
        say(f"  torch / gad = {t_torch / t_gad:.2f}x (the torch sequence's own traffic is larger than 28 B/param: its GB/s column "
            "is the algorithm's bytes over its time, not what it moved)")
        # one iteration with N = 3 from a common start: the two versions' results
        o0, k0 = o.clone(), k.clone()
        N = 3.0
        gad_iter()
        og, kg = o.clone(), k.clone()
        o.copy_(o0)
        k.copy_(k0)
        torch_iter()
        say(f"  one iteration, N = 3: |k_gad - k_torch| / |k| = {float((kg - k).norm() / k.norm()):.2e}, "
            f"|o_gad - o_torch| / |o| = {float((og - o).norm() / o.norm()):.2e};  dots = {dots.tolist()} (fp64) "
            f"against torch.dot fp32 {float(torch.dot(o0, g)):.9e}, {float(torch.dot(k0, g)):.9e}")
        del o, k, g, o0, k0, og, kg


def phase_step():
    import gad
    from src.datasets import create_dataset
    from src.ddpm_config import DDPMConfig
    from unconditional_generation import unlearn
    say("\nThe IU phase of one toy coalition: toy2 (128 images, 2 groups), Shapley seed 1, the full-width CIFAR U-Net, batches of 16")
    config = dict(DDPMConfig.cifar100_config, batch_size=16)
    dataset = create_dataset(dataset_name="toy2", train=True)
    args = types.SimpleNamespace(removal_dist="shapley", removal_seed=1, iu_ratio=0.5, device=dev)
    remaining_idx, removed_idx = unlearn.coalition(args, dataset)
    for attempt in ("first (cold: code objects, workspace, shadows)", "second"):
        gad.seed_everything(42)
        model = gad.UNet2DModel(**config["unet_config"]).to(dev)
        ema = gad.EMAModel(model.parameters())
        ema.to(dev)
        scheduler = gad.DDPMScheduler(**config["scheduler_config"])
        torch.cuda.synchronize()
        t0 = time.time()
        steps = unlearn.influence_unlearn(args, gad, config, dataset, model, ema, scheduler, remaining_idx, removed_idx)
        torch.cuda.synchronize()
        dt = time.time() - t0
        batches = -(-len(removed_idx) // 16) + 2 * steps
        say(f"  {attempt}: {dt * 1e3:9.1f} ms for {batches} forward / backward passes of <= 16 images and {steps - 1} WoodFisher iterations "
            f"(len(remaining loader) = {steps}); host clock around a device synchronise")
        del model, ema
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["kernels", "phase"], required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "influence.txt"))
    a = ap.parse_args()
    {"kernels": kernels_step, "phase": phase_step}[a.step]()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w" if a.step == "kernels" else "a") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
