"""Speed of the local model behaviours on the full-width CIFAR U-Net: (A) gad.local_model_behaviors against (B) the
reference-shaped loop of tests/local_ref.py on the same gad pipelines (batch-1 trajectories, 100-row loss batches - only calls
older than A, so B is the baseline).  n_samples 4, n_noises 50, 100 steps; every launch shape is warmed first, then A and B
alternate `--repeats` times in one process under a device-synchronised host clock.  B skips the pure-python image metrics (the
reference calls scikit-image there), which favours B.  Prints seconds per image of both, their spread and the ratio, and
A at other `rows_per_launch` values; `--only a` runs A alone (for a rocprofv3 --kernel-trace --stats run).
usage (GPU box): python tools/local_scores_bench.py [--only a] [--out profiles/local_scores.txt]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "group-attribution-for-diffusion-models_amd"), ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import torch  # noqa: E402

import gad  # noqa: E402
from local_ref import local_behaviors_loop  # noqa: E402
from src.ddpm_config import DDPMConfig  # noqa: E402

dev = torch.device("cuda:0")


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n_samples", type=int, default=4)
    ap.add_argument("--n_noises", type=int, default=50)
    ap.add_argument("--num_inference_steps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only", choices=["a"], default=None)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    n, k, T = args.n_samples, args.n_noises, args.num_inference_steps
    pipes = []
    for seed in (0, 1):
        torch.manual_seed(seed)
        net = gad.UNet2DModel(**DDPMConfig.cifar100_config["unet_config"]).to(dev).eval()
        pipes.append(gad.DDPMPipeline(net, gad.DDIMScheduler()))
    full_pipe, pipe = pipes
    lines = [f"local model behaviours, full-width CIFAR U-Net, n_samples={n} n_noises={k} steps={T} ({torch.cuda.get_device_name(0)})"]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def run_a(rpl=1000):
        return gad.local_model_behaviors(full_pipe, pipe, n, k, T, rows_per_launch=rpl)

    def run_b():
        return local_behaviors_loop(full_pipe, pipe, n, k, T, with_metrics=False)
    # warm-up of every launch shape (hipGraph capture of the batch-1 pipeline, workspaces, Winograd weights)
    gad.local_model_behaviors(full_pipe, pipe, n, 10, T)
    if args.only == "a":
        t, r = clock(run_a)
        say(f"A alone: {t / n:.3f} s/image, loss launches of {sorted(set(r.launch_rows))} rows")
        return
    local_behaviors_loop(full_pipe, pipe, 1, 2, T, with_metrics=False)
    ta, tb = [], []
    for _ in range(args.repeats):
        t, ra = clock(run_a)
        ta.append(t / n)
        t, rb = clock(run_b)
        tb.append(t / n)
    worst = max(abs(x - y) / abs(y) for x, y in zip(ra["diffusion_loss"], rb["diffusion_loss"]))
    say(f"A gad.local_model_behaviors  s/image: {' '.join(f'{x:.3f}' for x in ta)}   min {min(ta):.3f}  spread {max(ta) - min(ta):.3f}")
    say(f"B reference-shaped loop      s/image: {' '.join(f'{x:.3f}' for x in tb)}   min {min(tb):.3f}  spread {max(tb) - min(tb):.3f}")
    say(f"B / A = {min(tb) / min(ta):.2f}   (diffusion losses of A and B, each on its own full images, differ by at most {worst:.1e} relative)")
    say(f"100 x the per-image figures of this {n}-image run: A {100 * min(ta):.0f} s per coalition, B {100 * min(tb):.0f} s "
        "(measured at 100 samples: --only a --n_samples 100)")
    for rpl in (T, 500, 1000, 2000):
        run_a(rpl)
        ts = [clock(lambda: run_a(rpl))[0] / n for _ in range(2)]
        say(f"A with rows_per_launch={rpl:5d}: {min(ts):.3f} s/image")
    full = gad.local_model_behaviors(full_pipe, pipe, n, 1, T, return_images=True)["full_images"]
    ts = [clock(lambda: gad.local_model_behaviors(None, pipe, n, k, T, full_images=full))[0] / n for _ in range(2)]
    say(f"A with the full model's images passed in (full_images=): {min(ts):.3f} s/image")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
