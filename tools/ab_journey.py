"""Journey-TRAK: the fused ancestral DDPM step (csrc/sampler.hip) against gad.DDPMScheduler.step's torch path, and a whole
journey_latents on the CIFAR U-Net.  One process:

  step      ops.ddpm_step_raw (one launch, noise generated in the kernel) against gad.DDPMScheduler.step (about a dozen
            elementwise torch launches and a torch.randn) on [64][3][32][32] and [1024][3][32][32], t = 500, stride 10,
            CIFAR's scheduler (fixed_large, clip 1).  Bytes are the algorithm's: x and eps read, x_prev written, 12 B per
            element; GB/s = those bytes over the measured time, next to the fraction of the 6.3 TB/s a float4 copy reaches.
            At 64 rows the tensor is 0.8 MB (2.4 MB moved): both versions are launch-bound there and the figure is a launch
            count, not a bandwidth.
  journey   gad.trak.journey_latents(n_samples = 64, k_partition = 100) on the CIFAR U-Net: 99 U-Net forwards at batch 64 and
            99 steps, host clock around the call (it ends in a device-to-host copy), and the steps' share of it (their time in
            isolation over the call's time).

Method: device events around `ITERS` back-to-back calls after a warm-up of the same shape; `ROUNDS` rounds with the two versions
alternating inside each round; median and min .. max over the rounds.  The two versions do not compute equal numbers (the torch
path draws its noise from torch's generator); tests/test_gpu_journey.py holds the kernel to the fp64 restatement.

Run by hand on the GPU under a time limit:
    timeout -k 10 300 python tools/ab_journey.py --out profiles/journey_ab.txt"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "group-attribution-for-diffusion-models_amd"))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

dev = torch.device("cuda:0")
ITERS, ROUNDS, WARM = 500, 5, 20
HBM = 6.3e12                                                     # what a float4 copy reaches on the MI355X
LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def window(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e-3


def alternate(fns, iters=ITERS, warm=WARM):
    for fn in fns.values():
        window(fn, warm)
    out = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, fn in fns.items():
            out[k].append(window(fn, iters))
    return out


def report(name, ts, nbytes=None):
    med = statistics.median(ts)
    tail = f"   {nbytes / med / 1e9:8.1f} GB/s of {nbytes / 1e6:.1f} MB = {nbytes / med / HBM * 100:.1f} % of the HBM roof" if nbytes else ""
    say(f"  {name:44s} {med * 1e6:10.1f} us  ({min(ts) * 1e6:.1f} .. {max(ts) * 1e6:.1f}){tail}")
    return med


def step_pair(B, sch, t=500):
    from gad import ops
    gen = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(B, 3, 32, 32, device=dev, generator=gen)
    eps = torch.randn(B, 3, 32, 32, device=dev, generator=gen)
    out = torch.empty_like(x)
    seeds = torch.arange(B, device=dev, dtype=torch.int64) + (42 << 32)
    c = sch.config
    stride = c.num_train_timesteps // sch.num_inference_steps
    a_t, a_p = sch.alphas_cumprod[t].item(), sch.alphas_cumprod[t - stride].item()
    clip = float(c.clip_sample_range) if c.clip_sample else 0.0

    def fused():
        ops.ddpm_step_raw(x, eps, seeds, t, a_t, a_p, clip, c.variance_type, out=out)

    def torch_path():
        sch.step(eps, t, x)
    return fused, torch_path, 12 * x.numel()


def step_ab(sch):
    say("Ancestral DDPM step: gad_ddpm_step (one launch, in-kernel Philox noise) against gad.DDPMScheduler.step (torch)")
    say(f"device: {torch.cuda.get_device_name(0)}; {ITERS} calls per window after {WARM} warm-up, {ROUNDS} alternating rounds; median (min .. max)")
    per_step = {}
    for B in (64, 1024):
        fused, torch_path, nbytes = step_pair(B, sch)
        say(f"\n[{B}][3][32][32], t = 500 -> 490, {sch.config.variance_type}, clip {sch.config.clip_sample_range}")
        ts = alternate({"fused": fused, "torch": torch_path})
        f = report("gad_ddpm_step", ts["fused"], nbytes)
        t = report("DDPMScheduler.step (torch elementwise + randn)", ts["torch"], nbytes)
        say(f"  torch / fused = {t / f:.2f}x")
        per_step[B] = f
    return per_step


def journey(sch, step_s):
    import gad
    from gad.trak import journey_latents, journey_timesteps
    from src.ddpm_config import DDPMConfig
    torch.manual_seed(0)
    net = gad.UNet2DModel(**DDPMConfig.cifar_config["unet_config"]).to(dev)
    n, k = 64, 100
    K = len(journey_timesteps(k))
    say(f"\njourney_latents(n_samples = {n}, k_partition = {k}) on the CIFAR U-Net: {K - 1} forwards at batch {n} and {K - 1} steps")
    journey_latents(net, sch, n, k, device=dev)                   # warm-up: code objects, workspaces, derived weights
    ts = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        journey_latents(net, sch, n, k, device=dev)
        ts.append(time.perf_counter() - t0)
    med = statistics.median(ts)
    say(f"  whole call (host clock, ends in the device-to-host copy) {med * 1e3:10.1f} ms  ({min(ts) * 1e3:.1f} .. {max(ts) * 1e3:.1f})"
        f" = {med / (K - 1) * 1e3:.2f} ms per visited timestep")
    say(f"  its {K - 1} gad_ddpm_step launches, in isolation: {(K - 1) * step_s * 1e3:.2f} ms = {100 * (K - 1) * step_s / med:.2f} % of the call")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "journey_ab.txt"))
    a = ap.parse_args()
    import gad
    from src.ddpm_config import DDPMConfig
    sch = gad.DDPMScheduler(**DDPMConfig.cifar_config["scheduler_config"])
    sch.num_inference_steps = 100                                 # the reference's posterior stride (d_trak_grad.py:455-456)
    per_step = step_ab(sch)
    journey(sch, per_step[64])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
