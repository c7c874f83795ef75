"""Latent draws for the SD LoRA step: gad_latent_draw (csrc/latent.hip) against the same draw in torch ops and against encoding
the step's images, and the accuracy of the kernel's std = expf(0.5 logvar).  One process:

  draw      MomentSource.draw (one launch: gather, flip coin, in-kernel Philox noise, scale) at B = 64, n = 4 x 32 x 32 = 4096,
            N = 5000 rows of both orientations (0.33 GB resident), against the same draw in torch ops: index_select of the rows'
            two slabs, where on a random coin, clamp, exp, randn, mul, add.  Bytes are the algorithm's: mean and logvar read,
            x0 written, 12 B per element = 3.1 MB per launch: both versions are enqueue-bound there and the figure is a launch
            count, not a bandwidth (none is claimed).
  encode    what an encode per step would cost instead: gad_pixels_to_nchw + gad.AutoencoderKL.encode_moments of the same 64
            images at 256 x 256 on the SD VAE (seeded weights: the time does not depend on their values).
  std       the kernel's std against fp64.  ROCm's installed HIP documentation states no ulp bound for expf, so
            tests/test_gpu_latents.py takes twice the maximum observed here.  Two draws of the same (seed, row, step) on F = 1
            moments with mean 0, scale 1: logvar 0 gives z' = fl(1 * z) = the kernel's own z, logvar lv gives fl(std' z'), so
            |fl(std' z') / z' - std| / std over lv in [-30, 20] (and clamped beyond) bounds expf's relative error plus the
            product's one rounding (2^-24).  Reported in units of 2^-23.

Method: device events around `ITERS` back-to-back calls after a warm-up of the same shape; `ROUNDS` rounds with the versions
alternating inside each round; median and min .. max over the rounds.  The two draws do not compute equal numbers (the torch
path draws from torch's generator); tests/test_gpu_latents.py holds the kernel to the fp64 restatement.

Run by hand on the GPU under a time limit:
    timeout -k 10 300 python tools/ab_latents.py --out profiles/latents_ab.txt"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "group-attribution-for-diffusion-models_amd"))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

dev = torch.device("cuda:0")
ITERS, ROUNDS, WARM = 500, 5, 20
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


def report(name, ts, unit=1e6, suffix="us"):
    med = statistics.median(ts)
    say(f"  {name:64s} {med * unit:10.1f} {suffix}  ({min(ts) * unit:.1f} .. {max(ts) * unit:.1f})")
    return med


def draw_ab(N=5000, B=64, L=4, hw=32):
    import gad
    n = L * hw * hw
    say("Latent draw: gad_latent_draw (one launch) against the same draw in torch ops")
    say(f"device: {torch.cuda.get_device_name(0)}; {ITERS} calls per window after {WARM} warm-up, {ROUNDS} alternating rounds; median (min .. max)")
    say(f"\nmoments [{N}][2][{2 * L}][{hw}][{hw}] fp32 = {N * 2 * 2 * n * 4 / 1e9:.2f} GB resident, B = {B}, n = {n}: "
        f"{12 * B * n / 1e6:.1f} MB per launch at 12 B per element")
    gen = torch.Generator(device=dev).manual_seed(0)
    moments = torch.randn(N, 2, 2 * L, hw, hw, device=dev, generator=gen)
    src = gad.MomentSource(moments, 0.18215, seed=1)
    rows = torch.randperm(N, device=dev, generator=gen)[:B].contiguous()
    out = torch.empty(B, L, hw, hw, device=dev)
    step = [0]

    def fused():
        step[0] += 1
        src.draw(rows, step[0], sample=True, random_flip=True, out=out)

    def mode():
        src.draw(rows, 0, sample=False, random_flip=False, out=out)

    def torch_path():
        plain, flipped = moments[:, 0], moments[:, 1]
        a, b = plain.index_select(0, rows), flipped.index_select(0, rows)
        coin = torch.rand(B, 1, 1, 1, device=dev) < 0.5
        m = torch.where(coin, b, a)
        mean, logvar = m[:, :L], m[:, L:]
        std = torch.exp(0.5 * torch.clamp(logvar, -30.0, 20.0))
        return (mean + std * torch.randn(mean.shape, device=dev)) * 0.18215

    ts = alternate({"fused": fused, "mode": mode, "torch": torch_path})
    f = report("gad_latent_draw, sample + random flip", ts["fused"])
    report("gad_latent_draw, mode (scale * mean, no Philox)", ts["mode"])
    t = report("torch: 2 index_select, rand, where, clamp, exp, randn, mul, add", ts["torch"])
    say(f"  torch / fused = {t / f:.2f}x")
    del moments, src
    torch.cuda.empty_cache()
    return f


def encode_ab(draw_s, B=64, res=256):
    import gad
    from gad import ops
    from gad.similarity import pixel_lut
    from gad.vae import sd_vae_config
    say(f"\nEncoding the same {B} images per step instead: gad_pixels_to_nchw + AutoencoderKL.encode_moments at {res} x {res} (SD VAE, seeded)")
    vae = gad.AutoencoderKL.seeded(sd_vae_config(), 1).to(dev)
    px = torch.randint(0, 256, (B, res, res, 3), dtype=torch.uint8, device=dev)
    lut = torch.from_numpy(pixel_lut()).to(dev)

    def encode():
        vae.encode_moments(ops.pixels_to_nchw_raw(px, lut, flip=False))

    def to_nchw():
        ops.pixels_to_nchw_raw(px, lut, flip=True)

    encode()                                                        # warm-up: code objects, workspaces, derived weights
    torch.cuda.synchronize()
    ts = [window(encode, 1) for _ in range(3)]
    e = report(f"encode_moments of {B} images", ts, 1e3, "ms")
    report(f"gad_pixels_to_nchw of {B} images (flipped), alone", [window(to_nchw, 50) for _ in range(3)])
    say(f"  an encode per step = {e / draw_s:.0f} draws")


def std_accuracy():
    from gad import ops
    say("\nstd = expf(0.5 * clamp(logvar, -30, 20)) in the kernel against fp64, through fl(std' z') / z' (see the docstring)")
    n = 1 << 16
    lv = torch.linspace(-34.0, 24.0, n, dtype=torch.float64).to(torch.float32)
    lv[::7] = torch.empty(len(lv[::7])).uniform_(-30.0, 20.0, generator=torch.Generator().manual_seed(0))
    worst = 0.0
    for row, step in ((0, 1), (0, 2), (0, 3)):
        rows = torch.tensor([row], dtype=torch.int64, device=dev)
        unit = torch.zeros(1, 1, 2, n, 1, device=dev)
        test = unit.clone()
        test[0, 0, 1, :, 0] = lv.to(dev)
        z = ops.latent_draw_raw(unit, rows, 11, step, 1.0).flatten().cpu().double().numpy()
        p = ops.latent_draw_raw(test, rows, 11, step, 1.0).flatten().cpu().double().numpy()
        std = np.exp(0.5 * np.clip(lv.double().numpy(), -30.0, 20.0))
        keep = np.abs(z) > 1e-3
        rel = np.abs(p[keep] / z[keep] - std[keep]) / std[keep] / 2.0 ** -23
        worst = max(worst, rel.max())
        say(f"  step {step}: {keep.sum()} elements, max |std' - std| / std = {rel.max():.3f} x 2^-23 (mean {rel.mean():.3f})")
    say(f"  observed maximum {worst:.3f} x 2^-23, the product's rounding included; tests/test_gpu_latents.py takes twice that, "
        f"{2 * worst:.3f} x 2^-23, rounded up, as expf's share of k")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "latents_ab.txt"))
    ap.add_argument("--skip_encode", action="store_true")
    a = ap.parse_args()
    d = draw_ab()
    if not a.skip_encode:
        encode_ab(d)
    std_accuracy()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
