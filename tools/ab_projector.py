"""gad_jl_project (R generated on the fly, f32 MFMA) against the plain baseline (R generated in P-chunks with torch.randn,
then torch.matmul) at the CIFAR U-Net's gradient length P = 35.75 M, and the TRAK feature rate of the CIFAR U-Net at k = 10.
Which pipe bounds a shape: the MFMA bound is the issued f32 MFMA work (rows padded to 16 per M block) at the 157.3 TFLOP/s
peak; the generator's time is the G = 1 launch (its MFMA share is small); a launch near the generator time is bound by the
generator (VALU: Philox, Box-Muller), one near the sum of the two is serialised (the pipes do not overlap).  usage (GPU box): python tools/ab_projector.py"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "group-attribution-for-diffusion-models_amd"))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
from gad.trak import project_raw, workspace_bytes  # noqa: E402

dev = torch.device("cuda:0")
P = 35_750_000
PEAK_F32_MFMA = 157.3e12


def timeit(fn, iters=3, warm=1):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e-3


def baseline(a, d, chunk=1 << 18):
    out = torch.zeros(a.shape[0], d, device=dev)
    g = torch.Generator(device=dev).manual_seed(0)
    for p in range(0, P, chunk):
        e = min(P, p + chunk)
        out += a[:, p:e] @ torch.randn(e - p, d, device=dev, generator=g)
    return out


def issued_rows(G):
    mb = 1 if G <= 16 else 2 if G <= 32 else 4
    return 16 * mb * ((G + 63) // 64) if G > 64 else 16 * mb


def main():
    print(f"P = {P}; times are means of 3 launches after 1 warm-up")
    a_all = torch.randn(64, P, device=dev) / P ** 0.5
    times = {}
    print(f"{'type':10s} {'d':>5s} {'G':>3s} {'ms':>9s} {'R entries/s':>12s} {'Philox/s':>10s} {'MFMA useful':>11s} "
          f"{'MFMA issued':>11s} {'MFMA-bound ms':>13s}  bound")
    for proj_type in ("normal", "rademacher"):
        for d in (1024, 4096):
            for G in (1, 8, 32, 64):
                a = a_all[:G]
                out = torch.empty(G, d, device=dev)
                ws = torch.empty(workspace_bytes(G, P, d, proj_type), dtype=torch.uint8, device=dev)
                t = timeit(lambda: project_raw(a, out, P, 42, 0, proj_type, workspace=ws))
                times[(proj_type, d, G)] = t
                useful = 2.0 * G * P * d / t / PEAK_F32_MFMA
                issued = 2.0 * issued_rows(G) * P * d / t / PEAK_F32_MFMA
                mfma_ms = 2.0 * issued_rows(G) * P * d / PEAK_F32_MFMA * 1e3
                calls = P * d / 4 / t                # calls issued: one per lane per row per 64-column tile (4 entries used)
                t_gen = times[(proj_type, d, 1)]
                if t < 1.15 * t_gen:
                    bound = "generator (VALU)"
                elif t > 0.85 * (t_gen + mfma_ms * 1e-3):
                    bound = "generator + MFMA serialised"
                else:
                    bound = "generator + MFMA, part overlapped"
                print(f"{proj_type:10s} {d:5d} {G:3d} {t * 1e3:9.2f} {P * d / t:12.3e} {calls:10.3e} {useful:11.3f} "
                      f"{issued:11.3f} {mfma_ms:13.2f}  {bound}")
    print("\nbaseline: torch.randn R chunks of 262144 rows + torch.matmul (normal entries)")
    for d in (1024, 4096):
        for G in (1, 64):
            a = a_all[:G]
            t = timeit(lambda: baseline(a, d), iters=2)
            print(f"baseline   {d:5d} {G:3d} {t * 1e3:9.2f} ms   gad_jl_project is {t / times[('normal', d, G)]:.1f}x faster")

    # TRAK features of the CIFAR U-Net at k = 10: one fused forward / backward over the image's 10 (noisy, t) rows + 1/G of
    # a projection launch
    import gad
    from gad.trak import _GradStep, selected_timesteps
    from src.ddpm_config import DDPMConfig
    del a_all
    torch.cuda.empty_cache()
    net = gad.UNet2DModel(**DDPMConfig.cifar_config["unet_config"]).to(dev)
    step = _GradStep(net, gad.DDPMScheduler(**DDPMConfig.cifar_config["scheduler_config"]), "mean-squared-l2-norm")
    ts = torch.tensor(selected_timesteps("uniform", 10), device=dev)
    x = torch.rand(1, 3, 32, 32, device=dev).expand(10, 3, 32, 32).contiguous()
    n = torch.randn(10, 3, 32, 32, device=dev)
    t_fb = timeit(lambda: step(x, n, ts), iters=10, warm=3)
    print(f"\nCIFAR U-Net: P = {step.gflat.numel()} (flat, slot-padded), fwd/bwd of one image's k = 10 rows {t_fb * 1e3:.2f} ms")
    for proj_type in ("normal", "rademacher"):
        for d in (1024, 4096):
            for G in (8, 32, 64):
                t = t_fb + times[(proj_type, d, G)] / G
                print(f"features/s {proj_type:10s} d={d:5d} G={G:3d}: {1 / t:8.1f}  (projection share {times[(proj_type, d, G)] / G / t:.0%})")


if __name__ == "__main__":
    main()
