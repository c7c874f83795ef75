"""Forward time of the GroupNorm launches whose statistics were centred (profiles/gn_conditioning.txt): the fp32 two-pass
plan at the 64x64 levels of the SD and CelebA-HQ U-Nets, its two-source form, and the bf16-storage GroupNorm of the SD step.
usage: python tools/gn_conditioning_ab.py [--lib /path/to/another/libgad_hip.so] [--runs 5]
A/B against another build: run it alternately with and without --lib; every run prints one line per launch.
--offset M times inputs of mean M, std 1: randn (M = 0) never takes the second, centred sweep; M = 30 takes it in every chunk."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "group-attribution-for-diffusion-models_amd"))
sys.path.insert(0, ROOT)
os.environ.setdefault("GAD_OUTDIR", "/tmp/_out")
ap = argparse.ArgumentParser()
ap.add_argument("--lib", default=None)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--tag", default="")
ap.add_argument("--offset", type=float, default=0.0, help="mean of the inputs (std 1): 30 sends every chunk through the second, centred sweep")
args = ap.parse_args()
from gad import _capi
if args.lib:
    _capi.LIB_PATH = os.path.abspath(args.lib)
import torch
from gad import half, ops

dev = torch.device("cuda:0")


def timeit(fn, iters=50, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3          # us


def launches():
    for B, H, C in ((16, 64, 320), (64, 64, 224)):
        x, g, b = torch.randn(B, H, H, C, device=dev) + args.offset, torch.randn(C, device=dev), torch.randn(C, device=dev)
        yield f"fp32 [{B},{H},{H},{C}]", 8 * x.numel(), lambda x=x, g=g, b=b: ops.group_norm(x, g, b, 32, 1e-5, True)
    x, x2 = torch.randn(16, 64, 64, 640, device=dev) + args.offset, torch.randn(16, 64, 64, 320, device=dev) + args.offset
    g, b = torch.randn(960, device=dev), torch.randn(960, device=dev)
    yield "fp32 [16,64,64,640|320]", 8 * (x.numel() + x2.numel()), lambda: ops.group_norm_cat_raw(x, x2, g, b, 32, 1e-5, True)
    for B, HW, C in ((16, 4096, 320), (16, 1024, 640)):
        xh = (torch.randn(B, HW, C, device=dev) + args.offset).to(torch.bfloat16)
        g, b = torch.randn(C, device=dev), torch.randn(C, device=dev)
        yield f"bf16 [{B},{HW},{C}]", 4 * xh.numel(), lambda xh=xh, g=g, b=b: half.group_norm_raw(xh, None, g, b, 32, 1e-5, True)


with torch.no_grad():
    for name, nbytes, fn in launches():
        t = sorted(timeit(fn) for _ in range(args.runs))
        med = t[len(t) // 2]
        print(f"{args.tag:8s} {name:26s} median {med:8.1f} us  min {t[0]:8.1f}  max {t[-1]:8.1f}  {nbytes / med / 1e3:6.0f} GB/s", flush=True)
