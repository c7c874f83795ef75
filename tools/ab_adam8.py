"""A/B of the optimizer pass: fused clip + 8-bit blockwise Adam + EMA (gad_clip_adam8_ema) against the fp32 pass
(gad_clip_adam_ema), same process, alternating, each with its gad_sumsq launch and the EMA update included.

Sizes: 35.75 M parameters (the CIFAR U-Net) and 274 M (the CelebA LDM U-Net), as ONE parameter each - every block full, which is
what the large convolutions that hold nearly all of a U-Net's parameters give.  Reports device-event time per step and the share
of the HBM roof (6.3 TB/s achievable) at the passes' algorithmic bytes: 24 B per parameter (8-bit) and 36 B (fp32), plus the 4 B
per parameter gad_sumsq reads in both.  Needs a GPU; prints the report (profiles/adam8_ab.txt keeps one).

    python tools/ab_adam8.py [--sizes 35750000,274000000] [--iters 20]"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "group-attribution-for-diffusion-models_amd"))

HBM_ROOF = 6.3e12      # bytes / s achievable on an MI355X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="35750000,274000000")
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ab_adam8: needs a GPU (a timing taken anywhere else says nothing)")
    from gad import ops
    from gad.training import adam8_blocks
    dev = torch.device("cuda:0")
    print(f"device: {torch.cuda.get_device_name(dev)}")
    hp = dict(max_norm=1.0, lr=1e-4, betas=(0.9, 0.999), eps=1e-8)
    for n in (int(s) for s in a.sizes.split(",")):
        n = n // 8 * 8
        gen = torch.Generator(device=dev).manual_seed(0)
        p = torch.randn(n, device=dev, generator=gen)
        g = torch.randn(n, device=dev, generator=gen) * 1e-3
        ema, ss = p.clone(), torch.zeros(1, device=dev)
        m, v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
        lay = adam8_blocks([torch.empty(n, device="meta")], 1e-6)
        s1, s2 = torch.full((n,), 127, dtype=torch.uint8, device=dev), torch.zeros(n, dtype=torch.uint8, device=dev)
        a1, a2 = torch.zeros(lay.n_absmax, device=dev), torch.zeros(lay.n_absmax, device=dev)
        m32, v32 = torch.zeros(8, device=dev), torch.zeros(8, device=dev)
        blocks = torch.from_numpy(lay.table.view("u1").copy()).to(dev)
        step = [0]

        def fp32():
            ops.sumsq_raw(g, out=ss)
            ops.clip_adam_ema_raw(p, g, m, v, ema, ss, weight_decay=1e-6, adamw=True, step=step[0], ema_decay=0.9999, **hp)

        def bits8():
            ops.sumsq_raw(g, out=ss)
            ops.clip_adam8_ema_raw(p, g, ema, s1, s2, a1, a2, m32, v32, blocks, ss, step=step[0], ema_decay=0.9999, **hp)

        times = {"fp32": [], "8-bit": []}
        for it in range(3 + a.iters):                      # three warm-up rounds, then alternate
            for name, fn in (("fp32", fp32), ("8-bit", bits8)):
                step[0] = it + 1
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                if it >= 3:
                    times[name].append(e0.elapsed_time(e1) * 1e-3)
        print(f"\n{n / 1e6:.2f} M parameters, {lay.n_absmax} blocks, {a.iters} alternating steps (sumsq + optimizer + EMA):")
        for name, per in (("fp32", 36 + 4), ("8-bit", 24 + 4)):
            t = sorted(times[name])
            med = t[len(t) // 2]
            print(f"  {name:5s}: median {med * 1e3:8.3f} ms  (min {t[0] * 1e3:.3f}, max {t[-1] * 1e3:.3f})  {per} B/param -> "
                  f"{n * per / med / 1e12:5.2f} TB/s = {100 * n * per / med / HBM_ROOF:5.1f} % of the {HBM_ROOF / 1e12:.1f} TB/s HBM roof")
        f, e = sorted(times["fp32"])[a.iters // 2], sorted(times["8-bit"])[a.iters // 2]
        print(f"  8-bit / fp32 time: {e / f:.3f}   state: {(2 * n + 8 * lay.n_absmax) / 1e9:.3f} GB against {8 * n / 1e9:.3f} GB")
        assert torch.isfinite(p).all()
        del p, g, ema, m, v, s1, s2
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
