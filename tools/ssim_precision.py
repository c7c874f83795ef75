"""Where the 1e-10 SSIM bound of tests/test_gpu_local_scores.py comes from: a numpy emulation of gad_image_metrics' arithmetic
(fp32 pixels, five separable window sums, skimage's covariance form) against the fp64 loop oracle (oracle/skimage_ref.py), with
the products and the sums in fp64 (what csrc/local.hip does), with fp32 products and fp64 sums, and all in fp32.  The worst
case is the "bright" pair (small variance beside a mean near 1).  CPU only; prints the running maxima per image size.
usage: python tools/ssim_precision.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.skimage_ref import ssim_loops  # noqa: E402


def ssim_k(a, b, win=7, dr=1.0, prod=np.float64, acc=np.float64):
    """kernel arithmetic: fp32 inputs, products in `prod`, window sums / SSIM map / mean in `acc`"""
    H, W, C = a.shape
    NP = win * win
    C1, C2 = acc((0.01 * dr) ** 2), acc((0.03 * dr) ** 2)
    out = []
    for c in range(C):
        x, y = a[..., c].astype(np.float32), b[..., c].astype(np.float32)

        def box(p):
            p = p.astype(acc)
            r = np.zeros((H, W - win + 1), acc)
            for k in range(win):
                r = (r + p[:, k:k + W - win + 1]).astype(acc)
            s = np.zeros((H - win + 1, W - win + 1), acc)
            for k in range(win):
                s = (s + r[k:k + H - win + 1]).astype(acc)
            return (s / acc(NP)).astype(acc)
        xp, yp = x.astype(prod), y.astype(prod)
        ux, uy = box(x), box(y)
        uxx, uyy, uxy = box((xp * xp).astype(prod)), box((yp * yp).astype(prod)), box((xp * yp).astype(prod))
        cn = acc(NP / (NP - 1.0))
        vx, vy, vxy = cn * (uxx - ux * ux), cn * (uyy - uy * uy), cn * (uxy - ux * uy)
        S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))
        out.append(np.mean(S.astype(np.float64)))
    return float(np.mean(out))


def main():
    rng = np.random.default_rng(1)
    worst = {"f64/f64": 0.0, "f32prod/f64sum": 0.0, "f32/f32": 0.0}
    for (h, wd) in ((28, 28), (32, 32), (64, 64), (40, 24), (256, 256)):
        for c in (1, 3):
            if h == 256 and c == 3:
                continue
            for _ in range(3 if h < 256 else 1):
                a = (0.98 + 0.02 * rng.random((h, wd, c))).astype(np.float32)
                b = (0.98 + 0.02 * rng.random((h, wd, c))).astype(np.float32)
                s = np.clip(np.kron(rng.random((h // 4 + 2, wd // 4 + 2, c)), np.ones((4, 4, 1)))[:h, :wd], 0, 1).astype(np.float32)
                n = np.clip(s + 0.01 * rng.standard_normal(s.shape), 0, 1).astype(np.float32)
                r, r2 = rng.random((h, wd, c)).astype(np.float32), rng.random((h, wd, c)).astype(np.float32)
                for (p, q) in ((a, b), (s, n), (r, r2)):
                    ref = ssim_loops(p, q, data_range=1.0)
                    worst["f64/f64"] = max(worst["f64/f64"], abs(ssim_k(p, q) - ref))
                    worst["f32prod/f64sum"] = max(worst["f32prod/f64sum"], abs(ssim_k(p, q, prod=np.float32) - ref))
                    worst["f32/f32"] = max(worst["f32/f32"], abs(ssim_k(p, q, prod=np.float32, acc=np.float32) - ref))
        print(h, wd, worst, flush=True)


if __name__ == "__main__":
    main()
