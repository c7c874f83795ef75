"""Precision / recall of one coalition at the reference's sizes: the torch path (`make_manifold` + `calc_pr` of
src/attributions/global_scores/precision_recall.py: cdist tiles of 10 000 x 10 000, kthvalue, broadcast compare) against the
fused kernel (`make_manifold_device` + `calc_pr_device`, csrc/manifold.hip) on the same random fp16 features
(randn.clamp_min(0).half(), the look of post-ReLU fc features), and what the VGG16 extractor costs.

One step per process, so that each runs under a time limit of its own; every step appends its lines to --out:
  --step device --ngen N --d D   per coalition: the generated manifold's radii + both coverage passes against a cached reference
                                  manifold (N_ref = 50 000); once per dataset: the reference manifold's radii
  --step torch  --ngen N --d D   the same two figures on the torch path, and the two paths' precision / recall side by side
  --step vgg                     seconds per 1024 images of the seeded VGG16 at resolution 224 and 32
Times are medians of runs between device events after --warmup runs: --repeats of them, and more where a run is short (as
many as fit into half a second, 20 at the most).  Both paths' figures are taken the same way.  The share of the f16 MFMA peak is the
algorithm's 2 D (N_gen^2 + 2 N_gen N_ref) FLOP (tile padding not counted) over the time, over 16 x 157.3 TFLOP/s.
usage (GPU box):
  for d in 4096 2048; do for n in 1024 10240; do
    timeout -k 10 300 python tools/ab_manifold.py --step device --ngen $n --d $d --out profiles/manifold_ab.txt &&
    timeout -k 10 600 python tools/ab_manifold.py --step torch --ngen $n --d $d --out profiles/manifold_ab.txt || exit 1
  done; done && timeout -k 10 300 python tools/ab_manifold.py --step vgg --out profiles/manifold_ab.txt"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "group-attribution-for-diffusion-models_amd"), ROOT):
    sys.path.insert(0, p)

import torch  # noqa: E402

from src.attributions.global_scores import precision_recall as PR  # noqa: E402

dev = torch.device("cuda:0")
PEAK_F16_MFMA = 16 * 157.3e12
N_REF = 50_000
K = 3


def timed(fn, warmup, repeats):
    """-> (median seconds, the last result)"""
    for _ in range(warmup):
        r = fn()
    torch.cuda.synchronize()
    ts = []
    while len(ts) < repeats:
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        r = fn()
        e.record()
        torch.cuda.synchronize()
        ts.append(s.elapsed_time(e) * 1e-3)
        if len(ts) == 1:                                # short runs: as many as fit into half a second
            repeats = max(repeats, min(20, int(0.5 / max(ts[0], 1e-6))))
    return statistics.median(ts), r


def features(n, d, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.randn(n, d, device=dev, generator=g).clamp_min_(0).half()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=("device", "torch", "vgg"), required=True)
    ap.add_argument("--ngen", type=int, default=1024)
    ap.add_argument("--nref", type=int, default=N_REF)
    ap.add_argument("--d", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    if args.step == "vgg":
        from gad import vgg
        sd = vgg.seeded_state_dict(1234)
        x = torch.rand(1024, 3, 32, 32, generator=torch.Generator().manual_seed(0)).to(dev)
        for res in (224, 32):
            net = vgg.VGG16(sd, resolution=res).to(dev)
            t, _ = timed(lambda: net(x), args.warmup, args.repeats)
            say(f"vgg16 seeded, resolution {res:3d}: {t:8.3f} s per 1024 images ({1024 / t:7.0f} images/s, chunks of {min(net.max_batch, 1024)})")
            del net
    else:
        ng, nr, d = args.ngen, args.nref, args.d
        gen, ref = features(ng, d, 1), features(nr, d, 2)
        flop = 2.0 * d * (ng * ng + 2.0 * ng * nr)
        head = f"{args.step:6s} N_gen={ng:6d} N_ref={nr} D={d}:"
        if args.step == "device":
            t_ref, m_ref = timed(lambda: PR.make_manifold_device(ref, K), args.warmup, args.repeats)
            t, pr = timed(lambda: PR.calc_pr_device(PR.make_manifold_device(gen, K), m_ref), args.warmup, args.repeats)
            say(f"{head} per coalition {t * 1e3:10.2f} ms = {flop / t / PEAK_F16_MFMA:.3f} of the f16 MFMA peak; reference manifold "
                f"(once per dataset) {t_ref * 1e3:10.2f} ms = {2.0 * d * nr * nr / t_ref / PEAK_F16_MFMA:.3f}; precision {pr[0]:.6f} recall {pr[1]:.6f}")
        else:
            t_ref, m_ref = timed(lambda: PR.make_manifold(ref, K, 10000, 10000, dev), args.warmup, args.repeats)
            t, pr = timed(lambda: PR.calc_pr(PR.make_manifold(gen, K, 10000, 10000, dev), m_ref, 10000, 10000, dev), args.warmup, args.repeats)
            say(f"{head} per coalition {t * 1e3:10.2f} ms; reference manifold (once per dataset) {t_ref * 1e3:10.2f} ms; "
                f"precision {pr[0]:.6f} recall {pr[1]:.6f}")
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
