"""What the architecture-faithful score tail costs: images/s of the seeded InceptionV3 ("fid" variant, gad/inception.py) at
B = 256 from 32 x 32 inputs on the HIP operators (A), against the same architecture and weights as stock torch ops on the GPU
(B: tests/inception_ref.py in float32 - what a `GAD_FEATURE_NET_TS` TorchScript extractor would run).  Both are warmed, then
alternate `--repeats` times under a device-synchronised host clock.  A second, separate pass brackets every launch of A and
every BasicConv2d of B with device events: time per kernel family of A, and per layer of both - the layers where A loses
most are listed.  Last, the accuracy figures of tests/test_gpu_inception.py at B = 2: the float32 CPU reference's and the
HIP route's relative max-norm error against float64, both variants.
usage (GPU box): python tools/bench_score_tail.py [--batch 256] [--repeats 5] [--out profiles/score_tail_inception.txt]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "group-attribution-for-diffusion-models_amd"), ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import torch  # noqa: E402

import inception_ref as R  # noqa: E402
from gad import inception, ops  # noqa: E402

dev = torch.device("cuda:0")


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


class Events:
    """device-event brackets keyed by a name; totals in ms after a synchronise"""

    def __init__(self):
        self.rec = []

    def wrap(self, fn, key):
        def timed(*a, **kw):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            r = fn(*a, **kw)
            e.record()
            self.rec.append((key(*a, **kw) if callable(key) else key, s, e))
            return r
        return timed

    def totals(self):
        torch.cuda.synchronize()
        out = {}
        for k, s, e in self.rec:
            out[k] = out.get(k, 0.0) + s.elapsed_time(e)
        return out


def conv_family(name):
    _, _, kh, kw, stride, _, _ = inception._SPEC[name]
    return f"conv {kh}x{kw}" + (" s2" if stride == 2 else "")


def profile_hip(net, x):
    """-> ({family: ms}, {layer: ms of its convolution launch}, multiply-adds of the convolutions) of one forward; ReLU passes
    are their own family"""
    fam, layer = Events(), Events()
    saved = {n: getattr(ops, n) for n in ("conv_krsc_raw", "gemm_raw", "pool2d_raw", "relu_raw", "resize_bilinear_raw", "colsum_raw")}
    by_weight = {net.w[name][0].data_ptr(): name for name in inception._SPEC}
    conv_name, macs = [None], [0]

    def counted(*a, **kw):
        macs[0] += a[5] * a[6] * a[7]                     # M N K
        return saved["gemm_raw"](*a, **kw)

    def conv(x_, w, *a, **kw):
        conv_name[0] = by_weight[w.data_ptr()]
        return saved["conv_krsc_raw"](x_, w, *a, **kw)
    ops.conv_krsc_raw = conv
    ops.gemm_raw = fam.wrap(layer.wrap(counted, lambda *a, **kw: conv_name[0]), lambda *a, **kw: conv_family(conv_name[0]))
    for n, family in (("pool2d_raw", "pool2d"), ("relu_raw", "relu"), ("resize_bilinear_raw", "resize + 2x-1"),
                      ("colsum_raw", "global average")):
        setattr(ops, n, fam.wrap(saved[n], family))
    try:
        net(x)
    finally:
        for n, fn in saved.items():
            setattr(ops, n, fn)
    return fam.totals(), layer.totals(), macs[0]


def profile_stock(sd, x):
    """-> {layer: ms of conv + batch_norm + relu}"""
    ev, basic = Events(), R.basic
    R.basic = ev.wrap(basic, lambda sd_, name, *a, **kw: name)
    try:
        R.forward(sd, x, "fid", torch.float32)
    finally:
        R.basic = basic
    return ev.totals()


def accuracy(say):
    for variant in ("fid", "torchvision"):
        sd = inception.seeded_state_dict(variant, 1234)
        net = inception.InceptionV3(variant, sd, tag="seeded").to(dev)
        x = torch.rand(2, 3, 32, 32, generator=torch.Generator().manual_seed(2))
        p64, l64 = R.forward(sd, x, variant, torch.float64)
        p32, l32 = R.forward(sd, x, variant, torch.float32)
        pool3 = net(x.to(dev))
        logits = net.logits(pool3)
        for what, got, yard, ref in (("pool3", pool3.cpu(), p32, p64), ("logits", logits.cpu(), l32, l64)):
            rel = lambda a: float((a.double() - ref).abs().max() / ref.abs().max())      # noqa: E731
            say(f"  {variant:11s} {what:6s}: float32 CPU reference {rel(yard):.2e}, HIP route {rel(got):.2e}  (ratio {rel(got) / rel(yard):.2f}; bound 16)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    B = args.batch
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say(f"InceptionV3 score tail, seeded 'fid' variant, B={B} from 32x32 inputs, fp32 ({torch.cuda.get_device_name(0)})")
    sd = inception.seeded_state_dict("fid", 1234)
    net = inception.InceptionV3("fid", sd, tag="inception-fid-seeded1234").to(dev)
    sd_dev = {k: v.to(dev) for k, v in sd.items()}
    x = torch.rand(B, 3, 32, 32, generator=torch.Generator().manual_seed(0)).to(dev)

    def run_a():
        return net(x)

    def run_b():
        return torch.cat([R.forward(sd_dev, x[s:s + net.max_batch], "fid", torch.float32)[0] for s in range(0, B, net.max_batch)], 0)
    fa, fb = run_a(), run_b()                           # warm-up of every launch shape (and MIOpen's algorithm search)
    run_a(), run_b()
    ta, tb = [], []
    for _ in range(args.repeats):
        ta.append(clock(run_a)[0])
        tb.append(clock(run_b)[0])
    diff = float((fa - fb).abs().max() / fb.abs().max())
    say(f"A HIP operators (gad.inception)   s/batch: {' '.join(f'{t:.4f}' for t in ta)}   min {min(ta):.4f}  -> {B / min(ta):.0f} images/s")
    say(f"B stock torch ops, same weights   s/batch: {' '.join(f'{t:.4f}' for t in tb)}   min {min(tb):.4f}  -> {B / min(tb):.0f} images/s")
    say(f"A / B = {min(ta) / min(tb):.2f}  (both in chunks of {net.max_batch} images; pool3 of A and B differ by {diff:.1e} of the max norm)")

    fam, layer_a, macs = profile_hip(net, x)
    say(f"convolutions: {macs / B / 1e9:.2f} GMAC per image -> A {2 * macs / min(ta) / 1e12:.1f} TFLOP/s, B {2 * macs / min(tb) / 1e12:.1f} TFLOP/s end to end")
    layer_b = profile_stock(sd_dev, x[:net.max_batch])
    scale = B / min(B, net.max_batch)                   # B's profile covers one chunk
    total = sum(fam.values())
    say(f"A by kernel family (device events around every launch, one forward of {B} images; {total:.1f} ms in launches):")
    for k, ms in sorted(fam.items(), key=lambda kv: -kv[1]):
        say(f"  {k:16s} {ms:9.2f} ms  {100 * ms / total:5.1f} %")
    say("the one extra read and write per activation (ReLU as its own pass instead of a bit in the GEMM epilogue): the 'relu' row")
    say("layers where A's convolution launch loses most against B's conv + batch_norm + relu (ms per forward: A, B, A - B):")
    worst = sorted(layer_a, key=lambda n: -(layer_a[n] - scale * layer_b.get(n, 0.0)))[:12]
    for n in worst:
        b = scale * layer_b.get(n, 0.0)
        ci, co, kh, kw, stride, _, _ = inception._SPEC[n]
        say(f"  {n:26s} {ci:4d}->{co:4d} {kh}x{kw}{' s2' if stride == 2 else '   '} {layer_a[n]:8.2f} {b:8.2f} {layer_a[n] - b:+8.2f}")
    say(f"  (all convolutions: A {sum(layer_a.values()):.1f} ms, B's BasicConv2d {scale * sum(layer_b.values()):.1f} ms)")
    say("accuracy at B=2, seeded weights, relative max-norm error against the float64 CPU reference (tests/test_gpu_inception.py):")
    accuracy(say)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
