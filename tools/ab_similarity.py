"""Cosine similarities of the similarity baselines at the reference's sizes: the fused kernel (gad.cosine_rows,
csrc/similarity.hip) against the reference's statements on torch (text_to_image/baselines.py:232-248: normalise the rows of X,
normalise q, matmul; the fp32 training matrix resident on the device, all generated rows at once rather than one per pass) on
the same seeded operands, and the two results against each other.

One step per process, so that each runs under a time limit of its own; every step appends its lines to --out:
  --step kernel --kind u8|f32 --n N --m M --d D [--splits S]
  --step torch  --kind u8|f32 --n N --m M --d D      (u8: the decoded fp32 matrix, as the reference holds it)
Times are medians of runs between device events after --warmup runs: --repeats of them, and more where a run is short (as many
as fit into half a second, 20 at the most).  Per launch: the bytes the algorithm needs (N D operand bytes of X - 1 or 4 each - plus
Q and sim) against the bytes moved to and from HBM (the same, X once per block of 64 columns, plus the split partials written and
read back; Q is counted once - at most 39 MB here, re-read by every row tile out of the L2 / MALL), and
the share of the two roofs: bytes moved over 8.0 TB/s (HBM3E peak), 2 N M D FLOP over 157.3 TFLOP/s (fp32-input MFMA peak;
padding of M to 64 not counted).  The larger of the two least times over the measured time is the share of the roofline.
usage (GPU box):
  for shape in "u8 196608" "f32 196608" "f32 4096" "f32 512"; do set -- $shape
    timeout -k 10 300 python tools/ab_similarity.py --step kernel --kind $1 --d $2 --out profiles/similarity_ab.txt &&
    timeout -k 10 300 python tools/ab_similarity.py --step torch --kind $1 --d $2 --out profiles/similarity_ab.txt || exit 1
  done"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "group-attribution-for-diffusion-models_amd"), ROOT):
    sys.path.insert(0, p)

import torch  # noqa: E402

dev = torch.device("cuda:0")
PEAK_F32_MFMA = 157.3e12
PEAK_HBM = 8.0e12


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


def operands(kind, n, m, d):
    g = torch.Generator(device=dev).manual_seed(1)
    if kind == "u8":
        x = torch.randint(0, 256, (n, d), device=dev, generator=g, dtype=torch.uint8)
    else:
        x = torch.randn(n, d, device=dev, generator=g) + 0.3
    return x, torch.randn(m, d, device=dev, generator=g) + 0.3


def decoded(x):
    """uint8 -> the fp32 matrix the reference holds ((u / 255 - 0.5) / 0.5), in row chunks; fp32 passes through"""
    if x.dtype != torch.uint8:
        return x
    from gad import similarity
    lut = similarity._lut(x.device)
    return torch.cat([lut[x[s:s + 256].long()] for s in range(0, len(x), 256)], 0)


def reference_statements(x32, q):
    """baselines.py:232-248 with the generated rows side by side"""
    flat = x32 / x32.norm(dim=-1, keepdim=True)
    qn = q / q.norm(dim=-1, keepdim=True)
    return torch.matmul(flat, qn.T)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=("kernel", "torch"), required=True)
    ap.add_argument("--kind", choices=("u8", "f32"), default="u8")
    ap.add_argument("--n", type=int, default=5000)
    ap.add_argument("--m", type=int, default=50)
    ap.add_argument("--d", type=int, default=196608)
    ap.add_argument("--splits", type=int, default=0)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    from gad import _capi, similarity
    n, m, d = args.n, args.m, args.d
    x, q = operands(args.kind, n, m, d)
    elem = 1 if args.kind == "u8" else 4
    algo = n * d * elem + m * d * 4 + n * m * 4
    flop = 2.0 * n * m * d
    head = f"{args.step:6s} {args.kind:3s} N={n} M={m} D={d}:"
    if args.step == "kernel":
        lib = _capi.load()
        kind = _capi.SIM_X_U8 if args.kind == "u8" else _capi.SIM_X_F32
        ws = lib.gad_cosine_rows_workspace_bytes(n, m, d, kind, args.splits)
        blocks = -(-m // 64)
        moved = blocks * n * d * elem + m * d * 4 + 2 * ws + n * m * 4      # Q from HBM once: the row tiles' re-reads are L2 / MALL hits
        t, sim = timed(lambda: similarity.cosine_rows(x, q, splits=args.splits), args.warmup, args.repeats)
        least_mem, least_mfma = moved / PEAK_HBM, flop / PEAK_F32_MFMA
        bound = "HBM" if least_mem > least_mfma else "f32 MFMA"
        line = (f"{head} {t * 1e3:9.3f} ms; {moved / 1e9:.3f} GB moved for {algo / 1e9:.3f} GB algorithmic ({n * d * elem / 1e9:.3f} GB of X, "
                f"workspace {ws / 1e6:.1f} MB, splits={args.splits or 'auto'}); {moved / t / PEAK_HBM:.3f} of the HBM roof, "
                f"{flop / t / PEAK_F32_MFMA:.3f} of the f32 MFMA roof ({flop / t / 1e12:.1f} TFLOP/s); roofline bound {bound}, "
                f"share {max(least_mem, least_mfma) / t:.3f}")
    else:
        x32 = decoded(x)
        t, sim = timed(lambda: reference_statements(x32, q), args.warmup, args.repeats)
        moved = 4 * n * d * 4                                                   # X read for the norms, read and written normalised, read by the matmul
        line = (f"{head} {t * 1e3:9.3f} ms with fp32 X resident ({n * d * 4 / 1e9:.3f} GB; at least {moved / 1e9:.3f} GB moved per call: "
                f"norm pass, normalised copy, matmul); {flop / t / 1e12:.1f} TFLOP/s")
    other = reference_statements(decoded(x), q) if args.step == "kernel" else similarity.cosine_rows(x, q)
    line += f"; max |kernel - torch| {(sim - other).abs().max().item():.3e}"
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
