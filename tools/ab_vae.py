"""What the autoencoders (gad/vae.py) cost on the GPU, and their two kernels against the routes they replace.

One step per process, so that each runs under a time limit of its own; every step appends its lines to --out:
  --step decode      ms per image of both full-width decoders with seeded weights at their real latent sizes - the SD VAE on
                     4 x 32 x 32 (256 x 256 pixels), the CelebA VQ-VAE on 3 x 64 x 64 (256 x 256, lookup included) - at batch 1
                     and 8, and where a batch-8 decode spends its time by launch kind (device events around every launch)
  --step attention   gad_attention_fwd_d512 against ops.attention_core_unfused (three launches, the score tensor in HBM) at one
                     head of 512, T = 1024 (the VAEs' 32 x 32 mid block) and 4096 (64 x 64), at batches on both sides of a full
                     chip of workgroups (256): time and peak allocation - what gad/vae.py routes by
  --step lookup      gad_vq_lookup against torch.cdist(z, e).argmin(1) on 8 x 64 x 64 rows, K = 8192, D = 3, and how many
                     indices differ (cdist's matmul form may take the other of two near-tied codes)
Times are medians of runs between device events after --warmup runs: --repeats of them, and more where a run is short (as
many as fit into half a second, 20 at the most).
usage (GPU box):
  for s in decode attention lookup; do timeout -k 10 300 python tools/ab_vae.py --step $s --out profiles/vae_ab.txt || exit 1; done"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "group-attribution-for-diffusion-models_amd"), ROOT):
    sys.path.insert(0, p)

import torch  # noqa: E402

dev = torch.device("cuda:0")


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


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    r = fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated(dev) - base, r


LAUNCH_KINDS = ("conv_direct_raw", "group_norm_raw", "linear_fwd_raw", "attention_fwd_d512_raw", "attention_fwd_raw",
                "attention_core_qkv_raw", "vq_lookup_raw", "nchw_to_nhwc_raw", "nhwc_to_nchw_raw")


def launch_table(fn):
    """{launch kind: (calls, seconds)} of one run of fn, from device events around every `ops.*_raw` call it makes"""
    from gad import ops
    marks, saved = [], {k: getattr(ops, k) for k in LAUNCH_KINDS}

    def wrap(kind, f):
        def g(*a, **kw):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            r = f(*a, **kw)
            e.record()
            marks.append((kind, s, e))
            return r
        return g
    try:
        for k, f in saved.items():
            setattr(ops, k, wrap(k, f))
        fn()
        torch.cuda.synchronize()
    finally:
        for k, f in saved.items():
            setattr(ops, k, f)
    out = {}
    for kind, s, e in marks:
        n, t = out.get(kind, (0, 0.0))
        out[kind] = (n + 1, t + s.elapsed_time(e) * 1e-3)
    return out


def step_decode(args, say):
    from gad import vae
    for name, cls, cfg, hw in (("SD VAE (AutoencoderKL)", vae.AutoencoderKL, vae.sd_vae_config(), 32),
                               ("CelebA VQ-VAE (VQModel)", vae.VQModel, vae.celeba_vq_config(), 64)):
        m = cls.seeded(cfg, 1234).to(dev)
        for B in (1, 8):
            z = torch.randn(B, cfg.latent_channels, hw, hw, generator=torch.Generator().manual_seed(B)).to(dev)
            t, img = timed(lambda: m.decode(z).sample, args.warmup, args.repeats)
            say(f"{name}: decode [{B}, {cfg.latent_channels}, {hw}, {hw}] -> {tuple(img.shape)}: {t * 1e3:.2f} ms, "
                f"{t * 1e3 / B:.2f} ms per image")
        table = launch_table(lambda: m.decode(z))
        total = sum(t for _, t in table.values())
        for kind, (n, t) in sorted(table.items(), key=lambda kv: -kv[1][1]):
            say(f"    {kind:24s} {n:4d} launches {t * 1e3:8.2f} ms {100 * t / total:5.1f} %   (batch 8, one run, events per launch)")
        del m
        torch.cuda.empty_cache()


def step_attention(args, say):
    from gad import ops
    for B, T in ((2, 1024), (8, 1024), (1, 4096), (4, 4096), (8, 4096)):
        g = torch.Generator().manual_seed(T)
        q, k, v = (torch.randn(B, T, 512, generator=g).mul(s).to(dev) for s in (0.7, 0.7, 1.0))

        def fused():
            return ops.attention_fwd_d512_raw(q, k, v, B, 1, T, T, 512, 512, 512, 512)[0]

        def unfused():
            with torch.no_grad():
                return ops.attention_core_unfused(q, k, v, 1)
        tf, of = timed(fused, args.warmup, args.repeats)
        tu, ou = timed(unfused, args.warmup, args.repeats)
        pf, pu = peak_of(fused)[0], peak_of(unfused)[0]
        flop = 4.0 * B * T * T * 512
        say(f"attention d=512 B={B} T={T} ({B * ((T + 63) // 64)} workgroups): gad_attention_fwd_d512 {tf * 1e3:.3f} ms ({flop / tf * 1e-12:.1f} TFLOP/s), peak "
            f"{pf / 2**20:.1f} MiB | three-launch route {tu * 1e3:.3f} ms, peak {pu / 2**20:.1f} MiB | max |diff| "
            f"{(of - ou).abs().max().item():.2e}")


def step_lookup(args, say):
    from gad import ops
    g = torch.Generator().manual_seed(3)
    z, e = torch.randn(8 * 64 * 64, 3, generator=g).to(dev), torch.randn(8192, 3, generator=g).to(dev)
    tk, (idx, _) = timed(lambda: ops.vq_lookup_raw(z, e), args.warmup, args.repeats)
    tc, ref = timed(lambda: torch.cdist(z, e).argmin(1), args.warmup, args.repeats)
    pk, pc = peak_of(lambda: ops.vq_lookup_raw(z, e))[0], peak_of(lambda: torch.cdist(z, e).argmin(1))[0]
    say(f"lookup n={len(z)} K=8192 D=3: gad_vq_lookup {tk * 1e3:.3f} ms, peak {pk / 2**20:.2f} MiB | torch.cdist(...).argmin "
        f"{tc * 1e3:.3f} ms, peak {pc / 2**20:.1f} MiB | indices that differ: {(idx.long() != ref).sum().item()} of {len(z)}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["decode", "attention", "lookup"], required=True)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    def say(line):
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")
    {"decode": step_decode, "attention": step_attention, "lookup": step_lookup}[args.step](args, say)


if __name__ == "__main__":
    main()
