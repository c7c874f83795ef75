"""LoRA unlearning: the dropout LoRA down-projection kernels (csrc/lora.hip) against the unfused torch sequence, and a `lora` step
against a `gd` step of the CIFAR U-Net.

Step `kernels`: M = 32 768 tokens (B = 128, T = 256), C = 256, r = 16, three projections, p = 0.05.
  forward   gad_lora_down_dropout_fwd                        against 3 x torch dropout + 3 x down GEMM (x A^T, scaled)
  backward  gad_lora_down_dropout_bwd                        against 3 x (dropout's backward mask multiply, dA = dmid^T xd, dx += (dmid A) o m)
Bytes are the algorithm's: forward reads x once and writes three [M, r] (M C + 3 M r floats); backward reads x and dx, writes dx,
reads three dmid and writes the dA partials and results (3 M C + 3 M r + partials).  GB/s = those bytes over the measured time, and
the fraction of the 6.3 TB/s a float4 copy reaches on this part is printed next to it.  The torch sequence moves more than that
(three dropped copies written and read again): its GB/s column is the algorithm's bytes over its time.
Step `steps`: one `lora` training step (gad.get_peft_model + FusedTrainer with the LoRA+ groups) against one `gd` step
(FusedTrainer over every parameter) at B = 128 on the full CIFAR U-Net and on the pruned one (ratio 0.3), and the new kernels'
share of the lora step (their time at the step's own shapes, measured in isolation, over the step's time).

Method: device events around `ITERS` back-to-back calls after a warm-up of the same shape; `ROUNDS` rounds with the versions
alternating inside each round; median and min .. max over the rounds.

Run by hand on the GPU, each step in a process of its own under a time limit:
    timeout -k 10 300 python tools/ab_lora.py --step kernels --out profiles/lora_ab.txt && \\
    timeout -k 10 400 python tools/ab_lora.py --step steps --out profiles/lora_ab.txt
Each step appends its report to --out (the `kernels` step starts the file)."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "group-attribution-for-diffusion-models_amd"))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

dev = torch.device("cuda:0")
ITERS, ROUNDS, WARM = 20, 5, 5
HBM = 6.3e12                                                     # what a float4 copy reaches on the MI355X
PRUNED = dict(block_out_channels=[96, 192, 192, 192])            # unconditional_generation/prune.py at --pruning_ratio 0.3
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
    tail = f"   {nbytes / med / 1e9:8.1f} GB/s of {nbytes / 1e6:.1f} MB = {nbytes / med / HBM * 100:.0f} % of the HBM roof" if nbytes else ""
    say(f"  {name:46s} {med * 1e6:10.1f} us  ({min(ts) * 1e6:.1f} .. {max(ts) * 1e6:.1f}){tail}")
    return med


def kernel_pair(M, C, r, n_proj, p, s=2.0):
    """(fused forward, fused backward, torch forward, torch backward, forward bytes, backward bytes) on fresh operands"""
    from gad import _capi, ops
    import ctypes
    gen = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(M, C, device=dev, generator=gen)
    As = [torch.randn(r, C, device=dev, generator=gen) / C ** 0.5 for _ in range(n_proj)]
    dm = [torch.randn(M, r, device=dev, generator=gen) for _ in range(n_proj)]
    dx = torch.randn(M, C, device=dev, generator=gen)
    outs = [torch.empty_like(a) for a in As]
    step = [0]

    def fwd():
        step[0] += 1
        return ops.lora_down_dropout_fwd_raw(x, As, p, s, 1, step[0], 0)

    def bwd():
        ops.lora_down_dropout_bwd_raw(x, As, dm, dx, p, 1, step[0], 0, outs=outs)
    keep = [None] * n_proj

    def t_fwd():
        mids = []
        for j, a in enumerate(As):
            xd = torch.nn.functional.dropout(x, p, training=True)
            keep[j] = xd
            mids.append((xd @ a.t()) * s)
        return mids

    def t_bwd():
        for j, a in enumerate(As):
            xd = keep[j]                                           # the dropped copy autograd would have saved
            torch.mm(dm[j].t(), xd, out=outs[j])
            dx.add_((dm[j] @ a) * (xd != 0) / (1 - p))
    a_ = ops._lora_dropout_args(x, As, p, s, 1, 1, 0)
    partials = _capi.load().gad_lora_down_dropout_workspace_bytes(ctypes.byref(a_))
    fb = 4 * (M * C + n_proj * M * r)
    bb = 4 * (3 * M * C + n_proj * M * r + n_proj * r * C) + 2 * partials
    fwd()
    t_fwd()
    return fwd, bwd, t_fwd, t_bwd, fb, bb, partials


def kernels_step():
    M, C, r, n_proj, p = 32768, 256, 16, 3, 0.05
    say("Dropout LoRA down-projection: gad_lora_down_dropout_fwd / _bwd against the unfused torch sequence")
    say(f"device: {torch.cuda.get_device_name(0)}; {ITERS} calls per window after {WARM} warm-up, {ROUNDS} alternating rounds; median (min .. max)")
    fwd, bwd, t_fwd, t_bwd, fb, bb, partials = kernel_pair(M, C, r, n_proj, p)
    say(f"\nM = {M}, C = {C}, r = {r}, {n_proj} projections, p = {p}; dA partials {partials / 1e6:.1f} MB against {4 * M * C / 1e6:.1f} MB of x")
    ts = alternate({"fwd": fwd, "t_fwd": t_fwd, "bwd": bwd, "t_bwd": t_bwd})
    f, tf = report("fused forward", ts["fwd"], fb), report("torch: 3 dropout + 3 down GEMM", ts["t_fwd"], fb)
    b, tb = report("fused backward (dA and dx +=)", ts["bwd"], bb), report("torch: 3 x (dA GEMM, dx += masked GEMM)", ts["t_bwd"], bb)
    say(f"  forward torch / fused = {tf / f:.2f}x, backward torch / fused = {tb / b:.2f}x, both = {(tf + tb) / (f + b):.2f}x")
    say("  (HBM does not bind where the fraction above is small: the Philox rounds - one call per four elements and projection - are")
    say("   integer multiplies on the vector ALUs, as in csrc/projector.hip)")
    fwd0, bwd0, _, _, _, _, _ = kernel_pair(M, C, r, n_proj, 0.0)
    ts = alternate({"fwd0": fwd0, "bwd0": bwd0})
    report("p = 0: forward = 3 plain gad_gemm launches", ts["fwd0"], fb + 2 * 4 * M * C)
    report("p = 0: backward, mask-free instance", ts["bwd0"], bb)


def steps_step():
    import gad
    from src.ddpm_config import DDPMConfig
    B = 128
    say(f"\nOne training step at B = {B}: `lora` (r = 16, p = 0.05, LoRA+ groups) against `gd` (every parameter)")
    share = {}
    for label, overrides in (("CIFAR U-Net", {}), ("CIFAR U-Net pruned at ratio 0.3", PRUNED)):
        cfg = dict(DDPMConfig.cifar_config["unet_config"], **overrides)
        sch = gad.DDPMScheduler(**DDPMConfig.cifar_config["scheduler_config"])
        gen = torch.Generator(device=dev).manual_seed(0)
        x, e = torch.randn(B, 3, 32, 32, device=dev, generator=gen), torch.randn(B, 3, 32, 32, device=dev, generator=gen)
        t = torch.randint(0, 1000, (B,), device=dev, generator=gen)
        torch.manual_seed(0)
        net_gd = gad.UNet2DModel(**cfg).to(dev)
        tr_gd = gad.FusedTrainer(net_gd, sch, None, lr=1e-4)
        net_lo = gad.UNet2DModel(**cfg).to(dev)
        gad.get_peft_model(net_lo, gad.LoraConfig(r=16, lora_alpha=32, lora_dropout=0.05, target_modules=["to_q", "to_k", "to_v"]))
        params, groups = gad.lora_parameters(net_lo, 16)
        tr_lo = gad.FusedTrainer(net_lo, sch, None, lr=1e-4, params=params, groups=groups)
        net_gd.train()
        net_lo.train()
        say(f"\n{label}: {sum(p.numel() for p in net_gd.parameters())} parameters, {sum(p.numel() for p in params)} LoRA parameters in "
            f"{len(params) // 6} attention blocks")
        ts = alternate({"gd": lambda: tr_gd.step(x, e, t), "lora": lambda: tr_lo.step(x, e, t)}, iters=5, warm=3)
        g, l = report("gd step", ts["gd"]), report("lora step", ts["lora"])
        say(f"  gd / lora = {g / l:.2f}x")
        # the new kernels at the step's own shapes, in isolation
        total, shapes, orig = 0.0, [], gad.lora.LoraQKV.forward

        def recording(self, attn, h):
            shapes.append((h.shape[0] * h.shape[1], h.shape[2]))
            return orig(self, attn, h)
        gad.lora.LoraQKV.forward = recording
        try:
            tr_lo.step(x, e, t)
        finally:
            gad.lora.LoraQKV.forward = orig
        say(f"  token matrices of the attention blocks [M, C]: {shapes}")
        for M_, C in shapes:
            fwd, bwd, _, _, _, _, _ = kernel_pair(M_, C, 16, 3, 0.05)
            k = alternate({"f": fwd, "b": bwd}, iters=10, warm=3)
            total += statistics.median(k["f"]) + statistics.median(k["b"])
        share[label] = total / l
        say(f"  the dropout down-projection kernels of its attention blocks, in isolation: {total * 1e6:.1f} us = {100 * total / l:.1f} % of the lora step")
        del net_gd, net_lo, tr_gd, tr_lo
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["kernels", "steps"], required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lora_ab.txt"))
    a = ap.parse_args()
    {"kernels": kernels_step, "steps": steps_step}[a.step]()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w" if a.step == "kernels" else "a") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
