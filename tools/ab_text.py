"""The text towers of gad/text.py at full size with seeded weights - the text half of CLIP ViT-B/32 (clip_text_b32) and SD 1.x's
CLIPTextModel (sd_text_l14) - at 1, 2 and 64 prompts: milliseconds per batch of `hidden(ids)`, the causal attention kernel's
share of it, and that kernel against torch's own causal scaled_dot_product_attention on the same [B, H, 77, 64] operands.

One preset per process, so that each runs under a time limit of its own; every step appends its lines to --out.  Times are
medians of --repeats (at least 20) windows between events on the launch stream after --warmup windows; the tower is one call
per window, the attention kernels --inner launches per window (a single launch is a few microseconds: a window of one would
measure the events), the two attention paths alternating window by window.  The share is layers x (kernel time) over the
tower's time: a kernel's time inside a launch-bound sequence, not a profile.  FLOPs are the architecture's: per block
4 W^2 + 2 W mlp per token, twice, + 2 x 2 T W per token for Q K^T and P V over the full square (the mask saves half of them;
not counted as saved).
usage (GPU box):
  for p in clip_text_b32 sd_text_l14; do
    timeout -k 10 300 python tools/ab_text.py --preset $p --out profiles/text_ab.txt || exit 1
  done"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "group-attribution-for-diffusion-models_amd"), ROOT):
    sys.path.insert(0, p)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from gad import ops, text  # noqa: E402

dev = torch.device("cuda:0")
BATCHES = (1, 2, 64)


def tower_flops(cfg, batch):
    T, W = cfg.context, cfg.width
    per_block = T * (2 * 4 * W * W + 2 * 2 * W * cfg.mlp) + 2 * 2 * T * T * W
    return batch * float(cfg.layers * per_block)


def window(fn, inner):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(inner):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e-3 / inner


def timed(fns, inner, warmup, repeats):
    """medians of the callables' times per call, alternating them window by window"""
    for _ in range(warmup):
        for fn in fns:
            window(fn, inner)
    ts = [[] for _ in fns]
    for _ in range(repeats):
        for fn, t in zip(fns, ts):
            t.append(window(fn, inner))
    return [statistics.median(t) for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", choices=sorted(text.PRESETS), required=True)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    cfg = text.PRESETS[args.preset]
    tower = text.TextTower.seeded(args.preset, 1234).to(dev)
    T, W, H = cfg.context, cfg.width, cfg.heads
    d = W // H
    repeats = max(args.repeats, 20)
    lines = []
    for batch in BATCHES:
        g = torch.Generator().manual_seed(batch)
        ids = torch.randint(0, cfg.vocab - 2, (batch, T), generator=g)
        ids[:, 0], ids[:, T // 2:] = cfg.vocab - 2, cfg.vocab - 1
        (t_tower,) = timed([lambda: tower.hidden(ids)], 1, args.warmup, repeats)
        qkv = torch.randn(batch * T, 3 * W, generator=g).to(dev)
        q, k, v = (qkv[:, i * W:(i + 1) * W].reshape(batch, T, H, d).transpose(1, 2).contiguous() for i in range(3))
        with ops.operand_precision("f32"):
            t_hip, t_sdpa = timed([lambda: ops.attention_causal_qkv_raw(qkv, batch, T, W, H),
                                   lambda: F.scaled_dot_product_attention(q, k, v, is_causal=True)], args.inner, args.warmup, repeats)
        diff = (ops.attention_causal_qkv_raw(qkv, batch, T, W, H).view(batch, T, H, d).transpose(1, 2)
                - F.scaled_dot_product_attention(q, k, v, is_causal=True)).abs().max().item()
        flop = tower_flops(cfg, batch)
        lines.append(f"{args.preset} B = {batch:2d}: hidden(ids) {t_tower * 1e3:7.3f} ms per batch ({t_tower / batch * 1e3:6.3f} ms per prompt, "
                     f"{flop / 1e9:.1f} GFLOP, {flop / t_tower / 1e12:.2f} TFLOP/s end to end); causal kernel {t_hip * 1e6:7.1f} us per launch "
                     f"x {cfg.layers} layers = {cfg.layers * t_hip / t_tower * 100:4.1f} % of it; torch causal SDPA f32 on [{batch}, {H}, {T}, {d}] "
                     f"{t_sdpa * 1e6:7.1f} us ({t_sdpa / t_hip:.2f} x); max abs difference {diff:.2e}")
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
