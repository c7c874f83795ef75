"""The image towers of gad/vit.py at full size with seeded weights - CLIP ViT-B/32 at batch 50 (one SD behaviour run's
images), open-CLIP ViT-L/14 at batch 16, the BLIP-VQA vision tower at batch 32 - against the plain-torch restatement
(tests/vit_ref.py) moved to the GPU in float32 on stock torch ops, same weights, same images.

One tower per process, so that each runs under a time limit of its own; every step appends its lines to --out.  Times are
medians of --repeats (at least 20) runs between events on the launch stream after --warmup runs, the two paths alternating
run by run.  FLOPs are the architecture's: 2 x (patch embedding + per block 4 W^2 + 2 W mlp per token + 2 T W per token for
Q K^T and P V, each) + projection, padding not counted; the share is of the f32 MFMA peak, 155.4 TFLOP/s.  `--trace` runs the
HIP path alone a few times and nothing else: the run to put under `rocprofv3 --kernel-trace --stats` for the per-kernel split.
usage (GPU box):
  for p in clip_vit_b32 clip_vit_l14 blip_vqa_base; do
    timeout -k 10 300 python tools/ab_vit.py --preset $p --out profiles/vit_ab.txt || exit 1
  done"""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "group-attribution-for-diffusion-models_amd"), ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import torch  # noqa: E402

import vit_ref  # noqa: E402
from gad import _capi, vit  # noqa: E402
from gad._capi import A_KC, B_KC, GemmArgs  # noqa: E402

dev = torch.device("cuda:0")
PEAK_F32_MFMA = 155.4e12
BATCH = {"clip_vit_b32": 50, "clip_vit_l14": 16, "blip_vqa_base": 32}
INPUT = {"clip_vit_b32": 256, "clip_vit_l14": 256, "blip_vqa_base": 256}      # SD samples at 256; CelebA-HQ at 256


def tower_flops(cfg, batch):
    T, W, g = cfg.tokens, cfg.width, cfg.grid
    per_block = T * (2 * 4 * W * W + 2 * 2 * W * cfg.mlp) + 2 * 2 * T * T * W
    head = 2 * W * cfg.embed_dim if cfg.embed_dim else 0
    return batch * (2.0 * g * g * 3 * cfg.patch ** 2 * W + cfg.layers * per_block + head)


def timed_pair(fa, fb, warmup, repeats):
    """medians of the two callables' times, alternating them run by run -> (seconds a, seconds b)"""
    for _ in range(warmup):
        fa()
        fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(repeats):
        for fn, ts in ((fa, ta), (fb, tb)):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            torch.cuda.synchronize()
            ts.append(s.elapsed_time(e) * 1e-3)
    return statistics.median(ta), statistics.median(tb)


def kernel_id(M, N, K):
    """which gad_gemm kernel a dense [M, K] x [N, K]^T launch with a bias takes"""
    a = GemmArgs()
    a.A = a.B = a.C = a.bias = 1 << 20               # a host decision on shapes and alignment: nothing is dereferenced
    a.a_mode, a.b_mode, a.M, a.N, a.K, a.lda, a.ldb, a.ldc, a.batch, a.batch_inner, a.alpha = A_KC, B_KC, M, N, K, K, K, N, 1, 1, 1.0
    return _capi.load().gad_gemm_kernel_id(ctypes.byref(a))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", choices=sorted(BATCH), required=True)
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    cfg = vit.PRESETS[args.preset]
    batch = args.batch or BATCH[args.preset]
    sd = vit.seeded_state_dict(args.preset, 1234)
    tower = vit.VisionTower(args.preset, sd).to(dev)
    side = INPUT[args.preset]
    x = torch.rand(batch, 3, side, side, generator=torch.Generator().manual_seed(0)).to(dev)
    if args.trace:
        for _ in range(5):
            tower(x)
        torch.cuda.synchronize()
        return
    sd_dev = {k: v.to(dev) for k, v in sd.items()}

    def ref():
        with torch.no_grad():
            return vit_ref.forward(sd_dev, cfg, x, torch.float32, dev)

    t_hip, t_ref = timed_pair(lambda: tower(x), ref, args.warmup, max(args.repeats, 20))
    diff = (tower(x) - ref()).abs().max().item()
    flop = tower_flops(cfg, batch)
    lines = [f"{args.preset} batch {batch} from {side} x {side} (chunks of {min(tower.max_batch, batch)}): HIP {t_hip * 1e3:8.2f} ms "
             f"({t_hip / batch * 1e3:6.3f} ms per image, {flop / t_hip / PEAK_F32_MFMA:.3f} of the f32 MFMA peak over {flop / 1e9:.1f} GFLOP); "
             f"stock torch f32 {t_ref * 1e3:8.2f} ms ({t_ref / t_hip:.2f} x); max abs difference of the embeddings {diff:.2e}",
             f"{args.preset} gad_gemm_kernel_id: patch embedding (M = {batch * cfg.grid ** 2}, N = {cfg.width}, K = {3 * cfg.patch ** 2}) "
             f"{kernel_id(batch * cfg.grid ** 2, cfg.width, 3 * cfg.patch ** 2)}; qkv (M = {batch * cfg.tokens}, N = {3 * cfg.width}, "
             f"K = {cfg.width}) {kernel_id(batch * cfg.tokens, 3 * cfg.width, cfg.width)}; attention T = {cfg.tokens}, "
             f"{cfg.heads} heads of {cfg.width // cfg.heads}"]
    for s in lines:
        print(s, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
