"""Per-sample LoRA gradients of the SD U-Net (unpruned SD-1.x, r = 256, 32 x 32 latents, bf16 activations: the sd256-bf16 shapes):
(1) gad_hgemm_tn_seg against S separate gad_hgemm_tn launches at the shapes of the four U-Net levels and of the context;
(2) gradient rows per second of gad.trak.lora_per_sample_gradients for journey rows (k = 1) with 16 rows per backward against
    one row per backward - through the segmented sink with S = 1, and through the flat-buffer sink with B = 1, which is the
    method gradient_features uses - and for `--source train` with k timesteps per image in chunks of j;
(3) the projection of a [16][P] staging block (gad_jl_project), which every route pays per 16 rows.
Times are device-event means after warm-up; every shape is warmed before it is timed.  usage (GPU box): python tools/ab_per_sample.py [k]"""
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "group-attribution-for-diffusion-models_amd"))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import gad  # noqa: E402
from gad import half, ops, trak  # noqa: E402

dev = torch.device("cuda:0")
BF = torch.bfloat16


def timeit(fn, iters, warm=1):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e-3


def kernels():
    print("(1) segmented launch against S plain launches; us per call (mean of 50 after 5), useful FLOP rate of the segmented launch")
    print(f"{'shape':>26s} {'L':>5s} {'S':>3s} {'seg us':>8s} {'S x tn us':>10s} {'ratio':>6s} {'seg TF/s':>9s} {'MFMA rows padded':>17s}")
    shapes = [("level 0 dUp 320x256", 320, 256, 1024), ("level 0 dDown 256x320", 256, 320, 1024), ("level 1 dUp 640x256", 640, 256, 256),
              ("level 1 dDown 256x640", 256, 640, 256), ("level 2 dUp 1280x256", 1280, 256, 64), ("level 3 dUp 1280x256", 1280, 256, 16),
              ("context dDown 256x768", 256, 768, 77)]
    P = 50_000_000
    for name, M, N, L in shapes:
        for S in (16, 64):
            a = torch.randn(S * L, M, device=dev).to(BF)
            b = torch.randn(S * L, N, device=dev).to(BF)
            staging = torch.zeros(S, P if S == 16 else M * N, device=dev)
            stride = staging.stride(0)
            outs = [torch.empty(M, N, device=dev) for _ in range(S)]
            t_seg = timeit(lambda: half.wgrad_seg_raw(a, b, staging, M, N, S, stride), 50, 5)

            def plain():
                for s in range(S):
                    half.wgrad_raw(a[s * L:(s + 1) * L], b[s * L:(s + 1) * L], outs[s], accumulate=False)
            t_tn = timeit(plain, 50, 5)
            pad = 1.0 - L / (math.ceil(L / 64) * 64)
            print(f"{name:>26s} {L:5d} {S:3d} {t_seg * 1e6:8.1f} {t_tn * 1e6:10.1f} {t_tn / t_seg:6.2f} "
                  f"{2.0 * S * L * M * N / t_seg / 1e12:9.1f} {pad:17.0%}")
            del staging


def features(k):
    print("\n(2) gradient rows per second, SD-1.x U-Net, r = 256, 32 x 32 latents, context 77 x 768, bf16 activations, behaviour `loss`")
    gad.set_operand_precision("bf16")
    net = gad.UNet2DConditionModel().to(dev)
    net.inject_lora(rank=256)
    for n, p in net.named_parameters():
        if n.endswith("lora_layer.up.weight"):
            torch.nn.init.normal_(p, std=0.02)
    sch = gad.DDPMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", num_train_timesteps=1000)
    params, gflat = trak.lora_flat_gradient(net)
    P = gflat.numel()
    print(f"P = {P} (flat, slot-padded); staging [16][P] = {16 * P * 4 / 2 ** 30:.2f} GiB")
    g = torch.Generator().manual_seed(0)
    lat = torch.randn(16, 4, 32, 32, generator=g) * 0.8
    ctx = torch.randn(16, 77, 768, generator=g) * 0.5
    ts1 = torch.randint(0, 1000, (16, 1), generator=g)

    def rows(S, j, ts, n=16):
        for _ in trak.lora_per_sample_gradients(net, sch, lat[:n], ctx[:n], ts[:n], "loss", 16, samples_per_backward=S,
                                                timesteps_per_backward=j):
            pass

    t16 = timeit(lambda: rows(16, 1, ts1), 3, 1)
    t1 = timeit(lambda: rows(1, 1, ts1), 2, 1)

    def flat_b1():                                                # the method of gradient_features: flat sink, one row per backward
        for i in range(16):
            x, c, t = lat[i:i + 1].to(dev), ctx[i:i + 1].to(dev), ts1[i].to(dev)
            e = torch.randn_like(x)
            pred = net(sch.add_noise(x, e, t), t, c).sample.contiguous()
            _, d = ops.mse_fwd_bwd_raw(pred, e)
            ops.begin_backward_step()
            try:
                pred.backward(d)
            finally:
                ops.end_backward_step()
    staging = torch.empty(16, P, device=dev)

    def flat_b1_staged():
        flat_b1()
        staging[0].copy_(gflat)
    tf = timeit(flat_b1_staged, 2, 1)
    print(f"journey (k = 1), 16 rows: 16 rows per backward {t16 * 1e3:8.1f} ms = {16 / t16:7.1f} rows/s")
    print(f"                          1 row per backward, segmented sink S = 1 {t1 * 1e3:8.1f} ms = {16 / t1:7.1f} rows/s  ({t1 / t16:.2f}x slower)")
    print(f"                          1 row per backward, flat sink B = 1      {tf * 1e3:8.1f} ms = {16 / tf:7.1f} rows/s  ({tf / t16:.2f}x slower)")
    del staging
    tsk = torch.arange(0, 1000, 1000 // k).expand(16, -1)
    for S, j in ((16, 1), (16, 4), (4, 16)):
        t = timeit(lambda: rows(S, j, tsk), 1, 0 if k > 20 else 1)
        print(f"train (k = {k}), 16 images: S = {S:2d} images x j = {j:2d} timesteps per backward {t:7.2f} s = {16 / t:6.2f} images/s")
    t = timeit(lambda: rows(1, k, tsk, n=2), 1, 0)                 # one image per backward, its k timesteps as the batch
    print(f"train (k = {k}),  2 images: one image per backward, B = k = {k} {t:7.2f} s = {2 / t:6.2f} images/s")
    gad.set_operand_precision("no")
    print("\n(3) projection of a [16][P] staging block (one gad_jl_project launch, normal entries)")
    a = torch.randn(16, P, device=dev) / P ** 0.5
    for d in (1024, 4096, 32768):
        out = torch.empty(16, d, device=dev)
        ws = torch.empty(trak.workspace_bytes(16, P, d), dtype=torch.uint8, device=dev)
        t = timeit(lambda: trak.project_raw(a, out, P, 42, 0, "normal", workspace=ws), 1, 1)
        print(f"d = {d:5d}: {t * 1e3:9.1f} ms per 16 rows (workspace {ws.numel() / 2 ** 20:.0f} MiB)")


if __name__ == "__main__":
    kernels()
    features(int(sys.argv[1]) if len(sys.argv) > 1 else 100)
