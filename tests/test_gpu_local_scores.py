"""GPU tests of the local model behaviours: the three kernels of csrc/local.hip against fp64 host arithmetic and
oracle/skimage_ref.py, the wide-launch engine gad.local_model_behaviors against the reference-shaped loop of tests/local_ref.py
run on the same gad pipelines, its launch shapes at the defaults, and the two entry points end to end.

Bounds.  SSIM: 1e-10 absolute against the fp64 loop oracle - tools/ssim_precision.py measures 2.5e-14 for the kernel's
arithmetic (fp64 products and sums) and 2.6e-6 / 1.2e-5 for the two fp32 variants, so 1e-10 leaves four decades for another
summation order and is failed by either fp32 variant.  MSE / NRMSE: 1e-10 relative against float64 numpy (fp64 sums of
<= 196 608 exactly converted terms differ between two orders by at most n * 2^-53 ~ 2e-11).  add_noise: 4 * 2^-24 *
(|sqrt(ac) x0| + |sqrt(1-ac) eps|) (two fp32 coefficients, two products, one sum).  Segment means: 2^-22 relative (one fp32
rounding of an fp64 sum, with margin).  Losses under another launch plan: 1e-5 relative, images: 1.5 grey levels - the
project's bounds for the same situations (test_gpu_fullsize.py, test_fused_sampler_at_bench_width_equals_per_batch_launches)."""
import json
import math
import os
import re

import numpy as np
import pytest
import torch

from local_ref import _one_image, local_behaviors_loop, mse_f64
from oracle.skimage_ref import ssim_loops

pytestmark = pytest.mark.gpu
dev = torch.device("cuda:0")
TINY = dict(block_out_channels=[32, 32, 64, 64], norm_num_groups=8)
SSIM_ATOL, REL = 1e-10, 1e-10


@pytest.fixture(scope="module")
def ops():
    from gad import ops
    return ops


# ---------------------------------------------------------------- 3. gad_image_metrics ----
def metric_pairs(h, w, c, rng):
    """the six recipes: uniform pair, smooth image vs itself + N(0, 0.01) clipped, identical, constants, bright, binary"""
    f = np.float32
    smooth = np.clip(np.kron(rng.random((h // 4 + 2, w // 4 + 2, c)), np.ones((4, 4, 1)))[:h, :w], 0, 1).astype(f)
    same = rng.random((h, w, c)).astype(f)
    return [("uniform", rng.random((h, w, c)).astype(f), rng.random((h, w, c)).astype(f)),
            ("smooth+noise", smooth, np.clip(smooth + 0.01 * rng.standard_normal(smooth.shape), 0, 1).astype(f)),
            ("identical", same, same.copy()),
            ("constant", np.full((h, w, c), 0.3, f), np.full((h, w, c), 0.7, f)),
            ("bright", (0.98 + 0.02 * rng.random((h, w, c))).astype(f), (0.98 + 0.02 * rng.random((h, w, c))).astype(f)),
            ("binary", (rng.random((h, w, c)) < 0.5).astype(f), (rng.random((h, w, c)) < 0.5).astype(f))]


def check_metrics(got, a, b, what):
    """one [3] fp64 row of gad_image_metrics against the oracle on the same fp32 pair"""
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    mse = mse_f64(a, b)
    nrmse = math.sqrt(mse) / math.sqrt(float(np.mean(a64 * a64)))
    ssim = ssim_loops(a, b, data_range=1.0)
    print(f"{what}: mse rel {abs(got[0] - mse) / max(mse, 1e-300):.2e}  nrmse rel {abs(got[1] - nrmse) / max(nrmse, 1e-300):.2e}  "
          f"ssim abs {abs(got[2] - ssim):.2e}")
    if np.array_equal(a, b):
        assert got[0] == 0.0 and got[1] == 0.0 and got[2] == 1.0, (what, got)
    assert abs(got[0] - mse) <= REL * mse, (what, got[0], mse)
    assert abs(got[1] - nrmse) <= REL * nrmse, (what, got[1], nrmse)
    assert abs(got[2] - ssim) <= SSIM_ATOL, (what, got[2], ssim)


@pytest.mark.parametrize("h,w,c", [(28, 28, 1), (28, 28, 3), (32, 32, 1), (32, 32, 3), (64, 64, 1), (64, 64, 3), (40, 24, 1),
                                   (40, 24, 3), (256, 256, 1)])
def test_image_metrics_against_the_loop_oracle(ops, h, w, c):
    rng = np.random.default_rng(1000 * h + 10 * w + c)
    pairs = metric_pairs(h, w, c, rng)
    a = torch.from_numpy(np.stack([p[1] for p in pairs])).to(dev)
    b = torch.from_numpy(np.stack([p[2] for p in pairs])).to(dev)
    got = ops.image_metrics_raw(a, b)                                   # all pairs of this size in one launch
    assert got.dtype == torch.float64 and got.shape == (len(pairs), 3)
    g = got.cpu().numpy()
    for i, (name, pa, pb) in enumerate(pairs):
        check_metrics(g[i], pa, pb, f"{h}x{w}x{c} {name}")
    # a pair's result depends neither on its position in the batch nor on N, and two runs agree bit for bit
    assert torch.equal(ops.image_metrics_raw(a, b), got)
    perm = torch.tensor([4, 0, 5, 2, 1, 3], device=dev)
    assert torch.equal(ops.image_metrics_raw(a[perm].contiguous(), b[perm].contiguous()), got[perm])
    for i in (0, 4):
        assert torch.equal(ops.image_metrics_raw(a[i:i + 1].contiguous(), b[i:i + 1].contiguous()), got[i:i + 1])
    big = ops.image_metrics_raw(torch.cat([a, a, b]), torch.cat([b, a, b]))
    assert torch.equal(big[:len(pairs)], got)
    assert bool((big[len(pairs):, :2] == 0).all()) and bool((big[len(pairs):, 2] == 1).all())


def test_image_metrics_refuses_small_images_and_other_windows(ops):
    from gad._capi import GadError
    x = torch.rand(2, 6, 32, 3, device=dev)
    with pytest.raises(GadError, match="H < win"):
        ops.image_metrics_raw(x, x)
    rng = np.random.default_rng(5)
    a, b = rng.random((1, 20, 17, 2)).astype(np.float32), rng.random((1, 20, 17, 2)).astype(np.float32)
    for win in (3, 11):                                                  # not the reference's call, but the same definition
        got = ops.image_metrics_raw(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev), win=win).cpu().numpy()[0]
        assert abs(got[2] - ssim_loops(a[0], b[0], data_range=1.0, win=win)) <= SSIM_ATOL


# ---------------------------------------------------------------- 4. gad_add_noise_bcast ----
@pytest.mark.parametrize("C,H,W", [(3, 32, 32), (1, 28, 28), (3, 5, 7)])
@pytest.mark.parametrize("draws", [1, 3])
def test_add_noise_bcast_against_fp64(ops, C, H, W, draws):
    import gad
    T, images = 7, 3                                                    # T is no multiple of the 256-thread block
    rpi = draws * T
    R = images * rpi
    g = torch.Generator().manual_seed(C * 100 + H + draws)
    x0, eps = torch.rand(images, C, H, W, generator=g), torch.randn(R, C, H, W, generator=g)
    sch = gad.DDIMScheduler()
    t = torch.tensor([999, 857, 571, 300, 142, 1, 0])
    ac = sch.alphas_cumprod
    got = ops.add_noise_bcast_raw(x0.to(dev), eps.to(dev), t.to(dev), ac.to(dev), rpi)
    assert got.shape == (R, H, W, C)
    a = ac[t.repeat(R // T)].double()
    A = a.sqrt()[:, None, None, None] * x0.repeat_interleave(rpi, 0).double()
    B = (1 - a).sqrt()[:, None, None, None] * eps.double()
    bound = (4 * 2.0 ** -24 * (A.abs() + B.abs())).permute(0, 2, 3, 1)
    err = (got.cpu().double() - (A + B).permute(0, 2, 3, 1)).abs()
    print(f"add_noise_bcast C={C} {H}x{W} rows/image={rpi}: max err / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= bound).all())
    # layout: the three-pass form it replaces
    rows = x0.repeat_interleave(rpi, 0).contiguous().to(dev)
    want = ops.nchw_to_nhwc_raw(sch.add_noise(rows, eps.to(dev), t.repeat(R // T).to(dev)))
    assert bool(((got - want).abs().cpu().double() <= bound).all())
    # a timestep outside the table is not read: NaN rows, nothing else
    bad = ops.add_noise_bcast_raw(x0.to(dev), eps.to(dev), torch.tensor([999, 1000, 571, 300, 142, -1, 0], device=dev),
                                  ac.to(dev), rpi)
    nan_rows = torch.isnan(bad).flatten(1).all(1).cpu()
    assert nan_rows.tolist() == [(r % T) in (1, 5) for r in range(R)]
    assert torch.equal(bad[~nan_rows.to(dev)], got[~nan_rows.to(dev)])


# ---------------------------------------------------------------- 5. gad_mse_segments ----
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("HW", [(8, 8), (32, 32), (64, 64)])
@pytest.mark.parametrize("rps", [1, 7, 100])
def test_mse_segments_against_fp64(ops, C, HW, rps):
    H, W = HW
    S = 3
    R = S * rps
    g = torch.Generator().manual_seed(C + H + rps)
    pred, eps = torch.randn(R, H, W, C, generator=g).to(dev), torch.randn(R, C, H, W, generator=g).to(dev)
    got = ops.mse_segments_raw(pred, eps, rps)
    want = (pred.double() - eps.double().permute(0, 2, 3, 1)).pow(2).view(S, -1).mean(1)
    rel = ((got.double() - want).abs() / want).max().item()
    print(f"mse_segments C={C} HW={H * W} rows/segment={rps}: max rel err {rel:.2e}")
    assert got.dtype == torch.float32 and got.shape == (S,) and rel <= 2.0 ** -22
    assert torch.equal(ops.mse_segments_raw(pred, eps, rps), got)                       # run to run
    mid = ops.mse_segments_raw(pred[rps:2 * rps].contiguous(), eps[rps:2 * rps].contiguous(), rps)
    assert torch.equal(mid, got[1:2])                                                   # the same segment in another R
    two = ops.mse_segments_raw(pred[rps:].contiguous(), eps[rps:].contiguous(), rps)
    assert torch.equal(two, got[1:])


def test_local_kernels_stay_inside_their_buffers(ops):
    """out, xt and both workspaces at exactly their sizes between poisoned guard bands (the pattern of test_gpu_guards.py)"""
    import test_gpu_guards as G
    g = torch.Generator().manual_seed(3)
    T, rpi, C, H, W = 7, 14, 3, 9, 11
    R = 3 * rpi
    x0, eps = torch.rand(3, C, H, W, generator=g).to(dev), torch.randn(R, C, H, W, generator=g).to(dev)
    t, ac = torch.tensor([900, 700, 500, 300, 100, 10, 0], device=dev), torch.linspace(0.9999, 0.01, 1000).to(dev)
    pred = torch.randn(R, H, W, C, generator=g).to(dev)
    a, b = torch.rand(5, 40, 24, 3, generator=g).to(dev), torch.rand(5, 40, 24, 3, generator=g).to(dev)
    plain = (ops.add_noise_bcast_raw(x0, eps, t, ac, rpi), ops.mse_segments_raw(pred, eps, T), ops.image_metrics_raw(a, b))
    guards = G.Guards()
    ops.SCRATCH_ALLOC, ops.OUT_ALLOC = guards.scratch, guards.out
    ops.OUT_ALLOC_DT = lambda shape, device, dtype: guards._alloc("out64", 8 * math.prod(shape), device).view(dtype).view(shape)
    try:
        guarded = (ops.add_noise_bcast_raw(x0, eps, t, ac, rpi), ops.mse_segments_raw(pred, eps, T), ops.image_metrics_raw(a, b))
        torch.cuda.synchronize()
    finally:
        ops.SCRATCH_ALLOC = ops.OUT_ALLOC = ops.OUT_ALLOC_DT = None
    guards.check()
    assert sorted(guards.kinds()) == ["metrics_ws", "out", "out", "out64", "segments_ws"]
    for p, q in zip(plain, guarded):
        assert torch.equal(p, q)


# ---------------------------------------------------------------- 6. engine vs the reference-shaped loop ----
def _small_pipes():
    import gad
    from src.ddpm_config import DDPMConfig
    ucfg = dict(DDPMConfig.cifar100_config["unet_config"], **TINY)
    pipes = []
    for seed in (0, 1):
        torch.manual_seed(seed)
        pipes.append(gad.DDPMPipeline(gad.UNet2DModel(**ucfg).to(dev).eval(), gad.DDIMScheduler()))
    return pipes


def rel_close(a, b, rel):
    return all(abs(x - y) <= rel * abs(y) for x, y in zip(a, b))


def test_engine_matches_the_reference_shaped_loop():
    import gad
    full_pipe, pipe = _small_pipes()
    n, k, T = 5, 3, 6
    res = gad.local_model_behaviors(full_pipe, pipe, n, k, T, return_images=True)
    full, removal = res["full_images"], res["images"]
    assert full.shape == removal.shape == (n, 32, 32, 3) and res.x0_space == "image"
    assert all(len(res[key]) == n for key in ("mse", "nrmse", "ssim", "diffusion_loss"))
    # the loss of both on the engine's own full images: same noise values by construction, another launch width
    loop = local_behaviors_loop(full_pipe, pipe, n, k, T, full_images=full, with_metrics=False, return_images=True)
    for s in range(n):
        print(f"image {s}: diffusion loss engine {res['diffusion_loss'][s]:.8e} loop {loop['diffusion_loss'][s]:.8e} "
              f"rel {abs(res['diffusion_loss'][s] - loop['diffusion_loss'][s]) / loop['diffusion_loss'][s]:.2e}")
    assert rel_close(res["diffusion_loss"], loop["diffusion_loss"], 1e-5)
    # the metrics, recomputed by the oracle on the engine's own image pairs
    fa, ra = full.cpu().numpy(), removal.cpu().numpy()
    for s in range(n):
        check_metrics((res["mse"][s], res["nrmse"][s], res["ssim"][s]), fa[s], ra[s], f"engine pair {s}")
    # wide-launch generation against the batch-1 pipeline calls: no pixel more than one grey level apart
    one = np.stack([_one_image(full_pipe, s, T)[0] for s in range(n)])
    d_full, d_rem = np.abs(one - fa).max() * 255, np.abs(loop["images"] - ra).max() * 255
    print(f"wide vs batch-1 generation: max difference {d_full:.4f} (full) {d_rem:.4f} (removal) grey levels")
    assert d_full <= 1.5 and d_rem <= 1.5
    # launch plans: whole draws per launch, several images per launch, results independent of the plan
    by_plan = {}
    for rpl, rows in ((T, (T,) * (n * k)), (3 * T, (3 * T,) * n), (1000, (n * k * T,))):
        r = gad.local_model_behaviors(None, pipe, n, k, T, rows_per_launch=rpl, full_images=full)
        assert r.launch_rows == rows, (rpl, r.launch_rows)
        again = gad.local_model_behaviors(None, pipe, n, k, T, rows_per_launch=rpl, full_images=full)
        assert again["diffusion_loss"] == r["diffusion_loss"] and again["ssim"] == r["ssim"] and again["mse"] == r["mse"]
        by_plan[rpl] = r["diffusion_loss"]
        assert r["mse"] == res["mse"] and r["nrmse"] == res["nrmse"] and r["ssim"] == res["ssim"]
    assert by_plan[1000] == res["diffusion_loss"]
    assert rel_close(by_plan[T], by_plan[1000], 1e-5) and rel_close(by_plan[3 * T], by_plan[1000], 1e-5)
    # 5 images at 2 draws x 6 steps under 30 rows per launch: two images per launch, the last one alone
    r = gad.local_model_behaviors(full_pipe, pipe, 5, 2, T, rows_per_launch=30)
    assert r.launch_rows == (24, 24, 12)


# ---------------------------------------------------------------- 7. launch shape of the defaults ----
def test_default_launch_shape_on_the_full_width_unet():
    import gad
    from src.ddpm_config import DDPMConfig
    torch.manual_seed(0)
    net = gad.UNet2DModel(**DDPMConfig.cifar100_config["unet_config"]).to(dev).eval()
    pipe = gad.DDPMPipeline(net, gad.DDIMScheduler())
    res = gad.local_model_behaviors(pipe, pipe, 2, 10, 100, return_images=True)
    assert res.launch_rows == (1000, 1000)
    assert res["mse"] == [0.0, 0.0] and res["nrmse"] == [0.0, 0.0] and res["ssim"] == [1.0, 1.0]
    l0, l1 = res["diffusion_loss"]
    print(f"full-width CIFAR U-Net, full == removal: diffusion losses {l0:.8e} {l1:.8e}")
    assert math.isfinite(l0) and math.isfinite(l1) and l0 > 0 and l1 > 0 and l0 != l1
    # the 1000-row launches against the 100-row loop on the same full images: the project's bound for one loss under another plan
    loop = local_behaviors_loop(pipe, pipe, 2, 10, 100, full_images=res["full_images"], with_metrics=False)
    print("   the loop's, on the same images: " + " ".join(f"{v:.8e}" for v in loop["diffusion_loss"]))
    assert rel_close(res["diffusion_loss"], loop["diffusion_loss"], 1e-5)


def test_mnist_and_celeba_latent_shapes():
    import gad
    from src.ddpm_config import DDPMConfig
    torch.manual_seed(0)
    mnist = dict(DDPMConfig.mnist_config["unet_config"], block_out_channels=[32, 32, 64, 64], norm_num_groups=8)
    nets = [gad.UNet2DModel(**mnist).to(dev).eval() for _ in range(2)]
    full_pipe, pipe = (gad.DDPMPipeline(n, gad.DDIMScheduler()) for n in nets)
    res = gad.local_model_behaviors(full_pipe, pipe, 3, 2, 5, return_images=True)
    assert res["full_images"].shape == (3, 32, 32, 1) and res.launch_rows == (30,) and res.x0_space == "image"
    loop = local_behaviors_loop(full_pipe, pipe, 3, 2, 5, full_images=res["full_images"], with_metrics=False)
    assert rel_close(res["diffusion_loss"], loop["diffusion_loss"], 1e-5)
    fa, ra = res["full_images"].cpu().numpy(), res["images"].cpu().numpy()
    check_metrics((res["mse"][0], res["nrmse"][0], res["ssim"][0]), fa[0], ra[0], "mnist-shaped pair 0")

    celeba = dict(DDPMConfig.celeba_config["unet_config"], block_out_channels=[32, 64, 64, 64], attention_head_dim=8,
                  norm_num_groups=8, sample_size=64)
    sc = {k: v for k, v in DDPMConfig.celeba_config["scheduler_config"].items() if not k.startswith("_")}
    nets = [gad.UNet2DModel(**celeba).to(dev).eval() for _ in range(2)]
    full_pipe, pipe = (gad.LDMPipeline(unet=n, vqvae=None, scheduler=gad.DDIMScheduler(**sc)) for n in nets)
    res = gad.local_model_behaviors(full_pipe, pipe, 2, 2, 4, return_images=True)
    assert res["full_images"].shape == (2, 64, 64, 3) and res.launch_rows == (16,) and res.x0_space == "latent-as-image"
    loop = local_behaviors_loop(full_pipe, pipe, 2, 2, 4, full_images=res["full_images"], with_metrics=False)
    assert rel_close(res["diffusion_loss"], loop["diffusion_loss"], 1e-5)
    fa, ra = res["full_images"].cpu().numpy(), res["images"].cpu().numpy()
    check_metrics((res["mse"][1], res["nrmse"][1], res["ssim"][1]), fa[1], ra[1], "celeba-latent-shaped pair 1")


# ---------------------------------------------------------------- 8. entry points ----
VALUE = re.compile(r"^-?\d\.\d{8}e[+-]\d\d$")


def test_local_entry_points_on_gpu(tmp_path, monkeypatch):
    from src.ddpm_config import DDPMConfig
    cfg = {**DDPMConfig.cifar100_config}
    cfg["unet_config"] = dict(cfg["unet_config"], **TINY)
    cfg["n_samples"] = 4
    cfg["training_steps"] = dict(cfg["training_steps"], retrain=3)
    cfg["ckpt_freq"] = dict(cfg["ckpt_freq"], retrain=3)
    cfg["sample_freq"] = dict(cfg["sample_freq"], retrain=3)
    monkeypatch.setattr(DDPMConfig, "cifar100_config", cfg)
    from unconditional_generation import calculate_local_scores as local_main
    from unconditional_generation import main as train_main
    from unconditional_generation import unlearn as unlearn_main
    out, db, db2 = str(tmp_path / "res"), str(tmp_path / "db.jsonl"), str(tmp_path / "local.jsonl")
    train = ["--dataset", "toy2", "--method", "retrain", "--outdir", out, "--batch_size", "16", "--num_inference_steps", "10",
             "--log_freq", "1"]
    assert train_main.main(train_main.parse_args(train))
    assert train_main.main(train_main.parse_args(train + ["--removal_dist", "shapley", "--removal_seed", "1"]))
    mdir = os.path.join(out, "toy2", "retrain", "models", "full")
    rdir = os.path.join(out, "toy2", "retrain", "models", "shapley", "shapley_seed=1")
    ck = torch.load(os.path.join(mdir, "ckpt_steps_00000003.pt"), weights_only=False)
    pdir = os.path.join(out, "toy2", "pruned", "models", "pruner=magnitude_pruning_ratio=0.3_threshold=0.05")
    os.makedirs(pdir)
    torch.save({"unet": ck["unet"], "unet_config": ck["unet_config"]}, os.path.join(pdir, "ckpt_steps_00000000.pt"))
    n, common = 4, ["--n_samples", "4", "--n_noises", "3", "--num_inference_steps", "10"]
    keys = [f"generated_image_{s}_{k}" for s in range(n) for k in ("mse", "nrmse", "ssim", "diffusion_loss")] + \
        ["avg_mse", "avg_nrmse", "avg_ssim", "avg_total_loss"]
    # sFT for three steps, then the local behaviours of the fine-tuned model
    sft = ["--dataset", "toy2", "--removal_dist", "shapley", "--removal_seed", "1", "--outdir", out, "--db", db, "--batch_size", "8",
           "--model_behavior", "local"] + common
    assert unlearn_main.main(unlearn_main.parse_args(sft + ["--method", "gd", "--load", mdir, "--gd_steps", "3"]))
    # ... and of the coalition's retrained model as it is (no fine-tuning step), which calculate_local_scores.py can load too
    assert unlearn_main.main(unlearn_main.parse_args(sft + ["--method", "gd_u", "--load", rdir, "--gd_steps", "0", "--use_ema"]))
    assert local_main.main(local_main.parse_args(["--dataset", "toy2", "--method", "retrain", "--removal_dist", "shapley",
                                                  "--removal_seed", "1", "--full_model_dir", mdir, "--outdir", out, "--db", db2,
                                                  "--use_ema", "--exp_name", "local"] + common))
    tuned, kept, local = [json.loads(l) for l in open(db)] + [json.loads(open(db2).readline())]
    for row in (tuned, kept, local):
        assert all(isinstance(row[k], str) and VALUE.match(row[k]) and math.isfinite(float(row[k])) for k in keys)
        assert len(row["remaining_idx"]) == 64 and len(row["removed_idx"]) == 64
    assert tuned["trained_steps"] == 3 and kept["trained_steps"] == 0 and local["removal_model_dir"] == rdir
    assert kept["remaining_idx"] == local["remaining_idx"] == tuned["remaining_idx"]
    assert float(tuned["avg_mse"]) > 0 and float(kept["avg_mse"]) > 0
    for k in keys:                                                      # the same two models through both entry points
        a, b = float(kept[k]), float(local[k])
        print(f"{k}: unlearn {kept[k]} calculate_local_scores {local[k]}")
        if k.endswith("loss"):
            assert abs(a - b) <= 1e-5 * abs(b), k
        elif k.endswith("ssim"):
            assert abs(a - b) <= SSIM_ATOL + 1e-8, k                    # 8 printed decimals
        else:
            assert abs(a - b) <= (REL + 1e-8) * abs(b), k
    for s in range(n):
        assert os.path.exists(os.path.join(out, "toy2", "gd_u", "samples", "shapley", "shapley_seed=1", f"generated_image_{s}.png"))
        assert os.path.exists(os.path.join(out, "toy2", "local_scores", "ema_generated_samples", f"generated_image_{s}.png"))
