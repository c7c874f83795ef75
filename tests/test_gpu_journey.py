"""GPU tests of Journey-TRAK: gad_ddpm_step against the fp64 restatement with a derived per-element bound, its row independence
and determinism, journey_latents and journey_gradient_features against the oracle U-Net, and the kept entry points end to end."""
import functools
import os

import numpy as np
import pytest
import torch

from jl_ref import jl_project
from journey_ref import ddpm_step

pytestmark = pytest.mark.gpu
dev = torch.device("cuda:0")
TINY = dict(block_out_channels=[32, 32, 64, 64], norm_num_groups=8)
SEEDS = [(42 << 32) | 1, (0x9E3779B9 << 32) | 0xFFFFFFFF, (7 << 32) | 123456]      # non-zero high words
STRIDE, GUARD = 10, 64


@functools.lru_cache(maxsize=None)
def _alphas(t):
    """(abar_t, abar_prev) of the CIFAR linear betas with stride 10, as python floats holding the fp32 table values"""
    import gad
    ac = gad.DDPMScheduler().alphas_cumprod
    return ac[t].item(), (ac[t - STRIDE].item() if t - STRIDE >= 0 else 1.0)


@functools.lru_cache(maxsize=None)
def _inputs(n):
    g = torch.Generator().manual_seed(n)
    return torch.randn(3, n, generator=g), torch.randn(3, n, generator=g)


@functools.lru_cache(maxsize=None)
def _want(n, t, clip, variance_type):
    x, eps = _inputs(n)
    return ddpm_step(x.numpy(), eps.numpy(), SEEDS, t, *_alphas(t), clip, variance_type)


def _step(x, eps, seeds, t, clip, variance_type, out=None):
    from gad import ops
    seeds = torch.tensor([s - (1 << 64) if s >= 1 << 63 else s for s in seeds], dtype=torch.int64, device=dev)
    out = ops.ddpm_step_raw(x, eps, seeds, t, *_alphas(t), clip, variance_type, out=out)
    torch.cuda.synchronize()
    return out


def _guarded(B, n):
    buf = torch.full((GUARD + B * n + GUARD,), float("nan"), device=dev)
    return buf, buf[GUARD:GUARD + B * n].view(B, n)


@pytest.mark.parametrize("clip", [0.0, 1.0])
@pytest.mark.parametrize("variance_type", ["fixed_small", "fixed_large"])
@pytest.mark.parametrize("t", [999, 10, 5, 0])
@pytest.mark.parametrize("n", [192, 3076])
def test_step_matches_the_restatement(n, t, variance_type, clip):
    """|got - want| <= 8 * 2^-23 * (c0 (|x| + sqrt(1 - abar_t) |eps|) / sqrt(abar_t) [x0 unclipped] + c0 clip [clipped] + c1 |x|
    + sigma |z|) + sigma * 1e-6 * (1 + |z|): eight fp32 roundings of the expression as written, plus the bound this project
    holds its device Box-Muller to (test_gpu_trak.py, test_one_hot_rows_return_rows_of_r)."""
    x, eps = _inputs(n)
    w = _want(n, t, clip, variance_type)
    buf, out = _guarded(3, n)
    got = _step(x.to(dev), eps.to(dev), SEEDS, t, clip, variance_type, out=out).cpu().numpy().astype(np.float64)
    ax, ae, az = np.abs(x.numpy().astype(np.float64)), np.abs(eps.numpy().astype(np.float64)), np.abs(w["z"])
    x0_mag = np.where(w["clipped"], clip, (ax + w["sb"] * ae) / w["sa"])
    bound = 8 * 2.0 ** -23 * (w["c0"] * x0_mag + w["c1"] * ax + w["sigma"] * az) + w["sigma"] * 1e-6 * (1 + az)
    err = np.abs(got - w["x_prev"])
    print(f"n={n} t={t} {variance_type} clip={clip}: max err {err.max():.3e}, max err / bound {(err / bound).max():.3f}, "
          f"clipped {w['clipped'].mean():.3f}")
    assert np.isfinite(got).all()
    assert (err <= bound).all(), (err / bound).max()
    assert torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[-GUARD:]).all()          # the guard bands are untouched
    if t == 999 and clip > 0:
        assert w["clipped"].mean() > 0.95                                                # the clip is active almost everywhere
    if t == 5:
        assert _alphas(t)[1] == 1.0 and w["sigma"] > 0                                   # abar_prev = 1, noise still added


@pytest.mark.parametrize("n", [192, 3076])
def test_step_at_t0_adds_no_noise(n):
    x, eps = (v.to(dev) for v in _inputs(n))
    small = _step(x, eps, SEEDS, 0, 1.0, "fixed_small")
    large = _step(x, eps, SEEDS, 0, 1.0, "fixed_large")
    assert torch.equal(small, large)                                 # the kernel's own mean, whatever the variance type
    other = _step(x, eps, [s + 1 for s in SEEDS], 0, 1.0, "fixed_small")
    assert torch.equal(small, other)                                 # ... and whatever the seed


def test_rows_are_independent_and_launches_repeat():
    n, t = 3076, 500
    g = torch.Generator().manual_seed(3)
    x, eps = torch.randn(5, n, generator=g).to(dev), torch.randn(5, n, generator=g).to(dev)
    seeds = [(42 << 32) | s for s in (9, 4, 2, 7, 5)]
    full = _step(x, eps, seeds, t, 1.0, "fixed_small")
    assert torch.equal(full, _step(x, eps, seeds, t, 1.0, "fixed_small"))                # a repeated launch
    alone = _step(x[1:2].contiguous(), eps[1:2].contiguous(), seeds[1:2], t, 1.0, "fixed_small")
    assert torch.equal(alone[0], full[1])                            # the row alone == the row placed second of five
    inplace = x.clone()
    assert _step(inplace, eps, seeds, t, 1.0, "fixed_small", out=inplace) is inplace
    assert torch.equal(inplace, full)                                # in place == out of place


def test_noise_streams_are_uncorrelated():
    """x = eps = 0 with fixed_large: x_prev = sigma z.  12 288 elements: the standard error of a correlation is 0.009."""
    n = 12288
    zero = torch.zeros(1, n, device=dev)

    def z(seed, t):
        out = _step(zero, zero, [seed], t, 0.0, "fixed_large").flatten().cpu().double()
        a_t, a_p = _alphas(t)
        return out / (1.0 - a_t / a_p) ** 0.5
    base = z(SEEDS[0], 500)
    assert abs(base.mean().item()) < 5 / n ** 0.5 and abs(base.var().item() - 1) < 5 * (2 / n) ** 0.5
    for other in (z(SEEDS[0] + 1, 500), z(SEEDS[0] ^ (1 << 32), 500), z(SEEDS[0], 499)):   # seed low / high word, t
        c = torch.corrcoef(torch.stack([base, other]))[0, 1].item()
        assert abs(c) < 0.05, c


# ---- trajectories and their features on the TINY U-Net of test_gpu_trak.py, against the oracle model ----
N_SAMPLES, K_PART, OPT_SEED = 3, 4, 42


@functools.lru_cache(maxsize=None)
def _models():
    import gad
    from oracle import diffusers_ref as R
    from src.ddpm_config import DDPMConfig
    ucfg = dict(DDPMConfig.cifar100_config["unet_config"], **TINY)
    scfg = DDPMConfig.cifar100_config["scheduler_config"]
    torch.manual_seed(0)
    ref = R.UNet2DModel(**ucfg)
    net = gad.UNet2DModel(**ucfg)
    net.load_state_dict(ref.state_dict())
    net.to(dev)
    net.flatten_parameters()
    return ref, net, gad.DDPMScheduler(**scfg)


@functools.lru_cache(maxsize=None)
def _latents(batch_size):
    from gad.trak import journey_latents
    _, net, sch = _models()
    return journey_latents(net, sch, N_SAMPLES, K_PART, opt_seed=OPT_SEED, batch_size=batch_size, device=dev)


@functools.lru_cache(maxsize=None)
def _oracle_latents():
    """The restatement on the CPU: the oracle U-Net with the same weights, stepped by journey_ref.ddpm_step in fp64 (the latent
    is rounded to fp32 where it enters the U-Net, as the engine holds it)."""
    from gad.trak import journey_timesteps
    ref, _, sch = _models()
    c = sch.config
    ts = journey_timesteps(K_PART, c.num_train_timesteps)
    stride = c.num_train_timesteps // 100
    ac = sch.alphas_cumprod
    clip = float(c.clip_sample_range) if c.clip_sample else 0.0
    x = torch.cat([torch.randn((1, 3, 32, 32), generator=torch.Generator(dev).manual_seed(s), device=dev).cpu()
                   for s in range(N_SAMPLES)])
    traj = [x.numpy().astype(np.float64)]
    seeds = [(OPT_SEED << 32) | s for s in range(N_SAMPLES)]
    with torch.no_grad():
        for t in ts[:-1]:
            eps = ref(x, torch.full((N_SAMPLES,), t, dtype=torch.long)).sample
            a_p = ac[t - stride].item() if t - stride >= 0 else 1.0
            w = ddpm_step(x.reshape(N_SAMPLES, -1).numpy(), eps.reshape(N_SAMPLES, -1).numpy(), seeds, t, ac[t].item(), a_p, clip,
                          c.variance_type)
            traj.append(w["x_prev"].reshape(x.shape))
            x = torch.from_numpy(w["x_prev"].astype(np.float32)).reshape(x.shape)
    return np.stack(traj[::-1], axis=1)                              # [N][K][C][H][W], index K - 1 = the initial noise


def _row_rel(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    flat = (got.shape[0] * got.shape[1], -1)
    return np.linalg.norm((got - want).reshape(flat), axis=1) / np.linalg.norm(want.reshape(flat), axis=1)


def test_journey_latents_match_the_oracle_trajectory():
    got = _latents(2)                                                # two batches: 2 rows, then 1
    assert got.shape == (N_SAMPLES, 4, 3, 32, 32) and got.dtype == torch.float32 and not got.is_cuda
    for s in range(N_SAMPLES):                                       # index K - 1 is the seeded draw, bit for bit
        want = torch.randn((1, 3, 32, 32), generator=torch.Generator(dev).manual_seed(s), device=dev)[0].cpu()
        assert torch.equal(got[s, 3], want)
    rel = _row_rel(got.numpy(), _oracle_latents())
    print("journey_latents vs oracle, relative row error:", rel)
    assert rel.max() <= 1e-4, rel


def test_journey_latents_do_not_depend_on_the_batch_size():
    a, b = _latents(2), _latents(3)
    assert torch.equal(a[:, 3], b[:, 3])
    rel = _row_rel(a.numpy(), b.numpy())
    assert rel.max() <= 1e-4, rel


def _oracle_gradients(latents, behaviour, timesteps, k_partition):
    """torch autograd per-sample gradients of the oracle model on the latents as they are (no add_noise), summed over the rows
    and divided by k_partition, laid out like the engine's flat gradient buffer"""
    from gad.coalition import seed_everything
    from gad.training import flat_views
    ref, net, _ = _models()
    ref_params = dict(ref.named_parameters())
    names = [n for n, _ in net.named_parameters()]
    P = net.flat[1].numel()
    like = torch.empty((latents.shape[0],) + tuple(latents.shape[2:]), device=dev)
    noises = []
    for t in timesteps:
        seed_everything(OPT_SEED * 1000 + t)
        noises.append(torch.randn_like(like).cpu())
    noise = torch.stack(noises, dim=1)
    ts = torch.tensor(list(timesteps))
    rows = []
    for i in range(latents.shape[0]):
        ref.zero_grad()
        pred = ref(latents[i, :len(timesteps)], ts).sample
        target = noise[i] if behaviour == "loss" else torch.zeros_like(pred)
        f = torch.nn.functional.mse_loss(pred, target, reduction="none").reshape(len(timesteps), -1).mean(dim=1)
        (f.sum() / k_partition).backward()
        flat = torch.zeros(P)
        for v, n in zip(flat_views([p for _, p in net.named_parameters()], flat), names):
            v.copy_(ref_params[n].grad)
        rows.append(flat.numpy().astype(np.float64))
    return np.stack(rows)


def test_journey_features_match_autograd_per_sample_gradients():
    from gad.trak import Projector, journey_gradient_features, selected_timesteps
    _, net, sch = _models()
    latents = _latents(2)
    timesteps, d = selected_timesteps("uniform", K_PART), 64
    assert timesteps == [0, 250, 500, 750]
    proj = Projector(grad_dim=net.flat[1].numel(), proj_dim=d, seed=OPT_SEED, proj_type="normal", device=dev, max_batch_size=2)
    feats = {}
    for behaviour in ("loss", "mean-squared-l2-norm"):
        got = feats[behaviour] = journey_gradient_features(net, sch, latents, behaviour, timesteps, proj, opt_seed=OPT_SEED,
                                                           k_partition=K_PART)
        want = jl_project(_oracle_gradients(latents, behaviour, timesteps, K_PART), d, OPT_SEED)
        rel = np.linalg.norm(got.numpy() - want, axis=1) / np.linalg.norm(want, axis=1)
        print(behaviour, "relative row error:", rel)
        assert rel.max() <= 1e-4, (behaviour, rel)
    # the divisor is k_partition, not the number of rows
    half = journey_gradient_features(net, sch, latents, "loss", timesteps, proj, opt_seed=OPT_SEED, k_partition=2 * K_PART)
    full = feats["loss"]
    assert ((2 * half - full).norm(dim=1) / full.norm(dim=1)).max().item() <= 1e-5


def test_journey_entry_points_end_to_end(tmp_path, monkeypatch):
    import gad
    import src.constants as constants
    from src.attributions.methods import d_trak_grad as D
    from src.attributions.methods.compute_gradient_score import compute_gradient_scores
    from src.ddpm_config import DDPMConfig
    monkeypatch.setenv("GAD_SYNTH_SCALE", "0.00061")                 # cifar2: 6 training images
    monkeypatch.setattr(constants, "OUTDIR", str(tmp_path))
    mdir = tmp_path / "cifar2" / "retrain" / "models" / "full"
    mdir.mkdir(parents=True)
    torch.manual_seed(0)
    net = gad.UNet2DModel(**dict(DDPMConfig.cifar2_config["unet_config"], **TINY))
    torch.save({"unet": net.state_dict()}, mdir / f"ckpt_steps_{3:0>8}.pt")
    flags = ["--method", "retrain", "--dataset", "cifar2", "--model_behavior", "loss", "--t_strategy", "uniform",
             "--k_partition", "3", "--projector_dim", "64", "--outdir", str(tmp_path)]

    def run(extra=()):
        a = D.parse_args(flags + list(extra))
        a.unet_overrides = TINY
        return D.main(a)

    assert os.path.getsize(run()) == 6 * 64 * 4                      # the train features
    gen = ["--calculate_gen_grad", "--n_samples", "3"]
    path = run(gen)
    assert path == str(tmp_path / "cifar2" / "d_trak" / "full" / "gen_f=loss_t=uniform_k=3_d=64")
    assert os.path.getsize(path) == 3 * 64 * 4
    first = np.fromfile(path, dtype=np.float32).reshape(3, 64).copy()
    assert np.isfinite(first).all() and (np.abs(first).sum(1) > 0).all()
    run(gen)
    assert np.array_equal(first, np.fromfile(path, dtype=np.float32).reshape(3, 64))         # rerun: bit-identical

    from types import SimpleNamespace
    args = SimpleNamespace(dataset="cifar2", sample_dir=None, gradient_type="journey_trak", k_partition=3, projector_dim=64,
                           sample_size=3, model_behavior_key="fid", by_class=False, by="mean")
    scores = compute_gradient_scores(args)
    assert scores.shape == (3, 6) and np.isfinite(scores).all()
