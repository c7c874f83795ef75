"""GPU tests of influence unlearning: the two WoodFisher kernels (csrc/influence.hip) against fp64 numpy on the sizes at which
they can go wrong, `gad.InfluenceUnlearner` against tests/influence_ref.py over the oracle U-Net in double, and
`unlearn.py --method iu` on the HIP backend.

Sizes: 1 and 3 (tail only), 4 (one float4), 1027 (one workgroup, ragged), 262 147 (256 workgroups + tail) and
2 097 152 + 1024 + 3 (one float4 group per lane of a workgroup past the 2048-workgroup cap: the grid-stride loop takes a second
trip).  Every launch below runs with its vectors, its two doubles and its exactly-sized workspace between poisoned bands."""
import functools
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
dev = torch.device("cuda:0")
SIZES = (1, 3, 4, 1027, 262147, 2048 * 256 * 4 + 1024 + 3)
FAMILIES = ("normal", "positive", "cancelling")
PAD, POISON = 4096, 0xA5                # band bytes on each side (a multiple of 16: what follows stays 16-byte aligned)


@pytest.fixture(scope="module")
def lib():
    from gad import _capi
    return _capi.load()


def _stream():
    from gad import ops
    return ops._stream()


class Banded:
    """`nbytes` of device memory between two poisoned bands"""

    def __init__(self, nbytes):
        self.buf = torch.full((PAD + nbytes + PAD,), POISON, dtype=torch.uint8, device=dev)
        self.nbytes = nbytes
        self.ptr = self.buf.data_ptr() + PAD
        assert self.ptr % 16 == 0

    def view(self, dtype):
        return self.buf[PAD:PAD + self.nbytes].view(dtype)

    def intact(self):
        return bool((self.buf[:PAD] == POISON).all()) and bool((self.buf[PAD + self.nbytes:] == POISON).all())


def banded_f32(a):
    b = Banded(a.size * 4)
    b.view(torch.float32).copy_(torch.tensor(a))
    return b


@functools.lru_cache(maxsize=None)
def vectors(n, family):
    """seeded fp32 (o, k, g) on the host; computed once per (n, family) and never written"""
    rng = np.random.default_rng(1000 + n % 997 + 7 * FAMILIES.index(family))
    g = rng.standard_normal(n).astype(np.float32)
    o = rng.standard_normal(n).astype(np.float32)
    k = rng.standard_normal(n).astype(np.float32)
    if family == "positive":                       # o = g: every term of o.g is a square
        o = g.copy()
    elif family == "cancelling":                   # k = g with alternating signs times a ramp up to 1e3: k.g cancels
        sign = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
        k = (g * sign * np.linspace(1.0, 1e3, n)).astype(np.float32)
    for a in (o, k, g):
        a.setflags(write=False)
    return o, k, g


def dot64(a, b):
    """(a.b, sum |a_i b_i|): exact fp64 products summed pairwise in extended precision"""
    p = a.astype(np.float64) * b.astype(np.float64)
    return float(p.astype(np.longdouble).sum()), float(np.abs(p).astype(np.longdouble).sum())


def launch_dots(lib, o, k, g, n, dots=None, ws=None):
    need = lib.gad_wf_dots_workspace_bytes(n)
    dots = Banded(16) if dots is None else dots
    ws = Banded(need) if ws is None else ws
    rc = lib.gad_wf_dots(o.ptr, k.ptr, g.ptr, n, dots.ptr, ws.ptr, need, _stream())
    assert rc == 0, lib.gad_last_error()
    return dots, ws


# ---- 5 ----
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("n", SIZES)
def test_wf_dots_against_fp64(lib, n, family):
    """|err| <= 1e-10 * sum |a_i b_i| for each dot product: the products are exact in fp64 and the fp64 sums cost at most
    n * 2^-53 = 2e-10 relative to sum |.| at n = 2e6 in the worst order; the tree order is far below that.  Two launches
    give equal bits; the two doubles and the workspace at exactly the queried size keep their bands intact."""
    o, k, g = vectors(n, family)
    bo, bk, bg = banded_f32(o), banded_f32(k), banded_f32(g)
    d1, w1 = launch_dots(lib, bo, bk, bg, n)
    d2, w2 = launch_dots(lib, bo, bk, bg, n)
    got = d1.view(torch.float64).cpu().numpy()
    for i, a in enumerate((o, k)):
        want, scale = dot64(a, g)
        err = abs(float(got[i]) - want)
        print(f"n={n} {family} dot{i}: got {got[i]:.17e} want {want:.17e} err/sum|.| = {err / scale:.3e}")
        assert err <= 1e-10 * scale, (i, err / scale)
    assert got.tobytes() == d2.view(torch.float64).cpu().numpy().tobytes()
    for b in (d1, w1, d2, w2, bo, bk, bg):
        assert b.intact()
    for b, a in ((bo, o), (bk, k), (bg, g)):                       # inputs are read, never written
        assert np.array_equal(b.view(torch.float32).cpu().numpy(), a)


# ---- 6 ----
def update64(o, k, d0, d1, N):
    """fp64 step from fp32 inputs -> (o', k', bound_o, bound_k): per element 2^-22 (|x| + |c x_o|), one rounding of the
    coefficient and one of the fma"""
    o64, k64 = o.astype(np.float64), k.astype(np.float64)
    ck, co = d1 / (N + d0), d0 / (N + d0)
    return (o64 - co * o64, k64 - ck * o64, 2.0 ** -22 * (np.abs(o64) + np.abs(co * o64)), 2.0 ** -22 * (np.abs(k64) + np.abs(ck * o64)))


@pytest.mark.parametrize("dots,N", [((0.731, -1.913), 3.0), ((3.0, 1.5), 3.0)], ids=["generic", "c_o=0.5"])
@pytest.mark.parametrize("n", SIZES)
def test_wf_update_against_fp64(lib, n, dots, N):
    """k' and o' against fp64 of the same fp32 inputs and the same dots.  With dots = (3, 1.5), N = 3 the coefficients are
    c_o = 0.5, c_k = 0.25: a k updated from the NEW o would be off by 0.125 |o|, 1e-1 at unit scale."""
    o, k, _ = vectors(n, "normal")
    bo, bk, bd = banded_f32(o), banded_f32(k), Banded(16)
    bd.view(torch.float64).copy_(torch.tensor(dots, dtype=torch.float64))
    assert lib.gad_wf_update(bo.ptr, bk.ptr, bd.ptr, N, n, _stream()) == 0, lib.gad_last_error()
    o1, k1 = bo.view(torch.float32).cpu().numpy().astype(np.float64), bk.view(torch.float32).cpu().numpy().astype(np.float64)
    wo, wk, bound_o, bound_k = update64(o, k, dots[0], dots[1], N)
    print(f"n={n}: max |k' - k'_64| / bound = {np.max(np.abs(k1 - wk) / np.maximum(bound_k, 1e-300)):.3f}, "
          f"max |o' - o'_64| / bound = {np.max(np.abs(o1 - wo) / np.maximum(bound_o, 1e-300)):.3f}")
    assert np.all(np.abs(k1 - wk) <= bound_k) and np.all(np.abs(o1 - wo) <= bound_o)
    if dots == (3.0, 1.5) and n >= 1027:
        wrong = k.astype(np.float64) - 0.25 * wo                    # what the wrong order would give
        assert np.max(np.abs(wrong - wk)) > 1e-1
    assert bo.intact() and bk.intact() and bd.intact()
    assert np.array_equal(bd.view(torch.float64).cpu().numpy(), np.array(dots))


@pytest.mark.parametrize("n", (1027, 262147))
def test_wf_three_chained_iterations(lib, n):
    """dots + update three times against the fp64 recursion from the same fp32 start, within three times the one-step bound
    evaluated on the fp64 trajectory's magnitudes.  Gradients share a direction and have unit norm, o starts as the first of them
    (as in the recursion), k leans on the same direction and N = 3, so N + o.g stays away from 0 and the coefficients are O(0.1)."""
    rng = np.random.default_rng(n)
    base = rng.standard_normal(n)
    gs = [((base + 0.5 * rng.standard_normal(n)) / np.sqrt(1.25 * n)).astype(np.float32) for _ in range(4)]
    o, k, N = gs[0].copy(), ((0.5 * base + rng.standard_normal(n)) / np.sqrt(1.25 * n)).astype(np.float32), 3.0
    bo, bk, dots, ws = banded_f32(o), banded_f32(k), Banded(16), Banded(lib.gad_wf_dots_workspace_bytes(n))
    o64, k64 = o.astype(np.float64), k.astype(np.float64)
    mag_o, mag_k = np.zeros(n), np.zeros(n)
    for g in gs[1:]:
        bg = banded_f32(g)
        launch_dots(lib, bo, bk, bg, n, dots, ws)
        assert lib.gad_wf_update(bo.ptr, bk.ptr, dots.ptr, N, n, _stream()) == 0, lib.gad_last_error()
        g64 = g.astype(np.float64)
        tmp, kg = float(o64 @ g64), float(k64 @ g64)
        ck, co = kg / (N + tmp), tmp / (N + tmp)
        mag_k = np.maximum(mag_k, np.abs(k64) + np.abs(ck * o64))
        mag_o = np.maximum(mag_o, np.abs(o64) + np.abs(co * o64))
        k64, o64 = k64 - ck * o64, o64 - co * o64
        assert bg.intact()
    o3, k3 = bo.view(torch.float32).cpu().numpy().astype(np.float64), bk.view(torch.float32).cpu().numpy().astype(np.float64)
    rk, ro = np.max(np.abs(k3 - k64) / (3 * 2.0 ** -22 * mag_k)), np.max(np.abs(o3 - o64) / (3 * 2.0 ** -22 * mag_o))
    print(f"n={n}: three iterations, max error / (3 x one-step bound): k {rk:.3f}, o {ro:.3f}; |k3 - k0| / |k0| = "
          f"{np.linalg.norm(k64 - k.astype(np.float64)) / np.linalg.norm(k):.3f}")
    assert rk <= 1.0 and ro <= 1.0
    assert np.linalg.norm(k64 - k.astype(np.float64)) > 1e-3 * np.linalg.norm(k)       # the recursion moved k
    assert all(b.intact() for b in (bo, bk, dots, ws))


# ---- 7 ----
TINY = dict(block_out_channels=[32, 32, 64, 64], norm_num_groups=8)


def test_influence_unlearner_against_the_oracle_in_double():
    """gad.InfluenceUnlearner on the TINY U-Net against influence_ref over the oracle model cast to double, on shared explicit
    batches (16 removed + 24 remaining images in batches of 8; counts 2 and 3 as for five labels).  With F and R the two
    weighted gradient sums of the reference side:  |dw_gpu - dw_ref| / (|F| + |R|) <= 2e-3  - the project's bound for parameter
    gradients against the oracle; dw is a combination of those gradients with coefficients that are ratios
    of their dot products, and the denominator is the scale of the terms that are subtracted, so the cancellation in F - R is not
    charged to the kernels.  Then apply(): forward and forward + backward agree with the oracle carrying the same perturbed weights
    (output 1e-4, parameter gradients < 2e-3 relative per tensor), which stale rotated / Winograd / bf16 shadows would fail."""
    import gad
    import influence_ref as IR
    from gad.training import flat_views
    from oracle import diffusers_ref as R
    from src.ddpm_config import DDPMConfig
    ucfg = dict(DDPMConfig.cifar100_config["unet_config"], **TINY)
    scfg = DDPMConfig.cifar100_config["scheduler_config"]
    torch.manual_seed(0)
    ref = R.UNet2DModel(**ucfg)
    net = gad.UNet2DModel(**ucfg)
    net.load_state_dict(ref.state_dict())
    net.to(dev)
    net.train()
    sch_r = R.DDPMScheduler(**scfg)
    g = torch.Generator().manual_seed(11)

    def batches(n_images):
        out = []
        for _ in range(n_images // 8):
            x, e = torch.rand(8, 3, 32, 32, generator=g) * 2 - 1, torch.randn(8, 3, 32, 32, generator=g)
            out.append((x, e, R.antithetic_timesteps(torch.randint(0, 1000, (5,), generator=g), 1000, 8)))
        return out
    removed, remaining = batches(16), batches(24)
    again = [remaining[i] for i in (2, 0, 1)]                      # a fresh shuffle of the remaining loader
    f, r = 2, 3

    def on_dev(bs):
        return [tuple(v.to(dev) for v in b) for b in bs]
    want, F, Rw = IR.delta_w(ref, sch_r, removed, remaining, again, f, r)

    u = gad.InfluenceUnlearner(net, gad.DDPMScheduler(**scfg))
    forget, retain = u.gradient_sum(on_dev(removed)), u.gradient_sum(on_dev(remaining))
    retain.mul_(f / ((f + r) * r))
    forget.div_(f + r)
    delta = u.woodfisher(on_dev(again), r, forget.sub_(retain))
    assert net.training                                            # eval inside, the caller's mode afterwards
    params = list(net.parameters())
    got = torch.cat([v.reshape(-1) for v in flat_views(params, delta)]).double().cpu()
    assert [tuple(p.shape) for p in params] == [tuple(p.shape) for p in ref.parameters()]
    err = float((got - want).norm() / (F.norm() + Rw.norm()))
    print(f"|dw_gpu - dw_ref| / (|F| + |R|) = {err:.3e}   (|dw_ref| = {want.norm():.3e}, |F| = {F.norm():.3e}, |R| = {Rw.norm():.3e}, "
          f"|dw_ref - (F - R)| / |F - R| = {(want - (F - Rw)).norm() / (F - Rw).norm():.3e})")
    assert err <= 2e-3
    covered = torch.zeros_like(delta, dtype=torch.bool)
    for _, off, n in u.flat._gad_params:
        covered[off:off + n] = True
    assert int((~covered).sum()) > 0 and bool((delta[~covered] == 0).all())       # the slot padding stays exactly zero

    # apply: a perturbation of 5 % of the weights' norm (from the reference side's numbers), large enough to move the output
    theta = torch.cat([p.detach().reshape(-1) for p in ref.parameters()]).double()
    ratio = float(0.05 * theta.norm() / want.norm())
    x, e, t = remaining[0]
    net.eval()
    with torch.no_grad():
        before = net(x.to(dev), t.to(dev)).sample.cpu()
    u.apply(delta, ratio)
    with torch.no_grad():
        for p, d in zip(ref.parameters(), flat_views(params, delta)):
            p.add_(ratio * d.cpu())
    ref.eval()
    with torch.no_grad():
        after = net(x.to(dev), t.to(dev)).sample.cpu()
        want_after = ref(x, t).sample
    moved, out_err = float((after - before).abs().max()), float((after - want_after).abs().max())
    print(f"ratio {ratio:.3e}: output moved by {moved:.3e}, max |gpu - oracle| after apply = {out_err:.3e}")
    assert moved > 1e-3 and out_err <= 1e-4
    gflat = u.step(x.to(dev), e.to(dev), t.to(dev))                 # forward + backward through the refreshed shadows
    torch.nn.functional.mse_loss(ref(sch_r.add_noise(x, e, t), t).sample, e).backward()
    worst = 0.0
    for (name, p), gv in zip(ref.named_parameters(), flat_views(params, gflat)):
        gg, gr = gv.detach().cpu().double().flatten(), p.grad.double().flatten()
        if name.endswith("to_k.bias"):                              # analytically zero: both sides hold rounding noise
            continue
        rel = float((gg - gr).norm() / gr.norm().clamp_min(1e-30))
        worst = max(worst, rel)
        assert rel < 2e-3, (name, rel)
    print(f"worst per-tensor relative gradient error after apply: {worst:.3e}")


# ---- 8 ----
def test_iu_entry_point_on_the_hip_backend(tmp_path, monkeypatch):
    """train 3 steps on toy2, then `--method iu --removal_dist shapley` twice with the same seeds: a finite FID, trained_steps =
    len(remaining loader), the preview named with iu_ratio, and a bit-identical flat parameter buffer after apply (no atomics
    anywhere in the path)."""
    import gad
    from src.ddpm_config import DDPMConfig
    cfg = {**DDPMConfig.cifar100_config}
    cfg["unet_config"] = dict(cfg["unet_config"], **TINY)
    cfg["n_samples"] = 4
    cfg["batch_size"] = 16
    for k in ("training_steps", "ckpt_freq", "sample_freq"):
        cfg[k] = dict(cfg[k], retrain=3)
    monkeypatch.setattr(DDPMConfig, "cifar100_config", cfg)
    from unconditional_generation import main as train_main
    from unconditional_generation import unlearn as unlearn_main
    out, db = str(tmp_path / "res"), str(tmp_path / "db.jsonl")
    assert train_main.main(train_main.parse_args(["--dataset", "toy2", "--method", "retrain", "--outdir", out, "--batch_size", "16",
                                                  "--num_inference_steps", "10", "--log_freq", "1"]))
    mdir = os.path.join(out, "toy2", "retrain", "models", "full")
    ck = torch.load(os.path.join(mdir, "ckpt_steps_00000003.pt"), weights_only=False)
    pdir = os.path.join(out, "toy2", "pruned", "models", "pruner=magnitude_pruning_ratio=0.3_threshold=0.05")
    os.makedirs(pdir)
    torch.save({"unet": ck["unet"], "unet_config": ck["unet_config"]}, os.path.join(pdir, "ckpt_steps_00000000.pt"))
    kept = []
    apply = gad.InfluenceUnlearner.apply

    def recording_apply(self, delta, ratio):
        start = self.flat.detach().clone()
        apply(self, delta, ratio)
        kept.append((start, self.flat.detach().clone()))
    monkeypatch.setattr(gad.InfluenceUnlearner, "apply", recording_apply)
    argv = ["--dataset", "toy2", "--method", "iu", "--removal_dist", "shapley", "--removal_seed", "1", "--load", mdir, "--outdir", out,
            "--db", db, "--iu_ratio", "0.5", "--n_samples", "16", "--batch_size", "8", "--num_inference_steps", "10"]
    assert unlearn_main.main(unlearn_main.parse_args(argv + ["--model_behavior", "global"]))
    assert unlearn_main.main(unlearn_main.parse_args(argv))          # the same seeds again; the behaviour is not needed twice
    row = json.loads(open(db).readline())
    steps = (len(row["remaining_idx"]) + 15) // 16
    assert np.isfinite(row["fid_value"]) and len(row["remaining_idx"]) == 64 and row["trained_steps"] == steps == 4
    assert row["method"] == "iu" and row["total_steps_time"] > 0
    assert os.path.exists(os.path.join(out, "toy2", "iu", "samples", "shapley", "shapley_seed=1",
                                       f"prutirb_ratio_0.5_steps_{steps:0>8}.png"))
    (s1, a1), (s2, a2) = kept
    assert torch.equal(s1, s2) and torch.equal(a1, a2)
    assert bool(torch.isfinite(a1).all()) and not torch.equal(a1, s1)                # apply moved the weights
