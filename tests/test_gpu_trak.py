"""GPU tests of the TRAK / D-TRAK features: gad_jl_project against the numpy generator and an fp64 oracle, its
determinism, a Johnson-Lindenstrauss check at the CIFAR U-Net's size, the engine's features against torch autograd
per-sample gradients of the oracle model, and the kept entry points end to end."""
import os

import numpy as np
import pytest
import torch

from jl_ref import jl_project, jl_rows

pytestmark = pytest.mark.gpu
dev = torch.device("cuda:0")
TINY = dict(block_out_channels=[32, 32, 64, 64], norm_num_groups=8)
P_ODD, LDA = 1237, 1240          # P is not a multiple of any tile (4-row loads, 16-row steps, 256-row slabs)


def _rows(G, seed=0):
    """[G][LDA] device rows, NaN past P (the kernel must not read them into the product)"""
    g = torch.Generator().manual_seed(seed)
    a = torch.full((G, LDA), float("nan"))
    a[:, :P_ODD] = torch.randn(G, P_ODD, generator=g)
    return a.to(dev)


def _project(a, P, d, seed=5, model_id=0, proj_type="normal", p0=0, out=None, accumulate=False):
    from gad.trak import project_raw
    out = torch.zeros(a.shape[0], d, device=dev) if out is None else out
    project_raw(a, out, P, seed, model_id, proj_type, p0, accumulate)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("proj_type", ["normal", "rademacher"])
def test_one_hot_rows_return_rows_of_r(proj_type):
    G, P, d = 8, 300, 256
    p0 = (1 << 33) + 12345                                          # the row's high word is part of the counter
    picks = np.array([0, 1, 17, 63, 64, 150, 298, 299])
    a = torch.zeros(G, P)
    a[np.arange(G), picks] = 1.0
    got = _project(a.to(dev), P, d, seed=77, model_id=3, proj_type=proj_type, p0=p0).cpu().numpy().astype(np.float64)
    want = jl_rows(p0 + picks, d, 77, 3, proj_type)
    if proj_type == "rademacher":
        assert np.array_equal(got, want)
    else:
        assert np.all(np.abs(got - want) <= 1e-6 * (1 + np.abs(want))), np.abs(got - want).max()


_ORACLE_R = {}


@pytest.mark.parametrize("proj_type", ["normal", "rademacher"])
@pytest.mark.parametrize("d", [64, 1024])
@pytest.mark.parametrize("G", [1, 3, 8, 64])
def test_projection_matches_fp64_oracle(G, d, proj_type):
    key = (d, proj_type)
    if key not in _ORACLE_R:
        _ORACLE_R[key] = jl_rows(np.arange(P_ODD), d, 5, 0, proj_type)
    a = _rows(G, seed=G)
    got = _project(a, P_ODD, d, proj_type=proj_type).cpu().numpy().astype(np.float64)
    want = a[:, :P_ODD].cpu().numpy().astype(np.float64) @ _ORACLE_R[key]
    rel = np.linalg.norm(got - want, axis=1) / np.linalg.norm(want, axis=1)
    assert rel.max() <= 1e-5, rel


@pytest.mark.parametrize("proj_type", ["normal", "rademacher"])
def test_determinism_and_chunking(proj_type):
    d = 1024
    a = _rows(8, seed=11)
    full = _project(a, P_ODD, d, proj_type=proj_type)
    assert torch.equal(full, _project(a, P_ODD, d, proj_type=proj_type))             # repeated launches
    for g in (0, 3, 7):                                                               # a row alone == the row in a batch
        assert torch.equal(full[g:g + 1], _project(a[g:g + 1], P_ODD, d, proj_type=proj_type))
    # p0 chunks with accumulate (600 columns keep the second chunk 16-B aligned)
    part = _project(a[:, :600], 600, d, proj_type=proj_type)
    part = _project(a[:, 600:], P_ODD - 600, d, proj_type=proj_type, p0=600, out=part, accumulate=True)
    rel = ((part - full).norm(dim=1) / full.norm(dim=1)).max().item()
    assert rel <= 1e-5, rel
    # another seed / model_id: uncorrelated features
    f = full.flatten().cpu().double()
    for kw in (dict(seed=6), dict(model_id=1)):
        o = _project(a, P_ODD, d, proj_type=proj_type, **kw).flatten().cpu().double()
        c = torch.corrcoef(torch.stack([f, o]))[0, 1].item()
        assert abs(c) < 0.05, (kw, c)


def test_jl_inner_products_at_cifar_unet_size():
    """P = 35.75 M (the CIFAR U-Net), d = 1024: <Rx, Ry> / d estimates <x, y> with standard deviation
    sqrt((|x|^2 |y|^2 + <x, y>^2) / d) for unit-variance R."""
    P, d = 35_750_000, 1024
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(P, device=dev, generator=g)
    z = torch.randn(P, device=dev, generator=g)
    a = torch.stack([x, 0.6 * x + 0.8 * z, z, -x]) / P ** 0.5
    for proj_type in ("normal", "rademacher"):
        phi = _project(a, P, d, proj_type=proj_type).double()
        est = (phi @ phi.T) / d
        ip = (a.double() @ a.double().T)
        n2 = torch.diagonal(ip)
        sd = ((n2[:, None] * n2[None, :] + ip ** 2) / d).sqrt()
        assert ((est - ip).abs() <= 5 * sd).all(), ((est - ip) / sd)
        assert torch.isfinite(phi).all()


def _oracle_features(ref, net, scfg, images, behaviour, timesteps, opt_seed):
    """torch autograd per-sample gradients of the oracle model, laid out like the engine's flat gradient buffer"""
    from gad.coalition import seed_everything
    from gad.training import flat_views
    from oracle import diffusers_ref as R
    sch = R.DDPMScheduler(**scfg)
    ref_params = dict(ref.named_parameters())
    names = [n for n, _ in net.named_parameters()]
    P = net.flat[1].numel()
    rows = []
    image = images.to(dev)
    noises = []
    for t in timesteps:
        seed_everything(opt_seed * 1000 + t)
        noises.append(torch.randn_like(image).cpu())
    noise = torch.stack(noises, dim=1)
    for i in range(images.shape[0]):
        ref.zero_grad()
        k = len(timesteps)
        x = images[i:i + 1].expand(k, *images.shape[1:])
        ts = torch.tensor(list(timesteps))
        pred = ref(sch.add_noise(x, noise[i], ts), ts).sample
        target = noise[i] if behaviour == "loss" else torch.zeros_like(pred)
        torch.nn.functional.mse_loss(pred, target).backward()
        flat = torch.zeros(P)
        for v, n in zip(flat_views([p for _, p in net.named_parameters()], flat), names):
            v.copy_(ref_params[n].grad)
        rows.append(flat.numpy().astype(np.float64))
    return np.stack(rows)


def test_engine_features_match_autograd_per_sample_gradients():
    import gad
    from gad.trak import Projector, gradient_features
    from oracle import diffusers_ref as R
    from src.ddpm_config import DDPMConfig
    ucfg = dict(DDPMConfig.cifar100_config["unet_config"], **TINY)
    scfg = DDPMConfig.cifar100_config["scheduler_config"]
    torch.manual_seed(0)
    ref = R.UNet2DModel(**ucfg)
    net = gad.UNet2DModel(**ucfg)
    net.load_state_dict(ref.state_dict())
    net.to(dev)
    _, gflat = net.flatten_parameters()
    images = torch.rand(3, 3, 32, 32, generator=torch.Generator().manual_seed(2)) * 2 - 1
    timesteps, d = [0, 250, 500, 750], 64
    proj = Projector(grad_dim=gflat.numel(), proj_dim=d, seed=42, proj_type="normal", device=dev, max_batch_size=2)
    got, grads = {}, []
    for behaviour in ("loss", "mean-squared-l2-norm"):
        got[behaviour] = gradient_features(net, gad.DDPMScheduler(**scfg), images, behaviour, timesteps, proj, opt_seed=42)
        grads.append(_oracle_features(ref, net, scfg, images, behaviour, timesteps, 42))
    want = jl_project(np.concatenate(grads), d, 42)
    for i, behaviour in enumerate(("loss", "mean-squared-l2-norm")):
        w = want[3 * i:3 * i + 3]
        rel = np.linalg.norm(got[behaviour].numpy() - w, axis=1) / np.linalg.norm(w, axis=1)
        assert rel.max() <= 1e-4, (behaviour, rel)


def test_entry_points_end_to_end(tmp_path, monkeypatch):
    from PIL import Image
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
    sdir = tmp_path / "samples"
    sdir.mkdir()
    rng = np.random.default_rng(0)
    for i in range(3):
        Image.fromarray(rng.integers(0, 256, (32, 32, 3), dtype=np.uint8)).save(sdir / f"{i}.png")
    flags = ["--method", "retrain", "--dataset", "cifar2", "--model_behavior", "mean-squared-l2-norm", "--t_strategy",
             "uniform", "--k_partition", "3", "--projector_dim", "64", "--outdir", str(tmp_path)]

    def run(extra=()):
        a = D.parse_args(flags + list(extra))
        a.unet_overrides = TINY
        return D.main(a)

    path = run()
    assert path == str(tmp_path / "cifar2" / "d_trak" / "full" / "train_f=mean-squared-l2-norm_t=uniform_k=3_d=64")
    assert os.path.getsize(path) == 6 * 64 * 4
    first = np.fromfile(path, dtype=np.float32).reshape(6, 64).copy()
    assert np.isfinite(first).all() and (np.abs(first).sum(1) > 0).all()
    run()
    assert np.array_equal(first, np.fromfile(path, dtype=np.float32).reshape(6, 64))         # rerun: bit-identical
    vpath = run(["--sample_dir", str(sdir)])
    assert vpath == str(sdir / "d_trak" / "reference_f=mean-squared-l2-norm_t=uniform_k=3_d=64")
    assert os.path.getsize(vpath) == 3 * 64 * 4

    from types import SimpleNamespace
    args = SimpleNamespace(dataset="cifar2", sample_dir=str(sdir), gradient_type="d_trak", k_partition=3, projector_dim=64,
                           sample_size=None, model_behavior_key="fid", by_class=False, by="mean")
    scores = compute_gradient_scores(args)
    assert scores.shape == (3, 6) and np.isfinite(scores).all()
