"""CPU checks of influence unlearning (`unlearn.py --method iu`): the test-side fp64 restatement (tests/influence_ref.py)
against a golden the reference's own get_grad / woodfisher_diff produced (tests/golden/make_influence_golden.py), the entry
point's plumbing on the CPU oracle backend, and the host side of the three WoodFisher entry points."""
import json
import os
import re
import types

import numpy as np
import pytest
import torch

import influence_ref as IR
import oracle_backend as OB
from gad import _capi

P = 1 << 20                               # placeholder address: the refusals below happen before anything is launched
CAP = 2048 * 256 * 4                      # elements one sweep of the full grid covers


def _err(lib):
    return lib.gad_last_error().decode()


# ---- 1 / 2: the restatement reproduces what the reference's own functions computed ----
@pytest.fixture(scope="module")
def golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "influence.npz")))


def golden_batches(G, which, first_draw):
    """(image, noise, timesteps) batches of one loader pass, with the draws the reference made in that pass"""
    images, n_t = torch.from_numpy(G["images"]), IR.ToyScheduler().config.num_train_timesteps
    out = []
    for i, idx in enumerate(G[which]):
        half = torch.from_numpy(G["half_timesteps"][first_draw + i])
        t = torch.cat([half, n_t - half - 1])[:len(idx)]
        out.append((images[idx], torch.from_numpy(G["noise"][first_draw + i]), t))
    return out


def test_restatement_reproduces_the_reference_golden(golden):
    G = golden
    model = IR.ToyEps()
    model.load_state_dict({k[len("weight."):]: torch.from_numpy(v) for k, v in G.items() if k.startswith("weight.")})
    sch = IR.ToyScheduler()
    labels = G["labels"]
    n_rm, n_re = len(G["removed_batches"]), len(G["remaining_batches"])
    forget_count = IR.distinct_labels(labels[b] for b in G["removed_batches"])
    retain_count = IR.distinct_labels(labels[b] for b in G["remaining_batches"])
    assert (forget_count, retain_count) == (int(G["forget_count"]), int(G["retain_count"])) == (2, 3)    # labels, not 16 / 24 images
    delta, F, R = IR.delta_w(model, sch, golden_batches(G, "removed_batches", 0), golden_batches(G, "remaining_batches", n_rm),
                             golden_batches(G, "wf_batches", n_rm + n_re), forget_count, retain_count)

    def rel(a, b):
        b = torch.from_numpy(b).double()
        return float((a - b).norm() / b.norm())
    errs = dict(forget_grad=rel(F, G["forget_grad"]), retain_grad=rel(R, G["retain_grad"]), delta_w=rel(delta, G["delta_w"]))
    print("relative L2 against the reference's fp32 vectors:", errs)
    assert errs["delta_w"] <= 1e-5 and errs["forget_grad"] <= 1e-5 and errs["retain_grad"] <= 1e-5
    # the recursion is not a no-op on this input: k moved away from F - R
    assert float((delta - (F - R)).norm() / (F - R).norm()) > 1e-2


# ---- 3: the entry point on the oracle backend ----
TINY = dict(block_out_channels=[32, 32, 64, 64], norm_num_groups=8)
BATCH = 16


@pytest.fixture()
def tiny_registry(monkeypatch):
    from src.ddpm_config import DDPMConfig
    cfg = {**DDPMConfig.cifar100_config}
    cfg["unet_config"] = dict(cfg["unet_config"], **TINY)
    cfg["n_samples"] = 4
    cfg["batch_size"] = BATCH
    monkeypatch.setattr(DDPMConfig, "cifar100_config", cfg)
    return cfg


def iu_backend():
    """tests/oracle_backend.py plus an InfluenceUnlearner built on influence_ref; the instances are kept for the asserts"""
    ns = types.SimpleNamespace(**{k: getattr(OB, k) for k in dir(OB) if not k.startswith("_")})
    ns.made = []

    class Unlearner(IR.InfluenceUnlearner):
        def __init__(self, model, scheduler):
            super().__init__(model, scheduler)
            ns.made.append(self)

        def apply(self, delta, ratio):
            before = [p.detach().clone() for p in self.model.parameters()]
            super().apply(delta, ratio)
            self.moved = max(float((p.detach() - b).abs().max()) for p, b in zip(self.model.parameters(), before))
    ns.InfluenceUnlearner = Unlearner
    return ns


def write_checkpoints(cfg, out):
    """What a training run and prune.py leave behind for unlearn.py: the full model's checkpoint and the pruned architecture"""
    torch.manual_seed(0)
    ucfg = dict(cfg["unet_config"])
    model = OB.UNet2DModel(**ucfg)
    ema = OB.EMAModel(model.parameters())
    ema.optimization_step = 3
    mdir = os.path.join(out, "toy2", "retrain", "models", "full")
    pdir = os.path.join(out, "toy2", "pruned", "models", "pruner=magnitude_pruning_ratio=0.3_threshold=0.05")
    os.makedirs(mdir)
    os.makedirs(pdir)
    unet = {k: v.detach().clone() for k, v in model.state_dict().items()}
    torch.save({"unet": unet, "unet_config": ucfg, "unet_ema": ema.state_dict()}, os.path.join(mdir, "ckpt_steps_00000003.pt"))
    torch.save({"unet": unet, "unet_config": ucfg}, os.path.join(pdir, "ckpt_steps_00000000.pt"))
    return mdir


def test_iu_entry_point_on_the_cpu_oracle(tmp_path, tiny_registry):
    from unconditional_generation import unlearn
    out, db = str(tmp_path / "results"), str(tmp_path / "db.jsonl")
    mdir = write_checkpoints(tiny_registry, out)
    base = ["--dataset", "toy2", "--method", "iu", "--load", mdir, "--outdir", out, "--db", db, "--iu_ratio", "0.25",
            "--model_behavior", "global", "--n_samples", "8", "--batch_size", "4", "--num_inference_steps", "3", "--device", "cpu"]
    BE = iu_backend()
    assert unlearn.main(unlearn.parse_args(base + ["--removal_dist", "shapley", "--removal_seed", "1"]), backend=BE)
    row = json.loads(open(db).readline())
    assert row["method"] == "iu" and np.isfinite(row["fid_value"]) and row["total_steps_time"] > 0
    n_rem, n_rm = len(row["remaining_idx"]), len(row["removed_idx"])
    assert (n_rem, n_rm) == (64, 64)
    steps = (n_rem + BATCH - 1) // BATCH                               # len(remaining loader)
    assert row["trained_steps"] == steps == 4
    preview = os.path.join(out, "toy2", "iu", "samples", "shapley", "shapley_seed=1", f"prutirb_ratio_0.25_steps_{steps:0>8}.png")
    assert os.path.exists(preview)
    (u,) = BE.made
    # removed loader, remaining loader, then the remaining loader again for the recursion; toy2 has one label per half, so the
    # label counts are (1, 1) where the image counts would be (64, 64): N = retain_count = 1
    assert u.calls[:3] == [("gradient_sum", 4), ("gradient_sum", steps), ("woodfisher", steps, 1)]
    assert u.calls[3][:2] == ("apply", 0.25) and u.calls[3][2] > 0 and u.moved > 0
    ds_labels = torch.as_tensor([0] * 64 + [1] * 64)
    args = types.SimpleNamespace(removal_dist="shapley")
    assert unlearn.iu_counts(args, ds_labels[:64], ds_labels[64:]) == (1, 1)
    args.removal_dist = "loo"                                          # the deliberate deviation: every other rule counts images
    assert unlearn.iu_counts(args, ds_labels[:96], ds_labels[96:]) == (32, 96)

    # --removal_dist unset: nothing is removed -> no loader over nothing, forget_count = 0, a zero perturbation
    BE = iu_backend()
    assert unlearn.main(unlearn.parse_args(base), backend=BE)
    row = json.loads(open(db).readlines()[1])
    assert len(row["remaining_idx"]) == 128 and row["removed_idx"] == [] and row["trained_steps"] == 8
    (u,) = BE.made
    assert u.calls[:3] == [("gradient_sum", 0), ("gradient_sum", 8), ("woodfisher", 8, 128)]
    assert u.calls[3] == ("apply", 0.25, 0.0) and u.moved == 0.0       # the checkpointed weights are unchanged by apply


def test_other_methods_still_raise(tmp_path):
    from unconditional_generation import unlearn
    for m in ("esd", "lora", "retrain", "prune_fine_tune"):
        with pytest.raises(NotImplementedError, match="influence unlearning"):
            unlearn.main(unlearn.parse_args(["--method", m, "--db", str(tmp_path / "db.jsonl")]))


# ---- 4: the host side of the three entry points ----
NEW = ("gad_wf_dots_workspace_bytes", "gad_wf_dots", "gad_wf_update")


def test_wf_symbols_are_declared_exported_and_bound():
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "gad.h")).read()
    lib = _capi.load()
    for n in NEW:
        assert re.search(rf"\b{n}\s*\(", hdr), n
        assert n in _capi.SIGNATURES and hasattr(lib, n), n
    import gad
    assert hasattr(gad.ops, "wf_dots_raw") and hasattr(gad.ops, "wf_update_raw") and hasattr(gad, "InfluenceUnlearner")


def test_wf_workspace_query_is_monotone_and_saturates():
    lib = _capi.load()
    q = lib.gad_wf_dots_workspace_bytes
    assert q(0) == -1 and "positive" in _err(lib) and q(-5) == -1
    assert q(1) == q(3) == q(4) == q(1024) == 16                       # one workgroup: one fp64 pair
    assert q(1027) == 16 and q(1028) == 32 and q(262147) == 256 * 16   # whole float4 groups decide; the n % 4 tail rides along
    ns = sorted({1, 3, 4, 1023, 1024, 1025, 1027, 4096, 262147, CAP - 1024, CAP - 1, CAP, CAP + 1, CAP + 1027, 1 << 25, 35_750_000,
                 860_000_000, 1 << 40})
    sizes = [q(n) for n in ns]
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and all(s % 16 == 0 for s in sizes)
    assert all(q(n) == 2048 * 16 for n in ns if n >= CAP) and q(CAP - 1024) < 2048 * 16


def test_wf_host_refusals():
    lib = _capi.load()
    n = 1027
    need = lib.gad_wf_dots_workspace_bytes(n)

    def dots(o=P, k=2 * P, g=3 * P, n=n, d=4 * P, ws=5 * P, ws_bytes=need):
        return lib.gad_wf_dots(o, k, g, n, d, ws, ws_bytes, None)
    for null in ("o", "k", "g", "d", "ws"):
        assert dots(**{null: None}) != 0 and "null" in _err(lib), null
    for vec in ("o", "k", "g"):
        assert dots(**{vec: 6 * P + 4}) != 0 and "16-byte" in _err(lib), vec
    assert dots(d=4 * P + 4) != 0 and "8-byte" in _err(lib)
    assert dots(ws=5 * P + 4) != 0 and "8-byte" in _err(lib)
    assert dots(ws_bytes=need - 1) != 0 and "ws_bytes" in _err(lib)
    assert dots(n=0) != 0 and "positive" in _err(lib)

    def update(o=P, k=2 * P, d=4 * P, N=3.0, n=n):
        return lib.gad_wf_update(o, k, d, N, n, None)
    for null in ("o", "k", "d"):
        assert update(**{null: None}) != 0 and "null" in _err(lib), null
    for vec in ("o", "k"):
        assert update(**{vec: 6 * P + 8}) != 0 and "16-byte" in _err(lib), vec
    assert update(d=4 * P + 4) != 0 and "8-byte" in _err(lib)
    assert update(n=0) != 0 and "positive" in _err(lib)
    assert update(k=P) != 0 and "different" in _err(lib)


def test_influence_unlearner_has_no_cpu_path():
    import gad
    ucfg = dict(block_out_channels=(32, 32), down_block_types=("DownBlock2D", "DownBlock2D"),
                up_block_types=("UpBlock2D", "UpBlock2D"), layers_per_block=1, attention_head_dim=None, sample_size=8)
    net = gad.UNet2DModel(**ucfg)
    u = gad.InfluenceUnlearner(net, gad.DDPMScheduler())
    batch = (torch.zeros(2, 3, 8, 8), torch.zeros(2, 3, 8, 8), torch.tensor([1, 2]))
    with pytest.raises(_capi.GadError):
        u.gradient_sum([batch])
    assert net.training                                                # the mode is given back when a batch fails, too
