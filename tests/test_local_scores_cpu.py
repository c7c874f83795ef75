"""CPU checks of the local model behaviours: the three C entry points (declared, exported, bound, host-side refusals without a
GPU) and the two entry points' plumbing - `unlearn.py --model_behavior local` and `calculate_local_scores.py` - driven by the
CPU oracle backend with tests/local_ref.py::local_behaviors_loop as its `local_model_behaviors`."""
import json
import os
import re
import types

import numpy as np
import pytest
import torch

import oracle_backend as OB
from gad import _capi
from local_ref import local_behaviors_loop

P = 1 << 20                               # placeholder address: the refusals below happen before anything is launched
NEW = ("gad_image_metrics", "gad_add_noise_bcast", "gad_mse_segments")


def _err(lib):
    return lib.gad_last_error().decode()


def test_new_symbols_are_declared_exported_and_bound():
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "gad.h")).read()
    lib = _capi.load()
    for n in NEW + ("gad_image_metrics_workspace_bytes", "gad_mse_segments_workspace_bytes"):
        assert re.search(rf"\b{n}\s*\(", hdr), n
        assert n in _capi.SIGNATURES and hasattr(lib, n), n
    from gad import ops
    assert all(hasattr(ops, f) for f in ("image_metrics_raw", "add_noise_bcast_raw", "mse_segments_raw"))


def test_image_metrics_host_refusals():
    lib = _capi.load()
    need = lib.gad_image_metrics_workspace_bytes(4, 32, 32, 3, 7)
    assert need > 0 and lib.gad_image_metrics_workspace_bytes(8, 32, 32, 3, 7) == 2 * need
    assert lib.gad_image_metrics_workspace_bytes(1, 256, 256, 1, 7) > lib.gad_image_metrics_workspace_bytes(1, 64, 64, 1, 7)

    def call(a=P, b=2 * P, out=3 * P, N=4, H=32, W=32, C=3, win=7, ws=4 * P, ws_bytes=need):
        return lib.gad_image_metrics(a, b, out, N, H, W, C, win, 1.0, 0.01, 0.03, ws, ws_bytes, None)
    for null in ("a", "b", "out", "ws"):
        assert call(**{null: None}) != 0 and "null" in _err(lib), null
    assert call(H=6) != 0 and "H < win" in _err(lib)
    assert call(W=5) != 0 and "win" in _err(lib)
    assert lib.gad_image_metrics_workspace_bytes(4, 6, 32, 3, 7) == -1 and "H < win" in _err(lib)
    assert call(win=8) != 0 and "odd" in _err(lib)
    assert call(ws_bytes=need - 8) != 0 and "workspace_bytes" in _err(lib)
    assert call(out=3 * P + 4) != 0 and "aligned" in _err(lib)
    assert call(N=0) != 0


def test_add_noise_bcast_host_refusals():
    lib = _capi.load()

    def call(x0=P, eps=2 * P, t=3 * P, ac=4 * P, xt=5 * P, R=60, rpi=30, T=10, C=3, HW=1024, n_train=1000):
        return lib.gad_add_noise_bcast(x0, eps, t, ac, xt, R, rpi, T, C, HW, n_train, None)
    for null in ("x0", "eps", "t", "ac", "xt"):
        assert call(**{null: None}) != 0 and "null" in _err(lib), null
    assert call(R=65, rpi=65) != 0 and "R % T != 0" in _err(lib)
    assert call(rpi=15) != 0 and "rows_per_image" in _err(lib)            # not whole draws
    assert call(rpi=40) != 0 and "rows_per_image" in _err(lib)            # does not divide R
    assert call(HW=0) != 0 and call(C=0) != 0 and call(T=0) != 0


def test_mse_segments_host_refusals():
    lib = _capi.load()
    need = lib.gad_mse_segments_workspace_bytes(700, 7, 3, 1024)
    assert need > 0 and lib.gad_mse_segments_workspace_bytes(0, 7, 3, 1024) == -1

    def call(pred=P, eps=2 * P, out=3 * P, R=700, rps=7, C=3, HW=1024, ws=4 * P, ws_bytes=need):
        return lib.gad_mse_segments(pred, eps, out, R, rps, C, HW, ws, ws_bytes, None)
    for null in ("pred", "eps", "out", "ws"):
        assert call(**{null: None}) != 0 and "null" in _err(lib), null
    assert call(rps=9) != 0 and "R % rows_per_segment != 0" in _err(lib)
    assert call(ws_bytes=need - 1) != 0 and "workspace_bytes" in _err(lib)
    assert call(ws=4 * P + 4) != 0 and "aligned" in _err(lib)


def test_engine_has_no_cpu_path():
    import gad
    ucfg = dict(block_out_channels=(32, 32), down_block_types=("DownBlock2D", "DownBlock2D"),
                up_block_types=("UpBlock2D", "UpBlock2D"), layers_per_block=1, attention_head_dim=None, sample_size=8)
    pipe = gad.DDPMPipeline(gad.UNet2DModel(**ucfg), gad.DDIMScheduler())
    with pytest.raises(_capi.GadError):
        gad.local_model_behaviors(pipe, pipe, 1, 1, 2)


# ---- entry points on the CPU oracle ----
TINY = dict(block_out_channels=[32, 32, 64, 64], norm_num_groups=8)
VALUE = re.compile(r"^-?\d\.\d{8}e[+-]\d\d$")
LOCAL = ("mse", "nrmse", "ssim", "diffusion_loss")
AVG = {"mse": "avg_mse", "nrmse": "avg_nrmse", "ssim": "avg_ssim", "diffusion_loss": "avg_total_loss"}


@pytest.fixture()
def tiny_registry(monkeypatch):
    from src.ddpm_config import DDPMConfig
    cfg = {**DDPMConfig.cifar100_config}
    cfg["unet_config"] = dict(cfg["unet_config"], **TINY)
    cfg["n_samples"] = 4
    cfg["training_steps"] = dict(cfg["training_steps"], retrain=2)
    cfg["sample_freq"] = dict(cfg["sample_freq"], retrain=2)
    cfg["ckpt_freq"] = dict(cfg["ckpt_freq"], retrain=1)
    monkeypatch.setattr(DDPMConfig, "cifar100_config", cfg)
    return cfg


def loop_backend():
    """tests/oracle_backend.py plus the reference-shaped loop as its local_model_behaviors"""
    ns = types.SimpleNamespace(**{k: getattr(OB, k) for k in dir(OB) if not k.startswith("_")})
    ns.local_model_behaviors = local_behaviors_loop
    return ns


def check_local_row(row, n_samples):
    for s in range(n_samples):
        for k in LOCAL:
            v = row[f"generated_image_{s}_{k}"]
            assert isinstance(v, str) and VALUE.match(v), (s, k, v)
    assert f"generated_image_{n_samples}_mse" not in row
    for k in LOCAL:
        assert isinstance(row[AVG[k]], str) and VALUE.match(row[AVG[k]]), k
        mean = float(np.mean([float(row[f"generated_image_{s}_{k}"]) for s in range(n_samples)]))
        assert abs(float(row[AVG[k]]) - mean) <= 1e-7 * abs(mean) + 1e-300, k


@pytest.mark.timeout(900)
def test_local_entry_points_on_the_cpu_oracle(tmp_path, tiny_registry):
    from unconditional_generation import calculate_local_scores as local_main
    from unconditional_generation import main as train_main
    from unconditional_generation import unlearn as unlearn_main
    BE = loop_backend()
    out, db = str(tmp_path / "results"), str(tmp_path / "db.jsonl")
    n, common = 3, ["--n_samples", "3", "--n_noises", "2", "--num_inference_steps", "5", "--device", "cpu"]
    # the full model, and one retrained on a Shapley coalition
    train = ["--dataset", "toy2", "--method", "retrain", "--outdir", out, "--db", str(tmp_path / "train.jsonl"),
             "--batch_size", "8", "--num_inference_steps", "5", "--device", "cpu", "--log_freq", "1"]
    assert train_main.main(train_main.parse_args(train), backend=OB)
    assert train_main.main(train_main.parse_args(train + ["--removal_dist", "shapley", "--removal_seed", "1"]), backend=OB)
    mdir = os.path.join(out, "toy2", "retrain", "models", "full")
    ck = torch.load(os.path.join(mdir, "ckpt_steps_00000002.pt"), weights_only=False)
    pdir = os.path.join(out, "toy2", "pruned", "models", "pruner=magnitude_pruning_ratio=0.3_threshold=0.05")
    os.makedirs(pdir)
    torch.save({"unet": ck["unet"], "unet_config": ck["unet_config"]}, os.path.join(pdir, "ckpt_steps_00000000.pt"))

    # ---- unlearn.py: global row as before, local row with the new keys ----
    sft = ["--dataset", "toy2", "--method", "gd", "--removal_dist", "shapley", "--removal_seed", "1", "--load", mdir,
           "--outdir", out, "--db", db, "--gd_steps", "2", "--batch_size", "4", "--exp_name", "e"]
    g = unlearn_main.parse_args(sft + ["--model_behavior", "global", "--n_samples", "8", "--num_inference_steps", "5",
                                       "--device", "cpu"])
    assert unlearn_main.main(g, backend=BE)
    u = unlearn_main.parse_args(sft + ["--model_behavior", "local"] + common)
    assert unlearn_main.main(u, backend=BE)
    grow, lrow = [json.loads(l) for l in open(db)]
    need = {"dataset", "method", "removal_dist", "removal_seed", "exp_name", "gd_steps", "remaining_idx", "removed_idx",
            "fid_value", "total_steps_time", "total_sampling_time", "trained_steps", "device", "opt_seed"}
    assert need <= set(grow) and np.isfinite(grow["fid_value"])
    assert not any(k.startswith("generated_image_") or k.startswith("avg_") for k in grow)
    assert (need - {"fid_value"}) <= set(lrow) and "fid_value" not in lrow
    check_local_row(lrow, n)
    assert lrow["remaining_idx"] == grow["remaining_idx"] and lrow["removed_idx"] == grow["removed_idx"]
    assert len(lrow["remaining_idx"]) == 64 and len(lrow["removed_idx"]) == 64
    assert lrow["trained_steps"] == 2 and lrow["method"] == "gd" and lrow["model_behavior"] == "local"
    assert float(lrow["avg_mse"]) > 0 and float(lrow["avg_ssim"]) < 1        # two fine-tuning steps moved the model
    sdir = os.path.join(out, "toy2", "gd", "samples", "shapley", "shapley_seed=1")
    from PIL import Image
    for s in range(n):
        assert Image.open(os.path.join(sdir, f"generated_image_{s}.png")).size == (32, 32)

    # ---- calculate_local_scores.py on the checkpoints the training runs left ----
    db2 = str(tmp_path / "local.jsonl")
    base = ["--dataset", "toy2", "--method", "retrain", "--full_model_dir", mdir, "--outdir", out, "--db", db2] + common
    assert local_main.main(local_main.parse_args(base + ["--exp_name", "same"]), backend=BE)            # removal dir defaults to "full"
    assert local_main.main(local_main.parse_args(base + ["--removal_dist", "shapley", "--removal_seed", "1",
                                                         "--exp_name", "shapley1"]), backend=BE)
    same, shap = [json.loads(l) for l in open(db2)]
    check_local_row(same, n)
    check_local_row(shap, n)
    assert same["removal_model_dir"] == mdir and len(same["remaining_idx"]) == 128 and same["removed_idx"] == []
    for s in range(n):                                                   # identical models: identical images
        assert float(same[f"generated_image_{s}_mse"]) == 0.0 and float(same[f"generated_image_{s}_nrmse"]) == 0.0
        assert float(same[f"generated_image_{s}_ssim"]) == 1.0
        assert float(same[f"generated_image_{s}_diffusion_loss"]) > 0
    rdir = os.path.join(out, "toy2", "retrain", "models", "shapley", "shapley_seed=1")
    assert shap["removal_model_dir"] == rdir
    rck = torch.load(os.path.join(rdir, "ckpt_steps_00000002.pt"), weights_only=False)
    assert shap["remaining_idx"] == rck["remaining_idx"].tolist() and shap["removed_idx"] == rck["removed_idx"].tolist()
    assert shap["remaining_idx"] == lrow["remaining_idx"]                # the same coalition as the sFT run above
    assert float(shap["avg_mse"]) > 0
    # the loss is computed on the full model's image, which does not depend on the removal model: same seeds, same x0
    gdir = os.path.join(out, "toy2", "local_scores", "generated_samples")
    for s in range(n):
        a = np.asarray(Image.open(os.path.join(gdir, f"generated_image_{s}.png")))
        b = np.asarray(Image.open(os.path.join(sdir, f"generated_image_{s}.png")))
        assert a.shape == (32, 32, 3) and np.array_equal(a, b)
    # --use_ema takes the EMA weights and its own sample directory
    assert local_main.main(local_main.parse_args(base + ["--use_ema", "--exp_name", "ema"]), backend=BE)
    ema = [json.loads(l) for l in open(db2)][-1]
    check_local_row(ema, n)
    assert ema["use_ema"] is True and os.path.exists(os.path.join(out, "toy2", "local_scores", "ema_generated_samples",
                                                                  "generated_image_0.png"))


def test_local_scores_removal_directory_grammar():
    from unconditional_generation import calculate_local_scores as L
    mk = lambda *a: L.parse_args(["--full_model_dir", "x", "--db", "y", "--method", "retrain", *a])      # noqa: E731
    assert L.removal_directory(mk()) == "full"
    assert L.removal_directory(mk("--excluded_class", "3")) == "excluded_3"
    assert L.removal_directory(mk("--removal_dist", "datamodel", "--datamodel_alpha", "0.25", "--removal_seed", "7")) == \
        "datamodel/datamodel_alpha=0.25_seed=7"
    assert L.removal_directory(mk("--removal_dist", "shapley", "--removal_seed", "3")) == "shapley/shapley_seed=3"
    a = mk()
    assert (a.n_samples, a.n_noises, a.num_inference_steps, a.use_ema, a.device) == (100, 50, 100, False, "cuda:0")
    with pytest.raises(SystemExit):
        L.parse_args(["--db", "y"])                                      # --full_model_dir is required
