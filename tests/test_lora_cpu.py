"""CPU checks of LoRA unlearning (`unlearn.py --method lora`): the numpy restatement of the dropout mask (tests/lora_ref.py),
`gad.get_peft_model` and the LoRA+ grouping, the header / ctypes agreement on the new struct and symbols with the host-side
refusals of the new entry points, and the entry point's plumbing on the CPU oracle backend (tests/lora_backend.py)."""
import ctypes
import json
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import lora_backend
import lora_ref as LR
from gad import _capi

SEED = 20240531                     # fixed: the statistics below were checked for this seed and hold for it
P = 1 << 20                         # placeholder address: the refusals happen before anything is launched
TINY = dict(block_out_channels=[32, 32, 64, 64], norm_num_groups=8)


# ---- 1: the mask restatement ----
def test_mask_is_a_deterministic_function_of_its_arguments():
    base = dict(seed=SEED, offset=3, layer=1, j=0)
    a = LR.keep_words(SEED, 3, 1, 0, np.arange(1000), 256)
    assert np.array_equal(a, LR.keep_words(SEED, 3, 1, 0, np.arange(1000), 256))
    assert a.shape == (1000, 256) and int(a.max()) < 2 ** 32
    # rows and channels are addressed, not enumerated: a window of the same rows / a narrower C gives the same words
    assert np.array_equal(a[500:510, :30], LR.keep_words(SEED, 3, 1, 0, np.arange(500, 510), 30))
    for other in (dict(base, j=1), dict(base, layer=2), dict(base, offset=4), dict(base, seed=SEED + 1)):
        b = LR.keep_words(other["seed"], other["offset"], other["layer"], other["j"], np.arange(1000), 256)
        assert float((a == b).mean()) < 1e-3, other          # independent 32-bit words collide with probability 2^-32
    # the row's high half is part of the counter
    assert not np.array_equal(LR.keep_words(SEED, 3, 1, 0, [5], 8), LR.keep_words(SEED, 3, 1, 0, [5 + (1 << 32)], 8))
    assert LR.keep_mask(SEED, 3, 1, 0, 64, 32, 0.0).all()    # p = 0 keeps everything
    assert LR.threshold(0.05) == 214748364 and LR.threshold(0.5) == 1 << 31


@pytest.mark.parametrize("p", [0.05, 0.5])
def test_dropped_fraction_is_within_six_sigma(p):
    keep = np.stack([LR.keep_mask(SEED, 1, 0, j, 1000, 256, p) for j in range(3)])
    n = keep.size
    dropped, sigma = 1.0 - keep.mean(), math.sqrt(n * p * (1 - p)) / n
    print(f"p={p}: dropped {dropped:.6f} over {n} elements, sigma {sigma:.2e}, |dropped - p| / sigma = {abs(dropped - p) / sigma:.2f}")
    assert abs(dropped - p) <= 6 * sigma
    per_j = 1.0 - keep.reshape(3, -1).mean(axis=1)
    assert np.all(np.abs(per_j - p) <= 6 * sigma * math.sqrt(3))


# ---- 2: get_peft_model and the LoRA+ groups ----
def tiny_gad_model():
    import gad
    from src.ddpm_config import DDPMConfig
    return gad.UNet2DModel(**dict(DDPMConfig.cifar100_config["unet_config"], **TINY))


def test_get_peft_model_freezes_the_base_and_follows_the_recipe():
    import gad
    from gad.nn import Attention
    from gad.training import SLOT
    torch.manual_seed(7)
    net = tiny_gad_model()
    base = {n: p.detach().clone() for n, p in net.named_parameters()}
    attns = [m for m in net.modules() if isinstance(m, Attention)]
    assert len(attns) >= 2
    torch.manual_seed(11)
    out = gad.get_peft_model(net, gad.LoraConfig(r=16, lora_alpha=32, lora_dropout=0.05, target_modules=["to_q", "to_v", "to_k"]))
    after = torch.rand(4)                                          # the generator's state after the call
    assert out is net
    # the recipe, replayed: per projection in module order two nn.Linear constructions, then kaiming_uniform_(A, a = sqrt 5)
    torch.manual_seed(11)
    want = []
    for m in attns:
        for name in ("to_q", "to_k", "to_v"):
            o, i = getattr(m, name).weight.shape
            a, b = torch.nn.Linear(i, 16, bias=False), torch.nn.Linear(16, o, bias=False)
            torch.nn.init.kaiming_uniform_(a.weight, a=math.sqrt(5))
            want.append(a.weight.detach().clone())
    assert torch.equal(after, torch.rand(4))                       # the same number of draws
    got = [a for m in attns for _, a, _ in m.lora_qkv.matrices()]
    assert len(got) == len(want) == 3 * len(attns)
    for g, w in zip(got, want):
        assert torch.equal(g.detach(), w) and float(g.abs().max()) <= 1 / math.sqrt(g.shape[1]) and g.shape[0] == 16
    trainable = [n for n, p in net.named_parameters() if p.requires_grad]
    assert trainable and all("lora_qkv" in n for n in trainable) and len(trainable) == 6 * len(attns)
    for n, p in net.named_parameters():
        if "lora_qkv" not in n:
            assert not p.requires_grad and torch.equal(p.detach(), base[n])
    for m in attns:
        lq = m.lora_qkv
        assert lq.scale == 2.0 and lq.p == 0.05 and [n for n, _, _ in lq.matrices()] == ["to_q", "to_k", "to_v"]
        for name, a, b in lq.matrices():
            assert not bool(b.detach().any()) and tuple(b.shape) == (getattr(m, name).weight.shape[0], 16)
    assert [m.lora_qkv.layer for m in attns] == list(range(len(attns)))
    # [all A | all B], multipliers 1 and 16, slices on slot boundaries that cover the buffer flatten_params would build
    params, groups = gad.lora_parameters(net, 16)
    n = len(got)
    assert all(p is g for p, g in zip(params[:n], got)) and all(not bool(p.detach().any()) for p in params[n:]) and len(params) == 2 * n
    (sa, ma), (sb, mb) = groups
    assert (ma, mb) == (1.0, 16.0) and sa.start == 0 and sa.stop == sb.start
    slot = lambda k: (k + SLOT - 1) // SLOT * SLOT             # noqa: E731
    assert sa.stop == sum(slot(p.numel()) for p in params[:n]) and sb.stop - sb.start == sum(slot(p.numel()) for p in params[n:])


def test_get_peft_model_refusals():
    import gad
    with pytest.raises(NotImplementedError, match="target_modules"):
        gad.get_peft_model(tiny_gad_model(), gad.LoraConfig(r=16, target_modules=["to_q", "to_out.0"]))
    with pytest.raises(_capi.GadError, match="multiple of 4"):
        gad.get_peft_model(tiny_gad_model(), gad.LoraConfig(r=6))
    with pytest.raises(_capi.GadError, match="lora_dropout"):
        gad.get_peft_model(tiny_gad_model(), gad.LoraConfig(r=8, lora_dropout=1.0))
    from gad.nn import Attention
    net = tiny_gad_model()
    attn = next(m for m in net.modules() if isinstance(m, Attention))
    attn.dim_head, attn.dpad = 23, 24                              # what a head-grouped-pruned CelebA block looks like
    with pytest.raises(NotImplementedError, match="head-grouped-pruned"):
        gad.get_peft_model(net, gad.LoraConfig(r=8))
    assert all(p.requires_grad for p in net.parameters())          # refused before anything was changed


def test_trainer_groups_are_checked_on_the_host():
    """the LoRA+ groups of FusedTrainer are runs of whole slots of the flat buffer; the constructor (host code) checks them"""
    from gad.training import FusedTrainer, SLOT

    def make(groups):
        params = [torch.nn.Parameter(torch.randn(4, 6)), torch.nn.Parameter(torch.zeros(5, 4))]      # 24 and 20 floats: slots of 24 each
        return FusedTrainer(None, None, None, params=params, groups=groups), params
    t, params = make([(slice(0, 24), 1.0), (slice(24, 48), 16.0)])
    assert t.groups == [(slice(0, 24), 1.0), (slice(24, 48), 16.0)] and t.flat.numel() == 48 and 24 % SLOT == 0
    assert params[1].data_ptr() == t.flat.data_ptr() + 4 * 24                       # the second group starts where B lives
    assert make(None)[0].groups is None
    for bad in ([(slice(0, 20), 1.0)], [(slice(4, 24), 1.0)], [(slice(0, 56), 1.0)], [(slice(24, 24), 1.0)], [(slice(0, 48, 2), 1.0)]):
        with pytest.raises(ValueError, match="whole slots"):
            make(bad)


# ---- 3: header and binding ----
NEW = ("gad_lora_down_dropout_workspace_bytes", "gad_lora_down_dropout_fwd", "gad_lora_down_dropout_bwd", "gad_lora_merge")


def test_lora_symbols_and_struct_layout(tmp_path):
    lib = _capi.load()
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "gad.h")).read()
    for n in NEW:
        assert n in hdr and n in _capi.SIGNATURES and hasattr(lib, n), n
    cls = _capi.LoraDropoutArgs
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "gad.h"', 'int main(void) {',
           '  printf("size %zu\\n", sizeof(gad_lora_dropout_args));']
    src += [f'  printf("{f} %zu\\n", offsetof(gad_lora_dropout_args, {f}));' for f, _ in cls._fields_]
    src += ['  return 0;', '}']
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    inc = os.path.join(os.path.dirname(__file__), "..", "include")
    subprocess.run(["gcc", "-I", inc, str(c), "-o", str(tmp_path / "layout")], check=True)
    got = dict(line.split() for line in subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(cls)
    for f, _ in cls._fields_:
        assert int(got[f]) == getattr(cls, f).offset, f


def good_args(**kw):
    a = _capi.LoraDropoutArgs()
    a.x, a.ldx, a.M, a.C, a.r, a.n_proj, a.dx, a.ld_dx = P, 256, 1000, 256, 16, 3, 2 * P, 256
    for j in range(4):
        a.A[j], a.mid[j], a.dmid[j], a.dA[j] = (3 + j) * P, (8 + j) * P, (13 + j) * P, (18 + j) * P
    a.p, a.scale, a.workspace, a.workspace_bytes = 0.05, 2.0, 30 * P, 1 << 40
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_lora_host_refusals_and_workspace_query():
    lib = _capi.load()
    err = lambda: lib.gad_last_error().decode()                    # noqa: E731
    fwd, bwd, q = lib.gad_lora_down_dropout_fwd, lib.gad_lora_down_dropout_bwd, lib.gad_lora_down_dropout_workspace_bytes
    for p in (-0.1, 1.0, 1.5, float("nan")):
        for f in (fwd, bwd):
            assert f(ctypes.byref(good_args(p=p)), None) != 0 and "outside [0, 1)" in err(), p
        assert q(ctypes.byref(good_args(p=p))) == -1
    for n in (0, 5, -1):
        assert fwd(ctypes.byref(good_args(n_proj=n)), None) != 0 and "n_proj" in err() and "1..4" in err()
        assert bwd(ctypes.byref(good_args(n_proj=n)), None) != 0 and "n_proj" in err()
    for r in (0, 2, 6, 68):
        assert fwd(ctypes.byref(good_args(r=r)), None) != 0 and "rank" in err()
    assert fwd(ctypes.byref(good_args(x=None)), None) != 0 and "null pointer" in err()
    assert bwd(ctypes.byref(good_args(dx=None)), None) != 0 and "null pointer" in err()
    assert bwd(ctypes.byref(good_args(workspace=None)), None) != 0 and "null pointer" in err()
    a = good_args()
    a.A[2] = None
    assert fwd(ctypes.byref(a), None) != 0 and "null pointer" in err() and "A[2]" in err()
    a = good_args()
    a.dmid[1] = None
    assert bwd(ctypes.byref(a), None) != 0 and "null pointer" in err()
    assert fwd(ctypes.byref(good_args(ldx=128)), None) != 0 and "ldx" in err()
    need = q(ctypes.byref(good_args()))
    assert bwd(ctypes.byref(good_args(workspace_bytes=need - 1)), None) != 0 and "short workspace" in err()
    # the dA partials: one [n_proj x 16][C] panel per row slab, at most 256 slabs, far below the bytes of x at training sizes
    assert need == 63 * 3 * 16 * 256 * 4                                          # M = 1000: 63 slabs of 16 rows
    big = q(ctypes.byref(good_args(M=32768)))
    assert big == 256 * 3 * 16 * 256 * 4 and big < 0.4 * 32768 * 256 * 4
    assert q(ctypes.byref(good_args(M=32768, r=20))) == 2 * big                  # ranks pad to whole 16-wide tiles
    assert q(ctypes.byref(good_args(M=1, n_proj=1, C=30, r=4))) == 16 * 30 * 4
    assert q(ctypes.byref(good_args(M=32768, p=0.0))) >= big                      # covers the plain forward launches too
    assert lib.gad_lora_merge(None, 8, P, P, 8, 8, 4, 1.0, None) != 0 and "null pointer" in err()
    assert lib.gad_lora_merge(P, 4, P, P, 8, 8, 4, 1.0, None) != 0 and "ldw" in err()


def test_lora_ops_have_no_cpu_path():
    from gad import ops
    with pytest.raises(_capi.GadError):
        ops.lora_down_dropout_fwd_raw(torch.zeros(4, 8), [torch.zeros(4, 8)], 0.05, 1.0, 1, 1, 0)


# ---- 4: the entry point on the oracle backend ----
@pytest.fixture()
def tiny_registry(monkeypatch):
    from src.ddpm_config import DDPMConfig
    cfg = {**DDPMConfig.cifar100_config}
    cfg["unet_config"] = dict(cfg["unet_config"], **TINY)
    cfg["n_samples"] = 4
    cfg["batch_size"] = 16
    monkeypatch.setattr(DDPMConfig, "cifar100_config", cfg)
    return cfg


def write_checkpoints(cfg, out):
    """what a training run and prune.py leave behind for unlearn.py (as tests/test_influence_cpu.py does)"""
    import oracle_backend as OB
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
    return mdir, {n: unet[n] for n, _ in model.named_parameters()}


def test_lora_entry_point_on_the_cpu_oracle(tmp_path, tiny_registry, monkeypatch):
    from unconditional_generation import unlearn
    out, db = str(tmp_path / "results"), str(tmp_path / "db.jsonl")
    mdir, unet = write_checkpoints(tiny_registry, out)
    base = ["--dataset", "toy2", "--method", "lora", "--load", mdir, "--outdir", out, "--db", db, "--gd_steps", "3", "--lora_rank", "8",
            "--lora_dropout", "0.25", "--removal_dist", "shapley", "--removal_seed", "1", "--model_behavior", "global", "--n_samples", "8",
            "--batch_size", "4", "--num_inference_steps", "3", "--device", "cpu"]
    BE = lora_backend.make()
    kept = {}
    store = BE.EMAModel.store

    def recording_store(self, parameters):                         # the shared tail's first call: shadows and model as the method left them
        parameters = list(parameters)
        kept["ema"], kept["params"] = self, [p.detach().clone() for p in parameters]
        kept["frozen"] = [p.requires_grad for p in parameters]
        store(self, parameters)
    monkeypatch.setattr(BE.EMAModel, "store", recording_store)
    assert unlearn.main(unlearn.parse_args(base), backend=BE)
    row = json.loads(open(db).readline())
    assert row["method"] == "lora" and row["lora_rank"] == 8 and row["lora_dropout"] == 0.25
    assert row["gd_steps"] == 3 and row["trained_steps"] == 3 and np.isfinite(row["fid_value"]) and row["total_steps_time"] > 0
    assert len(row["remaining_idx"]) == 64
    names = [e[0] for e in BE.log]
    assert names == ["get_peft_model", "lora_parameters", "FusedTrainer", "merge_and_unload"]
    assert BE.log[0][1:] == (8, 32, 0.25, ("to_q", "to_v", "to_k"))                # lora_alpha = 32 whatever the rank
    assert BE.log[1][2] == 16 and BE.log[2][2] == [BE.log[2][1], 16 * BE.log[2][1]]   # LoRA+: B at 16 x the registry's lr
    assert BE.log[3][1] > 0                                                         # the B matrices moved away from zero
    # the reference's EMA quirk: shadows = the merged weights, step counter advanced by gd_steps; the base apart from the merged
    # projections is untouched and no LoRA parameter is left on the model
    ema, params = kept["ema"], kept["params"]
    assert ema.optimization_step == 3 + 3 and len(params) == len(unet) == len(ema.shadow_params) and not any(kept["frozen"])
    moved = 0
    for (name, before), p, s in zip(unet.items(), params, ema.shadow_params):
        assert torch.equal(p, s), name
        if any(name.endswith(f"{n}.weight") for n in ("to_q", "to_k", "to_v")):
            moved += int(not torch.equal(p, before))
        else:
            assert torch.equal(p, before), name
    assert moved > 0
    assert os.path.exists(os.path.join(out, "toy2", "lora", "samples", "shapley", "shapley_seed=1", "prutirb_ratio_0.5_steps_00000003.png"))

    for extra, word in ((["--use_8bit_optimizer"], "use_8bit_optimizer"), (["--gradient_accumulation_steps", "2"], "gradient_accumulation_steps")):
        with pytest.raises(NotImplementedError, match=word):
            unlearn.main(unlearn.parse_args(base + extra), backend=lora_backend.make())
    argv = [a if a != "toy2" else "imagenette" for a in base]
    with pytest.raises(NotImplementedError, match="imagenette"):
        unlearn.main(unlearn.parse_args(argv), backend=lora_backend.make())
    no_load = [a for i, a in enumerate(base) if a != "--load" and base[i - 1] != "--load"]
    with pytest.raises(NotImplementedError, match="without --load"):       # there is no checkpoint to adapt
        unlearn.main(unlearn.parse_args(no_load), backend=lora_backend.make())
    for m in ("esd", "retrain", "prune_fine_tune"):
        with pytest.raises(NotImplementedError, match="LoRA unlearning"):
            unlearn.main(unlearn.parse_args(["--method", m, "--db", db]))
