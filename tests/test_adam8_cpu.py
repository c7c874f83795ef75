"""8-bit blockwise Adam without a GPU: the code maps, the C structs, the host-side refusals of the launch, the block table, the
entry points' plumbing of --use_8bit_optimizer, and the restatement (tests/adam8_ref.py) against itself in fp32 and fp64."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import adam8_backend as AB
import adam8_ref as R
from gad import _capi
from gad.training import ADAM8_BLOCK, ADAM8_MIN_SIZE, SLOT, FusedTrainer, adam8_blocks
from unconditional_generation import main as train_main
from unconditional_generation import unlearn as unlearn_main


def _lib_map(signed):
    buf = (ctypes.c_float * 256)()
    assert _capi.load().gad_adam8_qmap(int(signed), buf) == 0
    return torch.tensor(list(buf), dtype=torch.float32)


def test_qmap_equals_the_closed_form_bit_for_bit():
    for signed, want in zip((True, False), R.qmaps(torch.float32)):
        got = _lib_map(signed)
        assert got.dtype == want.dtype and got.shape == (256,)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))
        assert (got[1:] > got[:-1]).all()                                    # 256 distinct values, ascending
        assert got[-1].item() == 1.0 and got[127 if signed else 0].item() == 0.0
        assert (got == 0).sum() == 1
    s, u = _lib_map(True), _lib_map(False)
    assert torch.equal(s[:127], -s[128:255].flip(0)) and abs(s[0].item() + 0.9929688) < 1e-6 and s.min() > -1
    assert (u >= 0).all()
    # the closed form read literally: midpoints of torch.linspace(0.1, 1, n + 1), times 10^(i-6)
    pos = torch.cat([(lambda e: (e[1:] + e[:-1]) / 2)(torch.linspace(0.1, 1, 2 ** i + 1, dtype=torch.float64)) * 10.0 ** (i - 6)
                     for i in range(7)])
    assert torch.allclose(s[128:255].double(), pos, rtol=2e-7, atol=0)
    upos = torch.cat([(lambda e: (e[1:] + e[:-1]) / 2)(torch.linspace(0.1, 1, 2 ** (i + 1) + 1, dtype=torch.float64)) * 10.0 ** (i - 6)
                      for i in range(7)])
    assert torch.allclose(u[1:255].double(), upos, rtol=2e-7, atol=0)
    assert _capi.load().gad_adam8_qmap(1, None) != 0 and b"null" in _capi.load().gad_last_error()


def test_adam8_struct_layout_matches_header(tmp_path):
    """sizeof / offsetof of gad_adam8_args and gad_adam8_block as gcc lays out include/gad.h against the ctypes mirrors (the
    method of test_capi_cpu.py::test_struct_layout_matches_header), and the numpy record adam8_blocks fills"""
    structs = {"gad_adam8_args": _capi.Adam8Args, "gad_adam8_block": _capi.Adam8Block}
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "gad.h"', 'int main(void) {']
    for cname, cls in structs.items():
        src.append(f'  printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in cls._fields_:
            src.append(f'  printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    src += ['  return 0;', '}']
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "layout"
    inc = os.path.join(os.path.dirname(__file__), "..", "include")
    subprocess.run(["gcc", "-I", inc, str(c), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for cname, cls in structs.items():
        assert int(got[cname]) == ctypes.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(cls, fname).offset, f"{cname}.{fname}"
    dt = adam8_blocks([torch.empty(8)], 0.0).table.dtype
    assert dt.itemsize == ctypes.sizeof(_capi.Adam8Block)
    for fname, _ in _capi.Adam8Block._fields_:
        assert dt.fields[fname][1] == getattr(_capi.Adam8Block, fname).offset, fname


def test_launch_refuses_bad_arguments_on_the_host():
    lib = _capi.load()
    a = _capi.Adam8Args()
    assert lib.gad_clip_adam8_ema(ctypes.byref(a), None) != 0 and b"null" in lib.gad_last_error()
    assert lib.gad_clip_adam8_ema(None, None) != 0 and b"null" in lib.gad_last_error()
    ptrs = ("p", "g", "ema", "state1", "state2", "absmax1", "absmax2", "m32", "v32", "blocks")

    def good():
        a = _capi.Adam8Args()
        for i, f in enumerate(ptrs):
            setattr(a, f, (i + 1) << 20)
        a.n, a.n32, a.n_absmax, a.n_blocks, a.step = 4096, 8, 2, 2, 1
        a.lr, a.beta1, a.beta2, a.eps = 1e-3, 0.9, 0.999, 1e-8
        return a
    for f in ptrs:
        if f == "ema":
            continue                                                         # optional
        a = good()
        setattr(a, f, None)
        assert lib.gad_clip_adam8_ema(ctypes.byref(a), None) != 0 and b"null" in lib.gad_last_error(), f
    for f in ("p", "g", "ema", "state1", "state2", "m32", "v32"):
        a = good()
        setattr(a, f, getattr(a, f) + 4)
        assert lib.gad_clip_adam8_ema(ctypes.byref(a), None) != 0 and b"aligned" in lib.gad_last_error(), f
    a = good()
    a.step = 0
    assert lib.gad_clip_adam8_ema(ctypes.byref(a), None) != 0 and b"step" in lib.gad_last_error()
    a = good()
    a.n_blocks = 0
    assert lib.gad_clip_adam8_ema(ctypes.byref(a), None) != 0 and b"empty" in lib.gad_last_error()


def test_block_table():
    sizes = (8, 4095, 4096, 4097, 3 * 2048 + 777)
    names = ["a.bias", "b.weight", "c.weight", "norm.bias", "e.weight"]
    params = [torch.empty(n) for n in sizes]
    lay = adam8_blocks(params, 1e-6, no_decay=["bias" in n for n in names])
    t = lay.table
    assert ADAM8_BLOCK == 2048 and ADAM8_MIN_SIZE == 4096 and R.BLOCK == 2048 and R.MIN_SIZE == 4096 and R.SLOT == SLOT
    slot = lambda n: (n + SLOT - 1) // SLOT * SLOT      # noqa: E731
    starts = np.cumsum([0] + [slot(n) for n in sizes])
    per = [t[(t["offset"] >= starts[i]) & (t["offset"] < starts[i + 1])] for i in range(len(sizes))]
    assert sum(len(x) for x in per) == len(t)
    assert [bool(x["fp32"].all()) for x in per] == [True, True, False, False, False]
    assert [bool(x["fp32"].any()) for x in per] == [True, True, False, False, False]
    assert [x["len"].tolist() for x in per[2:]] == [[2048, 2048], [2048, 2048, 1], [2048, 2048, 2048, 777]]
    assert [int(x["len"].sum()) for x in per] == list(sizes)
    for i, x in enumerate(per):
        assert x["offset"][0] == starts[i] and starts[i] % SLOT == 0
        assert (x["offset"] % SLOT == 0).all()
        assert (np.diff(x["offset"]) == x["len"][:-1]).all()                 # back to back inside the parameter
        assert x["offset"][-1] + x["len"][-1] == starts[i] + sizes[i]        # ... and never into the padding
        assert (x["len"] >= 1).all() and (x["len"] <= 2048).all()
        assert np.allclose(x["weight_decay"], 0.0 if "bias" in names[i] else 1e-6)
    assert lay.n_absmax == 2 + 3 + 4 and t["state"][t["fp32"] == 0].tolist() == list(range(9))
    small = t[t["fp32"] == 1]
    assert small["state"].tolist() == [0, 8, 8 + 2048] and lay.n32 == 8 + 4096 and (small["state"] % 4 == 0).all()
    assert [(s, n) for s, _, n, _, _ in lay.params] == [(True, 8), (True, 4095), (False, 4096), (False, 4097), (False, 6921)]
    assert (adam8_blocks(params, 1e-6).table["weight_decay"] > 0).all()      # no mask: everything decays
    with pytest.raises(ValueError):
        adam8_blocks(params, 1e-6, no_decay=[True])
    # conv weights count by numel whatever their shape; blocks run over the storage order
    lay4 = adam8_blocks([torch.empty(64, 32, 3, 3)], 0.0)
    assert lay4.table["len"].tolist() == [2048] * 9 and lay4.n_absmax == 9


def test_trainer_keywords():
    ps = [torch.nn.Parameter(torch.randn(5000)), torch.nn.Parameter(torch.randn(16))]
    with pytest.raises(ValueError, match="groups"):
        FusedTrainer(None, None, None, params=ps, groups=[(slice(0, 5000), 1.0)], optim_bits=8)
    with pytest.raises(ValueError, match="optim_bits"):
        FusedTrainer(None, None, None, params=ps, optim_bits=4)
    tr = FusedTrainer(None, None, None, params=ps, optim_bits=8, weight_decay=1e-2, no_decay=[False, True])
    s = tr.state8
    assert tr.m is None and tr.v is None
    assert s["state1"].dtype == torch.uint8 and (s["state1"] == 127).all() and (s["state2"] == 0).all()
    assert s["state1"].numel() == tr.flat.numel() == 5000 + 16
    assert (s["absmax1"] == 0).all() and (s["absmax2"] == 0).all() and s["absmax1"].numel() == 3 and s["m32"].numel() == 16
    assert tr._blocks8.numel() == 4 * ctypes.sizeof(_capi.Adam8Block)
    sd = tr.state_dict()
    assert sd["state"] == {} and sd["param_groups"][0]["optim_bits"] == 8
    tr.step_count = 3
    s["state1"][:5000] = torch.arange(5000) % 256
    s["absmax1"][:] = torch.tensor([1.0, 2.0, 3.0])
    s["m32"][:16] = torch.arange(16.0)
    sd = tr.state_dict()
    assert set(sd["state"][0]) == {"state1", "state2", "absmax1", "absmax2", "qmap1", "qmap2", "step"}
    assert set(sd["state"][1]) == {"state1", "state2", "step"}
    assert sd["state"][0]["state1"].dtype == torch.uint8 and sd["state"][0]["state1"].shape == (5000,)
    assert sd["state"][1]["state1"].dtype == torch.float32 and torch.equal(sd["state"][0]["qmap1"], _lib_map(True))
    tr2 = FusedTrainer(None, None, None, params=[torch.nn.Parameter(torch.randn(5000)), torch.nn.Parameter(torch.randn(16))], optim_bits=8)
    tr2.load_state_dict(sd)
    assert tr2.step_count == 3 and all(torch.equal(tr2.state8[k], s[k]) for k in s)
    fp32 = FusedTrainer(None, None, None, params=[torch.nn.Parameter(torch.randn(5000)), torch.nn.Parameter(torch.randn(16))])
    fp32.step_count = 3
    with pytest.raises(ValueError, match="8-bit"):
        tr2.load_state_dict(fp32.state_dict())                               # exp_avg / exp_avg_sq: not this trainer's state
    wrong = {"state": {0: dict(sd["state"][0], state1=sd["state"][0]["state1"].float()), 1: sd["state"][1]}, "param_groups": sd["param_groups"]}
    with pytest.raises(ValueError, match="torch.float32"):
        tr2.load_state_dict(wrong)


# ---- entry points ----------------------------------------------------------------------------------------------------
TINY = dict(block_out_channels=[32, 32, 64, 64], norm_num_groups=8)


def _registry(monkeypatch, **opt_kwargs):
    from src.ddpm_config import DDPMConfig
    cfg = {**DDPMConfig.cifar100_config}
    cfg["unet_config"] = dict(cfg["unet_config"], **TINY)
    cfg["optimizer_config"] = {"class_name": cfg["optimizer_config"]["class_name"],
                               "kwargs": dict(cfg["optimizer_config"]["kwargs"], **opt_kwargs)}
    monkeypatch.setattr(DDPMConfig, "cifar100_config", cfg)
    return cfg


def _main_args(tmp_path, *extra):
    return train_main.parse_args(["--dataset", "toy2", "--method", "retrain", "--outdir", str(tmp_path / "train"), "--db",
                                  str(tmp_path / "db.jsonl"), "--batch_size", "8", "--device", "cpu", *extra])


def _unlearn_args(tmp_path, cfg, *extra):
    out = tmp_path / "results"
    torch.manual_seed(0)
    m = AB.UNet2DModel(**cfg["unet_config"])
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    pdir = out / "toy2" / "pruned" / "models" / "pruner=magnitude_pruning_ratio=0.3_threshold=0.05"
    mdir = out / "toy2" / "retrain" / "models" / "full"
    os.makedirs(pdir, exist_ok=True)
    os.makedirs(mdir, exist_ok=True)
    torch.save({"unet": sd, "unet_config": dict(cfg["unet_config"])}, pdir / "ckpt_steps_00000000.pt")
    torch.save({"unet": sd, "unet_ema": AB.EMAModel(m.parameters()).state_dict()}, mdir / "ckpt_steps_00000002.pt")
    return unlearn_main.parse_args(["--dataset", "toy2", "--method", "gd", "--removal_dist", "shapley", "--removal_seed", "0", "--load",
                                    str(mdir), "--outdir", str(out), "--db", str(tmp_path / "db.jsonl"), "--gd_steps", "1",
                                    "--device", "cpu", *extra])


def test_toy2_registry_has_no_decay_key_so_the_flag_raises_keyerror(tmp_path, monkeypatch):
    """toy2 runs on the cifar100 config, whose optimizer kwargs carry no weight_decay: with --use_8bit_optimizer both entry
    points raise KeyError('weight_decay'), as the reference does (main.py:574, unlearn.py:459)."""
    cfg = _registry(monkeypatch)
    assert "weight_decay" not in cfg["optimizer_config"]["kwargs"]           # what the registry implies
    AB.CALLS.clear()
    with pytest.raises(KeyError, match="weight_decay"):
        train_main.main(_main_args(tmp_path, "--use_8bit_optimizer"), backend=AB)
    with pytest.raises(KeyError, match="weight_decay"):
        unlearn_main.main(_unlearn_args(tmp_path, cfg, "--use_8bit_optimizer"), backend=AB)
    assert AB.CALLS == []


def test_entry_points_hand_the_flag_to_the_trainer(tmp_path, monkeypatch):
    cfg = _registry(monkeypatch, weight_decay=1e-6)
    for run, args in ((train_main.main, _main_args(tmp_path, "--use_8bit_optimizer")),
                      (unlearn_main.main, _unlearn_args(tmp_path, cfg, "--use_8bit_optimizer"))):
        AB.CALLS.clear()
        with pytest.raises(AB.Reached):
            run(args, backend=AB)
        (kw,) = AB.CALLS
        assert kw["optim_bits"] == 8 and kw["weight_decay"] == 1e-6 and kw["lr"] == 1e-4 and "adamw" not in kw
        assert kw["no_decay"] == ["bias" in n for n in kw["names"]] and any(kw["no_decay"]) and not all(kw["no_decay"])
    # without the flag a backend is never handed the new keywords
    for run, args in ((train_main.main, _main_args(tmp_path)), (unlearn_main.main, _unlearn_args(tmp_path, cfg))):
        AB.CALLS.clear()
        with pytest.raises(AB.Reached):
            run(args, backend=AB)
        (kw,) = AB.CALLS
        assert "optim_bits" not in kw and "no_decay" not in kw and kw["weight_decay"] == 1e-6
    with pytest.raises(NotImplementedError, match="gradient_accumulation_steps"):
        train_main.main(_main_args(tmp_path, "--use_8bit_optimizer", "--gradient_accumulation_steps", "2"), backend=AB)


def test_sd_lora_entry_point_knows_the_flag():
    from text_to_image import train_text_to_image_lora as T
    assert T.parse_args(["--train_data_dir", "x", "--use_8bit_adam"]).use_8bit_adam is True
    assert T.parse_args(["--train_data_dir", "x"]).use_8bit_adam is False


# ---- the restatement against itself ------------------------------------------------------------------------------------
def test_nearest_code_is_the_first_argmin():
    g = torch.Generator().manual_seed(0)
    for qmap in R.qmaps(torch.float64):
        lo = float(qmap[0])
        x = torch.cat([torch.rand(4000, generator=g, dtype=torch.float64) * (1 - lo) + lo, qmap, (qmap[1:] + qmap[:-1]) / 2,
                       torch.randn(2000, generator=g, dtype=torch.float64) * 1e-6, torch.tensor([-1.0, 1.0, 0.0])]).clamp_(-1 if lo < 0 else 0, 1)
        want = (x[:, None] - qmap[None, :]).abs().argmin(1)                  # torch: the first of several minima
        assert torch.equal(R.nearest_code(qmap, x), want)


def test_fp32_restatement_keeps_the_cap_against_fp64():
    """Six teacher-forced steps on the GPU test's inputs: the restatement in fp32 against itself in fp64, each fp64 step starting
    from the state the fp32 run holds.  At most 0.1 % of the codes differ and none by more than one level - the cap the GPU
    test sets for the kernel is one fp32 arithmetic keeps."""
    sizes, p0, grads = R.make_case()
    hp = dict(R.CASE_HP)
    lay = adam8_blocks([torch.empty(n) for n in sizes], hp.pop("weight_decay"), no_decay=R.CASE_NO_DECAY)
    st = R.case_state(lay, sizes, p0)
    clipped, saw126, saw_underflow = [], False, False
    for t, gs in enumerate(grads, 1):
        g = R.flat_grad(lay, st["p"].numel(), gs)
        ss = float(g.double().square().sum())
        clipped.append(ss > 1.0)
        lo = R.adam8_step(st, g, lay.table, sumsq=ss, step=t, dtype=torch.float32, **hp)
        hi = R.adam8_step(st, g, lay.table, sumsq=ss, step=t, dtype=torch.float64, **hp)
        for k in ("state1", "state2"):
            R.codes_agree(lo[k], hi[k], f"step {t} {k}")
        for k in ("p", "ema", "absmax1", "absmax2", "m32", "v32"):
            # fp32 moments: beta1 m + (1-beta1) g cancels where m and g differ in sign, so an element's error is a few ulps of
            # the LARGER term, not of the result: absolute, at 1e-6 of the buffer's largest moment
            atol = {"p": 1e-6, "ema": 1e-6, "m32": 1e-6 * float(hi["m32"].abs().max()), "v32": 1e-6 * float(hi["v32"].abs().max())}.get(k, 0.0)
            assert torch.allclose(lo[k].double(), hi[k], rtol=1e-6, atol=atol), (t, k)
            assert torch.isfinite(hi[k]).all()
        # what the case is built to exercise
        (_, off5, n5, first5, nb5), (_, off6, n6, first6, nb6) = lay.params[5], lay.params[6]
        assert (hi["state1"][off5:off5 + n5] == 127).all() and (hi["state2"][off5:off5 + n5] == 0).all()
        assert (hi["absmax1"][first5:first5 + nb5] == 0).all() and (hi["absmax2"][first5:first5 + nb5] == 0).all()
        saw126 |= bool((hi["state1"][lay.params[2][1]:lay.params[2][1] + 4096] == 126).any())
        saw_underflow |= bool(((hi["state2"][off6:off6 + n6] == 0) & (g[off6:off6 + n6] != 0)).any())
        st = {k: (v.to(torch.float32) if v.dtype == torch.float64 else v) for k, v in lo.items()}
    assert any(clipped) and not all(clipped) and saw126 and saw_underflow
    # padding and the code bytes under fp32-state parameters were never written
    for (small, off, cnt, _, _) in lay.params:
        pad = slice(off + cnt, off + (cnt + SLOT - 1) // SLOT * SLOT)
        assert (st["p"][pad] == 0).all() and (st["state1"][pad] == 127).all() and (st["state2"][pad] == 0).all()
        if small:
            assert (st["state1"][off:off + cnt] == 127).all() and (st["state2"][off:off + cnt] == 0).all()
