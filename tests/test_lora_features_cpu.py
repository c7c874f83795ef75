"""CPU checks of the SD LoRA gradient features: the C ABI of the segmented token-axis contraction (exported, declared, bound,
struct layout, refusals before any HIP call), text_to_image/traks.py against an fp64 numpy restatement of its formulas, and the
flags / defaults / output paths of text_to_image/grad_text_to_image_lora.py."""
import ctypes
import hashlib
import os
import re
import subprocess

import numpy as np
import pandas as pd
import pytest
import torch

INC = os.path.join(os.path.dirname(__file__), "..", "include")


def _layout(tmp_path, cname, fields):
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "gad.h"', 'int main(void) {',
           f'  printf("size %zu\\n", sizeof({cname}));']
    src += [f'  printf("{f} %zu\\n", offsetof({cname}, {f}));' for f in fields]
    src += ['  return 0;', '}']
    c = tmp_path / f"{cname}.c"
    c.write_text("\n".join(src))
    exe = tmp_path / cname
    subprocess.run(["gcc", "-I", INC, str(c), "-o", str(exe)], check=True)
    return {k: int(v) for k, v in (line.split() for line in
                                   subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())}


def test_seg_entry_points_exported_declared_bound(tmp_path):
    from gad import _capi
    lib = _capi.load()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(INC, "gad.h")).read(), flags=re.S)
    for name in ("gad_hgemm_tn_seg", "gad_hgemm_tn_seg_workspace_bytes"):
        assert hasattr(lib, name) and name in _capi.SIGNATURES
        assert re.search(rf"\b{name}\s*\(\s*const gad_hgemm_seg_args\s*\*", hdr), name
    cls = _capi.HGemmSegArgs
    got = _layout(tmp_path, "gad_hgemm_seg_args", [f for f, _ in cls._fields_])
    assert got["size"] == ctypes.sizeof(cls)
    for f, _ in cls._fields_:
        assert got[f] == getattr(cls, f).offset, f
    assert cls.c_seg_stride.size == 8                            # segment outputs are ~200 MB apart


def test_hgemm_args_layout_is_what_it_was(tmp_path):
    """gad_hgemm_args is untouched by the new entry points: the parent commit's size and field offsets, byte for byte"""
    from gad import _capi
    cls = _capi.HGemmArgs
    got = _layout(tmp_path, "gad_hgemm_args", [f for f, _ in cls._fields_])
    desc = ";".join(f"{f}@{got[f]}" for f, _ in cls._fields_) + f";size={got['size']}"
    assert got["size"] == ctypes.sizeof(cls) == 200
    assert hashlib.sha256(desc.encode()).hexdigest() == PARENT_HGEMM_LAYOUT, desc


PARENT_HGEMM_LAYOUT = "04d6c36186e273e7905210568537d27da8f1bfe207c995421720360eb9f7f271"


def _seg(**kw):
    from gad import _capi
    a = _capi.HGemmSegArgs()
    base = dict(A=4096, B=8192, C=16384, ws=1 << 20, ws_bytes=1 << 40, M=320, N=256, L=1000, S=16, lda=320, ldb=256, ldc=256,
                c_seg_stride=50_000_000, alpha=1.0, accumulate=0, splitk_hint=0)
    base.update(kw)
    for k, v in base.items():
        setattr(a, k, v)
    return a


def test_seg_workspace_query_depends_on_the_segment_not_on_the_batch():
    from gad import _capi
    lib = _capi.load()
    q = lambda **kw: lib.gad_hgemm_tn_seg_workspace_bytes(ctypes.byref(_seg(**kw)))  # noqa: E731
    one = q(S=1)
    assert one == 4 * 320 * 256 * 4                              # L = 1000: 16 K steps in 4 slices of at least 256 rows
    assert q(S=16) == 16 * one and q(S=64) == 64 * one           # the plan is a function of (M, N, L)
    assert q(L=16) == 0 and q(L=77) == 0 and q(L=256) == 0       # short segments are not split
    assert q(L=4096) == 16 * one                                 # never more than 4 slices
    assert q(L=300, splitk_hint=3) == 16 * 3 * 320 * 256 * 4


@pytest.mark.parametrize("bad, word", [
    (dict(A=0), b"null"), (dict(B=0), b"null"), (dict(C=0), b"null"),
    (dict(S=0), b"S = 0"), (dict(S=-2), b"S = -2"),
    (dict(L=0), b"L = 0"), (dict(L=-5), b"L = -5"),
    (dict(S=60000, L=60000), b"int32 row index"),
    (dict(c_seg_stride=319 * 256 + 255), b"overlap"),
    (dict(ldc=260, c_seg_stride=320 * 256), b"overlap"),
    (dict(lda=324), b"misaligned row strides"), (dict(ldb=250), b"misaligned row strides"), (dict(lda=312), b"misaligned row strides"),
    (dict(A=4100), b"16-byte aligned"),
    (dict(ldc=200), b"ldc < N"),
    (dict(ws_bytes=1000), b"workspace too small"), (dict(ws=0), b"workspace too small"),
])
def test_seg_refusals_name_the_cause_without_a_gpu(bad, word):
    from gad import _capi
    lib = _capi.load()
    assert lib.gad_hgemm_tn_seg(ctypes.byref(_seg(**bad)), None) != 0
    assert word in lib.gad_last_error(), lib.gad_last_error()
    if b"workspace" not in word:                                 # the size query refuses the same arguments
        assert lib.gad_hgemm_tn_seg_workspace_bytes(ctypes.byref(_seg(**bad))) == -1


def test_seg_stride_at_its_minimum_passes_the_checks():
    from gad import _capi
    lib = _capi.load()
    assert lib.gad_hgemm_tn_seg_workspace_bytes(ctypes.byref(_seg(c_seg_stride=319 * 256 + 256))) > 0
    assert lib.gad_hgemm_tn_seg_workspace_bytes(ctypes.byref(_seg(M=37, N=21, lda=40, ldb=24, ldc=24, L=77, c_seg_stride=36 * 24 + 21))) == 0


# ---------------------------------------------------------------------------------------------------------------
# traks.py
# ---------------------------------------------------------------------------------------------------------------
def _fp64_scores(train, train_d, gen, gen_d, journey, lam):
    """the formulas of the reference's traks.py:131-188 in fp64 numpy"""
    out = {}
    sim = gen @ train.T / (np.linalg.norm(gen, axis=1, keepdims=True) @ np.linalg.norm(train, axis=1, keepdims=True).T)
    out["grad_sim"] = sim.mean(0)
    d = train.shape[1]
    x = np.linalg.inv(train.T @ train + lam * np.eye(d)) @ train.T
    infl = gen @ x
    out["trak"] = infl.mean(0)
    out["relative_influence"] = (infl / np.linalg.norm(x, axis=0)).mean(0)
    out["renorm_influence"] = (infl / np.linalg.norm(train, axis=1)).mean(0)
    out["journey_trak"] = (journey @ x).mean(0)
    xd = np.linalg.inv(train_d.T @ train_d + lam * np.eye(d)) @ train_d.T
    out["dtrak"] = (gen_d @ xd).mean(0)
    return out


def test_traks_matches_fp64_restatement(tmp_path):
    """train 40 x 64, generated 6 x 64, journey 12 x 64, 5 groups of uneven size, lam = 0.5: every saved array within 2e-4 of its
    largest absolute value of the fp64 formulas (the reference's fp32 torch.inverse is 2.6e-5 / 2.9e-5 off on that scale for trak /
    relative_influence; an element-wise relative bar would not hold on near-zero scores); rank files = stable argsort"""
    from text_to_image import traks
    g = torch.Generator().manual_seed(0)
    d, k = 64, 7
    feats = {n: torch.randn(r, d, generator=g) for n, r in (("train", 40), ("train_d", 40), ("gen", 6), ("gen_d", 6), ("journey", 12))}
    root = tmp_path / "artbench_post_impressionism"
    for sub in ("train", "generated", "generated_journey"):
        (root / "gradients" / sub).mkdir(parents=True)
    suffix = f"num_timesteps={k}_proj_dim={d}.pt"
    torch.save(feats["train"], root / "gradients" / "train" / f"emb_f=loss_{suffix}")
    torch.save(feats["train_d"], root / "gradients" / "train" / f"emb_f=mean-squared-l2-norm_{suffix}")
    torch.save(feats["gen"], root / "gradients" / "generated" / f"emb_f=loss_{suffix}")
    torch.save(feats["gen_d"], root / "gradients" / "generated" / f"emb_f=mean-squared-l2-norm_{suffix}")
    torch.save(feats["journey"], root / "gradients" / "generated_journey" / f"emb_f=loss_num_journey_points=4_num_journey_noises=1_proj_dim={d}.pt")
    sizes = [13, 3, 9, 1, 14]
    artists = [f"artist_{i}" for i, n in enumerate(sizes) for _ in range(n)]
    order = np.random.default_rng(1).permutation(40)
    artists = [artists[i] for i in order]
    pd.DataFrame({"index": range(40), "artist": artists, "filename": [f"img_{i}.jpg" for i in range(40)]}).to_csv(
        root / "gradients" / "train" / "group.csv", index=False)
    data = tmp_path / "data"
    data.mkdir()
    pd.DataFrame({"artist": [f"artist_{i}" for i in range(5)]}).to_csv(data / "post_impressionism_artists.csv", index=False)
    args = traks.parse_args(["--output_dir", str(root), "--num_timesteps", str(k), "--proj_dim", str(d), "--lam", "0.5",
                             "--num_journey_points", "4", "--train_data_dir", str(data), "--device", "cpu"])
    assert (args.group, args.cls, args.dataset) == ("artist", "post_impressionism", "artbench")
    assert traks.parse_args(["--output_dir", "/o"]).lam == 0.5 and traks.parse_args(["--output_dir", "/o"]).proj_dim == 32768
    out_dir = traks.main(args)
    assert out_dir == str(root / "baselines")

    want = _fp64_scores(*(feats[n].double().numpy() for n in ("train", "train_d", "gen", "gen_d", "journey")), 0.5)
    idx = [np.where(np.array(artists) == f"artist_{i}")[0] for i in range(5)]
    assert sorted(len(i) for i in idx) == sorted(sizes)
    expect = {"avg_grad_sim": [want["grad_sim"][i].mean() for i in idx], "max_grad_sim": [want["grad_sim"][i].max() for i in idx]}
    for m in ("trak", "relative_influence", "renorm_influence", "journey_trak", "dtrak"):
        expect[m] = [want[m][i].sum() for i in idx]
    assert sorted(os.listdir(out_dir)) == sorted([f"artist_{m}.npy" for m in expect] +
                                                 [f"all_generated_images_artist_rank_{m}.npy" for m in expect])
    for m, w in expect.items():
        got = np.load(os.path.join(out_dir, f"artist_{m}.npy"))
        w = np.asarray(w, dtype=np.float64).reshape(5, 1)
        assert got.shape == (5, 1)
        err = np.abs(got - w).max() / np.abs(w).max()
        print(f"{m}: max error / max |value| = {err:.2e}")
        assert err <= 2e-4, (m, err)
        rank = np.load(os.path.join(out_dir, f"all_generated_images_artist_rank_{m}.npy"))
        assert np.array_equal(rank, np.argsort(-got.mean(axis=-1), kind="stable"))


# ---------------------------------------------------------------------------------------------------------------
# grad_text_to_image_lora.py
# ---------------------------------------------------------------------------------------------------------------
def test_grad_text_to_image_lora_defaults_and_paths():
    from text_to_image import grad_text_to_image_lora as G
    a = G.parse_args(["--train_data_dir", "/d/artbench-10-imagefolder-split/train", "--output_dir", "/o", "--f", "loss",
                      "--lora_dir", "/l"])
    assert (a.source, a.seed, a.num_images, a.generation_seed, a.num_journey_points, a.num_journey_noises, a.resolution,
            a.train_batch_size, a.cls_key, a.cls, a.lora_steps, a.num_timesteps, a.proj_dim, a.pretrained_model_name_or_path,
            a.center_crop, a.random_flip, a.dataloader_num_workers) == \
        ("train", 42, 50, 42, 50, 1, 256, 16, "style", "post_impressionism", None, 100, 32768, "lambdalabs/miniSD-diffusers",
         False, False, 0)
    assert G.dataset_name(a) == "artbench_post_impressionism"
    assert G.output_directory(a) == "/o/artbench_post_impressionism/gradients/train"
    assert G.output_filename(a) == "emb_f=loss_num_timesteps=100_proj_dim=32768.pt"
    assert G.lora_weight_name(a) == "pytorch_lora_weights.safetensors"
    a = G.parse_args(["--train_data_dir", "/d/artbench", "--output_dir", "/o", "--f", "mean-squared-l2-norm", "--source", "generated",
                      "--num_timesteps", "10", "--proj_dim", "4096", "--lora_steps", "200"])
    assert G.output_directory(a) == "/o/artbench_post_impressionism/gradients/generated"
    assert G.output_filename(a) == "emb_f=mean-squared-l2-norm_num_timesteps=10_proj_dim=4096.pt"
    assert G.lora_weight_name(a) == "pytorch_lora_weights_200.safetensors"
    a = G.parse_args(["--train_data_dir", "/d/artbench", "--output_dir", "/o", "--f", "loss", "--source", "generated_journey",
                      "--num_journey_points", "25", "--num_journey_noises", "2"])
    assert G.output_directory(a) == "/o/artbench_post_impressionism/gradients/generated_journey"
    assert G.output_filename(a) == "emb_f=loss_num_journey_points=25_num_journey_noises=2_proj_dim=32768.pt"
    assert list(G.journey_points(100, 50)) == list(range(1, 100, 2)) and len(G.journey_points(100, 50)) == 50
    assert list(G.journey_points(10, 3)) == [1, 4, 7]
    with pytest.raises(SystemExit):
        G.parse_args(["--train_data_dir", "/d", "--output_dir", "/o"])                       # --f is required
    with pytest.raises(ValueError, match="training folder"):
        G.parse_args(["--f", "loss"])
    with pytest.raises(SystemExit):
        G.parse_args(["--train_data_dir", "/d", "--f", "loss", "--source", "validation"])
