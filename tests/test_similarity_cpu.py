"""CPU checks of the similarity baselines: the two C entry points (declared, exported, bound, every host-side refusal without a
GPU, the workspace query), the host statements of gad/similarity.py on a canned matrix (values, dtypes, shapes, rank order
under ties, file names, what text_to_image/baseline_lds.py asks of the arrays) and the entry points' refusals."""
import os
import re

import numpy as np
import pytest
import torch

import similarity_ref as SR
from gad import _capi
from gad import similarity as S

P = 1 << 20                               # placeholder address: the refusals below happen before anything is launched
F32, U8 = _capi.SIM_X_F32, _capi.SIM_X_U8


def _err(lib):
    return lib.gad_last_error().decode()


def test_new_symbols_are_declared_exported_and_bound():
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "gad.h")).read()
    lib = _capi.load()
    for n in ("gad_cosine_rows", "gad_cosine_rows_workspace_bytes"):
        assert re.search(rf"\b{n}\s*\(", hdr), n
        assert n in _capi.SIGNATURES and hasattr(lib, n), n
    assert re.search(r"GAD_SIM_X_F32\s*=\s*0", hdr) and re.search(r"GAD_SIM_X_U8\s*=\s*1", hdr)
    import gad
    assert all(hasattr(gad, f) for f in ("cosine_rows", "group_aggregate", "write_baselines"))


def test_workspace_query():
    lib = _capi.load()
    q = lib.gad_cosine_rows_workspace_bytes
    sizes = [q(130, 33, 1040, U8, s) for s in (1, 2, 3, 7, 64)]
    assert all(a > 0 for a in sizes) and sizes == sorted(sizes) and len(set(sizes)) == len(sizes)       # monotone in splits
    assert sizes[0] >= 4 * (130 * 33 + 130 + 33) and sizes[3] >= 7 * 4 * (130 * 33 + 130 + 33)
    assert q(130, 33, 1040, F32, 3) == q(130, 33, 1040, U8, 3)                                          # one plan for both kinds
    auto = q(5000, 50, 196608, U8, 0)
    assert auto in [q(5000, 50, 196608, U8, s) for s in range(1, 65)]                                   # the automatic count is one of them
    assert q(5000, 64, 196608, U8, 0) // q(5000, 1, 196608, U8, 0) >= 32                                # ... and does not shrink with M
    for bad in ((0, 1, 16, U8, 0), (1, 0, 16, U8, 0), (1, 1, 0, U8, 0), (1, 1, 8, U8, 0), (1, 1, 6, F32, 0), (1, 1, 16, 2, 0),
                (1, 1, 16, -1, 0), (1, 1, 16, U8, -1), (1, 1, 16, U8, 1 << 20), (-5, 1, 16, F32, 0), (1, 1, -16, F32, 0)):
        assert q(*bad) == -1 and _err(lib), bad
    assert q(1, 1, 4, F32, 0) > 0 and q(1, 1, 16, U8, 0) > 0


def test_cosine_rows_host_refusals():
    lib = _capi.load()
    need = lib.gad_cosine_rows_workspace_bytes(130, 33, 1040, U8, 3)

    def call(X=P, kind=U8, ldx=1040, lut=2 * P, Q=3 * P, ldq=1040, sim=4 * P, N=130, M=33, D=1040, splits=3, ws=5 * P,
             ws_bytes=need):
        return lib.gad_cosine_rows(X, kind, ldx, lut, Q, ldq, sim, N, M, D, splits, ws, ws_bytes, None)
    for null in ("X", "Q", "sim", "ws"):
        assert call(**{null: None}) != 0 and "null" in _err(lib), null
    assert call(lut=None) != 0 and "lut" in _err(lib)                       # a table is required with uint8 ...
    assert call(kind=7) != 0 and "x_kind" in _err(lib)
    for arg in ("X", "Q", "ws"):
        assert call(**{arg: P + 8}) != 0 and "aligned" in _err(lib), arg
    assert call(sim=4 * P + 2) != 0 and "aligned" in _err(lib)
    assert call(lut=2 * P + 2) != 0 and "aligned" in _err(lib)
    assert call(D=1032, ldx=1056, ldq=1056) != 0 and "multiple of 16" in _err(lib)     # uint8 quantum
    assert call(kind=F32, D=1038) != 0 and "multiple of 4" in _err(lib)                # fp32 quantum
    assert call(ldx=1048) != 0 and "stride of X" in _err(lib)                          # 8 more bytes: not a multiple of 16
    assert call(ldq=1042) != 0 and "stride of Q" in _err(lib)
    assert call(kind=F32, ldx=1042) != 0 and "stride of X" in _err(lib)
    assert call(ldx=1024) != 0 and "< D" in _err(lib)
    assert call(ldq=1036) != 0 and "< D" in _err(lib)
    for zero in ("N", "M", "D"):
        assert call(**{zero: 0}) != 0 and zero in _err(lib), zero
        assert call(**{zero: -3}) != 0 and zero in _err(lib), zero
    assert call(splits=-1) != 0 and "splits" in _err(lib)
    assert call(ws_bytes=need - 1) != 0 and "workspace" in _err(lib)
    assert call(splits=7) != 0 and "workspace" in _err(lib)                 # sized for three splits
    # ... and what is accepted up to the launch is not tried here: that needs a GPU


def test_cosine_rows_has_no_cpu_path():
    with pytest.raises(_capi.GadError):
        S.cosine_rows(torch.zeros(4, 16), torch.zeros(2, 16))
    with pytest.raises(_capi.GadError):
        S.cosine_rows(torch.zeros(4, 16, dtype=torch.uint8), torch.zeros(2, 16))


def test_pixel_lut_is_the_fp32_transform():
    lut = S.pixel_lut()
    assert lut.dtype == np.float32 and lut.shape == (256,)
    assert np.array_equal(lut, SR.pixel_lut())
    want = torch.arange(256, dtype=torch.uint8).float().div(255)            # ToTensor
    want = (want - 0.5) / 0.5                                               # Normalize([0.5], [0.5])
    assert np.array_equal(lut, want.numpy())
    assert lut[0] == -1.0 and lut[255] == 1.0 and not np.any(lut == 0.0)


# ---- the host statements on a canned matrix: eighths, so every float32 sum is exact whatever its order ----
SIM = (np.array([[4, -2, 7], [1, 1, 7], [4, 8, -8], [0, 1, 0], [4, -2, 3], [-3, 5, 3], [4, 8, 2], [6, 0, -1]]) / 8.0).astype(np.float32)
GROUPS = [np.array([0, 2]), np.array([5]), np.array([1, 3, 7]), np.array([4, 6])]      # groups 0 and 3 tie in column 0


def test_group_aggregate_values_dtypes_shapes():
    gmax, gavg = S.group_aggregate(SIM, GROUPS)
    assert gmax.dtype == np.float64 and gavg.dtype == np.float64 and gmax.shape == gavg.shape == (4, 3)
    wmax, wavg = SR.group_max_avg(SIM, GROUPS)
    assert np.array_equal(gmax, wmax) and np.array_equal(gavg, wavg)
    assert np.array_equal(gavg, gavg.astype(np.float32).astype(np.float64))           # float64 holding float32 means
    assert gavg[2, 0] == float(np.float32(7 / 8) / np.float32(3))                     # the mean of three is rounded in float32
    assert gavg[2, 0] != (7 / 8) / 3
    as_dict = S.group_aggregate(SIM, {i: g for i, g in enumerate(GROUPS)})
    assert np.array_equal(as_dict[0], gmax) and np.array_equal(as_dict[1], gavg)
    vmax, vavg = S.group_aggregate(SIM[:, 1], GROUPS)                                 # a score vector: [G, 1]
    assert vmax.shape == vavg.shape == (4, 1) and np.array_equal(vmax[:, 0], gmax[:, 1]) and np.array_equal(vavg[:, 0], gavg[:, 1])


def test_group_aggregate_refuses_an_empty_group_by_name():
    with pytest.raises(ValueError, match="group 2"):
        S.group_aggregate(SIM, [np.array([0]), np.array([1]), np.array([], dtype=np.int64)])


def test_write_baselines_files_and_stable_ranks(tmp_path):
    gmax, gavg = S.group_aggregate(SIM, GROUPS)
    out = S.write_baselines(str(tmp_path), "artist", {"max_pixel_similarity": gmax, "avg_pixel_similarity": gavg})
    assert out == os.path.join(str(tmp_path), "baselines")
    want = set()
    for name, arr in (("max_pixel_similarity", gmax), ("avg_pixel_similarity", gavg)):
        want |= {f"artist_{name}.npy", f"all_generated_images_artist_rank_{name}.npy"}
        want |= {f"generated_image_{i}_artist_rank_{name}.npy" for i in range(3)}
        assert np.array_equal(np.load(os.path.join(out, f"artist_{name}.npy")), arr)
        for i in range(3):
            rank = np.load(os.path.join(out, f"generated_image_{i}_artist_rank_{name}.npy"))
            assert np.array_equal(rank, SR.stable_rank(arr[:, i])), (name, i)
        rank = np.load(os.path.join(out, f"all_generated_images_artist_rank_{name}.npy"))
        assert np.array_equal(rank, SR.stable_rank(arr.mean(axis=-1)))
    assert set(os.listdir(out)) == want
    # ties: groups 0 and 3 share the column-0 maximum 4/8 and keep their index order
    assert gmax[0, 0] == gmax[3, 0]
    r0 = np.load(os.path.join(out, "generated_image_0_artist_rank_max_pixel_similarity.npy")).tolist()
    assert r0.index(0) + 1 == r0.index(3)
    # a [G, 1] array without the per-image files: the aesthetic program's set
    out2 = S.write_baselines(str(tmp_path / "a"), "filename", {"max_aesthetic_score": gmax[:, :1]}, per_image=False)
    assert set(os.listdir(out2)) == {"filename_max_aesthetic_score.npy", "all_generated_images_filename_rank_max_aesthetic_score.npy"}
    assert np.array_equal(np.load(os.path.join(out2, "all_generated_images_filename_rank_max_aesthetic_score.npy")),
                          SR.stable_rank(gmax[:, 0]))


def test_arrays_load_through_the_baseline_lds_reader_conditions(tmp_path):
    """text_to_image/baseline_lds.py reads `{baseline}.npy` and requires shape[0] == num_groups and shape[-1] >=
    num_model_behaviors; with one behaviour it averages over the last axis."""
    gmax, gavg = S.group_aggregate(SIM, GROUPS)
    out = S.write_baselines(str(tmp_path), "artist", {"max_clip_similarity": gmax, "avg_clip_similarity": gavg,
                                                      "avg_aesthetic_score": gavg[:, :1]})
    for baseline, behaviours in (("artist_max_clip_similarity", 3), ("artist_avg_clip_similarity", 1), ("artist_avg_aesthetic_score", 1)):
        with open(os.path.join(out, f"{baseline}.npy"), "rb") as handle:
            attrs_all = np.load(handle)
        assert attrs_all.shape[0] == len(GROUPS)
        assert attrs_all.shape[-1] >= behaviours
        if behaviours == 1:
            attrs_all = np.mean(attrs_all, axis=-1, keepdims=True)
        assert attrs_all.shape == (len(GROUPS), behaviours) and np.isfinite(attrs_all).all()


# ---- the entry points' refusals: all before anything touches a device ----
ENV = ("GAD_SD_SCORER", "GAD_VAE_DECODER_TS", "GAD_CLIP_B32_WEIGHTS", "GAD_CLIP_L14_WEIGHTS", "GAD_AESTHETIC_WEIGHTS")


@pytest.fixture
def clean_env(monkeypatch):
    for v in ENV:
        monkeypatch.delenv(v, raising=False)
    return monkeypatch


@pytest.fixture
def tiny_cache(tmp_path):
    from text_to_image.train_text_to_image_lora import synthetic_cache
    d = tmp_path / "train"
    synthetic_cache(str(d / "latent_cache.pt"), n=12, n_artists=3, res=32, ctx_dim=8)
    return str(d)


def _programs():
    from text_to_image import aesthetic_score, baselines, clip_similarity, pixel_similarity
    return baselines, pixel_similarity, clip_similarity, aesthetic_score


def _args(mod, tmp_path, data_dir, *extra):
    argv = ["--output_dir", str(tmp_path / "out"), "--train_data_dir", data_dir, "--resolution", "32", "--device", "cpu", *extra]
    if mod.__name__.split(".")[-1] != "aesthetic_score":
        argv += ["--reference_lora_dir", str(tmp_path / "lora")]
    return mod.parse_args(argv)


def test_entry_points_keep_the_reference_flags_and_defaults(tmp_path):
    baselines, pixel, clip, aest = _programs()
    for mod in (baselines, pixel, clip):
        a = mod.parse_args(["--reference_lora_dir", "x", "--output_dir", "y"])
        assert (a.pretrained_model_name_or_path, a.revision, a.variant) == ("lambdalabs/miniSD-diffusers", None, None)
        assert (a.dataset, a.num_images, a.resolution, a.seed, a.cls, a.group) == ("artbench", 50, 256, 42, "post_impressionism", "artist")
        assert (a.dataloader_num_workers, a.batch_size) == (4, 2048)
        assert (a.num_inference_steps, a.guidance_scale, a.train_pixels, a.synthetic_cache) == (100, 7.5, None, False)
        with pytest.raises(SystemExit):
            mod.parse_args(["--output_dir", "y"])
    a = aest.parse_args(["--output_dir", "y"])
    assert (a.dataset, a.cls, a.group, a.dataloader_num_workers, a.batch_size) == ("artbench", "post_impressionism", "artist", 2, 1024)
    assert not hasattr(a, "num_images") and not hasattr(a, "reference_lora_dir")


def test_partial_settings_are_refused_before_anything_is_loaded(clean_env, tmp_path):
    baselines, pixel, clip, aest = _programs()
    nowhere = str(tmp_path / "no_such_dir")                 # nothing is read: the refusal names the setting, not a file
    px = str(tmp_path / "px.npy")
    clean_env.setenv("GAD_VAE_DECODER_TS", "/x/decoder.pt")
    for mod in (baselines, clip):
        with pytest.raises(ValueError, match="GAD_CLIP_B32_WEIGHTS"):
            mod.main(_args(mod, tmp_path, nowhere, "--train_pixels", px))
    with pytest.raises(ValueError, match="--train_pixels"):
        pixel.main(_args(pixel, tmp_path, nowhere))
    clean_env.delenv("GAD_VAE_DECODER_TS")
    for mod in (baselines, pixel, clip):
        with pytest.raises(ValueError, match="GAD_VAE_DECODER_TS"):
            mod.main(_args(mod, tmp_path, nowhere, "--train_pixels", px))
    clean_env.setenv("GAD_SD_SCORER", "clip-seeded")        # seeded towers still need a decoder and images
    with pytest.raises(ValueError, match="GAD_VAE_DECODER_TS"):
        clip.main(_args(clip, tmp_path, nowhere, "--train_pixels", px))
    with pytest.raises(ValueError, match="--train_pixels"):
        aest.main(_args(aest, tmp_path, nowhere))
    clean_env.setenv("GAD_SD_SCORER", "resnet")
    with pytest.raises(ValueError, match="clip-seeded"):
        aest.main(_args(aest, tmp_path, nowhere))
    clean_env.delenv("GAD_SD_SCORER")
    clean_env.setenv("GAD_CLIP_L14_WEIGHTS", "/x/l14.pt")
    with pytest.raises(ValueError, match="GAD_AESTHETIC_WEIGHTS"):
        aest.main(_args(aest, tmp_path, nowhere, "--train_pixels", px))
    clean_env.setenv("GAD_AESTHETIC_WEIGHTS", "/x/head.pt")
    with pytest.raises(ValueError, match="--train_pixels"):
        aest.main(_args(aest, tmp_path, nowhere))
    # each program asks only for what it uses: the aesthetic variables do not disturb the similarity programs' stand-in path,
    # which gets as far as the missing cache
    with pytest.raises(FileNotFoundError, match="synthetic_cache"):
        pixel.main(_args(pixel, tmp_path, nowhere))


def test_missing_cache_is_refused_without_synthetic_cache(clean_env, tmp_path):
    for mod in _programs():
        with pytest.raises(FileNotFoundError, match="--synthetic_cache"):
            mod.main(_args(mod, tmp_path, str(tmp_path / "empty")))
    assert not os.path.exists(tmp_path / "empty")


def test_train_pixels_of_the_wrong_size_or_length_are_refused(clean_env, tmp_path, tiny_cache):
    baselines, pixel, clip, aest = _programs()
    clean_env.setenv("GAD_VAE_DECODER_TS", "/x/decoder.pt")
    clean_env.setenv("GAD_SD_SCORER", "clip-seeded")

    def save(name, arr):
        np.save(str(tmp_path / name), arr)
        return str(tmp_path / name)
    short = save("short.npy", np.zeros((11, 32, 32, 3), dtype=np.uint8))
    big = save("big.npy", np.zeros((12, 64, 64, 3), dtype=np.uint8))
    f32 = save("f32.npy", np.zeros((12, 32, 32, 3), dtype=np.float32))
    chw = save("chw.npy", np.zeros((12, 3, 32, 32), dtype=np.uint8))
    for mod in (baselines, pixel, clip, aest):
        with pytest.raises(ValueError, match="11 images.*12"):
            mod.main(_args(mod, tmp_path, tiny_cache, "--train_pixels", short))
        with pytest.raises(ValueError, match="64 x 64.*--resolution is 32"):
            mod.main(_args(mod, tmp_path, tiny_cache, "--train_pixels", big))
        for bad in (f32, chw):
            with pytest.raises(ValueError, match=r"uint8 \[N, H, W, 3\]"):
                mod.main(_args(mod, tmp_path, tiny_cache, "--train_pixels", bad))
    assert not os.path.exists(tmp_path / "out")             # nothing was written


def test_a_cpu_device_is_refused(clean_env, tmp_path, tiny_cache):
    for mod in _programs():
        with pytest.raises(_capi.GadError, match="no CPU path"):
            mod.main(_args(mod, tmp_path, tiny_cache))
