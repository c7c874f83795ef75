"""CPU checks of the image -> latent path: the host restatement of the reference's transform (gad/latents.py), the pixel table,
the moment-cache schema and every refusal by its message, the two C entry points' ABI and host-side refusals, encode_dataset.py
with an injected stand-in encoder, the restatement's flip coin, and the trainer's new flags."""
import ctypes
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pandas as pd
import pytest
import torch
from PIL import Image

from latent_ref import latent_coin, latent_noise


# ---- the transform -----------------------------------------------------------------------------------------------------------
def test_resized_size_is_torchvisions_int_rule():
    from gad.latents import resized_size
    assert resized_size(256, 256, 256) == (256, 256)
    assert resized_size(300, 200, 256) == (384, 256)                 # landscape: h is the short edge
    assert resized_size(200, 300, 256) == (256, 384)
    assert resized_size(333, 257, 256) == (int(256 * 333 / 257), 256) == (331, 256)      # truncation, not rounding (331.7)
    assert resized_size(257, 333, 256) == (256, 331)
    assert resized_size(17, 31, 16) == (16, 29)                      # 29.18
    assert resized_size(1, 5, 7) == (7, 35)                          # upscaling


def test_center_crop_box_rounds_half_to_even_like_the_reference():
    from gad.latents import center_crop_box
    assert center_crop_box(384, 256, 256) == (64, 0, 320, 256)
    assert center_crop_box(331, 256, 256) == (38, 0, 294, 256)       # (331 - 256) / 2 = 37.5 -> round() -> 38
    assert center_crop_box(256, 261, 256) == (0, 2, 256, 258)        # 2.5 -> 2: python's round, as torchvision's int(round())
    assert center_crop_box(19, 16, 16) == (2, 0, 18, 16)             # 1.5 -> 2
    assert center_crop_box(16, 16, 16) == (0, 0, 16, 16)
    with pytest.raises(ValueError, match="smaller than"):
        center_crop_box(15, 16, 16)


def test_pixel_table_equals_torchs_two_fp32_steps_bit_for_bit():
    from gad.similarity import pixel_lut
    u = torch.arange(256, dtype=torch.uint8)
    x = u.to(torch.float32).div(255)                                 # ToTensor
    want = (x - 0.5) / 0.5                                           # Normalize([0.5], [0.5])
    assert want.dtype == torch.float32
    assert torch.equal(torch.from_numpy(pixel_lut()), want)
    assert pixel_lut()[0] == -1.0 and pixel_lut()[255] == 1.0


def _png(path, arr):
    Image.fromarray(arr).save(path)
    return arr


def test_load_image_u8_identity_resize_crop_and_refusal(tmp_path):
    from gad.latents import center_crop_box, load_image_u8, resized_size
    rng = np.random.RandomState(0)
    a = _png(tmp_path / "a.png", rng.randint(0, 256, (16, 16, 3), dtype=np.uint8))
    for crop in (False, True):
        got = load_image_u8(str(tmp_path / "a.png"), 16, crop)
        assert got.dtype == np.uint8 and got.shape == (16, 16, 3) and np.array_equal(got, a)
    # grey-scale is converted to RGB
    g = _png(tmp_path / "g.png", rng.randint(0, 256, (16, 16), dtype=np.uint8))
    assert np.array_equal(load_image_u8(str(tmp_path / "g.png"), 16, False), np.repeat(g[:, :, None], 3, 2))
    # non-square, odd: [h = 21][w = 37] at resolution 16 -> resized (28, 16) -> columns 6 .. 22
    b = _png(tmp_path / "b.png", rng.randint(0, 256, (21, 37, 3), dtype=np.uint8))
    size = resized_size(37, 21, 16)
    assert size == (28, 16)
    want = np.asarray(Image.fromarray(b).resize(size, Image.BILINEAR).crop(center_crop_box(*size, 16)))
    got = load_image_u8(str(tmp_path / "b.png"), 16, True)
    assert got.shape == (16, 16, 3) and np.array_equal(got, want)
    with pytest.raises(ValueError, match=r"b\.png: resized to 28 x 16, not 16 x 16.*RandomCrop"):
        load_image_u8(str(tmp_path / "b.png"), 16, False)


# ---- moment_cache.pt -----------------------------------------------------------------------------------------------------------
def _meta(n):
    return dict(artist=[f"a{i % 2}" for i in range(n)], filename=[f"f{i}.png" for i in range(n)], style=["s"] * n,
                caption=["a painting"] * n)


def _cache_args(n=3, F=2):
    g = torch.Generator().manual_seed(0)
    return dict(moments=torch.randn(n, F, 8, 2, 2, generator=g), text_emb=torch.randn(1, 77, 12, generator=g), metadata=_meta(n),
                scaling_factor=0.18215, resolution=16, vae_tag="standin")


def test_moment_cache_round_trip(tmp_path):
    from gad.latents import load_moment_cache, write_moment_cache
    for F in (1, 2):
        a = _cache_args(F=F)
        path = str(tmp_path / f"sub{F}" / "moment_cache.pt")
        write_moment_cache(path, **a)
        c = load_moment_cache(path)
        assert torch.equal(c["moments"], a["moments"]) and c["moments"].dtype == torch.float32
        assert torch.equal(c["text_emb"], a["text_emb"])
        assert c["flips"] is (F == 2) and c["scaling_factor"] == 0.18215 and c["resolution"] == 16 and c["vae_tag"] == "standin"
        for k in ("artist", "filename", "style", "caption"):
            assert c[k] == a["metadata"][k]


@pytest.mark.parametrize("key", ["moments", "flips", "scaling_factor", "resolution", "vae_tag", "text_emb", "artist", "filename",
                                 "style", "caption"])
def test_moment_cache_missing_key_is_named(tmp_path, key):
    from gad.latents import load_moment_cache, write_moment_cache
    path = str(tmp_path / "moment_cache.pt")
    c = write_moment_cache(path, **_cache_args())
    del c[key]
    torch.save(c, path)
    with pytest.raises(KeyError, match=f"moment_cache.pt: key '{key}' is missing"):
        load_moment_cache(path)


@pytest.mark.parametrize("change, word", [
    (dict(moments=torch.zeros(3, 2, 8, 2)), "key 'moments' must be fp32"),
    (dict(moments=torch.zeros(3, 3, 8, 2, 2)), "key 'moments' must be fp32"),
    (dict(moments=torch.zeros(3, 2, 7, 2, 2)), "key 'moments' must be fp32"),
    (dict(moments=torch.zeros(3, 2, 8, 2, 2, dtype=torch.float64)), "key 'moments' must be fp32"),
    (dict(flips=False), "key 'flips' is False"),
    (dict(text_emb=torch.zeros(2, 77, 12)), "key 'text_emb' must be"),
    (dict(artist=["a"]), "key 'artist' has 1 entries for 3 rows"),
    (dict(caption=["c"] * 4), "key 'caption' has 4 entries for 3 rows"),
])
def test_moment_cache_misshapen_key_is_named(tmp_path, change, word):
    from gad.latents import load_moment_cache, write_moment_cache
    path = str(tmp_path / "moment_cache.pt")
    c = write_moment_cache(path, **_cache_args())
    c.update(change)
    torch.save(c, path)
    with pytest.raises(ValueError, match=word):
        load_moment_cache(path)


def test_moment_cache_other_refusals(tmp_path):
    from gad import MomentSource, _capi
    from gad.latents import load_moment_cache, write_moment_cache
    with pytest.raises(FileNotFoundError, match="encode_dataset.py"):
        load_moment_cache(str(tmp_path / "moment_cache.pt"))
    a = _cache_args()
    del a["metadata"]["style"]
    with pytest.raises(KeyError, match="style"):
        write_moment_cache(str(tmp_path / "m.pt"), **a)
    with pytest.raises(_capi.GadError, match="device tensor"):
        MomentSource(torch.zeros(3, 2, 8, 2, 2), 0.18215, 0)


# ---- the C entry points --------------------------------------------------------------------------------------------------------
def test_abi_declared_bound_and_exported():
    from gad import _capi
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "gad.h")).read()
    assert "int gad_latent_draw(const float* moments, int64_t N, int32_t F, int64_t n, const int64_t* rows, int32_t B, float* x0," in hdr
    assert "counter (0xFFFFFFFF, r, step, 3)" in hdr and "counter (e >> 2, r, step, 3)" in hdr
    assert "enum gad_latent_flags { GAD_LATENT_SAMPLE = 1, GAD_LATENT_RANDOM_FLIP = 2 };" in hdr
    assert (_capi.LATENT_SAMPLE, _capi.LATENT_RANDOM_FLIP) == (1, 2)
    res, argtypes = _capi.SIGNATURES["gad_latent_draw"]
    assert res is ctypes.c_int and len(argtypes) == 13
    assert argtypes[1] is ctypes.c_int64 and argtypes[2] is ctypes.c_int32 and argtypes[8] is ctypes.c_int64
    assert argtypes[9] is ctypes.c_uint32 and argtypes[10] is ctypes.c_float
    res, argtypes = _capi.SIGNATURES["gad_pixels_to_nchw"]
    assert res is ctypes.c_int and len(argtypes) == 9
    out = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert " T gad_latent_draw" in out and " T gad_pixels_to_nchw" in out


_DRAW = dict(moments=4096, N=5, F=2, n=3072, rows=16384, B=3, x0=8192, flipped=20480, seed=7, step=1, scale=0.5, flags=3)


@pytest.mark.parametrize("bad, word", [
    (dict(moments=None), b"null pointer moments"),
    (dict(rows=None), b"null pointer rows"),
    (dict(x0=None), b"null pointer x0"),
    (dict(moments=4100), b"moments must be 16-B aligned"),
    (dict(x0=8200), b"x0 must be 16-B aligned"),
    (dict(rows=16388), b"rows must be 8-B aligned"),
    (dict(n=3074), b"n=3074"),
    (dict(n=0), b"n=0"),
    (dict(n=4 * (2 ** 32 - 1)), b"reaches the coin's block index"),
    (dict(N=2 ** 32), b"N=4294967296"),
    (dict(N=0), b"N=0"),
    (dict(F=0), b"F=0"),
    (dict(F=3), b"F=3"),
    (dict(F=1, flags=2), b"GAD_LATENT_RANDOM_FLIP needs the flipped slab (F=1"),
    (dict(F=1, flags=3), b"GAD_LATENT_RANDOM_FLIP needs the flipped slab (F=1"),
    (dict(flags=4), b"unknown flag in flags=0x4"),
    (dict(flags=-1), b"unknown flag"),
    (dict(B=0), b"B=0"),
    (dict(B=-2), b"B=-2"),
])
def test_latent_draw_host_refusals_before_any_hip_call(bad, word):
    """Every refusal returns before a HIP call, so a CPU-only machine reaches it (these pointers are not device memory)."""
    from gad import _capi
    lib = _capi.load()
    a = dict(_DRAW, **bad)
    rc = lib.gad_latent_draw(a["moments"], a["N"], a["F"], a["n"], a["rows"], a["B"], a["x0"], a["flipped"], a["seed"], a["step"],
                             a["scale"], a["flags"], None)
    assert rc != 0
    assert word in lib.gad_last_error(), lib.gad_last_error()


_PIX = dict(src=4097, dst=8192, B=2, H=5, W=7, C=3, lut=12288, flip=1)


@pytest.mark.parametrize("bad, word", [
    (dict(src=None), b"null pointer src"),
    (dict(dst=None), b"null pointer dst"),
    (dict(lut=None), b"null pointer lut"),
    (dict(dst=8196), b"dst must be 16-B aligned"),
    (dict(lut=12290), b"lut must be 4-B aligned"),
    (dict(B=0), b"B=0"),
    (dict(H=0), b"H=0"),
    (dict(W=-1), b"W=-1"),
    (dict(C=0), b"C=0"),
    (dict(flip=2), b"flip=2"),
    (dict(B=2 ** 62, H=2 ** 20, W=2 ** 20), b"overflows"),
])
def test_pixels_to_nchw_host_refusals_before_any_hip_call(bad, word):
    from gad import _capi
    lib = _capi.load()
    a = dict(_PIX, **bad)
    rc = lib.gad_pixels_to_nchw(a["src"], a["dst"], a["B"], a["H"], a["W"], a["C"], a["lut"], a["flip"], None)
    assert rc != 0
    assert word in lib.gad_last_error(), lib.gad_last_error()


# ---- encode_dataset.py ---------------------------------------------------------------------------------------------------------
class StandInVAE:
    """8 x 8 average pooling as the encoder: moments [B, 8, H/8, W/8] = pooled | -pooled | first two channels of pooled"""
    tag = "standin-vae"
    config = SimpleNamespace(scaling_factor=0.5, latent_channels=4)

    def encode_moments(self, x):
        p = torch.nn.functional.avg_pool2d(x, 8)
        return torch.cat([p, -p, p[:, :2]], 1)


def _folder(tmp_path, n=6, side=16):
    rng = np.random.RandomState(1)
    data = tmp_path / "artbench"
    data.mkdir()
    order = [3, 0, 5, 1, 4, 2][:n]                                    # metadata.csv's order is not the directory's
    images = {}
    rows = []
    for i in order:
        name = f"img_{i}.png"
        images[name] = _png(data / name, rng.randint(0, 256, (side, side, 3), dtype=np.uint8))
        rows.append(dict(file_name=name, caption="a post-impressionist painting", artist=f"artist_{i % 3}",
                         style="post_impressionism" if i != 4 else "cubism", filename=name))
    pd.DataFrame(rows).to_csv(data / "metadata.csv", index=False)
    return data, images


def _encode_args(data, *extra):
    from text_to_image import encode_dataset as E
    return E, E.parse_args(["--train_data_dir", str(data), "--resolution", "16", "--center_crop", "--cls_key", "style", "--cls",
                            "post_impressionism", "--batch_size", "4", "--device", "cpu", *extra])


def test_encode_dataset_with_a_stand_in_encoder(tmp_path):
    from gad.latents import load_moment_cache
    from gad.similarity import pixel_lut
    data, images = _folder(tmp_path)
    E, a = _encode_args(data)
    text = torch.randn(77, 12, generator=torch.Generator().manual_seed(2))
    assert E.main(a, vae=StandInVAE(), text_emb=text)
    names = ["img_3.png", "img_0.png", "img_5.png", "img_1.png", "img_2.png"]            # csv order, the cubist row filtered out
    c = load_moment_cache(str(data / "moment_cache.pt"))
    assert c["filename"] == names and c["artist"] == ["artist_0", "artist_0", "artist_2", "artist_1", "artist_2"]
    assert c["flips"] is True and c["resolution"] == 16 and c["scaling_factor"] == 0.5 and c["vae_tag"] == "standin-vae"
    assert tuple(c["moments"].shape) == (5, 2, 8, 2, 2) and torch.equal(c["text_emb"], text[None])
    px = np.load(data / "train_pixels.npy")
    assert px.dtype == np.uint8 and np.array_equal(px, np.stack([images[f] for f in names]))
    x = torch.from_numpy(pixel_lut())[torch.from_numpy(px).long()].permute(0, 3, 1, 2)
    vae = StandInVAE()
    assert torch.equal(c["moments"][:, 0], vae.encode_moments(x))
    assert torch.equal(c["moments"][:, 1], vae.encode_moments(x.flip(3)))
    assert not torch.equal(c["moments"][:, 0], c["moments"][:, 1])
    lc = torch.load(data / "latent_cache.pt", weights_only=False)
    assert torch.equal(lc["latents"], c["moments"][:, 0, :4] * 0.5) and tuple(lc["latents"].shape) == (5, 4, 2, 2)
    assert torch.equal(lc["text_emb"], c["text_emb"]) and lc["filename"] == names and lc["style"] == ["post_impressionism"] * 5
    # an existing output is not overwritten without --overwrite
    with pytest.raises(FileExistsError, match="moment_cache.pt exists: pass --overwrite"):
        E.main(a, vae=StandInVAE(), text_emb=text)
    E, a = _encode_args(data, "--overwrite", "--no_flip")
    assert E.main(a, vae=StandInVAE(), text_emb={"cond": text, "uncond": text})
    c1 = load_moment_cache(str(data / "moment_cache.pt"))
    assert c1["flips"] is False and torch.equal(c1["moments"][:, 0], c["moments"][:, 0]) and c1["moments"].shape[1] == 1


def test_encode_dataset_refusals_come_before_any_image_is_read(tmp_path, monkeypatch):
    data = tmp_path / "nothing_here"                                  # no metadata.csv, no image: reading either would raise otherwise
    data.mkdir()
    E, a = _encode_args(data)
    for var in ("GAD_VAE_WEIGHTS", "GAD_SD_TEXT_WEIGHTS", "GAD_CLIP_BPE"):
        monkeypatch.delenv(var, raising=False)
    with pytest.raises(ValueError, match="GAD_VAE_WEIGHTS is not set"):
        E.main(a, text_emb=torch.zeros(77, 12))
    with pytest.raises(ValueError, match="no text source: pass --text_emb FILE, or set GAD_SD_TEXT_WEIGHTS and GAD_CLIP_BPE"):
        E.main(a, vae=StandInVAE())
    monkeypatch.setenv("GAD_SD_TEXT_WEIGHTS", "/weights")             # the weights without a vocabulary: gad.text's own refusal
    with pytest.raises(ValueError, match="GAD_CLIP_BPE is not"):
        E.main(a, vae=StandInVAE())


def test_encode_dataset_text_forms_and_random_crop_refusal(tmp_path):
    data, _ = _folder(tmp_path)
    E, a = _encode_args(data)
    cap = "a post-impressionist painting"
    per = {cap: torch.ones(77, 12)}
    assert E.main(a, vae=StandInVAE(), text_emb=per)
    assert tuple(torch.load(data / "moment_cache.pt", weights_only=False)["text_emb"].shape) == (5, 77, 12)
    E, a = _encode_args(data, "--overwrite")
    with pytest.raises(KeyError, match="1 absent"):
        E.main(a, vae=StandInVAE(), text_emb={"another caption": torch.ones(77, 12)})
    with pytest.raises(ValueError, match="shared embedding must be"):
        E.main(a, vae=StandInVAE(), text_emb=torch.ones(2, 77, 12))
    _png(data / "img_0.png", np.zeros((16, 24, 3), dtype=np.uint8))
    a.center_crop = False
    with pytest.raises(ValueError, match=r"img_0\.png: resized to 24 x 16, not 16 x 16"):
        E.main(a, vae=StandInVAE(), text_emb=per)


# ---- the restatement -----------------------------------------------------------------------------------------------------------
def test_restatement_coin_is_fair_and_noise_is_standard():
    rows, steps = np.arange(64), np.arange(64)
    coins = np.concatenate([latent_coin(0x1234567890ABCDEF, rows, s) for s in steps])
    assert coins.size == 4096 and set(coins.tolist()) == {0, 1}
    sigma = 0.5 / np.sqrt(coins.size)
    assert abs(coins.mean() - 0.5) < 5 * sigma, coins.mean()
    assert np.array_equal(latent_coin(7, [3, 3, 1], 9)[:2], latent_coin(7, [3], 9).repeat(2))       # a function of (seed, r, step)
    z = latent_noise(0x1234567890ABCDEF, 2, 5, 12288)
    assert abs(z.mean()) < 5 / np.sqrt(z.size) and abs(z.std() - 1) < 0.03
    for other in (latent_noise(0x1234567890ABCDEF, 2, 6, 12288), latent_noise(0x1234567890ABCDEF, 3, 5, 12288),
                  latent_noise(0x1234567890ABCDEE, 2, 5, 12288), latent_noise(0x0234567890ABCDEF, 2, 5, 12288)):
        assert abs(np.corrcoef(z, other)[0, 1]) < 0.05


# ---- the trainer's flags -------------------------------------------------------------------------------------------------------
def test_trainer_flags_parse_and_cache_stays_the_default():
    from text_to_image import train_text_to_image_lora as T
    a = T.parse_args(["--train_data_dir", "/d"])
    assert a.latent_source == "cache" and a.center_crop is False and a.random_flip is False
    a = T.parse_args(["--train_data_dir", "/d", "--center_crop", "--random_flip", "--latent_source", "moments"])
    assert a.latent_source == "moments" and a.center_crop and a.random_flip
    with pytest.raises(SystemExit):
        T.parse_args(["--train_data_dir", "/d", "--latent_source", "pixels"])


def test_trainer_refuses_a_cache_that_contradicts_its_flags(tmp_path):
    from gad.latents import write_moment_cache
    from text_to_image import train_text_to_image_lora as T
    base = ["--train_data_dir", str(tmp_path), "--latent_source", "moments", "--resolution", "16"]
    with pytest.raises(FileNotFoundError, match="moment_cache.pt not found"):
        T.load_moments(T.parse_args(base))
    write_moment_cache(str(tmp_path / "moment_cache.pt"), **_cache_args(F=1))
    assert T.load_moments(T.parse_args(base))["flips"] is False
    with pytest.raises(ValueError, match="--random_flip: .*moment_cache.pt was written with --no_flip"):
        T.load_moments(T.parse_args(base + ["--random_flip"]))
    with pytest.raises(ValueError, match="--resolution 32: .*moment_cache.pt was encoded at resolution 16"):
        T.load_moments(T.parse_args(base[:-1] + ["32"]))


def test_training_rows_serves_both_files():
    from text_to_image import train_text_to_image_lora as T
    a = T.parse_args(["--train_data_dir", "/d", "--cls_key", "artist", "--cls", "a1"])
    cache = _meta(5)
    assert T.training_rows(a, cache, 5, "/nowhere").tolist() == [1, 3]
    a = T.parse_args(["--train_data_dir", "/d"])
    assert T.training_rows(a, cache, 5, "/nowhere").tolist() == [0, 1, 2, 3, 4]
