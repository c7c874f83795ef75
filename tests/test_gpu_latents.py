"""GPU tests of the image -> latent path: gad_latent_draw against the fp64 restatement (tests/latent_ref.py) with a derived
per-element bound, its row independence and determinism, the flip coin, gad_pixels_to_nchw against the table, encode_dataset.py
end to end on a small seeded AutoencoderKL, and the trainer under --latent_source moments."""
import functools
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

from latent_ref import latent_coin, latent_draw

pytestmark = pytest.mark.gpu
dev = torch.device("cuda:0")
GUARD = 64
SEED = (0x9E3779B9 << 32) | 0xFFFFFFF1            # non-zero high word, bit 63 set
ROWS = [3, 0, 3]                                   # dataset row 3 twice in the batch
SCALE = 0.18215

# k of the SAMPLE bound, in units of 2^-23 relative to |m| + std |z|, from the expression as written,
#   x0 = scale * (m + expf(0.5f * clamp(lv)) * z):
# 0.5f * lv and the clamp are exact; the product std * z, the sum m + (.) and the product scale * (.) round once each, at most
# 2^-24 = 0.5 x 2^-23 relative to a magnitude of at most |m| + std |z| (a fused multiply-add drops one of them): 1.5.  ROCm's
# installed HIP documentation states no ulp bound for expf, so its share is measured: tools/ab_latents.py (profiles/latents_ab.txt)
# observed at most EXPF_OBSERVED x 2^-23 for |std' - std| / std against fp64 on the MI355X (the rounding of the product it is
# measured through included), and twice that is taken.  The 1.01
# covers the second-order products of these relative errors (each below 2^-21).
EXPF_OBSERVED = 1.039
K = (1.5 + 2 * EXPF_OBSERVED) * 1.01


@functools.lru_cache(maxsize=None)
def _moments(n):
    """[5][2][2][n]: N(0,1) means; logvars N(0, 4^2) with entries pushed outside [-30, 20] on both sides"""
    g = torch.Generator().manual_seed(n)
    mo = torch.randn(5, 2, 2, n, generator=g)
    lv = mo[:, :, 1]
    lv.mul_(4.0)
    lv[:, :, 5::17] = 20.0 + 30.0 * torch.rand(lv[:, :, 5::17].shape, generator=g)           # clamped to 20
    lv[:, :, 2::13] = -30.0 - 50.0 * torch.rand(lv[:, :, 2::13].shape, generator=g)          # clamped to -30
    return mo


@functools.lru_cache(maxsize=None)
def _want(n, sample, random_flip):
    return latent_draw(_moments(n).numpy(), ROWS, SEED, 7, SCALE, sample=sample, random_flip=random_flip)


def _draw(moments, rows, seed, step, scale, sample=True, random_flip=False, out=None, flipped=None):
    """moments [N][F][2][n] -> x0 [B][n] through ops.latent_draw_raw's [N, F, 2L, h, w] with L = 1, h = n, w = 1"""
    from gad import ops
    N, F, _, n = moments.shape
    rows = torch.as_tensor(rows, dtype=torch.int64).to(dev)
    x0 = ops.latent_draw_raw(moments.view(N, F, 2, n, 1), rows, seed, step, scale, sample=sample, random_flip=random_flip,
                             out=None if out is None else out.view(len(rows), 1, n, 1), flipped=flipped)
    torch.cuda.synchronize()
    return x0.view(len(rows), n)


def _guarded(B, n):
    buf = torch.full((GUARD + B * n + GUARD,), float("nan"), device=dev)
    fbuf = torch.full((GUARD + B + GUARD,), 0xAB, dtype=torch.uint8, device=dev)              # bytes have no NaN: a sentinel
    return buf, buf[GUARD:GUARD + B * n].view(B, n), fbuf, fbuf[GUARD:GUARD + B]


def _bands_untouched(buf, fbuf):
    return bool(torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[-GUARD:]).all()
                and (fbuf[:GUARD] == 0xAB).all() and (fbuf[-GUARD:] == 0xAB).all())


@pytest.mark.parametrize("random_flip", [False, True])
@pytest.mark.parametrize("n", [192, 3076])
def test_mode_is_exactly_scale_times_mean(n, random_flip):
    w = _want(n, False, random_flip)
    buf, out, fbuf, flipped = _guarded(3, n)
    got = _draw(_moments(n).to(dev), ROWS, SEED, 7, SCALE, sample=False, random_flip=random_flip, out=out, flipped=flipped)
    want = torch.from_numpy(w["m"].astype(np.float32)) * torch.tensor(SCALE, dtype=torch.float32)         # fl(scale * m)
    assert torch.equal(got.cpu(), want)
    assert flipped.cpu().tolist() == w["flipped"].tolist()
    assert _bands_untouched(buf, fbuf)
    assert torch.equal(got[0], got[2])


@pytest.mark.parametrize("random_flip", [False, True])
@pytest.mark.parametrize("n", [192, 3076])
def test_sample_matches_the_restatement(n, random_flip):
    """|got - want| <= scale * (K * 2^-23 * (|m| + std |z|) + std * 1e-6 * (1 + |z|)): K from the roundings of the expression as
    written plus expf's measured share (above), and the bound this project holds its device Box-Muller to (test_gpu_trak.py,
    test_gpu_journey.py)."""
    w = _want(n, True, random_flip)
    buf, out, fbuf, flipped = _guarded(3, n)
    got = _draw(_moments(n).to(dev), ROWS, SEED, 7, SCALE, sample=True, random_flip=random_flip, out=out, flipped=flipped)
    got = got.cpu().numpy().astype(np.float64)
    am, az, std = np.abs(w["m"]), np.abs(w["z"]), w["std"]
    bound = SCALE * (K * 2.0 ** -23 * (am + std * az) + std * 1e-6 * (1 + az))
    err = np.abs(got - w["x0"])
    print(f"n={n} random_flip={random_flip}: max err {err.max():.3e}, max err / bound {(err / bound).max():.3f}, "
          f"std in [{std.min():.3e}, {std.max():.3e}], flipped {w['flipped'].tolist()}")
    assert np.isfinite(got).all()
    assert std.min() == np.exp(-15.0) and std.max() == np.exp(10.0)                     # both clamps are active
    assert (err <= bound).all(), (err / bound).max()
    assert flipped.cpu().tolist() == w["flipped"].tolist()
    assert _bands_untouched(buf, fbuf)
    assert np.array_equal(got[0], got[2])                                               # the repeated row, at both positions


def test_rows_are_independent_and_launches_repeat():
    n = 3076
    mo = _moments(n).to(dev)
    rows = [4, 1, 3, 0, 2]
    full = _draw(mo, rows, SEED, 500, SCALE, random_flip=True)
    assert torch.equal(full, _draw(mo, rows, SEED, 500, SCALE, random_flip=True))       # a repeated launch
    alone = _draw(mo, rows[1:2], SEED, 500, SCALE, random_flip=True)
    assert torch.equal(alone[0], full[1])                                               # the row alone == the row placed second of five
    assert not torch.equal(full[0], full[1])
    clamped = _draw(mo, [-7, 99], SEED, 500, SCALE, random_flip=True)                   # the kernel clamps to [0, N)
    assert torch.equal(clamped[0], full[3]) and torch.equal(clamped[1], full[0])


def test_noise_streams_are_uncorrelated():
    """mean 0, logvar 0, scale 1: x0 = z.  12 288 elements: the standard error of a correlation is 0.009."""
    n = 12288
    zero = torch.zeros(2, 1, 2, n, device=dev)

    def z(seed, step, row=0):
        return _draw(zero, [row], seed, step, 1.0).flatten().cpu().double().numpy()

    base = z(SEED, 7)
    assert abs(base.mean()) < 5 / np.sqrt(n) and abs(base.std() - 1) < 0.03
    for other in (z(SEED, 8), z(SEED ^ 1, 7), z(SEED ^ (1 << 32), 7), z(SEED, 7, row=1)):
        assert abs(np.corrcoef(base, other)[0, 1]) < 0.05
    assert np.array_equal(base, z(SEED, 7))


def test_flip_coin_picks_the_slab_and_agrees_with_the_restatement():
    """The flipped slab is the negated plain slab and every mean is positive, so in MODE the output's sign says which slab was
    read: 64 rows x 64 steps."""
    N, n = 64, 8
    plain = torch.rand(N, 1, 2, n, generator=torch.Generator().manual_seed(0)) + 0.5
    mo = torch.cat([plain, -plain], 1).to(dev)
    rows = torch.arange(N)
    flipped = torch.empty(N, dtype=torch.uint8, device=dev)
    heads = 0
    for step in range(64):
        got = _draw(mo, rows, SEED, step, 1.0, sample=False, random_flip=True, flipped=flipped).cpu()
        coin = latent_coin(SEED, rows.numpy(), step)
        f = flipped.cpu().numpy().astype(np.int64)
        assert np.array_equal(f, coin)
        assert np.array_equal((got < 0).all(1).numpy(), coin == 1) and np.array_equal((got > 0).all(1).numpy(), coin == 0)
        heads += int(coin.sum())
        if step % 16 == 0:
            got = _draw(mo, rows, SEED, step, 1.0, sample=False, random_flip=False, flipped=flipped).cpu()
            assert (flipped == 0).all() and (got > 0).all()
    assert abs(heads / 4096 - 0.5) < 5 * 0.5 / 64


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("shape", [(2, 5, 7, 3), (2, 18, 33, 3), (3, 6, 8, 3), (2, 9, 36, 1), (1, 4, 1028, 4)])
def test_pixels_to_nchw_is_the_table_lookup(shape, flip):
    """5 x 7 and 18 x 33 take the scalar path (odd W); 6 x 8, 9 x 36 and 4 x 1028 (more than one workgroup) the float4 path"""
    from gad import ops
    from gad.similarity import pixel_lut
    B, H, W, Cn = shape
    px = torch.randint(0, 256, shape, dtype=torch.uint8, generator=torch.Generator().manual_seed(W))
    px.view(-1)[:2] = torch.tensor([0, 255], dtype=torch.uint8)
    lut = torch.from_numpy(pixel_lut())
    want = lut[px.long()].permute(0, 3, 1, 2)
    want = (want.flip(3) if flip else want).contiguous()
    buf = torch.full((GUARD + px.numel() + GUARD,), float("nan"), device=dev)
    out = buf[GUARD:GUARD + px.numel()].view(B, Cn, H, W)
    got = ops.pixels_to_nchw_raw(px.to(dev), lut.to(dev), flip=flip, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr() and torch.equal(got.cpu(), want)
    assert torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[-GUARD:]).all()


# ---- the programs ----------------------------------------------------------------------------------------------------------------
def _folder(tmp_path, n=6, side=32):
    import pandas as pd
    rng = np.random.RandomState(1)
    data = tmp_path / "artbench"
    data.mkdir()
    rows, images = [], []
    for i in (3, 0, 5, 1, 4, 2)[:n]:
        name = f"img_{i}.png"
        arr = rng.randint(0, 256, (side, side, 3), dtype=np.uint8)
        Image.fromarray(arr).save(data / name)
        images.append(arr)
        rows.append(dict(file_name=name, caption="a painting", artist=f"artist_{i % 3}", style="post_impressionism", filename=name))
    pd.DataFrame(rows).to_csv(data / "metadata.csv", index=False)
    return data, np.stack(images)


def test_encode_dataset_end_to_end_on_a_small_autoencoder(tmp_path):
    import gad
    from gad import vae as V
    from gad.latents import load_moment_cache
    from gad.similarity import pixel_lut
    from text_to_image import encode_dataset as E
    data, images = _folder(tmp_path)
    cfg = V.make_config("kl", (32, 64), 1, 4, 8)
    vae = gad.AutoencoderKL.seeded(cfg, 3)
    text = torch.randn(77, 96, generator=torch.Generator().manual_seed(2))
    a = E.parse_args(["--train_data_dir", str(data), "--resolution", "32", "--center_crop", "--batch_size", "4"])
    assert E.main(a, vae=vae, text_emb=text)
    c = load_moment_cache(str(data / "moment_cache.pt"))
    assert c["filename"] == [f"img_{i}.png" for i in (3, 0, 5, 1, 4, 2)] and c["flips"] is True and c["vae_tag"] == vae.tag
    assert np.array_equal(np.load(data / "train_pixels.npy"), images)
    x = torch.from_numpy(pixel_lut())[torch.from_numpy(images).long()].permute(0, 3, 1, 2).contiguous()     # prepared on the host
    for f, xf in enumerate((x, x.flip(3).contiguous())):
        want = torch.cat([vae.encode_moments(xf[s:s + 4].to(dev)) for s in (0, 4)]).cpu()                    # the program's batches
        assert tuple(want.shape) == (6, 8, 16, 16)
        assert torch.equal(c["moments"][:, f], want)
    assert not torch.equal(c["moments"][:, 0], c["moments"][:, 1])
    lc = torch.load(data / "latent_cache.pt", weights_only=False)
    assert torch.equal(lc["latents"], c["moments"][:, 0, :4] * cfg.scaling_factor)


def _moment_folder(tmp_path, n=40, res=128, ctx=96):
    from gad.latents import write_moment_cache
    g = torch.Generator().manual_seed(5)
    data = tmp_path / "artbench"
    mo = torch.randn(n, 2, 8, res // 8, res // 8, generator=g)
    mo[:, :, 4:] = mo[:, :, 4:] - 2.0                                                   # std around e^-1: the sample matters
    meta = dict(artist=[f"artist_{i % 5}" for i in range(n)], filename=[f"img_{i}.png" for i in range(n)],
                style=["post_impressionism"] * n, caption=["a painting"] * n)
    write_moment_cache(str(data / "moment_cache.pt"), mo, torch.randn(1, 77, ctx, generator=g) * 0.5, meta, 0.18215, res, "standin")
    torch.save({"latents": mo[:, 0, :4] * 0.18215, "text_emb": torch.randn(1, 77, ctx, generator=g) * 0.5, **meta},
               data / "latent_cache.pt")
    return data


def _train(data, out, *extra):
    from safetensors.torch import load_file
    from text_to_image import train_text_to_image_lora as T
    over = json.dumps(dict(block_out_channels=(64, 128, 128, 128), attention_head_dim=4, cross_attention_dim=96, sample_size=16))
    a = T.parse_args(["--train_data_dir", str(data), "--output_dir", str(out), "--cls_key", "style", "--cls", "post_impressionism",
                      "--resolution", "128", "--train_batch_size", "8", "--unet_overrides", over, "--rank", "4", "--method", "retrain",
                      "--max_train_steps", "3", "--learning_rate", "1e-3", *extra])
    assert T.main(a)
    return load_file(os.path.join(a.model_outdir, "pytorch_lora_weights.safetensors"))


def test_trainer_draws_from_the_moments_reproducibly(tmp_path, monkeypatch):
    from gad import ops
    data = _moment_folder(tmp_path)
    moments = ["--latent_source", "moments", "--random_flip", "--center_crop"]
    calls = []
    real = ops.latent_draw_raw
    monkeypatch.setattr(ops, "latent_draw_raw", lambda *a, **k: (calls.append(k.get("random_flip")), real(*a, **k))[1])
    first = _train(data, tmp_path / "a", *moments, "--seed", "1")
    assert calls == [True] * 3                                                          # one draw per step, with the coin
    again = _train(data, tmp_path / "b", *moments, "--seed", "1")
    other = _train(data, tmp_path / "c", *moments, "--seed", "2")
    assert first.keys() == again.keys() == other.keys() and len(first) > 0
    assert all(torch.equal(first[k], again[k]) for k in first)
    assert any(not torch.equal(first[k], other[k]) for k in first)

    def refuse(*a, **k):
        raise AssertionError("the default source must not launch gad_latent_draw")
    monkeypatch.setattr(ops, "latent_draw_raw", refuse)
    default = _train(data, tmp_path / "d", "--seed", "1", "--random_flip", "--center_crop")
    assert default.keys() == first.keys() and all(torch.isfinite(v).all() for v in default.values())
