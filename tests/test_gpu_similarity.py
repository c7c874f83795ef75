"""gad_cosine_rows (csrc/similarity.hip) against fp64 on the MI355X, its determinism and edge contracts, and the four baseline
programs end to end on a tiny synthetic cache.  References: tests/similarity_ref.py."""
import json
import os
import pickle

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import similarity_ref as SR
from gad import _capi
from gad import similarity as S

pytestmark = pytest.mark.gpu
dev = torch.device("cuda:0")
F32, U8 = _capi.SIM_X_F32, _capi.SIM_X_U8
GUARD = 64                                 # floats in front of and behind sim; 4 x that many bytes around the workspace
FILL = -123.5

#        N    M   D-index  padded  splits       every N, M, D, ld and splits value at least once with each kind
SHAPES = [(1, 1, 0, False, 7), (130, 33, 1, True, 3), (257, 65, 2, True, 0), (257, 50, 2, False, 7), (130, 64, 1, False, 1),
          (1, 65, 2, True, 3), (257, 1, 0, True, 0), (130, 50, 0, False, 3)]
DIMS = {F32: (4, 132, 1028), U8: (16, 272, 1040)}
CASES = [(kind, N, M, DIMS[kind][di], pad, splits) for kind in (F32, U8) for (N, M, di, pad, splits) in SHAPES]
_inputs = {}


def make_inputs(kind, N, M, D, pad):
    """(x host, q host, ld, sim64): uniform bytes / fp32 N(0.3, 1) so the dots do not cancel; the padding columns hold 255 / NaN.
    Built once per shape and shared."""
    key = (kind, N, M, D, pad)
    if key not in _inputs:
        rng = np.random.RandomState(1000 * N + 10 * M + D + kind)
        ld = D + ((16 if kind == U8 else 4) if pad else 0)
        if kind == U8:
            x = np.full((N, ld), 255, dtype=np.uint8)
            x[:, :D] = rng.randint(0, 256, size=(N, D), dtype=np.uint8)
        else:
            x = np.full((N, ld), np.nan, dtype=np.float32)
            x[:, :D] = rng.normal(0.3, 1.0, size=(N, D)).astype(np.float32)
        ldq = D + (4 if pad else 0)
        q = np.full((M, ldq), np.nan, dtype=np.float32)
        q[:, :D] = rng.normal(0.3, 1.0, size=(M, D)).astype(np.float32)
        sim64 = SR.cosine64(x[:, :D], q[:, :D])
        for a in (x, q, sim64):
            a.setflags(write=False)
        _inputs[key] = (x, q, sim64)
    return _inputs[key]


_lut_dev = None


def lut_dev():
    global _lut_dev
    if _lut_dev is None:
        _lut_dev = torch.from_numpy(SR.pixel_lut()).to(dev)
    return _lut_dev


def launch(x, q, kind, D, splits, N=None, M=None, ldx=None, ldq=None, ws_bytes=None, expect_ok=True):
    """The raw C call on device copies of x [N, ld] and q [M, ldq] with guard bands around sim and the workspace ->
    (sim [N, M] host, rc); the bands are checked here."""
    lib = _capi.load()
    xd, qd = (t if isinstance(t, torch.Tensor) else torch.from_numpy(np.array(t)).to(dev) for t in (x, q))
    N, M = xd.shape[0] if N is None else N, qd.shape[0] if M is None else M
    ldx, ldq = xd.stride(0) if ldx is None else ldx, qd.stride(0) if ldq is None else ldq
    need = lib.gad_cosine_rows_workspace_bytes(N, M, D, kind, splits)
    alloc = max(need, 0)
    simbuf = torch.full((2 * GUARD + N * M,), FILL, dtype=torch.float32, device=dev)
    wsbuf = torch.full((alloc + 8 * GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    rc = lib.gad_cosine_rows(xd.data_ptr(), kind, ldx, lut_dev().data_ptr() if kind == U8 else None, qd.data_ptr(), ldq,
                             simbuf.data_ptr() + 4 * GUARD, N, M, D, splits, wsbuf.data_ptr() + 4 * GUARD,
                             need if ws_bytes is None else ws_bytes, None)
    torch.cuda.synchronize()
    assert (rc == 0) == expect_ok, lib.gad_last_error().decode()
    s, w = simbuf.cpu().numpy(), wsbuf.cpu().numpy()
    assert np.all(s[:GUARD] == FILL) and np.all(s[GUARD + N * M:] == FILL), "guard band around sim"
    assert np.all(w[:4 * GUARD] == 0xA5) and np.all(w[4 * GUARD + alloc:] == 0xA5), "guard band around the workspace"
    return s[GUARD:GUARD + N * M].reshape(N, M), rc


@pytest.mark.parametrize("kind,N,M,D,pad,splits", CASES)
def test_kernel_against_fp64(kind, N, M, D, pad, splits):
    x, q, sim64 = make_inputs(kind, N, M, D, pad)
    sim, _ = launch(x, q, kind, D, splits)
    err = np.abs(sim.astype(np.float64) - sim64).max()
    err_torch = np.abs(SR.cosine_torch32(x[:, :D], q[:, :D]).astype(np.float64) - sim64).max()
    print(f"\nsimilarity-error kind={'u8' if kind == U8 else 'f32'} N={N} M={M} D={D} ld={x.shape[1]} splits={splits} "
          f"kernel={err:.3e} torch_fp32={err_torch:.3e} bound={SR.tolerance(D):.3e}")
    assert np.isfinite(sim).all()
    assert err <= SR.tolerance(D)


@pytest.mark.parametrize("N,M,D,pad,splits", [(1, 1, 16, False, 7), (130, 33, 272, True, 3), (257, 65, 1040, True, 0)])
def test_uint8_through_the_table_equals_fp32_on_the_decoded_matrix(N, M, D, pad, splits):
    x, q, _ = make_inputs(U8, N, M, D, pad)
    a, _ = launch(x, q, U8, D, splits)
    decoded = SR.pixel_lut()[x]                                             # the padding decodes to 1.0 and is never read
    b, _ = launch(decoded, q, F32, D, splits)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_two_launches_are_bit_identical_and_column_blocks_are_independent():
    for kind, D in ((F32, 1028), (U8, 1040)):
        x, q, _ = make_inputs(kind, 257, 65, D, True)
        a, _ = launch(x, q, kind, D, 0)
        b, _ = launch(x, q, kind, D, 0)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        xd, qd = torch.from_numpy(np.array(x)).to(dev), torch.from_numpy(np.array(q)).to(dev)
        first, _ = launch(xd, qd[:64], kind, D, 0)                          # M = 65 is the launches M = 64 and M = 1
        last, _ = launch(xd, qd[64:], kind, D, 0)
        assert np.array_equal(a[:, :64].view(np.uint32), first.view(np.uint32))
        assert np.array_equal(a[:, 64:].view(np.uint32), last.view(np.uint32))


def test_a_zero_row_gives_a_nan_row_and_nothing_else_changes():
    x, q, _ = make_inputs(F32, 130, 33, 132, True)
    base, _ = launch(x, q, F32, 132, 3)
    z = np.array(x)
    z[77, :132] = 0.0
    got, _ = launch(z, q, F32, 132, 3)
    assert np.isnan(got[77]).all()
    keep = np.arange(130) != 77
    assert np.array_equal(got[keep].view(np.uint32), base[keep].view(np.uint32))


def test_refusals_launch_nothing():
    x, q, _ = make_inputs(U8, 130, 33, 272, True)
    lib = _capi.load()
    need = lib.gad_cosine_rows_workspace_bytes(130, 33, 272, U8, 3)
    for kw in (dict(ws_bytes=need - 1), dict(ldx=256), dict(ldq=270), dict(M=0), dict(splits=-1)):
        splits = kw.pop("splits", 3)
        sim, rc = launch(x, q, U8, 272, splits, expect_ok=False, **kw)
        assert rc != 0 and np.all(sim == FILL), kw
    sim, rc = launch(x, q, 5, 272, 3, expect_ok=False)
    assert rc != 0 and np.all(sim == FILL)


def test_cosine_rows_wrapper_takes_images_and_strided_rows():
    rng = np.random.RandomState(7)
    imgs = torch.from_numpy(rng.randint(0, 256, size=(37, 8, 6, 3), dtype=np.uint8)).to(dev)       # D = 144
    gen = torch.from_numpy(rng.normal(0.3, 1.0, size=(5, 8, 6, 3)).astype(np.float32)).to(dev)
    sim = S.cosine_rows(imgs, gen)
    assert sim.shape == (37, 5) and sim.dtype == torch.float32 and sim.device == imgs.device
    want = SR.cosine64(imgs.cpu().numpy().reshape(37, -1), gen.cpu().numpy().reshape(5, -1))
    assert np.abs(sim.cpu().numpy() - want).max() <= SR.tolerance(144)
    forced = S.cosine_rows(imgs, gen, splits=3)
    assert np.abs(forced.cpu().numpy() - want).max() <= SR.tolerance(144)
    wide = torch.full((37, 160), float("nan"), device=dev)
    wide[:, :144] = S._lut(dev)[imgs.reshape(37, -1).long()]
    view = S.cosine_rows(wide[:, :144], gen.reshape(5, -1))                 # a row-strided view is read in place
    assert torch.equal(view, sim)
    with pytest.raises(_capi.GadError):
        S.cosine_rows(imgs, gen[:, :4])
    with pytest.raises(_capi.GadError):
        S.cosine_rows(imgs.cpu(), gen)


# ---------------------------------------------------------------------------------------------------------------
# the four programs end to end
# ---------------------------------------------------------------------------------------------------------------
class _ToyDecoder(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Conv2d(4, 3, 1)

    def forward(self, x):
        return torch.tanh(F.interpolate(self.conv(x), scale_factor=8.0, mode="nearest"))


RES, N_IMG, N_ART, N_GEN = 128, 40, 6, 3
ENV = ("GAD_SD_SCORER", "GAD_VAE_DECODER_TS", "GAD_CLIP_B32_WEIGHTS", "GAD_CLIP_L14_WEIGHTS", "GAD_AESTHETIC_WEIGHTS")


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    import gad
    from test_gpu_sd import SMALL, rnd
    from text_to_image.train_text_to_image_lora import synthetic_cache
    root = tmp_path_factory.mktemp("similarity")
    data = root / "train"
    cache = synthetic_cache(str(data / "latent_cache.pt"), n=N_IMG, n_artists=N_ART, res=RES, ctx_dim=SMALL["cross_attention_dim"])
    torch.manual_seed(0)
    torch.jit.script(_ToyDecoder().eval()).save(str(root / "decoder.pt"))
    net = gad.UNet2DConditionModel(**SMALL).to(dev)
    for i, p in enumerate(net.inject_lora(rank=4)):
        with torch.no_grad():
            p.copy_(rnd(*p.shape, seed=50 + i, scale=0.05))
    net.save_attn_procs(str(root / "lora"))
    torch.save({k: v for k, v in net.state_dict().items() if "lora_layer" not in k}, root / "unet.pt")
    pixels = np.random.RandomState(3).randint(0, 256, size=(N_IMG, RES, RES, 3), dtype=np.uint8)
    np.save(str(root / "pixels.npy"), pixels)
    common = ["--train_data_dir", str(data), "--resolution", str(RES), "--group", "artist"]
    generate = ["--reference_lora_dir", str(root / "lora"), "--num_images", str(N_GEN), "--seed", "42", "--unet_overrides",
                json.dumps(SMALL), "--unet_weights", str(root / "unet.pt"), "--num_inference_steps", "2", "--batch_size", "16"]
    return dict(root=root, cache=cache, pixels=pixels, common=common, generate=generate)


@pytest.fixture
def env(monkeypatch):
    for v in ENV:
        monkeypatch.delenv(v, raising=False)
    return monkeypatch


def _seeded(env, world):
    from gad import vit
    from test_gpu_vit import TOWERS
    env.setitem(vit.PRESETS, "clip_vit_b32", TOWERS["t10"][0])
    env.setitem(vit.PRESETS, "clip_vit_l14", TOWERS["t50"][0])
    env.setenv("GAD_VAE_DECODER_TS", str(world["root"] / "decoder.pt"))
    env.setenv("GAD_SD_SCORER", "clip-seeded")
    return ["--train_pixels", str(world["root"] / "pixels.npy")]


def _expected_files(group, names, per_image):
    want = {"feature_extractor.json"}
    for name in names:
        want |= {f"{group}_{name}.npy", f"all_generated_images_{group}_rank_{name}.npy"}
        if per_image:
            want |= {f"generated_image_{i}_{group}_rank_{name}.npy" for i in range(N_GEN)}
    return want


def _check_similarity_run(res, out_dir, kinds):
    names = [f"{agg}_{k}" for k in kinds for agg in ("max", "avg")]
    assert set(os.listdir(out_dir)) == _expected_files("artist", names, True)
    for k in kinds:
        x, q = res[k]["x"].cpu().numpy(), res[k]["q"].cpu().numpy()
        x, q = x.reshape(len(x), -1), q.reshape(len(q), -1)
        assert x.shape[0] == N_IMG and q.shape == (N_GEN, x.shape[1])
        tol = SR.tolerance(x.shape[1])
        sim64 = SR.cosine64(x, q)
        assert np.abs(res[k]["sim"].cpu().numpy() - sim64).max() <= tol
        wmax, wavg = SR.group_max_avg(sim64.astype(np.float32), res["group_indices"])
        for agg, want in (("max", wmax), ("avg", wavg)):
            got = np.load(os.path.join(out_dir, f"artist_{agg}_{k}.npy"))
            assert got.dtype == np.float64 and got.shape == (N_ART, N_GEN)
            assert np.abs(got - want).max() <= tol, (agg, k)
            for i in range(N_GEN):
                rank = np.load(os.path.join(out_dir, f"generated_image_{i}_artist_rank_{agg}_{k}.npy"))
                assert np.array_equal(rank, SR.stable_rank(got[:, i]))
            rank = np.load(os.path.join(out_dir, f"all_generated_images_artist_rank_{agg}_{k}.npy"))
            assert np.array_equal(rank, SR.stable_rank(got.mean(axis=-1)))


def test_baselines_end_to_end(world, env, tmp_path):
    from text_to_image import baselines, clip_similarity, pixel_similarity
    from text_to_image.compute_model_behaviors import LatentScorer, latents_to_uint8
    kinds = (baselines.PIXEL, baselines.CLIP)
    groups = [np.where(np.array(world["cache"]["artist"]) == f"artist_{i:03d}")[0] for i in range(N_ART)]

    # ---- stand-ins: pseudo-images of the latents on both sides, LatentScorer embeddings
    out = tmp_path / "standin"
    res = baselines.main(baselines.parse_args(world["common"] + world["generate"] + ["--output_dir", str(out)]))
    assert all(np.array_equal(a, b) for a, b in zip(res["group_indices"], groups)) and len(res["group_indices"]) == N_ART
    lat = world["cache"]["latents"]
    want_x = np.stack([latents_to_uint8(lat[i:i + 1]) for i in range(N_IMG)])
    assert res[baselines.PIXEL]["x"].dtype == torch.uint8 and np.array_equal(res[baselines.PIXEL]["x"].cpu().numpy(), want_x)
    assert res[baselines.CLIP]["x"].shape == (N_IMG, 64)
    _check_similarity_run(res, str(out / "baselines"), kinds)
    tags = json.load(open(out / "baselines" / "feature_extractor.json"))
    assert tags == {baselines.PIXEL: baselines.PIXEL_STANDIN_TAG, baselines.CLIP: LatentScorer.TAG}

    # ---- seeded towers behind a toy TorchScript decoder, training pixels resident as uint8
    extra = _seeded(env, world)
    out = tmp_path / "seeded"
    res = baselines.main(baselines.parse_args(world["common"] + world["generate"] + extra + ["--output_dir", str(out)]))
    assert res[baselines.PIXEL]["x"].dtype == torch.uint8 and np.array_equal(res[baselines.PIXEL]["x"].cpu().numpy(), world["pixels"])
    assert res[baselines.PIXEL]["q"].shape == (N_GEN, RES * RES * 3) and res[baselines.CLIP]["x"].shape == (N_IMG, 32)
    _check_similarity_run(res, str(out / "baselines"), kinds)
    tags = json.load(open(out / "baselines" / "feature_extractor.json"))
    assert "seeded" in tags[baselines.CLIP] and "torchscript" in tags[baselines.CLIP] and "torchscript" in tags[baselines.PIXEL]

    # ---- the two halves write what the union writes
    for mod, kind in ((pixel_similarity, baselines.PIXEL), (clip_similarity, baselines.CLIP)):
        half = tmp_path / kind
        mod.main(mod.parse_args(world["common"] + world["generate"] + extra + ["--output_dir", str(half)]))
        names = [f"max_{kind}", f"avg_{kind}"]
        assert set(os.listdir(half / "baselines")) == _expected_files("artist", names, True)
        for f in os.listdir(half / "baselines"):
            if f.endswith(".npy"):
                assert np.array_equal(np.load(half / "baselines" / f), np.load(out / "baselines" / f)), f


def test_aesthetic_score_end_to_end(world, env, tmp_path):
    from gad import vit
    from text_to_image import aesthetic_score, baselines
    from text_to_image.compute_model_behaviors import LatentScorer
    names = ["max_aesthetic_score", "avg_aesthetic_score"]

    def check(res, out_dir):
        want = _expected_files("artist", names, False) | {"image_aesthetic_score.npy", "aesthetic_score_artist_indices_dict.pkl"}
        assert set(os.listdir(out_dir)) == want
        scores = np.load(os.path.join(out_dir, "image_aesthetic_score.npy"))
        assert scores.dtype == np.float32 and scores.shape == (N_IMG,) and np.array_equal(scores, res["scores"])
        with open(os.path.join(out_dir, "aesthetic_score_artist_indices_dict.pkl"), "rb") as handle:
            d = pickle.load(handle)
        assert type(d) is dict and list(d) == list(range(N_ART)) and all(type(k) is int for k in d)
        artists = np.array(world["cache"]["artist"])
        for i, idx in d.items():
            assert idx.dtype == np.int64 and np.array_equal(idx, np.where(artists == f"artist_{i:03d}")[0])
        wmax, wavg = SR.group_max_avg(scores[:, None], [d[i] for i in range(N_ART)])
        for agg, want_arr in (("max", wmax), ("avg", wavg)):
            got = np.load(os.path.join(out_dir, f"artist_{agg}_aesthetic_score.npy"))
            assert got.dtype == np.float64 and got.shape == (N_ART, 1)
            assert np.abs(got - want_arr).max() <= 16 * 2.0 ** -24 * np.abs(scores).max()      # float32 mean of at most 16 scores
            rank = np.load(os.path.join(out_dir, f"all_generated_images_artist_rank_{agg}_aesthetic_score.npy"))
            assert np.array_equal(rank, SR.stable_rank(got[:, 0]))
        return scores

    out = tmp_path / "standin"
    res = aesthetic_score.main(aesthetic_score.parse_args(world["common"] + ["--output_dir", str(out), "--batch_size", "16"]))
    check(res, str(out / "baselines"))
    assert json.load(open(out / "baselines" / "feature_extractor.json")) == {"aesthetic_score": LatentScorer.TAG}

    extra = _seeded(env, world)
    out = tmp_path / "seeded"
    res = aesthetic_score.main(aesthetic_score.parse_args(world["common"] + extra + ["--output_dir", str(out), "--batch_size", "16"]))
    scores = check(res, str(out / "baselines"))
    l14 = vit.VisionTower.seeded("clip_vit_l14").to(dev)
    head = vit.AestheticHead.seeded(l14).to(dev)
    px = torch.from_numpy(world["pixels"]).to(dev)
    direct = torch.cat([head(baselines.images01(px[s:s + 16])) for s in range(0, N_IMG, 16)]).cpu().numpy()
    assert np.array_equal(scores, direct)                                   # the head called directly on the same batches
    whole = head(baselines.images01(px)).cpu().numpy()
    assert np.abs(scores - whole).max() <= 1e-4 * max(1.0, np.abs(whole).max())
    tags = json.load(open(out / "baselines" / "feature_extractor.json"))
    assert "seeded" in tags["aesthetic_score"]
