"""The InceptionV3 score tail on the GPU (gad/inception.py, csrc/scorenet.hip) against tests/inception_ref.py in float64: the
three kernels on channel slices of over-allocated, sentinel-filled buffers; one real Mixed_5b with every branch checked in
its own slice; the whole net in both variants; and the scoring switch of gad/scoring.py."""
import numpy as np
import pytest
import torch

import inception_ref as R
from gad import _capi, inception, ops, scoring

pytestmark = pytest.mark.gpu
dev = torch.device("cuda:0")
SENTINEL = -12345.625
TAIL = 3                          # rows allocated past the end of every output


def _stream():
    return ops._stream()


def _filled(rows, ld, fill):
    """[rows + TAIL][ld] device buffer filled with `fill`"""
    return torch.full((rows + TAIL, ld), fill, device=dev, dtype=torch.float32)


def _untouched(buf, rows, c0, C):
    """every element outside [0, rows) x [c0, c0 + C) still holds the sentinel"""
    mask = torch.ones_like(buf, dtype=torch.bool)
    mask[:rows, c0:c0 + C] = False
    return bool((buf[mask] == SENTINEL).all())


def _ulps(got, want64):
    """|got - fp32(want)| in units of fp32(want)'s spacing"""
    w32 = want64.to(torch.float32).numpy()
    return np.abs(got.numpy().astype(np.float64) - w32.astype(np.float64)) / np.spacing(np.abs(w32)).astype(np.float64)


# B = 2; the 7 x 8 map pools 7 -> 3 and 8 -> 3 at once
POOL_GEOMS = {"max3s2_7x8": (7, 8, 3, 2, 0, (R.MAX,)), "pool3s1p1_5x5": (5, 5, 3, 1, 1, (R.AVG, R.AVG_VALID, R.MAX)),
              "pool2s2_6x4": (6, 4, 2, 2, 0, (R.MAX, R.AVG)), "pool3s2p1_9x6": (9, 6, 3, 2, 1, (R.MAX, R.AVG, R.AVG_VALID)),
              "avg3s1p1_70x3": (70, 3, 3, 1, 1, (R.AVG_VALID,))}       # 2 x 70 x 3 x 192 / 4 float4s: more than one workgroup


@pytest.mark.parametrize("geom", sorted(POOL_GEOMS))
def test_pool2d_on_channel_slices(geom):
    """Max exact; averages within 4 ulp of the fp32-rounded float64 value (nine adds and a divide); nothing outside the output
    slice is written, nothing outside the input slice is read (the other channels of x hold NaN)."""
    H, W, k, stride, pad, modes = POOL_GEOMS[geom]
    lib, B = _capi.load(), 2
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    g = torch.Generator().manual_seed(H * 100 + W)
    worst = 0.0
    for C in (6, 36, 192):
        x = torch.randn(B, H, W, C, generator=g)
        wants = {(relu, mode): R.pool_ref(x, k, stride, pad, mode, bool(relu)) for relu in (0, 1) for mode in modes}
        for ldx, cx in ((C, 0), (C + 28, 12), (C + 28, 5)):          # (C + 28, 5): a misaligned slice, the scalar path
            xbuf = _filled(B * H * W, ldx, float("nan"))
            xbuf[:B * H * W, cx:cx + C] = x.view(-1, C).to(dev)
            for ldy, cy in ((C, 0), (C + 28, 16), (C + 28, 7)):
                for relu in (0, 1):
                    for mode in modes:
                        ybuf = _filled(B * Ho * Wo, ldy, SENTINEL)
                        rc = lib.gad_pool2d(xbuf.data_ptr() + 4 * cx, ybuf.data_ptr() + 4 * cy, B, H, W, C, ldx, ldy, Ho, Wo, k, stride,
                                            pad, mode, relu, _stream())
                        assert rc == 0, lib.gad_last_error()
                        got = ybuf[:B * Ho * Wo, cy:cy + C].cpu().view(B, Ho, Wo, C)
                        want = wants[relu, mode]
                        case = (C, ldx, cx, ldy, cy, relu, mode)
                        assert _untouched(ybuf, B * Ho * Wo, cy, C), case
                        if mode == R.MAX:
                            assert torch.equal(got.double(), want), case
                        else:
                            u = float(_ulps(got, want).max())
                            worst = max(worst, u)
                            assert u <= 4.0, (case, u)
    print(f"pool2d {geom}: worst average {worst:.2f} ulp")
    if geom == "pool3s1p1_5x5":       # corners divide by 4 (padding excluded) or 9 (counted)
        ones = torch.ones(1, 5, 5, 4, device=dev)
        for mode, corner in ((R.AVG, np.float32(4) / np.float32(9)), (R.AVG_VALID, 1.0)):
            y = torch.empty_like(ones)
            assert lib.gad_pool2d(ones.data_ptr(), y.data_ptr(), 1, 5, 5, 4, 4, 4, 5, 5, 3, 1, 1, mode, 0, _stream()) == 0
            assert float(y[0, 0, 0, 0]) == float(corner) and float(y[0, 2, 2, 0]) == 1.0


@pytest.mark.parametrize("size,out,C", [(32, 299, 3), (4, 7, 3), (5, 3, 3), (8, 8, 3), (6, 11, 8)])
def test_resize_bilinear_matches_interpolate(size, out, C):
    """F.interpolate(bilinear, align_corners=False) in float64, then 2x - 1; |error| <= 2e-6 for inputs in [0,1] (a convex
    combination of four values, doubled).  (6, 11, 8): the float4 store path."""
    lib, B = _capi.load(), 2
    x = torch.rand(B, C, size, size + (1 if C == 8 else 0), generator=torch.Generator().manual_seed(size))
    W = x.shape[-1]
    Wo = out + (2 if C == 8 else 0)
    rows = B * out * Wo
    ybuf = _filled(rows, C, SENTINEL)
    xd = x.to(dev)
    assert lib.gad_resize_bilinear(xd.data_ptr(), ybuf.data_ptr(), B, C, size, W, out, Wo, 2.0, -1.0, _stream()) == 0, lib.gad_last_error()
    got = ybuf[:rows].cpu().view(B, out, Wo, C).double()
    want = R.resize_ref(x, (out, Wo), 2.0, -1.0)
    err = float((got - want).abs().max())
    print(f"resize {size}->{out} C={C}: max abs err {err:.2e}")
    assert err <= 2e-6
    assert bool((ybuf[rows:] == SENTINEL).all())
    if size == out:
        assert torch.equal(got.float(), (2 * x - 1).permute(0, 2, 3, 1))           # an exact transposing copy


@pytest.mark.parametrize("c0", [20, 21])
def test_relu_touches_only_its_slice(c0):
    """a [37][40] slice of a [37][96] buffer (+ rows past the end): exact, everything else untouched; c0 = 21: scalar path"""
    lib = _capi.load()
    buf = torch.full((37 + TAIL, 96), SENTINEL, device=dev)
    x = torch.randn(37, 40, generator=torch.Generator().manual_seed(c0))
    x[3, 5], x[4, 6] = 0.0, -0.0
    buf[:37, c0:c0 + 40] = x.to(dev)
    assert lib.gad_relu(buf.data_ptr() + 4 * c0, 37, 40, 96, _stream()) == 0, lib.gad_last_error()
    assert torch.equal(buf[:37, c0:c0 + 40].cpu(), x.clamp_min(0))
    assert _untouched(buf, 37, c0, 40)


def _rel(a, ref):
    """relative max-norm error against the float64 reference"""
    return float((a.double() - ref).abs().max() / ref.abs().max())


def _random_bn(sd, prefix, seed):
    """BatchNorm statistics that fold into non-trivial scales and biases"""
    g = torch.Generator().manual_seed(seed)
    sd = dict(sd)
    for k in [k for k in sd if k.startswith(prefix) and ".bn." in k]:
        n = sd[k].shape
        sd[k] = {"weight": torch.rand(n, generator=g) + 0.5, "bias": 0.2 * torch.randn(n, generator=g),
                 "running_mean": 0.2 * torch.randn(n, generator=g), "running_var": torch.rand(n, generator=g) + 0.5}[k.rsplit(".", 1)[1]]
    return sd


@pytest.fixture(scope="module")
def seeded_fid_sd():
    return inception.seeded_state_dict("fid", 1234)


@pytest.mark.parametrize("variant", ["fid", "torchvision"])
def test_mixed_5b_branches_land_in_their_slices(variant, seeded_fid_sd):
    """One real Mixed_5b at 35 x 35, B = 1, with random BatchNorm statistics: each branch in its own channel slice of the
    block output against the float64 reference.  Bound per branch: 16 x the error of the float32 CPU reference."""
    sd = _random_bn(seeded_fid_sd, "Mixed_5b.", 5)
    if variant == "torchvision":
        sd["fc.weight"], sd["fc.bias"] = sd["fc.weight"][:1000], sd["fc.bias"][:1000]
    net = inception.InceptionV3(variant, sd).to(dev)
    x = torch.rand(1, 192, 35, 35, generator=torch.Generator().manual_seed(35))
    with torch.no_grad():
        want = R.mixed_a_branches(sd, "Mixed_5b", x.double(), variant)
        yard = R.mixed_a_branches(sd, "Mixed_5b", x, variant)
        got = net.mixed_a(x.permute(0, 2, 3, 1).contiguous().to(dev), "Mixed_5b").cpu()
    assert got.shape == (1, 35, 35, 256)
    c0 = 0
    for name, w, y in zip(("branch1x1", "branch5x5", "branch3x3dbl", "branch_pool"), want, yard):
        n = w.shape[1]
        e_ref, e_hip = _rel(y, w), _rel(got[..., c0:c0 + n].permute(0, 3, 1, 2), w)
        print(f"Mixed_5b[{variant}].{name} [{c0}:{c0 + n}]: fp32 CPU {e_ref:.2e}, HIP {e_hip:.2e}")
        assert e_hip <= 16 * e_ref, (name, e_hip, e_ref)
        c0 += n
    assert c0 == 256 and float(got.min()) == 0.0


@pytest.mark.parametrize("variant", ["fid", "torchvision"])
def test_whole_net_against_the_float64_reference(variant):
    """Seeded weights, B = 2 from 32 x 32 inputs: pool3 and logits.  Yardstick: the float32 CPU reference's relative max-norm
    error against float64 on the same weights and inputs, measured here; the HIP result must be within 16 x that (fp32
    reassociation; the yardstick is about 6e-7: profiles/score_tail_inception.txt)."""
    net = inception.InceptionV3.seeded(variant, 1234)
    sd = inception.seeded_state_dict(variant, 1234)
    x = torch.rand(2, 3, 32, 32, generator=torch.Generator().manual_seed(2))
    p64, l64 = R.forward(sd, x, variant, torch.float64)
    p32, l32 = R.forward(sd, x, variant, torch.float32)
    net.to(dev)
    pool3 = net(x.to(dev))
    logits = net.logits(pool3)
    assert pool3.shape == (2, 2048) and logits.shape == (2, inception.VARIANTS[variant])
    assert net.tag == f"inception-{variant}-seeded1234"
    for what, got, yard, ref in (("pool3", pool3.cpu(), p32, p64), ("logits", logits.cpu(), l32, l64)):
        e_ref, e_hip = _rel(yard, ref), _rel(got, ref)
        print(f"InceptionV3[{variant}] {what}: fp32 CPU {e_ref:.2e}, HIP {e_hip:.2e} (ratio {e_hip / e_ref:.2f})")
        assert e_hip <= 16 * e_ref, (what, e_hip, e_ref)
    assert float(p64.abs().max()) > 0.1           # the seeded scale survived the 48 layers


def test_scoring_switch_and_unchanged_default(monkeypatch):
    """GAD_FEATURE_NET=inception-seeded: finite scores under a seeded tag.  Unset: the stand-in path, bit for bit what the
    same calls made before the switch existed (the score arithmetic restated on the stand-in's features)."""
    from src.attributions.global_scores.inception_score import inception_score_from_probs
    from src.attributions.global_scores.precision_recall import calc_pr, make_manifold
    from src.datasets import create_dataset
    for k in ("GAD_FEATURE_NET_TS", "GAD_INCEPTION_FID_WEIGHTS", "GAD_FEATURE_NET", "GAD_INCEPTION_IS_WEIGHTS"):
        monkeypatch.delenv(k, raising=False)
    ds = create_dataset("toy2", train=True)
    g = torch.Generator().manual_seed(0)
    gen = (ds.device_tensor("cpu")[:64].add(1).div(2) * 0.8 + 0.1 * torch.rand(64, 3, 32, 32, generator=g)).clamp(0, 1).to(dev)
    try:
        scoring._REF_STATS.clear()
        monkeypatch.setenv("GAD_FEATURE_NET", "inception-seeded")
        row = scoring.global_scores_against_dataset(gen, ds, dev, 64, 2048)
        assert row["feature_extractor"] == "inception-fid-seeded1234"
        assert all(np.isfinite(row[k]) for k in ("fid_value", "is", "precision", "recall"))
        assert row["fid_value"] > 0 and row["is"] > 0.999 and 0 <= row["precision"] <= 1 and 0 <= row["recall"] <= 1
        assert isinstance(scoring._REF_STATS[("net", "fid", None, "inception-seeded", None)], inception.InceptionV3)

        scoring._REF_STATS.clear()
        monkeypatch.delenv("GAD_FEATURE_NET")
        row = scoring.global_scores_against_dataset(gen, ds, dev, 64, 256)
        assert row["feature_extractor"] == "standin-seed1234-d256"
        net = scoring.FeatureNet(256, seed=1234).to(dev)
        ref_f = scoring.compute_features_torch(net, ds.device_tensor(dev).add_(1).div_(2), 256, dev)
        gen_f = scoring.compute_features_torch(net, gen, 256, dev)
        fid = scoring.frechet_distance_torch(*scoring.feature_stats_torch(gen_f), *scoring.feature_stats_torch(ref_f))
        p, r = calc_pr(make_manifold(gen_f, 3, 10000, 10000, dev), make_manifold(ref_f, 3, 10000, 10000, dev), 10000, 10000, dev)
        is_value = inception_score_from_probs(torch.softmax(gen_f[:, :1000].double(), dim=1).cpu().numpy())
        assert (row["fid_value"], row["is"], row["precision"], row["recall"]) == (fid, is_value, p, r)
    finally:
        scoring._REF_STATS.clear()
