"""The precision / recall tail on the GPU: csrc/manifold.hip (radii and coverage without a distance matrix) against the float64
restatements of tests/manifold_ref.py, gad/vgg.py against a plain-torch VGG16, and the `pr=` switch of gad/scoring.py.

The kernel's tile is 128 probe rows x 128 target columns and the target axis is split so that about 512 workgroups exist, so
shapes with more than 128 targets split on their own (130 -> 2 splits, 257 / 259 -> 3): no split hint is needed or offered.
A workgroup walks more than one target tile - what it does at the metric's sizes - once row tiles x column tiles exceed
512; the two `walks_several_tiles` tests take the smallest such shapes, with a last split shorter than the others."""
import numpy as np
import pytest
import torch

import manifold_ref as R
from gad import _capi, ops, scoring, vgg

pytestmark = pytest.mark.gpu
dev = torch.device("cuda:0")
TAIL = 3                          # rows allocated past the end of every matrix and output
KTH_SENTINEL = -7.5               # fp16-exact
WS_TAIL = 4096                    # bytes past the end of the workspace
WS_FILL = 0xA5


def _padded(f, ld):
    """fp16 [N, D] -> device [N + TAIL][ld] with NaN in the padding columns and the rows past the end"""
    buf = torch.full((f.shape[0] + TAIL, ld), float("nan"), device=dev, dtype=torch.float16)
    buf[:f.shape[0], :f.shape[1]] = f.to(dev)
    return buf


def _ws(nbytes):
    assert nbytes > 0, _capi.load().gad_last_error()
    return torch.full((nbytes + WS_TAIL,), WS_FILL, device=dev, dtype=torch.uint8)


def run_radii(f, k, pad=0):
    """gad_manifold_radii on over-allocated, sentinel-guarded buffers -> fp16 [N] on the host"""
    lib = _capi.load()
    (N, D), ld = f.shape, f.shape[1] + pad
    fbuf = _padded(f, ld)
    kth = torch.full((N + TAIL,), KTH_SENTINEL, device=dev, dtype=torch.float16)
    nbytes = lib.gad_manifold_radii_workspace_bytes(N, D, ld, k)
    ws = _ws(nbytes)
    rc = lib.gad_manifold_radii(fbuf.data_ptr(), N, D, ld, k, kth.data_ptr(), ws.data_ptr(), nbytes, ops._stream())
    assert rc == 0, lib.gad_last_error()
    assert bool((kth[N:] == KTH_SENTINEL).all()) and bool((ws[nbytes:] == WS_FILL).all())
    return kth[:N].cpu()


def run_cover(p, t, kth_t, pad_p=0, pad_t=0):
    """gad_manifold_cover on over-allocated, sentinel-guarded buffers -> bool [Np] on the host"""
    lib = _capi.load()
    (Np, D), Nt = p.shape, t.shape[0]
    ldp, ldt = D + pad_p, D + pad_t
    pbuf, tbuf = _padded(p, ldp), _padded(t, ldt)
    kbuf = torch.full((Nt + TAIL,), float("inf"), device=dev, dtype=torch.float16)     # a radius read past the end would cover everything
    kbuf[:Nt] = kth_t.to(dev)
    out = torch.full((Np + TAIL,), 77, device=dev, dtype=torch.uint8)
    nbytes = lib.gad_manifold_cover_workspace_bytes(Np, ldp, Nt, ldt, D)
    ws = _ws(nbytes)
    rc = lib.gad_manifold_cover(pbuf.data_ptr(), Np, ldp, tbuf.data_ptr(), Nt, ldt, D, kbuf.data_ptr(), out.data_ptr(), ws.data_ptr(),
                                nbytes, ops._stream())
    assert rc == 0, lib.gad_last_error()
    assert bool((out[Np:] == 77).all()) and bool((ws[nbytes:] == WS_FILL).all())
    got = out[:Np].cpu()
    assert bool(((got == 0) | (got == 1)).all())
    return got.bool()


def _integers(n, D, seed):
    """integer-valued features in [-8, 8]: every norm, dot product and d2 is an exact fp32 integer in any summation order"""
    return torch.randint(-8, 9, (n, D), generator=torch.Generator().manual_seed(seed)).half()


@pytest.mark.parametrize("N,D,k", [(5, 8, 3), (33, 24, 1), (130, 256, 3), (257, 4096, 3), (300, 72, 7)])
def test_radii_exact_on_integer_features(N, D, k):
    """bit for bit the reference, with a duplicated row (radius 0 for k = 1), an all-zero row, ld > D with NaN padding,
    sentinels behind the output and the workspace, and a second run bit-identical to the first"""
    f = _integers(N, D, N + D)
    f[1] = f[0]
    f[N - 1] = 0
    want = R.radii_ref(f, k)
    got = run_radii(f, k)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    if k == 1:
        assert float(got[0]) == 0.0 and float(got[1]) == 0.0
    padded = run_radii(f, k, pad=24)
    assert torch.equal(padded.view(torch.int16), want.view(torch.int16))
    assert torch.equal(run_radii(f, k).view(torch.int16), got.view(torch.int16))


@pytest.mark.parametrize("Np,Nt,D", [(1, 4, 8), (65, 130, 256), (200, 259, 4096)])
def test_cover_exact_on_integer_features(Np, Nt, D):
    """flags equal the reference; both outcomes occur (a probe that duplicates a target is covered, the radii are tightened
    until some probe is not)"""
    t = _integers(Nt, D, Nt)
    p = _integers(Np, D, Np + 1000)
    p[0] = t[Nt - 1]                                   # covered through the last column of a partial tile
    t[1] = 0
    kth = R.radii_ref(t, 3) if Nt > 3 else torch.zeros(Nt).half()
    if Np > 1:
        d = R.dist16_ref(p, t).float()
        kth = torch.minimum(kth.float(), d.min(0).values.median().expand(Nt)).half()   # radii near the probes' distances
    want = R.cover_ref(p, t, kth)
    got = run_cover(p, t, kth)
    assert torch.equal(got, want)
    assert bool(got[0]) and (Np == 1 or not bool(got.all()))
    assert torch.equal(run_cover(p, t, kth, pad_p=8, pad_t=40), want)
    assert torch.equal(run_cover(p, t, kth), got)


def _tiles_per_split(row_tiles, col_tiles):
    """the kernel's plan restated: about 512 workgroups -> (tiles a workgroup walks, splits, tiles of the last split)"""
    want = min(max(-(-512 // row_tiles), 1), col_tiles)
    tps = -(-col_tiles // want)
    splits = -(-col_tiles // tps)
    return tps, splits, col_tiles - (splits - 1) * tps


@pytest.mark.parametrize("N,D,k", [(3100, 72, 3), (5200, 8, 7)])
def test_radii_exact_when_a_workgroup_walks_several_tiles(N, D, k):
    """3100 rows: 25 x 25 tiles, 13 splits of 2 tiles, the last of 1; 5200 rows: 41 x 41 tiles, 11 splits of 4, the last of 1.
    The walk resets the accumulators per tile, carries the row's list across tiles and reuses the stage buffers the d2 patch
    aliases - bit for bit the reference, with ld > D, and twice the same.  The workspace's size confirms the plan: it holds
    the squared norms (N floats, rounded up to 256 bytes) and 2 x splits partial lists of 8 floats per row."""
    tps, splits, last = _tiles_per_split(-(-N // 128), -(-N // 128))
    assert tps >= 2 and 1 <= last < tps
    lib = _capi.load()
    assert lib.gad_manifold_radii_workspace_bytes(N, D, D, k) == -(-N * 4 // 256) * 256 + -(-2 * splits * N * 32 // 256) * 256
    f = _integers(N, D, N + D)
    f[N - 1] = f[0]                                     # the duplicate sits in the last, partial tile of the last split
    f[129] = 0
    want = R.radii_ref(f, k)
    got = run_radii(f, k, pad=8)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    assert torch.equal(run_radii(f, k, pad=8).view(torch.int16), got.view(torch.int16))
    assert torch.equal(run_radii(f, k).view(torch.int16), want.view(torch.int16))


def test_cover_exact_when_a_workgroup_walks_several_tiles():
    """1300 probes x 12700 targets, D = 40: 11 x 100 tiles, 34 splits of 3 tiles, the last of 1.  Each target's radius is the
    smallest probe distance to it or one fp16 step less, so that hits are rare and sit in every part of the walk: flags
    equal the reference, both outcomes occur, two runs agree.  The workspace holds both matrices' squared norms and
    2 x splits flag bytes per probe."""
    Np, Nt, D = 1300, 12700, 40
    tps, splits, last = _tiles_per_split(-(-Np // 128), -(-Nt // 128))
    assert tps >= 2 and 1 <= last < tps
    lib = _capi.load()
    assert lib.gad_manifold_cover_workspace_bytes(Np, D, Nt, D, D) == \
        -(-Np * 4 // 256) * 256 + -(-Nt * 4 // 256) * 256 + -(-2 * splits * Np // 256) * 256
    t = _integers(Nt, D, Nt)
    p = _integers(Np, D, Np + 1000)
    nearest = R.dist16_ref(p, t).min(0).values          # fp16 [Nt]: the closest probe of every target
    below = (nearest.view(torch.int16) - 1).view(torch.float16)   # one fp16 step less (all distances here are > 0)
    reach = torch.rand(Nt, generator=torch.Generator().manual_seed(5)) < 0.02
    kth = torch.where(reach, nearest, below)
    kth[Nt - 1] = nearest[Nt - 1]                       # a hit through the last column of the last split's only tile
    want = R.cover_ref(p, t, kth)
    assert 0 < int(want.sum()) < Np
    got = run_cover(p, t, kth, pad_p=8, pad_t=16)
    assert torch.equal(got, want)
    assert torch.equal(run_cover(p, t, kth, pad_p=8, pad_t=16), got)
    assert torch.equal(run_cover(p, t, kth), want)


@pytest.mark.parametrize("Np,Nt,D", [(300, 400, 256), (200, 500, 4096)])
def test_random_features_against_float64(Np, Nt, D):
    """randn.clamp_min(0).half(), seed 0, k = 3: every radius within one fp16 ulp of the float64 reference, at most 1 % of
    the radii and at most 1 % of the cover flags different (a condition on rounding ties, not a tolerance)"""
    g = torch.Generator().manual_seed(0)
    p = torch.randn(Np, D, generator=g).clamp_min(0).half()
    t = torch.randn(Nt, D, generator=g).clamp_min(0).half()
    want_kth = R.radii_ref(t, 3)
    got_kth = run_radii(t, 3)
    ulps = (got_kth.view(torch.int16).int() - want_kth.view(torch.int16).int()).abs()
    want_cov = R.cover_ref(p, t, want_kth)
    got_cov = run_cover(p, t, want_kth)
    n_kth, n_cov = int((ulps != 0).sum()), int((got_cov != want_cov).sum())
    print(f"manifold random {Np} x {Nt}, D={D}: {n_kth}/{Nt} radii differ (max {int(ulps.max())} ulp), {n_cov}/{Np} flags differ, "
          f"precision {float(want_cov.float().mean()):.3f}")
    assert int(ulps.max()) <= 1
    assert n_kth <= 0.01 * Nt and n_cov <= 0.01 * Np
    assert 0 < int(want_cov.sum()) < Np


def test_refusals_launch_nothing():
    lib = _capi.load()
    N, D = 40, 16
    f = _padded(_integers(N, D, 1), D)
    kth = torch.full((N + TAIL,), KTH_SENTINEL, device=dev, dtype=torch.float16)
    out = torch.full((N + TAIL,), 77, device=dev, dtype=torch.uint8)
    nbytes = lib.gad_manifold_radii_workspace_bytes(N, D, D, 3)
    cbytes = lib.gad_manifold_cover_workspace_bytes(N, D, N, D, D)
    ws = _ws(max(nbytes, cbytes))
    F, K, O, W, st = f.data_ptr(), kth.data_ptr(), out.data_ptr(), ws.data_ptr(), ops._stream()

    def refused(rc):
        assert rc != 0 and len(lib.gad_last_error()) > 0

    for k in (0, 8):
        assert lib.gad_manifold_radii_workspace_bytes(N, D, D, k) == -1
        refused(lib.gad_manifold_radii(F, N, D, D, k, K, W, nbytes, st))
    assert lib.gad_manifold_radii_workspace_bytes(3, D, D, 3) == -1
    refused(lib.gad_manifold_radii(F, 3, D, D, 3, K, W, nbytes, st))                  # N <= k
    assert lib.gad_manifold_radii_workspace_bytes(N, 12, 16, 3) == -1
    refused(lib.gad_manifold_radii(F, N, 12, 16, 3, K, W, nbytes, st))                # D not a multiple of 8
    assert lib.gad_manifold_radii_workspace_bytes(N, D, 8, 3) == -1
    refused(lib.gad_manifold_radii(F, N, D, 8, 3, K, W, nbytes, st))                  # ld < D
    refused(lib.gad_manifold_radii(F, N, D, D, 3, K, W, nbytes - 1, st))              # short workspace
    for args in ((None, N, D, D, 3, K, W), (F, N, D, D, 3, None, W), (F, N, D, D, 3, K, None)):
        refused(lib.gad_manifold_radii(*args, nbytes, st))
    kt = torch.ones(N, device=dev, dtype=torch.float16)
    good = [F, N, D, F, N, D, D, kt.data_ptr(), O, W, cbytes, st]
    for pos, bad in ((0, None), (3, None), (7, None), (8, None), (9, None), (6, 12), (2, 8), (5, 8), (10, cbytes - 1)):
        args = list(good)
        args[pos] = bad
        refused(lib.gad_manifold_cover(*args))
    assert lib.gad_manifold_cover_workspace_bytes(N, D, N, D, 12) == -1 and lib.gad_manifold_cover_workspace_bytes(N, 8, N, D, D) == -1
    torch.cuda.synchronize()
    # every call above was refused, so nothing has touched `ws` since its fill: a launch after a refusal (the norms pre-pass
    # comes first and writes into `ws`) would show here
    assert bool((kth == KTH_SENTINEL).all()) and bool((out == 77).all()) and bool((ws == WS_FILL).all())


# ---- VGG16 ----
def _rel(a, ref):
    """relative max-norm error against the float64 reference"""
    return float((a.double() - ref).abs().max() / ref.abs().max())


@pytest.fixture(scope="module")
def seeded_sd():
    return vgg.seeded_state_dict(1234)


@pytest.fixture(scope="module")
def trunk_224(seeded_sd):
    """one image through the plain-torch trunk at 224 in float64 and float32, shared by the two 224 tests"""
    x = torch.rand(1, 3, 32, 32, generator=torch.Generator().manual_seed(224))
    with torch.no_grad():
        return x, R.vgg_trunk_ref(seeded_sd, x, 224, torch.float64), R.vgg_trunk_ref(seeded_sd, x, 224, torch.float32)


def _check_vgg(what, got, yard, want):
    e_ref, e_hip = _rel(yard, want), _rel(got, want)
    print(f"VGG16 {what}: fp32 CPU {e_ref:.2e}, HIP {e_hip:.2e} (ratio {e_hip / e_ref:.2f})")
    assert got.shape == want.shape and want.shape[1] == 4096
    assert e_hip <= 16 * e_ref, (what, e_hip, e_ref)
    assert float(want.abs().max()) > 0.1              # the seeded scale survived the 15 layers


def test_vgg16_seeded_at_32(seeded_sd):
    """B = 3 at resolution 32 (1 x 1 final map, the 49 replicas folded into fc1) within 16 x the float32 CPU reference's own
    error against float64"""
    net = vgg.VGG16(seeded_sd, tag="vgg16-seeded1234", resolution=32).to(dev)
    x = torch.rand(3, 3, 32, 32, generator=torch.Generator().manual_seed(32))
    with torch.no_grad():
        want, yard = R.vgg_ref(seeded_sd, x, 32, torch.float64), R.vgg_ref(seeded_sd, x, 32, torch.float32)
    _check_vgg("seeded @32", net(x.to(dev)).cpu(), yard, want)
    assert vgg.VGG16.seeded(5, resolution=32).tag == "vgg16-seeded5"


@pytest.mark.parametrize("fc1", ["seeded", "random"])
def test_vgg16_at_224(fc1, seeded_sd, trunk_224):
    """B = 1 at resolution 224 (7 x 7 final map).  "random": a `classifier.0.weight` of its own draw, different at every
    (channel, position) - a wrong NHWC / NCHW column permutation of fc1 fails here"""
    sd = seeded_sd
    if fc1 == "random":
        sd = dict(seeded_sd)
        sd["classifier.0.weight"] = torch.randn(4096, 25088, generator=torch.Generator().manual_seed(9)) * (2.0 / 25088) ** 0.5
    x, flat64, flat32 = trunk_224
    with torch.no_grad():
        want, yard = R.vgg_head_ref(sd, flat64, torch.float64), R.vgg_head_ref(sd, flat32, torch.float32)
    net = vgg.VGG16(sd, resolution=224).to(dev)
    _check_vgg(f"{fc1} fc1 @224", net(x.to(dev)).cpu(), yard, want)


def test_scoring_switch_writes_the_pr_tag(monkeypatch):
    """GAD_PR_NET=vgg16-seeded on toy2 with 64 generated images: the tag gains `;pr=vgg16-seeded1234` and precision / recall
    are those of the reference functions on the same VGG16 features (at most 1 % of the flags may differ)"""
    from src.datasets import create_dataset
    for k in ("GAD_FEATURE_NET_TS", "GAD_INCEPTION_FID_WEIGHTS", "GAD_FEATURE_NET", "GAD_INCEPTION_IS_WEIGHTS", "GAD_VGG16_WEIGHTS"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("GAD_PR_NET", "vgg16-seeded")
    ds = create_dataset("toy2", train=True)
    g = torch.Generator().manual_seed(0)
    gen = (ds.device_tensor("cpu")[:64].add(1).div(2) * 0.8 + 0.1 * torch.rand(64, 3, 32, 32, generator=g)).clamp(0, 1).to(dev)
    try:
        scoring._REF_STATS.clear()
        row = scoring.global_scores_against_dataset(gen, ds, dev, 64, 256)
        assert row["feature_extractor"] == "standin-seed1234-d256;pr=vgg16-seeded1234"
        net = scoring._REF_STATS[("net", "pr", None, "vgg16-seeded")]
        assert isinstance(net, vgg.VGG16) and net.resolution == 224
        ref_f = scoring.compute_features_torch(net, ds.device_tensor(dev).add_(1).div_(2), 256, dev).half().cpu()
        gen_f = scoring.compute_features_torch(net, gen, 256, dev).half().cpu()
        p, r = R.pr_ref(gen_f, ref_f, 3)
        print(f"switch: precision {row['precision']:.4f} (reference {p:.4f}), recall {row['recall']:.4f} (reference {r:.4f})")
        assert abs(row["precision"] - p) <= 0.01 and abs(row["recall"] - r) <= 0.01
        assert all(np.isfinite(row[k]) for k in ("fid_value", "is", "precision", "recall"))
    finally:
        scoring._REF_STATS.clear()
