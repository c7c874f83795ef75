"""CPU checks of the InceptionV3 score tail (gad/inception.py, csrc/scorenet.hip): the three C entry points are exported and
refuse bad arguments before any HIP call; the key grammar, shapes and parameter counts of both variants; state-dict loading;
BatchNorm folding; the extractor precedence of gad/scoring.py; and the reference's own pool semantics (tests/inception_ref.py)."""
import ctypes
import hashlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import inception_ref as R
from gad import _capi, inception, scoring

P = 1 << 24                       # placeholder device addresses: the refusals come before anything reads them


def _pool(lib, x=P, y=2 * P, B=2, H=7, W=7, C=8, ldx=8, ldy=8, Ho=3, Wo=3, k=3, stride=2, pad=0, mode=0, relu=0):
    return lib.gad_pool2d(x, y, B, H, W, C, ldx, ldy, Ho, Wo, k, stride, pad, mode, relu, None)


def test_the_three_symbols_are_exported_and_bound():
    lib = _capi.load()
    for n in ("gad_pool2d", "gad_resize_bilinear", "gad_relu"):
        assert n in _capi.SIGNATURES and hasattr(lib, n), n


@pytest.mark.parametrize("kw,word", [
    (dict(k=4, Ho=2, Wo=2), "k=4"), (dict(ldy=7), "ldy"), (dict(ldx=4), "ldx"), (dict(Ho=4), "Ho=4"), (dict(Wo=2), "Wo=2"),
    (dict(x=None), "null"), (dict(y=None), "null"), (dict(C=0), "C=0"), (dict(C=-4), "C=-4"), (dict(stride=3), "stride"),
    (dict(pad=2), "pad"), (dict(mode=3), "mode"), (dict(B=0), "B=0"), (dict(H=2, Ho=0), "smaller"),
])
def test_pool_refuses_bad_arguments_without_a_device(kw, word):
    lib = _capi.load()
    assert _pool(lib, **kw) != 0
    assert word.encode() in lib.gad_last_error(), lib.gad_last_error()


def test_resize_and_relu_refuse_bad_arguments_without_a_device():
    lib = _capi.load()
    assert lib.gad_resize_bilinear(None, P, 2, 3, 32, 32, 299, 299, 2.0, -1.0, None) != 0 and b"null" in lib.gad_last_error()
    assert lib.gad_resize_bilinear(P, P, 2, 0, 32, 32, 299, 299, 2.0, -1.0, None) != 0 and b"C=0" in lib.gad_last_error()
    assert lib.gad_resize_bilinear(P, P, 2, 3, 32, 32, 0, 299, 2.0, -1.0, None) != 0 and b"Ho=0" in lib.gad_last_error()
    assert lib.gad_relu(None, 37, 40, 96, None) != 0 and b"null" in lib.gad_last_error()
    assert lib.gad_relu(P, 37, 40, 36, None) != 0 and b"ld=36" in lib.gad_last_error()
    assert lib.gad_relu(P, 0, 40, 96, None) != 0 and b"rows=0" in lib.gad_last_error()
    assert lib.gad_relu(P, 37, 0, 96, None) != 0 and b"C=0" in lib.gad_last_error()


# ---- architecture: keys, shapes, counts ----
@pytest.mark.parametrize("variant,ncls,total", [("fid", 1008, 23_850_960), ("torchvision", 1000, 23_834_568)])
def test_key_grammar_shapes_and_parameter_counts(variant, ncls, total):
    shapes = inception.expected_shapes(variant)
    assert len(inception.CONVS) == 94 and len(shapes) == 94 * 5 + 2
    for key, shape in {"Conv2d_1a_3x3.conv.weight": (32, 3, 3, 3), "Conv2d_1a_3x3.bn.running_var": (32,),
                       "Conv2d_3b_1x1.conv.weight": (80, 64, 1, 1), "Conv2d_4a_3x3.bn.bias": (192,),
                       "Mixed_5b.branch1x1.conv.weight": (64, 192, 1, 1), "Mixed_5b.branch5x5_2.conv.weight": (64, 48, 5, 5),
                       "Mixed_5b.branch_pool.conv.weight": (32, 192, 1, 1), "Mixed_5d.branch_pool.conv.weight": (64, 288, 1, 1),
                       "Mixed_6a.branch3x3dbl_3.conv.weight": (96, 96, 3, 3), "Mixed_6a.branch3x3.bn.weight": (384,),
                       "Mixed_6b.branch7x7_2.conv.weight": (128, 128, 1, 7), "Mixed_6c.branch7x7dbl_2.conv.weight": (160, 160, 7, 1),
                       "Mixed_6e.branch7x7dbl_5.conv.weight": (192, 192, 1, 7), "Mixed_7a.branch7x7x3_4.conv.weight": (192, 192, 3, 3),
                       "Mixed_7b.branch3x3dbl_1.conv.weight": (448, 1280, 1, 1), "Mixed_7c.branch3x3_2b.conv.weight": (384, 384, 3, 1),
                       "Mixed_7c.branch3x3_2b.bn.running_mean": (384,), "fc.weight": (ncls, 2048), "fc.bias": (ncls,)}.items():
        assert shapes[key] == shape, key
    assert not any(k.startswith("AuxLogits") or k.endswith("num_batches_tracked") for k in shapes)
    # parameters = conv weights + BatchNorm gamma / beta (+ fc); running statistics are buffers
    count = sum(int(np.prod(s)) for k, s in shapes.items() if not k.endswith(("running_mean", "running_var")))
    assert inception.param_count() == 21_785_568
    assert inception.param_count(variant) == count == total
    # the channels every block hands on, from the layer list alone
    width = {p: sum(co for n, _, co, *_ in inception.CONVS if n.startswith(p + ".") and n.split(".")[1] in last)
             for p, last in [("Mixed_5b", ("branch1x1", "branch5x5_2", "branch3x3dbl_3", "branch_pool")),
                             ("Mixed_6b", ("branch1x1", "branch7x7_3", "branch7x7dbl_5", "branch_pool")),
                             ("Mixed_7c", ("branch1x1", "branch3x3_2a", "branch3x3_2b", "branch3x3dbl_3a", "branch3x3dbl_3b", "branch_pool"))]}
    assert width == {"Mixed_5b": 256, "Mixed_6b": 768, "Mixed_7c": 2048}


@pytest.fixture(scope="module")
def seeded_sd():
    return inception.seeded_state_dict("fid", 7)


def test_seeded_weights_are_he_normal_and_reproducible(seeded_sd):
    again = inception.seeded_state_dict("fid", 7)
    w = seeded_sd["Mixed_6e.branch7x7dbl_5.conv.weight"]
    assert torch.equal(w, again["Mixed_6e.branch7x7dbl_5.conv.weight"])
    assert not torch.equal(w, inception.seeded_state_dict("fid", 8)["Mixed_6e.branch7x7dbl_5.conv.weight"])
    assert float(w.std()) == pytest.approx((2.0 / (192 * 7)) ** 0.5, rel=0.02)
    assert float(seeded_sd["Mixed_5c.branch1x1.bn.weight"].min()) == 1.0 and float(seeded_sd["Mixed_5c.branch1x1.bn.running_var"].max()) == 1.0
    assert float(seeded_sd["Mixed_5c.branch1x1.bn.bias"].abs().max()) == 0.0 and float(seeded_sd["fc.bias"].abs().max()) == 0.0


def test_state_dict_with_aux_head_and_batch_counters_loads(seeded_sd):
    sd = dict(seeded_sd)
    sd["AuxLogits.conv0.conv.weight"] = torch.zeros(128, 768, 1, 1)
    sd["AuxLogits.fc.bias"] = torch.zeros(1008)
    sd["Mixed_5b.branch1x1.bn.num_batches_tracked"] = torch.tensor(0)
    net = inception.InceptionV3("fid", sd)
    w, b = net.w["Mixed_6b.branch7x7_2"]
    assert w.shape == (128, 1, 7, 128) and w.is_contiguous() and w.dtype == torch.float32 and b.shape == (128,)
    assert net.w["fc"][0].shape == (1008, 2048) and len(net.w) == 95


def test_bad_state_dicts_are_rejected_by_key(seeded_sd):
    sd = dict(seeded_sd)
    sd["Mixed_7a.branch3x3_2.conv.weight"] = torch.zeros(320, 192, 3, 2)
    with pytest.raises(ValueError, match=r"Mixed_7a\.branch3x3_2\.conv\.weight.*\(320, 192, 3, 2\)"):
        inception.InceptionV3("fid", sd)
    with pytest.raises(ValueError, match=r"fc\.weight"):                     # the FID file's 1008-way fc is not torchvision's
        inception.InceptionV3("torchvision", seeded_sd)
    sd = dict(seeded_sd)
    del sd["Mixed_6d.branch_pool.bn.running_var"]
    with pytest.raises(KeyError, match=r"missing key 'Mixed_6d\.branch_pool\.bn\.running_var'"):
        inception.InceptionV3("fid", sd)
    sd = dict(seeded_sd)
    sd["Mixed_8a.branch1x1.conv.weight"] = torch.zeros(1)
    with pytest.raises(KeyError, match=r"unexpected key 'Mixed_8a\.branch1x1\.conv\.weight'"):
        inception.InceptionV3("fid", sd)
    with pytest.raises(ValueError, match="variant"):
        inception.InceptionV3("v4")


def test_bn_folding_matches_the_fp64_formula():
    """w' = w gamma / sqrt(var + eps), b' = beta - mean gamma / sqrt(var + eps) in fp64, rounded to fp32 once: against the same
    formula associated differently the folded values are the same fp32 numbers or their neighbours (1 ulp), and the folded
    convolution equals conv -> batch_norm in fp64 to fp32 rounding."""
    g = torch.Generator().manual_seed(3)
    w = torch.randn(24, 10, 1, 7, generator=g)
    gamma, beta = torch.rand(24, generator=g) + 0.5, torch.randn(24, generator=g)
    mean, var = torch.randn(24, generator=g), torch.rand(24, generator=g) * 2 + 0.01
    wf, bf = inception.fold_bn(w, gamma, beta, mean, var)
    assert wf.shape == (24, 1, 7, 10) and wf.dtype == bf.dtype == torch.float32
    inv = 1.0 / np.sqrt(var.double().numpy() + 1e-3)
    want_w = (w.double().numpy() * (gamma.double().numpy() * inv)[:, None, None, None]).transpose(0, 2, 3, 1)
    want_b = beta.double().numpy() - mean.double().numpy() * gamma.double().numpy() * inv
    for got, want in ((wf.numpy(), want_w), (bf.numpy(), want_b)):
        assert np.all(np.abs(got.astype(np.float64) - want) <= np.spacing(np.abs(want).astype(np.float32)))
    x = torch.randn(2, 10, 5, 9, generator=g, dtype=torch.float64)
    ref = F.batch_norm(F.conv2d(x, w.double(), None, 1, (0, 3)), mean.double(), var.double(), gamma.double(), beta.double(), False, 0.0, 1e-3)
    got = F.conv2d(x, wf.permute(0, 3, 1, 2).double(), bf.double(), 1, (0, 3))
    assert float((got - ref).abs().max()) < 4e-7 * float(ref.abs().max())


# ---- gad/scoring.py: which extractor a score row comes from ----
ENV = ("GAD_FEATURE_NET_TS", "GAD_INCEPTION_FID_WEIGHTS", "GAD_FEATURE_NET", "GAD_INCEPTION_IS_WEIGHTS")


def test_default_extractor_precedence_and_tags(monkeypatch, tmp_path, seeded_sd):
    cpu = torch.device("cpu")
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    # nothing set: the stand-in, with its own tag
    net = scoring.default_extractor(64, cpu)
    assert isinstance(net, scoring.FeatureNet) and scoring.extractor_tag(net) == "standin-seed1234-d64"
    assert scoring.is_extractor(cpu) is None
    # the seeded architecture: a tag that cannot be read as a weight file's
    monkeypatch.setenv("GAD_FEATURE_NET", "inception-seeded")
    net = scoring.default_extractor(2048, cpu, seed=7)
    assert isinstance(net, inception.InceptionV3) and net.variant == "fid" and net.dims == 2048
    assert scoring.extractor_tag(net) == "inception-fid-seeded7" and ":" not in scoring.extractor_tag(net)
    assert torch.equal(net.w["Mixed_7c.branch_pool"][0], inception.fold_bn(*(seeded_sd[f"Mixed_7c.branch_pool.{k}"] for k in (
        "conv.weight", "bn.weight", "bn.bias", "bn.running_mean", "bn.running_var")))[0])
    monkeypatch.setenv("GAD_FEATURE_NET", "inception")
    with pytest.raises(ValueError, match="inception-seeded"):
        scoring.default_extractor(2048, cpu)
    # a weight file wins over the seeded switch; its tag carries the file's hash
    path = tmp_path / "pt_inception.pth"
    torch.save(seeded_sd, path)
    digest = hashlib.sha256(path.read_bytes()).hexdigest()[:12]
    monkeypatch.setenv("GAD_FEATURE_NET", "inception-seeded")
    monkeypatch.setenv("GAD_INCEPTION_FID_WEIGHTS", str(path))
    net = scoring.default_extractor(2048, cpu)
    assert isinstance(net, inception.InceptionV3) and net.variant == "fid" and scoring.extractor_tag(net) == f"inception-fid:{digest}"
    # the FID file is not torchvision's: the IS switch rejects it by key
    monkeypatch.setenv("GAD_INCEPTION_IS_WEIGHTS", str(path))
    with pytest.raises(ValueError, match=r"fc\.weight"):
        scoring.is_extractor(cpu)
    tv = dict(seeded_sd)
    tv["fc.weight"], tv["fc.bias"] = seeded_sd["fc.weight"][:1000].clone(), seeded_sd["fc.bias"][:1000].clone()
    tv_path = tmp_path / "inception_v3.pth"
    torch.save(tv, tv_path)
    monkeypatch.setenv("GAD_INCEPTION_IS_WEIGHTS", str(tv_path))
    is_net = scoring.is_extractor(cpu)
    assert is_net.variant == "torchvision" and is_net.w["fc"][0].shape == (1000, 2048)
    assert scoring.extractor_tag(is_net) == f"inception-torchvision:{hashlib.sha256(tv_path.read_bytes()).hexdigest()[:12]}"
    # the TorchScript route still wins over all of them
    ts = tmp_path / "extractor.pt"
    torch.jit.script(_Tiny()).save(str(ts))
    monkeypatch.setenv("GAD_FEATURE_NET_TS", str(ts))
    net = scoring.default_extractor(2048, cpu)
    assert isinstance(net, scoring.ScriptedExtractor) and scoring.extractor_tag(net).startswith("torchscript:extractor.pt:")


class _Tiny(torch.nn.Module):
    def forward(self, x):
        return x.flatten(1)[:, :16]


def test_the_product_path_has_no_cpu_fallback(seeded_sd):
    net = inception.InceptionV3("fid", seeded_sd)
    with pytest.raises(_capi.GadError):
        net(torch.zeros(1, 3, 32, 32))


# ---- the reference's own pooling ----
def test_reference_pool_semantics_match_torch_on_a_5x5_map():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 5, 5, 6, generator=g, dtype=torch.float64)
    xc = x.permute(0, 3, 1, 2)
    back = lambda y: y.permute(0, 2, 3, 1)      # noqa: E731
    for relu in (False, True):
        xin = xc.clamp_min(0) if relu else xc
        for k, s, p in ((3, 1, 1), (3, 2, 0), (2, 2, 0), (3, 2, 1), (2, 1, 1)):
            assert torch.equal(R.pool_ref(x, k, s, p, R.MAX, relu), back(F.max_pool2d(xin, k, s, p)))
            torch.testing.assert_close(R.pool_ref(x, k, s, p, R.AVG, relu), back(F.avg_pool2d(xin, k, s, p)), rtol=1e-14, atol=1e-15)
            torch.testing.assert_close(R.pool_ref(x, k, s, p, R.AVG_VALID, relu),
                                       back(F.avg_pool2d(xin, k, s, p, count_include_pad=False)), rtol=1e-14, atol=1e-15)
    ones = torch.ones(1, 5, 5, 1, dtype=torch.float64)
    assert float(R.pool_ref(ones, 3, 1, 1, R.AVG)[0, 0, 0, 0]) == pytest.approx(4 / 9)        # a corner: four taps of nine
    assert float(R.pool_ref(ones, 3, 1, 1, R.AVG_VALID)[0, 0, 0, 0]) == 1.0                   # ... of four
    assert (R.MAX, R.AVG, R.AVG_VALID) == (_capi.POOL_MAX, _capi.POOL_AVG, _capi.POOL_AVG_VALID)
