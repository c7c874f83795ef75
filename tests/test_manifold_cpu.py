"""Host side of the VGG16 precision / recall tail: bindings, parameter shapes, the fc1 fold, the switch's environment
handling, and the float64 restatements of tests/manifold_ref.py against the project's torch path."""
import math

import pytest
import torch
import torch.nn.functional as F

import manifold_ref as R
from gad import _capi, scoring, vgg
from src.attributions.global_scores import precision_recall as PR


def test_manifold_symbols_are_bound():
    for name in ("gad_manifold_radii", "gad_manifold_radii_workspace_bytes", "gad_manifold_cover", "gad_manifold_cover_workspace_bytes"):
        assert name in _capi.SIGNATURES
    assert callable(PR.make_manifold_device) and callable(PR.calc_pr_device)


def test_vgg16_expected_shapes_count_through_fc2():
    shapes = vgg.expected_shapes()
    conv = sum(math.prod(s) for k, s in shapes.items() if k.startswith("features."))
    fc1 = sum(math.prod(s) for k, s in shapes.items() if k.startswith("classifier.0."))
    fc2 = sum(math.prod(s) for k, s in shapes.items() if k.startswith("classifier.3."))
    assert (conv, fc1, fc2) == (14714688, 102764544, 16781312)
    assert len(shapes) == 2 * 15 and vgg.VGG16.dims == 4096


def test_fc1_fold_is_the_adaptive_pool_of_a_1x1_map_and_the_nhwc_permutation():
    g = torch.Generator().manual_seed(3)
    w = torch.randn(16, 24 * 49, generator=g)
    x = torch.randn(5, 24, 1, 1, generator=g).double()
    want = F.linear(F.adaptive_avg_pool2d(x, 7).flatten(1), w.double())
    got = x.flatten(1) @ vgg.fold_fc1(w, 1).double().T
    assert float((got - want).abs().max()) <= 1e-5 * float(want.abs().max())          # one fp32 rounding of the folded weights
    x7 = torch.randn(5, 24, 7, 7, generator=g).double()
    want = F.linear(x7.flatten(1), w.double())
    got = x7.permute(0, 2, 3, 1).flatten(1) @ vgg.fold_fc1(w, 7).double().T           # NHWC flatten against permuted columns
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    with pytest.raises(ValueError):
        vgg.fold_fc1(w, 2)


def test_vgg16_refuses_resolutions_and_state_dicts_by_name(tmp_path):
    with pytest.raises(ValueError, match="resolution 64"):
        vgg.VGG16(resolution=64)
    sd = {k: torch.zeros(1) for k in vgg.expected_shapes()}
    with pytest.raises(ValueError, match="features.0.weight"):
        vgg.VGG16(sd)
    del sd["features.0.weight"]
    path = tmp_path / "vgg16_short.pth"
    torch.save(sd, path)
    with pytest.raises(KeyError, match="features.0.weight"):
        vgg.VGG16.from_file(str(path))


def test_pr_extractor_environment(monkeypatch):
    monkeypatch.delenv("GAD_VGG16_WEIGHTS", raising=False)
    monkeypatch.delenv("GAD_PR_NET", raising=False)
    assert scoring.pr_extractor("cpu") is None
    monkeypatch.setenv("GAD_PR_NET", "resnet")
    with pytest.raises(ValueError, match="GAD_PR_NET"):
        scoring.pr_extractor("cpu")
    made = []
    monkeypatch.setattr(vgg.VGG16, "seeded", classmethod(lambda cls, seed=1234, resolution=224: made.append(("seeded", seed)) or cls()))
    monkeypatch.setattr(vgg.VGG16, "from_file", classmethod(lambda cls, path, resolution=224: made.append(("file", path)) or cls()))
    monkeypatch.setenv("GAD_PR_NET", "vgg16-seeded")
    assert isinstance(scoring.pr_extractor("cpu"), vgg.VGG16)
    monkeypatch.setenv("GAD_VGG16_WEIGHTS", "/nowhere/vgg16.pth")                      # the weights file wins
    assert isinstance(scoring.pr_extractor("cpu"), vgg.VGG16)
    assert made == [("seeded", 1234), ("file", "/nowhere/vgg16.pth")]


def test_seeded_tag_and_small_seeded_shapes():
    sd = vgg.seeded_state_dict(7)
    assert {k: tuple(v.shape) for k, v in sd.items()} == vgg.expected_shapes()
    assert abs(float(sd["classifier.3.weight"].std()) - math.sqrt(2 / 4096)) < 1e-3


@pytest.mark.parametrize("n_gen,n_ref,D,k", [(40, 50, 16, 3), (9, 31, 8, 1)])
def test_reference_functions_agree_with_the_torch_path(n_gen, n_ref, D, k):
    """integer-valued features: every distance is exact in both arithmetics, so radii and means are equal"""
    g = torch.Generator().manual_seed(n_gen)
    gen = torch.randint(-8, 9, (n_gen, D), generator=g).half()
    ref = torch.randint(-8, 9, (n_ref, D), generator=g).half()
    ref[1] = ref[0]
    m_gen, m_ref = PR.make_manifold(gen, k, 16, 16, "cpu"), PR.make_manifold(ref, k, 16, 16, "cpu")
    assert torch.equal(m_gen.kth, R.radii_ref(gen, k)) and torch.equal(m_ref.kth, R.radii_ref(ref, k))
    if k == 1:
        assert float(m_ref.kth[0]) == 0.0
    p, r = PR.calc_pr(m_gen, m_ref, 16, 16, "cpu")
    assert (p, r) == pytest.approx(R.pr_ref(gen, ref, k), abs=1e-7)
