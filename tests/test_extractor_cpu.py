"""The host layer the score-tail networks share (gad/extractor.py) and the one table that says which of them runs
(gad/scoring.py: ROLES, resolve), without a GPU.  The networks themselves are not built here: their seeded state dicts and
`load_state_dict` are stubbed, so that the real `seeded` / `from_file` run and name the class and the tag."""
import hashlib

import pytest
import torch

from gad import extractor, inception, scoring, vgg, vit

WANT = {"a.weight": (2, 3), "a.bias": (2,)}


def _sd():
    return {"a.weight": torch.zeros(2, 3), "a.bias": torch.zeros(2)}


def test_check_state_dict_messages():
    extractor.check_state_dict("Net(x)", _sd(), WANT)
    sd = _sd()
    del sd["a.bias"]
    with pytest.raises(KeyError, match=r"Net\(x\): missing key 'a\.bias'"):
        extractor.check_state_dict("Net(x)", sd, WANT)
    sd = _sd()
    sd["a.weight"] = torch.zeros(3, 2)
    with pytest.raises(ValueError, match=r"Net\(x\): 'a\.weight' has shape \(3, 2\), expected \(2, 3\)"):
        extractor.check_state_dict("Net(x)", sd, WANT)
    sd = _sd()
    sd["b.weight"], sd["aux.weight"] = torch.zeros(1), torch.zeros(1)
    extractor.check_state_dict("Net(x)", sd, WANT)                                         # extra keys ignored
    with pytest.raises(KeyError, match=r"Net\(x\): unexpected key 'b\.weight'"):          # ... or refused, but for the tolerated ones
        extractor.check_state_dict("Net(x)", sd, WANT, extra=lambda k: k.startswith("aux."))
    del sd["b.weight"]
    extractor.check_state_dict("Net(x)", sd, WANT, extra=lambda k: k.startswith("aux."))
    # under a prefix the message names the key as the file has it
    pre = {"m." + k: v for k, v in _sd().items()}
    extractor.check_state_dict("Net(x)", pre, WANT, prefix="m.")
    del pre["m.a.bias"]
    with pytest.raises(KeyError, match=r"missing key 'm\.a\.bias'"):
        extractor.check_state_dict("Net(x)", pre, WANT, prefix="m.")


def test_file_tag_is_the_sha256_of_the_bytes(tmp_path):
    path = tmp_path / "weights.pth"
    path.write_bytes(b"not a checkpoint, only bytes" * 100)
    digest = hashlib.sha256(path.read_bytes()).hexdigest()[:12]
    assert extractor.file_digest(str(path)) == digest
    assert extractor.file_tag("vgg16", str(path)) == f"vgg16:weights.pth:{digest}"
    assert extractor.file_tag("inception-fid", str(path), basename=False) == f"inception-fid:{digest}"


def test_base_class_refuses_without_weights_and_moves_nested_weights():
    class Net(extractor.Extractor):
        owner, dims, max_batch = "Net(x)", 1, 2

        def _chunk(self, x):
            return x.flatten(1)[:, :1] + self.w["b"][0]

    net = Net("net-unloaded")
    with pytest.raises(extractor._capi.GadError, match=r"Net\(x\): no weights loaded"):
        net(torch.zeros(1, 3, 2, 2))
    net.w = {"b": (torch.ones(1), torch.zeros(1)), 0: {"ln": (torch.zeros(2), torch.zeros(2))}, "cls": torch.zeros(3)}
    assert net.to("cpu") is net and net.w[0]["ln"][1].shape == (2,)
    x = torch.arange(5 * 12, dtype=torch.float32).view(5, 3, 2, 2)                       # three chunks of at most two images
    assert torch.equal(net(x), x.flatten(1)[:, :1] + 1) and net.tag == "net-unloaded"


# role -> (class, the public function, tag seeded, tag from a file)
ROLES = {
    "fid": (inception.InceptionV3, lambda: scoring.default_extractor(64, "cpu"), "inception-fid-seeded1234", "inception-fid:{digest}"),
    "is": (inception.InceptionV3, lambda: scoring.is_extractor("cpu"), None, "inception-torchvision:{digest}"),
    "pr": (vgg.VGG16, lambda: scoring.pr_extractor("cpu"), "vgg16-seeded1234", "vgg16:w.pth:{digest}"),
    "diversity": (vit.VisionTower, lambda: scoring.diversity_extractor("cpu"), "blip_vqa_base-seeded1234", "blip_vqa_base:w.pth:{digest}"),
}


@pytest.fixture
def stubbed(monkeypatch, tmp_path):
    """no variable set, no weights made or checked; -> (path of a loadable file, its digest)"""
    for weights, switch, *_ in scoring.ROLES.values():
        monkeypatch.delenv(weights, raising=False)
        if switch:
            monkeypatch.delenv(switch, raising=False)
    monkeypatch.delenv("GAD_FEATURE_NET_TS", raising=False)
    for mod, cls in ((inception, inception.InceptionV3), (vgg, vgg.VGG16), (vit, vit.VisionTower)):
        monkeypatch.setattr(mod, "seeded_state_dict", lambda *a: None)
        monkeypatch.setattr(cls, "load_state_dict", lambda self, sd: self)
    path = tmp_path / "w.pth"
    torch.save({}, path)
    scoring._REF_STATS.clear()
    yield str(path), hashlib.sha256(path.read_bytes()).hexdigest()[:12]
    scoring._REF_STATS.clear()


def test_the_table_names_every_role():
    assert sorted(scoring.ROLES) == sorted(ROLES)


@pytest.mark.parametrize("role", sorted(ROLES))
def test_role_precedence(role, stubbed, monkeypatch):
    path, digest = stubbed
    cls, public, seeded_tag, file_tag = ROLES[role]
    weights, switch, value, _, _ = scoring.ROLES[role]
    # unset: None, or the stand-in where the caller has one
    assert scoring.resolve(role, "cpu") is None and scoring._REF_STATS == {}
    if role == "fid":
        net = public()
        assert isinstance(net, scoring.FeatureNet) and scoring.extractor_tag(net) == "standin-seed1234-d64"
    else:
        assert public() is None
    if switch:
        # the switch: the seeded class, under a tag no file can have
        monkeypatch.setenv(switch, value)
        for net in (public(), scoring.resolve(role, "cpu")):
            assert type(net) is cls and scoring.extractor_tag(net) == seeded_tag and ":" not in seeded_tag
        # any other value is refused, and the message names the one there is
        monkeypatch.setenv(switch, value + "-v2")
        for call in (public, lambda: scoring.resolve(role, "cpu")):
            with pytest.raises(ValueError, match=f"{switch}='{value}-v2': the only value is '{value}'"):
                call()
        monkeypatch.setenv(switch, value)
    # a file beats the switch; the tag carries the file's digest
    monkeypatch.setenv(weights, path)
    for net in (public(), scoring.resolve(role, "cpu")):
        assert type(net) is cls and scoring.extractor_tag(net) == file_tag.format(digest=digest)
    if role in ("fid", "is"):
        assert net.variant == ("fid" if role == "fid" else "torchvision")


@pytest.mark.parametrize("role", sorted(ROLES))
def test_resolve_builds_once_per_setting(role, stubbed, monkeypatch):
    path, _ = stubbed
    weights, switch, value, _, _ = scoring.ROLES[role]
    monkeypatch.setenv(weights, path)
    a = scoring.resolve(role, "cpu")
    assert scoring.resolve(role, "cpu") is a and scoring._REF_STATS[scoring.net_key(role)] is a
    assert list(scoring._REF_STATS) == [("net", role, path, None) + ((None,) if role == "fid" else ())]
    if switch:                                      # a changed variable: another network; the first one is still the first setting's
        monkeypatch.setenv(switch, value)
        monkeypatch.delenv(weights)
        b = scoring.resolve(role, "cpu")
        assert b is not a and scoring.resolve(role, "cpu") is b
        monkeypatch.setenv(weights, path)
        monkeypatch.delenv(switch)
        assert scoring.resolve(role, "cpu") is a
    # unset again: the caller's stand-in, kept likewise; without one, nothing
    monkeypatch.delenv(weights)
    assert scoring.resolve(role, "cpu") is None
    made = []
    s = scoring.resolve(role, "cpu", lambda: made.append(1) or scoring.FeatureNet(8))
    assert scoring.resolve(role, "cpu", lambda: made.append(1) or scoring.FeatureNet(8)) is s and made == [1]


def test_scripted_modules_take_their_tag_from_the_one_function(tmp_path):
    from text_to_image.compute_model_behaviors import ScriptedDecoder

    class Tiny(torch.nn.Module):
        def forward(self, x):
            return x.flatten(1)[:, :16]
    path = tmp_path / "mod.pt"
    torch.jit.script(Tiny()).save(str(path))
    tag = extractor.file_tag("torchscript", str(path))
    assert tag == f"torchscript:mod.pt:{hashlib.sha256(path.read_bytes()).hexdigest()[:12]}"
    assert scoring.ScriptedExtractor(str(path), "cpu").tag == tag and ScriptedDecoder(str(path), "cpu").tag == tag
