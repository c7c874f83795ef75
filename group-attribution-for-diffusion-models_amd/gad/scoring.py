"""Model-behaviour score tail for the CIFAR configuration (reference
src/attributions/global_scores/fid_score.py:23-107).

The reference extracts pool3 features with pytorch_fid's InceptionV3, whose weights are
fetched from a URL (fid_score.py:28) and are unobtainable offline; the feature extractor is
therefore a *seeded random-weight* conv stack built from the same HIP operators (the tail is
~1 % of a coalition's FLOPs), while the score arithmetic - float64 mean / covariance and the
Frechet distance - is restated exactly (fid_score.py:104-105 and
pytorch_fid.calculate_frechet_distance).  Where the weight files exist, `default_extractor` /
`is_extractor` put the real InceptionV3 (gad/inception.py, on the same operators) in its place."""
from __future__ import annotations

import os

import numpy as np
import torch
import torch.nn as nn

from . import nn as gnn
from . import ops
from .extractor import file_tag
from .inception import InceptionV3
from .vgg import VGG16
from .vit import VisionTower


class FeatureNet(nn.Module):
    """[B,3,32,32] in [0,1] -> [B,2048] features (GroupNorm/SiLU conv pyramid + global average pool)."""

    def __init__(self, dims=2048, seed=1234):
        super().__init__()
        rng = torch.random.get_rng_state()
        torch.manual_seed(seed)
        chans = [(3, 64, 1), (64, 128, 2), (128, 256, 2), (256, 512, 2)]
        self.convs = nn.ModuleList([gnn.Conv2d(ci, co, 3, stride=s, pad=(1, 1, 1, 1)) for ci, co, s in chans])
        self.norms = nn.ModuleList([gnn.GroupNorm(32, co, 1e-5) for _, co, _ in chans])
        self.head = gnn.Linear(512, dims)
        torch.random.set_rng_state(rng)
        self.dims, self.seed = dims, seed

    @torch.no_grad()
    def forward(self, images_nchw01):
        x = ops.nchw_to_nhwc_raw((images_nchw01.float() * 2 - 1).contiguous())
        for conv, norm in zip(self.convs, self.norms):
            x = norm(conv(x), silu=True)
        b, h, w, c = x.shape
        pooled = ops.colsum_raw(x.view(b * h * w, c), segments=b) / float(h * w)
        return self.head(pooled)


def extractor_tag(net) -> str:
    """What produced the features behind a score row.  The reference's rows come from InceptionV3 / VGG16 / BLIP with
    URL-fetched weights (fid_score.py:28, precision_recall.py:31, diversity_score.py:89); rows written under the seeded
    stand-in must never be mistaken for them, so every row carries this tag as `feature_extractor`."""
    return getattr(net, "tag", f"standin-seed{getattr(net, 'seed', '?')}-d{getattr(net, 'dims', '?')}")


class ScriptedExtractor(nn.Module):
    """A real extractor supplied as a TorchScript file ([B,3,H,W] in [0,1] -> [B,dims]; e.g. pytorch_fid's pool3 trunk
    scripted where its weights exist): `GAD_FEATURE_NET_TS=/path/extractor.pt`.  Runs with stock torch ops - the score
    tail is ~1 % of a coalition and off the hand-written path."""

    def __init__(self, path, device):
        super().__init__()
        self.mod = torch.jit.load(path, map_location=device).eval()
        self.tag = file_tag("torchscript", path)
        with torch.no_grad():
            self.dims = int(self.mod(torch.zeros(1, 3, 32, 32, device=device)).shape[1])

    @torch.no_grad()
    def forward(self, images_nchw01):
        return self.mod(images_nchw01.float()).float()


# Which network runs for a score: role -> (weights variable, switch variable, its one value, builder from a file, builder
# seeded).  A weights file wins over the switch (the same architecture with seeded weights: what the true tail costs, not what
# it scores); any other value of the switch is refused; with neither set the role has no network of its own.
ROLES = {
    # pytorch-fid's InceptionV3 state dict (reference fid_score.py), gad/inception.py
    "fid": ("GAD_INCEPTION_FID_WEIGHTS", "GAD_FEATURE_NET", "inception-seeded",
            lambda path: InceptionV3.from_file(path, "fid"), lambda seed: InceptionV3.seeded("fid", seed)),
    # torchvision's `inception_v3` state dict (reference inception_score.py); unset: `is` from the feature extractor's first 1000 dims
    "is": ("GAD_INCEPTION_IS_WEIGHTS", None, None, lambda path: InceptionV3.from_file(path, "torchvision"), None),
    # torchvision's `vgg16` state dict (reference precision_recall.py: VGG16 fc features), gad/vgg.py; unset: P/R from the feature extractor
    "pr": ("GAD_VGG16_WEIGHTS", "GAD_PR_NET", "vgg16-seeded", lambda path: VGG16.from_file(path), lambda seed: VGG16.seeded(seed)),
    # a state dict of `BlipForQuestionAnswering` or of its `vision_model` (reference diversity_score.py:89-120: the BLIP-VQA
    # vision tower's `pooler_output`), gad/vit.py
    "diversity": ("GAD_BLIP_VISION_WEIGHTS", "GAD_DIVERSITY_NET", "blip-seeded",
                  lambda path: VisionTower.from_file(path, "blip_vqa_base"), lambda seed: VisionTower.seeded("blip_vqa_base", seed)),
}


def _settings(role):
    """the role's environment, read once: (weights file, switch value), for "fid" also `GAD_FEATURE_NET_TS`"""
    names = ROLES[role][:2] + (("GAD_FEATURE_NET_TS",) if role == "fid" else ())
    return tuple(os.environ.get(n) if n else None for n in names)


def _build(role, device, settings, seed=1234):
    """`ROLES`' precedence on `settings` -> the network on `device`, or None with nothing set.  `GAD_FEATURE_NET_TS` (a
    TorchScript file, stock torch ops) wins for "fid"."""
    _, switch, value, from_file, seeded = ROLES[role]
    weights, kind, *ts = settings
    if ts and ts[0] and os.path.exists(ts[0]):
        return ScriptedExtractor(ts[0], device)
    if weights:
        return from_file(weights).to(device)
    if kind and kind == value:
        return seeded(seed).to(device)
    if kind:
        raise ValueError(f"{switch}={kind!r}: the only value is {value!r}")
    return None


_REF_STATS = {}


def net_key(role):
    """where `resolve` keeps the role's network under the environment as it stands"""
    return ("net", role) + _settings(role)


def resolve(role, device, standin=None):
    """The role's network, built once per process and setting.  With nothing set: `standin()`, kept likewise, or None -
    and then nothing is looked up or stored."""
    settings = _settings(role)
    key = ("net", role) + settings
    if key not in _REF_STATS:
        net = _build(role, device, settings)
        if net is None:
            if standin is None:
                return None
            net = standin()
        _REF_STATS[key] = net
    return _REF_STATS[key]


def default_extractor(dims, device, seed=1234):
    """The network behind `fid_value` (role "fid"), built afresh; with nothing set, the seeded stand-in."""
    net = _build("fid", device, _settings("fid"), seed)
    return FeatureNet(dims, seed=seed).to(device) if net is None else net


def is_extractor(device):
    """The classifier behind `is` (role "is"); None: `is` comes from the feature extractor's first 1000 dims, as before."""
    return _build("is", device, _settings("is"))


def pr_extractor(device):
    """The network behind `precision` / `recall` (role "pr"); None: P/R come from the feature extractor, as before."""
    return _build("pr", device, _settings("pr"))


def diversity_extractor(device):
    """The network behind the CelebA diversity score (role "diversity"); None: the seeded stand-in, as before."""
    return _build("diversity", device, _settings("diversity"))


from src.attributions.global_scores.fid_score import (calculate_frechet_distance as frechet_distance,  # noqa: E402,F401
                                                      compute_features_stats as feature_stats)


def feature_stats_torch(features: torch.Tensor):
    """float64 mean / unbiased covariance on the tensor's device (np.mean / np.cov(rowvar=False) semantics)."""
    f = features.double()
    mu = f.mean(dim=0)
    d = f - mu
    return mu, d.T @ d / (f.shape[0] - 1)


def frechet_distance_torch(mu1, sigma1, mu2, sigma2):
    """Same quantity as frechet_distance without the host sqrtm: Tr sqrt(S1 S2) = sum sqrt(eig(S1^1/2 S2 S1^1/2)),
    two symmetric float64 eigendecompositions on the tensors' device (the score-tail-on-device step of SURVEY
    section 8f-2; agrees with scipy's sqrtm route to ~1e-9 relative on well-conditioned inputs)."""
    diff = mu1 - mu2
    w, v = torch.linalg.eigh(sigma1)
    root1 = (v * w.clamp_min(0).sqrt()) @ v.T
    inner = root1 @ sigma2 @ root1
    ev = torch.linalg.eigvalsh((inner + inner.T) / 2).clamp_min(0)
    return float(diff @ diff + torch.trace(sigma1) + torch.trace(sigma2) - 2 * ev.sqrt().sum())


def compute_features(net: FeatureNet, images: torch.Tensor, batch_size: int, device) -> np.ndarray:
    """images [N,3,H,W] float in [0,1] (host or device) -> float64 [N, dims] (fid_score.py:74-102)."""
    out = np.empty((len(images), net.dims))
    for s in range(0, len(images), batch_size):
        f = net(images[s:s + batch_size].to(device))
        out[s:s + f.shape[0]] = f.double().cpu().numpy()
    return out


def compute_features_torch(net: FeatureNet, images: torch.Tensor, batch_size: int, device) -> torch.Tensor:
    """Like compute_features but the [N, dims] fp32 feature matrix stays in HBM."""
    return torch.cat([net(images[s:s + batch_size].to(device)) for s in range(0, len(images), batch_size)], 0)


def _fid_net(feature_dims, device):
    """role "fid", with the seeded stand-in where nothing is set: one extractor for every score of this process"""
    return resolve("fid", device, lambda: FeatureNet(feature_dims).to(device))


def _reference_features(dataset, device, batch_size, *nets, features=compute_features_torch):
    """the training set mapped to [0,1] - one copy of it - through each of `nets` -> their feature matrices"""
    ref = dataset.device_tensor(device).add_(1).div_(2)
    return [features(net, ref, max(batch_size, 256), device) for net in nets]


def fid_against_dataset(images01, dataset, device, batch_size=512, feature_dims=2048):
    """calculate_fid (fid_score.py:23-71) with the training set as the reference distribution (its
    mu/sigma play the role of the precomputed stats.pkl, :42-58; cached per dataset object)."""
    net = _fid_net(feature_dims, device)
    key = id(dataset)
    if key not in _REF_STATS:
        _REF_STATS[key] = feature_stats(*_reference_features(dataset, device, batch_size, net, features=compute_features))
    mu, sigma = feature_stats(compute_features(net, images01, max(batch_size, 256), device))
    return frechet_distance(mu, sigma, *_REF_STATS[key])


def _pr_reference(pr_net, net, dataset, device, batch_size, nhood_size):
    """The reference side with a P/R network, under a key of its own: the extractor's moments and the device manifold of
    `pr_net`'s fp16 features, both from one copy of the dataset (the extractor's own manifold is not built) -> that key."""
    from src.attributions.global_scores.precision_recall import make_manifold_device
    key = ("dev-pr", id(dataset), pr_net.tag, nhood_size)
    if key not in _REF_STATS:
        ref_f, ref_pr = _reference_features(dataset, device, batch_size, net, pr_net)
        _REF_STATS[key] = (feature_stats_torch(ref_f), make_manifold_device(ref_pr, nhood_size))
    return key


def global_scores_against_dataset(images01, dataset, device, batch_size=512, feature_dims=2048, nhood_size=3):
    """All four global behaviours unlearn.py writes for the CIFAR family (:807-837): fid_value, is, precision,
    recall - with the seeded stand-in extractor in place of Inception / VGG16 (URL-fetched weights):
    IS uses the softmax of the first 1000 feature dims as class probabilities, P/R the fp16 features
    (of the network `pr_extractor` names, where it names one: the row's tag then ends in `;pr=<tag>`).
    Features, float64 moments, the Frechet eigendecompositions and the P/R distance tiles all stay on the
    device; only the four scalars come back to the host."""
    from src.attributions.global_scores.inception_score import inception_score_from_probs
    from src.attributions.global_scores.precision_recall import calc_pr, make_manifold
    net = _fid_net(feature_dims, device)
    pr_net = resolve("pr", device)
    key = ("dev", id(dataset))
    if pr_net is not None:
        key = _pr_reference(pr_net, net, dataset, device, batch_size, nhood_size)
    if key not in _REF_STATS:
        (ref_f,) = _reference_features(dataset, device, batch_size, net)
        _REF_STATS[key] = (feature_stats_torch(ref_f), make_manifold(ref_f, nhood_size, 10000, 10000, device))
    (mu_r, sig_r), m_ref = _REF_STATS[key]
    gen_f = compute_features_torch(net, images01, max(batch_size, 256), device)
    mu, sig = feature_stats_torch(gen_f)
    fid = frechet_distance_torch(mu, sig, mu_r, sig_r)
    tag = extractor_tag(net)
    is_net = resolve("is", device)
    if is_net is None:
        probs = torch.softmax(gen_f[:, :1000].double(), dim=1).cpu().numpy()
    else:                    # the 1000 logits of torchvision's InceptionV3; the row says that `is` has a source of its own
        logits = torch.cat([is_net.logits(is_net(images01[s:s + batch_size].to(device))) for s in range(0, len(images01), batch_size)], 0)
        probs = torch.softmax(logits.double(), dim=1).cpu().numpy()
        tag = f"{tag};is={extractor_tag(is_net)}"
    is_value = inception_score_from_probs(probs)
    if pr_net is None:
        precision, recall = calc_pr(make_manifold(gen_f, nhood_size, 10000, 10000, device), m_ref, 10000, 10000, device)
    else:                    # VGG16 fc features, fp16 on the device; radii and coverage by the fused kernel (csrc/manifold.hip)
        from src.attributions.global_scores.precision_recall import calc_pr_device, make_manifold_device
        m_gen = make_manifold_device(compute_features_torch(pr_net, images01, max(batch_size, 256), device), nhood_size)
        precision, recall = calc_pr_device(m_gen, m_ref)
        tag = f"{tag};pr={extractor_tag(pr_net)}"
    return {"fid_value": fid, "is": is_value, "precision": precision, "recall": recall,
            "feature_extractor": tag}


def diversity_against_dataset(images01, dataset, device, num_cluster=20, batch_size=256, feature_dims=768, max_ref=2000,
                              decode=None):
    """The CelebA global behaviour unlearn.py writes (:787-803): entropy / cluster_count / cluster_proportions of
    calculate_diversity_score (diversity_score.py:82-188) - Ward clusters of the reference embeddings, generated samples
    assigned to the nearest cluster mean, log2 entropy of the proportions.  The BLIP-VQA vision tower (hub-fetched, :89-90)
    is replaced by the seeded stand-in extractor unless `diversity_extractor` names the real one; the reference set ({OUTDIR}/celeba/cluster_imgs there) is the training
    set itself (its first `max_ref` items), mapped to [0,1] like the pipeline output.  Embeddings are computed on the
    device; the Ward linkage stays scipy on the host, as in the reference.
    `decode` (a pipeline's `decoder`: latents [N,C,h,w] -> [N,3,H,W] in [0,1], with a `tag`): `images01` are decoded samples,
    so the reference latents are decoded the same way before they are embedded, and the row's tag gains `;dec=<tag>`."""
    from src.attributions.global_scores.diversity_score import diversity_from_embeddings
    net = resolve("diversity", device, lambda: FeatureNet(feature_dims, seed=4321).to(device))
    standin = isinstance(net, FeatureNet)

    def embed(images):       # the tower: the raw `pooler_output` in fp64, NOT normalised - what diversity_score.py:119-123 clusters
        f = compute_features_torch(net, images, batch_size, device).double()
        return (torch.nn.functional.normalize(f, dim=1) if standin else f).cpu().numpy()
    rkey = ("div_ref", id(dataset)) if standin else ("div_ref", id(dataset), net.tag)
    if decode is not None:
        rkey = (*rkey, "dec", decode.tag)
    if rkey not in _REF_STATS:
        idx = list(range(min(len(dataset), max_ref)))
        ref = dataset.device_tensor(device, idx)
        _REF_STATS[rkey] = embed(ref.add(1).div(2).clamp(0, 1) if decode is None else decode(ref))
    entropy, cluster_count, proportions, _, _ = diversity_from_embeddings(_REF_STATS[rkey], embed(images01.to(device)), num_cluster)
    return {"entropy": entropy, "cluster_count": cluster_count, "cluster_proportions": proportions,
            "feature_extractor": extractor_tag(net) if decode is None else f"{extractor_tag(net)};dec={decode.tag}"}
