"""InceptionV3 for the score tail: pool3 features for FID (reference src/attributions/global_scores/fid_score.py:23-107,
pytorch-fid's InceptionV3 with `pt_inception-2015-12-05-6726825d.pth`) and the 1000 logits for the Inception score
(inception_score.py, torchvision's `inception_v3`), on the HIP operators.

Eval only.  Every BasicConv2d (conv without bias -> BatchNorm eps=1e-3 -> ReLU) is one `gad_gemm` launch on weights with
the BatchNorm folded in (fp64, once, at load time) plus a `gad_relu` pass; the last convolution of every branch writes its
channel slice of the block output in place (ldc > N), the pool branches land there through `gad_pool2d`, and ONE ReLU pass
covers the whole concatenated block.  Activations are fp32 NHWC throughout.

Parameter names follow torchvision's grammar (`Conv2d_1a_3x3.conv.weight`, `Mixed_6a.branch3x3dbl_3.bn.running_var`,
`fc.weight`), so both published state dicts load as they are; `AuxLogits.*` and `*.num_batches_tracked` are ignored.

variant "fid": pytorch-fid's blocks - averages that exclude the padding in Mixed_5b..5d, 6b..6e and 7b, a 3/1/1 MAX pool in
Mixed_7c, a 1008-way fc.  variant "torchvision": averages that count the padding, 1000-way fc, transform_input=False."""
from __future__ import annotations

import math

import torch

from . import ops
from ._capi import POOL_AVG, POOL_AVG_VALID, POOL_MAX
from .extractor import Extractor, check_state_dict, file_tag, load_checkpoint

BN_EPS = 1e-3
VARIANTS = {"fid": 1008, "torchvision": 1000}       # variant -> fc outputs
RESIZE = 299


def _a(p, cin, pf):
    return [(f"{p}.branch1x1", cin, 64, 1, 1, 1, 0, 0), (f"{p}.branch5x5_1", cin, 48, 1, 1, 1, 0, 0),
            (f"{p}.branch5x5_2", 48, 64, 5, 5, 1, 2, 2), (f"{p}.branch3x3dbl_1", cin, 64, 1, 1, 1, 0, 0),
            (f"{p}.branch3x3dbl_2", 64, 96, 3, 3, 1, 1, 1), (f"{p}.branch3x3dbl_3", 96, 96, 3, 3, 1, 1, 1),
            (f"{p}.branch_pool", cin, pf, 1, 1, 1, 0, 0)]


def _c(p, c7):
    return [(f"{p}.branch1x1", 768, 192, 1, 1, 1, 0, 0), (f"{p}.branch7x7_1", 768, c7, 1, 1, 1, 0, 0),
            (f"{p}.branch7x7_2", c7, c7, 1, 7, 1, 0, 3), (f"{p}.branch7x7_3", c7, 192, 7, 1, 1, 3, 0),
            (f"{p}.branch7x7dbl_1", 768, c7, 1, 1, 1, 0, 0), (f"{p}.branch7x7dbl_2", c7, c7, 7, 1, 1, 3, 0),
            (f"{p}.branch7x7dbl_3", c7, c7, 1, 7, 1, 0, 3), (f"{p}.branch7x7dbl_4", c7, c7, 7, 1, 1, 3, 0),
            (f"{p}.branch7x7dbl_5", c7, 192, 1, 7, 1, 0, 3), (f"{p}.branch_pool", 768, 192, 1, 1, 1, 0, 0)]


def _e(p, cin):
    return [(f"{p}.branch1x1", cin, 320, 1, 1, 1, 0, 0), (f"{p}.branch3x3_1", cin, 384, 1, 1, 1, 0, 0),
            (f"{p}.branch3x3_2a", 384, 384, 1, 3, 1, 0, 1), (f"{p}.branch3x3_2b", 384, 384, 3, 1, 1, 1, 0),
            (f"{p}.branch3x3dbl_1", cin, 448, 1, 1, 1, 0, 0), (f"{p}.branch3x3dbl_2", 448, 384, 3, 3, 1, 1, 1),
            (f"{p}.branch3x3dbl_3a", 384, 384, 1, 3, 1, 0, 1), (f"{p}.branch3x3dbl_3b", 384, 384, 3, 1, 1, 1, 0),
            (f"{p}.branch_pool", cin, 192, 1, 1, 1, 0, 0)]


# every BasicConv2d of the trunk, in torchvision's module order: (name, Cin, Cout, KH, KW, stride, pad_h, pad_w)
CONVS = (
    [("Conv2d_1a_3x3", 3, 32, 3, 3, 2, 0, 0), ("Conv2d_2a_3x3", 32, 32, 3, 3, 1, 0, 0), ("Conv2d_2b_3x3", 32, 64, 3, 3, 1, 1, 1),
     ("Conv2d_3b_1x1", 64, 80, 1, 1, 1, 0, 0), ("Conv2d_4a_3x3", 80, 192, 3, 3, 1, 0, 0)]
    + _a("Mixed_5b", 192, 32) + _a("Mixed_5c", 256, 64) + _a("Mixed_5d", 288, 64)
    + [("Mixed_6a.branch3x3", 288, 384, 3, 3, 2, 0, 0), ("Mixed_6a.branch3x3dbl_1", 288, 64, 1, 1, 1, 0, 0),
       ("Mixed_6a.branch3x3dbl_2", 64, 96, 3, 3, 1, 1, 1), ("Mixed_6a.branch3x3dbl_3", 96, 96, 3, 3, 2, 0, 0)]
    + _c("Mixed_6b", 128) + _c("Mixed_6c", 160) + _c("Mixed_6d", 160) + _c("Mixed_6e", 192)
    + [("Mixed_7a.branch3x3_1", 768, 192, 1, 1, 1, 0, 0), ("Mixed_7a.branch3x3_2", 192, 320, 3, 3, 2, 0, 0),
       ("Mixed_7a.branch7x7x3_1", 768, 192, 1, 1, 1, 0, 0), ("Mixed_7a.branch7x7x3_2", 192, 192, 1, 7, 1, 0, 3),
       ("Mixed_7a.branch7x7x3_3", 192, 192, 7, 1, 1, 3, 0), ("Mixed_7a.branch7x7x3_4", 192, 192, 3, 3, 2, 0, 0)]
    + _e("Mixed_7b", 1280) + _e("Mixed_7c", 2048))
_SPEC = {c[0]: c[1:] for c in CONVS}
BN_KEYS = ("weight", "bias", "running_mean", "running_var")


def expected_shapes(variant):
    """{state-dict key: shape} of everything `load_state_dict` reads (torchvision's names)."""
    ncls = VARIANTS[variant]
    out = {}
    for name, ci, co, kh, kw, _, _, _ in CONVS:
        out[f"{name}.conv.weight"] = (co, ci, kh, kw)
        for k in BN_KEYS:
            out[f"{name}.bn.{k}"] = (co,)
    out["fc.weight"], out["fc.bias"] = (ncls, 2048), (ncls,)
    return out


def param_count(variant=None):
    """Trainable parameters (conv weights, BatchNorm gamma / beta; with `variant`, the fc as well) - running statistics are
    buffers, as torchvision counts."""
    n = sum(co * ci * kh * kw + 2 * co for _, ci, co, kh, kw, _, _, _ in CONVS)
    return n + (VARIANTS[variant] * 2049 if variant else 0)


def fold_bn(weight, gamma, beta, mean, var, eps=BN_EPS):
    """conv (no bias) -> eval BatchNorm as one conv: fp64 w' = w * gamma / sqrt(var + eps), b' = beta - mean * gamma /
    sqrt(var + eps), each rounded to fp32 once -> ([Cout][KH][KW][Cin] fp32, [Cout] fp32)."""
    s = gamma.double() / torch.sqrt(var.double() + eps)
    w = weight.double() * s[:, None, None, None]
    b = beta.double() - mean.double() * s
    return w.permute(0, 2, 3, 1).contiguous().float(), b.float()


def seeded_state_dict(variant, seed):
    """He-normal conv weights (std sqrt(2 / fan_in): the activation scale survives the 48 layers), BatchNorm gamma 1, beta 0,
    running mean 0 / var 1; fc N(0, 1 / 2048), zero bias."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for key, shape in expected_shapes(variant).items():
        if key.endswith("conv.weight"):
            sd[key] = torch.randn(shape, generator=g) * math.sqrt(2.0 / (shape[1] * shape[2] * shape[3]))
        elif key == "fc.weight":
            sd[key] = torch.randn(shape, generator=g) / math.sqrt(shape[1])
        elif key.endswith("bn.weight") or key.endswith("running_var"):
            sd[key] = torch.ones(shape)
        else:
            sd[key] = torch.zeros(shape)
    return sd


class InceptionV3(Extractor):
    """[B,3,H,W] in [0,1] -> pool3 [B,2048] (`forward`); `logits(pool3)` -> [B, 1008 | 1000]."""

    owner = "InceptionV3"
    dims = 2048
    max_batch = 64           # images per pass through the trunk (the 147 x 147 x 64 map of 64 images is 354 MB)

    def __init__(self, variant="fid", state_dict=None, tag=None):
        if variant not in VARIANTS:
            raise ValueError(f"InceptionV3 variant {variant!r}: use 'fid' or 'torchvision'")
        self.variant = variant
        self.avg = POOL_AVG_VALID if variant == "fid" else POOL_AVG
        super().__init__(tag or f"inception-{variant}-unloaded", state_dict)

    @classmethod
    def seeded(cls, variant="fid", seed=1234):
        return cls(variant, seeded_state_dict(variant, seed), tag=f"inception-{variant}-seeded{seed}")

    @classmethod
    def from_file(cls, path, variant):
        return cls(variant, load_checkpoint(path), tag=file_tag(f"inception-{variant}", path, basename=False))

    def load_state_dict(self, sd):
        check_state_dict(f"InceptionV3({self.variant})", sd, expected_shapes(self.variant),
                         extra=lambda k: k.startswith("AuxLogits.") or k.endswith("num_batches_tracked"))
        self.w = {name: fold_bn(sd[f"{name}.conv.weight"], *(sd[f"{name}.bn.{k}"] for k in BN_KEYS)) for name in _SPEC}
        self.w["fc"] = (sd["fc.weight"].detach().float().contiguous(), sd["fc.bias"].detach().float().contiguous())
        return self

    # ---- launches ----
    def _conv(self, x, name, out=None, c0=0, relu=True):
        """BasicConv2d `name` of x [B,H,W,Cin]; into channels [c0, c0 + Cout) of `out` [B,Ho,Wo,Ctot] if given (no ReLU: the
        block's one pass does it), else into a tensor of its own (ReLU'd unless relu=False)."""
        _, _, kh, kw, stride, ph, pw = _SPEC[name]
        y = ops.conv_krsc_raw(x, *self.w[name], kh, kw, stride, ph, pw, out, c0)
        return ops.relu_raw(y) if out is None and relu else y

    def _maxpool(self, x, relu_in):
        Bn, H, W, Cn = x.shape
        out = torch.empty((Bn, (H - 3) // 2 + 1, (W - 3) // 2 + 1, Cn), device=x.device, dtype=torch.float32)
        return ops.pool2d_raw(x, out, 0, 3, 2, 0, POOL_MAX, relu_in)

    def _block(self, x, ctot, stride=1):
        Bn, H, W, _ = x.shape
        Ho, Wo = ((H - 3) // 2 + 1, (W - 3) // 2 + 1) if stride == 2 else (H, W)
        return torch.empty((Bn, Ho, Wo, ctot), device=x.device, dtype=torch.float32)

    def _pool_branch(self, x, p, y, c0, mode=None):
        t = ops.pool2d_raw(x, torch.empty_like(x), 0, 3, 1, 1, self.avg if mode is None else mode)
        self._conv(t, f"{p}.branch_pool", y, c0)

    def mixed_a(self, x, p):
        pf = _SPEC[f"{p}.branch_pool"][1]
        y = self._block(x, 224 + pf)
        self._conv(x, f"{p}.branch1x1", y, 0)
        self._conv(self._conv(x, f"{p}.branch5x5_1"), f"{p}.branch5x5_2", y, 64)
        t = self._conv(self._conv(x, f"{p}.branch3x3dbl_1"), f"{p}.branch3x3dbl_2")
        self._conv(t, f"{p}.branch3x3dbl_3", y, 128)
        self._pool_branch(x, p, y, 224)
        return ops.relu_raw(y)

    def mixed_6a(self, x, p="Mixed_6a"):
        y = self._block(x, 768, 2)
        self._conv(x, f"{p}.branch3x3", y, 0)
        t = self._conv(self._conv(x, f"{p}.branch3x3dbl_1"), f"{p}.branch3x3dbl_2")
        self._conv(t, f"{p}.branch3x3dbl_3", y, 384)
        ops.pool2d_raw(x, y, 480, 3, 2, 0, POOL_MAX)
        return ops.relu_raw(y)

    def mixed_c(self, x, p):
        y = self._block(x, 768)
        self._conv(x, f"{p}.branch1x1", y, 0)
        t = self._conv(self._conv(x, f"{p}.branch7x7_1"), f"{p}.branch7x7_2")
        self._conv(t, f"{p}.branch7x7_3", y, 192)
        t = self._conv(x, f"{p}.branch7x7dbl_1")
        for i in (2, 3, 4):
            t = self._conv(t, f"{p}.branch7x7dbl_{i}")
        self._conv(t, f"{p}.branch7x7dbl_5", y, 384)
        self._pool_branch(x, p, y, 576)
        return ops.relu_raw(y)

    def mixed_7a(self, x, p="Mixed_7a"):
        y = self._block(x, 1280, 2)
        self._conv(self._conv(x, f"{p}.branch3x3_1"), f"{p}.branch3x3_2", y, 0)
        t = self._conv(x, f"{p}.branch7x7x3_1")
        for i in (2, 3):
            t = self._conv(t, f"{p}.branch7x7x3_{i}")
        self._conv(t, f"{p}.branch7x7x3_4", y, 320)
        ops.pool2d_raw(x, y, 512, 3, 2, 0, POOL_MAX)
        return ops.relu_raw(y)

    def mixed_e(self, x, p):
        y = self._block(x, 2048)
        self._conv(x, f"{p}.branch1x1", y, 0)
        t = self._conv(x, f"{p}.branch3x3_1")
        self._conv(t, f"{p}.branch3x3_2a", y, 320)
        self._conv(t, f"{p}.branch3x3_2b", y, 704)
        t = self._conv(self._conv(x, f"{p}.branch3x3dbl_1"), f"{p}.branch3x3dbl_2")
        self._conv(t, f"{p}.branch3x3dbl_3a", y, 1088)
        self._conv(t, f"{p}.branch3x3dbl_3b", y, 1472)
        # pytorch-fid's last block pools with a MAX (FIDInceptionE_2), the one before with the padding-excluding average
        self._pool_branch(x, p, y, 1856, POOL_MAX if (self.variant == "fid" and p == "Mixed_7c") else None)
        return ops.relu_raw(y)

    def preprocess(self, images_nchw01):
        """[B,3,H,W] in [0,1] -> NHWC [B,299,299,3] in [-1,1]: bilinear resize (align_corners=False) and 2x - 1 in one pass;
        a 299 x 299 input passes through the same kernel as an exact copy."""
        return ops.resize_bilinear_raw(ops._req(images_nchw01.float().contiguous(), "inception input"), RESIZE, 2.0, -1.0)

    def trunk(self, x):
        """NHWC [B,299,299,3] in [-1,1] -> the Mixed_7c map [B,8,8,2048]"""
        x = self._conv(self._conv(x, "Conv2d_1a_3x3"), "Conv2d_2a_3x3")
        x = self._maxpool(self._conv(x, "Conv2d_2b_3x3", relu=False), relu_in=True)      # max-pool commutes with the ReLU
        x = self._conv(x, "Conv2d_3b_1x1")
        x = self._maxpool(self._conv(x, "Conv2d_4a_3x3", relu=False), relu_in=True)
        for p in ("Mixed_5b", "Mixed_5c", "Mixed_5d"):
            x = self.mixed_a(x, p)
        x = self.mixed_6a(x)
        for p in ("Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e"):
            x = self.mixed_c(x, p)
        x = self.mixed_7a(x)
        return self.mixed_e(self.mixed_e(x, "Mixed_7b"), "Mixed_7c")

    def _chunk(self, images_nchw01):
        x = self.trunk(self.preprocess(images_nchw01))
        b, h, w, c = x.shape
        return ops.colsum_raw(x.view(b * h * w, c), segments=b) / float(h * w)

    @torch.no_grad()
    def logits(self, pool3):
        w, b = self.w["fc"]
        return ops.linear_fwd_raw(ops._req(pool3.contiguous(), "inception pool3"), w, b, force_f32=True)
