"""VGG16 for the precision / recall manifolds (reference src/attributions/global_scores/precision_recall.py, Kynkaanniemi et
al.: both manifolds are built from the 4096 outputs of VGG16's second fully connected layer), on the HIP operators - but for
one elementwise torch op on the 3-channel input, the mean subtraction in `preprocess`.

Eval only.  torchvision's `vgg16`: thirteen 3x3 convolutions (pad 1, bias, ReLU) at widths 64, 64, 128, 128, 256 x 3, 512 x 3,
512 x 3 with a 2x2 stride-2 max pool after the 2nd, 4th, 7th, 10th and 13th, then `classifier.0` 25088 -> 4096 + ReLU and
`classifier.3` 4096 -> 4096 + ReLU, whose outputs are the features; no dropout, no `classifier.6`.  Every convolution and both
Linears are one `gad_gemm` launch (the convolutions on the direct route: no Winograd weight is passed) plus a `gad_relu` pass; the ReLU in
front of a pool is the pool's own (`relu_in`: max commutes with it).  Activations are fp32 NHWC throughout.

State-dict keys are torchvision's (`features.N.weight/bias`, `classifier.0/3.weight/bias`); extra keys (`classifier.6.*`) are
ignored, missing keys and wrong shapes are refused by name.

Preprocessing convention: [B,3,H,W] in [0,1] is resized bilinearly (align_corners=False, `gad_resize_bilinear`) to
`resolution` and normalised with ImageNet's mean / std.  The 1 / std scale is folded into the first convolution's weights at
load time (fp64, rounded once), as BatchNorm is folded in inception.py.  The mean is subtracted from the 3-channel input in
front of the resize instead (the resize's weights sum to one, so the two commute): torchvision pads the NORMALISED image with
zeros, and a mean folded into the bias would be wrong along that border.  NVIDIA's TorchScript `vgg16.pt` (the reference's
extractor) cannot be fetched and its exact preprocessing is NOT claimed here; the row tag says which network ran.

fc1's columns: `classifier.0.weight` expects the (c, h, w) order of an NCHW flatten, the activations here are NHWC, so the
columns are permuted once at load.  `resolution` 224 ends in a 7 x 7 map (AdaptiveAvgPool2d(7) is the identity); `resolution`
32 ends in a 1 x 1 map, which AdaptiveAvgPool2d(7) replicates 49 times - the 49 column groups of `classifier.0.weight` are
summed at load (fp64) and fc1 contracts over 512.  Other resolutions are refused."""
from __future__ import annotations

import math

import torch

from . import _capi, ops
from ._capi import POOL_MAX
from .extractor import Extractor, check_state_dict, file_tag, load_checkpoint

# torchvision's cfg "D": (index in `features`, Cin, Cout) of every convolution, and the convolutions a max pool follows
CONVS = [(0, 3, 64), (2, 64, 64), (5, 64, 128), (7, 128, 128), (10, 128, 256), (12, 256, 256), (14, 256, 256),
         (17, 256, 512), (19, 512, 512), (21, 512, 512), (24, 512, 512), (26, 512, 512), (28, 512, 512)]
POOL_AFTER = {2, 7, 14, 21, 28}
FC_IN, FC = 512 * 7 * 7, 4096
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
RESOLUTIONS = {224: 7, 32: 1}            # resolution -> side of the final map


def expected_shapes():
    """{state-dict key: shape} of everything `load_state_dict` reads (torchvision's names)."""
    out = {}
    for idx, ci, co in CONVS:
        out[f"features.{idx}.weight"], out[f"features.{idx}.bias"] = (co, ci, 3, 3), (co,)
    out["classifier.0.weight"], out["classifier.0.bias"] = (FC, FC_IN), (FC,)
    out["classifier.3.weight"], out["classifier.3.bias"] = (FC, FC), (FC,)
    return out


def seeded_state_dict(seed):
    """He-normal weights (std sqrt(2 / fan_in): the activation scale survives the 15 layers), biases N(0, 0.1^2)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for key, shape in expected_shapes().items():
        if key.endswith("weight"):
            sd[key] = torch.randn(shape, generator=g) * math.sqrt(2.0 / math.prod(shape[1:]))
        else:
            sd[key] = torch.randn(shape, generator=g) * 0.1
    return sd


def fold_fc1(weight, side):
    """`classifier.0.weight` [4096][512 * 49 in (c, h, w) order] -> the matrix fc1 multiplies the NHWC-flattened final map by:
    side 7: columns permuted to (h, w, c); side 1: the 49 columns of each channel summed in fp64 (AdaptiveAvgPool2d(7) of a
    1 x 1 map is 49 copies) -> [4096][512]."""
    w = weight.detach().reshape(weight.shape[0], -1, 7, 7)
    if side == 7:
        return w.permute(0, 2, 3, 1).reshape(weight.shape[0], -1).float().contiguous()
    if side == 1:
        return w.double().sum(dim=(2, 3)).float().contiguous()
    raise ValueError(f"VGG16: a final map of {side} x {side} is not supported (7 or 1)")


class VGG16(Extractor):
    """[B,3,H,W] in [0,1] -> fc2 features [B,4096] (`forward`)."""

    owner = "VGG16"
    dims = FC

    def __init__(self, state_dict=None, tag=None, resolution=224):
        if resolution not in RESOLUTIONS:
            raise ValueError(f"VGG16: resolution {resolution} is not supported: use 224 (7 x 7 final map) or 32 (1 x 1, the 49 "
                             "replicas AdaptiveAvgPool2d(7) makes of it folded into fc1)")
        self.resolution, self.side = resolution, RESOLUTIONS[resolution]
        self.max_batch = 16 if resolution == 224 else 1024     # the 224 x 224 x 64 maps of 16 images are 2 x 205 MB
        self.mean = torch.tensor(MEAN, dtype=torch.float32).view(1, 3, 1, 1)
        super().__init__(tag or "vgg16-unloaded", state_dict)

    @classmethod
    def seeded(cls, seed=1234, resolution=224):
        return cls(seeded_state_dict(seed), tag=f"vgg16-seeded{seed}", resolution=resolution)

    @classmethod
    def from_file(cls, path, resolution=224):
        return cls(load_checkpoint(path), tag=file_tag("vgg16", path), resolution=resolution)

    def load_state_dict(self, sd):
        check_state_dict("VGG16", sd, expected_shapes())
        self.w = {}
        for idx, ci, _ in CONVS:
            w = sd[f"features.{idx}.weight"].detach()
            if idx == 0:           # (x - mean) / std: the scale goes into the weights
                w = (w.double() / torch.tensor(STD, dtype=torch.float64).view(1, 3, 1, 1)).float()
            self.w[idx] = (w.float().permute(0, 2, 3, 1).contiguous(), sd[f"features.{idx}.bias"].detach().float().contiguous())
        self.w["fc1"] = (fold_fc1(sd["classifier.0.weight"], self.side), sd["classifier.0.bias"].detach().float().contiguous())
        self.w["fc2"] = (sd["classifier.3.weight"].detach().float().contiguous(), sd["classifier.3.bias"].detach().float().contiguous())
        return self

    def to(self, device):
        self.mean = self.mean.to(device)
        return super().to(device)

    # ---- launches ----
    def _maxpool_relu(self, x):
        Bn, H, W, Cn = x.shape
        out = torch.empty((Bn, H // 2, W // 2, Cn), device=x.device, dtype=torch.float32)
        return ops.pool2d_raw(x, out, 0, 2, 2, 0, POOL_MAX, relu_in=True)

    def preprocess(self, images_nchw01):
        """[B,3,H,W] in [0,1] -> NHWC [B,R,R,3] = resize(x) - mean (the 1 / std scale lives in the first convolution)"""
        x = ops._req((images_nchw01.float() - self.mean).contiguous(), "vgg16 input")
        if x.shape[1] != 3:
            raise _capi.GadError(f"VGG16: expected 3 channels, got {x.shape[1]}")
        return ops.resize_bilinear_raw(x, self.resolution, 1.0, 0.0)

    def _chunk(self, images_nchw01):
        x = self.preprocess(images_nchw01)
        for idx, _, _ in CONVS:
            x = ops.conv_krsc_raw(x, *self.w[idx], 3, 3, 1, 1, 1)
            x = self._maxpool_relu(x) if idx in POOL_AFTER else ops.relu_raw(x)
        x = x.reshape(x.shape[0], -1)                     # NHWC flatten: (h, w, c), the order fc1's columns were put in
        for name in ("fc1", "fc2"):
            x = ops.relu_raw(ops.linear_fwd_raw(x, *self.w[name], force_f32=True))
        return x
