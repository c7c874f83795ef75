"""float64 restatements for the precision / recall manifolds (csrc/manifold.hip) and a plain-torch VGG16 (gad/vgg.py).

The distance under test is defined as d2 = max(0, |a|^2 + |b|^2 - 2 a.b) on the exact fp16 values and d16 = (half)
sqrt_f32(d2).  Here d2 is formed in float64 (exact to 1e-16 relative, exactly for integer-valued features) and then takes
the definition's last two steps: rounded to fp32, the correctly rounded fp32 square root, rounded to fp16."""
import torch
import torch.nn.functional as F

VGG_CONVS = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
VGG_POOL_AFTER = (2, 7, 14, 21, 28)
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def dist16_ref(a, b):
    """fp16 [Na, D], [Nb, D] -> fp16 [Na, Nb]"""
    a, b = a.double(), b.double()
    d2 = ((a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2.0 * (a @ b.T)).clamp_min(0.0)
    return d2.float().sqrt().half()


def radii_ref(f, k):
    """the (k+1)-th smallest distance of every row to all rows, itself included -> fp16 [N]"""
    return dist16_ref(f, f).float().kthvalue(k + 1, dim=1).values.half()


def cover_ref(probe, target, kth_target):
    """bool [Np]: the probe lies within some target's radius, compared on the fp16 values"""
    return (dist16_ref(probe, target).float() <= kth_target.float()[None, :]).any(dim=1)


def pr_ref(gen, ref, k):
    """(precision, recall) of fp16 feature matrices"""
    return (float(cover_ref(gen, ref, radii_ref(ref, k)).double().mean()), float(cover_ref(ref, gen, radii_ref(gen, k)).double().mean()))


def vgg_trunk_ref(sd, images01, resolution, dtype):
    """torchvision's vgg16 up to the flatten: resize, ImageNet normalisation, `features`, AdaptiveAvgPool2d(7) -> [B, 25088]"""
    x = F.interpolate(images01.to(dtype), (resolution, resolution), mode="bilinear", align_corners=False)
    x = (x - torch.tensor(MEAN, dtype=dtype).view(1, 3, 1, 1)) / torch.tensor(STD, dtype=dtype).view(1, 3, 1, 1)
    for idx in VGG_CONVS:
        x = F.relu(F.conv2d(x, sd[f"features.{idx}.weight"].to(dtype), sd[f"features.{idx}.bias"].to(dtype), padding=1))
        if idx in VGG_POOL_AFTER:
            x = F.max_pool2d(x, 2, 2)
    return F.adaptive_avg_pool2d(x, 7).flatten(1)


def vgg_head_ref(sd, flat, dtype):
    """classifier.0 + ReLU + classifier.3 + ReLU (no dropout in eval) -> [B, 4096]"""
    x = F.relu(F.linear(flat.to(dtype), sd["classifier.0.weight"].to(dtype), sd["classifier.0.bias"].to(dtype)))
    return F.relu(F.linear(x, sd["classifier.3.weight"].to(dtype), sd["classifier.3.bias"].to(dtype)))


def vgg_ref(sd, images01, resolution, dtype):
    return vgg_head_ref(sd, vgg_trunk_ref(sd, images01, resolution, dtype), dtype)
