"""TEST INFRASTRUCTURE ONLY.  InceptionV3 as torchvision / pytorch-fid compute it, restated with plain torch.nn.functional over
a state dict in torchvision's key grammar (`Mixed_6a.branch3x3dbl_3.bn.running_var`, ...): NCHW, unfolded BatchNorm
(eps 1e-3), any float dtype - run in float64 it is the reference the HIP route (gad/inception.py) is measured against, in
float32 the yardstick for how far a correct fp32 evaluation lies from it.

variant "fid": pytorch-fid's FIDInceptionA / C / E_1 (avg_pool2d(count_include_pad=False)) and FIDInceptionE_2 (max_pool2d
3/1/1 in Mixed_7c); variant "torchvision": avg_pool2d's default everywhere.

pool_ref / resize_ref are the kernels' references: pool_ref restates the three pooling modes tap by tap (checked against
F.max_pool2d / F.avg_pool2d in tests/test_inception_cpu.py), resize_ref is F.interpolate in float64."""
import torch
import torch.nn.functional as F

EPS = 1e-3


def basic(sd, name, x, stride=1, padding=0):
    """BasicConv2d: conv without bias -> eval BatchNorm -> ReLU"""
    t = x.dtype
    y = F.conv2d(x, sd[f"{name}.conv.weight"].to(t), None, stride, padding)
    y = F.batch_norm(y, sd[f"{name}.bn.running_mean"].to(t), sd[f"{name}.bn.running_var"].to(t), sd[f"{name}.bn.weight"].to(t),
                     sd[f"{name}.bn.bias"].to(t), False, 0.0, EPS)
    return F.relu(y)


def _avg(x, variant):
    return F.avg_pool2d(x, 3, 1, 1, count_include_pad=(variant != "fid"))


def mixed_a_branches(sd, p, x, variant):
    b1 = basic(sd, f"{p}.branch1x1", x)
    b5 = basic(sd, f"{p}.branch5x5_2", basic(sd, f"{p}.branch5x5_1", x), padding=2)
    b3 = basic(sd, f"{p}.branch3x3dbl_1", x)
    b3 = basic(sd, f"{p}.branch3x3dbl_3", basic(sd, f"{p}.branch3x3dbl_2", b3, padding=1), padding=1)
    bp = basic(sd, f"{p}.branch_pool", _avg(x, variant))
    return [b1, b5, b3, bp]


def mixed_6a(sd, p, x):
    b3 = basic(sd, f"{p}.branch3x3", x, stride=2)
    bd = basic(sd, f"{p}.branch3x3dbl_2", basic(sd, f"{p}.branch3x3dbl_1", x), padding=1)
    bd = basic(sd, f"{p}.branch3x3dbl_3", bd, stride=2)
    return torch.cat([b3, bd, F.max_pool2d(x, 3, 2)], 1)


def mixed_c(sd, p, x, variant):
    b1 = basic(sd, f"{p}.branch1x1", x)
    b7 = basic(sd, f"{p}.branch7x7_1", x)
    b7 = basic(sd, f"{p}.branch7x7_2", b7, padding=(0, 3))
    b7 = basic(sd, f"{p}.branch7x7_3", b7, padding=(3, 0))
    bd = basic(sd, f"{p}.branch7x7dbl_1", x)
    bd = basic(sd, f"{p}.branch7x7dbl_2", bd, padding=(3, 0))
    bd = basic(sd, f"{p}.branch7x7dbl_3", bd, padding=(0, 3))
    bd = basic(sd, f"{p}.branch7x7dbl_4", bd, padding=(3, 0))
    bd = basic(sd, f"{p}.branch7x7dbl_5", bd, padding=(0, 3))
    bp = basic(sd, f"{p}.branch_pool", _avg(x, variant))
    return torch.cat([b1, b7, bd, bp], 1)


def mixed_7a(sd, p, x):
    b3 = basic(sd, f"{p}.branch3x3_2", basic(sd, f"{p}.branch3x3_1", x), stride=2)
    b7 = basic(sd, f"{p}.branch7x7x3_1", x)
    b7 = basic(sd, f"{p}.branch7x7x3_2", b7, padding=(0, 3))
    b7 = basic(sd, f"{p}.branch7x7x3_3", b7, padding=(3, 0))
    b7 = basic(sd, f"{p}.branch7x7x3_4", b7, stride=2)
    return torch.cat([b3, b7, F.max_pool2d(x, 3, 2)], 1)


def mixed_e(sd, p, x, variant):
    b1 = basic(sd, f"{p}.branch1x1", x)
    b3 = basic(sd, f"{p}.branch3x3_1", x)
    b3 = torch.cat([basic(sd, f"{p}.branch3x3_2a", b3, padding=(0, 1)), basic(sd, f"{p}.branch3x3_2b", b3, padding=(1, 0))], 1)
    bd = basic(sd, f"{p}.branch3x3dbl_2", basic(sd, f"{p}.branch3x3dbl_1", x), padding=1)
    bd = torch.cat([basic(sd, f"{p}.branch3x3dbl_3a", bd, padding=(0, 1)), basic(sd, f"{p}.branch3x3dbl_3b", bd, padding=(1, 0))], 1)
    pooled = F.max_pool2d(x, 3, 1, 1) if (variant == "fid" and p == "Mixed_7c") else _avg(x, variant)
    return torch.cat([b1, b3, bd, basic(sd, f"{p}.branch_pool", pooled)], 1)


def preprocess(images01, dtype):
    x = F.interpolate(images01.to(dtype), size=(299, 299), mode="bilinear", align_corners=False)
    return 2 * x - 1


def stem(sd, x):
    x = basic(sd, "Conv2d_1a_3x3", x, stride=2)
    x = basic(sd, "Conv2d_2a_3x3", x)
    x = F.max_pool2d(basic(sd, "Conv2d_2b_3x3", x, padding=1), 3, 2)
    x = basic(sd, "Conv2d_3b_1x1", x)
    return F.max_pool2d(basic(sd, "Conv2d_4a_3x3", x), 3, 2)


@torch.no_grad()
def forward(sd, images01, variant, dtype=torch.float64):
    """[B,3,H,W] in [0,1] -> (pool3 [B,2048], logits [B, fc rows]) in `dtype`"""
    x = stem(sd, preprocess(images01, dtype))
    for p in ("Mixed_5b", "Mixed_5c", "Mixed_5d"):
        x = torch.cat(mixed_a_branches(sd, p, x, variant), 1)
    x = mixed_6a(sd, "Mixed_6a", x)
    for p in ("Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e"):
        x = mixed_c(sd, p, x, variant)
    x = mixed_7a(sd, "Mixed_7a", x)
    x = mixed_e(sd, "Mixed_7c", mixed_e(sd, "Mixed_7b", x, variant), variant)
    pool3 = x.mean(dim=(2, 3))
    return pool3, F.linear(pool3, sd["fc.weight"].to(dtype), sd["fc.bias"].to(dtype))


MAX, AVG, AVG_VALID = 0, 1, 2


def pool_ref(x_nhwc, k, stride, pad, mode, relu_in=False):
    """[B,H,W,C] -> float64 [B,Ho,Wo,C], tap by tap: max over the taps inside the map; sum over them divided by k*k (AVG: the
    padding counts, as zeros) or by their number (AVG_VALID).  relu_in pools relu(x)."""
    x = x_nhwc.double()
    if relu_in:
        x = x.clamp_min(0)
    B, H, W, C = x.shape
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    y = torch.empty(B, Ho, Wo, C, dtype=torch.float64)
    for oh in range(Ho):
        for ow in range(Wo):
            hs, ws = max(oh * stride - pad, 0), max(ow * stride - pad, 0)
            he, we = min(oh * stride - pad + k, H), min(ow * stride - pad + k, W)
            win = x[:, hs:he, ws:we, :].reshape(B, -1, C)
            if mode == MAX:
                y[:, oh, ow] = win.max(dim=1).values
            else:
                y[:, oh, ow] = win.sum(dim=1) / (k * k if mode == AVG else win.shape[1])
    return y


def resize_ref(x_nchw, size, a=1.0, b=0.0):
    """F.interpolate(bilinear, align_corners=False) in float64, y = a v + b, as NHWC [B,Ho,Wo,C]"""
    y = F.interpolate(x_nchw.double(), size=size, mode="bilinear", align_corners=False)
    return (a * y + b).permute(0, 2, 3, 1).contiguous()
