"""GroupNorm / LayerNorm kernels on inputs whose mean lies far from zero against their spread (tests/norm_cases.py), every
forward form and the backward that consumes its saved statistics, against fp64 of the same stored values.

randn data cannot tell a centred variance from `E[x^2] - E[x]^2`; these inputs can: at |mean| / std = 100 the second form
loses 60x the bound below in `rstd`.  What is compared: y, the saved mean / rstd (fp32 in both paths - where a bf16 output
would hide the error), dx, dgamma, dbeta.  Bound (norm_cases.check): err <= 8 max(e_ref, 2^-22 max|want|) with e_ref the
error of torch's fp32 CPU operator on the same input; bf16 outputs get one bf16 rounding of the result on top.
tests/test_norm_conditioning_cpu.py shows without a GPU that this bound rejects the uncentred formula and accepts a centred
one; profiles/gn_conditioning.txt has the measured figures of both.

Large launch shapes repeat a few distinct images (`reps`): the kernels treat every image alike, the fp64 reference is
computed once per distinct image, and parameter gradients (sums over images) scale exactly."""
import pytest
import torch
import torch.nn.functional as F

import norm_cases as nc

pytestmark = pytest.mark.gpu
dev = torch.device("cuda:0")
BF = torch.bfloat16


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from gad import ops as o
    return o


def _tile(t, reps):
    return t if reps == 1 else t.repeat(reps, *([1] * (t.dim() - 1)))


def _scaled(want, e_ref, reps):
    """reference of `reps` copies of the images: per-image quantities repeat, parameter gradients scale"""
    w, e = {}, dict(e_ref)
    for k, v in want.items():
        if k in ("dgamma", "dbeta"):
            w[k], e[k] = v * reps, e_ref[k] * reps
        else:
            w[k] = _tile(v, reps)
    return w, e


# ------------------------------------------------------------------------------------------------ fp32 GroupNorm ----
# B0 distinct images x reps, C, H, W, G.  Plans (csrc/norm.hip make_geo / make_slab):
FP32_SHAPES = {
    "sd64 two-pass 128x32px": (2, 1, 320, 64, 64, 32),          # [16, 64, 64, 320]'s chunks: any B <= 16 gives 128 chunks of 32 px
    "celeba64 two-pass 32x128px": (2, 32, 224, 64, 64, 32),     # [64, 64, 64, 224]: B = 64 gives 32 chunks of 128 px
    "ragged 96ch 48x48": (2, 1, 96, 48, 48, 32),                # 28 chunks of 83 px, the last one 63
    "ragged 224ch 44x44": (2, 1, 224, 44, 44, 32),              # 59 chunks of 33 px, the last one 22
    "one chunk 320ch 6x6": (2, 1, 320, 6, 6, 32),               # nch = 1 on the two-pass plan; per-channel slab by default
    "slab 128ch 32x32": (2, 1, 128, 32, 32, 32),                # 4 | cpg: slab plan by default
    "slab 256ch 16x16": (3, 1, 256, 16, 16, 32),
    "per-channel slab 96ch": (8, 1, 96, 32, 32, 32),            # 4 does not divide cpg = 3, 7, 10
    "per-channel slab 224ch": (8, 1, 224, 16, 16, 32),
    "per-channel slab 320ch": (8, 1, 320, 16, 16, 32),
}
DEFAULT_IS_TWO_PASS = {"sd64 two-pass 128x32px", "celeba64 two-pass 32x128px", "ragged 96ch 48x48", "ragged 224ch 44x44"}


def _fp32_plans():
    out = []
    for shape in FP32_SHAPES:
        for two_pass in (False, True):
            if two_pass and shape in DEFAULT_IS_TWO_PASS:
                continue                                          # the default plan already is the two-pass one
            out.append((shape, two_pass))
    return out


@pytest.mark.parametrize("case", list(nc.FP32_CASES))
@pytest.mark.parametrize("shape,two_pass", _fp32_plans())
def test_groupnorm_fp32(ops, shape, two_pass, case):
    B0, reps, C, H, W, G = FP32_SHAPES[shape]
    from gad import _capi
    a = _capi.GroupNormArgs()
    a.B, a.HW, a.C, a.G, a.flags = B0 * reps, H * W, C, G, _capi.GN_TWO_PASS if two_pass else 0
    assert bool(_capi.load().gad_groupnorm_one_pass(_capi.C.byref(a))) == (not two_pass and shape not in DEFAULT_IS_TWO_PASS)
    x = nc.FP32_CASES[case][0](B0, C, H * W, G, seed=11)
    gamma, beta = nc.affine(C, seed=1)
    dy = torch.randn(B0, C, H * W, generator=torch.Generator().manual_seed(12))
    want, e_ref = nc.group_norm_reference(x, G, gamma, beta, nc.EPS, False, dy)
    want, e_ref = _scaled(want, e_ref, reps)
    gx = _tile(nc.channels_last(x), reps).view(B0 * reps, H, W, C).to(dev).requires_grad_(True)
    gg, gb = gamma.to(dev).requires_grad_(True), beta.to(dev).requires_grad_(True)
    gdy = _tile(nc.channels_last(dy), reps).view(B0 * reps, H, W, C).to(dev)
    with ops.kernel_flags(gn_two_pass=two_pass):
        out = ops.group_norm(gx, gg, gb, G, nc.EPS, False)
        mean, rstd = out.grad_fn.saved_tensors[3:5]
        out.backward(gdy)
        with torch.no_grad():
            again = ops.group_norm(gx, gg, gb, G, nc.EPS, False)
    assert torch.equal(out, again)                                # fixed summation order: the same launch twice, the same bits
    got = {"y": out.view(B0 * reps, H * W, C).transpose(1, 2), "mean": mean, "rstd": rstd,
           "dx": gx.grad.view(B0 * reps, H * W, C).transpose(1, 2), "dgamma": gg.grad, "dbeta": gb.grad}
    if case == "constant":                                        # all partial sums exact: mean == 96, y == beta to 1 ulp
        assert bool((mean == 96.0).all())
        yb = (out.detach().cpu() - beta).abs()
        assert bool((yb <= torch.finfo(torch.float32).eps * beta.abs()).all())
    nc.check(got, want, e_ref, label=f"fp32 {shape} two_pass={int(two_pass)} {case}")


TWO_SOURCE = {  # B, C1, C2, H, G
    "sd64 640|320 two-pass": (2, 640, 320, 64, 32),
    "slab 128|128 32x32": (2, 128, 128, 32, 32),
    "slab 256|128 16x16 straddling": (2, 256, 128, 16, 32),
    "192|96 32x32 (9 per group)": (2, 192, 96, 32, 32),
}


TWO_SOURCE_DEFAULT_IS_TWO_PASS = {"sd64 640|320 two-pass", "192|96 32x32 (9 per group)"}


@pytest.mark.parametrize("case", list(nc.FP32_CASES))
@pytest.mark.parametrize("shape,two_pass", [(sh, tp) for sh in TWO_SOURCE for tp in (False, True)
                                            if not (tp and sh in TWO_SOURCE_DEFAULT_IS_TWO_PASS)])
def test_groupnorm_fp32_two_sources(ops, shape, two_pass, case):
    B, C1, C2, H, G = TWO_SOURCE[shape]
    C = C1 + C2
    from gad import _capi
    a = _capi.GroupNormArgs()
    a.B, a.HW, a.C, a.G, a.flags = B, H * H, C, G, _capi.GN_TWO_PASS if two_pass else 0
    assert bool(_capi.load().gad_groupnorm_one_pass(_capi.C.byref(a))) == (not two_pass and shape not in TWO_SOURCE_DEFAULT_IS_TWO_PASS)
    x = nc.FP32_CASES[case][0](B, C, H * H, G, seed=13)
    gamma, beta = nc.affine(C, seed=2)
    want, e_ref = nc.group_norm_reference(x, G, gamma, beta)
    xl = nc.channels_last(x).view(B, H, H, C)
    x1, x2 = xl[..., :C1].contiguous().to(dev), xl[..., C1:].contiguous().to(dev)
    y = torch.empty(B, H, H, C, device=dev)
    mean, rstd = torch.empty(B, G, device=dev), torch.empty(B, G, device=dev)
    gg, gb = gamma.to(dev), beta.to(dev)
    with ops.kernel_flags(gn_two_pass=two_pass):
        assert ops.group_norm_two_source_ok(x1, x2, G)
        a = ops._gn2_args(x1, x2, y, gg, gb, mean, rstd, G, nc.EPS, False)
        _capi.check(_capi.load().gad_groupnorm_silu_fwd(_capi.C.byref(a), ops._stream()), "gad_groupnorm_silu_fwd")
        again = ops.group_norm_cat_raw(x1, x2, gg, gb, G, nc.EPS, False)
    assert torch.equal(y, again)
    got = {"y": y.view(B, H * H, C).transpose(1, 2), "mean": mean, "rstd": rstd}
    if case == "constant":
        assert bool((mean == 96.0).all())
        assert bool(((y.cpu() - beta).abs() <= torch.finfo(torch.float32).eps * beta.abs()).all())
    nc.check(got, want, e_ref, label=f"fp32 two-source {shape} two_pass={int(two_pass)} {case}")


# ------------------------------------------------------------------------ GroupNorm writing the Winograd image ----
BT = torch.tensor([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0],
                   [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0], [0, 4, 0, -5, 0, 1]], dtype=torch.float64)


def _wino_input(y):
    """F(4x4, 3x3) input transform of y [B, C, H, W]: V [36][B * tiles][C] = B^T patch B over 6x6 patches at stride 4, pad 1"""
    B, C, H, W = y.shape
    p = F.pad(y, (1, 1, 1, 1)).unfold(2, 6, 4).unfold(3, 6, 4)            # [B, C, TH, TW, 6, 6]
    v = torch.einsum("ia,bctuad,jd->ijbtuc", BT.to(y.dtype), p, BT.to(y.dtype))
    return v.reshape(36, B * (H // 4) * (W // 4), C)


GN_WINO = {  # B, H, W, C, C1 (0: one source), G
    "128ch 32x32": (4, 32, 32, 128, 0, 32),
    "256ch 16x16": (2, 16, 16, 256, 0, 32),
    "256|128 16x16": (2, 16, 16, 384, 256, 32),
    "96ch 16x12 (12 per group)": (1, 16, 12, 96, 0, 8),
}


@pytest.mark.parametrize("case", list(nc.FP32_CASES))
@pytest.mark.parametrize("shape", list(GN_WINO))
def test_groupnorm_fp32_winograd_image(ops, shape, case):
    """gad_groupnorm_silu_wino4: mean / rstd against fp64, and V against the fp64 transform of the fp64 GroupNorm + SiLU.
    V's reference error is that of the transform applied to torch's fp32 GroupNorm + SiLU."""
    from gad import _capi
    lib = _capi.load()
    B, H, W, C, C1, G = GN_WINO[shape]
    x = nc.FP32_CASES[case][0](B, C, H * W, G, seed=17)
    gamma, beta = nc.affine(C, seed=3)
    want, e_ref = nc.group_norm_reference(x, G, gamma, beta, nc.EPS, True)
    want["V"] = _wino_input(want["y"].view(B, C, H, W))
    y32 = F.silu(F.group_norm(x, G, gamma, beta, nc.EPS)).view(B, C, H, W)
    e_ref["V"] = (_wino_input(y32).double() - want["V"]).abs().max().item()
    xl = nc.channels_last(x).view(B, H, W, C)
    x1, x2 = (xl.to(dev), None) if not C1 else (xl[..., :C1].contiguous().to(dev), xl[..., C1:].contiguous().to(dev))
    gg, gb = gamma.to(dev), beta.to(dev)
    a = _capi.GroupNormArgs()
    mean, rstd = torch.empty(B, G, device=dev), torch.empty(B, G, device=dev)
    a.x, a.gamma, a.beta, a.mean, a.rstd = x1.data_ptr(), gg.data_ptr(), gb.data_ptr(), mean.data_ptr(), rstd.data_ptr()
    a.B, a.HW, a.C, a.G, a.eps, a.silu = B, H * W, C, G, nc.EPS, 1
    if x2 is not None:
        a.x2, a.C1 = x2.data_ptr(), C1
    assert lib.gad_groupnorm_wino4_ok(_capi.C.byref(a), W) == 1
    T = B * (H // 4) * (W // 4)
    V, V2 = torch.zeros(36 * T * C, device=dev), torch.zeros(36 * T * C, device=dev)
    _capi.check(lib.gad_groupnorm_silu_wino4(_capi.C.byref(a), V.data_ptr(), W, ops._stream()), "gad_groupnorm_silu_wino4")
    _capi.check(lib.gad_groupnorm_silu_wino4(_capi.C.byref(a), V2.data_ptr(), W, ops._stream()), "gad_groupnorm_silu_wino4")
    assert torch.equal(V, V2)
    got = {"V": V.view(36, T, C), "mean": mean, "rstd": rstd}
    if case == "constant":                       # y = beta exactly, so V is the fp32 transform of beta: compare with its fp64 transform
        assert bool((mean == 96.0).all())
        Vb = _wino_input(F.silu(beta).double().view(1, C, 1, 1).expand(B, C, H, W))
        assert (V.view(36, T, C).cpu().double() - Vb).abs().max().item() <= 200 * 2.0 ** -22 * F.silu(beta).abs().max().item()   # |B^T . B| sums to 100; silu_f and the transform round a few ulp
    nc.check(got, want, e_ref, keys=("V", "mean", "rstd"), label=f"fp32 winograd image {shape} {case}")


# --------------------------------------------------------------------------------------- bf16-storage GroupNorm ----
HALF_SHAPES = {  # B0 distinct images x reps, HW, C, G
    "sd512 [16, 4096, 320]": (2, 8, 4096, 320, 32),
    "sd512 [16, 1024, 640]": (2, 8, 1024, 640, 32),
    "ragged [3, 90, 320]": (3, 1, 90, 320, 32),                   # 4 chunks of 23 rows, the last one 21
}


@pytest.mark.parametrize("case", list(nc.BF16_CASES))
@pytest.mark.parametrize("shape", list(HALF_SHAPES))
def test_groupnorm_bf16(ops, shape, case):
    """(no dgamma / dbeta here: the half path runs with frozen affine parameters and its backward computes dx only)"""
    from gad import half
    B0, reps, HW, C, G = HALF_SHAPES[shape]
    x = nc.BF16_CASES[case][0](B0, C, HW, G, seed=19)
    gamma, beta = nc.affine(C, seed=4)
    dy = torch.randn(B0, C, HW, generator=torch.Generator().manual_seed(20)).to(BF).float()
    want, e_ref = nc.group_norm_reference(x, G, gamma, beta, nc.EPS, False, dy)
    want, e_ref = _scaled(want, e_ref, reps)
    xh = _tile(nc.channels_last(x), reps).to(BF).to(dev)
    assert torch.equal(xh.float().cpu(), _tile(nc.channels_last(x), reps))              # stored exactly
    g_, b_ = torch.nn.Parameter(gamma.to(dev), requires_grad=False), torch.nn.Parameter(beta.to(dev), requires_grad=False)
    y, mean, rstd = half.group_norm_raw(xh, None, g_, b_, G, nc.EPS, False)
    xg = xh.clone().requires_grad_(True)
    out, alias = ops.group_norm_bypass(xg, g_, b_, G, nc.EPS, False)
    assert out.dtype == BF and torch.equal(out, y)
    m2, r2 = out.grad_fn.saved_tensors[1:3]
    assert torch.equal(m2, mean) and torch.equal(r2, rstd)
    out.backward(_tile(nc.channels_last(dy), reps).to(BF).to(dev))
    got = {"y": y.transpose(1, 2), "mean": mean, "rstd": rstd, "dx": xg.grad.transpose(1, 2)}
    if case == "constant":
        assert bool((mean == 96.0).all())
        assert torch.equal(y.float().cpu(), beta.to(BF).float().expand(B0 * reps, HW, C))   # beta, one bf16 rounding
    nc.check(got, want, e_ref, keys=("y", "mean", "rstd", "dx"), bf16_out=("y", "dx"), label=f"bf16 {shape} {case}")


HALF_TWO_SOURCE = {  # B0 x reps, HW, C1, C2, G
    "[16, 4096, 160|160]": (2, 8, 4096, 160, 160, 32),
    "[16, 1024, 320|320]": (2, 8, 1024, 320, 320, 32),
    "ragged [3, 90, 640|320]": (3, 1, 90, 640, 320, 32),
}


@pytest.mark.parametrize("case", list(nc.BF16_CASES))
@pytest.mark.parametrize("shape", list(HALF_TWO_SOURCE))
def test_groupnorm_bf16_two_sources(ops, shape, case):
    from gad import half
    B0, reps, HW, C1, C2, G = HALF_TWO_SOURCE[shape]
    C = C1 + C2
    x = nc.BF16_CASES[case][0](B0, C, HW, G, seed=23)
    gamma, beta = nc.affine(C, seed=5)
    want, e_ref = nc.group_norm_reference(x, G, gamma, beta)
    want, e_ref = _scaled(want, e_ref, reps)
    xl = _tile(nc.channels_last(x), reps).to(BF)
    x1, x2 = xl[..., :C1].contiguous().to(dev), xl[..., C1:].contiguous().to(dev)
    y, mean, rstd = half.group_norm_raw(x1, x2, gamma.to(dev), beta.to(dev), G, nc.EPS, False)
    y2, _, _ = half.group_norm_raw(x1, x2, gamma.to(dev), beta.to(dev), G, nc.EPS, False)
    assert torch.equal(y, y2)
    got = {"y": y.transpose(1, 2), "mean": mean, "rstd": rstd}
    nc.check(got, want, e_ref, bf16_out=("y",), label=f"bf16 two-source {shape} {case}")


# ---------------------------------------------------------------------------------------------------- LayerNorm ----
def _ln_input(cases, case, rows, C, seed):
    return cases[case][0](rows, C, 1, 1, seed=seed).view(rows, C)             # one "group" per row


@pytest.mark.parametrize("case", list(nc.FP32_CASES))
@pytest.mark.parametrize("rows,C", [(96, 320), (77, 1280)])
def test_layernorm_fp32(ops, rows, C, case):
    """transformer.hip's LayerNorm is centred already: expected to pass unchanged; this is what pins it"""
    x = _ln_input(nc.FP32_CASES, case, rows, C, 29)
    gamma, beta = nc.affine(C, seed=6)
    dy = torch.randn(rows, C, generator=torch.Generator().manual_seed(30))
    want, e_ref = nc.layer_norm_reference(x, gamma, beta, nc.EPS, dy)
    gx = x.to(dev).requires_grad_(True)
    gg, gb = gamma.to(dev).requires_grad_(True), beta.to(dev).requires_grad_(True)
    out = ops.layer_norm(gx, gg, gb, nc.EPS)
    mean, rstd = out.grad_fn.saved_tensors[2:4]
    out.backward(dy.to(dev))
    with torch.no_grad():
        assert torch.equal(out, ops.layer_norm(gx, gg, gb, nc.EPS))
    got = {"y": out, "mean": mean, "rstd": rstd, "dx": gx.grad, "dgamma": gg.grad, "dbeta": gb.grad}
    nc.check(got, want, e_ref, label=f"fp32 layernorm [{rows}, {C}] {case}")


@pytest.mark.parametrize("case", list(nc.BF16_CASES))
@pytest.mark.parametrize("rows,C", [(96, 320), (77, 1280)])
def test_layernorm_bf16(ops, rows, C, case):
    x = _ln_input(nc.BF16_CASES, case, rows, C, 31)
    gamma, beta = nc.affine(C, seed=7)
    dy = torch.randn(rows, C, generator=torch.Generator().manual_seed(32)).to(BF).float()
    want, e_ref = nc.layer_norm_reference(x, gamma, beta, nc.EPS, dy)
    g_, b_ = torch.nn.Parameter(gamma.to(dev), requires_grad=False), torch.nn.Parameter(beta.to(dev), requires_grad=False)
    xg = x.to(BF).to(dev).requires_grad_(True)
    out = ops.layer_norm(xg, g_, b_, nc.EPS)
    assert out.dtype == BF
    mean, rstd = out.grad_fn.saved_tensors[1:3]
    out.backward(dy.to(BF).to(dev))
    with torch.no_grad():
        assert torch.equal(out, ops.layer_norm(xg, g_, b_, nc.EPS))
    got = {"y": out, "mean": mean, "rstd": rstd, "dx": xg.grad}
    nc.check(got, want, e_ref, keys=("y", "mean", "rstd", "dx"), bf16_out=("y", "dx"), label=f"bf16 layernorm [{rows}, {C}] {case}")


# ------------------------------------------------------------------------------------------------- model level ----
def test_unet_forward_celeba_like_with_offset_activations(ops):
    """test_unet_forward_celeba_like's assertion where a user would meet the effect: the first GroupNorms run at a 64x64
    level (64 channels: two-pass plan) on activations that conv_in's bias of +30 moves far from zero."""
    from test_gpu_kernels import _models, close, rnd
    ref, mine, cfg = _models("celeba_config", dict(block_out_channels=[64, 128, 192, 224], sample_size=64))
    with torch.no_grad():
        ref.conv_in.bias.fill_(30.0)
        mine.conv_in.bias.fill_(30.0)
        x, t = rnd(2, 3, 64, 64, seed=1), torch.tensor([3, 700])
        got, want = mine(x.to(dev), t.to(dev)).sample, ref(x, t).sample
    print(f"celeba-like forward, conv_in.bias = 30: max err {(got.cpu() - want).abs().max().item():.3e} (ref max {want.abs().max().item():.3e})")
    close(got, want, atol=1e-4)
