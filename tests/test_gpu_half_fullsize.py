"""The bf16 activation path (csrc/half.hip, gad/half.py) at the launch shapes of the bench's SD lines: sd512 (B = 16, 64x64
latents) and sd256 (B = 64, 32x32 latents), LoRA r = 256, context [B, 77, 768].  tests/test_gpu_half.py checks the same kernels
at small shapes; at these sizes the planner picks tile / split-K forms that small shapes never reach.

Reference: fp64 on the device of the SAME bf16-rounded operands, so what is left is fp32 accumulation order and the final bf16
rounding (the tolerance model of tests/test_gpu_half.py: bf16 outputs 2^-8 |v| + 2e-5 sqrt(K); fp32 outputs 2e-5 sqrt(K) of the
scale; attention the norm-relative bars of test_h_attention_fwd_bwd).  Convolutions are nine per-tap fp64 matmuls over a shifted
view of the zero-padded (nearest-2x upsampled) input.

Every launch of the half path is summarised by a plan signature (entry point, gather kind, sources, output type, the C planner's
tile and whether K is split; (Tq, Tk, d) for attention; the channel count for the norms).  Each case below checks that its
launches have the signatures derived for it on the host, and test_model_launch_forms_are_all_covered fails when a full-size
model step makes a launch whose signature no case covers."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

from test_gpu_half import close_h, hguarded

pytestmark = pytest.mark.gpu
dev = torch.device("cuda:0")
BF = torch.bfloat16
SD512, SD256 = dict(latent=64, batch=16), dict(latent=32, batch=64)


@pytest.fixture(autouse=True)
def _free_memory():
    yield
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def drnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, device=dev, generator=torch.Generator(device=dev).manual_seed(seed)) * scale


def hbd(t):
    """bf16-rounded copy and the fp64 value of exactly those numbers, both on the device"""
    h = t.to(BF)
    return h, h.double()


def rel(got, want):
    return ((got.double() - want).norm() / want.norm()).item()


# ---------------------------------------------------------------------------------------------------------------
# plan signatures
# ---------------------------------------------------------------------------------------------------------------
class LaunchLog:
    """Signatures of the half path's launches.  Installed as ops.PROFILER around one extra call of hgemm_raw / wgrad_raw, it sees
    the argument struct the launch would get and asks the C planner for its form (that call launches nothing)."""

    def __init__(self):
        self.sigs = {}

    def add(self, sig, shape):
        self.sigs.setdefault(sig, shape)

    def hgemm(self, lib, a, tn=False):
        if tn:
            need = lib.gad_hgemm_tn_workspace_bytes(C.byref(a))
            assert need >= 0
            self.add(("tn", need > 0), (a.M, a.N, a.K))
            return
        tile, sk = C.c_int32(), C.c_int32()
        assert lib.gad_hgemm_plan(C.byref(a), C.byref(tile), C.byref(sk)) == 0, lib.gad_last_error()
        self.add(("hgemm", a.conv, a.stride if a.conv else 1, a.upsample, bool(a.A2) and bool(a.conv), bool(a.A2) and not a.conv,
                  a.out_f32, tile.value, sk.value > 1), (a.M, a.N, a.K, tile.value, sk.value))

    def plans(self):
        """(tile, split-K) of every hgemm launch seen"""
        return sorted({shape[3:] for sig, shape in self.sigs.items() if sig[0] == "hgemm"})


class recording:
    """Record the signatures of every half-path launch inside the block (launches still run).  dry=True: record only - no
    hgemm / hgemm_tn launch is made, operands may live on the host (used to derive the signatures a case must have)."""

    def __init__(self, dry=False):
        self.log, self.dry = LaunchLog(), dry

    def __enter__(self):
        from gad import half, ops
        self.saved = {n: getattr(half, n) for n in ("hgemm_raw", "wgrad_raw", "attention_core", "group_norm", "group_norm_bypass",
                                                    "group_norm_raw", "layer_norm", "layer_norm_bypass", "geglu")}
        log, dry, saved = self.log, self.dry, self.saved

        def contraction(name):
            def f(*args, **kw):
                prev, ops.PROFILER = ops.PROFILER, log
                ws_prev = ops.WS_OVERRIDE[0]
                if dry:
                    ops.WS_OVERRIDE[0] = torch.empty(0, dtype=torch.uint8)
                try:
                    saved[name](*args, **kw)
                finally:
                    ops.PROFILER, ops.WS_OVERRIDE[0] = prev, ws_prev
                if not dry:
                    saved[name](*args, **kw)
            return f

        def attn(q, k, v, heads, scale=None):
            log.add(("attn", q.shape[1], k.shape[1], q.shape[-1] // heads), tuple(q.shape))
            return saved["attention_core"](q, k, v, heads, scale)

        def norm(name, kind):
            def f(x, *args, **kw):
                c = x.shape[-1] + (args[0].shape[-1] if name == "group_norm_raw" and args[0] is not None else 0)
                log.add((kind, c), tuple(x.shape))
                return saved[name](x, *args, **kw)
            return f
        half.hgemm_raw, half.wgrad_raw = contraction("hgemm_raw"), contraction("wgrad_raw")
        half.attention_core = attn
        for n in ("group_norm", "group_norm_bypass", "group_norm_raw"):
            setattr(half, n, norm(n, "gn"))
        half.layer_norm, half.layer_norm_bypass, half.geglu = norm("layer_norm", "ln"), norm("layer_norm_bypass", "ln"), norm("geglu", "geglu")
        return self.log

    def __exit__(self, *exc):
        from gad import half
        for n, f in self.saved.items():
            setattr(half, n, f)
        return False


# ---------------------------------------------------------------------------------------------------------------
# (a) forward convolutions (and the dense launches the planner table names) at production shapes
# ---------------------------------------------------------------------------------------------------------------
def _geom(H, k, stride, ups):
    He = 2 * H if ups else H
    return (He + 2 * (k // 2) - k) // stride + 1


# name: B, H (= W), C1, C2 (second source, 0 = none), Cout, k, stride, upsample, expected (tile, split-K)
CONV_FWD = {
    "sd512_64x64_320": (16, 64, 320, 0, 320, 3, 1, False, (6, 1)),
    "sd512_32x32_640": (16, 32, 640, 0, 640, 3, 1, False, (6, 2)),
    "sd512_16x16_1280": (16, 16, 1280, 0, 1280, 3, 1, False, (6, 4)),
    "sd512_8x8_1280": (16, 8, 1280, 0, 1280, 3, 1, False, (7, 10)),
    "sd256_32x32_320": (64, 32, 320, 0, 320, 3, 1, False, (6, 1)),
    "up3_x2_64x64_640+320": (16, 64, 640, 320, 320, 3, 1, False, (6, 1)),
    "up2_x2_32x32_1280+640": (16, 32, 1280, 640, 640, 3, 1, False, (6, 2)),
    "up1_x2_16x16_1280+1280": (16, 16, 1280, 1280, 1280, 3, 1, False, (6, 4)),
    "up0_x2_8x8_1280+1280": (16, 8, 1280, 1280, 1280, 3, 1, False, (7, 16)),
    "down0_s2_64x64_320": (16, 64, 320, 0, 320, 3, 2, False, (6, 2)),
    "down1_s2_32x32_640": (16, 32, 640, 0, 640, 3, 2, False, (7, 5)),
    "down2_s2_16x16_1280": (16, 16, 1280, 0, 1280, 3, 2, False, (7, 10)),
    "up0_ups_8x8_1280": (16, 8, 1280, 0, 1280, 3, 1, True, (6, 4)),
    "up1_ups_16x16_1280": (16, 16, 1280, 0, 1280, 3, 1, True, (6, 1)),
    "up2_ups_32x32_640": (16, 32, 640, 0, 640, 3, 1, True, (6, 1)),
    "down1_shortcut_1x1_320_640": (16, 32, 320, 0, 640, 1, 1, False, (8, 1)),
    "up1_shortcut_1x1_2560_1280": (16, 16, 2560, 0, 1280, 1, 1, False, (6, 2)),
    "up3_shortcut_1x1_960_320": (16, 64, 960, 0, 320, 1, 1, False, (7, 1)),
    "conv_out_320_4": (16, 64, 320, 0, 4, 3, 1, False, (8, 1)),
}


def conv_ref(xd, wd, stride, ups):
    """fp64 NHWC convolution (pad k // 2) as nine per-tap matmuls: xd [B,H,W,Cin], wd [Cout,Cin,k,k] -> [B,Ho,Wo,Cout]"""
    k = wd.shape[-1]
    if ups:
        xd = xd.repeat_interleave(2, 1).repeat_interleave(2, 2)
    p = k // 2
    xp = F.pad(xd, (0, 0, p, p, p, p))
    Ho, Wo = (xp.shape[1] - k) // stride + 1, (xp.shape[2] - k) // stride + 1
    out = None
    for r in range(k):
        for s in range(k):
            t = xp[:, r:r + stride * (Ho - 1) + 1:stride, s:s + stride * (Wo - 1) + 1:stride, :] @ wd[:, :, r, s].T
            out = t if out is None else out + t
    return out


def _conv_operands(B, H, C1, C2, Cout, k, stride, ups, device, seed=0):
    Ho = _geom(H, k, stride, ups)
    mk = (lambda *s, seed, scale=1.0: drnd(*s, seed=seed, scale=scale)) if device == dev else \
        (lambda *s, seed, scale=1.0: torch.empty(*s))
    x = mk(B, H, H, C1, seed=seed + 1).to(BF)
    x2 = mk(B, H, H, C2, seed=seed + 2).to(BF) if C2 else None
    w = mk(Cout, k, k, C1 + C2, seed=seed + 3, scale=(k * k * (C1 + C2)) ** -0.5).to(BF)
    bias = mk(Cout, seed=seed + 4)
    temb = mk(B, Cout, seed=seed + 5)
    res = mk(B, Ho, Ho, Cout, seed=seed + 6).to(BF)
    return x, x2, w, bias, temb, res


def _conv_fwd_launch(x, x2, w, bias, temb, res, k, stride, ups):
    """what HConv2dFn.forward launches (a 1x1 convolution is a dense GEMM over the pixel rows), with the full epilogue"""
    from gad import half
    if k == 1:
        Cout = w.shape[0]
        return half.linear_raw(x.view(-1, x.shape[-1]), w.view(Cout, -1), bias, res.view(-1, Cout)).view(*x.shape[:-1], Cout)
    return half.conv_fwd_raw(x, w, bias, k, k, stride, (k // 2,) * 4, ups, rowadd=temb, residual=res, x2=x2)


def conv_fwd_sigs(row):
    B, H, C1, C2, Cout, k, stride, ups, _ = row
    with recording(dry=True) as log:
        _conv_fwd_launch(*_conv_operands(B, H, C1, C2, Cout, k, stride, ups, "cpu"), k, stride, ups)
    return log


@pytest.mark.parametrize("name", list(CONV_FWD))
def test_conv_fwd_fullsize_vs_fp64(name):
    B, H, C1, C2, Cout, k, stride, ups, plan = row = CONV_FWD[name]
    assert not (k == 1 and C2), "1x1 rows are single-source"
    x, x2, w, bias, temb, res = _conv_operands(B, H, C1, C2, Cout, k, stride, ups, dev)
    with recording() as log:
        y = _conv_fwd_launch(x, x2, w, bias, temb, res, k, stride, ups)
    assert log.plans() == [plan], f"{name}: ran {log.plans()}, the case documents {plan}"
    assert set(log.sigs) == set(conv_fwd_sigs(row).sigs)
    xd = torch.cat([x, x2], -1).double() if C2 else x.double()
    want = conv_ref(xd, w.double().permute(0, 3, 1, 2), stride, ups) + bias.double() + res.double()
    if k != 1:
        want += temb.double()[:, None, None, :]
    close_h(y, want.cpu(), extra=2e-5 * math.sqrt(k * k * (C1 + C2)), what=f"{name} conv fwd")


# dense launches the CPU planner test pins: M, N, K, alpha, bias, residual, expected (tile, split-K)
DENSE_FWD = {
    "geglu_proj_65536x2560x320": (65536, 2560, 320, 1.0, True, False, (7, 1)),
    "lora_down_65536x256x320": (65536, 256, 320, 0.5, False, False, (8, 1)),
    "linear_16x16_4096x1280x1280": (4096, 1280, 1280, 1.0, True, True, (9, 1)),
    "ff_out_8x8_1024x1280x5120": (1024, 1280, 5120, 1.0, True, True, (7, 4)),
    "geglu_proj_dgrad_65536x320x2560": (65536, 320, 2560, 1.0, False, False, (6, 1)),
}


def _dense_operands(M, N, K, has_bias, has_res, device):
    mk = (lambda *s, seed, scale=1.0: drnd(*s, seed=seed, scale=scale)) if device == dev else (lambda *s, seed, scale=1.0: torch.empty(*s))
    a = mk(M, K, seed=1).to(BF)
    b = mk(N, K, seed=2, scale=K ** -0.5).to(BF)
    return a, b, mk(N, seed=3) if has_bias else None, mk(M, N, seed=4).to(BF) if has_res else None


def dense_fwd_sigs(row):
    M, N, K, alpha, hb_, hr, _ = row
    from gad import half
    with recording(dry=True) as log:
        a, b, bias, res = _dense_operands(M, N, K, hb_, hr, "cpu")
        half.linear_raw(a, b, bias, res, alpha=alpha)
    return log


@pytest.mark.parametrize("name", list(DENSE_FWD))
def test_dense_fwd_fullsize_vs_fp64(name):
    from gad import half
    M, N, K, alpha, has_bias, has_res, plan = row = DENSE_FWD[name]
    a, b, bias, res = _dense_operands(M, N, K, has_bias, has_res, dev)
    with recording() as log:
        y = half.linear_raw(a, b, bias, res, alpha=alpha)
    assert log.plans() == [plan], f"{name}: ran {log.plans()}, the case documents {plan}"
    assert set(log.sigs) == set(dense_fwd_sigs(row).sigs)
    want = alpha * (a.double() @ b.double().T)
    if bias is not None:
        want += bias.double()
    if res is not None:
        want += res.double()
    close_h(y, want.cpu(), extra=2e-5 * math.sqrt(K), what=f"{name} dense fwd")


# ---------------------------------------------------------------------------------------------------------------
# (b) data gradients through HConv2dFn
# ---------------------------------------------------------------------------------------------------------------
CONV_DGRAD = {  # B, H, Cin, Cout, k, stride, upsample
    "3x3_s1_64x64_320": (16, 64, 320, 320, 3, 1, False),
    "3x3_s2_64x64_320": (16, 64, 320, 320, 3, 2, False),
    "3x3_s2_16x16_1280": (16, 16, 1280, 1280, 3, 2, False),
    "3x3_ups_32x32_640": (16, 32, 640, 640, 3, 1, True),
    "1x1_64x64_960_320": (16, 64, 960, 320, 1, 1, False),
    "conv_out_64x64_320_4": (16, 64, 320, 4, 3, 1, False),
}


def conv_dgrad_sigs(row):
    """the launches of HConv2dFn forward + backward (the backward's forms, as gad/half.py picks them)"""
    from gad import half
    B, H, Cin, Cout, k, stride, ups = row
    Ho = _geom(H, k, stride, ups)
    e = torch.empty
    with recording(dry=True) as log:
        x, dy = e(B, H, H, Cin, dtype=BF), e(B, Ho, Ho, Cout, dtype=BF)
        if k == 1:
            half.linear_raw(x.view(-1, Cin), e(Cout, Cin, dtype=BF))
            half.linear_raw(dy.view(-1, Cout), e(Cin, Cout, dtype=BF))
        else:
            half.conv_fwd_raw(x, e(Cout, 3, 3, Cin, dtype=BF), None, 3, 3, stride, (1,) * 4, ups)
            if stride == 2:
                half.conv_fwd_raw(dy, e(Cin, 3, 3, Cout, dtype=BF), None, 3, 3, 1, (1, 0, 1, 0), conv=2, out_hw=(H, H))
            else:
                c8 = (Cout + 7) // 8 * 8
                half.conv_fwd_raw(e(B, Ho, Ho, c8, dtype=BF), e(Cin, 3, 3, c8, dtype=BF), None, 3, 3)
    return log


@pytest.mark.parametrize("name", list(CONV_DGRAD))
def test_conv_dgrad_fullsize_vs_fp64_autograd(name):
    from gad import ops
    B, H, Cin, Cout, k, stride, ups = row = CONV_DGRAD[name]
    x, xd = hbd(drnd(B, H, H, Cin, seed=1))
    w = drnd(Cout, Cin, k, k, seed=2, scale=(k * k * Cin) ** -0.5).to(BF).float()
    wp = torch.nn.Parameter(w.contiguous(memory_format=torch.channels_last), requires_grad=False)
    xr = xd.clone().requires_grad_(True)
    want = conv_ref(xr, w.double(), stride, ups)
    dy, dyd = hbd(drnd(*want.shape, seed=3))
    want.backward(dyd)
    xg = x.clone().requires_grad_(True)
    with recording() as log:
        y = ops.conv2d(xg, wp, None, None, None, stride, (k // 2,) * 4, ups)
        assert y.dtype == BF
        y.backward(dy)
    assert set(log.sigs) == set(conv_dgrad_sigs(row).sigs), (sorted(log.sigs), log.plans())
    close_h(y, want.detach().cpu(), extra=2e-5 * math.sqrt(k * k * Cin), what=f"{name} conv fwd")
    extra = 2.0 ** -7 * xr.grad.abs().max().item() if ups else 0.0            # (as test_hconv_autograd_dgrad: four bf16 roundings)
    close_h(xg.grad, xr.grad.cpu(), extra=2e-5 * math.sqrt(k * k * Cout) * 2 + extra, what=f"{name} conv dgrad")


# ---------------------------------------------------------------------------------------------------------------
# (c) the LoRA linear at production rows, and the token-axis weight gradient
# ---------------------------------------------------------------------------------------------------------------
LORA = {  # M, K, N, r
    "to_q_64x64_r256": (16 * 4096, 320, 320, 256),             # dA, dB through G = dy^T x (the wide-rank route)
    "to_q_32x32_r256": (16 * 1024, 640, 640, 256),
    "to_k_context_r256": (16 * 77, 768, 320, 256),
    "to_q_64x64_r17": (16 * 4096, 320, 320, 17),               # ragged: padded to 24, direct dmid^T x / dy^T mid
}


def lora_sigs(row):
    from gad import half
    M, K, N, r = row
    r8 = (r + 7) // 8 * 8
    e = torch.empty
    with recording(dry=True) as log:
        x, dy, mid, dmid = e(M, K, dtype=BF), e(M, N, dtype=BF), e(M, r8, dtype=BF), e(M, r8, dtype=BF)
        half.linear_raw(x, e(r8, K, dtype=BF), alpha=0.5)
        half.linear_raw(x, e(N, K, dtype=BF), e(N), A2=mid, B2=e(N, r8, dtype=BF))
        half.linear_raw(dy, e(r8, N, dtype=BF), alpha=0.5)
        half.linear_raw(dy, e(K, N, dtype=BF), A2=dmid, B2=e(K, r8, dtype=BF))
        if N * K <= 1.5 * r * (N + K):
            half.wgrad_raw(dy, x, e(N, K), accumulate=False)
        else:
            half.wgrad_raw(dmid, x, e(r, K), accumulate=False)
            half.wgrad_raw(dy, mid, e(N, r), accumulate=False)
    return log


@pytest.mark.parametrize("name", list(LORA))
def test_lora_linear_fullsize_vs_fp64_autograd(name):
    from gad import ops
    M, K, N, r = row = LORA[name]
    x, xd = hbd(drnd(M, K, seed=1))
    w = drnd(N, K, seed=2, scale=0.05).to(BF).float()
    bias = drnd(N, seed=3)
    down = drnd(r, K, seed=4, scale=0.1).to(BF).float()
    up = drnd(N, r, seed=5, scale=0.1).to(BF).float()
    res, resd = hbd(drnd(M, N, seed=6))
    s = 0.5
    xr = xd.clone().requires_grad_(True)
    dr, ur = down.double().requires_grad_(True), up.double().requires_grad_(True)
    mid = s * (xr @ dr.T)
    y = xr @ w.double().T + bias.double() + mid.to(BF).double() @ ur.T + resd        # (mid is stored as bf16 on the device)
    y_exact = xr @ w.double().T + bias.double() + mid @ ur.T + resd
    dy, dyd = hbd(drnd(M, N, seed=7))
    y_exact.backward(dyd)
    wp = torch.nn.Parameter(w, requires_grad=False)
    bp = torch.nn.Parameter(bias, requires_grad=False)
    dp, upp = torch.nn.Parameter(down.clone()), torch.nn.Parameter(up.clone())
    xg = x.clone().requires_grad_(True)
    with recording() as log:
        out = ops.lora_linear(xg, wp, bp, dp, upp, s, res)
        out.backward(dy)
    assert set(log.sigs) == set(lora_sigs(row).sigs), sorted(log.sigs)
    flip = 2.0 ** -7 * mid.detach().abs().max().item() * up.abs().max().item()      # (as test_h_lora_linear_autograd)
    close_h(out, y.detach().cpu(), extra=3e-5 * math.sqrt(K + r) + flip, what=f"{name} lora fwd")
    assert rel(xg.grad, xr.grad) < 6e-3
    assert dp.grad.dtype == torch.float32 and upp.grad.dtype == torch.float32
    assert rel(dp.grad, dr.grad) < 6e-3 and rel(upp.grad, ur.grad) < 6e-3


@pytest.mark.parametrize("N,K", [(320, 320), (640, 640), (1280, 1280), (320, 768)])
def test_wgrad_tn_fullsize_vs_fp64(N, K):
    from gad import _capi, half
    from gad._capi import HGemmArgs
    T = 65536
    dy, dyd = hbd(drnd(T, N, seed=1))
    x, xd = hbd(drnd(T, K, seed=2))
    a = HGemmArgs()
    a.A, a.B, a.C = dy.data_ptr(), x.data_ptr(), 1 << 24
    a.M, a.N, a.K, a.lda, a.ldb, a.ldc, a.out_f32 = N, K, T, N, K, K, 1
    assert _capi.load().gad_hgemm_tn_workspace_bytes(C.byref(a)) > 0, "the plan does not split the token axis"
    want = dyd.T @ xd
    out = torch.full((N, K), 7.0, device=dev)
    with recording() as log:
        half.wgrad_raw(dy, x, out, accumulate=False)
    assert set(log.sigs) == {("tn", True)}
    tol = 2e-5 * math.sqrt(T) * max(1.0, want.abs().max().item())
    assert (out.double() - want).abs().max().item() < tol
    half.wgrad_raw(dy, x, out, accumulate=True, alpha=0.5)
    assert (out.double() - 1.5 * want).abs().max().item() < 2 * tol


# ---------------------------------------------------------------------------------------------------------------
# (d) attention at every SD level
# ---------------------------------------------------------------------------------------------------------------
ATTN = [  # B, Tq, Tk, heads, d
    (16, 4096, 4096, 8, 40), (16, 1024, 1024, 8, 80), (16, 256, 256, 8, 160), (16, 64, 64, 8, 160),                  # sd512 self
    (16, 4096, 77, 8, 40), (16, 1024, 77, 8, 80), (16, 256, 77, 8, 160), (16, 64, 77, 8, 160),                       # sd512 cross
    (64, 1024, 1024, 8, 40), (64, 1024, 77, 8, 40), (64, 256, 256, 8, 80), (64, 256, 77, 8, 80), (64, 16, 16, 8, 160),
    (64, 16, 77, 8, 160),                                                                                              # sd256
]


@pytest.mark.parametrize("B,Tq,Tk,heads,d", ATTN)
def test_attention_fullsize_vs_fp64(B, Tq, Tk, heads, d):
    from gad import ops
    C_ = heads * d
    q, k, v = (hbd(drnd(B, T, C_, seed=i, scale=sc))[0] for i, T, sc in ((1, Tq, 0.5), (2, Tk, 0.5), (3, Tk, 1.0)))
    do = drnd(B, Tq, C_, seed=4).to(BF)
    gq, gk, gv = (t.clone().requires_grad_(True) for t in (q, k, v))
    with recording() as log:
        out = ops.attention_core(gq, gk, gv, heads)
        out.backward(do)
    assert set(log.sigs) == {("attn", Tq, Tk, d)} and out.dtype == BF
    g = torch.Generator().manual_seed(B * Tq + Tk)
    pairs = [(0, 0), (B - 1, heads - 1)] + list(zip(torch.randint(0, B, (2,), generator=g).tolist(), torch.randint(0, heads, (2,), generator=g).tolist()))
    for b, h in pairs:
        cs = slice(h * d, (h + 1) * d)
        qr, kr, vr = (t[b, :, cs].double().requires_grad_(True) for t in (q, k, v))
        o = torch.softmax((qr @ kr.T) / math.sqrt(d), dim=-1) @ vr
        o.backward(do[b, :, cs].double())
        got = out[b, :, cs]
        assert rel(got, o.detach()) < 6e-3, (b, h)
        assert rel(gq.grad[b, :, cs], qr.grad) < 1.2e-2 and rel(gk.grad[b, :, cs], kr.grad) < 1.2e-2 and rel(gv.grad[b, :, cs], vr.grad) < 1.2e-2, (b, h)
        assert (got.double() - o.detach()).abs().max().item() < 0.03 * o.detach().abs().max().item(), (b, h)


# ---------------------------------------------------------------------------------------------------------------
# (e) GroupNorm (+SiLU, +bypass, two sources), LayerNorm, GEGLU at full rows
# ---------------------------------------------------------------------------------------------------------------
GN = [  # B, HW, C, silu: every width the SD U-Net normalises, at the level it does so
    (16, 4096, 320, True), (16, 4096, 640, True), (16, 4096, 960, True), (16, 1024, 640, False), (16, 1024, 1280, True),
    (16, 1024, 1920, True), (16, 256, 1280, True), (16, 256, 2560, True), (16, 256, 1920, False), (16, 64, 2560, True),
]


@pytest.mark.parametrize("B,HW,C,silu", GN)
def test_groupnorm_fullsize_vs_fp64(B, HW, C, silu):
    from gad import ops
    x, xd = hbd(drnd(B, HW, C, seed=1) * 1.5 + 0.3)
    gamma, beta = drnd(C, seed=2) * 0.2 + 1, drnd(C, seed=3) * 0.1
    xr = xd.clone().requires_grad_(True)
    y = F.group_norm(xr.transpose(1, 2), 32, gamma.double(), beta.double(), 1e-5).transpose(1, 2)
    if silu:
        y = F.silu(y)
    dy, dyd = hbd(drnd(B, HW, C, seed=4))
    byp, bypd = hbd(drnd(B, HW, C, seed=5))
    y.backward(dyd)
    g_, b_ = torch.nn.Parameter(gamma, requires_grad=False), torch.nn.Parameter(beta, requires_grad=False)
    xg = x.clone().requires_grad_(True)
    with recording() as log:
        out, alias = ops.group_norm_bypass(xg, g_, b_, 32, 1e-5, silu)
        torch.autograd.backward([out, alias], [dy, byp])
    assert set(log.sigs) == {("gn", C)}
    close_h(out, y.detach().cpu(), extra=2e-5, what="gn fwd")
    close_h(xg.grad, (xr.grad + bypd).cpu(), extra=3e-5 * max(1.0, xr.grad.abs().max().item()), what="gn bwd + bypass")


@pytest.mark.parametrize("B,HW,C1,C2", [(16, 4096, 640, 320), (16, 1024, 1280, 640), (16, 256, 1280, 1280), (16, 64, 1280, 1280)])
def test_groupnorm_two_sources_fullsize_vs_fp64(B, HW, C1, C2):
    from gad import half
    x1, x1d = hbd(drnd(B, HW, C1, seed=1))
    x2, x2d = hbd(drnd(B, HW, C2, seed=2) * 2 + 1)
    gamma, beta = drnd(C1 + C2, seed=3) * 0.2 + 1, drnd(C1 + C2, seed=4) * 0.1
    want = F.silu(F.group_norm(torch.cat([x1d, x2d], -1).transpose(1, 2), 32, gamma.double(), beta.double(), 1e-5).transpose(1, 2))
    y, _, _ = half.group_norm_raw(x1, x2, gamma, beta, 32, 1e-5, True)
    close_h(y, want.cpu(), extra=2e-5, what="two-source gn")


@pytest.mark.parametrize("rows,C", [(16 * 4096, 320), (16 * 1024, 640), (16 * 256, 1280), (64 * 16, 1280)])
def test_layernorm_fullsize_vs_fp64(rows, C):
    from gad import ops
    x, xd = hbd(drnd(rows, C, seed=1) * 1.7 + 0.4)
    gamma, beta = drnd(C, seed=2) * 0.2 + 1, drnd(C, seed=3) * 0.1
    xr = xd.clone().requires_grad_(True)
    y = F.layer_norm(xr, (C,), gamma.double(), beta.double(), 1e-5)
    dy, dyd = hbd(drnd(rows, C, seed=4))
    byp, bypd = hbd(drnd(rows, C, seed=5))
    y.backward(dyd)
    g_, b_ = torch.nn.Parameter(gamma, requires_grad=False), torch.nn.Parameter(beta, requires_grad=False)
    xg = x.clone().requires_grad_(True)
    with recording() as log:
        out, alias = ops.layer_norm_bypass(xg, g_, b_, 1e-5)
        torch.autograd.backward([out, alias], [dy, byp])
    assert set(log.sigs) == {("ln", C)}
    close_h(out, y.detach().cpu(), extra=2e-5, what="ln fwd")
    close_h(xg.grad, (xr.grad + bypd).cpu(), extra=3e-5 * max(1.0, xr.grad.abs().max().item()), what="ln bwd")


@pytest.mark.parametrize("rows,F2", [(16 * 4096, 2 * 1280), (16 * 1024, 2 * 2560), (16 * 256, 2 * 5120)])
def test_geglu_fullsize_vs_fp64(rows, F2):
    from gad import ops
    h, hd = hbd(drnd(rows, F2, seed=1))
    hr = hd.clone().requires_grad_(True)
    a, gate = hr.chunk(2, dim=-1)
    y = a * F.gelu(gate)
    dy, dyd = hbd(drnd(rows, F2 // 2, seed=2))
    y.backward(dyd)
    hg = h.clone().requires_grad_(True)
    with recording() as log:
        out = ops.geglu(hg)
        out.backward(dy)
    assert set(log.sigs) == {("geglu", F2)}
    close_h(out, y.detach().cpu(), extra=1e-6, what="geglu fwd")
    close_h(hg.grad, hr.grad.cpu(), extra=1e-6, what="geglu bwd")


# ---------------------------------------------------------------------------------------------------------------
# (f) guard bands at full size: every output and scratch region at exactly its queried size between poisoned bands
# ---------------------------------------------------------------------------------------------------------------
def test_guard_bands_fullsize():
    from gad import half, ops

    def P(t, grad=False):
        return torch.nn.Parameter(t, requires_grad=grad)
    B, H, C1, C2, Cout, k, stride, ups, _ = CONV_FWD["sd512_32x32_640"]
    cx, _, cw, cb, ct, cr = _conv_operands(B, H, C1, C2, Cout, k, stride, ups, dev)
    xo = drnd(16, 64, 64, 320, seed=11).to(BF)
    wo = P(drnd(4, 320, 3, 3, seed=12, scale=0.02).contiguous(memory_format=torch.channels_last))
    dyo = drnd(16, 64, 64, 4, seed=13).to(BF)
    xl, dyl = drnd(65536, 320, seed=14).to(BF), drnd(65536, 320, seed=15).to(BF)
    wl = P(drnd(320, 320, seed=16, scale=0.05))
    q, kk, v = (drnd(16, 4096, 320, seed=i, scale=0.5).to(BF) for i in (17, 18, 19))
    xg_ = drnd(16, 4096, 320, seed=20).to(BF)
    gam, bet = P(drnd(320, seed=21) * 0.1 + 1), P(drnd(320, seed=22) * 0.1)
    torch.manual_seed(0)

    def run():
        outs = [half.conv_fwd_raw(cx, cw, cb, 3, 3, rowadd=ct, residual=cr)]                  # (a) (6, 2): split-K workspace
        xg = xo.clone().requires_grad_(True)                                                  # (b) conv_out: the padded-to-8 dgrad
        y = ops.conv2d(xg, wo, None, None, None, 1, (1, 1, 1, 1), False)
        y.backward(dyo)
        outs += [y.detach(), xg.grad]
        down, up = P(drnd(256, 320, seed=23, scale=0.1), True), P(drnd(320, 256, seed=24, scale=0.1), True)   # (c) G-route, split tn
        xg = xl.clone().requires_grad_(True)
        o = ops.lora_linear(xg, wl, None, down, up, 0.5, None)
        o.backward(dyl)
        outs += [o.detach(), xg.grad, down.grad, up.grad]
        gq, gk, gv = (t.clone().requires_grad_(True) for t in (q, kk, v))                     # (d)
        o = ops.attention_core(gq, gk, gv, 8)
        o.backward(q)
        outs += [o.detach(), gq.grad, gk.grad, gv.grad]
        xg = xg_.clone().requires_grad_(True)                                                 # (e)
        o, al = ops.group_norm_bypass(xg, gam, bet, 32, 1e-5, True)
        torch.autograd.backward([o, al], [xg_, xg_])
        outs += [o.detach(), xg.grad]
        return outs
    got, g = hguarded(run)
    want = run()
    assert len(got) == len(want) and all(torch.equal(a, b) for a, b in zip(got, want))
    assert sum(kind == "ws" for kind, _, _ in g.regions) >= 2


# ---------------------------------------------------------------------------------------------------------------
# (g) the bf16 shadow of the LoRA flat buffer
# ---------------------------------------------------------------------------------------------------------------
def test_shadow_pairs_of_a_flat_buffer():
    from gad import half, ops
    from gad.training import flatten_params
    shapes = [(256, 320), (13,), (320, 256), (3, 5, 1, 1), (256, 768), (24, 320), (7,), (320, 24), (8, 1280)]
    params = [torch.nn.Parameter(drnd(*s, seed=i + 1)) for i, s in enumerate(shapes)]
    params[3] = torch.nn.Parameter(params[3].detach().contiguous(memory_format=torch.channels_last))
    flat, gflat = flatten_params(params)
    offs = [p._gad_flat[1] for p in params]
    assert any(o % 64 for o, s in zip(offs, shapes) if len(s) == 2), offs
    sh, sht = half._flat_pairs(flat)
    fl = flat.detach()

    def check():
        covered = torch.zeros(flat.numel(), dtype=torch.bool, device=dev)
        for p, o, s in zip(params, offs, shapes):
            if len(s) != 2:
                continue
            n = p.numel()
            want = fl[o:o + n].view(s).to(BF)
            assert torch.equal(sh[o:o + n].view(s), want), s
            assert torch.equal(sht[o:o + n].view(s[1], s[0]), want.T), s
            assert torch.equal(half._half_of(p), want) and torch.equal(half._half_t_of(p), want.T)
            covered[o:o + n] = True
        assert not sh[~covered].any() and not sht[~covered].any(), "the shadow wrote outside the 2-D residents"
    check()
    # the raw optimizer rewrites the buffer through a pointer: the next _flat_pairs must carry the new values
    before = fl.clone()
    m, v = torch.zeros_like(flat), torch.zeros_like(flat)
    gflat.copy_(drnd(flat.numel(), seed=99))
    ops.clip_adam_ema_raw(flat, gflat, m, v, None, None, max_norm=0.0, lr=0.05, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0,
                          adamw=True, step=1, ema_decay=0.0)
    torch.cuda.synchronize()
    assert not torch.equal(fl, before)
    sh, sht = half._flat_pairs(flat)
    check()


# ---------------------------------------------------------------------------------------------------------------
# (h) the whole SD U-Net at the bench shape: half path vs fp32 path, and one FusedTrainer step
# ---------------------------------------------------------------------------------------------------------------
def _sd_net(latent):
    import gad
    torch.manual_seed(0)
    with torch.device(dev):
        net = gad.UNet2DConditionModel(sample_size=latent)
    net.to(dev)
    lora = net.inject_lora(rank=256)
    with torch.no_grad():
        for n, p in net.named_parameters():
            if n.endswith("lora_layer.up.weight"):
                p.normal_(0.0, 0.02, generator=torch.Generator(device=dev).manual_seed(len(n)))
    return net, lora


def _sd_inputs(latent, batch, seed=0):
    x, noise = drnd(batch, 4, latent, latent, seed=seed + 1), drnd(batch, 4, latent, latent, seed=seed + 2)
    ctx = drnd(batch, 77, 768, seed=seed + 3)
    t = torch.randint(0, 1000, (batch,), generator=torch.Generator().manual_seed(seed + 4)).to(dev)
    return x, noise, ctx, t


def _fwd_bwd(net, x, t, ctx, noise):
    from gad import ops
    for p in net.parameters():
        p.grad = None
    y = net(x, t, ctx).sample
    _, d = ops.mse_fwd_bwd_raw(y.contiguous(), noise)
    y.backward(d)
    return y.detach().clone(), {n: p.grad.detach().clone() for n, p in net.named_parameters() if p.grad is not None}


class half_path:
    def __enter__(self):
        import gad
        from gad import ops
        gad.set_operand_precision("bf16")
        assert ops.half_activations()

    def __exit__(self, *exc):
        import gad
        gad.set_operand_precision("no")
        return False


def test_sd512_half_vs_fp32_and_one_trainer_step():
    import gad
    net, lora = _sd_net(64)
    x, noise, ctx, t = _sd_inputs(64, 16)
    y32, g32 = _fwd_bwd(net, x, t, ctx, noise)
    with half_path():
        y16, g16 = _fwd_bwd(net, x, t, ctx, noise)
    assert y16.dtype == torch.float32 and set(g16) == set(g32) and len(g16) == 32 * 4 * 2
    e = rel(y16, y32.double())
    assert e < 3e-2, e
    num = sum(((g16[n] - g32[n]).double() ** 2).sum().item() for n in g32)
    den = sum((g32[n].double() ** 2).sum().item() for n in g32)
    assert math.sqrt(num / den) < 8e-2, math.sqrt(num / den)
    for n in g32:
        a, b = g16[n].double().flatten(), g32[n].double().flatten()
        if b.norm() > 1e-3 * math.sqrt(den / len(g32)):
            assert (torch.dot(a, b) / (a.norm() * b.norm())).item() > 0.97, n
    del g32, g16
    # one optimizer step on the half path: the next half forward must see the new LoRA weights (the bf16 shadow is refreshed)
    for p in net.parameters():
        p.grad = None
    sch = gad.DDPMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", num_train_timesteps=1000)
    tr = gad.FusedTrainer(net, sch, None, lr=1e-2, weight_decay=1e-6, adamw=True, max_grad_norm=1.0, params=lora, use_graph=False)
    with half_path(), torch.no_grad():
        pre16 = net(x, t, ctx).sample.clone()                    # (fills the shadow cache of the flat buffer)
    with half_path():
        tr.step(x, noise, t, ctx)
    with torch.no_grad():
        post32 = net(x, t, ctx).sample.clone()
        with half_path():
            post16 = net(x, t, ctx).sample.clone()
    moved = rel(post16, pre16.double())
    assert moved > 0.1, f"the step moved the half-path output by {moved:.3e} only"
    e = rel(post16, post32.double())
    assert e < 3e-2, e


# ---------------------------------------------------------------------------------------------------------------
# (i) coverage: every launch form of a full-size sd512 / sd256 step is one that a case above checks against fp64
# ---------------------------------------------------------------------------------------------------------------
def covered_signatures():
    """what the cases above check, derived on the host (no launch): name of the case for each signature"""
    cov = {}
    for n, row in CONV_FWD.items():
        for s in conv_fwd_sigs(row).sigs:
            cov.setdefault(s, f"conv fwd {n}")
    for n, row in DENSE_FWD.items():
        for s in dense_fwd_sigs(row).sigs:
            cov.setdefault(s, f"dense fwd {n}")
    for n, row in CONV_DGRAD.items():
        for s in conv_dgrad_sigs(row).sigs:
            cov.setdefault(s, f"conv dgrad {n}")
    for n, row in LORA.items():
        for s in lora_sigs(row).sigs:
            cov.setdefault(s, f"lora {n}")
    cov.setdefault(("tn", True), "wgrad_tn")
    for B, Tq, Tk, heads, d in ATTN:
        cov.setdefault(("attn", Tq, Tk, d), "attention")
    for row in GN:
        cov.setdefault(("gn", row[2]), "groupnorm")
    for row in (16 * 4096, 320), (16 * 1024, 640), (16 * 256, 1280), (64 * 16, 1280):
        cov.setdefault(("ln", row[1]), "layernorm")
    for F2 in (2 * 1280, 2 * 2560, 2 * 5120):
        cov.setdefault(("geglu", F2), "geglu")
    return cov


def test_model_launch_forms_are_all_covered():
    cov = covered_signatures()
    missing = {}
    for cfg in (SD512, SD256):
        net, _ = _sd_net(cfg["latent"])
        x, noise, ctx, t = _sd_inputs(cfg["latent"], cfg["batch"])
        with half_path(), recording() as log:
            _fwd_bwd(net, x, t, ctx, noise)
        for s, shape in log.sigs.items():
            if s not in cov:
                missing.setdefault(s, (cfg, shape))
        del net
        torch.cuda.empty_cache()
    assert not missing, "launch forms no case checks against fp64:\n" + "\n".join(f"  {s}: {m}" for s, m in sorted(missing.items(), key=str))
