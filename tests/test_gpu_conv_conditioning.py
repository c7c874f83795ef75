"""The convolution routes that are NOT exact - Winograd F(4x4, 3x3) forward in its four forms (tile hints 8 .. 11), its weight
gradient, F(2x2) - and the direct routes as the baseline, on the inputs the network feeds: post-GroupNorm SiLU activations,
a mean far from zero, one hot channel, one large pixel, a zero-sum filter on a smooth ramp, a constant (tests/conv_cases.py;
the yardsticks are proved usable on the CPU by tests/test_conv_cases_cpu.py).

The bound, as in tests/norm_cases.py:  max |got - fp64| <= K * max(e_ref, 2^-22 max |fp64|), K = 8, e_ref = the error of an
fp32 CPU run of the same algorithm on the same inputs (F.conv2d / autograd; the torch emulation of the standard transforms).
Every figure is printed before it is asserted; profiles/conv_conditioning.txt holds the figures measured on the MI355X.

Beyond the bound: locality - removing a 1000-fold pixel changes no bit of any output whose taps (direct routes) or whose
tile's input window (Winograd) do not hold it; a constant input gives the interior, the four borders and the four corners
their own partial tap sums; the F(4x4) weight gradient is the same bits with and without the kept input image."""
import pytest
import torch

import conv_cases as CC

pytestmark = pytest.mark.gpu
dev = torch.device("cuda:0")

# name -> (tile hint, split hint, kernel flags, kernel id, algorithm whose fp32 CPU run is the yardstick)
ROUTES = {
    "engine-128": (1, 0, dict(no_wino=True), 0, "direct"),
    "engine-64": (2, 0, dict(no_wino=True), 0, "direct"),
    "engine-64-splitk2": (2, 2, dict(no_wino=True), 0, "direct"),
    "wino2": (7, 0, {}, 5, "wino2"),
    "wino4-planned": (8, 0, {}, 6, "wino4"),
    "wino4-fused32": (9, 0, {}, 6, "wino4"),
    "wino4-three-launch": (10, 0, {}, 6, "wino4"),
    "wino4-fused64": (11, 0, {}, 6, "wino4"),
}
_REF = {}


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from gad import ops as o
    return o


def reference(name, shape_key, algorithm):
    """computed once, shared, left unchanged"""
    key = (name, shape_key, algorithm)
    if key not in _REF:
        shape = CC.COND_SHAPES.get(shape_key) or CC.SIX_POSITION_SHAPES[shape_key]
        _REF[key] = CC.cond_forward_reference(*CC.cond_inputs(name, shape), algorithm)
    return _REF[key]


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous().to(dev)


def cl_weight(w):
    return w.to(dev).contiguous(memory_format=torch.channels_last)


def run(ops, x, w, route):
    """-> y [B, Cout, H, W] on the CPU; asserts the kernel family"""
    hint, splitk, flags, kid, _ = ROUTES[route]
    ops.PROFILER = prof = ops.GemmProfiler()
    try:
        with ops.kernel_flags(**flags):
            y = ops.conv2d_fwd_raw(nhwc(x), cl_weight(w), None, 1, CC.P1, False, tile_hint=hint, splitk_hint=splitk)
        torch.cuda.synchronize()
    finally:
        ops.PROFILER = None
    names = [k[0] for k in prof.summary()]
    assert names == [{0: "conv_fwd", 5: "conv_fwd_wino", 6: "conv_fwd_wino4"}[kid]], (route, names)
    return y.permute(0, 3, 1, 2).cpu()


@pytest.mark.parametrize("shape_key", list(CC.COND_SHAPES))
@pytest.mark.parametrize("name", CC.COND_NAMES)
def test_every_route_is_inside_the_bound(ops, name, shape_key):
    x, w = CC.cond_inputs(name, CC.COND_SHAPES[shape_key])
    bad = []
    for route in ROUTES:
        want, e_ref = reference(name, shape_key, ROUTES[route][4])
        err, b, line = CC.figure(run(ops, x, w, route), want, e_ref, f"COND fwd {route} {name} Cout={shape_key}")
        print(line, flush=True)
        if not err <= b:
            bad.append(line)
    assert not bad, "outside K * max(e_ref, 2^-22 max|want|):\n" + "\n".join(bad)


def six_position(ops, name, shape_key):
    shape = CC.SIX_POSITION_SHAPES[shape_key]
    x, w = CC.cond_inputs(name, shape)
    T = shape[0] * shape[3] * shape[4] // 16
    from gad import _capi
    import ctypes
    a = CC.plan_args(CC._r(shape_key, *shape, 3, 3, 1, CC.P1), "fwd", hint=10, no_wino4=False)
    assert _capi.load().gad_gemm_kernel_id(ctypes.byref(a)) == 6
    assert _capi.load().gad_gemm_wino_bytes(ctypes.byref(a)) == 4 * (36 * T * shape[1] + 24 * T * shape[2])
    want, e_ref = reference(name, shape_key, "wino4")
    err, b, line = CC.figure(run(ops, x, w, "wino4-three-launch"), want, e_ref, f"COND fwd wino4-six-position {name} {shape}")
    print(line, flush=True)
    assert err <= b, line


@pytest.mark.parametrize("name", ["randn", "spike"])
def test_six_position_product_kernel_is_inside_the_bound(ops, name):
    """the three-launch F(4x4) form at >= 1024 product blocks: 24 half-transformed panels instead of 36 products"""
    six_position(ops, name, "six")


@pytest.mark.parametrize("name", ["randn", "spike"])
def test_six_position_product_kernel_on_128x64_blocks_is_inside_the_bound(ops, name):
    """the same on (128 tiles x 64 channels) blocks: Cout = 64 (conv_cases.SIX_POSITION_SHAPE_128x64 derives the plan)"""
    six_position(ops, name, "six-128x64")


def _window_mask(H, W, f):
    """[H, W] bool: outputs whose dependence on a spike pixel is possible - f = 0: the 3x3 taps (direct routes); f = 2 / 4: the
    (f + 2)^2 input window of the output's f x f tile"""
    m = torch.zeros(H, W, dtype=torch.bool)
    for r, c in CC.SPIKES:
        for i in range(H):
            for j in range(W):
                if f == 0:
                    hit = abs(i - r) <= 1 and abs(j - c) <= 1
                else:
                    ti, tj = i // f * f, j // f * f
                    hit = ti - 1 <= r <= ti + f and tj - 1 <= c <= tj + f
                m[i, j] |= hit
    return m


@pytest.mark.parametrize("route", list(ROUTES))
def test_a_large_pixel_stays_local(ops, route):
    shape = CC.COND_SHAPES["68"]
    x1, w = CC.cond_inputs("spike", shape)
    x0, _ = CC.cond_inputs("spike_removed", shape)
    y1, y0 = run(ops, x1, w, route), run(ops, x0, w, route)
    far = ~_window_mask(shape[3], shape[4], {"direct": 0, "wino2": 2, "wino4": 4}[ROUTES[route][4]])
    assert far.sum() > 100
    assert torch.equal(y1[:, :, far], y0[:, :, far]), f"{route}: {(y1 != y0)[:, :, far].sum().item()} far outputs changed"
    assert not torch.equal(y1, y0)


@pytest.mark.parametrize("route", list(ROUTES))
def test_constant_input_gives_the_partial_tap_sums(ops, route):
    shape = CC.COND_SHAPES["68"]
    x, w = CC.cond_inputs("constant", shape)
    want, e_ref = reference("constant", "68", ROUTES[route][4])
    b = CC.bound(e_ref, want)
    y = run(ops, x, w, route).double()
    exp = CC.constant_expected(w)                              # [Cout, 3, 3]
    H, W = shape[3], shape[4]
    rc = torch.ones(H, dtype=torch.long)
    rc[0], rc[-1] = 0, 2
    cc = torch.ones(W, dtype=torch.long)
    cc[0], cc[-1] = 0, 2
    full = exp[:, rc][:, :, cc]                                # [Cout, H, W]
    worst = {}
    for name, (rs, cs) in {"interior": (1, 1), "top": (0, 1), "bottom": (2, 1), "left": (1, 0), "right": (1, 2), "top-left": (0, 0),
                           "top-right": (0, 2), "bottom-left": (2, 0), "bottom-right": (2, 2)}.items():
        sel = (rc == rs)[:, None] & (cc == cs)[None, :]
        worst[name] = (y[:, :, sel] - full[None][:, :, sel]).abs().max().item()
    print(f"COND constant {route}: bound {b:.3e} worst per class {worst}", flush=True)
    assert all(v <= b for v in worst.values()), (b, worst)


@pytest.mark.parametrize("name", ["randn", "silu", "spike"])
def test_winograd_weight_gradient_is_inside_the_bound_with_and_without_the_kept_image(ops, name):
    shape = CC.COND_SHAPES["64"]
    B, Ci, Co, H, W = shape
    x, w = CC.cond_inputs(name, shape)
    dy = torch.randn(B, Co, H, W, generator=torch.Generator().manual_seed(5))
    xg, dyg, wg = nhwc(x), nhwc(dy), cl_weight(w)
    keep = []
    ops.conv2d_fwd_raw(xg, wg, None, 1, CC.P1, False, tile_hint=9, keep_v=keep)
    assert len(keep) == 1
    ops.PROFILER = prof = ops.GemmProfiler()
    try:
        dw = ops.conv2d_wgrad_raw(dyg, xg, wg, 1, CC.P1, False, tile_hint=8)
        dw_v = ops.conv2d_wgrad_raw(dyg, xg, wg, 1, CC.P1, False, tile_hint=8, wino_v=keep[0])
        torch.cuda.synchronize()
    finally:
        ops.PROFILER = None
    assert [k[0] for k in prof.summary()] == ["conv_wgrad_wino4"], list(prof.summary())
    assert torch.equal(dw, dw_v)
    with ops.kernel_flags(no_wino=True):
        dw_direct = ops.conv2d_wgrad_raw(dyg, xg, wg, 1, CC.P1, False)
    bad = []
    for label, got, algorithm in (("wino4", dw, "wino4"), ("wino4-kept-image", dw_v, "wino4"), ("direct", dw_direct, "direct")):
        want, e_ref = CC.cond_wgrad_reference(x, dy, algorithm)
        err, b, line = CC.figure(got.cpu(), want, e_ref, f"COND wgrad {label} {name}")
        print(line, flush=True)
        if not err <= b:
            bad.append(line)
    assert not bad, "outside K * max(e_ref, 2^-22 max|want|):\n" + "\n".join(bad)
