"""The convolution cases themselves (tests/conv_cases.py), without a GPU: exactness of the integer cases belongs to the
inputs, not to a kernel; every row takes the route it claims (the host's own plan queries on placeholder pointers); the
edge table is whole; the Winograd emulations are the convolution; every conditioning case has a usable yardstick."""
import ctypes

import pytest
import torch

import conv_cases as CC


@pytest.fixture(scope="module")
def lib():
    from gad import _capi
    return _capi.load()


@pytest.mark.parametrize("row", CC.INTEGER_ROWS, ids=lambda r: r.label)
def test_integer_cases_are_exact_in_fp32(row):
    """fp32 torch on the CPU - direct convolution, the F(2x2) emulation where the row is a Winograd one, autograd for the
    gradients - equals fp64 bit for bit, and bf16 rounding of the operands changes nothing."""
    t = CC.draw(row)
    for k in ("x", "w", "dy"):
        assert torch.equal(t[k].float().to(torch.bfloat16).double(), t[k]), k
    for _, *epi in row.epilogues:
        want = CC.forward(row, t, epi)
        assert want.abs().max() < 2 ** 22
        assert torch.equal(CC.forward(row, t, epi, torch.float32).double(), want), (row.label, epi)
        if row.wscale == 4:
            got = CC.forward(row, t, epi, torch.float32, conv=lambda x, w: CC.wino_forward(x, w, 2, row.ups))
            assert torch.equal(got.double(), want), (row.label, epi, "F(2x2)")
    if len(row.dirs) > 1 or row.dirs != ("fwd",):
        want, got = CC.gradients(row, t), CC.gradients(row, t, torch.float32)
        for k in want:
            assert want[k].abs().max() < 2 ** 23 and torch.equal(got[k].double(), want[k]), (row.label, k)


def test_f2x2_weights_keep_the_transform_integral():
    """G w G^T of w in 4 * {-2..2} is integral: the reason the F(2x2) rows draw their weights from that set"""
    _, G, _ = CC._mats(2, torch.float64)
    w = 4 * torch.randint(-2, 3, (64, 32, 3, 3), generator=torch.Generator().manual_seed(0)).double()
    U = G @ w @ G.T
    assert torch.equal(U, U.round())


@pytest.mark.parametrize("row", CC.INTEGER_ROWS, ids=lambda r: r.label)
def test_rows_take_the_route_they_claim(lib, row):
    claims = dict(row.claims)
    assert set(claims) <= set(row.dirs)
    for direction, (kid, tile) in claims.items():
        for name, *epi in (row.epilogues if (direction == "fwd" and row.claim_full) else row.epilogues[:1]):
            got = CC.plan(CC.plan_args(row, direction, epilogue=epi if direction == "fwd" else (0, 0, 0)))
            assert got[0] == kid and (tile is None or got[1] == tile), (row.label, direction, name, got)
    for hint, (kid, tile) in row.wgrad_hints:
        got = CC.plan(CC.plan_args(row, "wgrad", hint=hint))
        assert got[:2] == (kid, tile), (row.label, hint, got)


def test_every_kernel_family_has_a_case(lib):
    """kernel ids 0 .. 5 among the integer rows (forward or gradient); 6 and 7 - F(4x4) forward and weight gradient, not exact -
    among the conditioning launches"""
    ids = set()
    for row in CC.INTEGER_ROWS:
        for direction, (kid, _) in row.claims:
            ids.add(kid)
    assert ids >= {0, 1, 2, 3, 4, 5}, ids
    B, Ci, Co, H, W = CC.COND_SHAPES["64"]
    row = CC._r("cond", B, Ci, Co, H, W, 3, 3, 1, CC.P1)
    forms = {hint: CC.plan(CC.plan_args(row, "fwd", hint=hint, no_wino4=False)) for hint in (8, 9, 10, 11)}
    assert all(v[0] == 6 for v in forms.values()), forms
    assert forms[9][1] == 32 and forms[10][1] == 128 and forms[11][1] == 64, forms
    assert CC.plan(CC.plan_args(row, "wgrad", hint=8, no_wino4=False))[0] == 7
    # the six-position product kernel: the three-launch form at >= 1024 product blocks has 24 panels, not 36 (wino_bytes says)
    B, Ci, Co, H, W = CC.SIX_POSITION_SHAPE
    big = CC.plan_args(CC._r("six", B, Ci, Co, H, W, 3, 3, 1, CC.P1), "fwd", hint=10, no_wino4=False)
    T = B * H * W // 16
    assert CC.plan(big)[0] == 6 and lib.gad_gemm_wino_bytes(ctypes.byref(big)) == 4 * (36 * T * Ci + 24 * T * Co)
    small = CC.plan_args(CC._r("six-1", B - 1, Ci, Co, H, W, 3, 3, 1, CC.P1), "fwd", hint=10, no_wino4=False)          # 170 x 1 x 6 < 1024 blocks
    T = (B - 1) * H * W // 16
    assert lib.gad_gemm_wino_bytes(ctypes.byref(small)) == 4 * (36 * T * Ci + 36 * T * Co)
    # ... and on its (128 tiles x 64 channels) blocks: 171 x 1 x 6 = 1026 blocks
    B, Ci, Co, H, W = CC.SIX_POSITION_SHAPE_128x64
    big = CC.plan_args(CC._r("six-128x64", B, Ci, Co, H, W, 3, 3, 1, CC.P1), "fwd", hint=10, no_wino4=False)
    T = B * H * W // 16
    assert -(-T // 128) * -(-Co // 64) * 6 == 1026
    assert CC.plan(big)[0] == 6 and lib.gad_gemm_wino_bytes(ctypes.byref(big)) == 4 * (36 * T * Ci + 24 * T * Co)


def test_the_edge_table_is_whole():
    """The cap that keeps a skip from hollowing the suite out: every row of the table is present for every direction it names
    (the GPU tests run every row x direction x variant and skip none)."""
    have = {(r.B, r.Cin, r.Cout, r.H, r.W, r.KH, r.KW, r.stride, r.pad, r.ups, r.entry): r for r in reversed(CC.EDGE_ROWS)}

    def has(*key, entry="fwd", dirs=("fwd",), **kw):
        r = have.get((*key, entry))
        assert r is not None and set(dirs) <= set(r.dirs), key
        for k, v in kw.items():
            assert getattr(r, k) == v, (key, k)
    all3 = ("fwd", "dgrad", "wgrad")
    has(3, 5, 7, 7, 5, 3, 3, 1, CC.P1, False, dirs=all3)
    has(2, 3, 128, 6, 5, 3, 3, 1, CC.P1, False, dirs=all3)
    for co in (1, 3, 4):
        has(2, 8, co, 6, 5, 3, 3, 1, CC.P1, False, dirs=all3)
    has(2, 36, 68, 9, 6, 3, 3, 2, (0, 1, 0, 1), False, dirs=all3)
    has(2, 36, 68, 9, 6, 3, 3, 2, CC.P1, False, dirs=all3)
    has(2, 32, 40, 5, 3, 3, 3, 1, CC.P1, True, dirs=all3)
    has(2, 32, 40, 6, 10, 1, 1, 1, CC.P0, False, dirs=all3)
    labels = set(CC.ROWS)
    for k in ("1x1", "3x3"):
        assert {f"{k}-two-source-32+64", f"{k}-two-source-96+32"} <= labels
    assert (CC.ROWS["1x1-two-source-32+64"].c1, CC.ROWS["1x1-two-source-96+32"].c1) == (32, 96)
    for form in ("1x7", "7x1", "1x3", "3x1", "5x5", "3x3s2p0"):
        for c0 in (20, 21):
            r = CC.ROWS[f"krsc-{form}-c0={c0}"]
            assert r.entry == "krsc" and r.c0 == c0 and r.ctot > c0 + r.Cout
    assert CC.ROWS["krsc-1x7-c0=20"].pad == (0, 0, 3, 3) and CC.ROWS["krsc-7x1-c0=20"].pad == (3, 3, 0, 0)
    assert CC.ROWS["krsc-5x5-c0=20"].pad == (2, 2, 2, 2) and (CC.ROWS["krsc-3x3s2p0-c0=20"].H, CC.ROWS["krsc-3x3s2p0-c0=20"].Ho) == (15, 7)
    has(2, 36, 68, 9, 6, 3, 3, 2, (0, 1, 0, 1), False, entry="direct")
    assert {r.ldx_pad for r in CC.INTEGER_ROWS if r.entry == "ldx"} == {1, 4}
    assert any(r.B * r.Ho * r.Wo < 64 for r in CC.INTEGER_ROWS)
    routes = {"route-patch-f32", "route-patch-bf16", "route-fewout", "route-wgrad-patch", "route-split-m", "route-split-n",
              "route-wino2-128x64", "route-wino2-cout68", "route-wino2-upsample"}
    assert routes <= labels
    assert dict(CC.ROWS["route-wgrad-patch"].wgrad_hints).keys() == {4, 5, 6} and CC.ROWS["route-wgrad-patch"].hint == 1
    assert CC.ROWS["route-split-m"].hint == 1000 + 128
    for r in CC.INTEGER_ROWS:                  # every row: no epilogue and the fullest its entry point passes; the whole cross of variants
        assert [e[0] for e in r.epilogues] == ["none", "full"]
        n = len(CC.variants(r))
        assert n >= (10 if r.entry in ("krsc", "direct") else 90), (r.label, n)


def test_variants_change_the_route_but_are_never_refused(lib):
    """Hints and flags move a launch between routes (that is their purpose); the plan query answers for every one of them."""
    for row in CC.ROUTE_ROWS:
        direction = row.dirs[0]
        seen = {CC.plan(CC.plan_args(row, direction, hint=t, splitk=s, flags=f, prec=p))[0] for t, s, f, p in CC.variants(row, direction)}
        assert dict(row.claims)[direction][0] in seen and all(0 <= k <= 7 for k in seen), (row.label, seen)


@pytest.mark.parametrize("f", [2, 4])
def test_winograd_emulations_are_the_convolution(f):
    """fp64: to rounding (1e-12); fp32 on randn: F(2x2) within a few times the direct fp32 error, F(4x4) about a decimal digit
    above it (its transforms amplify by up to 8 x 8 on the way out)"""
    g = torch.Generator().manual_seed(3)
    x, w = torch.randn(2, 32, 8, 12, generator=g), torch.randn(36, 32, 3, 3, generator=g) / 17
    want = CC.conv_ref(x.double(), w.double())
    assert CC._max_err(CC.wino_forward(x.double(), w.double(), f), want) < 1e-12
    assert CC._max_err(CC.wino_forward(x.double(), w.double(), f, ups=True), CC.conv_ref(x.double(), w.double(), ups=True)) < 1e-12
    e_direct, e_wino = CC._max_err(CC.conv_ref(x, w), want), CC._max_err(CC.wino_forward(x, w, f), want)
    assert e_direct < 1e-5 and e_wino < (8 if f == 2 else 40) * e_direct, (e_direct, e_wino)


def test_winograd_weight_gradient_emulation_is_the_gradient():
    g = torch.Generator().manual_seed(4)
    x, dy = torch.randn(2, 32, 8, 12, generator=g), torch.randn(2, 36, 8, 12, generator=g)
    want, e_direct = CC.cond_wgrad_reference(x, dy, "direct")
    assert CC._max_err(CC.wino4_wgrad(x.double(), dy.double()), want) < 1e-11
    _, e_wino = CC.cond_wgrad_reference(x, dy, "wino4")
    assert e_direct < 1e-4 and e_wino < 40 * e_direct, (e_direct, e_wino)


@pytest.mark.parametrize("name", CC.COND_NAMES)
def test_conditioning_cases_have_a_yardstick(name):
    for shape in CC.COND_SHAPES.values():
        x, w = CC.cond_inputs(name, shape)
        assert x.dtype == torch.float32 and x.shape == (shape[0], shape[1], shape[3], shape[4]) and torch.isfinite(x).all()
        for algorithm in ("direct", "wino2", "wino4"):
            want, e_ref = CC.cond_forward_reference(x, w, algorithm)
            assert e_ref == e_ref and e_ref < float("inf") and CC.bound(e_ref, want) > 0, (name, algorithm)
            print(CC.figure(want.float(), want, e_ref, f"{name} {shape[2]} {algorithm} (fp32 rounding of want)")[2])
    if name == "constant":
        exp = CC.constant_expected(w)
        assert CC._max_err(want[0, :, 5, 5], exp[:, 1, 1]) < 1e-9 and CC._max_err(want[0, :, 0, 15], exp[:, 0, 2]) < 1e-9
    if name == "spike":
        x0, w0 = CC.cond_inputs("spike_removed", CC.COND_SHAPES["64"])
        x1, w1 = CC.cond_inputs("spike", CC.COND_SHAPES["64"])
        diff = (x0 != x1).any(1).any(0)
        assert torch.equal(w0, w1) and diff.sum() == len(CC.SPIKES) and all(diff[r, c] for r, c in CC.SPIKES)
        assert all(abs(x1[0, 0, r, c]) == 1000 for r, c in CC.SPIKES)


def test_conditioning_weight_gradient_yardsticks():
    shape = CC.COND_SHAPES["64"]
    for name in ("randn", "silu", "spike"):
        x, _ = CC.cond_inputs(name, shape)
        dy = torch.randn(shape[0], shape[2], shape[3], shape[4], generator=torch.Generator().manual_seed(5))
        for algorithm in ("direct", "wino4"):
            want, e_ref = CC.cond_wgrad_reference(x, dy, algorithm)
            assert 0 < e_ref < float("inf") and CC.bound(e_ref, want) > 0
