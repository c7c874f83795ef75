"""gad_gemm's gather side (A_CONV, A_CONVT, B_WDGRAD, B_CONV, the F(2x2) Winograd transforms, the patch / few-output / split
kernels and the epilogues behind them), EXACTLY: integer operands whose every partial sum fp32 (and bf16 rounding) represents
(tests/conv_cases.py, proved on the CPU by tests/test_conv_cases_cpu.py), through the entry points the product uses, compared
with torch.equal against fp64 under every tile hint, split hint, kernel flag and operand precision.  Operands sit between NaN
slack - a padding tap computed as 0 * x[clamped] instead of being masked, or a gather that leaves its tensor, poisons the
output - and outputs between (and, for a channel slice, inside) the finite SENTINEL, which must come back untouched.  Every
launch states the kernel family the host picked: at the row's own hint it must be the route the row names, and always the one
the CPU plan query of the same arguments gives.  F(4x4) Winograd is not exact and is kept out (ops.kernel_flags(no_wino4=True));
it has tests/test_gpu_conv_conditioning.py."""
import ctypes
from contextlib import contextmanager

import pytest
import torch

import conv_cases as CC

pytestmark = pytest.mark.gpu
dev = torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from gad import ops as o
    return o


def recorder(ops):
    class Recorder(ops.GemmProfiler):
        """ops.PROFILER: notes (kernel id, tile, splitk, vec) of every launch, then launches as GemmProfiler does"""

        def __init__(self):
            super().__init__()
            self.plans = []

        def gemm(self, lib, a, batch):
            self.plans.append(CC.plan(a))
            super().gemm(lib, a, batch)
    return Recorder()


@contextmanager
def variant(ops, flags, prec, **more):
    """kernel flags + operand precision + the recorder; F(4x4) off"""
    rec = recorder(ops)
    ops.PROFILER = rec
    try:
        with ops.kernel_flags(no_wino4=True, **{f: True for f in flags}, **more), ops.operand_precision({"bf16": "bf16-operands"}.get(prec, prec)):
            yield rec
    finally:
        ops.PROFILER = None


class Buf:
    """contiguous fp64 values as fp32 in a flat device buffer between `fill` slack"""

    def __init__(self, values, lead=CC.LEAD, fill=float("nan")):
        values = values.contiguous()
        self.lead, self.n = lead, values.numel()
        self.buf = CC.flat(values.float(), lead, fill).to(dev)
        self.orig = self.buf.clone()
        self.t = self.buf[lead:lead + self.n].view(values.shape)

    def untouched(self):
        return torch.equal(self.buf.view(torch.int32), self.orig.view(torch.int32))


class Outputs:
    """ops.OUT_ALLOC: every output the entry points allocate is a view between SENTINEL slack"""

    def __init__(self, lead):
        self.lead, self.given = lead, []

    def __call__(self, shape, device):
        n = 1
        for s in shape:
            n *= s
        buf = torch.full((self.lead + n + CC.SLACK,), CC.SENTINEL, device=device, dtype=torch.float32)
        self.given.append((buf, n))
        return buf[self.lead:self.lead + n].view(shape)

    def slack_untouched(self):
        ok = all(torch.equal(b[:self.lead], torch.full_like(b[:self.lead], CC.SENTINEL)) and
                 torch.equal(b[self.lead + n:], torch.full_like(b[self.lead + n:], CC.SENTINEL)) for b, n in self.given)
        self.given = []
        return ok


@contextmanager
def outputs(ops, lead):
    o = Outputs(lead)
    ops.OUT_ALLOC = o
    try:
        yield o
    finally:
        ops.OUT_ALLOC = None


def describe(got, want):
    bad = torch.nonzero(~(got == want).reshape(-1)).flatten()
    i = bad[:3].tolist()
    return f"{len(bad)} of {got.numel()} differ, first at {i}: got {got.reshape(-1)[i].tolist()} want {want.reshape(-1)[i].tolist()}"


def report(failures):
    assert not failures, f"{len(failures)} launches wrong:\n" + "\n".join(failures[:25])


def weight(t, lead=CC.LEAD):
    """-> (Buf of the [Cout][KH][KW][Cin] storage, the logical [Cout, Cin, KH, KW] view of it)"""
    b = Buf(t["w"].permute(0, 2, 3, 1), lead)
    return b, b.t.permute(0, 3, 1, 2)


class Forward:
    """One row on the device: operands, and the launch through the row's entry point."""

    def __init__(self, ops, row, layout, poison=False):
        self.ops, self.row, self.layout = ops, row, layout
        self.t = t = CC.draw(row)
        self.elead = CC.LEAD + (1 if layout == "off1" else 0)
        x = CC.nhwc(t["x"])
        if poison:                             # pixel (0, 0) of every image: +inf on the device, 0 in the reference
            t["x"][:, :, 0, 0] = 0
            x[:, 0, 0, :] = float("inf")
        if row.entry == "ldx":
            x = CC.pad_pixels(x, row.Cin + row.ldx_pad)
        self.x = Buf(x[..., :row.c1] if row.c1 else x)
        self.x2 = Buf(x[..., row.c1:]) if row.c1 else None
        self.w, self.w_logical = weight(t)
        self.bias, self.rowadd = Buf(t["bias"], self.elead), Buf(t["rowadd"], self.elead)
        self.residual = Buf(CC.nhwc(t["residual"]), self.elead)
        self.inputs = [b for b in (self.x, self.x2, self.w, self.bias, self.rowadd, self.residual) if b is not None]

    def want(self, epi):
        return CC.nhwc(CC.forward(self.row, self.t, epi)).float().to(dev)

    def launch(self, epi, hint, splitk, prec, want):
        """want = self.want(epi) -> (y, expected y, y as [B, Ho, Wo, Cout]): for a krsc row y is the whole wide output, SENTINEL
        outside its channel slice"""
        ops, row = self.ops, self.row
        bias = self.bias.t if epi[0] else None
        rowadd = self.rowadd.t if epi[1] else None
        residual = self.residual.t if epi[2] else None
        if row.entry == "fwd":
            y = ops.conv2d_fwd_raw(self.x.t, self.w_logical, bias, row.stride, row.pad, row.ups, rowadd=rowadd, residual=residual,
                                   tile_hint=hint, splitk_hint=splitk, x2=self.x2.t if self.x2 else None)
            return y, want, y
        if row.entry == "direct":
            y = ops.conv_direct_raw(self.x.t, self.w.t, bias, row.stride, row.pad, row.ups, residual=residual)
            return y, want, y
        if row.entry == "krsc":
            wide = Buf(torch.full((row.B, row.Ho, row.Wo, row.ctot), CC.SENTINEL, dtype=torch.float64), self.elead, CC.SENTINEL)
            expect = wide.buf.clone()
            expect[wide.lead:wide.lead + wide.n].view(wide.t.shape)[..., row.c0:row.c0 + row.Cout] = want
            ops.conv_krsc_raw(self.x.t, self.w.t, bias, row.KH, row.KW, row.stride, row.pad[0], row.pad[2], out=wide.t, c0=row.c0)
            return wide.buf, expect, wide.t[..., row.c0:row.c0 + row.Cout]
        from gad._capi import A_CONV, B_KC, ConvGeom                       # ldx: the convolution's launch with the geometry spelt out
        y = ops._out((row.B, row.Ho, row.Wo, row.Cout), dev)
        Kd = row.KH * row.KW * row.Cin
        three = (row.KH, row.KW, row.stride, row.pad) == (3, 3, 1, CC.P1)
        a = ops.gemm_raw(self.x.t, self.w.t, y, A_CONV, B_KC, row.B * row.Ho * row.Wo, row.Cout, Kd, 0, Kd, row.Cout,
                         geom=ConvGeom(row.H, row.W, row.Cin, row.Cin + row.ldx_pad, row.Ho, row.Wo, row.KH, row.KW, row.stride,
                                       row.pad[0], row.pad[2], int(row.ups)),
                         bias=bias, rowadd=rowadd, rows_per_group=row.Ho * row.Wo, residual=residual, ldr=row.Cout, tile_hint=hint,
                         splitk_hint=splitk, launch=False,
                         B_bf16=ops.bf16_weight(self.w_logical) if (prec == "bf16" and three and row.Cin % 32 == 0) else None)
        scratch = ops._offer_wino(a, dev, self.w_logical, 2 if (three and hint in (0, 7) and splitk == 0) else 0)      # noqa: F841  (held until the launch is enqueued)
        ops._launch_gemm(a, dev)
        return y, want, y


def check_plans(failures, where, rec, mirror, claim=None):
    """every launch of this variant took the kernel family the CPU query names; the row's own launch, the one the row claims"""
    ids = [p[0] for p in rec.plans]
    if not ids or any(i != mirror[0] for i in ids):
        failures.append(f"{where}: launched kernel ids {ids}, the plan query on the same arguments says {mirror}")
    if claim is not None and (mirror[0] != claim[0] or (claim[1] is not None and rec.plans and rec.plans[0][1] != claim[1])):
        failures.append(f"{where}: the row claims (id, tile) {claim}, launched {rec.plans}")


@pytest.mark.parametrize("row", [r for r in CC.INTEGER_ROWS if "fwd" in r.dirs], ids=lambda r: r.label)
def test_forward_is_exact(ops, row):
    """no epilogue and the full one (bias + rowadd per image + residual) x both layouts x every variant"""
    failures = []
    claim = dict(row.claims).get("fwd")
    for layout in row.layouts:
        f = Forward(ops, row, layout)
        with outputs(ops, f.elead) as outs:
            for name, *epi in row.epilogues:
                want_y = f.want(epi)
                for i, (hint, splitk, flags, prec) in enumerate(CC.variants(row)):
                    where = f"{row.label} [{layout} epilogue {name} tile {hint} splitk {splitk} {flags} {prec}]"
                    with variant(ops, flags, prec) as rec:
                        got, want, _ = f.launch(epi, hint, splitk, prec, want_y)
                    own = i == 0 and layout == "aligned" and (name == "none" or row.claim_full)
                    check_plans(failures, where, rec, CC.plan(CC.plan_args(row, "fwd", hint, splitk, flags, prec, epi, layout)),
                                claim if own else None)
                    if not torch.equal(got, want):
                        failures.append(f"{where} plan {rec.plans}: {describe(got, want)}")
                    if not outs.slack_untouched():
                        failures.append(f"{where}: wrote outside its output")
        if not all(b.untouched() for b in f.inputs):
            failures.append(f"{row.label} [{layout}]: an operand buffer changed")
    report(failures)


@pytest.mark.parametrize("row", [r for r in CC.INTEGER_ROWS if "fwd" in r.dirs], ids=lambda r: r.label)
def test_padding_taps_are_masked_not_multiplied_by_zero(ops, row):
    """A padding tap computed as 0 * x[clamped] gives the right number from finite memory, whatever it read.  Here pixel (0, 0) of
    every image - where a masked offset of 0 lands - is +inf: every output whose taps (on the F(2x2) route: whose tile's 4 x 4 input
    window) do not hold that pixel must still be the exact finite value, under every variant."""
    f = Forward(ops, row, "aligned", poison=True)
    ind = torch.zeros(row.B, 1, row.H, row.W, dtype=torch.float64)
    ind[:, :, 0, 0] = 1
    touched = CC.conv_ref(ind, torch.ones(1, 1, row.KH, row.KW, dtype=torch.float64), row.stride, row.pad, row.ups) != 0
    far = (~touched).permute(0, 2, 3, 1).expand(row.B, row.Ho, row.Wo, row.Cout).to(dev)
    edge = 4 if row.ups else 2                 # F(2x2): the tiles whose windows (rows 2 t - 1 .. 2 t + 2) hold the pixel or its nearest-2x copies
    far_wino = far.clone()
    far_wino[:, :edge, :edge, :] = False
    assert far.any() and not far.all() and far_wino.any()
    want = f.want((0, 0, 0))
    assert torch.isfinite(want).all()
    failures = []
    for hint, splitk, flags, prec in CC.variants(row):
        with variant(ops, flags, prec) as rec:
            _, _, y = f.launch((0, 0, 0), hint, splitk, prec, want)
        sel = far_wino if rec.plans[0][0] == 5 else far
        if not torch.equal(y[sel], want[sel]):
            failures.append(f"{row.label} [tile {hint} splitk {splitk} {flags} {prec}] plan {rec.plans}: {describe(y[sel], want[sel])}")
    report(failures)


@pytest.mark.parametrize("row", [r for r in CC.INTEGER_ROWS if "dgrad" in r.dirs], ids=lambda r: r.label)
def test_data_gradient_is_exact(ops, row):
    """ops.conv2d_dgrad_raw (the data-gradient kernels, gad_upsample2x_bwd behind an upsample-fused conv) under every variant,
    and, where ops.dgrad_as_forward holds for a frozen weight, the forward convolution of dy with the rotated weight as
    ops._conv_backward runs it.  Cin % 4 != 0 on the transposed gather is refused with its message."""
    t = CC.draw(row)
    want = CC.nhwc(CC.gradients(row, t)["dx"]).float().to(dev)
    dy, (wb, w) = Buf(CC.nhwc(t["dy"])), weight(t)
    shape = (row.B, row.H, row.W, row.Cin)
    failures = []
    claim = dict(row.claims).get("dgrad")
    one_by_one = (row.KH, row.KW, row.pad) == (1, 1, CC.P0)
    if row.Cin % 4 != 0 and not one_by_one:
        from gad._capi import GadError
        with pytest.raises(GadError, match=CC.REFUSALS["dgrad-cin%4"]):
            ops.conv2d_dgrad_raw(dy.t, w, shape, row.stride, row.pad, row.ups)
        return
    with outputs(ops, CC.LEAD) as outs:
        for i, (hint, splitk, flags, prec) in enumerate(CC.variants(row, "dgrad")):
            where = f"{row.label} dgrad [tile {hint} splitk {splitk} {flags} {prec}]"
            with variant(ops, flags, prec, native_dgrad=True) as rec:
                got = ops.conv2d_dgrad_raw(dy.t, w, shape, row.stride, row.pad, row.ups, tile_hint=hint, splitk_hint=splitk)
            check_plans(failures, where, rec, CC.plan(CC.plan_args(row, "dgrad", hint, splitk, flags, prec)), claim if i == 0 else None)
            if not torch.equal(got, want):
                failures.append(f"{where} plan {rec.plans}: {describe(got, want)}")
            if not outs.slack_untouched():
                failures.append(f"{where}: wrote outside its output")
        assert ops.dgrad_as_forward(w, row.stride, row.pad) == CC.dgrad_as_forward(row)
        if CC.dgrad_as_forward(row):
            for flags in CC.FLAG_SETS:
                for prec in CC.PRECISIONS:
                    where = f"{row.label} dgrad as forward [{flags} {prec}]"
                    with variant(ops, flags, prec) as rec:
                        got = ops.conv2d_fwd_raw(dy.t, ops.rotated_weight(w), None)
                        if row.ups:
                            got = ops._upsample2x_bwd(got, shape)
                    check_plans(failures, where, rec, CC.plan(CC.plan_args(row, "dgrad", flags=flags, prec=prec, as_forward=True)))
                    if not torch.equal(got, want):
                        failures.append(f"{where} plan {rec.plans}: {describe(got, want)}")
                    if not outs.slack_untouched():
                        failures.append(f"{where}: wrote outside its output")
    if not (dy.untouched() and wb.untouched()):
        failures.append(f"{row.label}: an operand buffer changed")
    report(failures)


@pytest.mark.parametrize("row", [r for r in CC.INTEGER_ROWS if "wgrad" in r.dirs], ids=lambda r: r.label)
def test_weight_gradient_and_column_sums_are_exact(ops, row):
    """ops.conv2d_wgrad_raw on the engine, the patch kernel (128 / 96 / 64 / 32-channel tiles) and the M split, and ops.colsum_raw
    (the bias gradient) of the same dy."""
    t = CC.draw(row)
    g = CC.gradients(row, t)
    want = g["dw"].float().to(dev)
    dy, x, (_, w) = Buf(CC.nhwc(t["dy"])), Buf(CC.nhwc(t["x"])), weight(t)
    failures = []
    claims = {row.hint: dict(row.claims).get("wgrad"), **dict(row.wgrad_hints)}
    with outputs(ops, CC.LEAD) as outs:
        for i, (hint, splitk, flags, prec) in enumerate(CC.variants(row, "wgrad")):
            where = f"{row.label} wgrad [tile {hint} splitk {splitk} {flags} {prec}]"
            with variant(ops, flags, prec) as rec:
                got = ops.conv2d_wgrad_raw(dy.t, x.t, w, row.stride, row.pad, row.ups, tile_hint=hint, splitk_hint=splitk)
            own = (i == 0 or hint in dict(row.wgrad_hints)) and splitk == 0 and not flags and prec == row.prec
            check_plans(failures, where, rec, CC.plan(CC.plan_args(row, "wgrad", hint, splitk, flags, prec)), claims.get(hint) if own else None)
            if not torch.equal(got, want):
                failures.append(f"{where} plan {rec.plans}: {describe(got, want)}")
            if not outs.slack_untouched():
                failures.append(f"{where}: wrote outside its output")
    db = ops.colsum_raw(dy.t.view(-1, row.Cout), 1).view(-1)
    if not torch.equal(db, g["dbias"].float().to(dev)):
        failures.append(f"{row.label} colsum: {describe(db, g['dbias'].float().to(dev))}")
    if not (dy.untouched() and x.untouched()):
        failures.append(f"{row.label}: an operand buffer changed")
    report(failures)


def test_an_operand_off_the_16_byte_grid_is_refused(ops):
    """gad_gemm reads A and B as float4 wherever the shapes allow: an x one float off the grid is refused before anything runs"""
    from gad._capi import GadError
    row = CC.ROWS["down-asym-pad"]
    t = CC.draw(row)
    x, (_, w) = Buf(CC.nhwc(t["x"]), CC.LEAD + 1), weight(t)
    with pytest.raises(GadError, match=CC.REFUSALS["x-off-grid"]):
        ops.conv2d_fwd_raw(x.t, w, None, row.stride, row.pad, row.ups)
    wb, w1 = weight(t, CC.LEAD + 1)
    with pytest.raises(GadError, match=CC.REFUSALS["x-off-grid"]):
        ops.conv2d_fwd_raw(Buf(CC.nhwc(t["x"])).t, w1, None, row.stride, row.pad, row.ups)


def test_library_and_cpu_query_are_the_same_build(ops):
    """the plan mirror runs the loaded library's own queries: nothing here is a second planner"""
    from gad import _capi
    a = CC.plan_args(CC.ROWS["route-fewout"])
    assert _capi.load().gad_gemm_kernel_id(ctypes.byref(a)) == 4
