"""The host side of the convolution launches, without a GPU: what gad/ops.py launches and asks the library for each case of
tests/conv_launch_trace.py is what tests/golden/conv_launch_trace.json recorded before the launch wrappers were refactored -
the same launches in the same order with every argument field equal, and no more route queries than then."""
import json
import os

import pytest

import conv_launch_trace as T
from gad import _capi


@pytest.fixture(scope="module")
def recorded(golden_dir):
    with open(os.path.join(golden_dir, "conv_launch_trace.json")) as f:
        return json.load(f)["cases"]


def test_the_recorded_trace_has_every_case(recorded):
    assert sorted(recorded) == sorted(name for name, _, _ in T.CASES)


def _describe(got, want):
    """the first field that differs, by name where the argument is a struct"""
    if got[0] != want[0] or len(got) != len(want):
        return f"{got[0]} ({len(got)} arguments) != {want[0]} ({len(want)})"
    types = _capi.SIGNATURES.get(got[0], (None, []))[1]
    for i, (g, w) in enumerate(zip(got[1:], want[1:])):
        if g == w:
            continue
        t = types[i] if i < len(types) else None
        if isinstance(g, list) and isinstance(w, list) and len(g) == len(w) and t is not None and hasattr(t, "_type_"):
            fields = [f for f, _ in t._type_._fields_]
            return f"{got[0]}: " + ", ".join(f"{f} {a} != {b}" for f, a, b in zip(fields, g, w) if a != b)
        return f"{got[0]} argument {i}: {g} != {w}"
    return "equal"


@pytest.mark.parametrize("name,fn,hooked", T.CASES, ids=[name for name, _, _ in T.CASES])
def test_launches_match_the_recorded_trace(recorded, name, fn, hooked):
    got = json.loads(json.dumps(T.run_case(_capi.load(), fn, hooked)))
    want = recorded[name]
    assert [l[0] for l in got["launches"]] == [l[0] for l in want["launches"]]
    for g, w in zip(got["launches"], want["launches"]):
        assert g == w, _describe(g, w)
    assert got.get("route_stats") == want.get("route_stats")
    assert set(got["queries"]) <= set(want["queries"]), (got["queries"], want["queries"])
    for q, n in got["queries"].items():
        assert n <= want["queries"][q], (got["queries"], want["queries"])


def test_the_prefilter_never_withholds_what_the_planner_would_take():
    """Over the forward-convolution rows of the route grid (tests/test_capi_cpu.py), with the row's switches and operand
    precision set: where ops.wino_prefilter offers no Winograd form, the library - offered BOTH forms - must not route the
    launch to a Winograd kernel (ids 5, 6).  The pre-filter only saves work; it must not change a route."""
    import ctypes

    from gad import ops
    from test_capi_cpu import _P, gemm_route_grid
    lib, bad, none, taken, rows = _capi.load(), [], 0, 0, 0
    for a in gemm_route_grid():
        if (a.a_mode, a.b_mode) != (_capi.A_CONV, _capi.B_KC):
            continue
        g = a.g
        with ops.kernel_flags():
            ops.KERNEL_FLAGS["gemm"] = a.flags
            ops.OPERAND_PRECISION[0], prec = a.operand_precision, ops.OPERAND_PRECISION[0]
            try:
                form = ops.wino_prefilter((g.KH, g.KW), g.stride, (g.pad_t, g.pad_t, g.pad_l, g.pad_l), bool(a.A2), a.N, g.C, (g.Ho, g.Wo),
                                          a.tile_hint, a.splitk_hint)[0]
            finally:
                ops.OPERAND_PRECISION[0] = prec
        a.B_wino, a.B_wino4 = 7 * _P, 8 * _P
        kid = lib.gad_gemm_kernel_id(ctypes.byref(a))
        rows += 1
        none += form == 0
        taken += kid in (5, 6)
        if form == 0 and kid in (5, 6):
            bad.append(((g.H, g.W, g.C, g.Ho, g.Wo, g.KH, g.stride, g.pad_t, g.upsample, a.M, a.N, a.tile_hint, a.splitk_hint,
                         a.operand_precision, a.flags), kid))
    assert rows > 10000 and 0 < none < rows and taken > 100
    assert not bad, f"{len(bad)} rows: the pre-filter offers nothing, the planner would take {bad[:10]}"
