"""gad_gemm's generic engine (csrc/gemm_f32.hip: gemm_kernel, gemm_bf16_kernel, splitk_reduce_kernel; csrc/gemm_dev.h: store_block) on padded,
batched and misaligned operands, EXACTLY: integer operands whose every partial sum fp32 (and bf16 rounding) represents, the
whole output buffer - row padding, gaps between batch slabs, floats before an offset pointer - compared with torch.equal
against the CPU restatement of the ABI (tests/gemm_ref.py; cases: tests/gemm_cases.py, checked on the CPU by
tests/test_gemm_abi_cpu.py).  Operand padding is NaN: a kernel that multiplies padding instead of masking it poisons its
output.  Every launch first states which instance the host picked (gad_gemm_plan / _kernel_id / _uses_bf16 /
_workspace_bytes) and is not run when that is not the instance the case is about."""
import ctypes
import math
from contextlib import contextmanager

import pytest
import torch

import gemm_cases as GC
import gemm_ref as R

pytestmark = pytest.mark.gpu
dev = torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from gad import ops as o
    return o


class Recorder:
    """Stands in for ops.PROFILER: gemm_raw hands it the finished GemmArgs.  It asks the host what the launch will run,
    lets `expect(record)` refuse it, and only then launches."""

    def __init__(self, ops, expect=None):
        self.ops, self.expect, self.records = ops, expect, []

    def gemm(self, lib, a, batch):
        from gad._capi import check
        tile, sk, vec = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        check(lib.gad_gemm_plan(ctypes.byref(a), ctypes.byref(tile), ctypes.byref(sk), ctypes.byref(vec)), "gad_gemm_plan")
        rec = dict(tile=tile.value, splitk=sk.value, vec=vec.value, kernel_id=lib.gad_gemm_kernel_id(ctypes.byref(a)),
                   uses_bf16=lib.gad_gemm_uses_bf16(ctypes.byref(a)), ws_bytes=lib.gad_gemm_workspace_bytes(ctypes.byref(a)))
        self.records.append(rec)
        if self.expect is not None:
            self.expect(rec)
        check(lib.gad_gemm(ctypes.byref(a), self.ops._stream()), "gad_gemm")


@contextmanager
def recording(ops, expect=None):
    rec = Recorder(ops, expect)
    ops.PROFILER = rec
    try:
        yield rec
    finally:
        ops.PROFILER = None


def expect_plan(L, tile_hint, splitk_hint, bf16_mode, unhinted=None):
    """What the host must report for launch L (asserted BEFORE the launch runs).  tile_hint 3 asks for the 128 x 64 form, which
    exists for fp32 float4 launches only: elsewhere the hint changes nothing, and the plan must be the un-hinted one."""
    vec = GC.float4_rule(L)
    bf16 = bf16_mode and vec == 4
    form_128x64 = tile_hint == 3 and vec == 4 and not bf16_mode
    ksteps = -(-L.K // 32)

    def expect(rec):
        ctx = (L, tile_hint, splitk_hint, bf16_mode, rec)
        assert rec["vec"] == vec, ctx
        assert rec["kernel_id"] == (1 if bf16 else 0) and rec["uses_bf16"] == (1 if bf16 else 0), ctx
        if tile_hint == 1 or form_128x64:
            assert rec["tile"] == 128, ctx
        elif tile_hint == 2:
            assert rec["tile"] == 64, ctx
        else:
            assert rec["tile"] in (64, 128), ctx
            if tile_hint == 3:
                assert unhinted is not None and (rec["tile"], rec["splitk"]) == (unhinted["tile"], unhinted["splitk"]), ctx
        if form_128x64:
            assert rec["splitk"] == 1, ctx                     # the 128 x 64 form never splits
        elif splitk_hint > 0:
            assert 1 <= rec["splitk"] <= splitk_hint, ctx
            assert (rec["splitk"] > 1) == (ksteps >= 2), ctx   # a forced split happens wherever there are two K steps to share out
        else:
            assert 1 <= rec["splitk"] <= ksteps, ctx
        assert rec["ws_bytes"] == (max(1, L.batch) * rec["splitk"] * L.M * L.N * 4 if rec["splitk"] > 1 else 0), ctx
    return expect


class OnDevice:
    """A case's flat buffers as fp32 device tensors, and its expected output buffer."""

    def __init__(self, case, bf16_reference=False):
        self.case, L, b = case, case.L, case.bufs
        self.t = {k: v.float().to(dev) for k, v in b.items()}
        ref = dict(b)
        if bf16_reference:                                     # the product of RNE-rounded operands (NaN padding stays NaN)
            for k in ("A", "B", "A_k2", "B_k2"):
                if k in ref:
                    ref[k] = ref[k].float().to(torch.bfloat16).double()
        self.want = R.expected(L, ref["A"], ref["B"], ref["C0"], **{k: ref.get(k) for k in ("bias", "rowadd", "residual", "A_k2", "B_k2")})
        self.want32 = self.want.float()
        self.exact = torch.equal(self.want32.double(), self.want)
        self.want32 = self.want32.to(dev)

    def launch(self, ops, tile_hint=0, splitk_hint=0):
        """-> the whole output buffer after the launch"""
        L, t = self.case.L, self.t
        C = t["C0"].clone()
        kw = dict(alpha=L.alpha, batch=L.batch, batch_inner=L.batch_inner, sA=L.sA, sB=L.sB, sC=L.sC, tile_hint=tile_hint,
                  splitk_hint=splitk_hint)
        if "bias" in t:
            kw["bias"] = t["bias"][L.off_bias:]
        if "rowadd" in t:
            G = (L.M + L.rows_per_group - 1) // L.rows_per_group
            kw["rowadd"] = torch.as_strided(t["rowadd"], (G, L.N), (L.ld_rowadd, 1), L.off_rowadd)
            kw["rows_per_group"] = L.rows_per_group
        if "residual" in t:
            kw["residual"], kw["ldr"] = t["residual"][L.off_residual:], L.ldr
        if L.k_split > 0:
            K2 = L.K - L.k_split
            kw["A_k2"] = torch.as_strided(t["A_k2"], (L.M, L.lda_k2), (L.lda_k2, 1))
            kw["B_k2"] = torch.as_strided(t["B_k2"], (L.N if L.b_mode == R.B_KC else K2, L.ldb_k2), (L.ldb_k2, 1))
            kw["k_split"] = L.k_split
        ops.gemm_raw(t["A"][L.off_A:], t["B"][L.off_B:], C[L.off_C:], L.a_mode, L.b_mode, L.M, L.N, L.K, L.lda, L.ldb, L.ldc, **kw)
        return C


def mismatch(got, want32):
    """None when the buffers are bit-equal as numbers, else a short description of the difference."""
    if torch.equal(got, want32):
        return None
    bad = torch.nonzero(~(got == want32)).flatten()
    i = bad[:4].tolist()
    return f"{len(bad)} of {got.numel()} floats differ, first at {i}: got {got[i].tolist()} want {want32[i].tolist()}"


def run_exact(ops, case, hints, flag_sets=()):
    """Launch `case` at every (tile_hint, splitk_hint) of `hints` in fp32 and in bf16 mode; -> the list of failures.
    flag_sets: ops.kernel_flags keyword sets under which every launch is repeated and must give the identical buffer."""
    g = OnDevice(case)
    assert g.exact, case.label
    failures = []
    for mode in (None, "bf16"):
        unhinted = {}
        for tile_hint, splitk_hint in hints:
            with recording(ops, expect_plan(case.L, tile_hint, splitk_hint, mode == "bf16", unhinted.get(splitk_hint))) as rec:
                with ops.operand_precision(mode or "f32"):
                    got = g.launch(ops, tile_hint, splitk_hint)
                for flags in flag_sets:
                    with ops.kernel_flags(**flags), ops.operand_precision(mode or "f32"):
                        again = g.launch(ops, tile_hint, splitk_hint)
                    if not torch.equal(again, got):
                        failures.append(f"{case.label} [{mode or 'fp32'} tile {tile_hint} splitk {splitk_hint}] differs under {flags}")
            assert len(rec.records) == 1 + len(flag_sets)
            if tile_hint == 0:
                unhinted[splitk_hint] = rec.records[0]
            bad = mismatch(got, g.want32)
            if bad:
                failures.append(f"{case.label} [{mode or 'fp32'} tile {tile_hint} splitk {splitk_hint} plan {rec.records[0]}]: {bad}")
    return failures


def report(failures):
    assert not failures, f"{len(failures)} launches wrong:\n" + "\n".join(failures[:20])


DENSE_HINTS = [(t, s) for t in (0, 1, 2, 3) for s in (0, 2, 3)]
FLAG_SETS = (dict(scalar_epilogue=True), dict(general_loaders=True))


@pytest.mark.parametrize("shape", GC.DENSE_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("pair", list(GC.MODE_PAIRS))
def test_dense_launches_are_exact(ops, pair, shape):
    """Leading dimensions (tight, + 4, + 1) x epilogues (none; alpha, bias, rowadd, residual each on its own stride with
    rows_per_group 1 / 3 / M; the same with C or the bias one float off the float4 grid, or ldr / ld_rowadd odd) x tile hints
    0..3 x split hints 0 / 2 / 3 x {fp32, bf16 operands}.  The full epilogue is also run with the scalar epilogue and with the
    masking loaders forced, and must not change by a bit."""
    failures = []
    for case in GC.dense_cases(pair, shape):
        flags = FLAG_SETS if "epilogue all_" in case.label else ()
        failures += run_exact(ops, case, DENSE_HINTS, flags)
    report(failures)


@pytest.mark.parametrize("pair", ["kc_kc", "kc_mc"])
def test_k_concatenated_launches_are_exact(ops, pair):
    """The fused LoRA linear: k >= k_split read from A_k2 / B_k2 on their own (padded) leading dimensions; K tails of 4 and 12
    (masking loaders) and a whole K step (lean loaders); 128 x 128, 64 x 64 and 128 x 64 tiles."""
    failures = []
    for case in GC.kcat_cases(pair):
        failures += run_exact(ops, case, [(0, 0), (1, 0), (2, 0), (3, 0)])
    report(failures)


@pytest.mark.parametrize("form", GC.ATTN_FORMS)
def test_attention_layout_batches_are_exact(ops, form):
    """batch 6 = 2 x 3 heads interleaved in [B][T][3 d] token tensors, scores [B][3][Tq][Tk] with a padded outer stride: the
    three products of ops.UnfusedAttentionCoreFn, with a forced split where K has two steps."""
    failures = []
    for case in GC.attention_cases(form):
        hints = [(1, 0), (2, 0)] + ([(1, 2), (2, 2)] if "(64, 64, 32)" in case.label else [])
        failures += run_exact(ops, case, [(0, 0)] + hints)
    report(failures)


@pytest.mark.parametrize("pair", list(GC.MODE_PAIRS))
def test_slab_layout_batches_are_exact(ops, pair):
    """batch 5 with batch_inner 0: slabs 4 floats apart (the Winograd product panels' layout), K = 64 split in two, bias and a
    residual that shares C's batch stride but has its own row stride."""
    failures = []
    for case in GC.slab_cases(pair):
        failures += run_exact(ops, case, [(0, 2), (1, 2), (2, 2)])
    report(failures)


def test_odd_batch_strides_take_the_dword_loaders(ops):
    """A head stride one float off the float4 grid (rows still float4-able): the launch must run vec 1 and in fp32 whatever the
    operand precision allows (gad.h, next to strideA0) - expect_plan refuses to launch anything else - and is exact."""
    failures = []
    for case in GC.odd_stride_cases():
        assert GC.float4_rule(case.L) == 1
        failures += run_exact(ops, case, [(0, 0), (1, 0), (2, 0)])
    report(failures)


@pytest.mark.parametrize("pair", list(GC.MODE_PAIRS))
def test_padded_randn_launch_against_fp64(ops, pair):
    """randn operands at (256, 132, 1000), every leading dimension + 4, the full epilogue: the fp32 rule of test_gpu_kernels.py
    (rtol 2e-4, atol 2e-5 sqrt(K) of the output scale) and, for bf16 operands, that of
    test_gemm_row_contiguous_layouts_bf16_operands (rtol 1e-5, atol 2e-6 sqrt(K)) against the product of RNE-rounded operands.
    Everything outside the computed elements must still be the sentinel."""
    case = GC.accuracy_case(pair)
    L = case.L
    for mode, rtol, atol in ((None, 2e-4, 2e-5 * math.sqrt(L.K)), ("bf16", 1e-5, 2e-6 * math.sqrt(L.K))):
        g = OnDevice(case, bf16_reference=mode == "bf16")
        computed = g.want != GC.SENTINEL
        for tile_hint in (1, 2):
            with recording(ops, expect_plan(L, tile_hint, 0, mode == "bf16")), ops.operand_precision(mode or "f32"):
                got = g.launch(ops, tile_hint).cpu().double()
            assert torch.equal(got[~computed], g.want[~computed])
            ref = g.want[computed].abs().max().item()
            err = (got[computed] - g.want[computed]).abs().max().item()
            print(f"{case.label} {mode or 'fp32'} tile {tile_hint}: max err {err:.3e} (ref max {ref:.3e}, atol {atol * max(1.0, ref):.3e})")
            assert torch.allclose(got[computed], g.want[computed], rtol=rtol, atol=atol * max(1.0, ref)), f"max err {err:.3e} (ref max {ref:.3e})"
