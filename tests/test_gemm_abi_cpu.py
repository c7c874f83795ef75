"""The CPU restatement of gad_gemm's dense ABI (tests/gemm_ref.py) against torch.einsum on contiguous copies, over every
case list the GPU suite runs (tests/gemm_cases.py); the bound that makes the integer cases exact in fp32; and a check that
the whole-buffer comparison bites: three subtly wrong launches give a different buffer.  No GPU."""
from dataclasses import replace

import pytest
import torch

import gemm_cases as GC
import gemm_ref as R

LISTS = dict(GC.all_case_lists())


def _einsum_buffer(case):
    """The expected output buffer built WITHOUT gemm_ref's index arithmetic: einsum on the contiguous logical tensors,
    written through a strided view of the sentinel-filled buffer."""
    L, lg = case.L, case.logical
    want = L.alpha * torch.einsum("zmk,znk->zmn", lg["a"], lg["b"])
    if "bias" in lg:
        want = want + lg["bias"][None, None, :]
    if "rowadd" in lg:
        want = want + lg["rowadd"][torch.arange(L.M) // L.rows_per_group][None]
    if "residual" in lg:
        want = want + lg["residual"]
    Z = max(1, L.batch)
    sizes, strides = (Z // L.inner, L.inner, L.M, L.N), (L.sC[0], L.sC[1], L.ldc, 1)
    out = case.bufs["C0"].clone()
    GC.block(out, L.off_C, sizes, strides).copy_(want.reshape(sizes))
    written = torch.zeros_like(out, dtype=torch.bool)
    GC.block(written, L.off_C, sizes, strides).fill_(True)
    assert int(written.sum()) == Z * L.M * L.N                 # no two output elements share an address
    return out, written


@pytest.mark.parametrize("name", list(LISTS))
def test_restatement_equals_einsum_on_contiguous_copies(name):
    n = 0
    for case in LISTS[name]():
        L, b = case.L, case.bufs
        got = R.expected(L, b["A"], b["B"], b["C0"], **case.operands())
        want, written = _einsum_buffer(case)
        assert not torch.isnan(got).any(), case.label          # no operand padding was read
        assert (got[~written] == GC.SENTINEL).all() and (got[written] != GC.SENTINEL).all(), case.label
        if name.startswith("accuracy"):                        # randn data: fp64 rounding of two summation orders
            assert torch.allclose(got, want, rtol=0, atol=1e-11), case.label
            continue
        assert torch.equal(got, want), case.label
        # exactness: integer operands in [-4, 4], epilogue integers in [-8, 8] (three of them: 24), alpha in {1, 0.5, -2}
        assert L.K <= 1024 and L.alpha in GC.ALPHAS
        for k in ("A", "B", "A_k2", "B_k2"):
            v = b.get(k)
            assert v is None or (v[~torch.isnan(v)].abs() <= 4).all() and (v[~torch.isnan(v)] == v[~torch.isnan(v)].round()).all()
        for k in ("bias", "rowadd", "residual"):
            v = b.get(k)
            assert v is None or (v[~torch.isnan(v)].abs() <= 8).all() and (v[~torch.isnan(v)] == v[~torch.isnan(v)].round()).all()
        assert R.max_scaled_acc(L, b["A"], b["B"], b.get("A_k2"), b.get("B_k2")) + 24 < 2 ** 24, case.label
        assert (got[written] * 2 == (got[written] * 2).round()).all()      # integers or half-integers, which SENTINEL is not
        n += 1
    assert n > 0 or name.startswith("accuracy")


@pytest.mark.parametrize("pair", list(GC.MODE_PAIRS))
def test_subtly_wrong_launches_give_a_different_buffer(pair):
    """What a dropped K element, a bias read one column off or a wrong rowadd group would do to the exact comparison."""
    shape = (63, 65, 36)
    case = GC.build("bite", GC.dense_launch(pair, shape, "pad4", "all_rpg3"), 11, bias=True, rowadd=True, residual=True)
    L, b = case.L, case.bufs
    b["bias"][L.N] = 5.0                                       # the float after the bias (padding) must be readable for the shifted variant
    good = R.expected(L, b["A"], b["B"], b["C0"], **case.operands())
    for wrong in (replace(L, K=L.K - 1), replace(L, off_bias=1), replace(L, rows_per_group=L.rows_per_group + 1)):
        bad = R.expected(wrong, b["A"], b["B"], b["C0"], **case.operands())
        assert not torch.isnan(bad).any()
        diff = bad != good
        assert diff.any() and int(diff.sum()) > L.M            # not a stray element: most rows change
        assert (bad == GC.SENTINEL).sum() == (good == GC.SENTINEL).sum()


def test_float4_rule_of_the_cases():
    """The case lists reach both loader widths for every mode pair, and the odd-stride cases are vec 1 by their batch
    strides alone (their row strides and extents are float4-able)."""
    for pair in GC.MODE_PAIRS:
        vecs = {GC.float4_rule(GC.dense_launch(pair, s, ld, "none")) for s in GC.DENSE_SHAPES for ld in GC.LD_VARIANTS}
        assert vecs == {1, 4}
    for case in GC.odd_stride_cases():
        L = case.L
        assert GC.float4_rule(L) == 1 and GC.float4_rule(replace(L, batch=1)) == 4
        assert L.lda % 4 == 0 and L.ldb % 4 == 0 and L.K % 4 == 0
    for form in GC.ATTN_FORMS:
        assert all(GC.float4_rule(c.L) == 4 for c in GC.attention_cases(form))
