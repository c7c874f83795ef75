"""Row softmax on its own (gad_softmax_fwd / gad_softmax_bwd, csrc/elementwise.hip: one wave per row, four rows per
workgroup) - the two launches of the unfused attention route that are not gad_gemm - against torch in fp64."""
import pytest
import torch

pytestmark = pytest.mark.gpu
dev = torch.device("cuda:0")
POISON = -12345.75


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from gad import ops as o
    return o


def _inputs(rows, n, shifts, seed):
    """randn * 3 logits, row r moved by shifts[r] (a whole row at +-3e4 changes nothing mathematically, and gives NaN or 0
    without the max subtraction), dp randn; each as a flat buffer with one poisoned float after the last row."""
    g = torch.Generator().manual_seed(seed)
    s = torch.randn(rows, n, generator=g) * 3
    for r, sh in enumerate(shifts):
        s[r] += sh
    dp = torch.randn(rows, n, generator=g)
    return [torch.cat([t.flatten(), torch.tensor([POISON])]).to(dev) for t in (s, dp)]


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 77, 1000])
@pytest.mark.parametrize("rows", [1, 5, 8])
def test_row_softmax_forward_and_backward(ops, rows, n):
    """Forward: rtol 2e-5, atol 1e-7 against torch.softmax in fp64 of the same fp32 logits (scale is a power of two, so
    s * scale is exact; an element that is not negligible has |x - max| < 88, whose fp32 rounding is <= 88 * 2^-24 ~ 5e-6
    relative after exp, plus a few ulp each for expf, the n-term sum and the reciprocal); row sums within n * 2^-23 of 1.
    Backward: |err| <= 6e-5 * scale * max|dp| against autograd in fp64 (the gradient tolerance of test_gpu_attention.py for
    O(1) data).  In-place launches (p == s, ds == dp) are bit-identical to the out-of-place ones, and neither writes the float
    after the last row."""
    from gad import _capi
    lib = _capi.load()
    # rows >= 2: row 0 at +3e4 and row 1 at -3e4 in the same launch; a single row takes the three in turn
    for shifts in ([(3e4, -3e4)] if rows >= 2 else [(0.0,), (3e4,), (-3e4,)]):
        for scale in (1.0, 0.125):
            s, dp = _inputs(rows, n, shifts, seed=rows * 1000 + n)
            ctx = (rows, n, shifts, scale)
            p = torch.full_like(s, POISON)
            _capi.check(lib.gad_softmax_fwd(s.data_ptr(), p.data_ptr(), rows, n, scale, ops._stream()), "gad_softmax_fwd")
            assert p[-1].item() == POISON and s[-1].item() == POISON, ctx
            s64 = s[:-1].reshape(rows, n).cpu().double().requires_grad_(True)
            want = torch.softmax(s64 * scale, dim=1)
            got = p[:-1].reshape(rows, n).cpu().double()
            err = (got - want.detach()).abs().max().item()
            sums = (got.sum(1) - 1).abs().max().item()
            print(f"softmax fwd {ctx}: max err {err:.3e}, row sums off by {sums:.3e} (bound {n * 2.0 ** -23:.3e})")
            assert torch.allclose(got, want.detach(), rtol=2e-5, atol=1e-7), (ctx, err)
            assert sums <= n * 2.0 ** -23, (ctx, sums)
            ds = torch.full_like(s, POISON)
            _capi.check(lib.gad_softmax_bwd(p.data_ptr(), dp.data_ptr(), ds.data_ptr(), rows, n, scale, ops._stream()), "gad_softmax_bwd")
            assert ds[-1].item() == POISON, ctx
            dp64 = dp[:-1].reshape(rows, n).cpu().double()
            want.backward(dp64)
            gerr = (ds[:-1].reshape(rows, n).cpu().double() - s64.grad).abs().max().item()
            bound = 6e-5 * scale * dp64.abs().max().item()
            print(f"softmax bwd {ctx}: max err {gerr:.3e} (bound {bound:.3e})")
            assert gerr <= bound, (ctx, gerr, bound)
            # in place
            s2, dp2 = s.clone(), dp.clone()
            _capi.check(lib.gad_softmax_fwd(s2.data_ptr(), s2.data_ptr(), rows, n, scale, ops._stream()), "gad_softmax_fwd")
            assert torch.equal(s2, p), ctx                     # (the poisoned float included)
            _capi.check(lib.gad_softmax_bwd(s2.data_ptr(), dp2.data_ptr(), dp2.data_ptr(), rows, n, scale, ops._stream()), "gad_softmax_bwd")
            assert torch.equal(dp2, ds), ctx
