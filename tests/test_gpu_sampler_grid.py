"""The streaming grid rule (gad_stream_grid and its rows-by-chunks form, csrc/gad_common.h) as the sampler kernels of
csrc/sampler.hip use it.  The kernels are elementwise, so a result cannot depend on the grid: one launch past the 2048-workgroup
clamp must equal two launches, each below it, on the two halves of the tensor bit for bit, and a two-row DDPM launch (a 2 x 2 grid)
must equal the two single-row launches.  All pointers are valid and 16-B aligned."""
import pytest
import torch

pytestmark = pytest.mark.gpu
dev = torch.device("cuda:0")

NV = 2048 * 256 + 3                  # float4 items: one 256-thread row of lanes past the clamp (2049 workgroups asked for, 2048 given)
N = 4 * NV
HALF = 4 * (NV // 2)                 # the split stays on a float4 boundary: 262145 and 262146 float4 (1025 workgroups each)


def rnd(n, seed):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed)).to(dev)


def test_ddim_step_past_the_clamp_equals_its_two_halves():
    from gad import ops
    x, eps = rnd(N, 1), rnd(N, 2)
    a_t, a_p, clip = 0.25, 0.5, 1.0                           # the clamp is active: x0 = 2 x - sqrt(3) eps leaves [-1, 1] often
    whole = ops.ddim_step_raw(x, eps, a_t, a_p, clip)
    parts = [ops.ddim_step_raw(x[s], eps[s], a_t, a_p, clip) for s in (slice(0, HALF), slice(HALF, N))]
    assert torch.equal(whole, torch.cat(parts))
    assert whole.isfinite().all() and not torch.equal(whole, x)


def test_guided_plms_step_past_the_clamp_equals_its_two_halves():
    from gad import ops
    from gad.schedulers import PLMS_WEIGHTS, plms_coefficients
    x, eu, ec, h1 = rnd(N, 3), rnd(N, 4), rnd(N, 5), rnd(N, 6)
    cs, cm = plms_coefficients(0.25, 0.5)
    w, g = PLMS_WEIGHTS[2], 7.5                               # one history term

    def run(s):
        return ops.plms_step_raw(x[s], torch.cat([eu[s], ec[s]]), cs, cm, w, history=[h1[s]], guidance=g)
    whole = run(slice(0, N))
    assert torch.equal(whole, torch.cat([run(slice(0, HALF)), run(slice(HALF, N))]))
    assert whole.isfinite().all() and not torch.equal(whole, x)


def test_ddpm_step_of_two_rows_equals_two_single_row_launches():
    from gad import ops
    B, n, t = 2, 1028, 7                                      # 257 float4 per row: two workgroups along x, the rows along y
    x, eps = rnd(B * n, 7).view(B, n), rnd(B * n, 8).view(B, n)
    seeds = torch.tensor([12345, -(1 << 40) + 9], dtype=torch.int64, device=dev)
    a_t, a_p = 0.25, 0.5
    for variance in ("fixed_small", "fixed_large"):
        both = ops.ddpm_step_raw(x, eps, seeds, t, a_t, a_p, 1.0, variance)
        rows = [ops.ddpm_step_raw(x[b:b + 1], eps[b:b + 1], seeds[b:b + 1], t, a_t, a_p, 1.0, variance) for b in range(B)]
        assert torch.equal(both, torch.cat(rows))
        assert both.isfinite().all() and not torch.equal(both[0], both[1])
