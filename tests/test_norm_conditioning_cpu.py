"""The bound of tests/norm_cases.py separates the two ways of computing a GroupNorm variance, without a GPU: an fp32
emulation of `SS - S mean` per chunk (what csrc/norm.hip's two-pass plan and csrc/half.hip's GroupNorm computed before
they were centred) is REJECTED by the very bound function the GPU test imports, and a chunk-centred form (mean first, then
sum (x - mean)^2, fp32 Chan merge) is ACCEPTED, on the generator's cases at the production chunk geometries.  This keeps
tests/test_gpu_norm_conditioning.py from silently becoming vacuous, and shows that torch's fp32 operator - the reference of
the bound - leaves a correct fp32 kernel room inside it."""
import pytest
import torch

import norm_cases as nc

B, HW, G = 2, 4096, 32
# (storage, name, channels, pixels per chunk): the two-pass plan's chunks at the 64x64 level of the SD U-Net ([16, 64, 64, 320]:
# 128 chunks of 32 pixels) and of CelebA-HQ ([64, 64, 64, 224]: 32 chunks of 128 pixels); the half path's 64-row chunks
# ([16, 4096, 320]), whose sums the parent added up over the whole group before it subtracted
GEOMETRIES = [("fp32", "sd", 320, 32), ("fp32", "celeba", 224, 128), ("bf16", "half", 320, 64)]


def _cases(storage):
    return nc.FP32_CASES if storage == "fp32" else nc.BF16_CASES


def _params():
    return [(s, g, C, cp, name) for s, g, C, cp in GEOMETRIES for name in _cases(s)]


@pytest.mark.parametrize("storage", ["fp32", "bf16"])
def test_exact_shift_is_exact_in_the_storage_type(storage):
    dt = torch.float32 if storage == "fp32" else torch.bfloat16
    for c, grid in nc.EXACT_SHIFTS[storage]:
        x0 = nc.exact_shift_base(B, 64, 256, grid, seed=3)
        x = nc.exact_shift(c, grid)(B, 64, 256, 8, seed=3)
        xs, x0s = x.to(dt), x0.to(dt)
        assert torch.equal(xs.float(), x) and torch.equal(x0s.float(), x0)            # representable as stored
        back = (xs - torch.tensor(float(c), dtype=dt)).to(dt)
        bits = torch.int32 if dt == torch.float32 else torch.int16
        assert torch.equal(back.view(bits), x0s.view(bits))                            # (x0 + c) - c == x0 bitwise: no rounding anywhere
        assert float(x0.min()) >= -4 and float(x0.max()) < 4
    for name, (make, _) in _cases(storage).items():
        x = make(B, 64, 256, 8, seed=1)
        assert torch.equal(x.to(dt).float(), x), name                                 # every case is exact in its storage type


def test_mixed_case_neighbouring_groups_differ():
    x = nc.mixed(4, 320, 64, 32, seed=5)
    m = x.view(4, 32, -1).mean(-1)
    assert bool(((m[:, 1:] - m[:, :-1]).abs() > 5).all())
    assert {int(v) for v in m.round().unique().tolist()} <= {0, 10, -10, 100, -100}


def test_outlier_and_constant_cases():
    for first in (True, False):
        x = nc.outlier(first)(2, 320, 256, 32, seed=2).view(2, 32, -1)
        assert bool(((x == 1000.0).sum(-1) == 1).all())
        assert bool((x[:, :, 0] == 1000.0).all()) == first
    assert bool((nc.constant(2, 64, 16, 8) == 96.0).all())


@pytest.mark.parametrize("storage,geo,C,cp,name", _params())
def test_bound_rejects_the_uncentred_variance_and_accepts_the_centred_one(storage, geo, C, cp, name):
    make, mean_over_std = _cases(storage)[name]
    x = make(B, C, HW, G, seed=7)
    one, zero = torch.ones(C), torch.zeros(C)
    want, e_ref = nc.group_norm_reference(x, G, one, zero)
    keys = ("y", "mean", "rstd")
    # (b) chunk-centred, Chan merge in fp32: accepted everywhere, both outlier placements included
    cen = nc.emulate_group_norm(x, G, cp, centred=True)
    r_cen = {k: nc.ratio(cen[k], want[k], e_ref[k]) for k in keys}
    # (a) SS - S mean: per chunk + Chan merge (fp32 two-pass plan); over the whole group (half path)
    unc = nc.emulate_group_norm(x, G, cp if storage == "fp32" else None, centred=False)
    r_unc = {k: nc.ratio(unc[k], want[k], e_ref[k]) for k in keys}
    print(f"{storage} {geo} {name}: centred {r_cen}  uncentred {r_unc}")
    assert all(r <= 1.0 for r in r_cen.values()), r_cen
    if name == "constant":
        assert bool((cen["mean"] == 96.0).all()) and bool((cen["y"] == 0.0).all())
    shifted = name.startswith("offset") or name == "mixed" or (name.startswith("exact_shift") and mean_over_std >= 64 / 2.31)
    if shifted:
        assert r_unc["rstd"] > 1.0, r_unc
        if mean_over_std >= 100:                      # fp32 chunks and the whole-group form of the bf16 storage alike
            assert r_unc["y"] > 1.0, r_unc
