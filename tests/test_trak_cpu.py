"""CPU checks of the TRAK / D-TRAK features: the generator restatement against the Random123 known answers, the
gad_jl_args ABI, the host-side refusals of gad_jl_project, the score formulas and the kept entry point's flags."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from jl_ref import jl_rows, philox4x32_10


def test_philox_known_answers():
    got = philox4x32_10([0, 0, 0, 0], (0, 0))
    assert [int(w) for w in got] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    got = philox4x32_10([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], (0xA4093822, 0x299F31D0))
    assert [int(w) for w in got] == [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]


def test_generator_entries_are_unit_variance():
    z = jl_rows(np.arange(512) + (1 << 33), 256, seed=3, model_id=1)
    assert abs(z.mean()) < 0.02 and abs(z.var() - 1) < 0.02 and np.isfinite(z).all()
    r = jl_rows(np.arange(64), 256, seed=3, proj_type="rademacher")
    assert set(np.unique(r)) == {-1.0, 1.0} and abs(r.mean()) < 0.03
    # a column block of the normal map is one Philox call on (block, row lo, row hi, 0)
    x = philox4x32_10([5, 7, 0, 0], (9, 2))
    u0, u1 = [(float(np.float32(float(w))) * 2.0 ** -32 + 2.0 ** -33) for w in x[:2]]
    want = np.sqrt(-2 * np.log(np.float32(u0))) * np.cos(2 * np.pi * np.float32(u1))
    assert abs(jl_rows([7], 24, seed=9, model_id=2)[0, 20] - want) < 1e-6


def test_jl_args_layout_matches_header(tmp_path):
    from gad import _capi
    cls = _capi.JLArgs
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "gad.h"', 'int main(void) {',
           '  printf("size %zu\\n", sizeof(gad_jl_args));']
    src += [f'  printf("{f} %zu\\n", offsetof(gad_jl_args, {f}));' for f, _ in cls._fields_]
    src += ['  return 0;', '}']
    c = tmp_path / "jl_layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "jl_layout"
    inc = os.path.join(os.path.dirname(__file__), "..", "include")
    subprocess.run(["gcc", "-I", inc, str(c), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(cls)
    for f, _ in cls._fields_:
        assert int(got[f]) == getattr(cls, f).offset, f


def _args(**kw):
    from gad.trak import jl_args
    base = dict(a=4096, lda=1024, G=3, P=1000, d=128, seed=1, model_id=0, proj_type="normal", out=8192, workspace=16384,
                workspace_bytes=1 << 30)
    base.update(kw)
    return jl_args(**base)


def test_workspace_query():
    from gad import _capi
    from gad.trak import workspace_bytes
    lib = _capi.load()
    n1 = lib.gad_jl_project_workspace_bytes(ctypes.byref(_args(G=1)))
    n8 = lib.gad_jl_project_workspace_bytes(ctypes.byref(_args(G=8)))
    assert n1 > 0 and n8 == 8 * n1 and n1 % (128 * 4) == 0          # slabs x G x d floats; the plan does not depend on G
    assert workspace_bytes(8, 1000, 128) == n8
    assert workspace_bytes(4, 35_750_000, 1024) == 4 * workspace_bytes(1, 35_750_000, 1024)
    assert lib.gad_jl_project_workspace_bytes(ctypes.byref(_args(d=100))) == -1


@pytest.mark.parametrize("bad, word", [
    (dict(d=96), b"multiple of 64"),
    (dict(d=0), b"multiple of 64"),
    (dict(G=0), b"G=0"),
    (dict(lda=996), b"below P"),
    (dict(lda=1002, P=1001), b"multiple of 4"),
    (dict(a=4100), b"misaligned"),
    (dict(out=8196), b"misaligned"),
    (dict(workspace=16388), b"misaligned"),
    (dict(workspace_bytes=64), b"workspace_bytes"),
    (dict(out=None), b"null"),
    (dict(P=0), b"P=0"),
])
def test_refusals_before_any_hip_call(bad, word):
    """Every refusal returns before a HIP call, so a CPU-only machine reaches it (these pointers are not device memory)."""
    from gad import _capi
    lib = _capi.load()
    assert lib.gad_jl_project(ctypes.byref(_args(**bad)), None) != 0
    assert word in lib.gad_last_error(), lib.gad_last_error()
    assert lib.gad_jl_project(None, None) != 0


def test_projector_refuses_unknown_type_and_behaviour():
    from gad.trak import ProjectionType, _GradStep
    with pytest.raises(ValueError):
        ProjectionType("sparse")
    with pytest.raises(NotImplementedError, match="ssim"):
        _GradStep(None, None, "ssim")


def _numpy_scores(train, val, kind):
    k = np.linalg.inv(train.T @ train + 0.5 * np.eye(train.shape[1]))
    if kind == "vanilla_gradient":
        tn = train / np.sqrt((train ** 2).sum(1))[:, None]
        vn = val / np.sqrt((val ** 2).sum(1))[:, None]
        return vn @ tn.T
    proj = train @ k
    mag = {"relative_if": np.sqrt((proj ** 2).sum(1)), "renormalized_if": np.sqrt((train ** 2).sum(1))}.get(kind, 1.0)
    return (val @ proj.T) / mag


@pytest.mark.parametrize("kind", ["trak", "d_trak", "vanilla_gradient", "relative_if", "renormalized_if"])
def test_score_formulas(kind):
    from src.attributions.methods.compute_gradient_score import gradient_scores, trak_kernel_inverse
    rng = np.random.default_rng(0)
    train = rng.standard_normal((40, 16)).astype(np.float32)
    val = rng.standard_normal((5, 16)).astype(np.float32)
    want = _numpy_scores(train.astype(np.float64), val.astype(np.float64), kind)
    np.testing.assert_allclose(gradient_scores(train, val, kind), want, rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(gradient_scores(train, val, kind, trak_kernel_inverse(train)), want, rtol=1e-10, atol=1e-12)


def test_aggregate_by_class():
    from src.attributions.methods.compute_gradient_score import aggregate_by_class
    ds = [(None, l) for l in [3, 1, 3, 7, 1, 1]]
    s = np.arange(12.0).reshape(2, 6)
    got = aggregate_by_class(s, ds, "mean")
    np.testing.assert_allclose(got, [[(1 + 4 + 5) / 3, (0 + 2) / 2, 3], [(7 + 10 + 11) / 3, (6 + 8) / 2, 9]])
    np.testing.assert_allclose(aggregate_by_class(s[0], ds, "max"), [[5, 2, 3]])
    np.testing.assert_allclose(aggregate_by_class(s, ds, "max"), [[11, 8, 9]] * 2)


def test_d_trak_grad_defaults_and_paths():
    from src.attributions.methods import d_trak_grad as D
    a = D.parse_args(["--method", "retrain", "--dataset", "cifar", "--model_behavior", "mean-squared-l2-norm",
                      "--t_strategy", "uniform", "--k_partition", "10", "--outdir", "/o"])
    assert (a.opt_seed, a.projector_dim, a.device, a.removal_seed, a.datamodel_alpha, a.calculate_gen_grad) == \
        (42, 1024, "cuda:0", 0, 0.5, False)
    assert D.save_path(a) == "/o/cifar/d_trak/full/train_f=mean-squared-l2-norm_t=uniform_k=10_d=1024"
    assert D.model_directory(a) == "/o/cifar/retrain/models/full"
    a = D.parse_args(["--method", "retrain", "--dataset", "cifar2", "--model_behavior", "loss", "--t_strategy", "cumulative",
                      "--k_partition", "4", "--projector_dim", "64", "--removal_dist", "datamodel", "--removal_seed", "3",
                      "--outdir", "/o"])
    assert D.save_path(a) == "/o/cifar2/d_trak/datamodel/datamodel_alpha=0.5_seed=3/train_f=loss_t=cumulative_k=4_d=64"
    a = D.parse_args(["--method", "retrain", "--dataset", "cifar", "--model_behavior", "loss", "--t_strategy", "uniform",
                      "--k_partition", "10", "--sample_dir", "/s"])
    assert D.save_path(a) == "/s/d_trak/reference_f=loss_t=uniform_k=10_d=1024"
    a.calculate_gen_grad = True
    with pytest.raises(NotImplementedError, match="calculate_gen_grad"):
        D.main(a)
    from gad.trak import selected_timesteps
    assert selected_timesteps("uniform", 10) == list(range(0, 1000, 100))
    assert selected_timesteps("cumulative", 4) == [0, 1, 2, 3]
