"""CPU checks of Journey-TRAK: the visited timesteps, the restatement of gad_ddpm_step's variance noise, the entry point's ABI and
its host-side refusals (no GPU is reached), d_trak_grad's --calculate_gen_grad flags and the journey_trak score route."""
import ctypes
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

from jl_ref import philox4x32_10, uniform
from journey_ref import ddpm_noise

SEED = (42 << 32) | 7                      # a noise key with a non-zero high word, as journey_latents forms them


def test_journey_timesteps():
    from gad.trak import journey_timesteps
    assert journey_timesteps(10) == [999, 899, 799, 699, 599, 499, 399, 299, 199, 99]
    assert journey_timesteps(3) == [999, 666, 333, 0]
    ts = journey_timesteps(100)
    assert ts[-1] == 9 and len(ts) == 100
    assert journey_timesteps(4, 8) == [7, 5, 3, 1]
    for k in (3, 7, 10, 100, 1000):                                   # ceil(T / (T // k)) visits
        assert len(journey_timesteps(k)) == -(-1000 // (1000 // k))


def test_journey_seeds_are_opt_seed_high_sample_low():
    from gad.trak import journey_seeds
    assert journey_seeds(42, range(3)) == [(42 << 32) | s for s in range(3)]
    assert journey_seeds(0xFFFFFFFF, [1]) == [((0xFFFFFFFF << 32) | 1) - (1 << 64)]      # the int64 that holds those 64 bits


def test_noise_restatement_block_by_block():
    t, n = 333, 22                                                    # n is not a multiple of 4: the last block is cut
    z = ddpm_noise([SEED], t, n)[0]
    for b in range((n + 3) // 4):
        u = uniform(philox4x32_10([b, t, 0, 2], (SEED & 0xFFFFFFFF, SEED >> 32)))
        r01, r23 = np.sqrt(-2 * np.log(u[0])), np.sqrt(-2 * np.log(u[2]))
        want = [r01 * np.cos(2 * np.pi * u[1]), r01 * np.sin(2 * np.pi * u[1]),
                r23 * np.cos(2 * np.pi * u[3]), r23 * np.sin(2 * np.pi * u[3])]
        want = np.array(want)[:n - 4 * b]                             # numpy's vector and scalar cos / sin may differ by an ulp
        assert np.all(np.abs(z[4 * b:4 * b + 4] - want) <= 1e-15 * (1 + np.abs(want)))


def test_noise_restatement_moments_and_independence():
    n = 1 << 17
    z = ddpm_noise([SEED, SEED + 1], 500, n)
    z_t = ddpm_noise([SEED], 499, n)[0]
    assert np.isfinite(z).all()
    for row in (z[0], z[1], z_t):
        assert abs(row.mean()) <= 5 * (1.0 / n) ** 0.5                # standard error of the mean of n unit normals
        assert abs(row.var() - 1.0) <= 5 * (2.0 / n) ** 0.5           # ... and of their variance
    for a, b in ((z[0], z[1]), (z[0], z_t)):                          # another seed, another t: standard error 0.0028
        assert abs(np.corrcoef(a, b)[0, 1]) < 0.02


def test_abi_declared_bound_and_exported():
    from gad import _capi
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "gad.h")).read()
    assert "int gad_ddpm_step(const float* x, const float* eps, float* x_prev, int32_t B, int64_t n, const int64_t* seeds" in hdr
    assert "counter (e >> 2, t, 0, 2)" in hdr
    res, argtypes = _capi.SIGNATURES["gad_ddpm_step"]
    assert res is ctypes.c_int and len(argtypes) == 12
    assert argtypes[3] is ctypes.c_int32 and argtypes[4] is ctypes.c_int64 and argtypes[7] is ctypes.c_float
    assert hasattr(_capi.load(), "gad_ddpm_step")
    out = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert " T gad_ddpm_step" in out


_GOOD = dict(x=4096, eps=8192, x_prev=12288, B=3, n=3072, seeds=16384, t=10, alpha_t=0.5, alpha_prev=0.75, clip=1.0,
             variance_type=0)


@pytest.mark.parametrize("bad, word", [
    (dict(x=None), b"null pointer x"),
    (dict(eps=None), b"null pointer eps"),
    (dict(x_prev=None), b"null pointer x_prev"),
    (dict(seeds=None), b"null pointer seeds"),
    (dict(x=4100), b"x must be 16-B aligned"),
    (dict(eps=8200), b"eps must be 16-B aligned"),
    (dict(x_prev=12292), b"x_prev must be 16-B aligned"),
    (dict(n=3074), b"n=3074"),
    (dict(n=0), b"n=0"),
    (dict(B=0), b"B=0"),
    (dict(B=-2), b"B=-2"),
    (dict(t=-1), b"t=-1"),
    (dict(alpha_t=0.0), b"alpha_t=0"),
    (dict(alpha_t=1.5, alpha_prev=1.0), b"alpha_t=1.5"),
    (dict(alpha_prev=1.25), b"alpha_prev=1.25"),
    (dict(alpha_prev=0.0), b"alpha_prev=0"),
    (dict(alpha_prev=0.25), b"alpha_prev=0.25 below alpha_t=0.5"),
    (dict(variance_type=2), b"variance_type 2"),
    (dict(variance_type=-1), b"variance_type -1"),
])
def test_host_refusals_before_any_hip_call(bad, word):
    """Every refusal returns before a HIP call, so a CPU-only machine reaches it (these pointers are not device memory)."""
    from gad import _capi
    lib = _capi.load()
    a = dict(_GOOD, **bad)
    rc = lib.gad_ddpm_step(a["x"], a["eps"], a["x_prev"], a["B"], a["n"], a["seeds"], a["t"], a["alpha_t"], a["alpha_prev"],
                           a["clip"], a["variance_type"], None)
    assert rc != 0
    assert word in lib.gad_last_error(), lib.gad_last_error()


def _gen_args(*extra):
    from src.attributions.methods import d_trak_grad as D
    return D, D.parse_args(["--method", "retrain", "--dataset", "cifar", "--model_behavior", "loss", "--t_strategy", "uniform",
                            "--k_partition", "10", "--outdir", "/o", "--calculate_gen_grad", *extra])


def test_d_trak_grad_gen_path_and_required_flags():
    D, a = _gen_args("--n_samples", "5")
    assert D.save_path(a) == "/o/cifar/d_trak/full/gen_f=loss_t=uniform_k=10_d=1024"
    D, a = _gen_args()
    with pytest.raises(ValueError, match="--n_samples"):
        D.main(a)
    D, a = _gen_args("--n_samples", "5")
    a.k_partition = None
    with pytest.raises(ValueError, match="--k_partition"):
        D.main(a)
    D, a = _gen_args("--n_samples", "5")
    a.t_strategy = None
    with pytest.raises(ValueError, match="--t_strategy"):
        D.main(a)
    D, a = _gen_args("--n_samples", "5", "--sample_dir", "/s")
    with pytest.raises(NotImplementedError, match="calculate_gen_grad"):
        D.main(a)
    D, a = _gen_args("--n_samples", "5")
    a.dataset = "celeba"
    with pytest.raises(NotImplementedError, match="celeba"):
        D.main(a)


def test_journey_trak_scores(tmp_path, monkeypatch):
    """journey_trak: the validation features are the gen_ memmap under OUTDIR (sample_size rows, no --sample_dir); train side,
    kernel and formula are trak's.  Refused by name before this route existed."""
    import src.constants as constants
    from src.attributions.methods.compute_gradient_score import compute_gradient_scores
    from src.datasets import create_dataset
    monkeypatch.setenv("GAD_SYNTH_SCALE", "0.00061")                 # cifar2: 6 training images
    monkeypatch.setattr(constants, "OUTDIR", str(tmp_path))
    n_train, d = len(create_dataset(dataset_name="cifar2", train=True)), 16
    rng = np.random.default_rng(0)
    train = rng.standard_normal((n_train, d)).astype(np.float32)
    val = rng.standard_normal((7, d)).astype(np.float32)
    fdir = tmp_path / "cifar2" / "d_trak" / "full"
    fdir.mkdir(parents=True)
    train.tofile(fdir / "train_f=loss_t=uniform_k=10_d=16")
    val.tofile(fdir / "gen_f=loss_t=uniform_k=10_d=16")
    args = SimpleNamespace(dataset="cifar2", sample_dir=None, gradient_type="journey_trak", k_partition=10, projector_dim=d,
                           sample_size=5, model_behavior_key="fid", by_class=False, by="mean")
    got = compute_gradient_scores(args)
    t64, v64 = train.astype(np.float64), val.astype(np.float64)
    want = v64[:5] @ (t64 @ np.linalg.inv(t64.T @ t64 + 0.5 * np.eye(d))).T
    assert got.shape == (5, n_train)
    np.testing.assert_allclose(got, want, rtol=1e-10)
    args.sample_size = 9
    with pytest.raises(ValueError, match=r"7 rows.*sample_size=9"):
        compute_gradient_scores(args)
