"""CPU checks of the PNDM (PLMS) sampler: the timestep lists, the host state machine against the fp64 restatement, the transfer's
DDIM identity, the constructor's refusals, gad_plms_step's ABI and host-side refusals (no GPU is reached) and the --sampler flag
of the three text-to-image entry points."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import pndm_ref

SD = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", set_alpha_to_one=False, steps_offset=1,
          skip_prk_steps=True)


def test_timestep_lists():
    import gad
    sch = gad.sd_scheduler("pndm")
    assert isinstance(sch, gad.PNDMScheduler)
    sch.set_timesteps(4)
    assert sch.timesteps.tolist() == [751, 501, 501, 251, 1]
    sch.set_timesteps(100)
    ts = sch.timesteps.tolist()
    assert ts[:4] == [991, 981, 981, 971] and ts[-1] == 1 and len(ts) == 101 and len(set(ts)) == 100
    assert ts == pndm_ref.timesteps(100).tolist()
    sch.set_timesteps(1)
    assert sch.timesteps.tolist() == [1]
    with pytest.raises(ValueError, match="num_train_timesteps"):
        sch.set_timesteps(1001)


def test_sd_scheduler_configurations():
    import gad
    for name, cls in (("ddim", gad.DDIMScheduler), ("pndm", gad.PNDMScheduler)):
        c = gad.sd_scheduler(name).config
        assert isinstance(gad.sd_scheduler(name), cls)
        assert (c.beta_start, c.beta_end, c.beta_schedule, c.steps_offset, c.set_alpha_to_one) == (0.00085, 0.012, "scaled_linear", 1, False)
    assert gad.sd_scheduler("ddim").config.clip_sample is False
    assert gad.sd_scheduler().config == gad.sd_scheduler("ddim").config
    with pytest.raises(ValueError, match="euler"):
        gad.sd_scheduler("euler")
    sch = gad.sd_scheduler("pndm")
    again = gad.PNDMScheduler.from_config(sch.config)
    assert dict(again.config) == dict(sch.config)
    assert np.array_equal(sch.alphas_cumprod.double().numpy(), pndm_ref.sd_alphas_cumprod())
    assert sch.final_alpha_cumprod.item() == sch.alphas_cumprod[0].item()
    assert gad.PNDMScheduler(skip_prk_steps=True, set_alpha_to_one=True).final_alpha_cumprod.item() == 1.0


def test_plan_follows_the_restatement_over_a_run():
    """n = 6: seven steps, so every row of the multistep table is taken and the three-deep history turns over"""
    import gad
    from gad.schedulers import plms_coefficients, plms_plan
    sch = gad.sd_scheduler("pndm")
    ref = pndm_ref.PNDMRef(sch.alphas_cumprod.double().numpy())
    sch.set_timesteps(6)
    ref.set_timesteps(6)
    assert sch.timesteps.tolist() == [831, 665, 665, 499, 333, 167, 1] == ref.timesteps.tolist()
    rng = np.random.default_rng(0)
    x = rng.standard_normal(8)
    r, n_stored = 1000 // 6, 0
    for counter, t in enumerate(sch.timesteps.tolist()):
        x = ref.step(0.3 * x + 0.1 * np.sin(t / 1000), t, x)
        want = ref.last
        t_from, t_to, w, push, use_saved, save = plms_plan(counter, n_stored, t, r)
        assert (t_from, t_to, push, use_saved, save) == (want["t_from"], want["t_to"], want["push"], want["use_saved"], want["save"])
        assert w == want["weights"]                                   # the same fp64 quotients
        assert sum(1 for v in w[1:] if v != 0.0) <= n_stored            # no weight on a prediction that is not stored
        a_t = sch.alphas_cumprod[t_from].item()
        a_p = sch.alphas_cumprod[t_to].item() if t_to >= 0 else sch.final_alpha_cumprod.item()
        assert plms_coefficients(a_t, a_p) == pytest.approx((want["cs"], want["cm"]), rel=1e-15)
        sch.counter, sch.n_stored = counter, n_stored                  # the scheduler's own view of that state
        assert sch.step_plan(t)[:2] == plms_coefficients(a_t, a_p) and sch.step_plan(t)[2:] == (w, push, use_saved, save)
        if counter == 0:
            assert save and push and not use_saved and w == (1.0, 0.0, 0.0, 0.0)
        if counter == 1:
            assert not push and use_saved and not save and (t_from, t_to) == (831, 665) and w == (0.5, 0.5, 0.0, 0.0)
        if counter == 6:
            assert t_to < 0 and want["final"] and a_p == sch.alphas_cumprod[0].item()
        n_stored = min(n_stored + int(push), 3)
    assert n_stored == 3 and abs(sum(w) - 1.0) < 1e-15
    sch.set_timesteps(6)                                                # a new trajectory starts from an empty history
    assert (sch.counter, sch.n_stored) == (0, 0)
    with pytest.raises(ValueError, match="counter=2 with 0 stored"):
        plms_plan(2, 0, 665, r)
    with pytest.raises(ValueError, match="set_timesteps"):
        gad.sd_scheduler("pndm").step_plan(1)


def test_transfer_with_unit_weight_is_the_ddim_update():
    """weights (1, 0, 0, 0): x_prev = cs x - cm e must be gad_ddim_step's formula (include/gad.h, eta = 0, no clipping)
    x0 = (x - sqrt(1 - a_t) e) / sqrt(a_t); x' = sqrt(a_p) x0 + sqrt(1 - a_p) e, to 1e-12 relative in fp64 over the 100 (t, prev)
    pairs of the SD schedule at 100 steps (the last one steps to the final alpha)"""
    import gad
    from gad.schedulers import plms_coefficients
    ac = gad.sd_scheduler("pndm").alphas_cumprod.double().numpy()
    rng = np.random.default_rng(1)
    x, e = rng.standard_normal(64), rng.standard_normal(64)
    pairs = [(t, t - 10) for t in range(991, 0, -10)]
    assert len(pairs) == 100 and pairs[-1] == (1, -9)
    for t, prev in pairs:
        a_t, a_p = ac[t], ac[prev] if prev >= 0 else ac[0]
        cs, cm = plms_coefficients(a_t, a_p)
        cm_ddim = np.sqrt(a_p) * np.sqrt(1 - a_t) / np.sqrt(a_t) - np.sqrt(1 - a_p)
        assert abs(cs - np.sqrt(a_p) / np.sqrt(a_t)) <= 1e-12 * cs and abs(cm - cm_ddim) <= 1e-12 * abs(cm_ddim), (t, cm, cm_ddim)
        ddim = np.sqrt(a_p) * (x - np.sqrt(1 - a_t) * e) / np.sqrt(a_t) + np.sqrt(1 - a_p) * e
        got = cs * x - cm * e
        assert np.all(np.abs(got - ddim) <= 1e-12 * (np.abs(cs * x) + np.abs(cm * e))), t


def test_refusals_by_name():
    import gad
    with pytest.raises(NotImplementedError, match="skip_prk_steps=False"):
        gad.PNDMScheduler()                                             # diffusers' default runs the Runge-Kutta warm-up
    with pytest.raises(NotImplementedError, match="skip_prk_steps=False"):
        gad.PNDMScheduler(**dict(SD, skip_prk_steps=False))
    with pytest.raises(NotImplementedError, match="v_prediction"):
        gad.PNDMScheduler(**SD, prediction_type="v_prediction")
    for spacing in ("trailing", "linspace"):
        with pytest.raises(NotImplementedError, match=spacing):
            gad.PNDMScheduler(**SD, timestep_spacing=spacing)
    with pytest.raises(NotImplementedError, match="beta_schedule"):
        gad.PNDMScheduler(**dict(SD, beta_schedule="squaredcos_cap_v2"))


def test_abi_declared_bound_and_exported():
    from gad import _capi
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "gad.h")).read()
    assert ("int gad_plms_step(const float* x, const float* eps_u, const float* eps_c, float guidance, const float* h1, "
            "const float* h2,") in hdr
    assert "enum gad_plms_saved { GAD_PLMS_SAVED_NONE = 0, GAD_PLMS_SAVE = 1, GAD_PLMS_USE_SAVED = 2 };" in hdr
    assert (_capi.PLMS_SAVED_NONE, _capi.PLMS_SAVE, _capi.PLMS_USE_SAVED) == (0, 1, 2)
    res, argtypes = _capi.SIGNATURES["gad_plms_step"]
    assert res is ctypes.c_int and len(argtypes) == 19
    assert argtypes[3] is ctypes.c_float and argtypes[9] is ctypes.c_int32 and argtypes[11] is ctypes.c_int64
    assert all(a is ctypes.c_double for a in argtypes[12:18]) and argtypes[18] is ctypes.c_void_p
    assert hasattr(_capi.load(), "gad_plms_step")
    out = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert " T gad_plms_step" in out


# a guided four-term step with a push into the slot read as h3, in place; none of these is device memory
GOOD = dict(x=4096, eps_u=8192, eps_c=12288, guidance=7.5, h1=16384, h2=20480, h3=24576, push=24576, x_saved=None, saved_mode=0,
            x_prev=4096, n=1024, cs=1.01, cm=-0.02, w0=55 / 24, w1=-59 / 24, w2=37 / 24, w3=-9 / 24)
NAN, INF = float("nan"), float("inf")
REFUSALS = [
    (dict(x=None), b"null pointer x"),
    (dict(eps_u=None), b"null pointer eps_u"),
    (dict(x_prev=None), b"null pointer x_prev"),
    (dict(saved_mode=1), b"null pointer x_saved with saved_mode 1"),
    (dict(saved_mode=2), b"null pointer x_saved with saved_mode 2"),
    (dict(saved_mode=3, x_saved=28672), b"unknown saved_mode 3"),
    (dict(saved_mode=-1), b"unknown saved_mode -1"),
    (dict(x=4100), b"x must be 16-B aligned"),
    (dict(eps_u=8196), b"eps_u must be 16-B aligned"),
    (dict(eps_c=12296), b"eps_c must be 16-B aligned"),
    (dict(h1=16388), b"h1 must be 16-B aligned"),
    (dict(h2=20488), b"h2 must be 16-B aligned"),
    (dict(h3=24580), b"h3 must be 16-B aligned"),
    (dict(push=24584), b"push must be 16-B aligned"),
    (dict(saved_mode=1, x_saved=28676), b"x_saved must be 16-B aligned"),
    (dict(x_prev=32772), b"x_prev must be 16-B aligned"),
    (dict(n=1026), b"n=1026"),
    (dict(n=0), b"n=0"),
    (dict(n=-4), b"n=-4"),
    (dict(h1=None, w1=0.0), b"h2 without h1"),
    (dict(h2=None, w2=0.0), b"h3 without h2"),
    (dict(h3=None, push=28672), b"w3=-0.375 with a null h3"),
    (dict(h2=None, h3=None, w3=0.0, push=28672), b"w2=1.54167 with a null h2"),
    (dict(h1=None, h2=None, h3=None, w2=0.0, w3=0.0, push=28672), b"w1=-2.45833 with a null h1"),
    (dict(cs=0.0), b"cs=0"),
    (dict(cs=-1.0), b"cs=-1"),
    (dict(cs=NAN), b"cs=nan"),
    (dict(cs=1e300), b"cs=1e+300"),                                   # finite in fp64, not after the rounding to fp32
    (dict(cm=INF), b"cm=inf"),
    (dict(w0=NAN), b"w0=nan"),
    (dict(w1=INF), b"w1=inf"),
    (dict(w2=-INF), b"w2=-inf"),
    (dict(w3=NAN), b"w3=nan"),
    (dict(guidance=NAN), b"guidance=nan"),
    (dict(x_prev=8192, x=8192), b"x_prev aliases eps or a history slot"),
    (dict(x_prev=16384), b"x_prev aliases eps or a history slot"),
    (dict(push=4096), b"push aliases x, x_prev or eps"),
    (dict(push=12288), b"push aliases x, x_prev or eps"),
    (dict(saved_mode=1, x_saved=4096), b"x_saved aliases x, x_prev or push"),
    (dict(saved_mode=2, x_saved=24576), b"x_saved aliases x, x_prev or push"),
]


def plms_call(lib, a):
    return lib.gad_plms_step(a["x"], a["eps_u"], a["eps_c"], a["guidance"], a["h1"], a["h2"], a["h3"], a["push"], a["x_saved"],
                             a["saved_mode"], a["x_prev"], a["n"], a["cs"], a["cm"], a["w0"], a["w1"], a["w2"], a["w3"], None)


@pytest.mark.parametrize("bad, word", REFUSALS)
def test_host_refusals_before_any_hip_call(bad, word):
    """Every refusal returns before a HIP call, so a CPU-only machine reaches it (these pointers are not device memory)."""
    from gad import _capi
    lib = _capi.load()
    rc = plms_call(lib, dict(GOOD, **bad))
    assert rc != 0
    assert word in lib.gad_last_error(), lib.gad_last_error()


def test_wrapper_refuses_host_tensors_and_sizes():
    import torch
    from gad import _capi, ops
    x = torch.zeros(8)
    with pytest.raises(_capi.GadError, match="plms x: expected a contiguous fp32 device tensor"):
        ops.plms_step_raw(x, x, 1.0, 0.1, (1.0, 0.0, 0.0, 0.0))


def test_sampler_flag_on_the_three_entry_points():
    from text_to_image import baselines as B
    from text_to_image import compute_model_behaviors as M
    from text_to_image import grad_text_to_image_lora as G
    cases = [(M.parse_args, ["--reference_lora_dir", "/r", "--db", "/d.jsonl", "--exp_name", "e"]),
             (B.parse_args, ["--reference_lora_dir", "/r", "--output_dir", "/o"]),
             (G.parse_args, ["--train_data_dir", "/d/artbench", "--output_dir", "/o", "--f", "loss", "--source", "generated_journey"])]
    for parse, base in cases:
        assert parse(base).sampler == "ddim"
        assert parse(base + ["--sampler", "pndm"]).sampler == "pndm"
        assert parse(base + ["--sampler", "ddim"]).sampler == "ddim"
        with pytest.raises(SystemExit):
            parse(base + ["--sampler", "euler"])
    a = M.parse_args(cases[0][1] + ["--sampler", "pndm"])
    assert "sampler" not in M.REFERENCE_KEYS and a.num_inference_steps == 100      # the row and the other defaults are untouched
    g = G.parse_args(cases[2][1] + ["--sampler", "pndm"])
    assert G.output_filename(g) == "emb_f=loss_num_journey_points=50_num_journey_noises=1_proj_dim=32768.pt"
    assert list(G.journey_points(101, 50)) == list(range(1, 101, 2))                # 101 callbacks under pndm at 100 steps
