"""The host rules the three schedulers share (gad/schedulers.py, on _Base): the (alpha_t, alpha_prev) pair with its final
alpha, the x0 clamp, the leading-spacing timestep grid, and the randn_tensor draw.  No GPU and no library are needed.  The
expected timestep lists come from the restatements (tests/pndm_ref.py, oracle/diffusers_ref.py), not from the code under test."""
import pytest
import torch

import pndm_ref
from oracle import diffusers_ref as R


def _schedulers(**kw):
    import gad
    return gad.DDPMScheduler(**kw), gad.DDIMScheduler(**kw), gad.PNDMScheduler(skip_prk_steps=True, **kw)


@pytest.mark.parametrize("set_alpha_to_one", [True, False])
def test_alpha_pair_takes_the_final_alpha_past_the_last_step(set_alpha_to_one):
    import gad
    for sch in (gad.DDIMScheduler(set_alpha_to_one=set_alpha_to_one),
                gad.PNDMScheduler(skip_prk_steps=True, set_alpha_to_one=set_alpha_to_one)):
        final = 1.0 if set_alpha_to_one else sch.alphas_cumprod[0].item()
        assert sch.final_alpha_cumprod.item() == final
        assert sch.alpha_pair(3, -1) == (sch.alphas_cumprod[3].item(), final)
        assert sch.alpha_pair(0, -10) == (sch.alphas_cumprod[0].item(), final)
    ddpm = gad.DDPMScheduler()
    assert ddpm.alpha_pair(3, -1) == (ddpm.alphas_cumprod[3].item(), 1.0)


def test_alpha_pair_is_the_fp32_table_otherwise():
    for sch in _schedulers():
        ac = sch.alphas_cumprod
        assert ac.dtype == torch.float32
        for t_from, t_to in ((999, 989), (10, 0), (1, 0), (500, 499)):
            pair = sch.alpha_pair(t_from, t_to)
            assert pair == (ac[t_from].item(), ac[t_to].item()) and all(type(v) is float for v in pair)
            assert all(torch.tensor(v, dtype=torch.float32).item() == v for v in pair)      # python floats of fp32 values


def test_alpha_pair_is_what_the_step_rules_read():
    import gad
    ddim = gad.sd_scheduler("ddim")
    ddim.set_timesteps(4)                                   # 751, 501, 251, 1; stride 250
    assert ddim.step_coefficients(751) == ddim.alpha_pair(751, 501)
    assert ddim.step_coefficients(1) == (ddim.alphas_cumprod[1].item(), ddim.alphas_cumprod[0].item())   # set_alpha_to_one False
    pndm = gad.sd_scheduler("pndm")
    pndm.set_timesteps(4)
    cs, cm = pndm.step_plan(751)[:2]
    assert (cs, cm) == gad.schedulers.plms_coefficients(*pndm.alpha_pair(751, 501))
    assert (cs, cm) == pytest.approx(pndm_ref.transfer(*pndm.alpha_pair(751, 501)), rel=1e-12)   # a few fp64 roundings apart


def test_clip_of_the_three_schedulers():
    import gad
    assert gad.DDPMScheduler().clip == 1.0 and gad.DDIMScheduler().clip == 1.0
    assert gad.DDPMScheduler(clip_sample_range=2.5).clip == 2.5 and gad.DDIMScheduler(clip_sample_range=2.5).clip == 2.5
    assert gad.DDPMScheduler(clip_sample=False, clip_sample_range=2.5).clip == 0.0
    assert gad.DDIMScheduler(clip_sample=False).clip == 0.0 and gad.sd_scheduler("ddim").clip == 0.0
    assert gad.PNDMScheduler(skip_prk_steps=True).clip == 0.0 and gad.sd_scheduler("pndm").clip == 0.0     # PNDM has no clamp
    assert all(type(s.clip) is float for s in (gad.DDPMScheduler(clip_sample_range=2), gad.sd_scheduler("pndm")))


@pytest.mark.parametrize("steps_offset", [0, 1])
@pytest.mark.parametrize("n", [1, 4, 50, 1000])
def test_the_three_set_timesteps_share_one_grid(n, steps_offset):
    ddpm, ddim, pndm = _schedulers(steps_offset=steps_offset)
    ref = R.DDIMScheduler(steps_offset=steps_offset)
    ref.set_timesteps(n)
    want = ref.timesteps.tolist()                           # diffusers' DDPM and DDIM build the same leading grid
    assert len(want) == n and want[-1] == steps_offset
    for sch in (ddpm, ddim):
        sch.set_timesteps(n)
        assert sch.timesteps.dtype == torch.int64 and sch.timesteps.tolist() == want
        assert sch.num_inference_steps == n and sch.stride == 1000 // n
    pndm.set_timesteps(n)
    assert pndm.timesteps.dtype == torch.int64
    assert pndm.timesteps.tolist() == pndm_ref.timesteps(n, 1000, steps_offset).tolist()
    assert len(pndm.timesteps) == (n + 1 if n > 1 else 1)   # the second-to-last entry is visited twice
    for sch in (ddpm, ddim, pndm):
        with pytest.raises(ValueError, match="num_train_timesteps"):
            sch.set_timesteps(1001)


def test_randn_tensor_is_the_host_draw_it_replaces():
    from gad.schedulers import randn_tensor
    shape = (2, 3, 5, 7)
    want = torch.randn(shape, generator=torch.Generator().manual_seed(11), dtype=torch.float32)
    got = randn_tensor(shape, torch.Generator().manual_seed(11), torch.device("cpu"))
    assert got.dtype == torch.float32 and got.device.type == "cpu" and torch.equal(got, want)
    want64 = torch.randn(shape, generator=torch.Generator().manual_seed(11), dtype=torch.float64)
    assert torch.equal(randn_tensor(shape, torch.Generator().manual_seed(11), "cpu", torch.float64), want64)
    g = torch.Generator().manual_seed(5)                    # consecutive draws advance the one generator, as at the call sites
    a, b = randn_tensor(shape, g, "cpu"), randn_tensor(shape, g, "cpu")
    h = torch.Generator().manual_seed(5)
    assert torch.equal(a, torch.randn(shape, generator=h)) and torch.equal(b, torch.randn(shape, generator=h))
    torch.manual_seed(3)                                    # no generator: the device's default one
    c = randn_tensor(shape, None, "cpu")
    torch.manual_seed(3)
    assert torch.equal(c, torch.randn(shape))
