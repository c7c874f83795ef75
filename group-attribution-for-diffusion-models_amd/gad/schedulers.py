"""DDPM / DDIM / PNDM schedulers with the diffusers-0.24 constructor keys and methods the
reference calls (main.py:551,686,698; src/diffusion_utils.py:311,406).
Tables are float32 on the host exactly as diffusers builds them; the per-element work
(add_noise, the DDIM update, the PLMS step) runs in one fused HIP kernel each."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import torch

from . import ops
from .nn import FrozenConfig


def _betas(beta_start, beta_end, n, schedule, trained_betas=None):
    if trained_betas is not None:
        return torch.tensor(trained_betas, dtype=torch.float32)
    if schedule == "linear":
        return torch.linspace(beta_start, beta_end, n, dtype=torch.float32)
    if schedule == "scaled_linear":
        return torch.linspace(beta_start ** 0.5, beta_end ** 0.5, n, dtype=torch.float32) ** 2
    raise NotImplementedError(f"beta_schedule={schedule}")


def randn_tensor(shape, generator, device, dtype=torch.float32):
    """diffusers' randn_tensor: a CPU generator draws on the host and the tensor is moved (the same noise on every device);
    any other generator, or none, draws on `device`."""
    if generator is not None and generator.device.type == "cpu":
        return torch.randn(shape, generator=generator, dtype=dtype).to(device)
    return torch.randn(shape, generator=generator, dtype=dtype, device=device)


class _Base:
    @property
    def clip(self):
        """The x0 clamp of the step kernels: clip_sample_range, or 0.0 (no clamp) without clip_sample (PNDM has none)."""
        c = self.config
        return float(c.clip_sample_range) if c.get("clip_sample") else 0.0

    @property
    def stride(self):
        """Timesteps between two visited ones, T // n (needs set_timesteps)."""
        return self.config.num_train_timesteps // self.num_inference_steps

    def alpha_pair(self, t_from, t_to):
        """(alpha_bar[t_from], alpha_bar[t_to]) as python floats holding the float32 table values; t_to < 0 is past the
        last step and takes the final alpha: final_alpha_cumprod where the scheduler has one, 1.0 for DDPM."""
        ac = self.alphas_cumprod
        final = getattr(self, "final_alpha_cumprod", None)
        a_to = ac[t_to].item() if t_to >= 0 else 1.0 if final is None else final.item()
        return ac[t_from].item(), a_to

    def _set_inference_steps(self, num_inference_steps):
        """Records n and returns the ascending leading-spacing grid k (T // n) + steps_offset, k = 0 .. n - 1 (int64)."""
        if num_inference_steps > self.config.num_train_timesteps:
            raise ValueError("num_inference_steps > num_train_timesteps")
        self.num_inference_steps = num_inference_steps
        return (np.arange(0, num_inference_steps) * self.stride).round().astype(np.int64) + self.config.steps_offset

    def _tables(self, c):
        self.betas = _betas(c["beta_start"], c["beta_end"], c["num_train_timesteps"], c["beta_schedule"],
                            c.get("trained_betas"))
        self.alphas = 1.0 - self.betas
        self.alphas_cumprod = torch.cumprod(self.alphas, dim=0)
        self._ac_dev = {}
        self.init_noise_sigma = 1.0
        self.num_inference_steps = None

    def _ac_on(self, device):
        key = (device.type, device.index)
        if key not in self._ac_dev:
            self._ac_dev[key] = self.alphas_cumprod.to(device)
        return self._ac_dev[key]

    def add_noise(self, original_samples, noise, timesteps):
        """x_t = sqrt(acp[t]) x_0 + sqrt(1-acp[t]) eps, per-sample t (fused gather + axpby kernel)."""
        x0 = original_samples.contiguous()
        return ops.add_noise_raw(x0, noise.contiguous(), timesteps.to(x0.device), self._ac_on(x0.device))

    def scale_model_input(self, sample, timestep=None):
        return sample


class DDPMScheduler(_Base):
    def __init__(self, num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear",
                 trained_betas=None, variance_type="fixed_small", clip_sample=True, prediction_type="epsilon",
                 thresholding=False, dynamic_thresholding_ratio=0.995, clip_sample_range=1.0, sample_max_value=1.0,
                 timestep_spacing="leading", steps_offset=0, **unused):
        c = dict(locals())
        for k in ("self", "unused", "__class__"):
            c.pop(k, None)
        self.config = FrozenConfig(c)
        self._tables(self.config)
        self.timesteps = torch.from_numpy(np.arange(0, num_train_timesteps)[::-1].copy())

    def set_timesteps(self, num_inference_steps, device=None):
        self.timesteps = torch.from_numpy(self._set_inference_steps(num_inference_steps)[::-1].copy())

    def step(self, model_output, timestep, sample, generator=None, return_dict=True):
        """Ancestral DDPM update (diffusers DDPMScheduler.step, epsilon prediction, variance_type fixed_small / fixed_large):
        x0 = (x - sqrt(1-abar_t) eps) / sqrt(abar_t), clipped; mean = c0 x0 + c1 x; x_prev = mean + sigma z for t > 0.
        Off the reference's hot path - its samplers are DDIM (src/diffusion_utils.py:311,406) and this scheduler only
        supplies add_noise there - so it is plain torch on the tensors' device."""
        c = self.config
        if c.prediction_type != "epsilon" or c.thresholding or c.variance_type not in ("fixed_small", "fixed_large"):
            raise NotImplementedError("DDPMScheduler.step: epsilon prediction with fixed variance only")
        t = int(timestep)
        a_t, a_p = self.alpha_pair(t, t - (self.stride if self.num_inference_steps else 1))    # no set_timesteps: all T steps
        cur_alpha = a_t / a_p
        cur_beta = 1.0 - cur_alpha
        x0 = (sample - (1.0 - a_t) ** 0.5 * model_output) / a_t ** 0.5
        if c.clip_sample:
            x0 = x0.clamp(-c.clip_sample_range, c.clip_sample_range)
        mean = (a_p ** 0.5 * cur_beta / (1.0 - a_t)) * x0 + (cur_alpha ** 0.5 * (1.0 - a_p) / (1.0 - a_t)) * sample
        if t > 0:
            var = max((1.0 - a_p) / (1.0 - a_t) * cur_beta, 1e-20) if c.variance_type == "fixed_small" else cur_beta
            mean = mean + var ** 0.5 * randn_tensor(sample.shape, generator, sample.device, sample.dtype)
        return SimpleNamespace(prev_sample=mean)


def min_snr_weights(alphas_cumprod, timesteps, snr_gamma):
    """compute_snr + the epsilon-prediction weights of train_text_to_image_lora.py:1276-1290:
    SNR_t = abar_t / (1 - abar_t);  w_t = min(SNR_t, gamma) / SNR_t."""
    a = alphas_cumprod.to(timesteps.device)[timesteps].float()
    snr = a / (1.0 - a)
    return torch.minimum(snr, torch.full_like(snr, float(snr_gamma))) / snr


class DDIMScheduler(_Base):
    def __init__(self, num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear",
                 trained_betas=None, clip_sample=True, set_alpha_to_one=True, steps_offset=0,
                 prediction_type="epsilon", thresholding=False, dynamic_thresholding_ratio=0.995,
                 clip_sample_range=1.0, sample_max_value=1.0, timestep_spacing="leading",
                 rescale_betas_zero_snr=False, **unused):
        c = dict(locals())
        for k in ("self", "unused", "__class__"):
            c.pop(k, None)
        self.config = FrozenConfig(c)
        if prediction_type != "epsilon" or thresholding or timestep_spacing != "leading" or rescale_betas_zero_snr:
            raise NotImplementedError("DDIMScheduler: only the reference's epsilon / leading configuration")
        self._tables(self.config)
        self.final_alpha_cumprod = torch.tensor(1.0) if set_alpha_to_one else self.alphas_cumprod[0]
        self.timesteps = torch.from_numpy(np.arange(0, num_train_timesteps)[::-1].copy().astype(np.int64))

    @classmethod
    def from_config(cls, config):
        return cls(**dict(config))

    def set_timesteps(self, num_inference_steps, device=None):
        self.timesteps = torch.from_numpy(self._set_inference_steps(num_inference_steps)[::-1].copy())   # host data: the loop index

    def step_coefficients(self, timestep):
        """(alpha_bar_t, alpha_bar_prev) as python floats holding the float32 table values."""
        t = int(timestep)
        return self.alpha_pair(t, t - self.stride)

    def step(self, model_output, timestep, sample, eta=0.0, use_clipped_model_output=False, generator=None,
             variance_noise=None, return_dict=True, out=None):
        if eta != 0.0 or use_clipped_model_output:
            raise NotImplementedError("DDIMScheduler.step: the reference samples with eta=0 "
                                      "(src/diffusion_utils.py:336-341)")
        a_t, a_p = self.step_coefficients(timestep)
        prev = ops.ddim_step_raw(sample.contiguous(), model_output.contiguous(), a_t, a_p, self.clip, out=out)
        return SimpleNamespace(prev_sample=prev)


# ------------------------------------------------------------------------------------------------------------------
# PNDM (PLMS): the sampler SD-1.x repositories ship.  diffusers is not installed, so its semantics are restated
# (tests/pndm_ref.py is the pinned truth).  The state machine is host code; everything done to the latents
# is one gad_plms_step launch.
# ------------------------------------------------------------------------------------------------------------------
PLMS_WEIGHTS = {1: (1.0, 0.0, 0.0, 0.0), 2: (3 / 2, -1 / 2, 0.0, 0.0), 3: (23 / 12, -16 / 12, 5 / 12, 0.0),
                4: (55 / 24, -59 / 24, 37 / 24, -9 / 24)}        # Adams-Bashforth, newest prediction first


def plms_plan(counter: int, n_stored: int, t: int, r: int):
    """The PLMS state machine of one step as pure host code.  `counter`: steps taken since set_timesteps; `n_stored`: noise
    predictions in the history before this step (at most three are kept); `t`: the timestep passed in; `r`: the stride
    num_train_timesteps // num_inference_steps.  -> (t_from, t_to, weights, push, use_saved, save): the transfer runs from
    t_from to t_to (t_to < 0: the final alpha), m = w0 e + w1 h1 + w2 h2 + w3 h3 with h1 the newest stored prediction, `push`
    stores e, `save` remembers the sample, `use_saved` steps from the remembered sample instead of the one passed in."""
    counter, n_stored, t, r = int(counter), int(n_stored), int(t), int(r)
    if counter < 0 or n_stored != (counter if counter <= 1 else min(counter - 1, 3)):
        raise ValueError(f"plms_plan: counter={counter} with {n_stored} stored predictions is not a state step() reaches")
    if counter == 1:                                      # the second visit of the first timestep's successor: a corrector
        return t + r, t, (0.5, 0.5, 0.0, 0.0), False, True, False
    return t, t - r, PLMS_WEIGHTS[n_stored + 1], True, False, counter == 0


def plms_coefficients(a_t: float, a_p: float):
    """PNDMScheduler._get_prev_sample as x_prev = cs x - cm m, in fp64 from the two table values."""
    a_t, a_p = float(a_t), float(a_p)
    cs = (a_p / a_t) ** 0.5
    cm = (a_p - a_t) / (a_t * (1.0 - a_p) ** 0.5 + (a_t * (1.0 - a_t) * a_p) ** 0.5)
    return cs, cm


class PNDMScheduler(_Base):
    """diffusers-0.24 PNDMScheduler restricted to what Stable Diffusion runs: skip_prk_steps=True (PLMS only), epsilon
    prediction, leading spacing.  `n` inference steps make n + 1 entries in `timesteps` (the second is visited twice) and
    n + 1 U-Net evaluations.  The history of noise predictions is a three-slot device ring owned by the scheduler."""
    RING = 3

    def __init__(self, num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear", trained_betas=None,
                 skip_prk_steps=False, set_alpha_to_one=False, prediction_type="epsilon", timestep_spacing="leading",
                 steps_offset=0, **unused):
        c = dict(locals())
        for k in ("self", "unused", "__class__"):
            c.pop(k, None)
        self.config = FrozenConfig(c)
        if not skip_prk_steps:
            raise NotImplementedError("PNDMScheduler: skip_prk_steps=False (the Runge-Kutta warm-up steps) is not implemented; "
                                      "Stable Diffusion ships skip_prk_steps=True")
        if prediction_type != "epsilon":
            raise NotImplementedError(f"PNDMScheduler: prediction_type={prediction_type!r} is not implemented (epsilon only)")
        if timestep_spacing != "leading":
            raise NotImplementedError(f"PNDMScheduler: timestep_spacing={timestep_spacing!r} is not implemented (leading only)")
        self._tables(self.config)
        self.final_alpha_cumprod = torch.tensor(1.0) if set_alpha_to_one else self.alphas_cumprod[0]
        self.timesteps = torch.from_numpy(np.arange(0, num_train_timesteps)[::-1].copy().astype(np.int64))
        self._ring = self._saved = None
        self._reset()

    @classmethod
    def from_config(cls, config):
        return cls(**dict(config))

    def _reset(self):
        self.counter = 0
        self.n_stored = 0                 # predictions held, at most RING
        self._newest = -1                 # ring slot of the newest one

    def set_timesteps(self, num_inference_steps, device=None):
        ts = self._set_inference_steps(num_inference_steps)
        self.timesteps = torch.from_numpy(np.concatenate([ts[:-1], ts[-2:-1], ts[-1:]])[::-1].copy())   # host data, as DDIM's
        self._reset()

    def step_plan(self, timestep):
        """(cs, cm, weights, push, use_saved, save) of the step about to be taken at `timestep` (host floats, fp64)."""
        if self.num_inference_steps is None:
            raise ValueError("PNDMScheduler: set_timesteps has not been called")
        t_from, t_to, w, push, use_saved, save = plms_plan(self.counter, self.n_stored, int(timestep), self.stride)
        return (*plms_coefficients(*self.alpha_pair(t_from, t_to)), w, push, use_saved, save)

    def _state(self, sample):
        if self._ring is None or self._ring.device != sample.device or self._ring.shape[1] != sample.numel():
            if self.counter != 0:
                raise ValueError(f"PNDMScheduler.step: the sample has {sample.numel()} elements on {sample.device}, the history of "
                                 "this trajectory was made for another shape or device (call set_timesteps to start over)")
            self._ring = torch.empty(self.RING, sample.numel(), device=sample.device, dtype=torch.float32)
            self._saved = torch.empty(sample.numel(), device=sample.device, dtype=torch.float32)
        return self._ring, self._saved

    def _launch(self, eps, timestep, sample, guidance, out):
        from . import _capi
        cs, cm, w, push, use_saved, save = self.step_plan(timestep)
        ring, saved = self._state(sample)
        history = [ring[(self._newest - i) % self.RING] for i in range(self.n_stored)]
        slot = (self._newest + 1) % self.RING
        mode = _capi.PLMS_SAVE if save else _capi.PLMS_USE_SAVED if use_saved else _capi.PLMS_SAVED_NONE
        prev = ops.plms_step_raw(sample, eps, cs, cm, w, history=history, push=ring[slot] if push else None,
                                 x_saved=saved if mode != _capi.PLMS_SAVED_NONE else None, saved_mode=mode, guidance=guidance,
                                 out=out)
        if push:
            self._newest, self.n_stored = slot, min(self.n_stored + 1, self.RING)
        self.counter += 1
        return prev

    def step(self, model_output, timestep, sample, return_dict=True, out=None):
        """x_prev of one PLMS step, one gad_plms_step launch without guidance.  `out` may be `sample` (in place)."""
        prev = self._launch(model_output.contiguous(), timestep, sample.contiguous(), None, out)
        return SimpleNamespace(prev_sample=prev)

    def step_guided(self, eps_uc, timestep, sample, guidance_scale, out=None):
        """The same step on the U-Net output of the doubled batch [uncond ; cond]: classifier-free guidance is part of the
        launch, and the guided prediction is what enters the history.  Returns x_prev (`out` may be `sample`)."""
        return self._launch(eps_uc, timestep, sample, float(guidance_scale), out)


def sd_scheduler(name="ddim"):
    """The SD-1.x configuration of either sampler: scaled_linear betas 0.00085 .. 0.012, steps_offset 1, set_alpha_to_one False."""
    kw = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", set_alpha_to_one=False, steps_offset=1)
    if name == "ddim":
        return DDIMScheduler(clip_sample=False, **kw)
    if name == "pndm":
        return PNDMScheduler(skip_prk_steps=True, **kw)
    raise ValueError(f"sd_scheduler: sampler {name!r}, expected 'ddim' or 'pndm'")
