"""DDPMPipeline / DDIMPipeline with the call signature the reference uses
(src/diffusion_utils.py:336-341,404-412; unconditional_generation/unlearn.py:761-765).

The denoising loop keeps x_t resident in HBM as NHWC; the U-Net forward plus the fused
DDIM update of one step are captured once into a hipGraph per (model, batch) and
replayed for every timestep and every batch (launch-bound otherwise: ~250 kernel
launches per step).  The initial noise is drawn exactly like diffusers' randn_tensor: a
CPU generator draws on the host and the tensor is moved (bit-exact noise parity)."""
from __future__ import annotations

from types import SimpleNamespace

import torch

from . import ops
from .schedulers import DDIMScheduler, PNDMScheduler, randn_tensor


def denoising_steps(x, timesteps, tdev, predict, update):
    """The denoising loop of every sampler, as a generator: per host timestep t it fills the device timestep tensor `tdev`,
    takes eps = predict(x, tdev) and lets update(x, eps, t) write x.  Yields (step index, t) once per enqueued step - the
    callers' per-step hook (a callback; the coalition scheduler interleaves other work there) - and returns x."""
    for i, t in enumerate(timesteps):
        tdev.fill_(t)
        update(x, predict(x, tdev), t)
        yield i, t
    return x


def ddim_update(scheduler):
    """update(x, eps, t) of denoising_steps for a DDIMScheduler: one gad_ddim_step launch, in place."""
    clip = scheduler.clip

    def update(x, eps, t):
        a_t, a_p = scheduler.step_coefficients(t)
        ops.ddim_step_raw(x, eps, a_t, a_p, clip, out=x)
    return update


class DDPMPipeline:
    def __init__(self, unet, scheduler):
        self.unet, self.scheduler = unet, scheduler
        self.vqvae = None
        self.device = unet.device
        self._graphs = {}
        self.use_graph = True

    def to(self, device):
        self.unet.to(device)
        self.device = torch.device(device)
        return self

    def _decode(self, x_nhwc):
        return x_nhwc

    decoder = None            # LDMPipeline with a VQ-VAE: latents -> [0,1] images, for whoever scores decoded samples

    def _run_steps(self, x, num_inference_steps, generator=None):
        """x: NHWC device tensor, updated in place through all timesteps."""
        sch = self.scheduler
        ts = sch.timesteps.tolist()
        tdev = torch.empty(x.shape[0], device=x.device, dtype=torch.int64)
        ddim = isinstance(sch, DDIMScheduler)
        if ddim:
            update = ddim_update(sch)
        else:
            # any other scheduler with the diffusers step() protocol (DDPMScheduler: ancestral sampling).  Off the
            # reference's path (its samplers are DDIM); the step sees NCHW views so that its noise draws keep diffusers' order
            def update(x, eps, t):
                nxt = sch.step(eps.permute(0, 3, 1, 2), t, x.permute(0, 3, 1, 2), generator=generator).prev_sample
                x.copy_(nxt.permute(0, 2, 3, 1))
        if not (self.use_graph and ddim):
            for _ in denoising_steps(x, ts, tdev, self.unet.forward_nhwc, update):
                pass
            return x
        # one captured graph per distinct (a_t, a_p) would defeat the purpose: capture the U-Net
        # forward once (t is a device tensor) and launch the tiny DDIM kernel eagerly after it.
        key = (x.shape[0], tuple(x.shape[1:]))
        g = self._graphs.get(key)
        if g is None:
            g = SimpleNamespace(x=torch.zeros_like(x), t=torch.zeros_like(tdev), eps=None, graph=None)
            side = torch.cuda.Stream(device=x.device)
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):                         # warm-up outside capture (workspace alloc)
                self.unet.forward_nhwc(g.x, g.t)
            torch.cuda.current_stream().wait_stream(side)
            g.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g.graph):
                g.eps = self.unet.forward_nhwc(g.x, g.t)
            self._graphs[key] = g
        g.x.copy_(x)
        ops.refresh_wino(self.unet)            # derived weights the captured launches read at fixed addresses

        def replay(_x, _t):                    # the capture reads g.x and g.t, the state and timestep tensor of this loop
            g.graph.replay()
            return g.eps
        for _ in denoising_steps(g.x, ts, g.t, replay, update):
            pass
        x.copy_(g.x)
        return x

    @torch.no_grad()
    def __call__(self, batch_size=1, generator=None, num_inference_steps=1000, output_type="pil", eta=0.0,
                 return_dict=True):
        if eta != 0.0:
            raise NotImplementedError("eta != 0")
        cfg = self.unet.config
        ss = cfg.sample_size if isinstance(cfg.sample_size, (tuple, list)) else (cfg.sample_size, cfg.sample_size)
        shape = (batch_size, cfg.in_channels, *ss)
        noise = randn_tensor(shape, generator, self.device)
        self.scheduler.set_timesteps(num_inference_steps)
        x = ops.nchw_to_nhwc_raw(noise.contiguous())
        x = self._run_steps(x, num_inference_steps, generator)
        x = self._decode(x)
        img = ops.to_image01_raw(x)                               # (x/2+0.5).clamp(0,1); already NHWC
        if output_type == "tensor":
            return SimpleNamespace(images=img)
        images = img.cpu().numpy()
        if output_type == "pil":
            from PIL import Image
            images = [Image.fromarray((im * 255).round().astype("uint8").squeeze()) for im in images]
        return SimpleNamespace(images=images)


class LDMPipeline(DDPMPipeline):
    """diffusers.LDMPipeline as the reference drives it for CelebA-HQ (src/diffusion_utils.py:393-412, unlearn.py:753-765):
    the same denoising loop on 3x64x64 latents, then `latents / vqvae.config.scaling_factor` through `vqvae.decode` and the
    usual (x/2+0.5).clamp(0,1).  The VQ-VAE is any module with diffusers' decode protocol (hub-fetched in the reference,
    `CompVis/ldm-celebahq-256`); with `vqvae=None` - what `--precompute_stage reuse` leaves the reference with
    (main.py:531-533) - the pipeline returns the latents through the same post-processing."""

    def __init__(self, unet, vqvae=None, scheduler=None):
        super().__init__(unet, scheduler if scheduler is not None else DDIMScheduler())
        self.vqvae = vqvae

    def _decode(self, x_nhwc):
        if self.vqvae is None:
            return x_nhwc
        lat = ops.nhwc_to_nchw_raw(x_nhwc) / float(getattr(self.vqvae.config, "scaling_factor", 1.0))
        img = self.vqvae.decode(lat).sample
        return ops.nchw_to_nhwc_raw(img.to(torch.float32).contiguous())

    @property
    def decoder(self):
        return LatentDecoder(self) if self.vqvae is not None else None


class LatentDecoder:
    """[N,C,h,w] latents as the pipeline samples and the latent dataset stores them (times scaling_factor) -> [N,3,H,W]
    images in [0,1] through the pipeline's own decode and post-processing; `tag` names the weights behind it."""

    def __init__(self, pipeline, batch=64):
        self.pipeline, self.batch = pipeline, batch
        self.tag = getattr(pipeline.vqvae, "tag", type(pipeline.vqvae).__name__)

    @torch.no_grad()
    def __call__(self, latents_nchw):
        p = self.pipeline
        out = []
        for s in range(0, len(latents_nchw), self.batch):
            x = ops.nchw_to_nhwc_raw(latents_nchw[s:s + self.batch].to(p.device, torch.float32).contiguous())
            out.append(ops.to_image01_raw(p._decode(x)).permute(0, 3, 1, 2))
        return torch.cat(out, 0)


class DDIMPipeline(DDPMPipeline):
    """Same loop; re-creates the scheduler from the given one's config like diffusers does."""

    def __init__(self, unet, scheduler):
        super().__init__(unet, DDIMScheduler.from_config(scheduler.config))


class StableDiffusionLatentPipeline:
    """The U-Net half of StableDiffusionPipeline.__call__ as driven by the reference's behaviour script
    (text_to_image/compute_model_behaviors.py:311-326): classifier-free guidance on a doubled batch and the
    scheduler update, returning LATENTS.  The VAE decoder and the CLIP text encoder (hub-fetched, frozen,
    off the hot path) stay outside: the caller passes prompt / negative-prompt embeddings and decodes.
    Scheduler: the sampler class shipped with miniSD is unknown offline, so it is a parameter - a DDIMScheduler
    (the default, `sd_scheduler("ddim")`: one gad_cfg_ddim_step per step) or a PNDMScheduler (`sd_scheduler("pndm")`, what
    SD-1.x repositories normally ship: len(timesteps) = num_inference_steps + 1 U-Net calls, one gad_plms_step each)."""

    def __init__(self, unet, scheduler=None):
        from .schedulers import sd_scheduler
        self.unet = unet
        self.scheduler = scheduler or sd_scheduler("ddim")
        self.device = unet.device

    @torch.no_grad()
    def __call__(self, prompt_embeds, negative_prompt_embeds, num_inference_steps=100, guidance_scale=7.5,
                 generator=None, height=None, width=None, callback=None):
        """callback(step_idx, t, latents): called after every scheduler update with the updated NCHW latents (a copy) - the
        diffusers `callback` hook that grad_text_to_image_lora.py uses to collect the journey of a generation."""
        cfg = self.unet.config
        B = prompt_embeds.shape[0]
        hw = (height or cfg.sample_size * 8) // 8, (width or cfg.sample_size * 8) // 8
        shape = (B, cfg.in_channels, *hw)
        lat = randn_tensor(shape, generator, self.device)
        sch = self.scheduler
        sch.set_timesteps(num_inference_steps)
        x = ops.nchw_to_nhwc_raw((lat * sch.init_noise_sigma).contiguous())
        ctx = torch.cat([negative_prompt_embeds, prompt_embeds], 0).to(self.device, torch.float32).contiguous()
        t2 = torch.empty(2 * B, device=self.device, dtype=torch.int64)
        clip = sch.clip

        def predict(x, t2):
            return self.unet.forward_nhwc(torch.cat([x, x], 0), t2, ctx)

        def update(x, eps, t):
            if isinstance(sch, PNDMScheduler):
                sch.step_guided(eps, t, x, guidance_scale, out=x)
            else:
                a_t, a_p = sch.step_coefficients(t)
                ops.cfg_ddim_step_raw(x, eps, guidance_scale, a_t, a_p, clip, out=x)
        for i, t in denoising_steps(x, sch.timesteps.tolist(), t2, predict, update):
            if callback is not None:
                callback(i, t, ops.nhwc_to_nchw_raw(x))
        return SimpleNamespace(latents=ops.nhwc_to_nchw_raw(x))


def sd_simple_loss(unet, scheduler, latents0, prompt_embeds, timesteps, n_noises=3, generator=None):
    """compute_model_behaviors.py:391-417: mean over `n_noises` of MSE(unet(add_noise(z0, eps, t_list), t_list), eps)
    with the batch being the scheduler's whole timestep list."""
    dev = unet.device
    T = timesteps.shape[0]
    z = latents0.to(dev).expand(T, -1, -1, -1).contiguous()
    ctx = prompt_embeds.to(dev).expand(T, -1, -1).contiguous()
    total = 0.0
    with torch.no_grad():
        for _ in range(n_noises):
            eps = randn_tensor(z.shape, generator, dev)
            noisy = scheduler.add_noise(z, eps, timesteps.to(dev))
            pred = unet(noisy, timesteps.to(dev), ctx).sample
            loss, _ = ops.mse_fwd_bwd_raw(pred.contiguous(), eps)
            total += float(loss)
    return total / n_noises
