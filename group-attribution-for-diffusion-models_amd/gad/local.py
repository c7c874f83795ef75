"""Local model behaviours of the unconditional models (reference unconditional_generation/unlearn.py:871-948 and
calculate_local_scores.py:303-374): per generated image, how the coalition model differs from the full model on that sample
- MSE / NRMSE / SSIM between the two models' images from the same seed, and the coalition model's diffusion loss on the full
model's image at the sampler's timesteps.

The reference issues this as batch-1 trajectories and 100-row loss batches.  Here the same numbers come from launches as wide
as the sampler's: the seeds' trajectories are stacked along N (`FusedSampler`, per-seed host noise, bit-identical), all image
pairs go through one `gad_image_metrics` launch (fp64), and the loss runs whole noise draws - about `rows_per_launch` rows -
through `gad_add_noise_bcast -> UNet2DModel.forward_nhwc -> gad_mse_segments`.  Nothing between generation and the final
`[n_samples]` results touches the host."""
from __future__ import annotations

import torch

from . import _capi, ops
from .coalition import FusedSampler
from .nn import UNet2DModel
from .schedulers import DDIMScheduler

KEYS = ("mse", "nrmse", "ssim", "diffusion_loss")


class LocalBehaviors(dict):
    """The four per-image lists (KEYS), plus what the engine did: `launch_rows` (rows of every loss launch), `x0_space`
    ("image", "vqvae-latent", or "latent-as-image" when an LDM pipeline without its VQ-VAE hands its latents through the image
    post-processing).  With `return_images=True` the dict also holds the NHWC [0,1] device images of both models under
    "full_images" and "images"."""
    launch_rows = ()
    x0_space = "image"


def _check(pipe, what):
    if not isinstance(pipe.unet, UNet2DModel) or pipe.unet.device.type != "cuda":
        raise _capi.GadError(f"local_model_behaviors: the {what} pipeline needs a gad.UNet2DModel on the GPU (no CPU path)")
    if not isinstance(pipe.scheduler, DDIMScheduler):
        raise _capi.GadError(f"local_model_behaviors: the {what} pipeline samples with {type(pipe.scheduler).__name__}; "
                             "the wide-launch sampler implements DDIM (what the reference's pipelines use)")


def generate_local_images(pipeline, seeds, num_inference_steps, fuse):
    """Image s = pipeline(batch_size=1, generator=torch.Generator().manual_seed(s), output_type="numpy"), for every seed, `fuse`
    trajectories per launch -> NHWC float images in [0,1] on the device (no uint8 round trip)."""
    fs = FusedSampler(pipeline.unet, pipeline.scheduler, batch_size=1, fuse=fuse)
    out = []
    for g0 in range(0, len(seeds), fuse):
        grp = list(seeds[g0:g0 + fuse])
        x = fs.initial_noise(grp, [1] * len(grp))
        img = fs.denoise(x, num_inference_steps)                 # x holds the final x_0 afterwards (updated in place)
        if getattr(pipeline, "vqvae", None) is not None:
            img = ops.to_image01_raw(pipeline._decode(x))
        out.append(img)
    return out[0] if len(out) == 1 else torch.cat(out, 0)


@torch.no_grad()
def local_model_behaviors(full_pipeline, pipeline, n_samples, n_noises, num_inference_steps, *, rows_per_launch=1000,
                          full_images=None, return_images=False):
    """-> LocalBehaviors: {"mse", "nrmse", "ssim", "diffusion_loss"}, each a list of `n_samples` floats, image s from seed s.

    full_images: the full model's NHWC [0,1] images of seeds 0..n_samples-1 (they do not depend on the coalition: a caller
    scoring many coalitions generates them once, `return_images=True`, and passes them back in)."""
    if n_samples < 1 or n_noises < 1 or rows_per_launch < 1:
        raise ValueError("n_samples, n_noises and rows_per_launch must be >= 1")
    _check(pipeline, "removal")
    dev = pipeline.unet.device
    nets = [pipeline.unet] + ([full_pipeline.unet] if full_images is None else [])
    was_training = [n.training for n in nets]
    for n in nets:
        n.eval()
    try:
        seeds = list(range(n_samples))
        fuse = min(n_samples, rows_per_launch)
        # ---- 1. generation ----
        if full_images is None:
            _check(full_pipeline, "full")
            full = generate_local_images(full_pipeline, seeds, num_inference_steps, fuse)
        else:
            full = torch.as_tensor(full_images).to(dev, torch.float32).contiguous()
            if full.ndim != 4 or full.shape[0] != n_samples:
                raise ValueError(f"full_images: expected [{n_samples}][H][W][C], got {tuple(full.shape)}")
        removal = generate_local_images(pipeline, seeds, num_inference_steps, fuse)
        # ---- 2. image metrics: one launch over all pairs ----
        metrics = ops.image_metrics_raw(full, removal, win=7, data_range=1.0)
        # ---- 3. diffusion loss of the removal model on the full model's images ----
        x0 = ops.nhwc_to_nchw_raw(full)                           # the post-processed [0,1] image as it is (unlearn.py:913-943)
        vqvae = getattr(pipeline, "vqvae", None)
        space = "image"
        if vqvae is not None and hasattr(vqvae, "encode"):        # unlearn.py:930-932
            x0 = (vqvae.encode(x0, False)[0] * float(getattr(vqvae.config, "scaling_factor", 1.0))).to(torch.float32).contiguous()
            space = "vqvae-latent"
        elif hasattr(pipeline, "vqvae") and type(pipeline).__name__ == "LDMPipeline":
            space = "latent-as-image"
        sch = pipeline.scheduler
        sch.set_timesteps(num_inference_steps)
        ts = sch.timesteps.to(dev, torch.int64).contiguous()
        T = ts.shape[0]
        ac = sch._ac_on(dev)
        _, C, H, W = x0.shape
        per_image = n_noises * T
        group = max(1, rows_per_launch // per_image)              # images per launch when one image's draws are few
        draws = n_noises if group > 1 else min(n_noises, max(1, rows_per_launch // T))   # draws per launch otherwise
        max_rows = group * per_image if group > 1 else draws * T
        eps = torch.empty((min(group, n_samples) * per_image, C, H, W), device=dev, dtype=torch.float32)
        xt = torch.empty((max_rows, H, W, C), device=dev, dtype=torch.float32)
        t_rows = ts.repeat(max_rows // T)
        seg = torch.empty(n_samples * n_noises, device=dev, dtype=torch.float32)
        launch_rows = []

        def launch(e, x0_part, rows_per_image, seg_out):
            rows = e.shape[0]
            ops.add_noise_bcast_raw(x0_part, e, ts, ac, rows_per_image, out=xt[:rows])
            pred = pipeline.unet.forward_nhwc(xt[:rows], t_rows[:rows])
            ops.mse_segments_raw(pred, e, T, out=seg_out)
            launch_rows.append(rows)

        for s0 in range(0, n_samples, group):
            k = min(group, n_samples - s0)
            for i in range(k):
                # one randn per draw, in order: the values the reference's loop sees from this generator on this device
                g = torch.Generator(device=dev).manual_seed(s0 + i)
                for d in range(n_noises):
                    at = (i * n_noises + d) * T
                    torch.randn((T, C, H, W), generator=g, out=eps[at:at + T])
            if group > 1:
                launch(eps[:k * per_image], x0[s0:s0 + k], per_image, seg[s0 * n_noises:(s0 + k) * n_noises])
            else:
                for d0 in range(0, n_noises, draws):
                    d1 = min(n_noises, d0 + draws)
                    launch(eps[d0 * T:d1 * T], x0[s0:s0 + 1], (d1 - d0) * T, seg[s0 * n_noises + d0:s0 * n_noises + d1])
        loss = seg.view(n_samples, n_noises).double().mean(1)
        host = torch.cat([metrics, loss[:, None]], 1).cpu()       # the one transfer: [n_samples][4] fp64
    finally:
        for n, tr in zip(nets, was_training):
            n.train(tr)
    res = LocalBehaviors({k: host[:, j].tolist() for j, k in enumerate(KEYS)})
    res.launch_rows, res.x0_space = tuple(launch_rows), space
    if return_images:
        res["full_images"], res["images"] = full, removal
    return res
