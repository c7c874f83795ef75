"""TEST INFRASTRUCTURE ONLY.  The local model behaviours as the reference computes them (unconditional_generation/unlearn.py:
871-948, calculate_local_scores.py:303-374), restated step for step for any backend's pipelines: per seed one batch-1 pipeline
call per model, the scikit-image metrics through oracle/skimage_ref.py, and the diffusion loss as n_noises forwards of the
scheduler's T timesteps on noise drawn draw by draw from a device generator seeded with the sample's seed.

On gad pipelines it uses only calls older than gad.local_model_behaviors (`pipeline(batch_size=1, generator=...)`,
`scheduler.add_noise`, `unet(...)`, `ops.mse_fwd_bwd_raw`), so it is the baseline the wide-launch engine is compared with."""
import numpy as np
import torch

from oracle.skimage_ref import nrmse_loops, ssim_loops

KEYS = ("mse", "nrmse", "ssim", "diffusion_loss")


def mse_f64(a, b):
    d = np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)
    return float(np.mean(d * d))


def _one_image(pipeline, seed, num_inference_steps):
    """[1][H][W][C] float numpy image in [0,1] of one seed (unlearn.py:861-869)"""
    return np.asarray(pipeline(batch_size=1, generator=torch.Generator().manual_seed(seed),
                               num_inference_steps=num_inference_steps, output_type="numpy").images)


def _mse_loss(pred, noise):
    if pred.is_cuda:
        from gad import ops
        return ops.mse_fwd_bwd_raw(pred.contiguous(), noise.contiguous())[0][0]
    return torch.nn.functional.mse_loss(pred, noise)


def local_behaviors_loop(full_pipeline, pipeline, n_samples, n_noises, num_inference_steps, full_images=None, with_metrics=True,
                         return_images=False):
    """-> {"mse", "nrmse", "ssim", "diffusion_loss"}: lists of n_samples floats.  full_images ([n][H][W][C] in [0,1]) replaces
    the full model's pipeline calls; with_metrics=False skips the (slow, pure-python) image metrics and returns NaN for them;
    return_images=True adds the images of both models ("full_images", "images": [n][H][W][C] numpy) to the result."""
    fulls, removals = [], []
    dev = torch.device(pipeline.device)
    out = {k: [] for k in KEYS}
    for seed in range(n_samples):
        if full_images is None:
            full = _one_image(full_pipeline, seed, num_inference_steps)
        else:
            full = np.asarray(torch.as_tensor(full_images[seed:seed + 1]).detach().cpu().float())
        removal = _one_image(pipeline, seed, num_inference_steps)
        fulls.append(full[0])
        removals.append(removal[0])
        if with_metrics:
            out["mse"].append(mse_f64(full[0], removal[0]))
            out["nrmse"].append(nrmse_loops(full[0], removal[0]))
            out["ssim"].append(ssim_loops(full[0], removal[0], data_range=1.0))
        else:
            for k in KEYS[:3]:
                out[k].append(float("nan"))
        # the post-processed [0,1] image goes to add_noise as it is (unlearn.py:913-943)
        x0 = torch.from_numpy(full).permute(0, 3, 1, 2).to(dev)
        pipeline.scheduler.set_timesteps(num_inference_steps)
        timesteps = pipeline.scheduler.timesteps.to(dev)
        gen = torch.Generator(device=dev).manual_seed(seed)
        with torch.no_grad():
            vqvae = getattr(pipeline, "vqvae", None)
            if vqvae is not None and hasattr(vqvae, "encode"):
                x0 = vqvae.encode(x0, False)[0] * vqvae.config.scaling_factor
            rows = x0.expand(timesteps.shape[0], -1, -1, -1).contiguous()
            total = 0
            for _ in range(n_noises):
                noises = torch.randn((timesteps.shape[0], *x0.shape[1:]), generator=gen, device=dev)
                noisy = pipeline.scheduler.add_noise(rows, noises, timesteps)
                pred = pipeline.unet(noisy, timesteps).sample
                total = total + _mse_loss(pred, noises)
            total = total / n_noises
        out["diffusion_loss"].append(float(total))
    if return_images:
        out["full_images"], out["images"] = np.stack(fulls), np.stack(removals)
    return out
