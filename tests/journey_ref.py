"""numpy fp64 restatement of gad_ddpm_step (include/gad.h): the variance noise from Philox-4x32-10 as restated in jl_ref
(key = the row's 64-bit seed, counter (e >> 2, t, 0, 2), the projector's uniform and Box-Muller maps) and the ancestral DDPM
update in fp64, fed the same fp32 inputs."""
import numpy as np

from jl_ref import MASK, philox4x32_10, uniform


def ddpm_noise(seeds, t, n):
    """z [len(seeds)][n] in fp64: element e of row b is word e & 3 of philox4x32_10([e >> 2, t, 0, 2], (seed lo, seed hi))
    mapped r01 cos, r01 sin, r23 cos, r23 sin (the exact Box-Muller of the kernel's fp32 uniforms)"""
    blocks = (n + 3) // 4
    ctr = np.zeros((blocks, 4), dtype=np.uint64)
    ctr[:, 0] = np.arange(blocks, dtype=np.uint64)
    ctr[:, 1] = t
    ctr[:, 3] = 2
    rows = []
    for s in seeds:
        s = int(s) & 0xFFFFFFFFFFFFFFFF
        u = uniform(philox4x32_10(ctr, (s & MASK, s >> 32)))            # [blocks][4]
        r01 = np.sqrt(-2.0 * np.log(u[:, 0]))
        r23 = np.sqrt(-2.0 * np.log(u[:, 2]))
        z = np.stack([r01 * np.cos(2 * np.pi * u[:, 1]), r01 * np.sin(2 * np.pi * u[:, 1]),
                      r23 * np.cos(2 * np.pi * u[:, 3]), r23 * np.sin(2 * np.pi * u[:, 3])], axis=-1)
        rows.append(z.reshape(-1)[:n])
    return np.stack(rows)


def ddpm_step(x, eps, seeds, t, a_t, a_prev, clip, variance_type):
    """x, eps [B][n] (fp32 values), a_t / a_prev the fp32 table values -> dict of fp64 arrays and coefficients:
    x0 (after the clamp), clipped (where the clamp acted), mean, z, x_prev, and c0, c1, sigma, sa, sb"""
    x = np.asarray(x, dtype=np.float64)
    eps = np.asarray(eps, dtype=np.float64)
    a_t, a_prev = float(np.float32(a_t)), float(np.float32(a_prev))
    cur_alpha = a_t / a_prev
    sa, sb = np.sqrt(a_t), np.sqrt(1.0 - a_t)
    c0 = np.sqrt(a_prev) * (1.0 - cur_alpha) / (1.0 - a_t)
    c1 = np.sqrt(cur_alpha) * (1.0 - a_prev) / (1.0 - a_t)
    raw = (x - sb * eps) / sa
    clipped = (np.abs(raw) > clip) if clip > 0 else np.zeros(raw.shape, dtype=bool)
    x0 = np.clip(raw, -clip, clip) if clip > 0 else raw
    mean = c0 * x0 + c1 * x
    if variance_type == "fixed_small":
        var = max((1.0 - a_prev) / (1.0 - a_t) * (1.0 - cur_alpha), 1e-20)
    elif variance_type == "fixed_large":
        var = 1.0 - cur_alpha
    else:
        raise ValueError(variance_type)
    sigma = np.sqrt(var) if t > 0 else 0.0
    z = ddpm_noise(seeds, t, x.shape[1]) if t > 0 else np.zeros_like(x)
    return dict(x0=x0, clipped=clipped, mean=mean, z=z, x_prev=mean + sigma * z, c0=c0, c1=c1, sigma=sigma, sa=sa, sb=sb)
