"""numpy fp64 restatement of gad_latent_draw (include/gad.h) on Philox-4x32-10 as restated in jl_ref: key = the 64-bit seed,
the flip coin from counter (0xFFFFFFFF, r, step, 3), the noise from counter (e >> 2, r, step, 3) through the projector's uniform
and Box-Muller maps, and the reparameterised sample in fp64, fed the same fp32 moments."""
import numpy as np

from jl_ref import MASK, philox4x32_10, uniform

TAG, COIN_BLOCK = 3, 0xFFFFFFFF


def _key(seed):
    s = int(seed) & 0xFFFFFFFFFFFFFFFF
    return s & MASK, s >> 32


def latent_coin(seed, rows, step):
    """bit 0 of word 0 of philox4x32_10([0xFFFFFFFF, r, step, 3], (seed lo, seed hi)) for every r of `rows` -> int array"""
    rows = np.asarray(rows, dtype=np.uint64)
    ctr = np.zeros((len(rows), 4), dtype=np.uint64)
    ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3] = COIN_BLOCK, rows, int(step) & MASK, TAG
    return (philox4x32_10(ctr, _key(seed))[:, 0] & np.uint64(1)).astype(np.int64)


def latent_noise(seed, r, step, n):
    """z [n] in fp64: element e is word e & 3 of philox4x32_10([e >> 2, r, step, 3], key) mapped r01 cos, r01 sin, r23 cos,
    r23 sin (the exact Box-Muller of the kernel's fp32 uniforms)"""
    blocks = (n + 3) // 4
    ctr = np.zeros((blocks, 4), dtype=np.uint64)
    ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3] = np.arange(blocks, dtype=np.uint64), int(r), int(step) & MASK, TAG
    u = uniform(philox4x32_10(ctr, _key(seed)))
    r01 = np.sqrt(-2.0 * np.log(u[:, 0]))
    r23 = np.sqrt(-2.0 * np.log(u[:, 2]))
    z = np.stack([r01 * np.cos(2 * np.pi * u[:, 1]), r01 * np.sin(2 * np.pi * u[:, 1]),
                  r23 * np.cos(2 * np.pi * u[:, 3]), r23 * np.sin(2 * np.pi * u[:, 3])], axis=-1)
    return z.reshape(-1)[:n]


def latent_draw(moments, rows, seed, step, scale, sample=True, random_flip=False):
    """moments [N][F][2][n] (fp32 values), rows [B] -> dict of fp64 arrays [B][n]: m, std, z, x0, and flipped [B]"""
    mo = np.asarray(moments, dtype=np.float64)
    N, F = mo.shape[:2]
    mo = mo.reshape(N, F, 2, -1)
    n = mo.shape[3]
    rows = np.clip(np.asarray(rows, dtype=np.int64), 0, N - 1)
    flipped = latent_coin(seed, rows, step) if (random_flip and F == 2) else np.zeros(len(rows), dtype=np.int64)
    m = np.stack([mo[r, f, 0] for r, f in zip(rows, flipped)])
    lv = np.stack([mo[r, f, 1] for r, f in zip(rows, flipped)])
    std = np.exp(0.5 * np.clip(lv, -30.0, 20.0))
    scale = float(np.float32(scale))
    if sample:
        z = np.stack([latent_noise(seed, r, step, n) for r in rows])
        x0 = scale * (m + std * z)
    else:
        z = np.zeros_like(m)
        x0 = scale * m
    return dict(m=m, std=std, z=z, x0=x0, flipped=flipped)
