"""numpy restatement of the random matrix of gad_jl_project (include/gad.h): Philox-4x32-10 with the Random123
constants, key (seed, model_id), counter (column block, row lo, row hi, type), and the two entry maps."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(ctr, key):
    """ctr: [..., 4] uint32-valued, key: (k0, k1) -> [..., 4] uint64 arrays holding 32-bit words"""
    ctr = np.asarray(ctr, dtype=np.uint64)
    c0, c1, c2, c3 = (ctr[..., i].copy() for i in range(4))
    k0, k1 = np.uint64(key[0] & MASK), np.uint64(key[1] & MASK)
    for _ in range(10):
        p0 = np.uint64(M0) * c0
        p1 = np.uint64(M1) * c2
        hi0, lo0 = p0 >> np.uint64(32), p0 & np.uint64(MASK)
        hi1, lo1 = p1 >> np.uint64(32), p1 & np.uint64(MASK)
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0 = (k0 + np.uint64(W0)) & np.uint64(MASK)
        k1 = (k1 + np.uint64(W1)) & np.uint64(MASK)
    return np.stack([c0, c1, c2, c3], axis=-1)


def uniform(x):
    """u = fl32(fl32(x) * 2^-32 + 2^-33): the fp64 sum is exact, so one rounding to fp32 equals the kernel's fma"""
    xf = np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)
    return (xf * 2.0 ** -32 + 2.0 ** -33).astype(np.float32).astype(np.float64)


def _counters(rows, blocks, type_):
    rows = np.asarray(rows, dtype=np.uint64)
    ctr = np.zeros((len(rows), len(blocks), 4), dtype=np.uint64)
    ctr[..., 0] = np.asarray(blocks, dtype=np.uint64)[None, :]
    ctr[..., 1] = (rows & np.uint64(MASK))[:, None]
    ctr[..., 2] = (rows >> np.uint64(32))[:, None]
    ctr[..., 3] = type_
    return ctr


def jl_rows(rows, d, seed, model_id=0, proj_type="normal"):
    """R[rows][:d] in fp64 (normal: the exact Box-Muller of the kernel's fp32 uniforms; rademacher: exact +-1)"""
    if proj_type == "normal":
        x = philox4x32_10(_counters(rows, np.arange(d // 4), 0), (seed, model_id))     # [n][d/4][4]
        u = uniform(x)
        r01 = np.sqrt(-2.0 * np.log(u[..., 0]))
        r23 = np.sqrt(-2.0 * np.log(u[..., 2]))
        z = np.stack([r01 * np.cos(2 * np.pi * u[..., 1]), r01 * np.sin(2 * np.pi * u[..., 1]),
                      r23 * np.cos(2 * np.pi * u[..., 3]), r23 * np.sin(2 * np.pi * u[..., 3])], axis=-1)
        return z.reshape(len(rows), -1)[:, :d]
    x = philox4x32_10(_counters(rows, np.arange((d + 127) // 128), 1), (seed, model_id))  # [n][d/128][4]
    j = np.arange(128)
    bits = (x[..., j // 32] >> (j % 32).astype(np.uint64)) & np.uint64(1)                 # [n][d/128][128]
    return (1.0 - 2.0 * bits.astype(np.float64)).reshape(len(rows), -1)[:, :d]


def jl_project(a, d, seed, model_id=0, proj_type="normal", p0=0, block=4096):
    """fp64 oracle of out = a[G][P] @ R[p0 : p0 + P][:d]"""
    a = np.asarray(a, dtype=np.float64)
    out = np.zeros((a.shape[0], d))
    for s in range(0, a.shape[1], block):
        e = min(a.shape[1], s + block)
        out += a[:, s:e] @ jl_rows(np.arange(p0 + s, p0 + e), d, seed, model_id, proj_type)
    return out
