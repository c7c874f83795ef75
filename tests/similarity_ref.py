"""The arithmetic of the similarity baselines, restated for the tests (no GPU, none of the project's kernels):
cosine in fp64 from the exact fp32 / table values, the torch-CPU fp32 form of the reference's statements, group max / avg and
the rank files' order."""
import numpy as np
import torch


def pixel_lut():
    """byte -> the fp32 value of ToTensor + Normalize([0.5], [0.5]): every step rounded to fp32"""
    out = np.empty(256, dtype=np.float32)
    for u in range(256):
        out[u] = np.float32(np.float32(np.float32(u) / np.float32(255.0)) - np.float32(0.5)) / np.float32(0.5)
    return out


def decode(x):
    """uint8 [N, D] -> the fp32 matrix the kernel contracts; fp32 passes through"""
    x = np.asarray(x)
    return pixel_lut()[x] if x.dtype == np.uint8 else x.astype(np.float32, copy=False)


def cosine64(x, q):
    """[N, D] (uint8 or fp32), [M, D] fp32 -> [N, M] float64 cosines of the exact operand values"""
    a, b = decode(x).astype(np.float64), np.asarray(q, dtype=np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (a @ b.T) / (np.sqrt((a * a).sum(1))[:, None] * np.sqrt((b * b).sum(1))[None, :])


def cosine_torch32(x, q):
    """The reference's statements on torch-CPU fp32: normalise the rows of X, normalise q, matmul - one q at a time"""
    a = torch.from_numpy(decode(x).copy())
    a = a / a.norm(dim=-1, keepdim=True)
    cols = []
    for row in torch.from_numpy(np.asarray(q, dtype=np.float32).copy()):
        row = row / row.norm(dim=-1, keepdim=True)
        cols.append(torch.matmul(a, row).numpy())
    return np.stack(cols, axis=1).astype(np.float32)


def tolerance(D):
    """|sim - sim64| <= (D + 16) 2^-24: the first-order bound of an fp32 dot product in any summation order, relative to
    |x||q| by Cauchy-Schwarz, with 16 units for the norms' square roots, their product and the quotient"""
    return (D + 16) * 2.0 ** -24


def group_max_avg(sim, group_indices):
    """float32 [N, M] -> (max, avg) float64 [G, M]: per group and column, the max and the mean rounded to float32 (from the
    exact fp64 sum: equal to a float32 mean wherever the float32 sum is exact, within the group size in ulps elsewhere)"""
    sim = np.asarray(sim, dtype=np.float32)
    G, M = len(group_indices), sim.shape[1]
    gmax, gavg = np.empty((G, M), dtype=np.float64), np.empty((G, M), dtype=np.float64)
    for g, idx in enumerate(group_indices):
        for m in range(M):
            col = sim[np.asarray(idx), m].astype(np.float64)
            gmax[g, m] = np.max(col)
            gavg[g, m] = float(np.float32(np.sum(col) / len(col)))
    return gmax, gavg


def stable_rank(values):
    """descending order of a vector, ties by index: the rank files"""
    values = np.asarray(values)
    return np.array(sorted(range(len(values)), key=lambda i: (-values[i], i)), dtype=np.int64)
