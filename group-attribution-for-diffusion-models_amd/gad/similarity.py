"""Similarity baselines of the text-to-image experiment (reference text_to_image/pixel_similarity.py, clip_similarity.py,
baselines.py, aesthetic_score.py): every cosine between training rows and generated rows in one launch (csrc/similarity.hip),
and the host statements that turn the matrix into the group arrays and rank files text_to_image/baseline_lds.py reads."""
from __future__ import annotations

import os

import numpy as np
import torch

from . import _capi, ops
from ._capi import check

_LUTS = {}


def pixel_lut():
    """The 256 fp32 values ToTensor + Normalize([0.5], [0.5]) give a byte: ((float)u / 255.0f - 0.5f) / 0.5f, in fp32 steps."""
    u = np.arange(256, dtype=np.float32)
    return (u / np.float32(255.0) - np.float32(0.5)) / np.float32(0.5)


def _lut(device):
    key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
    if key not in _LUTS:
        _LUTS[key] = torch.from_numpy(pixel_lut()).to(device)
    return _LUTS[key]


def _rows(t, name, dtypes):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _capi.GadError(f"cosine_rows: {name} must be a device tensor (there is no CPU path)")
    if t.dtype not in dtypes or t.dim() < 2:
        raise _capi.GadError(f"cosine_rows: {name} must be [rows, ...] of {' or '.join(str(d) for d in dtypes)}, got "
                             f"{t.dtype} {tuple(t.shape)}")
    if t.dim() > 2 or t.stride(1) != 1 or t.stride(0) < t.shape[1]:
        t = t.reshape(t.shape[0], -1)
        if t.stride(1) != 1 or t.stride(0) < t.shape[1]:
            t = t.contiguous()
    return t


def cosine_rows(X, Q, *, splits=0):
    """sim [N, M] fp32 = cosine of every row of X [N, ...] (float32, or uint8 pixels read as (u / 255 - 0.5) / 0.5) with every
    row of Q [M, ...] (float32, the same trailing size), by gad_cosine_rows.  A row-major 2-D view with a row stride is taken
    as it is.  `splits`: 0 lets the launch choose how many ways the contraction is cut, a positive value forces that many."""
    x, q = _rows(X, "X", (torch.float32, torch.uint8)), _rows(Q, "Q", (torch.float32,))
    if x.device != q.device or x.shape[1] != q.shape[1]:
        raise _capi.GadError(f"cosine_rows: X {tuple(x.shape)} on {x.device} and Q {tuple(q.shape)} on {q.device} must share "
                             "the device and the row length")
    u8 = x.dtype == torch.uint8
    kind = _capi.SIM_X_U8 if u8 else _capi.SIM_X_F32
    (N, D), M = x.shape, q.shape[0]
    lib = _capi.load()
    nbytes = lib.gad_cosine_rows_workspace_bytes(N, M, D, kind, splits)
    check(nbytes < 0, "gad_cosine_rows_workspace_bytes")
    with torch.cuda.device(x.device):
        lut = _lut(x.device) if u8 else None
        ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        sim = torch.empty((N, M), dtype=torch.float32, device=x.device)
        check(lib.gad_cosine_rows(x.data_ptr(), kind, x.stride(0), ops._ptr(lut), q.data_ptr(), q.stride(0), sim.data_ptr(),
                                  N, M, D, splits, ws.data_ptr(), nbytes, ops._stream()), "gad_cosine_rows")
    return sim


def group_aggregate(sim, group_indices):
    """(max [G, M], avg [G, M]) float64 of a float32 matrix sim [N, M] over the groups' rows: the reference's statements
    (baselines.py:266-279) - `.max(axis=0)` / `.mean(axis=0)` on the float32 rows, assigned into float64 zeros.  A vector
    [N] is taken as [N, 1] (aesthetic_score.py:137-144).  `group_indices`: a sequence of index arrays or a dict i -> array."""
    sim = np.asarray(sim)
    if sim.ndim == 1:
        sim = sim[:, None]
    items = list(group_indices.items()) if isinstance(group_indices, dict) else list(enumerate(group_indices))
    gmax = np.zeros(shape=(len(items), sim.shape[1]))
    gavg = np.zeros(shape=(len(items), sim.shape[1]))
    for i, idx in items:
        idx = np.asarray(idx)
        if idx.size == 0:
            raise ValueError(f"group {i} has no training image (max of an empty group)")
        rows = sim[idx, :]
        gmax[i, :] = rows.max(axis=0)
        gavg[i, :] = rows.mean(axis=0)
    return gmax, gavg


def write_baselines(output_dir, group, outputs, per_image=True):
    """The reference's files under {output_dir}/baselines for every name -> [G, M] array of `outputs`:
    {group}_{name}.npy, generated_image_{i}_{group}_rank_{name}.npy (when `per_image`; baselines.py:296-306) and
    all_generated_images_{group}_rank_{name}.npy - stable argsort of the negated column / of the negated row means
    (baselines.py:307, which is aesthetic_score.py:169 at M = 1).  Returns the directory."""
    out = os.path.join(output_dir, "baselines")
    os.makedirs(out, exist_ok=True)
    for name, arr in outputs.items():
        arr = np.asarray(arr)
        if arr.ndim != 2:
            raise ValueError(f"write_baselines: {name} must be [groups, images], got {arr.shape}")
        np.save(os.path.join(out, f"{group}_{name}.npy"), arr)
        if per_image:
            for i in range(arr.shape[1]):
                np.save(os.path.join(out, f"generated_image_{i}_{group}_rank_{name}.npy"), np.argsort(-arr[:, i], kind="stable"))
        np.save(os.path.join(out, f"all_generated_images_{group}_rank_{name}.npy"), np.argsort(-arr.mean(axis=-1), kind="stable"))
    return out
