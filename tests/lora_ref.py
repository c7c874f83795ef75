"""Test-side restatement of LoRA unlearning (gad/lora.py, csrc/lora.hip): the dropout keep mask in numpy (Philox as restated in
tests/jl_ref.py), peft's LoRA layer in torch - at whatever dtype the wrapped oracle model has, double in the GPU tests - taking
its masks from that function, and the LoRA+ Adam step in fp64.  Never imported by the product."""
import math

import numpy as np
import torch
import torch.nn as nn

from jl_ref import MASK, philox4x32_10

QKV = ("to_q", "to_k", "to_v")


def keep_words(seed, offset, layer, j, rows, C):
    """the 32-bit word of every (row, channel): Philox-4x32-10, key (seed, offset), counter (c >> 2, m lo, m hi, (layer << 2) | j),
    channel c takes word c & 3 -> uint64 [len(rows), C]"""
    rows = np.asarray(rows, dtype=np.uint64)
    blocks = (C + 3) // 4
    ctr = np.zeros((len(rows), blocks, 4), dtype=np.uint64)
    ctr[..., 0] = np.arange(blocks, dtype=np.uint64)[None, :]
    ctr[..., 1] = (rows & np.uint64(MASK))[:, None]
    ctr[..., 2] = (rows >> np.uint64(32))[:, None]
    ctr[..., 3] = np.uint64((layer << 2) | j)
    return philox4x32_10(ctr, (seed & MASK, offset & MASK)).reshape(len(rows), blocks * 4)[:, :C]


def threshold(p):
    return int(math.floor(p * 2.0 ** 32))


def keep_mask(seed, offset, layer, j, M, C, p, row0=0):
    """bool [M, C]: element kept when its word >= floor(p 2^32); p = 0 keeps everything"""
    return keep_words(seed, offset, layer, j, np.arange(row0, row0 + M), C) >= np.uint64(threshold(p))


def down_fwd(x, As, scale, p, seed, offset, layer):
    """fp64 mid_j = scale (x o m_j / (1 - p)) A_j^T and the bound's sum_c |x m a| -> ([mid_j], [abs sums])"""
    x = np.asarray(x, dtype=np.float64)
    out, mag = [], []
    for j, A in enumerate(As):
        xm = x * keep_mask(seed, offset, layer, j, *x.shape, p)
        A = np.asarray(A, dtype=np.float64)
        out.append(scale / (1.0 - p) * (xm @ A.T))
        mag.append(np.abs(xm) @ np.abs(A).T)
    return out, mag


def down_bwd(x, As, dmids, dx0, p, seed, offset, layer):
    """fp64 dA_j = dmid_j^T (x o m_j / (1 - p)), dx = dx0 + sum_j (dmid_j A_j) o m_j / (1 - p), and the two bounds' abs sums
    -> ([dA_j], dx, [sum_m |dmid x m|], sum_j sum_r |dmid a| m)"""
    x = np.asarray(x, dtype=np.float64)
    dx = np.asarray(dx0, dtype=np.float64).copy()
    dAs, magA, magx = [], [], np.zeros_like(dx)
    for j, (A, dm) in enumerate(zip(As, dmids)):
        keep = keep_mask(seed, offset, layer, j, *x.shape, p)
        A, dm = np.asarray(A, dtype=np.float64), np.asarray(dm, dtype=np.float64)
        dAs.append(dm.T @ (x * keep) / (1.0 - p))
        magA.append(np.abs(dm).T @ np.abs(x * keep))
        dx += (dm @ A) * keep / (1.0 - p)
        magx += (np.abs(dm) @ np.abs(A)) * keep
    return dAs, dx, magA, magx


class LoraLayer(nn.Module):
    """peft's LoRA branch as a `lora_layer` of the oracle's LoRACompatibleLinear: x -> B(A(dropout(x))) * lora_alpha / r.  The mask
    comes from `keep_mask` with this layer's (seed, offset, layer, j); rows are numbered batch-major over the flattened tokens."""

    def __init__(self, in_f, out_f, r, lora_alpha, p, seed, layer, j, dtype=torch.float32):
        super().__init__()
        a, b = nn.Linear(in_f, r, bias=False), nn.Linear(r, out_f, bias=False)      # the recipe's draws from the CPU generator
        nn.init.kaiming_uniform_(a.weight, a=math.sqrt(5))
        nn.init.zeros_(b.weight)
        self.A, self.B = nn.Parameter(a.weight.detach().to(dtype)), nn.Parameter(b.weight.detach().to(dtype))
        self.scale, self.p, self.seed, self.layer, self.j, self.offset = lora_alpha / r, p, seed, layer, j, 0

    def forward(self, x):
        x2 = x.reshape(-1, x.shape[-1])
        if self.training and self.p > 0:
            keep = keep_mask(self.seed, self.offset, self.layer, self.j, *x2.shape, self.p)
            x2 = x2 * torch.from_numpy(keep).to(x2.dtype) / (1.0 - self.p)
        return (x2 @ self.A.T @ self.B.T * self.scale).reshape(*x.shape[:-1], -1)


def attentions(model):
    return [m for m in model.modules() if all(hasattr(m, n) for n in QKV)]


def get_peft_model(model, r, lora_alpha, p, seed):
    """freeze the oracle model and give every attention block's to_q / to_k / to_v a LoraLayer (module order)"""
    for q in model.parameters():
        q.requires_grad_(False)
    dtype = next(model.parameters()).dtype
    for layer, m in enumerate(attentions(model)):
        for j, n in enumerate(QKV):
            lin = getattr(m, n)
            lin.set_lora_layer(LoraLayer(lin.in_features, lin.out_features, r, lora_alpha, p, seed, layer, j, dtype))
    return model


def lora_layers(model):
    """[[LoraLayer of to_q, to_k, to_v]] per attention block"""
    return [[getattr(m, n).lora_layer for n in QKV] for m in attentions(model) if m.to_q.lora_layer is not None]


def set_offset(model, offset):
    for ls in lora_layers(model):
        for l in ls:
            l.offset = offset


@torch.no_grad()
def merge_and_unload(model):
    for m in attentions(model):
        for n in QKV:
            lin = getattr(m, n)
            if lin.lora_layer is not None:
                lin.weight.add_(lin.lora_layer.scale * (lin.lora_layer.B @ lin.lora_layer.A).to(lin.weight.dtype))
                lin.set_lora_layer(None)
    return model


class LoraPlusAdam:
    """fp64 Adam (torch's defaults, no weight decay) over [all A | all B] with one clip norm over every gradient
    (clip_grad_norm_: coefficient min(1, max_norm / (norm + 1e-6))) and the B matrices at `ratio` times the A matrices' rate"""

    def __init__(self, As, Bs, lr, ratio=16.0, betas=(0.9, 0.999), eps=1e-8, max_norm=1.0):
        self.p = [np.asarray(a, dtype=np.float64).copy() for a in list(As) + list(Bs)]
        self.lr = [lr] * len(As) + [lr * ratio] * len(Bs)
        self.m, self.v = [np.zeros_like(a) for a in self.p], [np.zeros_like(a) for a in self.p]
        self.betas, self.eps, self.max_norm, self.t = betas, eps, max_norm, 0

    def step(self, grads):
        grads = [np.asarray(g, dtype=np.float64) for g in grads]
        norm = math.sqrt(sum(float((g * g).sum()) for g in grads))
        clip = min(1.0, self.max_norm / (norm + 1e-6))
        self.t += 1
        b1, b2 = self.betas
        for i, g in enumerate(grads):
            g = g * clip
            self.m[i] = b1 * self.m[i] + (1 - b1) * g
            self.v[i] = b2 * self.v[i] + (1 - b2) * g * g
            denom = np.sqrt(self.v[i]) / math.sqrt(1 - b2 ** self.t) + self.eps
            self.p[i] -= self.lr[i] / (1 - b1 ** self.t) * self.m[i] / denom
        return norm
