"""Functional torch restatement of diffusers 0.24's AutoencoderKL / VQModel (encoder, decoder, mid-block attention, codebook
lookup), written from the architecture's description and independent of gad/vae.py: it takes a state dict in diffusers' key
grammar, a config (any object with kind, block_out_channels, layers_per_block, latent_channels, norm_num_groups,
vq_embed_dim) and a dtype.  In float64 it is the reference the HIP models are measured against; in float32 on the CPU it is
the yardstick (what another summation order costs) their bounds are multiples of.

Also the seeded inputs the CPU yardstick test and the GPU tests share."""
import math
from types import SimpleNamespace

import torch
import torch.nn.functional as F

EPS = 1e-6


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


class Net:
    def __init__(self, sd, cfg, dtype):
        self.sd = {k: v.detach().to(dtype) for k, v in sd.items()}
        self.cfg, self.dtype, self.G = cfg, dtype, cfg.norm_num_groups

    def conv(self, name, x, stride=1, padding=1):
        return F.conv2d(x, self.sd[name + ".weight"], self.sd[name + ".bias"], stride=stride, padding=padding)

    def norm(self, name, x):
        return F.group_norm(x, self.G, self.sd[name + ".weight"], self.sd[name + ".bias"], EPS)

    def resnet(self, p, x):
        h = self.conv(p + "conv1", F.silu(self.norm(p + "norm1", x)))
        h = self.conv(p + "conv2", F.silu(self.norm(p + "norm2", h)))
        if p + "conv_shortcut.weight" in self.sd:
            x = self.conv(p + "conv_shortcut", x, padding=0)
        return x + h

    def attention(self, p, x):
        B, C, H, W = x.shape
        n = self.norm(p + "group_norm", x).view(B, C, H * W).transpose(1, 2)
        lin = lambda name, t: F.linear(t, self.sd[p + name + ".weight"], self.sd[p + name + ".bias"])      # noqa: E731
        q, k, v = lin("to_q", n), lin("to_k", n), lin("to_v", n)
        o = torch.softmax(q @ k.transpose(1, 2) / math.sqrt(C), dim=-1) @ v
        return x + lin("to_out.0", o).transpose(1, 2).reshape(B, C, H, W)

    def mid(self, p, x):
        return self.resnet(p + "resnets.1.", self.attention(p + "attentions.0.", self.resnet(p + "resnets.0.", x)))

    def decoder(self, z):
        cfg, p = self.cfg, "decoder."
        x = self.mid(p + "mid_block.", self.conv(p + "conv_in", z.to(self.dtype)))
        n = len(cfg.block_out_channels)
        for i in range(n):
            for j in range(cfg.layers_per_block + 1):
                x = self.resnet(f"{p}up_blocks.{i}.resnets.{j}.", x)
            if i != n - 1:
                x = self.conv(f"{p}up_blocks.{i}.upsamplers.0.conv", F.interpolate(x, scale_factor=2.0, mode="nearest"))
        return self.conv(p + "conv_out", F.silu(self.norm(p + "conv_norm_out", x)))

    def encoder(self, x):
        cfg, p = self.cfg, "encoder."
        x = self.conv(p + "conv_in", x.to(self.dtype))
        n = len(cfg.block_out_channels)
        for i in range(n):
            for j in range(cfg.layers_per_block):
                x = self.resnet(f"{p}down_blocks.{i}.resnets.{j}.", x)
            if i != n - 1:
                x = self.conv(f"{p}down_blocks.{i}.downsamplers.0.conv", F.pad(x, (0, 1, 0, 1)), stride=2, padding=0)
        x = self.mid(p + "mid_block.", x)
        return self.conv(p + "conv_out", F.silu(self.norm(p + "conv_norm_out", x)))

    # ---- whole models ----
    def moments(self, x):
        """quant_conv(encoder(x)): KL's mean | logvar, VQ's unquantised latents"""
        return self.conv("quant_conv", self.encoder(x), padding=0)

    def lookup(self, h):
        """NCHW latents -> (indices [B,h,w], z + (e - z) as NCHW); exact-difference distances, lowest index on ties"""
        e = self.sd["quantize.embedding.weight"]
        rows = h.permute(0, 2, 3, 1).reshape(-1, h.shape[1])
        idx = vq_argmin(rows, e)
        zq = rows + (e[idx] - rows)
        return idx.view(h.shape[0], h.shape[2], h.shape[3]), zq.view(h.shape[0], h.shape[2], h.shape[3], -1).permute(0, 3, 1, 2)

    def decode(self, z, force_not_quantize=False):
        z = z.to(self.dtype)
        if self.cfg.kind == "vq" and not force_not_quantize:
            z = self.lookup(z)[1]
        return self.decoder(self.conv("post_quant_conv", z, padding=0))


def vq_distances(rows, e):
    """[n, K] of sum_c (z_c - e_c)^2 in the rows' dtype, channels summed in order"""
    d = torch.zeros(rows.shape[0], e.shape[0], dtype=rows.dtype)
    for c in range(rows.shape[1]):
        df = rows[:, c:c + 1] - e[:, c].unsqueeze(0)
        d += df * df
    return d


def vq_argmin(rows, e, chunk=1024):
    out = []
    for s in range(0, rows.shape[0], chunk):
        out.append(vq_distances(rows[s:s + chunk], e).argmin(dim=1))      # torch.argmin: the first of equal minima
    return torch.cat(out)


def vq_relative_gap(rows, e, chunk=1024):
    """per row, (second smallest - smallest) / smallest distance, in the given dtype (inf for a single code)"""
    gaps = []
    for s in range(0, rows.shape[0], chunk):
        two = torch.topk(vq_distances(rows[s:s + chunk], e), min(2, e.shape[0]), dim=1, largest=False).values
        gaps.append((two[:, -1] - two[:, 0]) / two[:, 0] if e.shape[0] > 1 else torch.full((two.shape[0],), math.inf, dtype=rows.dtype))
    return torch.cat(gaps)


def sdpa(q, k, v, heads=1):
    """[B, T, heads*d] operands -> softmax(q k^T / sqrt(d)) v in the operands' dtype"""
    B, Tq, C = q.shape
    Tk, d = k.shape[1], C // heads
    split = lambda t, T: t.view(B, T, heads, d).transpose(1, 2)      # noqa: E731
    w = torch.softmax(split(q, Tq) @ split(k, Tk).transpose(-1, -2) / math.sqrt(d), dim=-1)
    return (w @ split(v, Tk)).transpose(1, 2).reshape(B, Tq, C)


def max_err(got, want64):
    return (got.detach().cpu().double() - want64.detach().double()).abs().max().item()


# ---- shared cases -----------------------------------------------------------------------------------------------------------
def cfg(kind, boc, layers, latent, groups, K=0):
    return SimpleNamespace(kind=kind, block_out_channels=tuple(boc), layers_per_block=layers, latent_channels=latent,
                           norm_num_groups=groups, in_channels=3, out_channels=3, scaling_factor=0.18215,
                           num_vq_embeddings=K, vq_embed_dim=latent)


TINY_KL = cfg("kl", (32, 64), 1, 4, 8)            # mid-block head of 64: gad_attention_fwd
WIDE_KL = cfg("kl", (64, 512), 1, 4, 32)          # mid-block head of 512: gad_attention_fwd_d512 or the three launches, by grid
TINY_VQ = cfg("vq", (32, 64), 1, 3, 8, K=64)
SD_VAE = cfg("kl", (128, 256, 512, 512), 2, 4, 32)
CELEBA_VQ = cfg("vq", (128, 256, 512), 2, 3, 32, K=8192)

ATTN_SHAPES = [(1, 1, 1), (2, 64, 64), (1, 33, 95), (2, 130, 70), (1, 300, 700)]      # B, Tq, Tk


def attention_inputs(B, Tq, Tk, d):
    """as tests/test_gpu_attention.py: q and k scaled by 0.7"""
    return rnd(B, Tq, d, seed=1, scale=0.7), rnd(B, Tk, d, seed=2, scale=0.7), rnd(B, Tk, d, seed=3)


def late_key_inputs(d):
    """T = 256; key 200 dominates query 17: the running maximum jumps at a late tile"""
    q, k, v = rnd(1, 256, d, seed=1, scale=0.3), rnd(1, 256, d, seed=2, scale=0.3), rnd(1, 256, d, seed=3)
    k[0, 200] = q[0, 17] * 60.0
    return q, k, v


def latent_input(c, B=1, h=5, w=7, seed=11):
    return rnd(B, c.latent_channels, h, w, seed=seed)


def image_input(c, B=1, h=10, w=14, seed=12):
    return rnd(B, c.in_channels, h, w, seed=seed, scale=0.5)
