"""The pre-LN transformer encoder that the image towers (gad/vit.py) and the text towers (gad/text.py) both are, on the HIP
operators: the block's launches, its weights under the three state-dict layouts, the rule seeded weights follow, the shared
configuration check and the activation budget behind `max_batch`.  A tower adds its own ends (patches or token ids in,
pooling and projection out) and names the one launch that differs, the attention.

    per block:  x += out_proj(attention(ln_1(x) W_qkv + b))          gad_layernorm_fwd, gad_gemm, <attention>, gad_gemm
                x += c_proj(act(c_fc(ln_2(x))))                      gad_layernorm_fwd, gad_gemm, gad_gelu, gad_gemm

The qkv projection is one [3W, W] contraction that the attention kernel reads in place; both residual adds ride in the
contraction's epilogue.  Eval only, fp32 throughout."""
from __future__ import annotations

import math

import torch

from . import ops
from ._capi import GELU_ERF, GELU_QUICK

# layout -> a block's names in a state dict; `qkv`: the (weight, bias) keys whose rows, stacked, are the [3W, W] projection
LAYOUTS = {
    "openai": dict(block="transformer.resblocks.{}.", ln1="ln_1", ln2="ln_2", qkv=(("attn.in_proj_weight", "attn.in_proj_bias"),),
                   out="attn.out_proj", fc="mlp.c_fc", proj="mlp.c_proj"),
    "hf_fused": dict(block="encoder.layers.{}.", ln1="layer_norm1", ln2="layer_norm2",                     # BLIP
                     qkv=(("self_attn.qkv.weight", "self_attn.qkv.bias"),), out="self_attn.projection", fc="mlp.fc1", proj="mlp.fc2"),
    "hf_split": dict(block="encoder.layers.{}.", ln1="layer_norm1", ln2="layer_norm2",                     # CLIPTextModel
                     qkv=tuple((f"self_attn.{n}_proj.weight", f"self_attn.{n}_proj.bias") for n in "qkv"),
                     out="self_attn.out_proj", fc="mlp.fc1", proj="mlp.fc2"),
}


def block_shapes(layout, i, W, M):
    """{key: shape} of block `i` in the layout's own names and order (seeded weights are drawn in this order)"""
    n = LAYOUTS[layout]
    p, out, rows = n["block"].format(i), {}, 3 * W // len(n["qkv"])
    for k in (n["ln1"], n["ln2"]):
        out[p + k + ".weight"], out[p + k + ".bias"] = (W,), (W,)
    for kw, kb in n["qkv"]:
        out[p + kw], out[p + kb] = (rows, W), (rows,)
    for k, shape in ((n["out"], (W, W)), (n["fc"], (M, W)), (n["proj"], (W, M))):
        out[p + k + ".weight"], out[p + k + ".bias"] = shape, shape[:1]
    return out


def load_block(get, layout, i):
    """Block `i` as the launches read it: dict(ln1, ln2, qkv, out, fc, proj) of (weight, bias); `get(key)` returns the fp32
    contiguous tensor under a key of `block_shapes`.  Separate q / k / v weights are stacked into the one projection."""
    n = LAYOUTS[layout]
    p = n["block"].format(i)

    def pair(k):
        return get(p + k + ".weight"), get(p + k + ".bias")
    qkv = [(get(p + kw), get(p + kb)) for kw, kb in n["qkv"]]
    qkv = qkv[0] if len(qkv) == 1 else (torch.cat([t[0] for t in qkv], 0).contiguous(), torch.cat([t[1] for t in qkv], 0).contiguous())
    return dict(ln1=pair(n["ln1"]), ln2=pair(n["ln2"]), qkv=qkv, out=pair(n["out"]), fc=pair(n["fc"]), proj=pair(n["proj"]))


def seeded(shapes, seed):
    """A state dict of `shapes` ({key: shape}) from one generator, in the dict's order: weights N(0, 1 / fan_in) (the residual
    stream keeps its scale through the blocks), LayerNorm gains 1 + N(0, 0.1^2), every bias and embedding N(0, 0.1^2) but the
    positional one (0.02^2).  Seeded towers stand in for pretrained ones under tags that database rows carry: the branches and
    their order stay as they are."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for key, shape in shapes.items():
        r = torch.randn(shape, generator=g)
        if key in ("proj", "text_projection"):
            sd[key] = r / math.sqrt(shape[0])
        elif any(n in key for n in ("ln_", "layer_norm", "layernorm")):
            sd[key] = 1 + 0.1 * r if key.endswith("weight") else 0.1 * r
        elif "position" in key:
            sd[key] = 0.02 * r
        elif "token_embedding" in key:
            sd[key] = 0.1 * r
        elif key.endswith("weight") and len(shape) > 1:
            sd[key] = r / math.sqrt(math.prod(shape[1:]))
        else:
            sd[key] = 0.1 * r
    return sd


def check_config(owner, cfg, grid=None):
    """Refuse an activation or a width the block's kernels do not take, under the tower's name.  `grid`: a vision tower's
    (image_size, patch), checked and named in the same refusal."""
    if cfg.act not in ("gelu", "quick_gelu"):
        raise ValueError(f"{owner}: act {cfg.act!r}: use 'gelu' or 'quick_gelu'")
    if (grid and grid[0] % grid[1]) or cfg.width % cfg.heads or cfg.width % 4:
        lead = f"image_size {grid[0]} must be a multiple of patch {grid[1]}, width {cfg.width}" if grid else f"width {cfg.width} must be a multiple"
        raise ValueError(f"{owner}: {lead} of heads {cfg.heads} and of 4")


def max_batch(tokens, width, mlp, extra=0):
    """Items per pass that keep the activations under 0.5 GB, rounded down to a power of two and capped at 256.  Alive at once
    per item, in floats: `tokens` rows of the two residual buffers, the normed copy and the attention output (4 W), the qkv
    projection (3 W) and the MLP hidden (mlp), plus `extra` (a vision tower's image)."""
    per_item = 4 * (tokens * (7 * width + mlp) + extra)
    return max(1, min(256, 1 << int(math.log2(max(1, (1 << 29) // per_item)))))


# ---- launches ----
def ln(x, gb, eps):
    return ops.layernorm_fwd_raw(x, *gb, eps)[0]


def block(x, Bn, T, width, heads, act, eps, blk, attention):
    """One block on the residual stream x [Bn T, width]; `attention`: `ops.attention_core_qkv_raw` or
    `ops.attention_causal_qkv_raw`"""
    qkv = ops.linear_fwd_raw(ln(x, blk["ln1"], eps), *blk["qkv"], force_f32=True)
    o = attention(qkv, Bn, T, width, heads)
    x = ops.linear_fwd_raw(o.view(Bn * T, width), *blk["out"], residual=x, force_f32=True)
    h = ops.linear_fwd_raw(ln(x, blk["ln2"], eps), *blk["fc"], force_f32=True)
    h = ops.gelu_raw(h, GELU_ERF if act == "gelu" else GELU_QUICK)
    return ops.linear_fwd_raw(h, *blk["proj"], residual=x, force_f32=True)
