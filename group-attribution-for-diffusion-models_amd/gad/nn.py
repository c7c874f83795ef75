"""diffusers-0.24-compatible model classes whose forward/backward run on the HIP
kernels (boundary (i) of SURVEY §8b: same class names, constructor keys, attribute and
state_dict names as the objects the reference builds at
unconditional_generation/main.py:234,332 and src/diffusion_utils.py:153).

Internals are MI355X-first: activations NHWC, conv weights stored [Cout,KH,KW,Cin],
all parameters (optionally) packed into one flat HBM buffer so that gradient clipping,
Adam and the EMA run as a single fused pass (``flatten_parameters``).
"""
from __future__ import annotations

import math
from types import SimpleNamespace

import torch
import torch.nn as nn

from . import ops


class FrozenConfig(dict):
    """dict with attribute access (mimics diffusers' FrozenDict ``model.config``)."""

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e


# ----------------------------------------------------------------------------------
# parameter holders (names match torch/diffusers so state_dicts interchange)
# ----------------------------------------------------------------------------------
class Conv2d(nn.Module):
    def __init__(self, cin, cout, k, stride=1, pad=(1, 1, 1, 1), upsample=False):
        super().__init__()
        ref = nn.Conv2d(cin, cout, k)          # torch default init == diffusers default init
        self.weight = nn.Parameter(ref.weight.detach().contiguous(memory_format=torch.channels_last))
        self.bias = nn.Parameter(ref.bias.detach().clone())
        self.stride, self.pad, self.upsample = stride, tuple(pad), upsample

    def forward(self, x, rowadd=None, residual=None, x2=None):
        if x2 is not None:       # channel concat read in place (inference only: the raw launch has no autograd node)
            return ops.conv2d_fwd_raw(x, self.weight, self.bias, self.stride, self.pad, self.upsample, rowadd, residual, x2=x2)
        return ops.conv2d(x, self.weight, self.bias, rowadd, residual, self.stride, self.pad, self.upsample)


class Linear(nn.Module):
    def __init__(self, cin, cout, bias=True):
        super().__init__()
        ref = nn.Linear(cin, cout, bias=bias)
        self.weight = nn.Parameter(ref.weight.detach().clone())
        self.bias = nn.Parameter(ref.bias.detach().clone()) if bias else None
        self.lora_layer = None

    def set_lora_layer(self, lora_layer):
        self.lora_layer = lora_layer

    def forward(self, x, residual=None, scale: float = 1.0):
        if self.lora_layer is None:
            return ops.linear(x, self.weight, self.bias, residual)
        # y = xW^T + b + scale * up(down(x))  (LoRACompatibleLinear)
        ll = self.lora_layer
        if x.dtype == torch.bfloat16 or ops.lora_fusable(self.weight.shape[1], self.weight.shape[0], ll.rank):      # (the half path pads ragged ranks)
            s = scale * (ll.network_alpha / ll.rank if ll.network_alpha is not None else 1.0)
            return ops.lora_linear(x, self.weight, self.bias, ll.down.weight, ll.up.weight, s, residual)   # one K-concatenated launch
        # ragged ranks that are not multiples of 4: the side path accumulates into the base GEMM's output (two launches)
        base = ops.linear(x, self.weight, self.bias, residual)
        return ll(x, residual=base, scale=scale)


class LoRALinearLayer(nn.Module):
    """diffusers.models.lora.LoRALinearLayer: down ~ N(0, 1/rank), up = 0;
    ranks may differ per projection (text_to_image/prune_lora.py:173-180)."""

    def __init__(self, in_features, out_features, rank=4, network_alpha=None):
        super().__init__()
        self.down = Linear(in_features, rank, bias=False)
        self.up = Linear(rank, out_features, bias=False)
        nn.init.normal_(self.down.weight, std=1 / rank)
        nn.init.zeros_(self.up.weight)
        self.network_alpha, self.rank = network_alpha, rank
        self.in_features, self.out_features = in_features, out_features

    def forward(self, x, residual=None, scale: float = 1.0):
        s = scale * (self.network_alpha / self.rank if self.network_alpha is not None else 1.0)
        mid = self.down(x)
        if s != 1.0:
            mid = mid * s
        return self.up(mid, residual=residual)


class GroupNorm(nn.Module):
    def __init__(self, groups, channels, eps):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(channels))
        self.bias = nn.Parameter(torch.zeros(channels))
        self.num_groups, self.eps = groups, eps

    def forward(self, x, silu=False, x2=None):
        if x2 is not None:
            return ops.group_norm_cat_raw(x, x2, self.weight, self.bias, self.num_groups, self.eps, silu)
        return ops.group_norm(x, self.weight, self.bias, self.num_groups, self.eps, silu)

    def with_bypass(self, x, silu=False):
        """(norm(x), alias of x for the block's residual branch): the backward sums both gradients in the norm's own
        kernel instead of an elementwise launch (ops.GroupNormBypassFn)."""
        return ops.group_norm_bypass(x, self.weight, self.bias, self.num_groups, self.eps, silu)


# ----------------------------------------------------------------------------------
# blocks
# ----------------------------------------------------------------------------------
class ResnetBlock2D(nn.Module):
    def __init__(self, cin, cout, temb_c, groups, eps):
        super().__init__()
        self.norm1 = GroupNorm(groups, cin, eps)
        self.conv1 = Conv2d(cin, cout, 3)
        self.time_emb_proj = Linear(temb_c, cout)
        self.norm2 = GroupNorm(groups, cout, eps)
        self.conv2 = Conv2d(cout, cout, 3)
        self.conv_shortcut = Conv2d(cin, cout, 1, pad=(0, 0, 0, 0)) if cin != cout else None

    def forward(self, x, temb_act, x2=None):
        """x2: the block input is cat([x, x2], channels) (up blocks); norm1 and conv_shortcut read both in place."""
        if not torch.is_grad_enabled() and x.dtype != torch.bfloat16:
            # sampling: each norm -> silu -> conv half is one fused op - where the convolution takes the Winograd F(4x4) route the
            # norm writes the route's transformed input directly (ops.gn_silu_conv3x3_raw), else the two ordinary launches run
            n1, n2 = self.norm1, self.norm2
            row = getattr(self, "_temb_row", None)                  # this block's columns of the model-wide projection (UNet2DModel._temb_rows)
            h = ops.gn_silu_conv3x3_raw(x, x2, n1.weight, n1.bias, n1.num_groups, n1.eps, self.conv1.weight, self.conv1.bias,
                                        rowadd=row if row is not None else self.time_emb_proj(temb_act))
            sc = self.conv_shortcut(x, x2=x2) if self.conv_shortcut is not None else x
            return ops.gn_silu_conv3x3_raw(h, None, n2.weight, n2.bias, n2.num_groups, n2.eps, self.conv2.weight, self.conv2.bias,
                                           residual=sc)
        # training: each norm -> silu -> conv half is one autograd node (ops.GnSiluConv3x3Fn) over the two ordinary launches: the
        # normalised activation is saved only for a trainable weight, whose gradient reads the transformed input an F(4x4) forward
        # launch kept; conv + bias + temb add / skip add are the convolution's epilogue
        n1, n2 = self.norm1, self.norm2
        if x2 is None:
            h, x = ops.gn_silu_conv3x3(x, n1.weight, n1.bias, n1.num_groups, n1.eps, self.conv1.weight, self.conv1.bias,
                                       rowadd=self.time_emb_proj(temb_act), bypass=True)     # x: this node's alias, for the shortcut below
        else:
            h = self.conv1(self.norm1(x, silu=True, x2=x2), rowadd=self.time_emb_proj(temb_act))
        sc = self.conv_shortcut(x, x2=x2) if self.conv_shortcut is not None else x
        return ops.gn_silu_conv3x3(h, n2.weight, n2.bias, n2.num_groups, n2.eps, self.conv2.weight, self.conv2.bias, residual=sc)

    def cat_in_place_ok(self, x, x2):
        """Inference only, and only when both consumers of the concatenation can gather from two sources."""
        return (not torch.is_grad_enabled() and self.conv_shortcut is not None and x.dtype != torch.bfloat16
                and ops.two_source_ok(x.shape[-1], x2.shape[-1])
                and ops.group_norm_two_source_ok(x, x2, self.norm1.num_groups))


class Attention(nn.Module):
    """Self-attention block with the semantics of AttnProcessor2_0
    (reference src/diffusers/models/attention_processor.py:1265-1341)."""

    def __init__(self, channels, heads, dim_head, eps, groups):
        super().__init__()
        inner = heads * dim_head
        self.heads, self.dim_head = heads, dim_head
        # head dims that are not a multiple of 4 (head-grouped-pruned CelebA: 23) run with zero-padded heads: ops.PadHeadsFn
        self.dpad = dim_head if dim_head % 4 == 0 else (dim_head + 7) // 8 * 8
        self.group_norm = GroupNorm(groups, channels, eps)
        self.to_q = Linear(channels, inner)
        self.to_k = Linear(channels, inner)
        self.to_v = Linear(channels, inner)
        self.to_out = nn.ModuleList([Linear(inner, channels), nn.Dropout(0.0)])

    def _padded(self):
        """(Wq, bq, Wk, bk, Wv, bv, Wo) with the heads zero-padded to self.dpad; differentiable (training) - in no-grad
        mode cached per weight version (sampling: thousands of forwards on fixed EMA weights)."""
        h, d, dp = self.heads, self.dim_head, self.dpad
        ps = (self.to_q.weight, self.to_q.bias, self.to_k.weight, self.to_k.bias, self.to_v.weight, self.to_v.bias)
        if torch.is_grad_enabled() or torch.cuda.is_current_stream_capturing():
            # (inside a hipGraph capture the padding launches belong to the graph: a replay re-pads the CURRENT weights, and
            #  nothing allocated from the capture's pool is cached on the module)
            return tuple(ops.pad_heads(p, h, d, dp, 0) for p in ps) + (ops.pad_heads(self.to_out[0].weight, h, d, dp, 1),)
        key = tuple(ops.weight_key(p) for p in ps + (self.to_out[0].weight,))
        if getattr(self, "_pad_key", None) != key:
            self._pad_w = tuple(ops.pad_heads(p, h, d, dp, 0) for p in ps) + (ops.pad_heads(self.to_out[0].weight, h, d, dp, 1),)
            self._pad_key = key
        return self._pad_w

    def _fused_qkv(self):
        """[3C, C] weight and [3C] bias of the three projections, concatenated once and reused while the parameters are
        unchanged (sampling: thousands of forwards on fixed EMA weights)."""
        ps = (self.to_q.weight, self.to_k.weight, self.to_v.weight, self.to_q.bias, self.to_k.bias, self.to_v.bias)
        key = tuple(ops.weight_key(p) for p in ps)           # incl. the epochs the raw optimizer kernels bump
        if getattr(self, "_qkv_key", None) != key:
            if self.dpad != self.dim_head:
                wq, bq, wk, bk, wv, bv, _ = self._padded()
                ps = (wq, wk, wv, bq, bk, bv)
            self._qkv_w = torch.cat([p.detach() for p in ps[:3]], 0).contiguous()
            self._qkv_b = torch.cat([p.detach() for p in ps[3:]], 0).contiguous()
            self._qkv_key = key
        return self._qkv_w, self._qkv_b

    def forward(self, x, scale: float = 1.0):
        b, hh, ww, c = x.shape
        h, x = self.group_norm.with_bypass(x)                        # :1297-1298 (NHWC: no transposes needed); x: alias for the residual
        res = x.view(b, hh * ww, c)
        h = h.view(b, hh * ww, c)
        lq = getattr(self, "lora_qkv", None)
        if lq is not None:             # peft-style LoRA with dropout on to_q / to_k / to_v (gad/lora.py): one node for the three
            q, k, v = lq(self, h)
            o = ops.attention_core(q, k, v, self.heads)
            return self.to_out[0](o, residual=res, scale=scale).view(b, hh, ww, c)
        lora = any(l.lora_layer is not None for l in (self.to_q, self.to_k, self.to_v, self.to_out[0]))
        padded = self.dpad != self.dim_head and not lora
        sm_scale = self.dim_head ** -0.5 if padded else None         # the softmax scale of the TRUE head dim (:1321-1323)
        if not torch.is_grad_enabled() and not lora and not torch.cuda.is_current_stream_capturing():
            # sampling: one [3C, C] projection instead of three (h is read once), q/k/v consumed in place.  Not inside a
            # hipGraph capture: a replayed graph would keep reading the cached copy after the parameters changed.
            w, bias = self._fused_qkv()
            qkv = ops.linear_fwd_raw(h.view(b * hh * ww, c), w, bias)
            o = ops.attention_core_qkv_raw(qkv, b, hh * ww, w.shape[0] // 3, self.heads, scale=sm_scale)   # inner dim: != c when pruned
            if padded:
                o = ops.linear(o, self._padded()[6], self.to_out[0].bias, res)
            else:
                o = self.to_out[0](o, residual=res, scale=scale)
            return o.view(b, hh, ww, c)
        if padded:
            wq, bq, wk, bk, wv, bv, wo = self._padded()
            q, k, v = ops.linear(h, wq, bq), ops.linear(h, wk, bk), ops.linear(h, wv, bv)
            o = ops.attention_core(q, k, v, self.heads, scale=sm_scale)
            return ops.linear(o, wo, self.to_out[0].bias, res).view(b, hh, ww, c)
        q, k, v = self.to_q(h, scale=scale), self.to_k(h, scale=scale), self.to_v(h, scale=scale)   # :1301-1309
        o = ops.attention_core(q, k, v, self.heads)                   # :1314-1325
        o = self.to_out[0](o, residual=res, scale=scale)              # :1329 + residual :1336-1337
        return o.view(b, hh, ww, c)


class DownBlock(nn.Module):
    def __init__(self, cin, cout, temb_c, layers, eps, groups, add_down, down_pad, attn=None):
        """attn: None or (heads, dim_head) of the block's attentions"""
        super().__init__()
        resnets = nn.ModuleList([ResnetBlock2D(cin if i == 0 else cout, cout, temb_c, groups, eps)
                                 for i in range(layers)])
        # registration order attentions -> resnets as in diffusers (parameters() order == EMA shadow list order)
        self.attentions = nn.ModuleList([Attention(cout, attn[0], attn[1], eps, groups)
                                         for _ in range(layers)]) if attn is not None else None
        self.resnets = resnets
        if add_down:
            pad = (0, 1, 0, 1) if down_pad == 0 else (down_pad,) * 4   # Downsample2D: F.pad(0,1,0,1) when padding==0
            self.downsamplers = nn.ModuleList([_Sampler(Conv2d(cout, cout, 3, stride=2, pad=pad))])
        else:
            self.downsamplers = None

    def forward(self, h, temb_act):
        outs = ()
        for i, r in enumerate(self.resnets):
            h = r(h, temb_act)
            if self.attentions is not None:
                h = self.attentions[i](h)
            outs += (h,)
        if self.downsamplers is not None:
            h = self.downsamplers[0](h)
            outs += (h,)
        return h, outs


class _Sampler(nn.Module):
    """Down/Upsample2D wrapper so the parameter is named ``...samplers.0.conv.weight``."""

    def __init__(self, conv):
        super().__init__()
        self.conv = conv

    def forward(self, x):
        return self.conv(x)


class UNetMidBlock2D(nn.Module):
    def __init__(self, c, temb_c, eps, groups, attn, add_attention=True):
        super().__init__()
        resnets = nn.ModuleList([ResnetBlock2D(c, c, temb_c, groups, eps), ResnetBlock2D(c, c, temb_c, groups, eps)])
        self.attentions = nn.ModuleList([Attention(c, attn[0], attn[1], eps, groups) if add_attention else None])
        self.resnets = resnets

    def forward(self, h, temb_act):
        h = self.resnets[0](h, temb_act)
        if self.attentions[0] is not None:
            h = self.attentions[0](h)
        return self.resnets[1](h, temb_act)


class UpBlock(nn.Module):
    def __init__(self, cin, prev_c, cout, temb_c, layers, eps, groups, add_up, attn=None):
        super().__init__()
        res = []
        for i in range(layers):
            skip_c = cin if i == layers - 1 else cout
            r_in = prev_c if i == 0 else cout
            res.append(ResnetBlock2D(r_in + skip_c, cout, temb_c, groups, eps))
        self.attentions = nn.ModuleList([Attention(cout, attn[0], attn[1], eps, groups)
                                         for _ in range(layers)]) if attn is not None else None
        self.resnets = nn.ModuleList(res)
        self.upsamplers = nn.ModuleList([_Sampler(Conv2d(cout, cout, 3, upsample=True))]) if add_up else None

    def forward(self, h, skips, temb_act):
        for i, r in enumerate(self.resnets):
            s, skips = skips[-1], skips[:-1]
            # torch.cat([h, skip], 1) of UpBlock2D; when sampling, its two consumers read h and skip in place
            h = r(h, temb_act, x2=s) if r.cat_in_place_ok(h, s) else r(ops.concat(h, s), temb_act)
            if self.attentions is not None:
                h = self.attentions[i](h)
        if self.upsamplers is not None:
            h = self.upsamplers[0](h)                                 # nearest-2x fused into the conv's gather
        return h


class TimestepEmbedding(nn.Module):
    def __init__(self, cin, dim):
        super().__init__()
        self.linear_1 = Linear(cin, dim)
        self.linear_2 = Linear(dim, dim)

    def forward(self, x):
        return self.linear_2(ops.silu(self.linear_1(x)))


class UNet2DModel(nn.Module):
    """diffusers.UNet2DModel on HIP kernels.  Accepts every key of the reference config
    dicts (src/ddpm_config.py:235-269, :423-451); unknown keys are kept in ``.config``."""

    def __init__(self, sample_size=None, in_channels=3, out_channels=3, center_input_sample=False,
                 time_embedding_type="positional", freq_shift=0, flip_sin_to_cos=True,
                 down_block_types=("DownBlock2D", "AttnDownBlock2D", "AttnDownBlock2D", "AttnDownBlock2D"),
                 up_block_types=("AttnUpBlock2D", "AttnUpBlock2D", "AttnUpBlock2D", "UpBlock2D"),
                 block_out_channels=(224, 448, 672, 896), layers_per_block=2, mid_block_scale_factor=1,
                 downsample_padding=1, downsample_type="conv", upsample_type="conv", dropout=0.0,
                 act_fn="silu", attention_head_dim=8, norm_num_groups=32, attn_norm_num_groups=None,
                 norm_eps=1e-5, resnet_time_scale_shift="default", add_attention=True,
                 class_embed_type=None, num_class_embeds=None, num_train_timesteps=None, attention_layout=None,
                 **unused):
        """attention_layout (not a diffusers key): [[heads, dim_head], ...] per resolution level for a head-grouped
        pruned model (unconditional_generation/prune.py): the reference keeps the pickled module whose to_q/k/v lost the
        same in-head channels in every head (prune.py:337-342), so heads stay and the head dim shrinks - a shape
        `channels // attention_head_dim` cannot express."""
        super().__init__()
        cfg = dict(locals())
        for k in ("self", "unused", "__class__"):
            cfg.pop(k, None)
        cfg.update(unused)
        self.config = FrozenConfig(cfg)
        if not (time_embedding_type == "positional" and act_fn == "silu" and class_embed_type is None
                and downsample_type == "conv" and upsample_type == "conv" and resnet_time_scale_shift == "default"
                and dropout == 0.0 and mid_block_scale_factor == 1 and attn_norm_num_groups is None):
            raise NotImplementedError("UNet2DModel: configuration outside the reference's registry")
        boc = list(block_out_channels)
        temb_c = boc[0] * 4

        def attn_of(level, c):          # (heads, dim_head) of the attentions at resolution level `level`
            if attention_layout is not None:
                return int(attention_layout[level][0]), int(attention_layout[level][1])
            hd = attention_head_dim if attention_head_dim is not None else c
            return c // hd, hd
        self.conv_in = Conv2d(in_channels, boc[0], 3)
        self.time_proj = SimpleNamespace(num_channels=boc[0], flip_sin_to_cos=flip_sin_to_cos,
                                         downscale_freq_shift=freq_shift)
        self.time_embedding = TimestepEmbedding(boc[0], temb_c)
        self.down_blocks = nn.ModuleList()
        out_c = boc[0]
        for i, typ in enumerate(down_block_types):
            in_c, out_c = out_c, boc[i]
            at = None
            if typ == "AttnDownBlock2D":
                at = attn_of(i, out_c)
            elif typ != "DownBlock2D":
                raise NotImplementedError(typ)
            self.down_blocks.append(DownBlock(in_c, out_c, temb_c, layers_per_block, norm_eps, norm_num_groups,
                                              i != len(boc) - 1, downsample_padding, at))
        self.mid_block = UNetMidBlock2D(boc[-1], temb_c, norm_eps, norm_num_groups, attn_of(len(boc) - 1, boc[-1]),
                                        add_attention)
        self.up_blocks = nn.ModuleList()
        rev = list(reversed(boc))
        out_c = rev[0]
        for i, typ in enumerate(up_block_types):
            prev_c, out_c = out_c, rev[i]
            in_c = rev[min(i + 1, len(boc) - 1)]
            at = None
            if typ == "AttnUpBlock2D":
                at = attn_of(len(boc) - 1 - i, out_c)
            elif typ != "UpBlock2D":
                raise NotImplementedError(typ)
            self.up_blocks.append(UpBlock(in_c, prev_c, out_c, temb_c, layers_per_block + 1, norm_eps,
                                          norm_num_groups, i != len(boc) - 1, at))
        g = norm_num_groups if norm_num_groups is not None else min(boc[0] // 4, 32)
        self.conv_norm_out = GroupNorm(g, boc[0], norm_eps)
        self.conv_out = Conv2d(boc[0], out_channels, 3)
        self._flat = None

    # ---- diffusers ModelMixin conveniences used by the reference ----
    @property
    def dtype(self):
        return self.conv_in.bias.dtype

    @property
    def device(self):
        return self.conv_in.bias.device

    def forward_nhwc(self, x, timestep):
        """x: NHWC fp32 device tensor; returns NHWC eps prediction."""
        t = timestep
        if not torch.is_tensor(t):
            t = torch.tensor([t], dtype=torch.long, device=x.device)
        elif t.ndim == 0:
            t = t[None]
        t = t.to(x.device)
        if t.shape[0] != x.shape[0]:
            t = t.expand(x.shape[0])
        tp = self.time_proj
        emb = ops.timestep_embedding(t, tp.num_channels, tp.flip_sin_to_cos, tp.downscale_freq_shift)
        temb_act = ops.silu(self.time_embedding(emb))       # SiLU(temb) is shared by every ResnetBlock2D
        resnets = self._temb_rows(temb_act)
        try:
            return self._blocks_nhwc(x, temb_act)
        finally:
            for r in resnets:
                r._temb_row = None

    def _temb_rows(self, temb_act):
        """Sampling (no grad): the time-embedding projections of ALL ResnetBlock2Ds (`time_emb_proj`: 22 Linear [512 -> Cout] on
        the same input, each a 14 us launch at 6 % of the MFMA peak) as ONE GEMM on the concatenated weights; each block adds its
        column block in its first convolution's epilogue.  The concatenation is rebuilt when a weight changes."""
        if torch.is_grad_enabled() or torch.cuda.is_current_stream_capturing():
            return ()
        rs = [m for m in self.modules() if isinstance(m, ResnetBlock2D)]
        if any(r.time_emb_proj.lora_layer is not None for r in rs):
            return ()
        key = tuple(ops.weight_key(p) for r in rs for p in (r.time_emb_proj.weight, r.time_emb_proj.bias))
        if getattr(self, "_temb_key", None) != key:
            self._temb_w = torch.cat([r.time_emb_proj.weight.detach() for r in rs], 0).contiguous()
            self._temb_b = torch.cat([r.time_emb_proj.bias.detach() for r in rs], 0).contiguous()
            self._temb_key = key
        allp = ops.linear_fwd_raw(temb_act, self._temb_w, self._temb_b)
        off = 0
        for r in rs:
            n = r.time_emb_proj.weight.shape[0]
            r._temb_row = allp[:, off:off + n]
            off += n
        return rs

    def _blocks_nhwc(self, x, temb_act):
        h = self.conv_in(x)
        skips = (h,)
        for blk in self.down_blocks:
            h, outs = blk(h, temb_act)
            skips += outs
        h = self.mid_block(h, temb_act)
        for blk in self.up_blocks:
            n = len(blk.resnets)
            res, skips = skips[-n:], skips[:-n]
            h = blk(h, res, temb_act)
        h = self.conv_norm_out(h, silu=True)
        return self.conv_out(h)

    def forward(self, sample, timestep):
        """sample: NCHW (diffusers convention) -> object with ``.sample`` NCHW."""
        if not sample.is_cuda:
            raise ops._capi.GadError("gad.UNet2DModel runs on the MI355X only (no CPU path); got a CPU tensor")
        x = sample.to(torch.float32).contiguous()
        if self.config.center_input_sample:
            x = 2 * x - 1.0
        y = self.forward_nhwc(ops.nchw_to_nhwc_raw(x), timestep)
        return SimpleNamespace(sample=ops.to_nchw(y))

    # ---- flat parameter storage ----
    def flatten_parameters(self):
        """Re-home every parameter (and its .grad) in one contiguous fp32 buffer; conv weights keep
        their [Cout,KH,KW,Cin] storage.  Returns (flat_params, flat_grads)."""
        from .training import flatten_params
        flat, gflat = flatten_params(self.parameters())
        self._flat = (flat, gflat)
        return flat, gflat

    @property
    def flat(self):
        if self._flat is None:
            raise ops._capi.GadError("call model.flatten_parameters() first")
        return self._flat
