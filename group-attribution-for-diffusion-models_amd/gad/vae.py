"""The autoencoders between latents and pixels - diffusers' `AutoencoderKL` (Stable Diffusion's VAE) and `VQModel`
(`CompVis/ldm-celebahq-256`'s VQ-VAE, reference unconditional_generation/unlearn.py:756) - on the HIP operators.

Eval only, in the style of gad/vgg.py and gad/vit.py: weights sit in a dict, launches go through the `*_raw` wrappers of
gad/ops.py, activations are fp32 NHWC internally, `decode` / `encode` take and return NCHW as diffusers does.

Every convolution is one `gad_gemm` launch on the direct fp32 route (no Winograd weight is passed: F(4x4) is 10-20x less
accurate per layer, and the decoder is a negligible share of a coalition); the upsampler's nearest-2x is folded into its
convolution's gather, the downsampler's pad (0,1,0,1) is the convolution's own asymmetric padding, a ResnetBlock's and the
attention's residual add is the epilogue of its last launch.  GroupNorm(+SiLU) is `gad_groupnorm_silu_fwd` (eps 1e-6).  The
mid-block attention is ONE head over all channels: q | k | v come from one fused [3C, C] projection and are read in place;
d <= 256 runs `gad_attention_fwd`; d = 512 - both full-size models - runs `gad_attention_fwd_d512` where its grid fills the
chip and the three-launch route (batched q k^T, row softmax, p v: `ops.attention_core_qkv_raw`) below that (`d512_route`);
any other width is refused.
VQModel's codebook lookup is `gad_vq_lookup`.  What stays in torch is elementwise work on the few-channel latents
(`DiagonalGaussian`: clamp, exp, the reparameterised sample).

Architecture (diffusers 0.24; there is no time embedding, every activation is SiLU):
  ResnetBlock2D(ci, co)   h = conv1(silu(norm1(x))); h = conv2(silu(norm2(h))); x = conv_shortcut(x) (1x1) iff ci != co; x + h
  mid block               resnets.0, attentions.0, resnets.1 at C = boc[-1]; attention: group_norm -> to_q / to_k / to_v ->
                          softmax(q k^T / sqrt(C)) v -> to_out.0 -> + block input.  Older files name the same Linears query,
                          key, value, proj_attn: both grammars load
  decoder                 conv_in(latent -> boc[-1]), mid block, up_blocks.i for o in reversed(boc): layers_per_block + 1
                          resnets (the first prev -> o) and, on all but the last, upsamplers.0.conv; conv_norm_out, SiLU, conv_out
  encoder                 conv_in(in -> boc[0]), down_blocks.i for o in boc: layers_per_block resnets and, on all but the last,
                          downsamplers.0.conv (stride 2); mid block; conv_norm_out, SiLU, conv_out(-> 2 latent if KL else latent)
  AutoencoderKL           encoder, quant_conv (1x1, 2L -> 2L), post_quant_conv (1x1, L -> L), decoder
  VQModel                 encoder, quant_conv (1x1, L -> E), quantize.embedding.weight [K, E], post_quant_conv (1x1, E -> L), decoder

A missing, unexpected or misshapen key is an error that names the key."""
from __future__ import annotations

import math
from types import SimpleNamespace

import torch

from . import _capi, ops
from .extractor import Extractor, check_state_dict, file_tag, load_checkpoint
from .schedulers import randn_tensor

EPS = 1e-6
# gad_attention_fwd_d512 takes a CU per workgroup of 64 queries (132 KB of LDS), so below one workgroup per CU its time is
# that of a full chip: 0.33 ms at T = 1024 and 1.26 ms at T = 4096 whatever the batch, against 0.08 / 0.20 ms (B = 2 / 8) and
# 0.42 ms (B = 1) of the three launches.  At 256 workgroups the two tie (1.31 / 1.29 ms, 32 MiB against the score tensor's
# 288), beyond that the fused kernel leads (profiles/vae_ab.txt).
D512_FUSED_MIN_WORKGROUPS = 256


def d512_route(batch, tokens):
    """which way the mid-block attention of a 512-wide model goes: "fused" (gad_attention_fwd_d512) or "three-launch" """
    return "fused" if batch * ((tokens + 63) // 64) >= D512_FUSED_MIN_WORKGROUPS else "three-launch"
OLD_ATTENTION_NAMES = {"query": "to_q", "key": "to_k", "value": "to_v", "proj_attn": "to_out.0"}


def make_config(kind, block_out_channels, layers_per_block, latent_channels, norm_num_groups=32, in_channels=3, out_channels=3,
                scaling_factor=0.18215, num_vq_embeddings=0, vq_embed_dim=None):
    """kind: "kl" | "vq".  A plain namespace: `scaling_factor` is writable (the reference sets it to 1 for CelebA)."""
    if kind not in ("kl", "vq"):
        raise ValueError(f"autoencoder kind {kind!r} is not 'kl' or 'vq'")
    return SimpleNamespace(kind=kind, block_out_channels=tuple(block_out_channels), layers_per_block=int(layers_per_block),
                           latent_channels=int(latent_channels), norm_num_groups=int(norm_num_groups), in_channels=int(in_channels),
                           out_channels=int(out_channels), scaling_factor=float(scaling_factor),
                           num_vq_embeddings=int(num_vq_embeddings),
                           vq_embed_dim=int(vq_embed_dim if vq_embed_dim is not None else latent_channels))


def sd_vae_config():
    return make_config("kl", (128, 256, 512, 512), 2, 4, 32, scaling_factor=0.18215)


def celeba_vq_config():
    from src.ddpm_config import DDPMConfig
    c = DDPMConfig.celeba_config["vqvae_config"]
    return make_config("vq", c["block_out_channels"], c["layers_per_block"], c["latent_channels"], c.get("norm_num_groups", 32),
                       c["in_channels"], c["out_channels"], c.get("scaling_factor", 0.18215), c["num_vq_embeddings"],
                       c.get("vq_embed_dim"))


PRESETS = {"SD_VAE": sd_vae_config, "CELEBA_VQ": celeba_vq_config}


# ---- key grammar -------------------------------------------------------------------------------------------------------
def _resnet_shapes(out, p, ci, co):
    out[p + "norm1.weight"], out[p + "norm1.bias"] = (ci,), (ci,)
    out[p + "conv1.weight"], out[p + "conv1.bias"] = (co, ci, 3, 3), (co,)
    out[p + "norm2.weight"], out[p + "norm2.bias"] = (co,), (co,)
    out[p + "conv2.weight"], out[p + "conv2.bias"] = (co, co, 3, 3), (co,)
    if ci != co:
        out[p + "conv_shortcut.weight"], out[p + "conv_shortcut.bias"] = (co, ci, 1, 1), (co,)


def _mid_shapes(out, p, c):
    _resnet_shapes(out, p + "resnets.0.", c, c)
    a = p + "attentions.0."
    out[a + "group_norm.weight"], out[a + "group_norm.bias"] = (c,), (c,)
    for n in ("to_q", "to_k", "to_v", "to_out.0"):
        out[a + n + ".weight"], out[a + n + ".bias"] = (c, c), (c,)
    _resnet_shapes(out, p + "resnets.1.", c, c)


def decoder_shapes(cfg, prefix="decoder."):
    boc, out = cfg.block_out_channels, {}
    out[prefix + "conv_in.weight"], out[prefix + "conv_in.bias"] = (boc[-1], cfg.latent_channels, 3, 3), (boc[-1],)
    _mid_shapes(out, prefix + "mid_block.", boc[-1])
    prev = boc[-1]
    for i, o in enumerate(reversed(boc)):
        for j in range(cfg.layers_per_block + 1):
            _resnet_shapes(out, f"{prefix}up_blocks.{i}.resnets.{j}.", prev if j == 0 else o, o)
        if i != len(boc) - 1:
            out[f"{prefix}up_blocks.{i}.upsamplers.0.conv.weight"], out[f"{prefix}up_blocks.{i}.upsamplers.0.conv.bias"] = (o, o, 3, 3), (o,)
        prev = o
    out[prefix + "conv_norm_out.weight"], out[prefix + "conv_norm_out.bias"] = (boc[0],), (boc[0],)
    out[prefix + "conv_out.weight"], out[prefix + "conv_out.bias"] = (cfg.out_channels, boc[0], 3, 3), (cfg.out_channels,)
    return out


def encoder_shapes(cfg, prefix="encoder."):
    boc, out = cfg.block_out_channels, {}
    out[prefix + "conv_in.weight"], out[prefix + "conv_in.bias"] = (boc[0], cfg.in_channels, 3, 3), (boc[0],)
    prev = boc[0]
    for i, o in enumerate(boc):
        for j in range(cfg.layers_per_block):
            _resnet_shapes(out, f"{prefix}down_blocks.{i}.resnets.{j}.", prev if j == 0 else o, o)
        if i != len(boc) - 1:
            out[f"{prefix}down_blocks.{i}.downsamplers.0.conv.weight"], out[f"{prefix}down_blocks.{i}.downsamplers.0.conv.bias"] = (o, o, 3, 3), (o,)
        prev = o
    _mid_shapes(out, prefix + "mid_block.", boc[-1])
    zc = 2 * cfg.latent_channels if cfg.kind == "kl" else cfg.latent_channels
    out[prefix + "conv_norm_out.weight"], out[prefix + "conv_norm_out.bias"] = (boc[-1],), (boc[-1],)
    out[prefix + "conv_out.weight"], out[prefix + "conv_out.bias"] = (zc, boc[-1], 3, 3), (zc,)
    return out


def expected_shapes(cfg):
    """{state-dict key: shape} of the whole file (diffusers' names, the newer attention grammar)."""
    out = {**encoder_shapes(cfg), **decoder_shapes(cfg)}
    L = cfg.latent_channels
    if cfg.kind == "kl":
        out["quant_conv.weight"], out["quant_conv.bias"] = (2 * L, 2 * L, 1, 1), (2 * L,)
        out["post_quant_conv.weight"], out["post_quant_conv.bias"] = (L, L, 1, 1), (L,)
    else:
        E = cfg.vq_embed_dim
        out["quant_conv.weight"], out["quant_conv.bias"] = (E, L, 1, 1), (E,)
        out["quantize.embedding.weight"] = (cfg.num_vq_embeddings, E)
        out["post_quant_conv.weight"], out["post_quant_conv.bias"] = (L, E, 1, 1), (L,)
    return out


def normalize_keys(sd):
    """Older files' attention names (query, key, value, proj_attn) -> to_q, to_k, to_v, to_out.0; everything else as it is."""
    out = {}
    for k, v in sd.items():
        parts = k.split(".")
        if "attentions" in parts and len(parts) >= 2 and parts[-2] in OLD_ATTENTION_NAMES:
            k = ".".join(parts[:-2] + [OLD_ATTENTION_NAMES[parts[-2]], parts[-1]])
        out[k] = v
    return out


def seeded_state_dict(cfg, seed):
    """Convolutions and Linears N(0, 1 / fan_in), norm scales 1 + N(0, 0.1^2), biases N(0, 0.1^2), codebook N(0, 1)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for key, shape in expected_shapes(cfg).items():
        r = torch.randn(shape, generator=g)
        if key == "quantize.embedding.weight":
            sd[key] = r
        elif key.endswith("bias"):
            sd[key] = r * 0.1
        elif len(shape) == 1:
            sd[key] = 1.0 + r * 0.1
        else:
            sd[key] = r / math.sqrt(math.prod(shape[1:]))
    return sd


def load_file(path):
    if str(path).endswith(".safetensors"):
        from safetensors.torch import load_file as st_load
        return st_load(str(path))
    return load_checkpoint(path)


class DiagonalGaussian:
    """diffusers' DiagonalGaussianDistribution of `moments` [B, 2L, h, w]: mean | logvar along the channels, logvar clamped
    to [-30, 20]."""

    def __init__(self, moments):
        self.mean, logvar = torch.chunk(moments, 2, dim=1)
        self.logvar = torch.clamp(logvar, -30.0, 20.0)
        self.std = torch.exp(0.5 * self.logvar)
        self.var = torch.exp(self.logvar)

    def mode(self):
        return self.mean

    def sample(self, generator=None):
        """mean + std * randn; a CPU generator draws on the host and the noise is moved (diffusers' randn_tensor)"""
        return self.mean + self.std * randn_tensor(self.mean.shape, generator, self.mean.device, self.mean.dtype)


class _Autoencoder(Extractor):
    """`max_batch` images per pass: a 256 x 256 x 128 activation is 32 MB per image"""
    kind = tag_kind = None

    def __init__(self, config, state_dict=None, tag=None):
        if config.kind != self.kind:
            raise ValueError(f"{self.owner}: the config is of kind {config.kind!r}, expected {self.kind!r}")
        c = config.block_out_channels[-1]
        if not (c <= 256 or ops.attention_d512_ok(c)):
            raise _capi.GadError(f"{self.owner}: the mid block's single attention head of {c} has no kernel (1..256 or 512)")
        self.config = SimpleNamespace(**vars(config))
        self.max_batch, self.device = 8, torch.device("cpu")
        super().__init__(tag or f"{self.tag_kind}-unloaded", state_dict)

    @classmethod
    def seeded(cls, cfg, seed=1234):
        return cls(cfg, seeded_state_dict(cfg, seed), tag=f"{cls.tag_kind}-seeded{seed}")

    @classmethod
    def from_file(cls, path, preset):
        """`preset`: a config (make_config) or the name of one in PRESETS"""
        cfg = PRESETS[preset]() if isinstance(preset, str) else preset
        return cls(cfg, load_file(path), tag=file_tag(cls.tag_kind, path))

    def to(self, device):
        self.device = torch.device(device)
        return super().to(device)

    # ---- weights ----
    def load_state_dict(self, sd):
        sd = normalize_keys(sd)
        want = expected_shapes(self.config)
        check_state_dict(self.owner, sd, want, extra=lambda k: False)
        w = {}
        f = lambda t: t.detach().float().contiguous()      # noqa: E731
        for key in want:
            if not key.endswith(".weight"):
                continue
            name, t = key[:-len(".weight")], sd[key]
            if ".attentions.0.to_" in key or name == "quantize.embedding":
                continue
            b = f(sd[name + ".bias"])
            w[name] = (f(t.permute(0, 2, 3, 1)) if t.ndim == 4 else f(t), b)       # convolutions: [Cout][KH][KW][Cin]
        for side in ("encoder.", "decoder."):
            a = side + "mid_block.attentions.0."
            w[a + "qkv"] = (f(torch.cat([sd[a + n + ".weight"] for n in ("to_q", "to_k", "to_v")], 0)),
                            f(torch.cat([sd[a + n + ".bias"] for n in ("to_q", "to_k", "to_v")], 0)))
            w[a + "to_out.0"] = (f(sd[a + "to_out.0.weight"]), f(sd[a + "to_out.0.bias"]))
        if self.kind == "vq":
            w["quantize.embedding"] = f(sd["quantize.embedding.weight"])
        self.w = w
        return self

    # ---- launches (NHWC) ----
    def _gn(self, name, x, silu):
        return ops.group_norm_raw(x, *self.w[name], self.config.norm_num_groups, EPS, silu)

    def _resnet(self, p, x):
        h = ops.conv_direct_raw(self._gn(p + "norm1", x, True), *self.w[p + "conv1"])
        h = self._gn(p + "norm2", h, True)
        if p + "conv_shortcut" in self.w:
            x = ops.conv_direct_raw(x, *self.w[p + "conv_shortcut"], pad=(0, 0, 0, 0))
        return ops.conv_direct_raw(h, *self.w[p + "conv2"], residual=x)

    def _attention(self, p, x):
        Bn, H, W, Cn = x.shape
        T = H * W
        n = self._gn(p + "group_norm", x, False).view(Bn * T, Cn)
        qkv = ops.linear_fwd_raw(n, *self.w[p + "qkv"], force_f32=True)                 # [B*T, 3C]: q | k | v, read in place
        q, k, v = qkv[:, 0:Cn], qkv[:, Cn:2 * Cn], qkv[:, 2 * Cn:3 * Cn]
        if Cn <= 256:
            o = ops.attention_fwd_raw(q, k, v, Bn, 1, T, T, Cn, 3 * Cn, 3 * Cn, 3 * Cn, need_lse=False)[0]
        elif d512_route(Bn, T) == "fused":
            o = ops.attention_fwd_d512_raw(q, k, v, Bn, 1, T, T, Cn, 3 * Cn, 3 * Cn, 3 * Cn)[0]
        else:
            o = ops.attention_core_qkv_raw(qkv, Bn, T, Cn, 1)
        y = ops.linear_fwd_raw(o.view(Bn * T, Cn), *self.w[p + "to_out.0"], residual=x.view(Bn * T, Cn), force_f32=True)
        return y.view(Bn, H, W, Cn)

    def _mid(self, p, x):
        x = self._resnet(p + "resnets.0.", x)
        x = self._attention(p + "attentions.0.", x)
        return self._resnet(p + "resnets.1.", x)

    def _decoder(self, x):
        cfg, p = self.config, "decoder."
        x = ops.conv_direct_raw(x, *self.w[p + "conv_in"])
        x = self._mid(p + "mid_block.", x)
        n = len(cfg.block_out_channels)
        for i in range(n):
            for j in range(cfg.layers_per_block + 1):
                x = self._resnet(f"{p}up_blocks.{i}.resnets.{j}.", x)
            if i != n - 1:
                x = ops.conv_direct_raw(x, *self.w[f"{p}up_blocks.{i}.upsamplers.0.conv"], upsample=True)
        return ops.conv_direct_raw(self._gn(p + "conv_norm_out", x, True), *self.w[p + "conv_out"])

    def _encoder(self, x):
        cfg, p = self.config, "encoder."
        x = ops.conv_direct_raw(x, *self.w[p + "conv_in"])
        n = len(cfg.block_out_channels)
        for i in range(n):
            for j in range(cfg.layers_per_block):
                x = self._resnet(f"{p}down_blocks.{i}.resnets.{j}.", x)
            if i != n - 1:
                x = ops.conv_direct_raw(x, *self.w[f"{p}down_blocks.{i}.downsamplers.0.conv"], stride=2, pad=(0, 1, 0, 1))
        x = self._mid(p + "mid_block.", x)
        return ops.conv_direct_raw(self._gn(p + "conv_norm_out", x, True), *self.w[p + "conv_out"])

    def _conv1x1(self, name, x):
        return ops.conv_direct_raw(x, *self.w[name], pad=(0, 0, 0, 0))

    def _nhwc(self, x_nchw, channels, what):
        if x_nchw.ndim != 4 or x_nchw.shape[1] != channels:
            raise _capi.GadError(f"{self.owner}: {what} expects [B, {channels}, H, W], got {tuple(x_nchw.shape)}")
        return ops.nchw_to_nhwc_raw(ops._req(x_nchw.to(self.device, torch.float32).contiguous(), what))

    @torch.no_grad()
    def encode_moments(self, x_nchw):
        """quant_conv(encoder(x)) as NCHW"""
        return self._chunked(lambda x: ops.nhwc_to_nchw_raw(
            self._conv1x1("quant_conv", self._encoder(self._nhwc(x, self.config.in_channels, "encode")))), x_nchw)


class AutoencoderKL(_Autoencoder):
    kind, owner, tag_kind = "kl", "AutoencoderKL", "autoencoder_kl"

    @torch.no_grad()
    def decode(self, z, return_dict=True):
        """z [B, L, h, w] (already divided by scaling_factor) -> `.sample` [B, out, 8h, 8w] for four blocks"""
        img = self._chunked(lambda c: ops.nhwc_to_nchw_raw(
            self._decoder(self._conv1x1("post_quant_conv", self._nhwc(c, self.config.latent_channels, "decode")))), z)
        return SimpleNamespace(sample=img) if return_dict else (img,)

    def encode(self, x, return_dict=True):
        dist = DiagonalGaussian(self.encode_moments(x))
        return SimpleNamespace(latent_dist=dist) if return_dict else (dist,)


class VQModel(_Autoencoder):
    kind, owner, tag_kind = "vq", "VQModel", "vqmodel"

    def lookup(self, h_nhwc):
        """NHWC latents [B, h, w, E] -> (nearest-code indices [B, h, w] int32, the straight-through value z + (e - z))"""
        Bn, H, W, E = h_nhwc.shape
        idx, zq = ops.vq_lookup_raw(h_nhwc.view(Bn * H * W, E), self.w["quantize.embedding"])
        return idx.view(Bn, H, W), zq.view(Bn, H, W, E)

    @torch.no_grad()
    def decode(self, h, force_not_quantize=False, return_dict=True):
        """h [B, E, h, w] (not quantised, already divided by scaling_factor) -> `.sample`"""
        def one(c):
            x = self._nhwc(c, self.config.vq_embed_dim, "decode")
            if not force_not_quantize:
                x = self.lookup(x)[1]
            return ops.nhwc_to_nchw_raw(self._decoder(self._conv1x1("post_quant_conv", x)))
        img = self._chunked(one, h)
        return SimpleNamespace(sample=img) if return_dict else (img,)

    def encode(self, x, return_dict=True):
        """`.latents` = quant_conv(encoder(x)), NOT quantised (diffusers quantises in decode)"""
        lat = self.encode_moments(x)
        return SimpleNamespace(latents=lat) if return_dict else (lat,)
