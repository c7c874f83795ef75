"""Vision Transformer image towers of the score tail, on the HIP operators: OpenAI CLIP ViT-B/32 (`clip_similarity`,
`clip_prompt_score`; reference text_to_image/compute_model_behaviors.py:243,358-388), open-CLIP ViT-L-14 with the LAION
aesthetic head (`aesthetic_score`; :253-262,419-431, src/aesthetics.py) and the BLIP-VQA vision tower whose `pooler_output`
the CelebA diversity score clusters (src/attributions/global_scores/diversity_score.py:89-120).

Eval only, fp32 throughout.  The three are one network, a pre-LN Vision Transformer (its blocks are gad/encoder.py's):

    patches = resize + crop + patchify(images)                       gad_resize_bicubic_patches   [B g g][P P 3]
    x = LN_pre?([cls | patches W_patch' + b'] + pos)                 gad_gemm, gad_vit_tokens     [B T][W]
    per block:  x += out_proj(attn(ln_1(x) W_qkv + b))               gad_layernorm_fwd, gad_gemm, gad_attention_fwd, gad_gemm
                x += c_proj(act(c_fc(ln_2(x))))                      gad_layernorm_fwd, gad_gemm, gad_gelu, gad_gemm
    CLIP:  ln_post(x[:, 0]) proj          BLIP:  post_layernorm(x)[:, 0]   (= post_layernorm(x[:, 0]): the norm is per row)

The qkv projection is one [3W, W] contraction that the attention kernel reads in place; both residual adds ride in the
contraction's epilogue.  `forward` returns the raw embedding, `embed_unit` the L2-normalised one (gad_l2_normalize_rows).

Preprocessing: [B,3,H,W] in [0,1].  CLIP: Resize(n_px, BICUBIC) of the shorter side + CenterCrop(n_px); BLIP: resize to
n_px x n_px.  Both are one launch that writes the patch matrix directly (the resized image never exists); the filter is
PIL's / torch's antialiased bicubic.  PIL's uint8 rounding of the intermediate and of the result is NOT reproduced: the
input here is a float tensor, not a PIL image.  (x - mean) / std is folded into the patch embedding at load time - the
convolution has stride = kernel and no padding, so W' = W / std per input channel and b' = b - sum W mean / std exactly
(fp64, rounded once) - and the resize runs with a = 1, b = 0.

State dicts (missing keys and wrong shapes are refused by name, extra keys ignored, fp16 tensors cast to fp32):
  OpenAI / open-CLIP layout, optional prefix `visual.`: conv1.weight, class_embedding, positional_embedding, ln_pre.*,
    transformer.resblocks.{i}.{ln_1,ln_2}.*, ...attn.in_proj_weight / in_proj_bias, ...attn.out_proj.*, ...mlp.c_fc.*,
    ...mlp.c_proj.*, ln_post.*, proj.
  HF BLIP layout, optional prefix `vision_model.`: embeddings.patch_embedding.{weight,bias}, embeddings.class_embedding,
    embeddings.position_embedding, encoder.layers.{i}.{layer_norm1,layer_norm2}.*, ...self_attn.qkv.*,
    ...self_attn.projection.*, ...mlp.{fc1,fc2}.*, post_layernorm.*.
The layout follows from the configuration: a tower with an `embed_dim` is CLIP's, one without is BLIP's."""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np
import torch

from . import _capi, encoder, ops
from ._capi import check
from .extractor import Extractor, check_state_dict, file_tag, load_checkpoint

CLIP_MEAN, CLIP_STD = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)


@dataclass(frozen=True)
class Config:
    image_size: int
    patch: int
    width: int
    layers: int
    heads: int
    mlp: int
    embed_dim: int | None            # CLIP's projection; None: BLIP (pooler_output, unprojected)
    act: str = "quick_gelu"          # "gelu" (exact erf) | "quick_gelu"
    ln_pre: bool = True
    patch_bias: bool = False
    eps: float = 1e-5
    mean: tuple = CLIP_MEAN
    std: tuple = CLIP_STD

    @property
    def grid(self):
        return self.image_size // self.patch

    @property
    def tokens(self):
        return self.grid * self.grid + 1

    @property
    def layout(self):
        return "clip" if self.embed_dim is not None else "blip"


PRESETS = {
    "clip_vit_b32": Config(224, 32, 768, 12, 12, 3072, 512),
    "clip_vit_l14": Config(224, 14, 1024, 24, 16, 4096, 768),
    "blip_vqa_base": Config(384, 16, 768, 12, 12, 3072, None, act="gelu", ln_pre=False, patch_bias=True, eps=1e-5),
}


def _config(preset_or_config):
    if isinstance(preset_or_config, Config):
        return preset_or_config, "vit"
    if preset_or_config not in PRESETS:
        raise ValueError(f"VisionTower: unknown preset {preset_or_config!r}: use one of {sorted(PRESETS)}")
    return PRESETS[preset_or_config], preset_or_config


# layout names -> the tower's own, around the blocks (`blocks`: their layout in gad/encoder.py); `lead`: the dimensions BLIP's
# embeddings keep in front for broadcasting
_NAMES = {
    "clip": dict(prefix="visual.", patch="conv1", cls="class_embedding", pos="positional_embedding", ln_pre="ln_pre",
                 blocks="openai", ln_post="ln_post", lead=()),
    "blip": dict(prefix="vision_model.", patch="embeddings.patch_embedding", cls="embeddings.class_embedding",
                 pos="embeddings.position_embedding", ln_pre="pre_layernorm", blocks="hf_fused", ln_post="post_layernorm", lead=(1,)),
}


def expected_shapes(preset_or_config):
    """{state-dict key without prefix: shape} of everything `load_state_dict` reads, in the layout's own names."""
    cfg, _ = _config(preset_or_config)
    W, n = cfg.width, _NAMES[cfg.layout]
    out = {n["patch"] + ".weight": (W, 3, cfg.patch, cfg.patch)}
    if cfg.patch_bias:
        out[n["patch"] + ".bias"] = (W,)
    out[n["cls"]], out[n["pos"]] = 2 * n["lead"] + (W,), n["lead"] + (cfg.tokens, W)
    if cfg.ln_pre:
        out[n["ln_pre"] + ".weight"], out[n["ln_pre"] + ".bias"] = (W,), (W,)
    for i in range(cfg.layers):
        out.update(encoder.block_shapes(n["blocks"], i, W, cfg.mlp))
    out[n["ln_post"] + ".weight"], out[n["ln_post"] + ".bias"] = (W,), (W,)
    if cfg.embed_dim is not None:
        out["proj"] = (W, cfg.embed_dim)
    return out


def seeded_state_dict(preset_or_config, seed):
    """`encoder.seeded` of `expected_shapes`"""
    return encoder.seeded(expected_shapes(preset_or_config), seed)


def fold_normalisation(weight, bias, mean, std):
    """Patch convolution [W, 3, P, P] (+ bias or None) on (x - mean) / std  ->  (W', b') on x: W' = W / std per input channel,
    b' = b - sum W mean / std, both in fp64 (the caller rounds them once to fp32)."""
    w = weight.detach().double()
    m = torch.tensor(mean, dtype=torch.float64).view(1, 3, 1, 1)
    s = torch.tensor(std, dtype=torch.float64).view(1, 3, 1, 1)
    w2 = w / s
    b = bias.detach().double() if bias is not None else torch.zeros(w.shape[0], dtype=torch.float64)
    b2 = b - (w2 * m).sum(dim=(1, 2, 3))
    return w2, b2


def resize_geometry(H, W, R, layout):
    """(rh, rw, oy, ox) of the virtual resized image and the crop origin: CLIP resizes the shorter side to R (torchvision's
    Resize(int): the longer one is int(R * long / short)) and crops the centre (CenterCrop: int(round((size - R) / 2)));
    BLIP resizes straight to R x R."""
    if layout == "blip":
        return R, R, 0, 0
    if H <= W:
        rh, rw = R, int(R * W / H)
    else:
        rh, rw = int(R * H / W), R
    return rh, rw, int(round((rh - R) / 2.0)), int(round((rw - R) / 2.0))


def bicubic_taps(n_in, n_out, origin, n):
    """The kernel's tap table on the host in fp64 (the library's own routine, no GPU needed): for resized indices
    [origin, origin + n) of an axis n_in -> n_out  ->  (start int32 [n], count int32 [n], weights float64 [n, kmax])."""
    lib = _capi.load()
    kmax = lib.gad_bicubic_max_taps(n_in, n_out)
    if kmax < 0:
        raise _capi.GadError(lib.gad_last_error().decode())
    start, count = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    w = np.zeros((n, kmax), dtype=np.float64)
    check(lib.gad_bicubic_taps(n_in, n_out, origin, n, start.ctypes.data, count.ctypes.data, w.ctypes.data), "gad_bicubic_taps")
    return start, count, w


def resize_matrix(n_in, n_out, origin, n, dtype=np.float64):
    """`bicubic_taps` as a dense [n, n_in] matrix (tests and references: resized = My @ image @ Mx.T)."""
    start, count, w = bicubic_taps(n_in, n_out, origin, n)
    M = np.zeros((n, n_in), dtype=np.float64)
    for o in range(n):
        M[o, start[o]:start[o] + count[o]] = w[o, :count[o]]
    return M.astype(dtype)


def resize_patches_raw(x, R, P, rh, rw, oy, ox, a=1.0, b=0.0):
    """[B,3,H,W] fp32 device tensor -> the patch matrix [B (R/P)^2, P P 3] (gad_resize_bicubic_patches)"""
    ops._req(x, "resize_bicubic_patches input")
    Bn, Cn, H, W = x.shape
    if Cn != 3:
        raise _capi.GadError(f"resize_bicubic_patches: expected 3 channels, got {Cn}")
    lib = _capi.load()
    need = lib.gad_resize_bicubic_patches_workspace_bytes(H, W, rh, rw, oy, ox, R, P)
    if need < 0:
        raise _capi.GadError(lib.gad_last_error().decode())
    ws = ops._scratch("ws", need, x.device)            # stream-ordered: safe to drop after the launch
    y = torch.empty((Bn * (R // P) ** 2, P * P * 3), device=x.device, dtype=torch.float32)
    check(lib.gad_resize_bicubic_patches(x.data_ptr(), y.data_ptr(), Bn, H, W, rh, rw, oy, ox, R, P, a, b, ws.data_ptr(), need,
                                         ops._stream()), "gad_resize_bicubic_patches")
    return y


class VisionTower(Extractor):
    """[B,3,H,W] in [0,1] -> embeddings [B, embed_dim or width] (`forward`); `embed_unit` L2-normalises them."""

    def __init__(self, preset_or_config, state_dict=None, tag=None):
        self.cfg, self.name = _config(preset_or_config)
        c = self.cfg
        encoder.check_config("VisionTower", c, grid=(c.image_size, c.patch))
        self.owner = f"VisionTower({self.name})"
        self.dims = c.embed_dim if c.embed_dim is not None else c.width
        # the blocks' activations plus the patch matrix g g 3 P P, in floats per image: B/32 50 x 8448 + 150528 = 0.57 M (2.3 MB),
        # L/14 257 x 11264 + 150528 = 3.0 M (12 MB), BLIP 577 x 8448 + 442368 = 5.3 M (21 MB) -> 0.5 GB holds 234 / 44 / 25 images:
        # 128 / 32 / 16
        self.max_batch = encoder.max_batch(c.tokens, c.width, c.mlp, extra=c.image_size * c.image_size * 3)
        super().__init__(tag or f"{self.name}-unloaded", state_dict)

    @classmethod
    def seeded(cls, preset_or_config, seed=1234):
        _, name = _config(preset_or_config)
        return cls(preset_or_config, seeded_state_dict(preset_or_config, seed), tag=f"{name}-seeded{seed}")

    @classmethod
    def from_file(cls, path, preset):
        return cls(preset, load_checkpoint(path, torchscript=True), tag=file_tag(preset, path))

    def load_state_dict(self, sd):
        cfg, names = self.cfg, _NAMES[self.cfg.layout]
        want = expected_shapes(cfg)
        prefix = names["prefix"] if any(k.startswith(names["prefix"]) for k in sd) and next(iter(want)) not in sd else ""
        check_state_dict(self.owner, sd, want, prefix)

        def get(k):
            return sd[prefix + k].detach().float().contiguous()

        def pair(k):
            return get(k + ".weight"), get(k + ".bias")

        w = {}
        pw = get(names["patch"] + ".weight")
        pb = get(names["patch"] + ".bias") if cfg.patch_bias else None
        pw, pb = fold_normalisation(pw, pb, cfg.mean, cfg.std)
        w["patch"] = (pw.float().permute(0, 2, 3, 1).reshape(cfg.width, -1).contiguous(), pb.float().contiguous())      # columns in (ph, pw, c) order
        w["cls"] = get(names["cls"]).reshape(cfg.width).contiguous()
        w["pos"] = get(names["pos"]).reshape(cfg.tokens, cfg.width).contiguous()
        if cfg.ln_pre:
            w["ln_pre"] = pair(names["ln_pre"])
        for i in range(cfg.layers):
            w[i] = encoder.load_block(get, names["blocks"], i)
        w["ln_post"] = pair(names["ln_post"])
        if cfg.embed_dim is not None:
            w["head"] = get("proj").t().contiguous()           # [embed, width]: K-contiguous like every Linear weight
        self.w = w
        return self

    # ---- launches ----
    def tokens(self, images_nchw01):
        """[B,3,H,W] in [0,1] -> the token sequence [B T, W] in front of the first block"""
        cfg = self.cfg
        x = ops._req(images_nchw01.float().contiguous(), f"{self.name} input")
        Bn, _, H, W = x.shape
        patches = resize_patches_raw(x, cfg.image_size, cfg.patch, *resize_geometry(H, W, cfg.image_size, cfg.layout))
        emb = ops.linear_fwd_raw(patches, *self.w["patch"], force_f32=True)
        out = torch.empty((Bn * cfg.tokens, cfg.width), device=x.device, dtype=torch.float32)
        g, b = self.w["ln_pre"] if cfg.ln_pre else (None, None)
        check(_capi.load().gad_vit_tokens(emb.data_ptr(), self.w["cls"].data_ptr(), self.w["pos"].data_ptr(), ops._ptr(g), ops._ptr(b),
                                          out.data_ptr(), Bn, cfg.tokens, cfg.width, cfg.eps, ops._stream()), "gad_vit_tokens")
        return out

    def _chunk(self, images_nchw01):
        cfg, Bn = self.cfg, images_nchw01.shape[0]
        x = self.tokens(images_nchw01)
        for i in range(cfg.layers):
            x = encoder.block(x, Bn, cfg.tokens, cfg.width, cfg.heads, cfg.act, cfg.eps, self.w[i], ops.attention_core_qkv_raw)
        pooled = encoder.ln(x.view(Bn, cfg.tokens, cfg.width)[:, 0].contiguous(), self.w["ln_post"], cfg.eps)
        return ops.linear_fwd_raw(pooled, self.w["head"], force_f32=True) if cfg.embed_dim is not None else pooled

    def forward(self, images_nchw01):
        with ops.operand_precision("f32"):                # the attention kernel follows the process-wide switch; this tower is fp32
            return super().forward(images_nchw01)

    def embed_unit(self, images_nchw01):
        out = self.forward(images_nchw01)
        return ops.l2_normalize_rows_raw(out if out.is_contiguous() else out.contiguous())


class AestheticHead:
    """LAION's aesthetic predictor on open-CLIP ViT-L-14 (reference src/aesthetics.py: nn.Linear(768, 1) on the L2-normalised
    image embedding): score = embed_unit(x) @ weight.T + bias.  State-dict keys `weight` [1, E], `bias` [1]."""

    def __init__(self, tower, state_dict=None, tag=None):
        self.tower, self.tag = tower, tag or "aesthetic-unloaded"
        self.weight = self.bias = None
        if state_dict is not None:
            self.load_state_dict(state_dict)

    @classmethod
    def seeded(cls, tower, seed=1234):
        g = torch.Generator().manual_seed(seed)
        sd = {"weight": torch.randn(1, tower.dims, generator=g) / math.sqrt(tower.dims), "bias": torch.randn(1, generator=g)}
        return cls(tower, sd, tag=f"aesthetic-seeded{seed}")

    @classmethod
    def from_file(cls, tower, path):
        return cls(tower, load_checkpoint(path, torchscript=True), tag=file_tag("aesthetic", path))

    def load_state_dict(self, sd):
        check_state_dict("AestheticHead", sd, {"weight": (1, self.tower.dims), "bias": (1,)})
        self.weight, self.bias = sd["weight"].detach().float().contiguous(), sd["bias"].detach().float().contiguous()
        return self

    def to(self, device):
        self.weight, self.bias = self.weight.to(device), self.bias.to(device)
        return self

    @torch.no_grad()
    def score_unit(self, unit):
        """[B, E] unit embeddings -> [B] scores (one contraction with the bias in its epilogue)"""
        return ops.linear_fwd_raw(unit, self.weight, self.bias, force_f32=True).view(-1)

    def __call__(self, images_nchw01):
        return self.score_unit(self.tower.embed_unit(images_nchw01))
