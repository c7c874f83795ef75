"""CLIP text towers on the HIP operators: the text half of OpenAI CLIP ViT-B/32 (`clip_prompt_score`; reference
text_to_image/compute_model_behaviors.py:302-306, clip.tokenize + encode_text) and Stable Diffusion 1.x's `CLIPTextModel`
(`text_encoder(ids)[0]`, the U-Net's cross-attention context; train_text_to_image_lora.py:723-731,1055,1249,
grad_text_to_image_lora.py:275-283, compute_model_behaviors.py:235,293-299).

Eval only, fp32 throughout.  Both are one network, a pre-LN transformer under a causal mask (its blocks are gad/encoder.py's):

    x = token_emb[ids] + pos                                         gad_text_tokens              [B T][W]
    per block:  x += out_proj(causal_attn(ln_1(x) W_qkv + b))        gad_layernorm_fwd, gad_gemm, gad_attention_causal_fwd, gad_gemm
                x += c_proj(quick_gelu(c_fc(ln_2(x))))               gad_layernorm_fwd, gad_gemm, gad_gelu, gad_gemm
    hidden = ln_final(x)                                             HF's last_hidden_state
    embed  = ln_final(x[b, eot(b)]) text_projection                  gad_gather_rows, gad_layernorm_fwd, gad_gemm

The qkv projection is one [3W, W] contraction that the causal attention kernel reads in place (HF's separate q / k / v
weights are stacked at load time); both residual adds ride in the contraction's epilogue.  LayerNorm is per row, so `embed`
gathers the B end-of-text rows first and normalises only those.

The end-of-text position is `argmax(ids[b])`: end-of-text is the highest id of CLIP's vocabulary, so OpenAI's argmax and HF's
"first eos" position are the same row - for any padding (the end token again, or 0) - as long as the ids come from that
vocabulary.  argmax takes the first maximum.

State dicts (missing keys and wrong shapes are refused by name, extra keys ignored, fp16 tensors cast to fp32):
  OpenAI layout, no prefix (a whole CLIP archive is fine: `visual.*` and `logit_scale` are extra keys): token_embedding.weight,
    positional_embedding, transformer.resblocks.{i}.{ln_1,ln_2}.*, ...attn.in_proj_weight / in_proj_bias, ...attn.out_proj.*,
    ...mlp.c_fc.*, ...mlp.c_proj.*, ln_final.*, text_projection [W, E].
  HF layout, optional prefix `text_model.`: embeddings.token_embedding.weight, embeddings.position_embedding.weight,
    encoder.layers.{i}.self_attn.{q_proj,k_proj,v_proj,out_proj}.*, ...layer_norm1.*, ...layer_norm2.*, ...mlp.{fc1,fc2}.*,
    final_layer_norm.*, and text_projection.weight [E, W] (never prefixed) when the configuration has an `embed_dim`.
The layout is read off the state dict (which of the two token-embedding keys it holds).

Environment (text_to_image/compute_model_behaviors.py, grad_text_to_image_lora.py, baselines.py):
  GAD_CLIP_BPE=/path          the tokenizer's vocabulary (gad/clip_bpe.py)
  GAD_SD_TEXT_WEIGHTS=/path   SD's text_encoder/model.safetensors or .bin
`python -m gad.text --prompt "..." --out pe.pt` writes `cond`, `uncond` and `clip_prompt` for whichever towers are configured."""
from __future__ import annotations

import os
from dataclasses import dataclass

import torch

from . import _capi, encoder, ops
from .extractor import Extractor, check_state_dict, file_tag, load_checkpoint


@dataclass(frozen=True)
class TextConfig:
    vocab: int
    context: int
    width: int
    layers: int
    heads: int
    mlp: int
    embed_dim: int | None            # the text projection; None: hidden states only (SD's CLIPTextModel)
    act: str = "quick_gelu"          # "gelu" (exact erf) | "quick_gelu"
    eps: float = 1e-5


PRESETS = {
    "clip_text_b32": TextConfig(49408, 77, 512, 12, 8, 2048, 512),
    "sd_text_l14": TextConfig(49408, 77, 768, 12, 12, 3072, None),
}
PRESET_LAYOUT = {"clip_text_b32": "openai", "sd_text_l14": "hf"}


def _config(preset_or_config):
    if isinstance(preset_or_config, TextConfig):
        return preset_or_config, "text"
    if preset_or_config not in PRESETS:
        raise ValueError(f"TextTower: unknown preset {preset_or_config!r}: use one of {sorted(PRESETS)}")
    return PRESETS[preset_or_config], preset_or_config


def _check_config(cfg):
    encoder.check_config("TextTower", cfg)
    if not ops.attention_causal_ok(cfg.context, cfg.width // cfg.heads):
        raise ValueError(f"TextTower: context {cfg.context} with head dim {cfg.width // cfg.heads}: the causal attention kernel "
                         f"takes 1..128 tokens and head dims 16, 32, 64")


def _layout(preset_or_config, layout):
    cfg, name = _config(preset_or_config)
    layout = layout or PRESET_LAYOUT.get(name) or ("openai" if cfg.embed_dim is not None else "hf")
    if layout not in ("openai", "hf"):
        raise ValueError(f"TextTower: layout {layout!r}: use 'openai' or 'hf'")
    if layout == "openai" and cfg.embed_dim is None:
        raise ValueError("TextTower: the OpenAI layout always has a text_projection: the configuration needs an embed_dim")
    return cfg, layout


# layout names -> the tower's own, around the blocks (`blocks`: their layout in gad/encoder.py)
_NAMES = {
    "openai": dict(tok="token_embedding.weight", pos="positional_embedding", blocks="openai", ln_final="ln_final"),
    "hf": dict(tok="embeddings.token_embedding.weight", pos="embeddings.position_embedding.weight", blocks="hf_split",
               ln_final="final_layer_norm"),
}


def expected_shapes(preset_or_config, layout=None):
    """{state-dict key without prefix: shape} of everything `load_state_dict` reads, in the layout's own names.  `layout`:
    'openai' | 'hf'; None: the preset's, or by `embed_dim` for a plain configuration."""
    cfg, layout = _layout(preset_or_config, layout)
    W, n = cfg.width, _NAMES[layout]
    out = {n["tok"]: (cfg.vocab, W), n["pos"]: (cfg.context, W)}
    for i in range(cfg.layers):
        out.update(encoder.block_shapes(n["blocks"], i, W, cfg.mlp))
    out[n["ln_final"] + ".weight"], out[n["ln_final"] + ".bias"] = (W,), (W,)
    if layout == "openai":
        out["text_projection"] = (W, cfg.embed_dim)
    elif cfg.embed_dim is not None:
        out["text_projection.weight"] = (cfg.embed_dim, W)
    return out


def seeded_state_dict(preset_or_config, seed, layout=None):
    """`encoder.seeded` of `expected_shapes`"""
    return encoder.seeded(expected_shapes(preset_or_config, layout), seed)


HF_PREFIX = "text_model."


class TextTower(Extractor):
    """token ids [B, context] (host or device integers) -> `hidden` [B, T, W], `embed` [B, embed_dim], `embed_unit`;
    `max_batch` prompts per pass."""

    def __init__(self, preset_or_config, state_dict=None, tag=None):
        self.cfg, self.name = _config(preset_or_config)
        _check_config(self.cfg)
        c = self.cfg
        self.owner = f"TextTower({self.name})"
        self.dims = c.embed_dim if c.embed_dim is not None else c.width
        # the blocks' activations in floats per prompt: B/32 77 x 5632 = 0.43 M (1.7 MB), SD's 77 x 8448 = 0.65 M (2.6 MB) -> 0.5 GB
        # holds 309 / 206 prompts: 256 / 128
        self.max_batch = encoder.max_batch(c.context, c.width, c.mlp)
        super().__init__(tag or f"{self.name}-unloaded", state_dict)

    @classmethod
    def seeded(cls, preset_or_config, seed=1234):
        _, name = _config(preset_or_config)
        return cls(preset_or_config, seeded_state_dict(preset_or_config, seed), tag=f"{name}-seeded{seed}")

    @classmethod
    def from_file(cls, path, preset):
        if path.endswith(".safetensors"):
            from safetensors.torch import load_file
            sd = load_file(path, device="cpu")
        else:
            sd = load_checkpoint(path, torchscript=True)
        return cls(preset, sd, tag=file_tag(preset, path))

    def load_state_dict(self, sd):
        cfg = self.cfg
        if "token_embedding.weight" in sd:
            layout, prefix = "openai", ""
        elif "embeddings.token_embedding.weight" in sd:
            layout, prefix = "hf", ""
        elif HF_PREFIX + "embeddings.token_embedding.weight" in sd:
            layout, prefix = "hf", HF_PREFIX
        else:
            raise KeyError(f"{self.owner}: missing key 'token_embedding.weight' (OpenAI layout) or "
                           f"'[{HF_PREFIX}]embeddings.token_embedding.weight' (HF layout)")
        want = expected_shapes(cfg, layout)
        head = want.pop("text_projection.weight", None)          # HF: beside `text_model`, not under it
        check_state_dict(self.owner, sd, want, prefix)
        if head is not None:
            check_state_dict(self.owner, sd, {"text_projection.weight": head})

        def get(k):
            return sd[prefix + k].detach().float().contiguous()

        n = _NAMES[layout]
        w = {"tok": get(n["tok"]), "pos": get(n["pos"])}
        for i in range(cfg.layers):
            w[i] = encoder.load_block(get, n["blocks"], i)
        w["ln_final"] = get(n["ln_final"] + ".weight"), get(n["ln_final"] + ".bias")
        if layout == "openai":
            w["head"] = get("text_projection").t().contiguous()         # [embed, width]: K-contiguous like every Linear weight
        elif head is not None:
            w["head"] = sd["text_projection.weight"].detach().float().contiguous()
        self.w = w
        return self

    # ---- launches ----
    def _trunk(self, ids):
        """ids [B, T] -> the residual stream after the last block [B T, W] (before ln_final)"""
        cfg = self.cfg
        x = ops.text_tokens_raw(ids, self.w["tok"], self.w["pos"])
        for i in range(cfg.layers):
            x = encoder.block(x, ids.shape[0], cfg.context, cfg.width, cfg.heads, cfg.act, cfg.eps, self.w[i], ops.attention_causal_qkv_raw)
        return x

    def _hidden_chunk(self, ids):
        return encoder.ln(self._trunk(ids), self.w["ln_final"], self.cfg.eps).view(ids.shape[0], self.cfg.context, self.cfg.width)

    def _pooled_chunk(self, ids):
        rows = ids.argmax(dim=-1)                                 # the end-of-text row (see the module docstring)
        return encoder.ln(ops.gather_rows_raw(self._trunk(ids), rows, self.cfg.context), self.w["ln_final"], self.cfg.eps)

    def _embed_chunk(self, ids):
        return ops.linear_fwd_raw(self._pooled_chunk(ids), self.w["head"], force_f32=True)

    @torch.no_grad()
    def _run(self, chunk, ids):
        ids = torch.as_tensor(ids)
        if ids.ndim != 2 or ids.shape[1] != self.cfg.context or ids.is_floating_point():
            raise _capi.GadError(f"{self.owner}: token ids must be integers [B, {self.cfg.context}], got {ids.dtype} {tuple(ids.shape)}")
        ids = ids.detach().cpu()                                  # a few hundred integers: they are checked and pooled on the host
        with ops.operand_precision("f32"):                        # this tower is fp32 whatever the process-wide switch says
            return self._chunked(chunk, ids)

    def hidden(self, ids):
        """[B, T, W] after the final LayerNorm: HF's `last_hidden_state`"""
        return self._run(self._hidden_chunk, ids)

    def pooled(self, ids):
        """[B, W]: ln_final of the end-of-text row, unprojected (HF's `pooler_output`)"""
        return self._run(self._pooled_chunk, ids)

    def embed(self, ids):
        """[B, embed_dim]: ln_final(x)[b, argmax(ids[b])] @ text_projection (OpenAI's `encode_text`, HF's `text_embeds`)"""
        if "head" not in self.w and self.w:
            raise _capi.GadError(f"{self.owner}: this tower has no text_projection (embed_dim is None): use `hidden`")
        return self._run(self._embed_chunk, ids)

    def embed_unit(self, ids):
        out = self.embed(ids)
        return ops.l2_normalize_rows_raw(out if out.is_contiguous() else out.contiguous())

    def __call__(self, ids):
        return self.embed(ids)


# ---- shims with the reference's names ---------------------------------------------------------------------------------------
class CLIPTextModel:
    """`text_encoder(input_ids)` of the reference's programs: returns `(last_hidden_state, pooler_output)`, so `[0]` is what
    they read.  SD 1.x's encoder (preset sd_text_l14) unless another preset is named."""

    def __init__(self, tower):
        self.tower, self.tag = tower, tower.tag

    @classmethod
    def from_file(cls, path, preset="sd_text_l14"):
        return cls(TextTower.from_file(path, preset))

    def to(self, device):
        self.tower.to(device)
        return self

    def __call__(self, input_ids):
        return self.tower.hidden(input_ids), self.tower.pooled(input_ids)


class _Encoding:
    def __init__(self, input_ids):
        self.input_ids = input_ids


class CLIPTokenizer:
    """`tokenizer(prompts, max_length=tokenizer.model_max_length, padding="max_length", truncation=True, return_tensors="pt")
    .input_ids` of the reference's programs, on gad/clip_bpe.py: padded with the end token, as SD's tokenizer pads."""

    model_max_length = 77

    def __init__(self, bpe):
        self.bpe = bpe

    @classmethod
    def from_path(cls, path):
        from .clip_bpe import ClipBPE
        return cls(ClipBPE(path))

    def __call__(self, text, max_length=None, padding="max_length", truncation=True, return_tensors="pt"):
        if padding != "max_length" or not truncation or return_tensors != "pt":
            raise ValueError("CLIPTokenizer: only padding='max_length', truncation=True, return_tensors='pt' are provided")
        texts = [text] if isinstance(text, str) else list(text)
        ids = self.bpe.encode_batch(texts, max_length or self.model_max_length, pad="eot")
        return _Encoding(torch.from_numpy(ids).long())


# ---- what the entry points read from the environment -----------------------------------------------------------------------
BPE_VAR, SD_TEXT_VAR, CLIP_B32_VAR = "GAD_CLIP_BPE", "GAD_SD_TEXT_WEIGHTS", "GAD_CLIP_B32_WEIGHTS"


def sd_text_setting():
    """Pure host code, before anything loads -> None (no GAD_SD_TEXT_WEIGHTS: prompts come from --prompt_embeds or the seeded
    stand-in, as before) or (weights path, vocabulary path).  The weights without a vocabulary are refused by name."""
    weights, bpe = os.environ.get(SD_TEXT_VAR), os.environ.get(BPE_VAR)
    if not weights:
        return None
    if not bpe:
        raise ValueError(f"{SD_TEXT_VAR} is set but {BPE_VAR} is not: the text encoder reads token ids, and the tokenizer needs "
                         f"its vocabulary (OpenAI's merges file, or a directory with vocab.json + merges.txt)")
    return weights, bpe


def sd_prompt_embeddings(prompt, device):
    """(cond, uncond, tag) from GAD_SD_TEXT_WEIGHTS + GAD_CLIP_BPE: cond = hidden(prompt), uncond = hidden("") - the empty
    negative prompt of the diffusers pipeline - each [77, W], both padded with the end token."""
    from .clip_bpe import ClipBPE
    weights, bpe = sd_text_setting()
    tower = TextTower.from_file(weights, "sd_text_l14").to(device)
    ids = ClipBPE(bpe).encode_batch([prompt, ""], tower.cfg.context, pad="eot")
    h = tower.hidden(torch.from_numpy(ids))
    return h[0], h[1], tower.tag


def prompt_context(prompt, prompt_embeds, ctx_dim, device):
    """What the text-to-image programs condition on -> (cond, uncond, prompt_encoder tag or None), each [77, ctx_dim].
    `prompt_embeds`: the loaded --prompt_embeds dict or None.  The file's keys win; GAD_SD_TEXT_WEIGHTS' encoder supplies what the
    file lacks (and only then is it loaded and its tag returned); with neither, the seeded stand-in for CLIP-text(prompt)."""
    pe = prompt_embeds or {}
    if sd_text_setting() is not None and not ("cond" in pe and "uncond" in pe):
        cond, uncond, tag = sd_prompt_embeddings(prompt, device)
        cond, uncond = pe["cond"].float() if "cond" in pe else cond, pe["uncond"].float() if "uncond" in pe else uncond
        if cond.shape[-1] != ctx_dim or uncond.shape[-1] != ctx_dim:
            raise ValueError(f"{SD_TEXT_VAR}: the context is {cond.shape[-1]} / {uncond.shape[-1]} wide, the U-Net's cross_attention_dim is {ctx_dim}")
        return cond, uncond, tag
    if prompt_embeds is not None:
        return pe["cond"].float(), pe["uncond"].float(), None
    import hashlib
    g = torch.Generator().manual_seed(int(hashlib.sha256(prompt.encode()).hexdigest()[:8], 16) % (2 ** 31))
    return torch.randn(77, ctx_dim, generator=g) * 0.5, torch.randn(77, ctx_dim, generator=g) * 0.5, None



def clip_prompt_embedding(prompt, weights_path, device):
    """(unit embedding [E], tower tag) of `prompt` as `clip.tokenize` + `encode_text` make it (zero padding) on the B/32 text
    tower - from the archive GAD_CLIP_B32_WEIGHTS names (`weights_path`), or seeded (None); needs GAD_CLIP_BPE"""
    from .clip_bpe import ClipBPE
    tower = (TextTower.from_file(weights_path, "clip_text_b32") if weights_path else TextTower.seeded("clip_text_b32")).to(device)
    ids = ClipBPE(os.environ[BPE_VAR]).encode_batch([prompt], tower.cfg.context, pad="zero")
    return tower.embed_unit(torch.from_numpy(ids))[0], tower.tag


def main(argv=None):
    import argparse
    p = argparse.ArgumentParser(description="write a --prompt_embeds file from whichever text towers the environment configures")
    p.add_argument("--prompt", type=str, required=True)
    p.add_argument("--out", type=str, required=True)
    p.add_argument("--device", type=str, default="cuda:0")
    a = p.parse_args(argv)
    if not os.environ.get(BPE_VAR):
        raise SystemExit(f"{BPE_VAR} is not set: no tokenizer vocabulary")
    device, out = torch.device(a.device), {}
    if sd_text_setting() is not None:
        sd = sd_prompt_embeddings(a.prompt, device)
        out["cond"], out["uncond"], out["prompt_encoder"] = sd[0].cpu(), sd[1].cpu(), sd[2]
    if os.environ.get(CLIP_B32_VAR) or os.environ.get("GAD_SD_SCORER") == "clip-seeded":
        e, tag = clip_prompt_embedding(a.prompt, os.environ.get(CLIP_B32_VAR), device)
        out["clip_prompt"], out["clip_prompt_encoder"] = e.cpu(), tag
    if not out:
        raise SystemExit(f"nothing to write: set {SD_TEXT_VAR} and / or {CLIP_B32_VAR} (or GAD_SD_SCORER=clip-seeded)")
    torch.save(out, a.out)
    print(f"wrote {sorted(out)} to {a.out}")


if __name__ == "__main__":
    main()
