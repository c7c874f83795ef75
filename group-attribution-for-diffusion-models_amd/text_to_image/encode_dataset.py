"""From an image folder to the files every Stable-Diffusion program here starts from.

The reference encodes inside its training loop (text_to_image/train_text_to_image_lora.py:1065-1077 resize, crop, flip;
:1220-1223 `vae.encode(x).latent_dist.sample() * scaling_factor`; :1055,1249 the text encoder).  The frozen encoders' outputs
are functions of (image, flipped or not) and of the caption, so they run once, here:

  metadata.csv (text_to_image/artbench/metadata.py) -> every image through gad.latents.load_image_u8 (RGB, bilinear resize,
  centre crop) -> the uint8 array on the device -> gad_pixels_to_nchw, plain then mirrored -> gad.AutoencoderKL.encode_moments

and writes under --train_data_dir, in metadata row order:

  moment_cache.pt    the posterior moments [N, F, 2L, h, w] of both orientations (F = 1 under --no_flip), the prompt
                     embeddings and the metadata columns (gad/latents.py): `--latent_source moments` of the trainer
  latent_cache.pt    latents = mean * scaling_factor of the unflipped encode - latent_dist.mode(), what the reference's gradient
                     script takes (grad_text_to_image_lora.py:435) - with the same embeddings and columns: what
                     train_text_to_image_lora.py (default), grad_text_to_image_lora.py and baselines.py read
  train_pixels.npy   uint8 [N, H, W, 3]: the file `baselines.py --train_pixels` asks for

Environment:
  GAD_VAE_WEIGHTS=/path                      the SD VAE's state dict (.pt or .safetensors, diffusers' AutoencoderKL keys)
  GAD_SD_TEXT_WEIGHTS=/path + GAD_CLIP_BPE   SD's text encoder and the tokenizer's vocabulary (gad/text.py): the unique captions
                                             are encoded; or pass --text_emb FILE (a [77, D] tensor shared by every row, a
                                             `--prompt_embeds` dict whose "cond" is shared, or {caption: [77, D]})
Both are looked for before any image is read, and an existing output is not overwritten without --overwrite."""
import argparse
import os
import sys

import numpy as np
import torch

_HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

from text_to_image.artbench.metadata import read_metadata  # noqa: E402

VAE_VAR = "GAD_VAE_WEIGHTS"


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="encode an image folder into moment_cache.pt, latent_cache.pt and train_pixels.npy")
    p.add_argument("--train_data_dir", type=str, required=True)
    p.add_argument("--resolution", type=int, default=256)
    p.add_argument("--center_crop", action="store_true")
    p.add_argument("--cls_key", type=str, default=None)
    p.add_argument("--cls", type=str, default=None)
    p.add_argument("--no_flip", action="store_true", help="encode the plain orientation only (the trainer then refuses --random_flip)")
    p.add_argument("--batch_size", type=int, default=64, help="images per encoder pass")
    p.add_argument("--text_emb", type=str, default=None, help="prompt embeddings file instead of the text encoder")
    p.add_argument("--overwrite", action="store_true")
    p.add_argument("--device", type=str, default="cuda:0")
    return p.parse_args(argv)


def _text_rows(obj, captions, what):
    """`obj`: a [T, D] / [1, T, D] tensor shared by every row, a dict with "cond" (a --prompt_embeds file), or {caption: [T, D]}
    -> [1, T, D] or [N, T, D] fp32"""
    if isinstance(obj, torch.Tensor):
        if obj.dim() not in (2, 3) or (obj.dim() == 3 and obj.shape[0] != 1):
            raise ValueError(f"{what}: a shared embedding must be [tokens, width] or [1, tokens, width], got {tuple(obj.shape)}")
        return obj.float().reshape(1, *obj.shape[-2:])
    if isinstance(obj, dict) and all(c in obj for c in captions):
        return torch.stack([obj[c].float() for c in captions])
    if isinstance(obj, dict) and "cond" in obj:
        return _text_rows(obj["cond"], captions, what)
    absent = [c for c in dict.fromkeys(captions) if not (isinstance(obj, dict) and c in obj)]
    raise KeyError(f"{what}: neither a tensor, nor a dict with 'cond', nor one entry per caption ({len(absent)} absent, e.g. {absent[:2]})")


def _encode_captions(captions, device):
    """hidden states of the unique captions through SD's text encoder, in row order; one shared row when all captions agree"""
    from gad.clip_bpe import ClipBPE
    from gad.text import TextTower, sd_text_setting
    weights, bpe = sd_text_setting()
    tower = TextTower.from_file(weights, "sd_text_l14").to(device)
    unique = list(dict.fromkeys(captions))
    ids = ClipBPE(bpe).encode_batch(unique, tower.cfg.context, pad="eot")
    hidden = tower.hidden(torch.from_numpy(ids)).float().cpu()
    if len(unique) == 1:
        return hidden[:1]
    index = {c: i for i, c in enumerate(unique)}
    return hidden[[index[c] for c in captions]]


def _to_nchw(pixels, lut, flip):
    """fp32 [B, 3, H, W] = lut[pixels], mirrored along W when `flip`: gad_pixels_to_nchw on the device.  On --device cpu (the tests'
    injected stand-in encoder; gad.AutoencoderKL has no CPU path) the same table lookup as host indexing."""
    if pixels.is_cuda:
        from gad import ops
        return ops.pixels_to_nchw_raw(pixels, lut, flip=flip)
    x = lut[pixels.long()].permute(0, 3, 1, 2)
    return (x.flip(3) if flip else x).contiguous()


def main(a, vae=None, text_emb=None):
    """`vae`: an object with `encode_moments([B,3,H,W]) -> [B,2L,h,w]`, `config.scaling_factor` and `tag` in place of the file
    GAD_VAE_WEIGHTS names; `text_emb`: what --text_emb's file would hold."""
    from gad.latents import LATENT_CACHE, MOMENT_CACHE, TRAIN_PIXELS, load_image_u8, write_moment_cache
    from gad.similarity import pixel_lut
    from gad.text import sd_text_setting
    outputs = [os.path.join(a.train_data_dir, f) for f in (MOMENT_CACHE, LATENT_CACHE, TRAIN_PIXELS)]
    existing = [f for f in outputs if os.path.exists(f)]
    if existing and not a.overwrite:
        raise FileExistsError(f"{existing[0]} exists: pass --overwrite to replace it")
    if vae is None and not os.environ.get(VAE_VAR):
        raise ValueError(f"{VAE_VAR} is not set: it names the SD VAE's state dict (.pt or .safetensors) the images are encoded with")
    if text_emb is None and a.text_emb is None and sd_text_setting() is None:
        raise ValueError("no text source: pass --text_emb FILE, or set GAD_SD_TEXT_WEIGHTS and GAD_CLIP_BPE to encode the captions")
    if a.batch_size < 1:
        raise ValueError(f"--batch_size {a.batch_size} must be >= 1")
    device = torch.device(a.device)

    df = read_metadata(a.train_data_dir, a.cls_key, a.cls)
    if len(df) == 0:
        raise ValueError(f"{a.train_data_dir}/metadata.csv has no row with {a.cls_key} == {a.cls!r}")
    captions = df["caption"].tolist()
    if text_emb is None and a.text_emb is not None:
        text_emb = torch.load(a.text_emb, map_location="cpu", weights_only=False)
    text = _text_rows(text_emb, captions, a.text_emb or "text_emb") if text_emb is not None else _encode_captions(captions, device)

    pixels_host = np.stack([load_image_u8(os.path.join(a.train_data_dir, f), a.resolution, a.center_crop) for f in df["file_name"]])
    if vae is None:
        import gad
        vae = gad.AutoencoderKL.from_file(os.environ[VAE_VAR], "SD_VAE")
    if hasattr(vae, "to"):
        vae = vae.to(device)
    pixels = torch.from_numpy(pixels_host).to(device)             # stays on the device as bytes: 5 000 x 256 x 256 x 3 = 0.98 GB
    lut = torch.from_numpy(pixel_lut()).to(device)
    n, orientations, moments = len(df), (False,) if a.no_flip else (False, True), None
    for s in range(0, n, a.batch_size):
        for f, flip in enumerate(orientations):
            m = vae.encode_moments(_to_nchw(pixels[s:s + a.batch_size], lut, flip)).float().cpu()
            if moments is None:
                moments = torch.empty((n, len(orientations)) + tuple(m.shape[1:]), dtype=torch.float32)
            moments[s:s + a.batch_size, f] = m

    sf = float(vae.config.scaling_factor)
    meta = {c: df[c].tolist() for c in ("artist", "filename", "style", "caption")}
    write_moment_cache(outputs[0], moments, text, meta, sf, a.resolution, getattr(vae, "tag", type(vae).__name__))
    L = moments.shape[2] // 2
    torch.save({"latents": moments[:, 0, :L] * sf, "text_emb": text, **meta}, outputs[1])
    np.save(outputs[2], pixels_host)
    print(f"{n} images at {a.resolution} x {a.resolution} -> {', '.join(outputs)}")
    return True


if __name__ == "__main__":
    main(parse_args())
