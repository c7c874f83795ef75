"""From images to the latents a Stable-Diffusion LoRA step trains on.

The reference trainer (text_to_image/train_text_to_image_lora.py:1065-1077, 1220-1223) resizes, crops and randomly flips every
image on every step and draws a fresh `vae.encode(x).latent_dist.sample() * scaling_factor`.  With a deterministic crop the
posterior is a function of (image, flipped or not): text_to_image/encode_dataset.py encodes every image once in both
orientations and writes the moments to `moment_cache.pt`; `MomentSource` keeps them in HBM and draws a step's batch from them in
one launch (gad_latent_draw: gather, flip coin, reparameterised sample, scale) - the reference's training distribution with
no encode per step.

The host transform restates torchvision's for a PIL image (torchvision is not installed here, so the restatement is not
pinned against it): Resize(int) -> CenterCrop -> ToTensor -> Normalize([0.5], [0.5])."""
from __future__ import annotations

import os

import numpy as np
import torch

from . import _capi, ops

MOMENT_CACHE, LATENT_CACHE, TRAIN_PIXELS = "moment_cache.pt", "latent_cache.pt", "train_pixels.npy"
METADATA_KEYS = ("artist", "filename", "style", "caption")
SCALAR_KEYS = ("flips", "scaling_factor", "resolution", "vae_tag")


# ---- the reference's transform, on the host ---------------------------------------------------------------------------------
def resized_size(w: int, h: int, resolution: int):
    """(w, h) after torchvision's Resize(resolution) with an int size: the smaller edge becomes `resolution`, the other
    int(resolution * long / short)"""
    if w <= h:
        return resolution, int(resolution * h / w)
    return int(resolution * w / h), resolution


def center_crop_box(w: int, h: int, size: int):
    """PIL box (left, top, right, bottom) of torchvision's CenterCrop(size) on a w x h image that is at least size x size"""
    if w < size or h < size:
        raise ValueError(f"center_crop_box: a {w} x {h} image is smaller than the {size} x {size} crop")
    top, left = int(round((h - size) / 2.0)), int(round((w - size) / 2.0))
    return left, top, left + size, top + size


def load_image_u8(path, resolution: int, center_crop: bool):
    """uint8 [resolution, resolution, 3] of the image at `path`: RGB, bilinear Resize(resolution), CenterCrop(resolution)"""
    from PIL import Image
    with Image.open(path) as im:
        im = im.convert("RGB")
        size = resized_size(im.width, im.height, resolution)
        if size != (im.width, im.height):
            im = im.resize(size, Image.BILINEAR)
        if center_crop:
            im = im.crop(center_crop_box(im.width, im.height, resolution))
        elif (im.width, im.height) != (resolution, resolution):
            raise ValueError(f"{path}: resized to {im.width} x {im.height}, not {resolution} x {resolution}: without --center_crop "
                             f"the reference takes a RandomCrop, and moments cannot be cached over random crops")
        return np.asarray(im, dtype=np.uint8).copy()


# ---- moment_cache.pt ---------------------------------------------------------------------------------------------------------
def check_moment_cache(cache, where="moment cache"):
    """Every key of the schema, by name: moments fp32 [N, F, 2L, h, w] with F in {1, 2}, flips == (F == 2), scaling_factor,
    resolution, vae_tag, text_emb [N or 1, T, D], and one list of N entries per metadata column."""
    for k in ("moments", "text_emb") + SCALAR_KEYS + METADATA_KEYS:
        if k not in cache:
            raise KeyError(f"{where}: key {k!r} is missing")
    m = cache["moments"]
    if not (isinstance(m, torch.Tensor) and m.dtype == torch.float32 and m.dim() == 5 and m.shape[1] in (1, 2)
            and m.shape[2] % 2 == 0 and m.shape[0] >= 1):
        raise ValueError(f"{where}: key 'moments' must be fp32 [N, F, 2L, h, w] with F in (1, 2), got "
                         f"{getattr(m, 'dtype', type(m))} {tuple(getattr(m, 'shape', ()))}")
    n = m.shape[0]
    if bool(cache["flips"]) != (m.shape[1] == 2):
        raise ValueError(f"{where}: key 'flips' is {cache['flips']!r} but 'moments' holds {m.shape[1]} orientation(s)")
    t = cache["text_emb"]
    if not (isinstance(t, torch.Tensor) and t.dim() == 3 and t.shape[0] in (1, n)):
        raise ValueError(f"{where}: key 'text_emb' must be [{n} or 1, tokens, width], got {tuple(getattr(t, 'shape', ()))}")
    for k in METADATA_KEYS:
        if len(cache[k]) != n:
            raise ValueError(f"{where}: key {k!r} has {len(cache[k])} entries for {n} rows of 'moments'")
    return cache


def write_moment_cache(path, moments, text_emb, metadata, scaling_factor, resolution, vae_tag):
    """`metadata`: {column: list} with at least METADATA_KEYS.  Returns the dict written."""
    missing = [k for k in METADATA_KEYS if k not in metadata]
    if missing:
        raise KeyError(f"write_moment_cache: metadata lacks {missing}")
    moments = moments.detach().to("cpu", torch.float32).contiguous() if isinstance(moments, torch.Tensor) else moments
    cache = {"moments": moments, "flips": bool(getattr(moments, "dim", lambda: 0)() == 5 and moments.shape[1] == 2),
             "scaling_factor": float(scaling_factor), "resolution": int(resolution), "vae_tag": str(vae_tag),
             "text_emb": text_emb.detach().to("cpu", torch.float32) if isinstance(text_emb, torch.Tensor) else text_emb}
    for k in METADATA_KEYS:
        cache[k] = list(metadata[k])
    check_moment_cache(cache, str(path))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    torch.save(cache, path)
    return cache


def load_moment_cache(path):
    if not os.path.exists(path):
        raise FileNotFoundError(f"{path} not found: text_to_image/encode_dataset.py writes it from the image folder")
    return check_moment_cache(torch.load(path, map_location="cpu", weights_only=False), str(path))


# ---- the resident source -----------------------------------------------------------------------------------------------------
class MomentSource:
    """Posterior moments [N, F, 2L, h, w] resident on the device; `draw` is one gad_latent_draw on the current stream.
    Row b of a draw is a function of (seed, rows[b], step) alone: reproducible, and independent of what shares the batch."""

    def __init__(self, moments, scaling_factor, seed=0):
        if not (isinstance(moments, torch.Tensor) and moments.is_cuda):
            raise _capi.GadError("MomentSource: moments must be a device tensor (there is no CPU path)")
        self.moments = ops._req(moments, "MomentSource moments")
        if moments.dim() != 5 or moments.shape[1] not in (1, 2) or moments.shape[2] % 2:
            raise _capi.GadError(f"MomentSource: moments must be [N, F, 2L, h, w] with F in (1, 2), got {tuple(moments.shape)}")
        self.scaling_factor, self.seed = float(scaling_factor), int(seed)

    def __len__(self):
        return self.moments.shape[0]

    @property
    def flips(self):
        return self.moments.shape[1] == 2

    def subset(self, keep):
        """Dataset rows `keep` (host indices), validated once here -> int64 device tensor to index and hand to `draw`"""
        keep = np.asarray(keep)
        if keep.ndim != 1 or keep.dtype.kind not in "iu":
            raise ValueError(f"MomentSource.subset: expected a 1-D integer index array, got {keep.dtype} {keep.shape}")
        if keep.size and (keep.min() < 0 or keep.max() >= len(self)):
            raise IndexError(f"MomentSource.subset: rows {int(keep.min())} .. {int(keep.max())} outside [0, {len(self)})")
        return torch.from_numpy(keep.astype(np.int64)).to(self.moments.device)

    def draw(self, rows, step, sample=True, random_flip=False, out=None, flipped=None):
        """x0 [B, L, h, w] for dataset rows `rows`: a device int64 tensor (from `subset`: not looked at on the host again, the
        kernel clamps) or host indices (validated, then uploaded)."""
        if not isinstance(rows, torch.Tensor) or not rows.is_cuda:
            rows = self.subset(rows.numpy() if isinstance(rows, torch.Tensor) else rows)
        if random_flip and not self.flips:
            raise _capi.GadError("MomentSource.draw: random_flip needs the flipped encodes, and these moments hold one orientation")
        return ops.latent_draw_raw(self.moments, rows.contiguous(), self.seed, step, self.scaling_factor, sample=sample,
                                   random_flip=random_flip, out=out, flipped=flipped)
