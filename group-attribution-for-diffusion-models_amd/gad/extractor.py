"""What the pretrained eval-only networks (gad/inception.py, gad/vgg.py, gad/vit.py, gad/text.py, gad/vae.py) share on the host:
the digest and tag of a weight file, reading it, refusing a state dict by key, and the class that carries weights, tag and the
chunked forward.  The launches themselves are the `*_raw` wrappers of gad/ops.py."""
from __future__ import annotations

import hashlib
import os

import torch

from . import _capi


def file_digest(path):
    """first 12 hex digits of the file's sha256: what a row's tag says about the weights behind it"""
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()[:12]


def file_tag(kind, path, basename=True):
    """`<kind>:<basename>:<digest>`, or `<kind>:<digest>`.  Tags are written into database rows: they stay as they are."""
    return f"{kind}:{os.path.basename(path)}:{file_digest(path)}" if basename else f"{kind}:{file_digest(path)}"


def load_checkpoint(path, torchscript=False):
    """A state dict from a plain checkpoint (tensors only); `torchscript`: also from a TorchScript archive (OpenAI's CLIP `.pt`
    files are JIT archives) or from under a `"state_dict"` key."""
    if not torchscript:
        return torch.load(path, map_location="cpu", weights_only=True)
    try:
        sd = torch.load(path, map_location="cpu", weights_only=True)
    except Exception:
        sd = torch.jit.load(path, map_location="cpu").state_dict()
    if isinstance(sd, dict) and "state_dict" in sd and isinstance(sd["state_dict"], dict):
        sd = sd["state_dict"]
    return sd


def check_state_dict(owner, sd, want, prefix="", extra=None):
    """Refuse `sd` by name unless it holds every key of `want` ({key: shape}, looked up under `prefix`) at that shape.
    `extra`: None ignores the other keys; a predicate refuses those it does not accept."""
    if extra is not None:
        for k in sd:
            if k not in want and not extra(k):
                raise KeyError(f"{owner}: unexpected key {k!r}")
    for k, shape in want.items():
        if prefix + k not in sd:
            raise KeyError(f"{owner}: missing key {prefix + k!r}")
        if tuple(sd[prefix + k].shape) != shape:
            raise ValueError(f"{owner}: {prefix + k!r} has shape {tuple(sd[prefix + k].shape)}, expected {shape}")


def _to(v, device):
    if isinstance(v, torch.Tensor):
        return v.to(device)
    if isinstance(v, tuple):
        return tuple(_to(t, device) for t in v)
    return {k: _to(t, device) for k, t in v.items()}


class Extractor:
    """A network whose weights sit in `w` and whose batch goes through in passes of at most `max_batch` items.  A subclass sets
    `owner` (the name its refusals carry), `max_batch`, `tag`, and fills `w` (tensors, tuples and dicts of them) in
    `load_state_dict`.  An image network ([B,3,H,W] in [0,1] -> features [B, `dims`]) runs one chunk in `_chunk` and inherits
    `forward`; one with other inputs or several entry points (the text towers, the autoencoders) calls `_chunked` itself."""

    owner = dims = max_batch = None

    def __init__(self, tag, state_dict=None):
        self.tag, self.w = tag, {}
        if state_dict is not None:
            self.load_state_dict(state_dict)

    def to(self, device):
        self.w = _to(self.w, device)
        return self

    def _chunked(self, fn, batch):
        """`fn` on at most `max_batch` items of `batch` at a time -> the results along dim 0; refused without weights"""
        if not self.w:
            raise _capi.GadError(f"{self.owner}: no weights loaded")
        outs = [fn(batch[s:s + self.max_batch]) for s in range(0, len(batch), self.max_batch)]
        return outs[0] if len(outs) == 1 else torch.cat(outs, 0)

    @torch.no_grad()
    def forward(self, images_nchw01):
        return self._chunked(self._chunk, images_nchw01)

    def __call__(self, images_nchw01):
        return self.forward(images_nchw01)
