"""CLIP's byte-pair tokenizer on the host (reference: `clip.tokenize` at text_to_image/compute_model_behaviors.py:302-306 and
`CLIPTokenizer` at train_text_to_image_lora.py:723-731 - one vocabulary, two padding conventions).  Nothing is bundled: the
vocabulary is a file the user supplies.

Accepted:
  * OpenAI's merges file (`bpe_simple_vocab_16e6.txt` or `.txt.gz`; the first line is a header).  The vocabulary is built the
    published way: the 256 `bytes_to_unicode` symbols, the same with `</w>`, one entry per merge, `<|startoftext|>`,
    `<|endoftext|>`.  Of the real file the first 48 894 merges count (49 408 ids); a shorter file gives all its merges.
  * a directory with `vocab.json` + `merges.txt` (the HF layout): ids come from vocab.json.

Text goes through html.unescape twice, whitespace collapse, strip and lower-casing, is split by the published pattern (the
`regex` module: it needs \\p{L} / \\p{N}), and each piece is encoded bytes -> byte symbols -> greedy lowest-rank merges with
`</w>` on the last symbol.  `ftfy.fix_text` runs first when `ftfy` imports and is SKIPPED otherwise: ASCII prompts (all of
ArtBench's) do not need it, and only ASCII prompts have been verified; text that ftfy would repair (mojibake, odd quotes) may
tokenise differently from the reference without it."""
from __future__ import annotations

import gzip
import html
import json
import os

import numpy as np

CONTEXT = 77
OPENAI_MERGES = 49152 - 256 - 2
SOT, EOT = "<|startoftext|>", "<|endoftext|>"
PATTERN = r"<\|startoftext\|>|<\|endoftext\|>|'s|'t|'re|'ve|'m|'ll|'d|[\p{L}]+|[\p{N}]|[^\s\p{L}\p{N}]+"


def bytes_to_unicode():
    """byte -> printable symbol, the published table: the printable Latin-1 bytes stand for themselves (in the order '!'..'~',
    '¡'..'¬', '®'..'ÿ'), the other 68 take code points from 256 on"""
    bs = list(range(ord("!"), ord("~") + 1)) + list(range(ord("¡"), ord("¬") + 1)) + list(range(ord("®"), ord("ÿ") + 1))
    cs = bs[:]
    n = 0
    for b in range(256):
        if b not in bs:
            bs.append(b)
            cs.append(256 + n)
            n += 1
    return dict(zip(bs, (chr(c) for c in cs)))


def _read_merges(path):
    opener = gzip.open if path.endswith(".gz") else open
    with opener(path, "rt", encoding="utf-8") as f:
        lines = f.read().split("\n")[1:]                       # the first line is a header
    merges = [tuple(line.split()) for line in lines if line.strip()]
    for m in merges:
        if len(m) != 2:
            raise ValueError(f"ClipBPE: {path}: a merge line must hold two symbols, got {' '.join(m)!r}")
    return merges


class ClipBPE:
    def __init__(self, path):
        try:
            import regex
        except ImportError as e:                                # pragma: no cover - the module is a stated requirement
            raise ImportError("ClipBPE needs the `regex` module (the published split pattern uses \\p{L} and \\p{N})") from e
        self.path = path
        self.byte_encoder = bytes_to_unicode()
        if os.path.isdir(path):
            for name in ("vocab.json", "merges.txt"):
                if not os.path.exists(os.path.join(path, name)):
                    raise FileNotFoundError(f"ClipBPE: {path} is a directory without {name}")
            with open(os.path.join(path, "vocab.json"), encoding="utf-8") as f:
                self.encoder = {k: int(v) for k, v in json.load(f).items()}
            merges = _read_merges(os.path.join(path, "merges.txt"))
        else:
            merges = _read_merges(path)[:OPENAI_MERGES]
            symbols = list(self.byte_encoder.values())
            vocab = symbols + [s + "</w>" for s in symbols] + ["".join(m) for m in merges] + [SOT, EOT]
            self.encoder = {s: i for i, s in enumerate(vocab)}
        for t in (SOT, EOT):
            if t not in self.encoder:
                raise ValueError(f"ClipBPE: {path}: the vocabulary has no {t}")
        self.ranks = {m: i for i, m in enumerate(merges)}
        self.sot, self.eot = self.encoder[SOT], self.encoder[EOT]
        self.vocab_size = max(self.encoder.values()) + 1
        self.cache = {SOT: SOT, EOT: EOT}
        self.pat = regex.compile(PATTERN, regex.IGNORECASE)
        try:
            import ftfy
            self._fix = ftfy.fix_text
        except ImportError:
            self._fix = None

    def clean(self, text):
        if self._fix is not None:
            text = self._fix(text)
        text = html.unescape(html.unescape(text))
        return " ".join(text.split()).strip().lower()

    def bpe(self, token):
        """symbols of one piece after the merges, joined by spaces"""
        if token in self.cache:
            return self.cache[token]
        word = tuple(token[:-1]) + (token[-1] + "</w>",)
        while len(word) > 1:
            pairs = set(zip(word[:-1], word[1:]))
            best = min(pairs, key=lambda p: self.ranks.get(p, float("inf")))
            if best not in self.ranks:
                break
            first, second = best
            merged, i = [], 0
            while i < len(word):
                if i + 1 < len(word) and word[i] == first and word[i + 1] == second:
                    merged.append(first + second)
                    i += 2
                else:
                    merged.append(word[i])
                    i += 1
            word = tuple(merged)
        out = " ".join(word)
        self.cache[token] = out
        return out

    def pieces(self, text):
        """ids of the text alone: no start, end or padding"""
        ids = []
        for token in self.pat.findall(self.clean(text)):
            token = "".join(self.byte_encoder[b] for b in token.encode("utf-8"))
            for s in self.bpe(token).split(" "):
                if s not in self.encoder:
                    raise KeyError(f"ClipBPE: {self.path}: the vocabulary has no symbol {s!r}")
                ids.append(self.encoder[s])
        return ids

    def encode(self, text, context=CONTEXT, pad="eot"):
        """int32 [context]: start + pieces + end, truncated so that the end token stays last, then padded with the end token
        (pad="eot": SD's CLIPTokenizer) or with 0 (pad="zero": clip.tokenize)"""
        if pad not in ("eot", "zero"):
            raise ValueError(f"ClipBPE.encode: pad={pad!r}: use 'eot' or 'zero'")
        if context < 2:
            raise ValueError(f"ClipBPE.encode: context={context} has no room for the start and end tokens")
        ids = [self.sot] + self.pieces(text)[:context - 2] + [self.eot]
        out = np.full((context,), self.eot if pad == "eot" else 0, dtype=np.int32)
        out[:len(ids)] = ids
        return out

    def encode_batch(self, texts, context=CONTEXT, pad="eot"):
        return np.stack([self.encode(t, context, pad) for t in texts])
