"""Derived copies of weights (bf16 casts, rotated 3x3 weights, Winograd forms, bf16 LoRA pairs) and the one rule that keeps
them fresh.  A stale copy does not crash - it trains or samples with old weights.  Weights change through torch (a version
counter moves) or behind its back, through a device pointer or `.data`; whoever does the latter says so with `written(buf)`
or `written_everywhere()`.  `stamp(t)` is everything that moves when `t` may have changed.  A `Shadow` of a flat buffer
(training.flatten_params) is fresh for a resident while the buffer's stamp and that resident's version are those of its
last refresh; a weight outside a buffer keeps what is derived from it under `weight_key` (`cached`).
Pure Python and torch: the owners (gad/ops.py, gad/half.py) supply the launches."""
from __future__ import annotations

from collections import namedtuple

Cached = namedtuple("Cached", "key value")       # what `cached` keeps on a weight
WEIGHT_EPOCH = [0]           # rare events that rewrite arbitrary parameters behind torch's back (EMA copy_to / restore ...)


def written(buf):
    """`buf` - a flat parameter buffer, or a shadow that further shadows derive from - was rewritten through a device pointer"""
    buf._gad_epoch = getattr(buf, "_gad_epoch", 0) + 1


def written_everywhere():
    """parameters were rewritten where no version counter moves and no one buffer can be named (`p.data.copy_`, a flat copy)"""
    WEIGHT_EPOCH[0] += 1


def stamp(t):
    """(torch's version counter, the global epoch, the epoch of the buffer that `t` is or - as a resident - lives in)"""
    home = getattr(t, "_gad_flat", None)
    return (t._version, WEIGHT_EPOCH[0], getattr(t if home is None else home[0], "_gad_epoch", 0))


def weight_key(w):
    """Cache key of anything derived from parameter `w`: its address and its stamp (spelled out: the samplers and the half path ask
    per layer and step; tests/test_shadows_cpu.py holds the two together).  Frozen parameters outside a flat buffer (the SD base
    U-Net under LoRA) therefore keep their derived copies across the optimizer steps that bump the buffer's epoch."""
    home = getattr(w, "_gad_flat", None)
    return (w.data_ptr(), w._version, WEIGHT_EPOCH[0], getattr(w if home is None else home[0], "_gad_epoch", 0))


def in_flat_buffer(w) -> bool:
    home = getattr(w, "_gad_flat", None)
    return home is not None and w.data_ptr() == home[0].data_ptr() + 4 * home[1]


class Shadow:
    """One derived copy of a whole buffer, allocated once and rewritten in place by `refresh(home)`, the owner's one launch:
    `buffers` (the bf16 pairs have two), `where` {source offset: (offset in the copy, floats)} for the Winograd forms, `views`
    the owner hands out per offset; `stamp` and `versions` {offset: resident version} as of the last refresh."""
    __slots__ = ("buffers", "refresh", "where", "views", "stamp", "versions")

    def __init__(self, buffers, refresh, where=None):
        self.buffers, self.refresh, self.where = tuple(buffers), refresh, where
        self.views, self.stamp, self.versions = {}, None, {}

    def fresh_for(self, home, off=None, w=None):
        """Bring the shadow of `home` up to date for its resident `w` at `off` (without one: for the buffer as stamped).  A resident
        written through torch (load_state_dict, p.copy_(), a torch.optim step) moves only ITS version counter, not the
        buffer's - the second test; the one refresh then covers every resident."""
        now = stamp(home)
        if self.stamp != now or (w is not None and self.versions.get(off, w._version) != w._version):
            self.refresh(home)
            self.stamp = now
            self.versions = {o_: p_._version for p_, o_, _ in getattr(home, "_gad_params", ())}
        return self


def cached(w, attr, make, fill=None):
    """What is derived from weight `w` and kept on it under `attr` (as .key, .value), valid while `weight_key(w)` stands.  Without
    `fill` a stale value is re-made by `make()`; with it, `make()` only allocates - once - and `fill(value)` writes, the first time
    and after every change, so the address never moves (captured graphs read the Winograd forms at theirs)."""
    key = weight_key(w)
    c = getattr(w, attr, None)
    if c is None or c.key != key:
        c = Cached(key, make() if c is None or fill is None else c.value)
        if fill is not None:
            fill(c.value)
        setattr(w, attr, c)
    return c.value
