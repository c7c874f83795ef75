"""Torch restatement of the 8-bit blockwise Adam step of csrc/optim8.hip (include/gad.h, gad_clip_adam8_ema) in a chosen dtype -
the pinned truth of the 8-bit optimizer tests.  bitsandbytes 0.42 Adam8bit / AdamW8bit semantics (blockwise, block 2048,
min_8bit_size 4096, no percentile clipping) restated from their published description; bitsandbytes itself is not a dependency.
Also the shared inputs of the CPU and GPU kernel tests (`make_case`).  Test-only; never imported by the product."""
import math

import numpy as np
import torch

BLOCK, MIN_SIZE, SLOT = 2048, 4096, 8


def qmaps(dtype=torch.float32):
    """(signed, unsigned) code maps by the closed form, 256 ascending values each.  The code values ARE fp32 numbers: computed
    in float64 (midpoint k of linspace(0.1, 1, n + 1) = 0.1 + 0.9 (2k + 1) / (2n), divided by the decade), rounded to fp32
    once, and only then cast to `dtype`."""
    def decade(i, n):
        k = torch.arange(n, dtype=torch.float64)
        return (0.1 + (0.9 * (2 * k + 1)) / (2 * n)) / float(10 ** (6 - i))
    pos = torch.cat([decade(i, 2 ** i) for i in range(7)]).to(torch.float32)
    signed = torch.cat([-pos.flip(0), torch.zeros(1), pos, torch.ones(1)])
    unsigned = torch.cat([torch.zeros(1), torch.cat([decade(i, 2 ** (i + 1)) for i in range(7)]).to(torch.float32), torch.ones(1)])
    return signed.to(dtype), unsigned.to(dtype)


def nearest_code(qmap, x):
    """index of the map value nearest to x, the lower index on a tie (qmap ascending)"""
    hi = torch.searchsorted(qmap, x.contiguous()).clamp_(max=qmap.numel() - 1)        # first value >= x
    lo = (hi - 1).clamp_(min=0)
    return torch.where((x - qmap[lo]) <= (qmap[hi] - x), lo, hi)


def adam8_step(state, g, table, *, sumsq, max_norm, lr, betas, eps, step, ema_decay, dtype=torch.float64):
    """One step from `state` (dict of CPU tensors: p, ema or None, state1, state2, absmax1, absmax2, m32, v32 - what the device
    holds) with the flat gradient `g` and the clip scalar `sumsq` (python float, or None for no clipping) over the block `table`
    (gad.training.adam8_blocks(...).table).  Returns the new state; p, ema, absmax and fp32 moments in `dtype`.
    Scalars follow the launch: step size and scaled eps are formed in double and rounded to `dtype`; 1-beta and 1-lr*wd are
    formed in `dtype`."""
    T = lambda x: torch.tensor(x, dtype=dtype)          # noqa: E731
    # the C ABI carries its scalars as fp32: 1 - fp32(0.999) is 1.00005e-3, and that, not 1e-3, is what the launch multiplies by
    f32 = lambda x: float(np.float32(x))                # noqa: E731
    max_norm, lr, betas, eps, ema_decay = f32(max_norm), f32(lr), (f32(betas[0]), f32(betas[1])), f32(eps), f32(ema_decay)
    q1, q2 = qmaps(dtype)
    n = state["p"].numel()
    rows = len(table)
    r_off = torch.from_numpy(table["offset"].astype(np.int64))
    r_len = torch.from_numpy(table["len"].astype(np.int64))
    r_state = torch.from_numpy(table["state"].astype(np.int64))
    r_wd = torch.from_numpy(table["weight_decay"].astype(np.float32)).to(dtype)
    r_32 = torch.from_numpy(table["fp32"].astype(np.int64)).bool()
    b = torch.repeat_interleave(torch.arange(rows), r_len)                   # block row of every active element
    idx = r_off[b] + (torch.arange(b.numel()) - torch.repeat_interleave(r_len.cumsum(0) - r_len, r_len))   # its flat index
    assert idx.numel() == idx.unique().numel() and int(idx.max()) < n
    is32 = r_32[b]
    side = torch.where(is32, r_state[b] + idx - r_off[b], torch.zeros_like(idx))
    slot = torch.where(is32, torch.zeros_like(idx), r_state[b])

    coef = T(1.0)
    if sumsq is not None:
        c = T(max_norm) / (T(sumsq).sqrt() + T(1e-6))
        coef = torch.minimum(c, T(1.0))
    b1, b2 = T(betas[0]), T(betas[1])
    sbc2 = math.sqrt(1.0 - betas[1] ** step)
    step_size, eps_c = T(lr * sbc2 / (1.0 - betas[0] ** step)), T(eps * sbc2)
    gg = g.to(dtype)[idx] * coef
    m = torch.where(is32, state["m32"].to(dtype)[side], q1[state["state1"][idx].long()] * state["absmax1"].to(dtype)[slot])
    v = torch.where(is32, state["v32"].to(dtype)[side], q2[state["state2"][idx].long()] * state["absmax2"].to(dtype)[slot])
    m = m * b1 + (1 - b1) * gg
    v = v * b2 + (1 - b2) * gg * gg
    p = state["p"].to(dtype)[idx]
    p = p - step_size * m / (v.sqrt() + eps_c)
    wd = r_wd[b]
    p = torch.where(wd > 0, p * (1 - T(lr) * wd), p)
    out = {k: (t.clone() if t is not None else None) for k, t in state.items()}
    for k in ("p", "ema", "absmax1", "absmax2", "m32", "v32"):
        if out[k] is not None:
            out[k] = out[k].to(dtype)
    out["p"][idx] = p
    if out["ema"] is not None:
        e = out["ema"][idx]
        out["ema"][idx] = e - (1 - T(ema_decay)) * (e - p)
    out["m32"][side[is32]] = m[is32]
    out["v32"][side[is32]] = v[is32]
    n1 = torch.zeros(rows, dtype=dtype).scatter_reduce_(0, b, m.abs(), "amax", include_self=True)
    n2 = torch.zeros(rows, dtype=dtype).scatter_reduce_(0, b, v, "amax", include_self=True)
    out["absmax1"][r_state[~r_32]] = n1[~r_32]
    out["absmax2"][r_state[~r_32]] = n2[~r_32]
    q = ~is32
    a1, a2 = n1[b], n2[b]
    c1 = nearest_code(q1, torch.where(a1 > 0, m / torch.where(a1 > 0, a1, torch.ones_like(a1)), torch.zeros_like(m)))
    c1 = torch.where((c1 == 127) & (m < 0), torch.full_like(c1, 126), c1)              # a negative moment keeps its sign
    c1 = torch.where(a1 > 0, c1, torch.full_like(c1, 127))                             # absmax 0: the zero code, no division
    c2 = nearest_code(q2, torch.where(a2 > 0, v / torch.where(a2 > 0, a2, torch.ones_like(a2)), torch.zeros_like(v)))
    c2 = torch.where(a2 > 0, c2, torch.zeros_like(c2))
    out["state1"][idx[q]] = c1[q].to(torch.uint8)
    out["state2"][idx[q]] = c2[q].to(torch.uint8)
    return out


def codes_agree(got, want, what, max_fraction=1e-3):
    """codes equal, except that at most `max_fraction` of them may differ by exactly one level -> number that differ"""
    d = (got.to(torch.int16) - want.to(torch.int16)).abs()
    bad = int((d > 0).sum())
    print(f"{what}: {bad} of {d.numel()} codes differ, largest difference {int(d.max()) if d.numel() else 0} levels")
    assert int(d.max()) <= 1, f"{what}: a code is off by {int(d.max())} levels"
    assert bad <= max_fraction * d.numel(), f"{what}: {bad} of {d.numel()} codes differ"
    return bad


# ---- the kernel tests' shared inputs ----------------------------------------------------------------------------------
CASE_SIZES = (8, 4095, 4096, 4097, 3 * 2048 + 777, 4096, 8192)       # [5]: never gets a gradient; [6]: gradient spans logspace(-3, 0)
CASE_NO_DECAY = (True, False, False, True, False, False, False)        # one small and one 8-bit tensor go undecayed
CASE_HP = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, max_norm=1.0, ema_decay=0.9, weight_decay=1e-6)
CASE_SCALES = (1.0, 1e-3, 1.0, 2e-3, 1.0, 1e-3)                         # gradient norm far above 1 (clip active) / below 1 (idle)


def make_case():
    """-> (sizes, p0 [list], grads [step][list]): the parameter set of the 8-bit kernel tests.  Every tensor with a gradient also
    holds a few elements whose gradient is tiny against the block's largest - negative ones, whose first moment must keep
    code 126, and positive ones, which take the zero code."""
    gen = torch.Generator().manual_seed(1234)
    p0 = [torch.randn(n, generator=gen) for n in CASE_SIZES]
    grads = []
    for scale in CASE_SCALES:
        gs = []
        for i, n in enumerate(CASE_SIZES):
            g = torch.randn(n, generator=gen) * scale
            if i == 5:
                g.zero_()
            if i == 6:
                g = g * torch.logspace(-3, 0, n)[torch.randperm(n, generator=gen)]
            if n >= 8 and i != 5:
                g[1::max(2, n // 5)] = -1e-9 * scale
                g[2::max(2, n // 5)] = 1e-9 * scale
            gs.append(g)
        grads.append(gs)
    return CASE_SIZES, p0, grads


def case_state(layout, sizes, p0):
    """the kernel tests' initial CPU state over the flat layout: parameters at their slots, EMA beside them, zero moments"""
    n = sum((s + SLOT - 1) // SLOT * SLOT for s in sizes)
    p = torch.zeros(n)
    for (_, off, cnt, _, _), t in zip(layout.params, p0):
        p[off:off + cnt] = t
    return dict(p=p, ema=p * 0.5, state1=torch.full((n,), 127, dtype=torch.uint8), state2=torch.zeros(n, dtype=torch.uint8),
                absmax1=torch.zeros(layout.n_absmax), absmax2=torch.zeros(layout.n_absmax),
                m32=torch.zeros(layout.n32), v32=torch.zeros(layout.n32))


def flat_grad(layout, n, gs):
    g = torch.zeros(n)
    for (_, off, cnt, _, _), t in zip(layout.params, gs):
        g[off:off + cnt] = t
    return g
