"""The launches of the convolution suites (tests/test_conv_cases_cpu.py proves the cases on the CPU,
tests/test_gpu_conv_exact.py and tests/test_gpu_conv_conditioning.py run them on gad_gemm's gather side: A_CONV, A_CONVT,
B_WDGRAD, B_CONV, the Winograd transforms and the epilogues behind them).  Nothing here needs a GPU.

Integer cases.  x and dy in [-4, 4], w in [-2, 2], bias / rowadd / residual in [-8, 8]: every product, partial sum, split-K
slab and epilogue value is an integer far below 2^24 (K <= 9 * 256, at most 2^17 pixels in a weight gradient), so fp32
computes it exactly in any order, under any split, and bf16 rounding of the operands changes nothing: the tests compare with
torch.equal against fp64.  For Winograd F(2x2, 3x3) w is drawn from 4 * {-2..2}: G w G^T divides by 4 and B^T d B, A^T M A only
add, so that route is exact as well.  F(4x4) has 1/6 and 1/24 in G and gets no integer case.

Layout (as tests/gemm_cases.py).  Every tensor sits in a flat buffer with LEAD floats before it and SLACK floats after it:
NaN around operands - a tap that multiplies padding instead of masking it poisons its output - and the finite SENTINEL
around and inside outputs, which must be unchanged outside the addressed elements.  Two layouts: "aligned" (everything on
the 16-byte grid) and "off1" (the output, bias, rowadd and residual one float off it: the scalar epilogue).  gad_gemm refuses
an A or B off the grid (`REFUSALS`), so the dword gathers (pick_vec 1) are reached the way the ABI reaches them: C % 4 != 0 or
ldx % 4 != 0.

Conditioning cases.  For the routes that are not exact - F(4x4) forward in its four forms, the F(4x4) weight gradient - and
the direct routes as the baseline, on the inputs the network feeds (post-GroupNorm SiLU activations, a hot channel, one
large pixel ...).  References and bound as in tests/norm_cases.py: `want` is fp64 of the stored fp32 values, `e_ref` the
max-norm error of an fp32 CPU computation of the SAME algorithm (F.conv2d / autograd for the direct routes; the torch
emulations below of the standard F(2x2) / F(4x4) transforms for the Winograd routes), and a result is accepted when

    max |got - want|  <=  K * max(e_ref, 2^-22 * max |want|),      K = 8   (norm_cases.K, not tuned here)."""
import ctypes
from dataclasses import dataclass, replace

import torch
import torch.nn.functional as F

from norm_cases import FLOOR, K  # noqa: F401  (the project's constants)

SENTINEL = -12345.75
LEAD = 8                       # floats before every tensor in its flat buffer ("off1": LEAD + 1 for the epilogue tensors)
SLACK = 8                      # floats after it
LAYOUTS = ("aligned", "off1")
P1 = (1, 1, 1, 1)
P0 = (0, 0, 0, 0)


@dataclass(frozen=True)
class Row:
    """One convolution.  `entry`: fwd = ops.conv2d_fwd_raw (and conv2d_dgrad_raw / conv2d_wgrad_raw / colsum_raw for the
    directions in `dirs`), krsc = ops.conv_krsc_raw into channels [c0, c0 + Cout) of a [.., ctot] output, direct =
    ops.conv_direct_raw, ldx = ops.gemm_raw with an explicit ConvGeom whose pixel stride is Cin + ldx_pad.
    `c1` > 0: two sources, cat([x[:, :c1], x[:, c1:]]).  `claims`: {direction: (kernel id, tile or None)} that
    gad_gemm_kernel_id / gad_gemm_plan must report at the row's own (`hint`, `flags`, `prec`), aligned layout, no epilogue -
    and with the full one where `claim_full`.  `wgrad_hints`: further tile hints of the weight gradient, {hint: (id, tile)}."""
    label: str
    B: int
    Cin: int
    Cout: int
    H: int
    W: int
    KH: int
    KW: int
    stride: int
    pad: tuple
    ups: bool = False
    entry: str = "fwd"
    c1: int = 0
    c0: int = 0
    ctot: int = 0
    ldx_pad: int = 0
    dirs: tuple = ("fwd", "dgrad", "wgrad")
    hint: int = 0
    flags: tuple = ()
    prec: str = "f32"
    claims: tuple = (("fwd", (0, None)),)
    claim_full: bool = True
    wgrad_hints: tuple = ()
    wscale: int = 1
    layouts: tuple = LAYOUTS
    seed: int = 0

    @property
    def He(self):
        return 2 * self.H if self.ups else self.H

    @property
    def We(self):
        return 2 * self.W if self.ups else self.W

    @property
    def Ho(self):
        return (self.He + self.pad[0] + self.pad[1] - self.KH) // self.stride + 1

    @property
    def Wo(self):
        return (self.We + self.pad[2] + self.pad[3] - self.KW) // self.stride + 1

    @property
    def epilogues(self):
        """what the entry point can pass: (name, has bias, has rowadd, has residual)"""
        return {"fwd": (("none", 0, 0, 0), ("full", 1, 1, 1)), "ldx": (("none", 0, 0, 0), ("full", 1, 1, 1)),
                "krsc": (("none", 0, 0, 0), ("full", 1, 0, 0)), "direct": (("none", 0, 0, 0), ("full", 1, 0, 1))}[self.entry]


def _r(label, B, Cin, Cout, H, W, KH, KW, stride, pad, ups=False, **kw):
    return Row(label, B, Cin, Cout, H, W, KH, KW, stride, tuple(pad), bool(ups), **kw)


ENGINE3 = (("fwd", (0, None)), ("dgrad", (0, None)), ("wgrad", (0, None)))
FWD = ("fwd",)

# ---- the edge table: B, Cin, Cout, H, W, KH, KW, stride, pad (t, b, l, r), upsample - a few thousand output pixels at most ----
EDGE_ROWS = [
    _r("ragged-everything", 3, 5, 7, 7, 5, 3, 3, 1, P1, claims=ENGINE3),                       # M = 105, scalar gather; dgrad refused (Cin % 4)
    _r("cin3-cout128", 2, 3, 128, 6, 5, 3, 3, 1, P1, claims=ENGINE3),
    _r("cout1", 2, 8, 1, 6, 5, 3, 3, 1, P1, claims=ENGINE3),
    _r("cout3", 2, 8, 3, 6, 5, 3, 3, 1, P1, claims=ENGINE3),
    _r("cout4", 2, 8, 4, 6, 5, 3, 3, 1, P1, claims=ENGINE3),
    _r("m15", 1, 8, 12, 3, 5, 3, 3, 1, P1, claims=ENGINE3),                                     # M < 64
    _r("down-asym-pad", 2, 36, 68, 9, 6, 3, 3, 2, (0, 1, 0, 1), claims=ENGINE3),                # Downsample2D: F.pad(0, 1, 0, 1)
    _r("down-pad1", 2, 36, 68, 9, 6, 3, 3, 2, P1, claims=ENGINE3),
    _r("upsample-odd-map", 2, 32, 40, 5, 3, 3, 3, 1, P1, True, claims=ENGINE3),
    _r("1x1", 2, 32, 40, 6, 10, 1, 1, 1, P0, claims=ENGINE3),                                   # dense loaders; general_loaders: the gather
    _r("1x1-two-source-32+64", 2, 96, 40, 6, 10, 1, 1, 1, P0, c1=32, dirs=FWD),
    _r("1x1-two-source-96+32", 2, 128, 40, 6, 10, 1, 1, 1, P0, c1=96, dirs=FWD),
    _r("3x3-two-source-32+64", 2, 96, 40, 6, 5, 3, 3, 1, P1, c1=32, dirs=FWD),
    _r("3x3-two-source-96+32", 2, 128, 40, 6, 5, 3, 3, 1, P1, c1=96, dirs=FWD),
]
# the score-tail forms through conv_krsc_raw, each into channels [c0, c0 + 24) of a 48-channel output: c0 = 20 with Cin = 20
# (float4 gather, float4 epilogue), c0 = 21 with Cin = 18 (dword gather, scalar epilogue)
for _name, _kh, _kw, _s, _ph, _pw, _h in (("1x7", 1, 7, 1, 0, 3, 9), ("7x1", 7, 1, 1, 3, 0, 9), ("1x3", 1, 3, 1, 0, 1, 9),
                                          ("3x1", 3, 1, 1, 1, 0, 9), ("5x5", 5, 5, 1, 2, 2, 9), ("3x3s2p0", 3, 3, 2, 0, 0, 15)):
    for _c0, _ci in ((20, 20), (21, 18)):
        EDGE_ROWS.append(_r(f"krsc-{_name}-c0={_c0}", 2, _ci, 24, _h, _h - 2 if _s == 1 else _h, _kh, _kw, _s, (_ph, _ph, _pw, _pw),
                            entry="krsc", c0=_c0, ctot=48, dirs=FWD, layouts=("aligned",)))
# ... and the autoencoders' through conv_direct_raw
EDGE_ROWS += [
    _r("direct-3x3s2-asym-pad", 2, 36, 68, 9, 6, 3, 3, 2, (0, 1, 0, 1), entry="direct", dirs=FWD, layouts=("aligned",)),
    _r("direct-3x3s2p0", 2, 20, 24, 15, 15, 3, 3, 2, P0, entry="direct", dirs=FWD, layouts=("aligned",)),
    _r("direct-5x5", 2, 18, 24, 9, 7, 5, 5, 1, (2, 2, 2, 2), entry="direct", dirs=FWD, layouts=("aligned",)),
    _r("direct-upsample", 2, 32, 40, 5, 3, 3, 3, 1, P1, True, entry="direct", dirs=FWD, layouts=("aligned",)),
    # ldx > C: channels [0, C) of pixels C + 4 / C + 1 floats apart, the gap channels NaN
    _r("ldx+4-3x3", 2, 32, 40, 6, 5, 3, 3, 1, P1, entry="ldx", ldx_pad=4, dirs=FWD),
    _r("ldx+1-3x3", 2, 32, 40, 6, 5, 3, 3, 1, P1, entry="ldx", ldx_pad=1, dirs=FWD),
    _r("ldx+4-1x1", 2, 32, 40, 6, 10, 1, 1, 1, P0, entry="ldx", ldx_pad=4, dirs=FWD),
    _r("ldx+1-1x1", 2, 32, 40, 6, 10, 1, 1, 1, P0, entry="ldx", ldx_pad=1, dirs=FWD),
    _r("ldx+4-3x3-s2", 2, 36, 68, 9, 6, 3, 3, 2, (0, 1, 0, 1), entry="ldx", ldx_pad=4, dirs=FWD),
    _r("ldx+4-wino2", 2, 32, 64, 6, 10, 3, 3, 1, P1, entry="ldx", ldx_pad=4, dirs=FWD, hint=7, wscale=4,
       claims=(("fwd", (5, 128)),), layouts=("aligned",)),
    _r("ldx+4-patch-bf16", 2, 32, 68, 8, 16, 3, 3, 1, P1, entry="ldx", ldx_pad=4, dirs=FWD, prec="bf16",
       claims=(("fwd", (3, 128)),), layouts=("aligned",)),
]

# ---- one launch per route, the smallest its own predicate admits (csrc/gemm_f32.hip) ----
ROUTE_ROWS = [
    # use_patch_conv_f32: whole 128-pixel row tiles and >= 192 workgroups.  48 x 2 tiles x a 2-way split of the four 32-channel
    # chunks (forward, 96-wide tiles: 48 x 3 x 2); hint 1 keeps the Winograd routes out.  Data gradient: 48 tiles x 4 of 8 chunks
    _r("route-patch-f32", 48, 128, 256, 8, 16, 3, 3, 1, P1, hint=1, layouts=("aligned",),
       claims=(("fwd", (2, 96)), ("dgrad", (2, 128)), ("wgrad", (2, 128)))),
    # use_patch_conv (bf16 operands): the same geometry, no block minimum
    _r("route-patch-bf16", 2, 32, 68, 8, 16, 3, 3, 1, P1, prec="bf16", dirs=FWD, claims=(("fwd", (3, 128)),)),
    # use_fewout_conv: <= 4 output channels, whole 256-pixel row tiles, no rowadd / residual
    _r("route-fewout", 1, 32, 3, 16, 16, 3, 3, 1, P1, dirs=FWD, claims=(("fwd", (4, 256)),), claim_full=False),
    # wgrad_patch_splits: 8-wide maps, Cin and Cout multiples of 32; tiles of 128 / 96 / 64 / 32 channels by hints 1 / 4 / 5 / 6
    _r("route-wgrad-patch", 3, 64, 96, 8, 8, 3, 3, 1, P1, hint=1, dirs=("wgrad",), claims=(("wgrad", (2, 128)),),
       wgrad_hints=((4, (2, 96)), (5, (2, 64)), (6, (2, 32)))),
    # wgrad_split_m, forced: rows [0, 128) on 128-channel tiles, the other 32 planned
    _r("route-split-m", 2, 32, 160, 8, 8, 3, 3, 1, P1, hint=1128, dirs=("wgrad",), claims=(("wgrad", (2, 224)),)),
    # patch_split_n: 224 = 128 + 96 columns where two exact launches beat every padded one: 342 row tiles make 128-wide tiles two
    # rounds of 512 workgroups and 96-wide ones three, the halves one round each.  The Winograd routes (the default here) off.
    _r("route-split-n", 342, 32, 224, 8, 16, 3, 3, 1, P1, flags=("no_wino",), dirs=FWD, claims=(("fwd", (2, 224)),),
       layouts=("aligned",)),
    # use_wino, F(2x2) (hint 7): 64 tiles x 128 channels unless 128 x 64 takes fewer rounds of 256 blocks - 65 x 17 x 15 = 16575
    # tiles of a 34 x 30 map (odd tile counts) do
    _r("route-wino2-128x64", 65, 32, 64, 34, 30, 3, 3, 1, P1, hint=7, wscale=4, dirs=FWD, claims=(("fwd", (5, 64)),),
       layouts=("aligned",)),
    _r("route-wino2-cout68", 2, 32, 68, 34, 30, 3, 3, 1, P1, hint=7, wscale=4, dirs=FWD, claims=(("fwd", (5, 128)),)),
    _r("route-wino2-upsample", 2, 32, 64, 5, 3, 3, 3, 1, P1, True, hint=7, wscale=4, dirs=FWD, claims=(("fwd", (5, 128)),)),
    # the generic engine on bf16 operands
    _r("route-engine-bf16", 2, 36, 68, 9, 6, 3, 3, 2, (0, 1, 0, 1), prec="bf16", dirs=FWD, claims=(("fwd", (1, None)),)),
]
INTEGER_ROWS = EDGE_ROWS + ROUTE_ROWS
ROWS = {r.label: r for r in INTEGER_ROWS}
assert len(ROWS) == len(INTEGER_ROWS)

# what the ABI refuses, and the words of its message
REFUSALS = {"dgrad-cin%4": "B_WDGRAD needs N%4==0", "x-off-grid": "A/B must be 16-byte aligned"}

# ---- variants: every case runs under all of these and must give the same bits ----
TILE_HINTS = (0, 1, 2)
SPLIT_HINTS = (0, 2, 3)
FLAG_SETS = ((), ("tap_major_k",), ("scalar_epilogue",), ("no_patch",), ("general_loaders",))
PRECISIONS = ("f32", "bf16")


def variants(row, direction="fwd"):
    """[(tile_hint, splitk_hint, flags, precision)]: the row's own launch first, then the full cross (the entry points of
    the score-tail / autoencoder launches take no hints and force fp32 products: flags x precisions)."""
    own = (row.hint, 0, row.flags, row.prec)
    if row.entry in ("krsc", "direct"):
        out = [(0, 0, f, p) for f in FLAG_SETS for p in PRECISIONS]
    else:
        out = [own] + [(t, s, f, p) for t in TILE_HINTS for s in SPLIT_HINTS for f in FLAG_SETS for p in PRECISIONS]
        if direction == "wgrad":
            out += [(h, 0, (), "f32") for h, _ in row.wgrad_hints]
    return list(dict.fromkeys(out))


# --------------------------------------------------------------------------------------------------- operands ----
def _ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def draw(row):
    """The logical fp64 tensors of an integer case, NCHW: x, w, bias [Cout], rowadd [B, Cout], residual and dy [B, Cout, Ho, Wo]"""
    g = torch.Generator().manual_seed(1000 + row.seed + sum(ord(c) for c in row.label))
    return dict(x=_ints(g, -4, 4, row.B, row.Cin, row.H, row.W), w=row.wscale * _ints(g, -2, 2, row.Cout, row.Cin, row.KH, row.KW),
                bias=_ints(g, -8, 8, row.Cout), rowadd=_ints(g, -8, 8, row.B, row.Cout),
                residual=_ints(g, -8, 8, row.B, row.Cout, row.Ho, row.Wo), dy=_ints(g, -4, 4, row.B, row.Cout, row.Ho, row.Wo))


def conv_ref(x, w, stride=1, pad=P1, ups=False):
    """torch's direct convolution in the dtype of x (NCHW); pad = (top, bottom, left, right)"""
    if ups:
        x = F.interpolate(x, scale_factor=2.0, mode="nearest")
    return F.conv2d(F.pad(x, (pad[2], pad[3], pad[0], pad[1])), w, stride=stride)


def forward(row, t, epilogue, dtype=torch.float64, conv=None):
    """y [B, Cout, Ho, Wo] in `dtype`; epilogue = (bias?, rowadd?, residual?); conv: another way to convolve (an emulation)"""
    x, w = t["x"].to(dtype), t["w"].to(dtype)
    y = conv(x, w) if conv is not None else conv_ref(x, w, row.stride, row.pad, row.ups)
    if epilogue[0]:
        y = y + t["bias"].to(dtype)[None, :, None, None]
    if epilogue[1]:
        y = y + t["rowadd"].to(dtype)[:, :, None, None]
    if epilogue[2]:
        y = y + t["residual"].to(dtype)
    return y


def gradients(row, t, dtype=torch.float64):
    """autograd in `dtype` -> dx [B, Cin, H, W], dw [Cout, Cin, KH, KW], dbias [Cout] (= the column sums of dy)"""
    x, w = (t[k].detach().to(dtype, copy=True).requires_grad_(True) for k in ("x", "w"))
    b = torch.zeros(row.Cout, dtype=dtype, requires_grad=True)
    (conv_ref(x, w, row.stride, row.pad, row.ups) + b[None, :, None, None]).backward(t["dy"].to(dtype))
    return dict(dx=x.grad, dw=w.grad, dbias=b.grad)


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def flat(values, lead=LEAD, fill=float("nan"), slack=SLACK):
    """contiguous `values` in a flat buffer of its dtype: `lead` floats of `fill`, the values, `slack` floats of `fill`"""
    buf = torch.full((lead + values.numel() + slack,), fill, dtype=values.dtype)
    buf[lead:lead + values.numel()] = values.reshape(-1)
    return buf


def pad_pixels(x_nhwc, ldx, fill=float("nan")):
    """[B, H, W, C] -> [B, H, W, ldx] with the gap channels `fill`"""
    out = torch.full((*x_nhwc.shape[:3], ldx), fill, dtype=x_nhwc.dtype)
    out[..., :x_nhwc.shape[-1]] = x_nhwc
    return out


# ------------------------------------------------------------------------------------- the host's plan, on the CPU ----
_P = 1 << 24                          # placeholder addresses: the queries read only their 16-byte alignment
_FLAG_BITS = dict(no_patch=1, tap_major_k=2, scalar_epilogue=4, general_loaders=8, no_wino=16)


def flag_bits(flags):
    return sum(_FLAG_BITS[f] for f in flags)


def _wino_weight_exists(co, ci, kh, kw, prec, bits):
    """ops.wino_weight: which weights get a Winograd form at all"""
    return (kh, kw) == (3, 3) and ci % 32 == 0 and co % 4 == 0 and co >= 64 and prec == "f32" and not bits & (16 | 1 | 4 | 2)


def plan_args(row, direction="fwd", hint=None, splitk=0, flags=None, prec=None, epilogue=(0, 0, 0), layout="aligned",
              as_forward=False, no_wino4=True):
    """The gad_gemm_args that the entry point of `row` builds for `direction` (fwd, dgrad, wgrad), on placeholder pointers: what
    gad_gemm_kernel_id / gad_gemm_plan are asked on the CPU.  The GPU tests assert that every real launch reports the same
    kernel id.  as_forward: the data gradient as ops._conv_backward runs it where ops.dgrad_as_forward holds - the forward
    convolution of dy with the rotated weight (hint 0).  no_wino4: under ops.kernel_flags(no_wino4=True), as every integer
    launch runs - F(4x4) is not exact; where the host would offer it, it offers F(2x2), which is (U = G w G^T is a multiple of 1/4)."""
    from gad import _capi as c
    hint = row.hint if hint is None else hint
    flags = row.flags if flags is None else flags
    prec = row.prec if prec is None else prec
    bits = flag_bits(flags)
    a = c.GemmArgs()
    a.A = a.B = a.C = _P
    a.alpha, a.tile_hint, a.splitk_hint, a.flags = 1.0, hint, splitk, bits
    a.operand_precision = 1 if (prec == "bf16" and row.entry not in ("krsc", "direct")) else 0
    B, Ci, Co, H, W, KH, KW, s, pad = row.B, row.Cin, row.Cout, row.H, row.W, row.KH, row.KW, row.stride, row.pad
    Ho, Wo, He, We = row.Ho, row.Wo, row.He, row.We
    off = 4 if layout == "off1" else 0
    one_by_one = (KH == 1 and KW == 1 and s == 1 and pad == P0 and not row.ups and Ci % 4 == 0 and Co % 4 == 0 and not bits & 8)
    if direction == "dgrad" and as_forward:
        fwd = replace(row, Cin=Co, Cout=Ci, H=He, W=We, ups=False, hint=0, entry="fwd", c1=0)
        return plan_args(fwd, "fwd", 0, 0, flags, prec, no_wino4=no_wino4)
    if direction == "fwd":
        a.a_mode, a.b_mode, a.M, a.N, a.K = c.A_CONV, c.B_KC, B * Ho * Wo, Co, KH * KW * Ci
        a.lda, a.ldb, a.ldc = 0, KH * KW * Ci, (row.ctot if row.entry == "krsc" else Co)
        a.g = c.ConvGeom(H, W, Ci, (row.c1 or Ci) + row.ldx_pad, Ho, Wo, KH, KW, s, pad[0], pad[2], int(row.ups))
        a.C = _P + 4 * row.c0 + off
        if row.c1:
            a.A2, a.a_split, a.ldx2 = _P, row.c1, Ci - row.c1
        a.rows_per_group = Ho * Wo if row.entry in ("fwd", "ldx") else 1
        a.ld_rowadd, a.ldr = (Co if epilogue[1] else 0), (0 if row.entry == "krsc" else Co)
        a.bias, a.rowadd, a.residual = (_P + off if e else None for e in epilogue)
        if row.entry in ("fwd", "ldx"):
            wino_ok = (KH, KW) == (3, 3) and s == 1 and not row.c1 and hint in (0, 7, 8, 9, 10, 11) and splitk == 0 and pad == P1
            exists = _wino_weight_exists(Co, Ci, KH, KW, prec, bits)
            f4 = Ho % 4 == 0 and Wo % 4 == 0 and not no_wino4
            if wino_ok and exists and (hint == 7 or (hint == 0 and not f4)):
                a.B_wino = _P
            if wino_ok and exists and hint != 7 and f4:
                a.B_wino4 = _P
    elif direction == "dgrad":
        if one_by_one:
            a.a_mode, a.b_mode, a.M, a.N, a.K, a.lda, a.ldb, a.ldc = c.A_KC, c.B_MC, B * H * W, Ci, Co, Co, Ci, Ci
        else:
            a.a_mode, a.b_mode, a.M, a.N, a.K = c.A_CONVT, c.B_WDGRAD, B * He * We, Ci, KH * KW * Co
            a.lda, a.ldb, a.ldc = 0, 0, Ci
            a.g = c.ConvGeom(Ho, Wo, Co, Co, He, We, KH, KW, s, pad[0], pad[2], 0)
        a.rows_per_group = 1
    elif direction == "wgrad":
        if one_by_one:
            a.a_mode, a.b_mode, a.M, a.N, a.K, a.lda, a.ldb, a.ldc = c.A_MC, c.B_MC, Co, Ci, B * H * W, Co, Ci, Ci
        else:
            a.a_mode, a.b_mode, a.M, a.N, a.K = c.A_MC, c.B_CONV, Co, KH * KW * Ci, B * Ho * Wo
            a.lda, a.ldb, a.ldc = Co, 0, KH * KW * Ci
            a.g = c.ConvGeom(H, W, Ci, Ci, Ho, Wo, KH, KW, s, pad[0], pad[2], int(row.ups))
            if ((KH, KW) == (3, 3) and s == 1 and pad == P1 and hint in (0, 8) and splitk == 0 and Ho % 4 == 0 and Wo % 4 == 0
                    and prec == "f32" and not no_wino4 and not bits & (16 | 1 | 4 | 2 | 8)):
                a.flags |= c.GEMM_WINO_WGRAD
        a.rows_per_group = 1
    else:
        raise ValueError(direction)
    return a


def plan(a):
    """-> (kernel id, tile, splitk, vec) of gad_gemm_kernel_id / gad_gemm_plan"""
    from gad import _capi as c
    lib = c.load()
    tile, sk, vec = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    c.check(lib.gad_gemm_plan(ctypes.byref(a), ctypes.byref(tile), ctypes.byref(sk), ctypes.byref(vec)), "gad_gemm_plan")
    return lib.gad_gemm_kernel_id(ctypes.byref(a)), tile.value, sk.value, vec.value


def dgrad_as_forward(row):
    """ops.dgrad_as_forward for a frozen weight of this row"""
    return (row.KH, row.KW) == (3, 3) and row.stride == 1 and row.pad == P1 and row.Cout % 32 == 0 and row.Cin >= 64


# ------------------------------------------------------------------------- Winograd, written from the mathematics ----
# F(m x m, 3 x 3) with interpolation points 0, +-1 (and +-2 for m = 4), infinity (Lavin & Gray 2016):  y = A^T [(G w G^T) (.) (B^T d B)] A
def _mats(f, dtype):
    if f == 2:
        BT = [[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]]
        G = [[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]]
        AT = [[1, 1, 1, 0], [0, 1, -1, -1]]
    else:
        BT = [[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0], [0, 4, 0, -5, 0, 1]]
        G = [[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]]
        AT = [[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]]
    return tuple(torch.tensor(m, dtype=torch.float64).to(dtype) for m in (BT, G, AT))


def _windows(x, f):
    """x [B, C, H, W] (H, W multiples of f) -> the (f + 2)^2 input windows of its f x f output tiles, zero padding 1:
    [B, C, H / f, W / f, f + 2, f + 2]"""
    return F.pad(x, (1, 1, 1, 1)).unfold(2, f + 2, f).unfold(3, f + 2, f)


def wino_forward(x, w, f, ups=False):
    """3x3 / stride 1 / pad 1 convolution in Winograd F(f x f, 3 x 3) form, every step in the dtype of x"""
    if ups:
        x = F.interpolate(x, scale_factor=2.0, mode="nearest")
    BT, G, AT = _mats(f, x.dtype)
    Bn, _, H, W = x.shape
    V = BT @ _windows(x, f) @ BT.T                              # [B, C, th, tw, n, n]
    U = G @ w @ G.T                                             # [O, C, n, n]
    M = torch.einsum("bcthij,ocij->bothij", V, U)
    Y = AT @ M @ AT.T                                           # [B, O, th, tw, f, f]
    return Y.permute(0, 1, 2, 4, 3, 5).reshape(Bn, w.shape[0], H, W)


def wino4_wgrad(x, dy, ups=False):
    """include/gad.h: dW = G^T [sum_tiles (A dy A^T) (.) (B^T x B)] G, every step in the dtype of x"""
    if ups:
        x = F.interpolate(x, scale_factor=2.0, mode="nearest")
    BT, G, AT = _mats(4, x.dtype)
    V = BT @ _windows(x, 4) @ BT.T                              # [B, C, th, tw, 6, 6]
    Wy = AT.T @ dy.unfold(2, 4, 4).unfold(3, 4, 4) @ AT         # [B, O, th, tw, 6, 6]
    dU = torch.einsum("bothij,bcthij->ocij", Wy, V)
    return G.T @ dU @ G


# ------------------------------------------------------------------------------------------ conditioning cases ----
# B, Cin, Cout, H, W; 68: the ragged channel block; 32: Cin is no multiple of 64, so the one-launch F(4x4) forms run their 32-deep
# stage-steps on the four-stage ring (the other ring depth and wait count)
COND_SHAPES = {"64": (2, 64, 64, 16, 16), "68": (2, 64, 68, 16, 16), "32": (2, 32, 64, 16, 16)}
SIX_POSITION_SHAPE = (171, 32, 128, 32, 32)     # the cheapest launch with tiles_m * tiles_n * 6 >= 1024: 64 x 128 blocks, T / 64 = B = 171, one 32-channel chunk
# The other block shape of the six-position kernel.  use_wino pads Cout to the block's channels: Cout = 64 pads to 64 on 64-channel
# blocks and to 128 on 128-channel ones, so it takes (128 tiles x 64 channels); T = 342 * 64 = 21888 tiles -> 171 x 1 blocks, x 6
# = 1026 >= 1024, the threshold of the six-position form.  (The plan query reports tile 128 for both block shapes; the 24-panel
# scratch size tells the six-position form from the 36 batched products.)
SIX_POSITION_SHAPE_128x64 = (342, 32, 64, 32, 32)
SIX_POSITION_SHAPES = {"six": SIX_POSITION_SHAPE, "six-128x64": SIX_POSITION_SHAPE_128x64}
SPIKES = ((0, 0), (7, 9))                       # a corner pixel and an interior one (no 6 x 6 window holds both)
COND_NAMES = ("randn", "silu", "offset(30,1)", "hot_channel", "spike", "highpass_ramp", "constant")


def cond_inputs(name, shape, seed=0):
    """-> (x [B, Cin, H, W], w [Cout, Cin, 3, 3]) fp32"""
    B, Ci, Co, H, W = shape
    g = torch.Generator().manual_seed(77 + seed)
    z = torch.randn(B, Ci, H, W, generator=g)
    w = torch.randn(Co, Ci, 3, 3, generator=g) / (9 * Ci) ** 0.5
    if name == "randn":
        x = z
    elif name == "silu":                        # SiLU(gamma z + beta) per channel: what conv1 / conv2 of a ResnetBlock2D read
        gamma, beta = 1 + 0.3 * torch.randn(Ci, generator=g), 0.2 * torch.randn(Ci, generator=g)
        x = F.silu(gamma[None, :, None, None] * z + beta[None, :, None, None])
    elif name == "offset(30,1)":
        x = 30.0 + z
    elif name == "hot_channel":
        x = z.clone()
        x[:, 0] *= 1000.0
        x[:, -1] *= 1000.0
    elif name == "spike":
        x = z.clone()
        sign = torch.where(torch.rand(2, Ci, generator=g) < 0.5, -1.0, 1.0)
        for i, (r, c) in enumerate(SPIKES):
            x[:, :, r, c] = 1000.0 * sign[i]
    elif name == "spike_removed":               # the same draw with the spike pixels left as they were
        return cond_inputs("randn", shape, seed)
    elif name == "highpass_ramp":
        w = w - w.mean((2, 3), keepdim=True)
        ramp = 0.5 * torch.arange(H)[:, None] + 0.25 * torch.arange(W)[None, :]
        x = ramp[None, None] + torch.arange(Ci)[None, :, None, None] / 8.0 + 0.01 * z
    elif name == "constant":
        x = torch.full((B, Ci, H, W), 96.0)
    else:
        raise ValueError(name)
    return x.float().contiguous(), w.float().contiguous()


def _max_err(a, b):
    return (a.double() - b.double()).abs().max().item()


def cond_forward_reference(x, w, algorithm):
    """-> (want fp64 [B, Cout, H, W], e_ref): e_ref = the max error of the fp32 CPU run of `algorithm` (direct, wino2, wino4)"""
    want = conv_ref(x.double(), w.double())
    got32 = conv_ref(x, w) if algorithm == "direct" else wino_forward(x, w, 2 if algorithm == "wino2" else 4)
    return want, _max_err(got32, want)


def cond_wgrad_reference(x, dy, algorithm):
    """the same for the weight gradient [Cout, Cin, 3, 3] (direct: fp32 autograd; wino4: the emulation)"""
    def autograd(dt):
        w = torch.zeros(dy.shape[1], x.shape[1], 3, 3, dtype=dt, requires_grad=True)
        conv_ref(x.to(dt), w).backward(dy.to(dt))
        return w.grad
    want = autograd(torch.float64)
    got32 = autograd(torch.float32) if algorithm == "direct" else wino4_wgrad(x, dy)
    return want, _max_err(got32, want)


def bound(e_ref, want, k=K):
    return k * max(e_ref, FLOOR * want.abs().max().item())


def figure(got, want, e_ref, label):
    """-> (err, bound, line): the line is what the tests print before they assert and what profiles/conv_conditioning.txt holds"""
    err = _max_err(got.detach().cpu(), want)
    b = bound(e_ref, want)
    return err, b, f"{label:60s} err {err:9.3e}  e_ref {e_ref:9.3e}  max|want| {want.abs().max().item():9.3e}  err/e_ref {err / max(e_ref, 1e-300):8.2f}  err/bound {err / b:7.3f}"


def constant_expected(w, value=96.0):
    """x = value everywhere, 3x3 / pad 1 on an H x W map: the output at (i, j) is value * the sum of the taps inside the map -
    -> fp64 [Cout, 3, 3] indexed by (row class, column class), class 0 = first row / column, 1 = interior, 2 = last"""
    wd = w.double().sum(1)                                      # [Cout, 3, 3]
    out = torch.zeros(w.shape[0], 3, 3, dtype=torch.float64)
    rows = {0: (1, 2), 1: (0, 1, 2), 2: (0, 1)}
    for rc, rs in rows.items():
        for cc, cs in rows.items():
            out[:, rc, cc] = value * sum(wd[:, r, s] for r in rs for s in cs)
    return out
