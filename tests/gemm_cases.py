"""The launches of the dense-engine ABI suite (tests/test_gemm_abi_cpu.py checks them against torch.einsum on the CPU,
tests/test_gpu_gemm_abi.py runs them on gad_gemm): each case is a gemm_ref.Launch plus its flat buffers, built from small
contiguous "logical" tensors by scattering them into NaN-filled storage at the launch's strides.

Integer cases: A, B in [-4, 4], bias / rowadd / residual in [-8, 8], alpha in {1, 0.5, -2}, K <= 1024 - every product,
partial sum, split-K slab and epilogue value is an integer or half-integer far below 2^24, so fp32 computes it exactly in
any order and bf16 rounding of the operands changes nothing: the tests compare with torch.equal.
Operand padding (row tails, gaps between batch slabs, floats before an offset pointer) is NaN; the output starts as
SENTINEL, a finite value no case can produce."""
from dataclasses import dataclass, field, replace

import torch

from gemm_ref import A_KC, A_MC, B_KC, B_MC, Launch

SENTINEL = -12345.75
SLACK = 8                      # floats past the last addressed element of every buffer (padding like the rest)
MODE_PAIRS = {"kc_kc": (A_KC, B_KC), "kc_mc": (A_KC, B_MC), "mc_mc": (A_MC, B_MC)}
DENSE_SHAPES = [(1, 4, 4), (65, 64, 32), (63, 65, 36), (129, 68, 96), (130, 132, 100), (70, 60, 37), (200, 192, 256)]
LD_VARIANTS = ("tight", "pad4", "odd")          # every ld as small as it goes / every ld + 4 (keeps float4) / lda, ldb + 1 (vec 1)
KCAT_SHAPES = [(65, 68, 32, 4), (130, 64, 64, 32), (33, 132, 96, 12)]       # (M, N, k_split, K2)
ATTN_SHAPES = [(33, 40, 8), (64, 64, 32), (5, 12, 24)]                      # (Tq, Tk, d)
ATTN_FORMS = ("qk", "pv", "ptdo")               # KC x KC scores, KC x MC P V, MC x MC P^T dO (ops.UnfusedAttentionCoreFn)


@dataclass
class Case:
    label: str
    L: Launch
    bufs: dict                                   # flat fp64 buffers: A, B, C0 and, where the launch has them, bias, rowadd, residual, A_k2, B_k2
    logical: dict = field(default_factory=dict)  # contiguous a [Z][M][K], b [Z][N][K], bias [N], rowadd [G][N], residual [Z][M][N]

    def operands(self):
        """keyword arguments of gemm_ref.expected"""
        return {k: self.bufs.get(k) for k in ("bias", "rowadd", "residual", "A_k2", "B_k2")}


def float4_rule(L):
    """include/gad.h: vec 4 when both operands can be read as 16-byte aligned float4 - the contiguous extent and the row
    stride of each are multiples of 4 and, in a batched launch, so are its batch strides (A and B themselves are aligned)."""
    ok = L.lda % 4 == 0 and L.ldb % 4 == 0
    ok = ok and (L.K if L.a_mode == A_KC else L.M) % 4 == 0 and (L.K if L.b_mode == B_KC else L.N) % 4 == 0
    if L.batch > 1:
        ok = ok and all(s % 4 == 0 for s in (*L.sA, *L.sB))
    return 4 if ok else 1


def _ints(gen, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=gen).double()


def _scatter(fill, off, sizes, strides, values):
    """A flat buffer just long enough for the strided block (+ SLACK), filled with `fill`, with `values` written at
    off + sum(index * stride)."""
    last = off + sum((n - 1) * s for n, s in zip(sizes, strides))
    buf = torch.full((last + 1 + SLACK,), fill, dtype=torch.float64)
    torch.as_strided(buf, sizes, strides, off).copy_(values)
    return buf


def block(buf, off, sizes, strides):
    return torch.as_strided(buf, sizes, strides, off)


def build(label, L, seed, bias=False, rowadd=False, residual=False, randn=False):
    """Draw the logical tensors of launch L and scatter them into flat buffers at L's strides and offsets."""
    g = torch.Generator().manual_seed(seed)
    Z = max(1, L.batch)
    inner = L.inner
    assert Z % inner == 0
    Z0 = Z // inner
    draw = (lambda lo, hi, *s: torch.randn(*s, generator=g).double()) if randn else (lambda lo, hi, *s: _ints(g, lo, hi, *s))
    a, b = draw(-4, 4, Z, L.M, L.K), draw(-4, 4, Z, L.N, L.K)
    k1 = L.k_split if L.k_split > 0 else L.K
    bufs, logical = {}, dict(a=a, b=b)

    def operand(x, off, k_contiguous, ld, s):    # x [Z][rows][k]
        x = x.reshape(Z0, inner, *x.shape[1:])
        if not k_contiguous:
            x = x.transpose(2, 3)
        return _scatter(float("nan"), off, tuple(x.shape), (s[0], s[1], ld, 1), x)
    bufs["A"] = operand(a[:, :, :k1], L.off_A, L.a_mode == A_KC, L.lda, L.sA)
    bufs["B"] = operand(b[:, :, :k1], L.off_B, L.b_mode == B_KC, L.ldb, L.sB)
    if L.k_split > 0:
        assert Z == 1
        bufs["A_k2"] = _scatter(float("nan"), 0, (L.M, L.K - k1), (L.lda_k2, 1), a[0, :, k1:])
        b2 = b[0, :, k1:] if L.b_mode == B_KC else b[0, :, k1:].T
        bufs["B_k2"] = _scatter(float("nan"), 0, tuple(b2.shape), (L.ldb_k2, 1), b2)
    csz = (Z0, inner, L.M, L.N)
    bufs["C0"] = _scatter(SENTINEL, L.off_C, csz, (L.sC[0], L.sC[1], L.ldc, 1), torch.full(csz, SENTINEL, dtype=torch.float64))
    if bias:
        logical["bias"] = draw(-8, 8, L.N)
        bufs["bias"] = _scatter(float("nan"), L.off_bias, (L.N,), (1,), logical["bias"])
    if rowadd:
        G = (L.M + L.rows_per_group - 1) // L.rows_per_group
        logical["rowadd"] = draw(-8, 8, G, L.N)
        bufs["rowadd"] = _scatter(float("nan"), L.off_rowadd, (G, L.N), (L.ld_rowadd, 1), logical["rowadd"])
    if residual:
        logical["residual"] = draw(-8, 8, Z, L.M, L.N)
        bufs["residual"] = _scatter(float("nan"), L.off_residual, csz, (L.sC[0], L.sC[1], L.ldr, 1), logical["residual"].reshape(csz))
    return Case(label, L, bufs, logical)


# ---- dense launches (batch 1): leading dimensions x epilogues ----
EPILOGUES = ("none", "all_rpg1", "all_rpg3", "all_rpgM", "c_off1", "bias_off1", "ldr_odd", "ld_rowadd_odd")
ALPHAS = (1.0, 0.5, -2.0)


def dense_launch(pair, shape, ld, epi):
    a_mode, b_mode = MODE_PAIRS[pair]
    M, N, K = shape
    pad = {"tight": 0, "pad4": 4, "odd": 1}[ld]
    lda = (K if a_mode == A_KC else M) + pad
    ldb = (K if b_mode == B_KC else N) + pad
    if epi == "none":
        return Launch(a_mode, b_mode, M, N, K, lda, ldb, N + (4 if ld == "pad4" else 0))
    # bias, rowadd, residual and alpha, each tensor on its own stride; then the float4 epilogue broken one way at a time
    rpg = {"all_rpg1": 1, "all_rpgM": M}.get(epi, 3)
    L = Launch(a_mode, b_mode, M, N, K, lda, ldb, N + 4, alpha=ALPHAS[EPILOGUES.index(epi) % 3], rows_per_group=rpg,
               ld_rowadd=N + 4, ldr=N + 8)
    return replace(L, **{"c_off1": dict(off_C=1), "bias_off1": dict(off_bias=1), "ldr_odd": dict(ldr=N + 1),
                         "ld_rowadd_odd": dict(ld_rowadd=N + 1)}.get(epi, {}))


def dense_cases(pair, shape):
    for i, ld in enumerate(LD_VARIANTS):
        for j, epi in enumerate(EPILOGUES):
            full = epi != "none"
            yield build(f"{pair} {shape} ld {ld} epilogue {epi}", dense_launch(pair, shape, ld, epi), 100 * i + j + sum(shape),
                        bias=full, rowadd=full, residual=full)


def accuracy_case(pair, seed=7):
    """randn operands at (256, 132, 1000), every leading dimension padded by 4, the full epilogue"""
    a_mode, b_mode = MODE_PAIRS[pair]
    M, N, K = 256, 132, 1000
    L = Launch(a_mode, b_mode, M, N, K, (K if a_mode == A_KC else M) + 4, (K if b_mode == B_KC else N) + 4, N + 4, alpha=0.5,
               rows_per_group=3, ld_rowadd=N + 4, ldr=N + 4)
    return build(f"{pair} randn", L, seed, bias=True, rowadd=True, residual=True, randn=True)


# ---- K-concatenated launches (the fused LoRA linear) ----
def kcat_cases(pair):
    a_mode, b_mode = MODE_PAIRS[pair]
    assert a_mode == A_KC
    for i, (M, N, ks, K2) in enumerate(KCAT_SHAPES):
        for epi in (False, True):
            L = Launch(a_mode, b_mode, M, N, ks + K2, ks + 4, ks if b_mode == B_KC else N, N + 4 if epi else N,
                       alpha=0.5 if epi else 1.0, ldr=N + 4 if epi else 0, k_split=ks, lda_k2=K2 + 4,
                       ldb_k2=(K2 if b_mode == B_KC else N) + 4)
            yield build(f"{pair} kcat {(M, N, ks, K2)} epilogue {epi}", L, 300 + 2 * i + epi, bias=epi, residual=epi)


# ---- batched launches ----
def attention_launch(form, Tq, Tk, d, heads=3, B=2, ld=None, head_stride=None, odd=()):
    """The three products of the unfused attention route on [B][T][heads * d] tensors and [B][heads][Tq][Tk] scores, the scores'
    outer stride padded by 8.  ld / head_stride: the row stride and the head stride of the token tensors (default heads * d
    and d); odd: which of "A", "B" take them (the others keep the defaults)."""
    C = heads * d
    P = dict(ld=Tk, s=(heads * Tq * Tk + 8, Tq * Tk))                       # the score tensor

    def tok(T, name):                                                       # a token tensor [B][T][heads * d]
        l_, h_ = (ld, head_stride) if name in odd else (C, d)
        return dict(ld=l_, s=(T * l_ + (8 if name == "C" else 0), h_))
    if form == "qk":      # S = alpha Q K^T
        A, Bm, Cm, modes, (M, N, K) = tok(Tq, "A"), tok(Tk, "B"), P, (A_KC, B_KC), (Tq, Tk, d)
    elif form == "pv":    # O = P V
        A, Bm, Cm, modes, (M, N, K) = P, tok(Tk, "B"), tok(Tq, "C"), (A_KC, B_MC), (Tq, d, Tk)
    else:                 # dV = P^T dO
        A, Bm, Cm, modes, (M, N, K) = P, tok(Tq, "B"), tok(Tk, "C"), (A_MC, B_MC), (Tk, d, Tq)
    return Launch(*modes, M, N, K, A["ld"], Bm["ld"], Cm["ld"], batch=B * heads, batch_inner=heads, sA=A["s"], sB=Bm["s"], sC=Cm["s"],
                  alpha=0.5 if form == "qk" else 1.0)


def attention_cases(form):
    for i, (Tq, Tk, d) in enumerate(ATTN_SHAPES):
        yield build(f"attention {form} {(Tq, Tk, d)}", attention_launch(form, Tq, Tk, d), 400 + i)


def odd_stride_cases():
    """d = 8 heads spaced 9 floats apart in rows of 28 (a multiple of 4): every row stride is float4-able, the head stride is
    not - for A, for B and for both."""
    for i, odd in enumerate((("A",), ("B",), ("A", "B"))):
        yield build(f"attention qk odd head stride of {odd}", attention_launch("qk", 33, 40, 8, ld=28, head_stride=9, odd=odd), 500 + i)


def slab_cases(pair):
    """batch 5, batch_inner 0 (means 1): slabs 4 floats apart, as the Winograd product panels are laid out; bias + residual,
    the residual on C's batch stride with its own (smaller) row stride."""
    a_mode, b_mode = MODE_PAIRS[pair]
    M, N, K = 68, 36, 64
    lda, ldb, ldc, ldr = (K if a_mode == A_KC else M) + 4, (K if b_mode == B_KC else N) + 4, N + 8, N + 4
    rows_a, rows_b = (M if a_mode == A_KC else K), (N if b_mode == B_KC else K)
    L = Launch(a_mode, b_mode, M, N, K, lda, ldb, ldc, batch=5, batch_inner=0, sA=(rows_a * lda + 4, 0), sB=(rows_b * ldb + 4, 0),
               sC=(M * ldc + 4, 0), alpha=-2.0, ldr=ldr)
    yield build(f"{pair} slabs", L, 600, bias=True, residual=True)


def all_case_lists():
    """(name, generator of cases) of every list above - what the CPU test walks."""
    for pair in MODE_PAIRS:
        for shape in DENSE_SHAPES:
            yield f"dense-{pair}-{shape}", lambda pair=pair, shape=shape: dense_cases(pair, shape)
        yield f"accuracy-{pair}", lambda pair=pair: iter([accuracy_case(pair)])
        yield f"slabs-{pair}", lambda pair=pair: slab_cases(pair)
    for pair in ("kc_kc", "kc_mc"):
        yield f"kcat-{pair}", lambda pair=pair: kcat_cases(pair)
    for form in ATTN_FORMS:
        yield f"attention-{form}", lambda form=form: attention_cases(form)
    yield "attention-odd-strides", odd_stride_cases
