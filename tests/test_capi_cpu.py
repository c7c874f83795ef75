"""CPU checks of the drop-in boundary: the shared library loads without a GPU and exports
every symbol include/gad.h declares; the ctypes structs match the C layout."""
import ctypes
import os
import re

import pytest

from gad import _capi


def _declared_symbols():
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "gad.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return sorted(set(re.findall(r"\b(gad_[a-z0-9_]+)\s*\(", hdr)))


def test_every_declared_symbol_is_exported_and_bound():
    lib = _capi.load()
    names = _declared_symbols()
    assert len(names) >= 25
    for n in names:
        assert hasattr(lib, n), n
        assert n in _capi.SIGNATURES, f"{n} declared in gad.h but not bound in _capi.SIGNATURES"
    assert sorted(_capi.SIGNATURES) == names
    assert lib.gad_version() >= 100


def test_struct_layout_matches_header(tmp_path):
    """Every field of every argument struct: sizeof and offsetof as gcc lays out include/gad.h against the ctypes
    mirror in gad/_capi.py (guards against a field drifting between the two)."""
    import subprocess
    structs = {"gad_conv_geom": _capi.ConvGeom, "gad_gemm_args": _capi.GemmArgs, "gad_groupnorm_args": _capi.GroupNormArgs,
               "gad_adam_args": _capi.AdamArgs, "gad_attention_args": _capi.AttentionArgs, "gad_hgemm_args": _capi.HGemmArgs}
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "gad.h"', 'int main(void) {']
    for cname, cls in structs.items():
        src.append(f'  printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in cls._fields_:
            src.append(f'  printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    src += ['  return 0;', '}']
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "layout"
    inc = os.path.join(os.path.dirname(__file__), "..", "include")
    subprocess.run(["gcc", "-I", inc, str(c), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for cname, cls in structs.items():
        assert int(got[cname]) == ctypes.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(cls, fname).offset, f"{cname}.{fname}"


def test_host_side_argument_validation_without_gpu():
    lib = _capi.load()
    a = _capi.GemmArgs()
    assert lib.gad_gemm(ctypes.byref(a), None) != 0          # null pointers are rejected on the host
    assert b"null" in lib.gad_last_error()
    a.A = a.B = a.C = 16
    a.M, a.N, a.K = 8, 8, 8
    a.lda = a.ldb = 8
    a.ldc = 4                                                  # ldc < N would write out of bounds
    assert lib.gad_gemm(ctypes.byref(a), None) != 0
    assert b"ldc" in lib.gad_last_error()


def test_product_path_has_no_cpu_fallback():
    import pytest
    import torch
    import gad
    net = gad.UNet2DModel(block_out_channels=(32, 32), down_block_types=("DownBlock2D", "DownBlock2D"),
                          up_block_types=("UpBlock2D", "UpBlock2D"), layers_per_block=1, attention_head_dim=None,
                          sample_size=8)
    with pytest.raises(_capi.GadError):
        net(torch.zeros(1, 3, 8, 8), torch.tensor([1]))


def test_error_state_is_per_thread():
    """the library is re-entrant; the last-error string is thread-local, so concurrent host threads
    (one per sampling stream) cannot read each other's failures."""
    import threading
    lib = _capi.load()
    seen = {}

    def worker(name, make_error):
        if make_error:
            a = _capi.GemmArgs()
            assert lib.gad_gemm(ctypes.byref(a), None) != 0
        barrier.wait()
        seen[name] = bytes(lib.gad_last_error())

    barrier = threading.Barrier(2)
    ts = [threading.Thread(target=worker, args=("bad", True)), threading.Thread(target=worker, args=("good", False))]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert b"null" in seen["bad"] and seen["good"] == b""


def _conv_args(a_mode, b_mode, M, N, K, H, W, C, Ho=None, Wo=None, k=3, stride=1, pad=1, ups=0, prec=0):
    a = _capi.GemmArgs()
    a.a_mode, a.b_mode, a.M, a.N, a.K = a_mode, b_mode, M, N, K
    a.lda, a.ldb, a.ldc = (M if a_mode == _capi.A_MC else K), K, N
    a.g = _capi.ConvGeom(H, W, C, C, Ho or H, Wo or W, k, k, stride, pad, pad, ups)
    a.operand_precision = prec
    return a


def test_kernel_family_selection_is_a_pure_host_decision():
    """gad_gemm_kernel_id: 0 generic fp32, 1 generic bf16, 2 LDS-patch fp32, 3 LDS-patch bf16 - decided from shapes
    alone, so it can be checked without a GPU (the GPU tests check that each family computes the same numbers)."""
    lib = _capi.load()
    kid = lambda a: lib.gad_gemm_kernel_id(ctypes.byref(a))     # noqa: E731
    big = 512 * 32 * 32
    fwd = _conv_args(_capi.A_CONV, _capi.B_KC, big, 128, 9 * 128, 32, 32, 128)
    assert kid(fwd) == 2                                                     # 3x3 s1 p1, whole-row tiles, 128-tile plan
    fwd.operand_precision = 1
    assert kid(fwd) == 3
    assert kid(_conv_args(_capi.A_CONV, _capi.B_KC, big // 4, 128, 9 * 128, 32, 32, 128, Ho=16, Wo=16, stride=2, pad=0)) == 0
    assert kid(_conv_args(_capi.A_CONV, _capi.B_KC, big, 128, 128, 32, 32, 128, k=1, pad=0)) == 0        # 1x1
    assert kid(_conv_args(_capi.A_CONV, _capi.B_KC, big, 128, 9 * 100, 32, 32, 100)) == 0               # C % 32 != 0
    assert kid(_conv_args(_capi.A_CONV, _capi.B_KC, 2 * 32 * 32, 128, 9 * 128, 32, 32, 128)) == 0       # tiny M: split-K plan
    small = _conv_args(_capi.A_CONV, _capi.B_KC, 1024 * 16, 256, 9 * 256, 4, 4, 256)                     # 4x4 maps, B = 1024
    assert kid(small) == 2 and lib.gad_gemm_workspace_bytes(ctypes.byref(small)) == 2 * 1024 * 16 * 256 * 4   # 2 chunk splits
    up = _conv_args(_capi.A_CONV, _capi.B_KC, big, 256, 9 * 256, 16, 16, 256, Ho=32, Wo=32, ups=1)
    assert kid(up) == 2                                                      # nearest-2x fused into the patch fetch
    dg = _conv_args(_capi.A_CONVT, _capi.B_WDGRAD, big, 128, 9 * 128, 32, 32, 128)
    assert kid(dg) == 2
    wg = _conv_args(_capi.A_MC, _capi.B_CONV, 128, 9 * 128, 128 * 32 * 32, 32, 32, 128)
    assert kid(wg) == 2 and lib.gad_gemm_workspace_bytes(ctypes.byref(wg)) == 128 * 128 * 1152 * 4     # 128 pixel splits
    lin = _capi.GemmArgs()
    lin.a_mode, lin.b_mode, lin.M, lin.N, lin.K, lin.lda, lin.ldb, lin.ldc = _capi.A_KC, _capi.B_KC, 4096, 256, 256, 256, 256, 256
    assert kid(lin) == 0
    lin.operand_precision = 1
    assert kid(lin) == 1 and lib.gad_gemm_uses_bf16(ctypes.byref(lin)) == 1
    lin.K = lin.lda = lin.ldb = 27                                           # no aligned float4 path: stays fp32
    assert kid(lin) == 0 and lib.gad_gemm_uses_bf16(ctypes.byref(lin)) == 0


def test_winograd_weight_gradient_plan_is_the_same_with_a_kept_input_image():
    """A 3x3 weight gradient in Winograd F(4x4) form (GAD_GEMM_WINO_WGRAD) given the forward launch's transformed input
    (GAD_GEMM_WINO_SKIP_INPUT + B_wino4 = V) is the same plan - kernel id 7, the same scratch request - as without it: only the
    input-transform launch is dropped (host decisions, no GPU); a misaligned image is refused before anything is launched."""
    lib = _capi.load()
    wg = _conv_args(_capi.A_MC, _capi.B_CONV, 128, 9 * 128, 128 * 32 * 32, 32, 32, 128)
    wg.A = wg.B = wg.C = 4096
    wg.lda, wg.ldc, wg.alpha = 128, 9 * 128, 1.0
    wg.flags = _capi.GEMM_WINO_WGRAD
    assert lib.gad_gemm_kernel_id(ctypes.byref(wg)) == 7
    need = lib.gad_gemm_wino_bytes(ctypes.byref(wg))
    T = 128 * 32 * 32 // 16
    assert need == 36 * 4 * (T * 128 + T * 128 + 128 * 128)                  # transformed dy, transformed x, the 36 product panels
    wg.flags |= _capi.GEMM_WINO_SKIP_INPUT
    wg.B_wino4 = 8192
    assert lib.gad_gemm_kernel_id(ctypes.byref(wg)) == 7 and lib.gad_gemm_wino_bytes(ctypes.byref(wg)) == need
    wg.wino_ws, wg.wino_ws_bytes, wg.B_wino4 = 1 << 20, need, 8196          # image not 16-byte aligned
    assert lib.gad_gemm(ctypes.byref(wg), None) != 0 and b"kept Winograd input image" in lib.gad_last_error()


def test_half_path_host_side_checks_and_planner_without_gpu():
    """gad_hgemm's argument validation and its planner are host code: misuse is rejected before anything is launched, and the
    tile / split-K choices for the SD step's shapes are the ones DESIGN.md §4.4 states (no GPU needed)."""
    lib = _capi.load()
    a = _capi.HGemmArgs()
    assert lib.gad_hgemm(ctypes.byref(a), None) != 0 and b"null" in lib.gad_last_error()
    a.A = a.B = a.C = 4096
    a.M, a.N, a.K, a.lda, a.ldb, a.ldc, a.k_split = 64, 64, 36, 40, 40, 64, 36
    assert lib.gad_hgemm(ctypes.byref(a), None) != 0 and b"multiples of 8" in lib.gad_last_error()      # K % 8
    a.K = a.k_split = 40
    a.A = 4098
    assert lib.gad_hgemm(ctypes.byref(a), None) != 0 and b"aligned" in lib.gad_last_error()
    assert lib.gad_hgemm_workspace_bytes(ctypes.byref(a)) < 0

    def plan(M, N, K, conv=False, out_f32=False):
        g = _capi.HGemmArgs()
        g.A = g.B = g.C = 4096
        g.M, g.N, g.K, g.ldb, g.ldc, g.out_f32 = M, N, K, K, N, int(out_f32)
        if conv:
            cin = K // 9
            hw = int(round((M // 16) ** 0.5))
            g.conv, g.KH, g.KW, g.Cin, g.H, g.W, g.Ho, g.Wo, g.stride, g.pad_t, g.pad_l = 1, 3, 3, cin, hw, hw, hw, hw, 1, 1, 1
            g.lda, g.k_split = cin, cin
        else:
            g.lda, g.k_split = K, K
        tile, sk = ctypes.c_int32(), ctypes.c_int32()
        assert lib.gad_hgemm_plan(ctypes.byref(g), ctypes.byref(tile), ctypes.byref(sk)) == 0, lib.gad_last_error()
        need = lib.gad_hgemm_workspace_bytes(ctypes.byref(g))
        assert need == (sk.value * M * N * 4 if sk.value > 1 else 0)
        return tile.value, sk.value
    assert plan(65536, 320, 2880, conv=True) == (6, 1)             # 64x64 maps: one round of 256 x 320 tiles on eight waves
    assert plan(16384, 640, 5760, conv=True) == (6, 2)             # 32x32 maps: the same form, two K slices
    assert plan(4096, 1280, 11520, conv=True) == (6, 4)
    t, sk = plan(1024, 1280, 11520, conv=True)                     # 8x8 maps: 128 x 320 tiles, split
    assert t == 7 and sk >= 8
    assert plan(65536, 2560, 320) == (7, 1)                        # GEGLU projection: full rounds of 128 x 320
    assert plan(65536, 256, 320) == (8, 1)                         # LoRA rank products: 128 x 128, four workgroups per CU
    assert plan(4096, 1280, 1280) == (9, 1)                        # 16x16 level Linear: more 128 x 128 tiles than 128 x 320 ones
    assert plan(65536, 4, 2880, conv=True)[0] in (1, 8, 9)         # conv_out


# ---- gad_gemm's route table: the five host queries over a fixed grid of launches, against tests/golden/gemm_routes.npz ----
ROUTE_COLUMNS = ("kernel_id", "tile", "splitk", "vec", "ws_bytes", "wino_bytes", "uses_bf16")
_P = 1 << 24                          # placeholder addresses: the queries read only their 16-byte alignment


def _route_args(a_mode, b_mode, M, N, K, geom=None, batch=1):
    a = _capi.GemmArgs()
    a.A, a.B, a.C = _P, 2 * _P, 3 * _P
    a.a_mode, a.b_mode, a.M, a.N, a.K, a.batch, a.alpha = a_mode, b_mode, M, N, K, batch, 1.0
    a.lda = M if a_mode == _capi.A_MC else (geom[2] if a_mode == _capi.A_CONV else K)
    a.ldb = N if b_mode == _capi.B_MC else K
    a.ldc = N
    if geom is not None:
        H, W, C, Ho, Wo, k, stride, pad, ups = geom
        a.g = _capi.ConvGeom(H, W, C, C, Ho, Wo, k, k, stride, pad, pad, ups)
    return a


def _set(**kw):
    def f(a):
        for k, v in kw.items():
            setattr(a, k, v)
    return f


def _ragged(a):                       # leading dimensions that break the float4 path
    a.lda += 1
    a.ldb += 1
    a.g.ldx = a.g.C + 1


def _epilogue(a):
    a.bias, a.residual, a.ldr = 4 * _P, 5 * _P, a.N
    a.rowadd, a.ld_rowadd, a.rows_per_group = 6 * _P, a.N, max(1, a.g.Ho * a.g.Wo)


def _split_m_hint(a):                 # forced weight-gradient row split: 128-channel tiles, then the rest
    a.tile_hint = 1000 + (a.M // 2 // 128 * 128 or 128)


F = _capi
WINO = dict(B_wino=7 * _P, B_wino4=8 * _P)
ROUTE_VARIANTS = [
    _set(operand_precision=1), _set(**WINO), _set(B_wino=7 * _P), _set(B_wino4=8 * _P),
    _set(flags=F.GEMM_NO_PATCH, **WINO), _set(flags=F.GEMM_TAP_MAJOR_K, **WINO), _set(flags=F.GEMM_SCALAR_EPILOGUE, **WINO),
    _set(flags=F.GEMM_GENERAL_LOADERS, **WINO), _set(flags=F.GEMM_NO_WINO, **WINO), _set(flags=F.GEMM_WINO_WGRAD),
    _set(flags=F.GEMM_WINO_WGRAD, tile_hint=8), _set(flags=F.GEMM_WINO_ONLY_INPUT, **WINO),
    _set(flags=F.GEMM_WINO_SKIP_INPUT, B_wino4=8 * _P), _set(flags=F.GEMM_WINO_WGRAD | F.GEMM_WINO_SKIP_INPUT, B_wino4=8 * _P),
    *[_set(tile_hint=t, **WINO) for t in range(1, 12)], _split_m_hint,
    _set(splitk_hint=1), _set(splitk_hint=2), _set(splitk_hint=5), _set(operand_precision=1, tile_hint=2),
    _epilogue, _set(residual=5 * _P, ldr=0, **WINO), _ragged, _set(C=3 * _P + 4, **WINO), _set(A=_P + 4, flags=F.GEMM_WINO_WGRAD),
    _set(operand_precision=1, flags=F.GEMM_NO_PATCH), _set(alpha=0.5, flags=F.GEMM_WINO_WGRAD),
]


def gemm_route_grid():
    """The deterministic grid of gad_gemm_args the route table is recorded on: every mode pair over maps 4..64 (odd, upsampled,
    stride 2, 1x1), channel counts 3..640, batches 1..1024; each shape plain, with bf16 operands, with its Winograd inputs and
    with a rotating pick of ROUTE_VARIANTS (switches, tile / split hints, epilogues, ragged or misaligned operands)."""
    geoms = [(s, s, s, s, 3, 1, 1, 0) for s in (4, 8, 16, 32, 64)] + [(s // 2, s // 2, s, s, 3, 1, 1, 1) for s in (8, 16, 32, 64)]
    geoms += [(s, s, s // 2, s // 2, 3, 2, 1, 0) for s in (8, 32, 64)] + [(7, 7, 7, 7, 3, 1, 1, 0), (12, 16, 12, 16, 3, 1, 1, 0)]
    geoms += [(s, s, s, s, 1, 1, 0, 0) for s in (8, 32)]
    chans = (3, 4, 32, 96, 128, 224, 256, 320, 448, 640)
    couts = (3, 4, 64, 96, 128, 224, 320, 448, 672)
    batches = (1, 2, 8, 64, 256, 1024)
    i = 0

    def emit(base, *extra):
        nonlocal i
        i += 1
        yield base()
        for v in [*extra] + [ROUTE_VARIANTS[(i * 7 + j * 13) % len(ROUTE_VARIANTS)] for j in range(3)]:
            a = base()
            v(a)
            yield a
    for gi, (H, W, Ho, Wo, k, s, p, u) in enumerate(geoms):
        for ci, C in enumerate(chans):
            for ni, N in enumerate(couts):
                B = batches[(gi + ci + ni) % len(batches)]
                B2 = batches[(gi + 2 * ci + 3 * ni + 1) % len(batches)]
                geom = (H, W, C, Ho, Wo, k, s, p, u)
                yield from emit(lambda: _route_args(F.A_CONV, F.B_KC, B * Ho * Wo, N, k * k * C, geom), _set(**WINO), _set(operand_precision=1))
                yield from emit(lambda: _route_args(F.A_CONV, F.B_KC, B2 * Ho * Wo, N, k * k * C, geom), _set(**WINO), _set(operand_precision=1))
                yield from emit(lambda: _route_args(F.A_CONVT, F.B_WDGRAD, B2 * Ho * Wo, N, k * k * C, geom), _set(operand_precision=1))
                yield from emit(lambda: _route_args(F.A_MC, F.B_CONV, N, k * k * C, B * Ho * Wo, geom), _set(flags=F.GEMM_WINO_WGRAD))
                yield from emit(lambda: _route_args(F.A_MC, F.B_CONV, N, k * k * C, B2 * Ho * Wo, geom), _set(flags=F.GEMM_WINO_WGRAD))
    for pair in ((F.A_KC, F.B_KC), (F.A_KC, F.B_MC), (F.A_MC, F.B_MC)):
        for M in (1, 7, 64, 256, 1000, 4096, 16384, 65536, 262144):
            for N in (3, 4, 64, 96, 128, 320, 640, 1280):
                for K in (4, 27, 32, 256, 320, 640, 2560):
                    for batch in (1, 36):
                        yield from emit(lambda: _route_args(*pair, M, N, K, batch=batch), _set(operand_precision=1))
    for M in (1024, 16384, 65536):    # two-source gathers (3x3 and 1x1) and the K-concatenated dense form
        for C1, C in ((128, 256), (256, 384), (320, 640), (96, 200)):
            for k in (1, 3):
                s = int((M // 4) ** 0.5)
                def two(k=k, C=C, C1=C1, s=s):
                    a = _route_args(F.A_CONV, F.B_KC, M, 320, k * k * C, (s, s, C, s, s, k, 1, k // 2, 0))
                    a.A2, a.a_split, a.ldx2, a.g.ldx = 9 * _P, C1, C - C1, C1
                    return a
                yield from emit(two, _set(operand_precision=1))
            def cat(C=C, C1=C1):
                a = _route_args(F.A_KC, F.B_KC, M, 320, C)
                a.lda, a.A_k2, a.B_k2, a.k_split, a.lda_k2, a.ldb_k2 = C1, 9 * _P, 10 * _P, C1, C - C1, C - C1
                return a
            yield from emit(cat, _set(operand_precision=1))


def gemm_route_table(lib):
    """The five route queries of every grid case, as int64 columns (ROUTE_COLUMNS) plus the cases' mode pairs."""
    rows, modes = [], []
    tile, sk, vec = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    for a in gemm_route_grid():
        r = ctypes.byref(a)
        assert lib.gad_gemm_plan(r, ctypes.byref(tile), ctypes.byref(sk), ctypes.byref(vec)) == 0
        rows.append((lib.gad_gemm_kernel_id(r), tile.value, sk.value, vec.value, lib.gad_gemm_workspace_bytes(r),
                     lib.gad_gemm_wino_bytes(r), lib.gad_gemm_uses_bf16(r)))
        modes.append((a.a_mode, a.b_mode))
    import numpy as np
    cols = np.array(rows, dtype=np.int64).T
    return dict(zip(ROUTE_COLUMNS, cols)), np.array(modes, dtype=np.int64)


def test_gemm_route_table_matches_the_recorded_one(golden_dir):
    """Every size query of gad_gemm reads the one route route_of resolves: kernel id, plan, workspace and Winograd bytes and
    the bf16 answer over the grid are the ones recorded from the library before that refactor (tests/golden/gemm_routes.npz).
    The one deliberate change: the bf16 LDS-patch route (kernel id 3) reports what it launches - 128 x 128 tiles, no split,
    no workspace - where the old planner reported the generic engine's plan."""
    import numpy as np
    want = dict(np.load(os.path.join(golden_dir, "gemm_routes.npz")))
    got, modes = gemm_route_table(_capi.load())
    kid = want["kernel_id"]
    assert len(got["kernel_id"]) == len(kid)
    patch_bf16 = kid == 3
    want["tile"][patch_bf16], want["splitk"][patch_bf16], want["ws_bytes"][patch_bf16] = 128, 1, 0
    for c in ROUTE_COLUMNS:
        bad = np.nonzero(got[c] != want[c])[0]
        assert len(bad) == 0, f"{c}: {len(bad)} cases differ, first {bad[:5].tolist()}: {got[c][bad[:5]].tolist()} != {want[c][bad[:5]].tolist()}"
    # what the grid covers
    fwd, wgrad = (modes[:, 0] == _capi.A_CONV) | (modes[:, 0] == _capi.A_CONVT), modes[:, 1] == _capi.B_CONV
    tile, ws = got["tile"], got["ws_bytes"]
    assert set(range(8)) <= set(kid.tolist())
    assert ((kid == 2) & (tile == 224) & fwd).any() and ((kid == 2) & (tile == 224) & wgrad).any()     # split-N, split-M
    assert ((kid == 6) & (tile == 65)).any()                                                           # narrow one-launch F(4x4)
    assert (got["vec"] == 1).any()
    assert (((kid == 0) | (kid == 1)) & (ws > 0)).any()                                                # generic split-K
    assert ((kid == 2) & fwd & (ws > 0)).any() and ((kid == 2) & wgrad & (ws > 0)).any()               # patch split-K, patch wgrad
    assert ((kid == 6) & (ws > 0)).any()                                                               # three-launch F(4x4)


@pytest.mark.parametrize("pair", [(F.A_KC, F.B_KC), (F.A_KC, F.B_MC), (F.A_MC, F.B_MC)])
def test_batch_strides_are_part_of_the_float4_decision(pair):
    """A batched launch whose A or B slabs do not start on the float4 grid takes the dword loaders and, whatever
    operand_precision allows, multiplies in fp32 (gad.h, next to strideA0): one odd stride out of the four is enough.  With
    batch <= 1 the strides are not read."""
    lib = _capi.load()
    tile, sk, vec = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()

    def query(batch, **strides):
        a = _route_args(*pair, 64, 64, 64, batch=batch)
        a.batch_inner, a.operand_precision = 3, 1
        a.strideA0, a.strideA1, a.strideB0, a.strideB1 = 64 * 64 * 3, 64 * 64, 64 * 64 * 3, 64 * 64
        a.strideC0, a.strideC1 = 64 * 64 * 3, 64 * 64
        for k, v in strides.items():
            setattr(a, k, v)
        assert lib.gad_gemm_plan(ctypes.byref(a), ctypes.byref(tile), ctypes.byref(sk), ctypes.byref(vec)) == 0
        return vec.value, lib.gad_gemm_uses_bf16(ctypes.byref(a)), lib.gad_gemm_kernel_id(ctypes.byref(a))

    assert query(6) == (4, 1, 1)
    for field in ("strideA0", "strideA1", "strideB0", "strideB1"):
        for odd in (9, 64 * 64 + 1, 64 * 64 + 2, 64 * 64 * 3 - 1):
            assert odd % 4 != 0
            assert query(6, **{field: odd}) == (1, 0, 0), (field, odd)
            assert query(1, **{field: odd})[0] == 4, (field, odd)
            assert query(6, **{field: odd + 4 - odd % 4}) == (4, 1, 1), (field, odd)


def test_winograd_stage_flags_are_refused_off_their_route():
    """GAD_GEMM_WINO_ONLY_INPUT / _SKIP_INPUT run one stage of a Winograd launch.  A launch routed anywhere else would run a
    direct kernel that reads A (which the caller may hold only as the transformed image): gad_gemm refuses it on the host."""
    lib = _capi.load()
    kid = lambda a: lib.gad_gemm_kernel_id(ctypes.byref(a))     # noqa: E731

    def refused(a, flag):
        return lib.gad_gemm(ctypes.byref(a), None) != 0 and flag.encode() in lib.gad_last_error()
    conv = _route_args(_capi.A_CONV, _capi.B_KC, 512 * 32 * 32, 128, 9 * 128, (32, 32, 128, 32, 32, 3, 1, 1, 0))
    conv.B_wino4 = 8 * _P
    conv.flags = _capi.GEMM_WINO_SKIP_INPUT
    assert kid(conv) == 6
    conv.flags |= _capi.GEMM_NO_WINO                                          # the same convolution routed direct
    assert kid(conv) == 2 and refused(conv, "GAD_GEMM_WINO_SKIP_INPUT")
    small = _route_args(_capi.A_CONV, _capi.B_KC, 2 * 8 * 8, 128, 9 * 128, (8, 8, 128, 8, 8, 3, 1, 1, 0))
    small.B_wino4, small.flags = 8 * _P, _capi.GEMM_WINO_SKIP_INPUT          # too small for Winograd: the planner stays direct
    assert kid(small) not in (5, 6) and refused(small, "GAD_GEMM_WINO_SKIP_INPUT")
    split = _route_args(_capi.A_CONV, _capi.B_KC, 64 * 32 * 32, 448, 9 * 224, (32, 32, 224, 32, 32, 3, 1, 1, 0))
    tile, sk, vec = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    assert lib.gad_gemm_plan(ctypes.byref(split), ctypes.byref(tile), ctypes.byref(sk), ctypes.byref(vec)) == 0
    assert tile.value == 224                                                  # the two launches over 128- / 96-wide tiles
    split.flags = _capi.GEMM_WINO_SKIP_INPUT
    assert refused(split, "GAD_GEMM_WINO_SKIP_INPUT")
    wg = _route_args(_capi.A_MC, _capi.B_CONV, 128, 9 * 128, 128 * 32 * 32, (32, 32, 128, 32, 32, 3, 1, 1, 0))
    wg.flags = _capi.GEMM_WINO_WGRAD | _capi.GEMM_WINO_ONLY_INPUT
    assert kid(wg) == 7 and refused(wg, "GAD_GEMM_WINO_ONLY_INPUT")


# ---- the attention router's table: its three host queries over a fixed grid, against tests/golden/attention_routes.npz ----
ATTN_ROUTE_COLUMNS = ("ws_bytes", "uses_bf16_fwd", "uses_bf16_bwd")
ATTN_DIMS = (1, 8, 16, 23, 24, 32, 40, 41, 48, 64, 80, 88, 96, 97, 128, 160, 192, 224, 256, 257)
ATTN_BH = ((1, 1), (1, 8), (2, 8), (2, 21), (4, 16), (16, 8), (64, 1), (64, 8), (128, 5), (256, 2), (1024, 1))
ATTN_T = ((4096, 4096), (4096, 77), (256, 77), (100, 300), (64, 4096), (16, 16), (1024, 1024), (520, 260))


def attention_route_grid():
    """The grid the attention route table is recorded on, as (gad_attention_args, case tuple): head dims on and off the
    instances (257: unsupported), (B, heads) from 1 to 1024 blocks, self- and cross-attention lengths, row strides on and off
    the float4 contract, q 16-byte aligned or not, both operand precisions, no flag / two-kernel backward / narrow forward."""
    for d in ATTN_DIMS:
        for B, heads in ATTN_BH:
            for Tq, Tk in ATTN_T:
                for pad in (0, 2, 4):
                    for mis in (0, 4):
                        for prec in (0, 1):
                            for flags in (0, 1, 2):
                                a, ld = _capi.AttentionArgs(), heads * d + pad
                                a.q, a.k, a.v, a.o, a.lse = _P + mis, 2 * _P, 3 * _P, 4 * _P, 5 * _P
                                a.d_o, a.delta, a.dq, a.dk, a.dv = 6 * _P, 7 * _P, 8 * _P, 9 * _P, 10 * _P
                                a.B, a.heads, a.Tq, a.Tk, a.d = B, heads, Tq, Tk, d
                                a.ldq = a.ldk = a.ldv = a.ldo = a.ld_do = a.ld_dq = a.ld_dk = a.ld_dv = ld
                                a.stride_q = a.stride_o = a.stride_do = a.stride_dq = Tq * ld
                                a.stride_k = a.stride_v = a.stride_dk = a.stride_dv = Tk * ld
                                a.scale, a.operand_precision, a.flags = d ** -0.5, prec, flags
                                yield a, (d, B, heads, Tq, Tk, pad, mis, prec, flags)


def attention_route_table(lib):
    """The three queries of every grid case as int64 columns (ATTN_ROUTE_COLUMNS), and the cases as an int64 matrix."""
    import numpy as np
    rows, cases = [], []
    for a, case in attention_route_grid():
        r = ctypes.byref(a)
        rows.append((lib.gad_attention_bwd_workspace_bytes(r), lib.gad_attention_uses_bf16(r, 0), lib.gad_attention_uses_bf16(r, 1)))
        cases.append(case)
    return dict(zip(ATTN_ROUTE_COLUMNS, np.array(rows, dtype=np.int64).T)), np.array(cases, dtype=np.int64)


def test_attention_route_table_matches_the_recorded_one(golden_dir):
    """Both attention queries read the one Route route_of resolves (csrc/attention.hip): the workspace bytes and the two bf16
    answers over the grid are the ones recorded from the library before that refactor (tests/golden/attention_routes.npz).
    The one deliberate change: with GAD_ATTN_TWO_KERNEL_BWD the launch runs the dQ + dK/dV pair and uses no workspace, and
    the size query now says so - 0 bytes, where the old one answered with the single-pass kernel's slabs."""
    import numpy as np
    want = dict(np.load(os.path.join(golden_dir, "attention_routes.npz")))
    got, cases = attention_route_table(_capi.load())
    d, B, heads, Tq, Tk, pad, mis, prec, flags = cases.T
    assert len(got["ws_bytes"]) == len(want["ws_bytes"]) == len(ATTN_DIMS) * len(ATTN_BH) * len(ATTN_T) * 3 * 2 * 2 * 3
    pair = (flags & _capi.ATTN_TWO_KERNEL_BWD) != 0
    assert (want["ws_bytes"][pair] > 0).any()
    want["ws_bytes"][pair] = 0
    for c in ATTN_ROUTE_COLUMNS:
        bad = np.nonzero(got[c] != want[c])[0]
        assert len(bad) == 0, f"{c}: {len(bad)} cases differ, first {cases[bad[:5]].tolist()}: {got[c][bad[:5]].tolist()} != {want[c][bad[:5]].tolist()}"
    # what the grid covers
    ws, bf_f, bf_b = (got[c] for c in ATTN_ROUTE_COLUMNS)
    slab = B * Tq * heads * d * 4
    assert (ws % slab == 0).all()
    blocks = ws // slab                                            # key blocks of the single-pass launches that take slabs
    assert (blocks == 2).any() and (blocks == 4).any() and (blocks > 4).any() and not (blocks == 1).any()
    fp32 = ~pair & (prec == 0)
    assert (ws[d > 96] == 0).all() and (fp32 & (d > 96) & (d <= 256)).any()                 # no single-pass instance
    few = fp32 & (d <= 96) & (B * heads == 1) & (Tk == 77)                                  # the few-keys rule keeps the pair
    assert (ws[few & (Tq == 4096)] == 0).all() and (ws[few & (Tq == 256)] > 0).all() and (few & (Tq == 4096)).any()
    assert (bf_f == 1).any() and (bf_b == 1).any() and (ws[bf_b == 1] == 0).all()           # bf16 launches run the pair
    rg = (pad == 2) | (mis != 0) | ~np.isin(d, (16, 24, 32, 40, 48, 64, 80, 96, 128, 160, 192, 224, 256))
    assert (bf_f[rg] == 0).all() and (bf_b[rg] == 0).all() and (rg & (prec == 1)).any()     # RG launches answer fp32
    assert (bf_b[~rg & (prec == 1)] == 1).all() and (bf_b[prec == 0] == 0).all()
    assert (rg & (prec == 1) & (ws > 0)).any()                                              # ... and take the single-pass kernel
    assert (d == 257).any() and (ws[d == 257] == 0).all() and (bf_f[d == 257] == 0).all()  # unsupported head dim
