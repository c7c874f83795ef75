"""Host-side operators over the C ABI: raw launch wrappers (``*_raw``) and
``torch.autograd.Function`` s that chain them.  PyTorch supplies device memory, the
stream and the autograd graph; every FLOP runs in libgad_hip.so.

Layout: activations are contiguous fp32 NHWC tensors ``[B, H, W, C]`` (or ``[M, C]``),
conv weights are parameters of logical shape ``[Cout, Cin, KH, KW]`` whose storage is
``[Cout, KH, KW, Cin]`` (torch channels_last), Linear weights ``[out, in]``.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional

import torch

from . import _capi
from ._capi import (A_CONV, A_CONVT, A_KC, A_MC, B_CONV, B_KC, B_MC, B_WDGRAD, Adam8Args, AdamArgs, ConvGeom, GemmArgs,
                    GroupNormArgs, check)
from .shadows import (WEIGHT_EPOCH, Shadow, cached, in_flat_buffer as _in_flat_buffer, weight_key, written,  # noqa: F401
                      written_everywhere)

# ----------------------------------------------------------------------------------
# plumbing
# ----------------------------------------------------------------------------------
_WS = {}
WS_BYTES = 1 << 30


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


WS_OVERRIDE = [None]         # a caller-provided workspace that replaces the per-stream one (FusedTrainer's graph capture: the launches recorded
#                              into a hipGraph must not share scratch with other streams' work, whatever stream the capture ran on)


def workspace(device) -> torch.Tensor:
    """One caller-owned scratch buffer per device AND stream (split-K partials, reduction partials): launches on one stream are
    ordered, so they can share it; two coalitions in flight on two streams (a training phase beside a sampling phase,
    coalition.run_pipelined) must not.  Allocated once per stream so that hipGraph replays see a fixed address."""
    if WS_OVERRIDE[0] is not None:
        return WS_OVERRIDE[0]
    stream = _raw_stream(device.index if device.index is not None else torch.cuda.current_device()) if _raw_stream is not None \
        else torch.cuda.current_stream(device).cuda_stream
    key = (device.type, device.index, stream)
    ws = _WS.get(key)
    if ws is None:
        ws = torch.empty(WS_BYTES, dtype=torch.uint8, device=device)
        _WS[key] = ws
    return ws


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _req(t: torch.Tensor, name: str):
    if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
        raise _capi.GadError(f"{name}: expected a contiguous fp32 device tensor, got {t.dtype} {t.device} "
                             f"contiguous={t.is_contiguous()}")
    return t


def weight_krsc(w: torch.Tensor) -> torch.Tensor:
    """View of a conv parameter as its physical [Cout, KH, KW, Cin] array (no copy)."""
    v = w.permute(0, 2, 3, 1)
    if not v.is_contiguous():
        raise _capi.GadError("conv weight storage must be [Cout,KH,KW,Cin] (channels_last)")
    return v


# ----------------------------------------------------------------------------------
# gradient sinks: when a parameter lives in a flat gradient buffer (training.flatten_params) its gradient
# kernels write straight into that slot while a FusedTrainer backward is running, and autograd is handed None for
# that parameter: no AccumulateGrad node runs, so there is no per-parameter clone / accumulate kernel and no
# memset of the flat buffer.  A second gradient for the same parameter within one step is added on top.
# Outside begin_/end_backward_step the sinks are ignored and .grad behaves as usual.
# ----------------------------------------------------------------------------------
_SINK_EPOCH = [0]        # sinks live on the parameter object: p._gad_sink (view), p._gad_sink_epoch (last write)
_SINK_ACTIVE = [False]


def begin_backward_step():
    """Call once per training step before backward(): marks every sink as not yet written and routes parameter
    gradients into the sinks until end_backward_step()."""
    _SINK_EPOCH[0] += 1
    _SINK_ACTIVE[0] = True


def end_backward_step():
    _SINK_ACTIVE[0] = False


# The per-sample sink (half.PerSampleSink, set by half.per_sample_gradients): while one is active the half-path LoRA linear writes
# the gradient of every SAMPLE of the batch into that sample's row of a [G][P] staging buffer (gad_hgemm_tn_seg) instead of
# the batch sum into the flat slot.  No other operator can produce per-sample gradients, so asking one for a parameter gradient
# in this mode is an error.
_PER_SAMPLE = [None]


def _sink(param):
    """(destination view or None, first_write flag)"""
    if _PER_SAMPLE[0] is not None and param is not None and param.requires_grad:
        raise _capi.GadError("per-sample gradient sink: only the LoRA matrices of the half-precision activation path have "
                             "per-sample gradients (csrc/half.hip: gad_hgemm_tn_seg)")
    v = getattr(param, "_gad_sink", None) if (param is not None and _SINK_ACTIVE[0]) else None
    if v is None:
        return None, True
    first = getattr(param, "_gad_sink_epoch", -1) != _SINK_EPOCH[0]
    param._gad_sink_epoch = _SINK_EPOCH[0]
    return v, first


def _deliver(param, grad):
    """Route a freshly computed gradient tensor: into the parameter's sink (returning None to autograd) if it has an
    active one, else back to autograd unchanged."""
    v, first = _sink(param)
    if v is None:
        return grad
    if first:
        v.copy_(grad)
    else:
        v.add_(grad)
    return None


# ----------------------------------------------------------------------------------
# raw contraction launches
# ----------------------------------------------------------------------------------
OPERAND_PRECISION = [0]      # 0: fp32 operands (reference default); 1: bf16 operands, fp32 storage (see gad.h); 2: bf16 ACTIVATIONS
#                              (gad/half.py: models that support it keep activations and their gradients in bf16; everything
#                              that still flows as fp32 - conv_in, the time-embedding MLP - runs as mode 1)


class operand_precision:
    """``with ops.operand_precision("bf16"):`` - the analogue of the reference's autocast
    (`--mixed_precision`, text_to_image/train_text_to_image_lora.py:659-668): contractions that have a bf16
    instance (conv forward, Linear forward, Q K^T) round A and B to bf16 in flight and accumulate in fp32;
    everything else, and all storage, stays fp32."""

    def __init__(self, name):
        if name not in ("f32", "fp32", "no", "bf16", "bf16-operands", "bf16-activations"):
            raise ValueError(f"operand precision {name!r}: use 'f32', 'bf16' (= 'bf16-activations') or 'bf16-operands'")
        self.value = {"bf16": 2, "bf16-activations": 2, "bf16-operands": 1}.get(name, 0)

    def __enter__(self):
        self.prev = OPERAND_PRECISION[0]
        OPERAND_PRECISION[0] = self.value
        return self

    def __exit__(self, *exc):
        OPERAND_PRECISION[0] = self.prev
        return False


def set_operand_precision(name):
    """Process-wide form of `operand_precision` for the entry points' --mixed_precision flag.  "fp16" maps to
    bf16: the MI355X-native 16-bit type, which with fp32's exponent range needs no loss scaling (the reference's
    GradScaler, accelerate's fp16 path).  "fp16" / "bf16" = half-precision ACTIVATIONS where the model supports them
    (UNet2DConditionModel: what the reference's SD jobs run) and bf16 operands elsewhere; "bf16-operands" = bf16
    operands with fp32 storage everywhere (the round-2..4 mode, kept for A/B)."""
    OPERAND_PRECISION[0] = 0 if name in (None, "no", "f32", "fp32") else operand_precision("bf16" if name in ("fp16", "bf16") else name).value


def half_activations() -> bool:
    """Is the half-precision activation path selected? (models that support it cast at their boundary: gad/sd.py)"""
    return OPERAND_PRECISION[0] == 2


# Kernel-family switches for A/B tools and the invariance tests (never set in production): they travel in the argument
# structs (gad_gemm_args.flags / gad_groupnorm_args.flags); the library itself reads no environment variable.
KERNEL_FLAGS = {"gemm": 0, "gn": 0, "native_dgrad": False, "two_kernel_attn_bwd": False, "narrow_attn_fwd": False, "no_wino4": False,
                "no_gn_wino": False}


class kernel_flags:
    """``with ops.kernel_flags(no_patch=True, tap_major_k=True, scalar_epilogue=True, general_loaders=True, gn_two_pass=True,
    native_dgrad=True): ...``  (native_dgrad is a host-side switch: data-gradient kernels instead of forward kernels on
    rotated weights, see `dgrad_as_forward`)"""

    def __init__(self, no_patch=False, tap_major_k=False, gn_two_pass=False, scalar_epilogue=False, general_loaders=False,
                 native_dgrad=False, two_kernel_attn_bwd=False, narrow_attn_fwd=False, no_wino=False, no_wino4=False, no_gn_wino=False):
        gemm = ((_capi.GEMM_NO_PATCH if no_patch else 0) | (_capi.GEMM_TAP_MAJOR_K if tap_major_k else 0)
                | (_capi.GEMM_NO_WINO if no_wino else 0)
                | (_capi.GEMM_SCALAR_EPILOGUE if scalar_epilogue else 0)
                | (_capi.GEMM_GENERAL_LOADERS if general_loaders else 0))
        self.values = {"gemm": gemm, "gn": _capi.GN_TWO_PASS if gn_two_pass else 0, "native_dgrad": native_dgrad,
                       "two_kernel_attn_bwd": two_kernel_attn_bwd, "narrow_attn_fwd": narrow_attn_fwd, "no_wino4": no_wino4,
                       "no_gn_wino": no_gn_wino}

    def __enter__(self):
        self.prev = dict(KERNEL_FLAGS)
        KERNEL_FLAGS.update(self.values)
        return self

    def __exit__(self, *exc):
        KERNEL_FLAGS.update(self.prev)
        return False


# Allocation hooks for the out-of-bounds canaries (tests/test_gpu_guards.py; never set in production): SCRATCH_ALLOC(kind,
# nbytes, device) -> uint8 tensor provides every caller-owned scratch region at EXACTLY the size the C ABI's *_bytes query
# returns (kind: "ws" split-K / reduction workspace, "wino" Winograd scratch, "attn_ws" dQ slabs); OUT_ALLOC(shape, device)
# provides output tensors.  The tests hand out views between poisoned guard bands and check the bands afterwards.
SCRATCH_ALLOC = None
OUT_ALLOC = None
OUT_ALLOC_DT = None          # the same for the half path's outputs: (shape, device, dtype) -> tensor (gad/half.py::_empty)


ROUTE_STATS = None         # a dict while tools/wino_route_stats.py counts which 3x3 launches take a Winograd route and who made their V


def _scratch(kind, nbytes, device):
    if SCRATCH_ALLOC is not None:
        return SCRATCH_ALLOC(kind, nbytes, device)
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def _out(shape, device):
    if OUT_ALLOC is not None:
        return OUT_ALLOC(tuple(shape), device)
    return torch.empty(tuple(shape), device=device, dtype=torch.float32)


def gemm_raw(A, B, Cout, a_mode, b_mode, M, N, K, lda, ldb, ldc, *, geom: Optional[ConvGeom] = None, alpha=1.0,
             bias=None, rowadd=None, rows_per_group=1, residual=None, ldr=0, batch=1, batch_inner=1,
             sA=(0, 0), sB=(0, 0), sC=(0, 0), tile_hint=0, splitk_hint=0, A2=None, a_split=0, B_bf16=None,
             A_k2=None, B_k2=None, k_split=0, force_f32=False, launch=True) -> GemmArgs:
    """One fp32 contraction: fills its argument struct (the stream's workspace attached) and launches it (`_launch_gemm`).
    `launch=False`: only the arguments - the convolution wrappers put a Winograd offer between the two.
    `force_f32`: exact fp32 products whatever the process-wide operand precision (small parameter-gradient products)."""
    ws = workspace(A.device)
    a = GemmArgs()
    a.A, a.B, a.C = A.data_ptr(), B.data_ptr(), Cout.data_ptr()
    a.a_mode, a.b_mode = a_mode, b_mode
    a.M, a.N, a.K = M, N, K
    a.lda, a.ldb, a.ldc = lda, ldb, ldc
    a.batch, a.batch_inner = batch, batch_inner
    a.strideA0, a.strideA1 = sA
    a.strideB0, a.strideB1 = sB
    a.strideC0, a.strideC1 = sC
    if geom is not None:
        a.g = geom
    a.alpha = alpha
    a.bias, a.rowadd, a.residual = _ptr(bias), _ptr(rowadd), _ptr(residual)
    a.rows_per_group = rows_per_group
    a.ld_rowadd = (rowadd.stride(0) if rowadd.ndim == 2 else rowadd.shape[-1]) if rowadd is not None else 0      # (a column block of a wider matrix: nn.UNet2DModel._temb_rows)
    a.ldr = ldr
    a.ws, a.ws_bytes = ws.data_ptr(), ws.numel()
    a.tile_hint, a.splitk_hint = tile_hint, splitk_hint
    a.operand_precision = 1 if (OPERAND_PRECISION[0] and not force_f32) else 0
    a.flags = KERNEL_FLAGS["gemm"]
    if A2 is not None:
        a.A2, a.a_split, a.ldx2 = A2.data_ptr(), a_split, A2.shape[-1]
    if B_bf16 is not None:
        a.B_bf16 = B_bf16.data_ptr()
    if A_k2 is not None:            # K-concatenated operands (fused LoRA): k >= k_split reads A_k2 / B_k2
        a.A_k2, a.B_k2, a.k_split = A_k2.data_ptr(), B_k2.data_ptr(), k_split
        a.lda_k2, a.ldb_k2 = A_k2.shape[-1], B_k2.shape[-1]
    if launch:
        _launch_gemm(a, A.device, batch)
    return a


def _launch_gemm(a, device, batch=1):
    """What every fp32 contraction launch shares: the canary workspace, the profiler, gad_gemm."""
    lib = _capi.load()
    if SCRATCH_ALLOC is not None:    # canary runs: the workspace at exactly the size the planner asks for this launch
        need = lib.gad_gemm_workspace_bytes(C.byref(a))
        ws = _scratch("ws", need, device) if need else None
        a.ws, a.ws_bytes = (ws.data_ptr() if need else None), need
    if PROFILER is not None:
        PROFILER.gemm(lib, a, batch)
        return
    check(lib.gad_gemm(C.byref(a), _stream()), "gad_gemm")


class GemmProfiler:
    """Brackets every contraction launch with HIP events on the launch stream (bench.py's live
    per-kernel timing).  Keyed by the kernel instance the C side picks (modes, tile, vec)."""
    NAMES = {(A_CONV, B_KC): "conv_fwd", (A_CONVT, B_WDGRAD): "conv_dgrad", (A_MC, B_CONV): "conv_wgrad",
             (A_KC, B_KC): "gemm_nt", (A_KC, B_MC): "gemm_nn", (A_MC, B_MC): "gemm_tn"}

    def __init__(self):
        self.records = []          # (key, flops, algorithmic bytes, start_event, end_event)

    def gemm(self, lib, a, batch):
        tile, sk, vec = C.c_int32(), C.c_int32(), C.c_int32()
        check(lib.gad_gemm_plan(C.byref(a), C.byref(tile), C.byref(sk), C.byref(vec)), "gad_gemm_plan")
        kid = lib.gad_gemm_kernel_id(C.byref(a))
        s, e, mid = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True), None
        s.record()
        if kid in (5, 6) and not (a.flags & _capi.GEMM_WINO_SKIP_INPUT):
            # a Winograd forward launch as its two stages with an event between them - the same kernels in the same order as
            # the plain call (GAD_GEMM_WINO_ONLY_INPUT / _SKIP_INPUT): input transform (an HBM stream) | products + output transform
            flags = a.flags
            mid = torch.cuda.Event(enable_timing=True)
            a.flags = flags | _capi.GEMM_WINO_ONLY_INPUT
            check(lib.gad_gemm(C.byref(a), _stream()), "gad_gemm")
            mid.record()
            a.flags = flags | _capi.GEMM_WINO_SKIP_INPUT
            check(lib.gad_gemm(C.byref(a), _stream()), "gad_gemm")
            a.flags = flags
        else:
            check(lib.gad_gemm(C.byref(a), _stream()), "gad_gemm")
        e.record()
        name = self.NAMES.get((a.a_mode, a.b_mode), "gemm") + ("", "_bf16", f"_patch_w{a.g.Wo}", f"_patch_bf16_w{a.g.Wo}", f"_fewout_valu_w{a.g.Wo}", "_wino", "_wino4", "_wino4")[kid]   # (the Winograd kernels are one instance for every map width)
        key = (name, tile.value, sk.value, vec.value)
        # algorithmic bytes: every operand once (gathered tensor, not its im2col expansion) + the output
        g = a.g
        if a.a_mode in (A_CONV, A_CONVT):
            a_elems = (a.M // max(1, g.Ho * g.Wo)) * g.H * g.W * g.C
        else:
            a_elems = a.M * a.K
        b_elems = (a.K // max(1, g.Ho * g.Wo)) * g.H * g.W * g.C if a.b_mode == B_CONV else a.N * a.K
        extra = a.M * a.N if a.residual else 0
        nbytes = 4.0 * max(1, batch) * (a_elems + b_elems + a.M * a.N + extra)
        flops = 2.0 * a.M * a.N * a.K * max(1, batch)
        # the MFMA work actually issued: Winograd F(4x4) multiplies 36 positions per 4x4 tile where the direct form multiplies
        # 16 x 9 (36/144), F(2x2) 16 per 2x2 tile instead of 36; the weight gradient's F(4x4) form likewise
        executed = flops * ({5: 16.0 / 36.0, 6: 0.25, 7: 0.25}.get(kid, 1.0))
        stage = None
        if kid in (5, 6):
            npos, tpx = (16, 4) if kid == 5 else (36, 16)
            v_bytes = 4.0 * npos * (a.M // tpx) * g.C
            # input stage: x in, V out (None: another kernel - GroupNorm - wrote V) | rest: V, U in, y out (+ residual in; the product
            # panels of the three-launch forms go out and back in on top of that: not algorithmic)
            stage = (mid, 4.0 * a_elems + v_bytes if mid is not None else 0.0, v_bytes + 4.0 * (b_elems * npos / 9.0 + a.M * a.N + extra))
        self.records.append((key, flops, nbytes, s, e, executed, stage))

    def hgemm(self, lib, a, tn=False):
        """Bracket a half-precision-path contraction (gad_hgemm / gad_hgemm_tn): bf16 operands and output (fp32 output for parameter gradients)."""
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        if tn:
            s.record()
            check(lib.gad_hgemm_tn(C.byref(a), _stream()), "gad_hgemm_tn")
            e.record()
            nbytes = 2.0 * a.K * (a.M + a.N) + 4.0 * a.M * a.N
            flops = 2.0 * a.M * a.N * a.K
            self.records.append((("hgemm_tn_wgrad", 128, 0, 8), flops, nbytes, s, e, flops, None))
            return
        tile, sk = C.c_int32(), C.c_int32()
        check(lib.gad_hgemm_plan(C.byref(a), C.byref(tile), C.byref(sk)), "gad_hgemm_plan")
        s.record()
        check(lib.gad_hgemm(C.byref(a), _stream()), "gad_hgemm")
        e.record()
        if a.conv:
            name = f"hconv{a.KH}x{a.KW}" + ("_s2dgrad" if a.conv == 2 else "_s2" if a.stride == 2 else "_up" if a.upsample else "")
            a_elems = (a.M // max(1, a.Ho * a.Wo)) * a.H * a.W * a.Cin
        else:
            name = "hgemm_wgrad" if a.out_f32 else "hgemm_lora" if a.A2 else "hgemm"
            a_elems = a.M * a.K
        nbytes = 2.0 * (a_elems + a.N * a.K + (a.M * a.N if a.residual else 0)) + (4.0 if a.out_f32 else 2.0) * a.M * a.N
        flops = 2.0 * a.M * a.N * a.K
        self.records.append(((name, {1: 128, 2: 320, 5: 256320, 6: 256320, 7: 320, 8: 128, 9: 128}[tile.value], sk.value, 8), flops, nbytes, s, e, flops, None))

    def attention(self, fn, a, what, elem_bytes=4):
        """Bracket a fused attention launch.  Algorithmic FLOPs: forward 4 B h Tq Tk d (Q K^T and P V), backward
        10 B h Tq Tk d (the five products of the minimal scheme; the recomputing kernels execute seven).  Bytes: q, k,
        v, o once forward; those plus dO, dq, dk, dv backward."""
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        check(fn(C.byref(a), _stream()), f"gad_attention_{what}")
        e.record()
        d_alg = getattr(a, "alg_d", a.d)               # zero-padded heads (ops.PadHeadsFn): count the TRUE head dim's FLOPs
        unit = float(a.B) * a.heads * a.Tq * a.Tk * d_alg
        qb, kb = float(elem_bytes) * a.B * a.Tq * a.heads * d_alg, float(elem_bytes) * a.B * a.Tk * a.heads * d_alg
        flops, nbytes = (4.0 * unit, 2 * qb + 2 * kb) if what == "fwd" else (10.0 * unit, 4 * qb + 4 * kb)
        self.records.append(((f"attn_{what}_d{d_alg}", a.Tq, a.Tk, elem_bytes), flops, nbytes, s, e, flops, None))

    def summary(self):
        """{key: dict(launches, ms, flops, bytes, executed[, ms_input, bytes_input, bytes_rest])} - call after a device
        synchronize.  flops = algorithmic (2 M N K of the direct form), executed = the MFMA work issued; Winograd forward
        launches also carry the duration and the stream bytes of their input-transform stage."""
        out = {}
        for key, fl, nb, s, e, ex, stage in self.records:
            d = out.setdefault(key, dict(launches=0, ms=0.0, flops=0.0, bytes=0.0, executed=0.0))
            d["launches"] += 1
            d["ms"] += s.elapsed_time(e)
            d["flops"] += fl
            d["bytes"] += nb
            d["executed"] += ex
            if stage is not None:
                d["bytes_rest"] = d.get("bytes_rest", 0.0) + stage[2]
                d.setdefault("ms_input", 0.0)
                d.setdefault("bytes_input", 0.0)
                d.setdefault("n_input", 0)
                if stage[0] is not None:                 # this launch ran its own input transform
                    d["ms_input"] += s.elapsed_time(stage[0])
                    d["bytes_input"] += stage[1]
                    d["n_input"] += 1
        return out


PROFILER = None


def _conv_out_size(h, k, stride, pad_lo, pad_hi):
    return (h + pad_lo + pad_hi - k) // stride + 1


def _conv_fwd_args(x, x_shape, w, bias, stride, pad, upsample, rowadd, residual, tile_hint, splitk_hint, x2=None):
    """-> (y, its gad_gemm arguments) for the forward convolution of the [B,H,W,C1] tensor at `x` - only its address and device
    are read, so the caller may hold it in another form."""
    Bn, H, W, C1 = x_shape
    Cin = C1
    if x2 is not None:
        _req(x2, "conv x2")
        if x2.shape[:3] != x_shape[:3]:
            raise _capi.GadError(f"conv x2 {tuple(x2.shape)} does not match x {tuple(x_shape)}")
        Cin = C1 + x2.shape[-1]
    wk = weight_krsc(w)
    Cout, KH, KW, wc = wk.shape
    if wc != Cin:
        raise _capi.GadError(f"conv weight expects {wc} input channels, got {Cin}")
    He, We = (2 * H, 2 * W) if upsample else (H, W)
    Ho = _conv_out_size(He, KH, stride, pad[0], pad[1])
    Wo = _conv_out_size(We, KW, stride, pad[2], pad[3])
    y = _out((Bn, Ho, Wo, Cout), x.device)
    g = ConvGeom(H, W, Cin, C1, Ho, Wo, KH, KW, stride, pad[0], pad[2], int(upsample))
    if residual is not None:
        _req(residual, "conv residual")
    return y, gemm_raw(x, wk, y, A_CONV, B_KC, Bn * Ho * Wo, Cout, KH * KW * Cin, 0, KH * KW * Cin, Cout, geom=g,
                       bias=bias, rowadd=rowadd, rows_per_group=Ho * Wo, residual=residual, ldr=Cout,
                       tile_hint=tile_hint, splitk_hint=splitk_hint, A2=x2, a_split=C1, launch=False,
                       B_bf16=bf16_weight(w) if (OPERAND_PRECISION[0] >= 1 and KH == 3 and Cin % 32 == 0 and x2 is None
                                                 and not torch.cuda.is_current_stream_capturing()) else None)


def conv2d_fwd_raw(x, w, bias, stride=1, pad=(1, 1, 1, 1), upsample=False, rowadd=None, residual=None,
                   tile_hint=0, splitk_hint=0, x2=None, keep_v=None):
    """x [B,H,W,Cin] -> y [B,Ho,Wo,Cout]; pad = (top, bottom, left, right).
    x2 [B,H,W,C2]: the conv input is cat([x, x2], channels) without materialising it (UpBlock2D's skip concat).
    `keep_v` (a list): a launch that takes an F(4x4) Winograd route appends its scratch - the transformed input V at its start -
    for the weight gradient of the same convolution, which takes it as `wino_v` and skips its own input transform (Conv2dFn)."""
    _req(x, "conv x")
    y, a = _conv_fwd_args(x, x.shape, w, bias, stride, pad, upsample, rowadd, residual, tile_hint, splitk_hint, x2)
    form = wino_prefilter(w.shape[2:], stride, pad, x2 is not None, w.shape[0], w.shape[1], y.shape[1:3], tile_hint, splitk_hint)[0]
    V = _offer_wino(a, x.device, w, form)
    if keep_v is not None and V is not None and form == 4:
        keep_v.append(V)
    _launch_gemm(a, x.device)
    return y


def bf16_weight(w):
    """bf16 (RNE) copy of a conv weight in its [Cout][KH][KW][Cin] storage: the bf16-mode patch convolution streams it by
    LDS-DMA instead of rounding the fp32 weights in every workgroup.  A parameter that lives in a flat buffer
    (training.flatten_params) is served from ONE bf16 shadow of the whole buffer, refreshed by a single cast when the
    weights changed (`Shadow.fresh_for`) - so training pays one cast per step, not one per layer; any other parameter
    caches its own copy."""
    if _in_flat_buffer(w):
        flat, off, n = w._gad_flat
        s = (getattr(flat, "_gad_bf16", None) or _bf16_shadow(flat)).fresh_for(flat, off, w)
        o, i, kh, kw = w.shape
        return s.buffers[0][off:off + n].view(o, kh, kw, i)
    return cached(w, "_gad_bf16", lambda: weight_krsc(w).detach().to(torch.bfloat16).contiguous())


def _bf16_shadow(flat):
    copy = torch.empty(flat.numel(), device=flat.device, dtype=torch.bfloat16)
    flat._gad_bf16 = s = Shadow((copy,), lambda home: copy.copy_(home.detach()))
    return s


def dgrad_as_forward(w, stride, pad) -> bool:
    """The data gradient of a 3x3 / stride-1 / pad-1 convolution is the FORWARD convolution of dy with the 180-degree-
    rotated, channel-transposed weight, and the forward patch kernels (4 x 1 waves, [n][k] weight tiles read as b128, 96 /
    128 / 160-channel tiles - no padding at the pruned widths 96 / 192 / 288; in bf16 mode the LDS-DMA bf16 weight stream)
    are faster than the data-gradient instances (128-column tiles, [k][n] weight tiles read as dwords).  Taken when the
    rotated copy is cheap: a FROZEN weight (the SD base U-Net under LoRA: made once) or one living in a flat parameter
    buffer (training.flatten_params: ONE launch per optimizer step rotates every 3x3 weight of the model,
    `gad_rotate_conv3x3`).  `kernel_flags(native_dgrad=True)` keeps the data-gradient kernels (A/B tools, tests)."""
    return (tuple(w.shape[2:]) == (3, 3) and stride == 1 and tuple(pad) == (1, 1, 1, 1) and w.shape[0] % 32 == 0
            and w.shape[1] >= 64 and (not w.requires_grad or _in_flat_buffer(w)) and not KERNEL_FLAGS["native_dgrad"])


def _rotate_conv3x3(flat, out, table, tiles):
    check(_capi.load().gad_rotate_conv3x3(flat.data_ptr(), out.data_ptr(), table.data_ptr(), tiles, _stream()), "gad_rotate_conv3x3")


def _rotated_shadow(flat):
    """The rotated shadow of a flat buffer is itself the home of further shadows (its bf16 cast, its Winograd forms): it carries
    the 3x3 resident list with the channel roles swapped, and every refresh announces that it was written."""
    rows = [(off, co, ci, a, b) for off, co, ci in _conv3x3_residents(flat) for a in range(0, co, 32) for b in range(0, ci, 32)]
    table = torch.tensor(rows, dtype=torch.int64, device=flat.device)
    out = torch.empty_like(flat)
    out._gad_conv3x3 = [(off, ci, co) for off, co, ci in _conv3x3_residents(flat)]      # rotated: [Cin][3][3][Cout]

    def refresh(home):
        _rotate_conv3x3(home, out, table, len(rows))
        written(out)
    flat._gad_rot = s = Shadow((out,), refresh)
    return s


def rotated_weight(w):
    """W'[ci][2-r][2-s][co] = W[co][r][s][ci] as a conv parameter of logical shape [Cin, Cout, 3, 3] (storage
    [Cin][3][3][Cout]).  A weight living in a flat parameter buffer is served from ONE rotated shadow of the buffer,
    refreshed by a single launch when the weights changed (`Shadow.fresh_for`; the returned view carries `_gad_flat`, so
    bf16 mode casts the whole shadow once, too); any other weight caches its own copy per version."""
    if _in_flat_buffer(w):
        flat, off, n = w._gad_flat
        s = (getattr(flat, "_gad_rot", None) or _rotated_shadow(flat)).fresh_for(flat, off, w)
        view = s.views.get(off)
        if view is None:
            co, ci = w.shape[0], w.shape[1]
            view = s.views[off] = s.buffers[0][off:off + n].view(ci, 3, 3, co).permute(0, 3, 1, 2)
            view._gad_flat = (s.buffers[0], off, n)
        return view
    # storage [Cin][KH][KW][Cout]
    return cached(w, "_gad_rot", lambda: weight_krsc(w).detach().flip(1, 2).permute(3, 1, 2, 0).contiguous().permute(0, 3, 1, 2))


def _conv3x3_residents(flat):
    """[(offset, Cout, Cin)] of the 3x3 conv weights stored in a flat parameter buffer ([Cout][3][3][Cin] each); a rotated
    shadow (`rotated_weight`) carries the list of its source with the channel roles swapped."""
    r = getattr(flat, "_gad_conv3x3", None)
    if r is None:
        r = [(off, p_.shape[0], p_.shape[1]) for p_, off, _ in getattr(flat, "_gad_params", ())
             if p_.ndim == 4 and tuple(p_.shape[2:]) == (3, 3)]
        flat._gad_conv3x3 = r
    return r


# ----------------------------------------------------------------------------------
# Winograd routes of the 3x3 convolutions: the host offers (`wino_prefilter`), the library's planner decides per launch, and
# the offer RETURNS the scratch the planner asked for - its caller holds it until the launch is enqueued (stream-ordered:
# safe to drop then) or hands it on as `keep_v`.
# ----------------------------------------------------------------------------------
def _wino_ok(co, ci):
    return ci % 32 == 0 and co % 4 == 0 and co >= 64


def wino_prefilter(kernel, stride, pad, two_source, Cout, Cin, out_map, tile_hint=0, splitk_hint=0):
    """-> (form, wgrad): the Winograd form of the weight the host offers a FORWARD launch of this convolution - 0 none, 2 F(2x2),
    4 F(4x4) - and whether it opts the convolution's WEIGHT GRADIENT into its F(4x4) form.  A pre-filter: it keeps the host
    from transforming weights and asking where the answer cannot be yes; the planner decides (`gad_gemm_wino_bytes`), and never
    takes what this withholds (tests/test_conv_launch_cpu.py).  F(4x4) wherever the output map is a multiple of 4 (it measured
    faster than F(2x2) at every shape of tools/ab_winograd.py), F(2x2) for the other maps; tile hints 7 / 8-11 force a form."""
    flags = KERNEL_FLAGS["gemm"]
    if (tuple(kernel) != (3, 3) or stride != 1 or tuple(pad) != (1, 1, 1, 1) or splitk_hint != 0 or OPERAND_PRECISION[0] >= 1
            or flags & (_capi.GEMM_NO_WINO | _capi.GEMM_NO_PATCH | _capi.GEMM_SCALAR_EPILOGUE | _capi.GEMM_TAP_MAJOR_K)):
        return 0, False
    f4_maps = out_map[0] % 4 == 0 and out_map[1] % 4 == 0 and not KERNEL_FLAGS["no_wino4"]
    wgrad = f4_maps and tile_hint in (0, 8) and not flags & _capi.GEMM_GENERAL_LOADERS
    if two_source or not _wino_ok(Cout, Cin) or tile_hint not in (0, 7, 8, 9, 10, 11):
        return 0, wgrad
    if f4_maps and tile_hint != 7:
        return 4, wgrad
    return (2 if tile_hint in (0, 7) else 0), wgrad


def _count_wino4(a, kid):
    if ROUTE_STATS is not None:      # tools/wino_route_stats.py
        key = (kid, a.M, a.N, a.K, bool(a.flags & _capi.GEMM_WINO_SKIP_INPUT), torch.is_grad_enabled())
        ROUTE_STATS[key] = ROUTE_STATS.get(key, 0) + 1


def _offer_wino(a, device, w, form, supplied=False):
    """The forward offer: attach the weight's Winograd `form`, ask the planner once, allocate the scratch it wants -> that scratch
    (the launch is on the form's route), or None with the pointers cleared.  `supplied`: the caller's own kernel writes the
    F(4x4) input image V into the scratch and the launch starts behind its input stage; any other route counts as declined."""
    U = wino_weight(w, form, offered=True) if form else None
    if U is None:
        return None
    setattr(a, "B_wino" if form == 2 else "B_wino4", U.data_ptr())
    need = _capi.load().gad_gemm_wino_bytes(C.byref(a))
    if not need or (supplied and form != 4):
        a.B_wino = a.B_wino4 = None
        return None
    V = _scratch("wino", need, device)
    a.wino_ws, a.wino_ws_bytes = V.data_ptr(), need
    if form == 4:
        a.flags |= _capi.GEMM_WINO_SKIP_INPUT if supplied else 0
        _count_wino4(a, 6)
    return V


def _opt_in_wino_wgrad(a, device, wino_v):
    """The weight gradient's opt-in, in the same shape: -> the scratch, or None with the flag cleared.  `wino_v`, the scratch a
    forward launch kept, replaces the input transform if it holds the whole image V: [36][pixels / 16][Cin] fp32."""
    a.flags |= _capi.GEMM_WINO_WGRAD
    need = _capi.load().gad_gemm_wino_bytes(C.byref(a))
    if not need:
        a.flags &= ~_capi.GEMM_WINO_WGRAD
        return None
    ws = _scratch("wino", need, device)
    a.wino_ws, a.wino_ws_bytes = ws.data_ptr(), need
    if wino_v is not None and wino_v.numel() >= 36 * (a.K // 16) * a.g.C * 4:
        a.B_wino4 = wino_v.data_ptr()
        a.flags |= _capi.GEMM_WINO_SKIP_INPUT
    _count_wino4(a, 7)
    return ws


def gn_silu_conv3x3_raw(x, x2, gamma, beta, G, eps, w, bias, rowadd=None, residual=None, tile_hint=0):
    """conv3x3(SiLU(GroupNorm(cat([x, x2])))) + bias + rowadd + residual, forward only (the sampler's ResnetBlock2D halves:
    reference diffusers ResnetBlock2D.forward, norm1 -> silu -> conv1 (+ temb) and norm2 -> silu -> conv2 (+ shortcut)).
    Where the convolution takes an F(4x4) Winograd route and the norm has a plan for it (`gad_groupnorm_wino4_ok`), GroupNorm
    writes the route's transformed input V directly - the normalised activation never exists in HBM and the route's input
    transform launch disappears; otherwise the two ordinary launches run.  Same results to fp32 rounding either way."""
    _req(x, "groupnorm x")
    Bn, H, W, C1 = x.shape
    Cin = C1 + (x2.shape[-1] if x2 is not None else 0)
    lib = _capi.load()

    def plain():
        h = group_norm_cat_raw(x, x2, gamma, beta, G, eps, True) if x2 is not None else group_norm(x, gamma, beta, G, eps, True)
        return conv2d_fwd_raw(h, w, bias, 1, (1, 1, 1, 1), False, rowadd=rowadd, residual=residual, tile_hint=tile_hint)
    form = wino_prefilter(w.shape[2:], 1, (1, 1, 1, 1), False, w.shape[0], Cin, (H, W), tile_hint)[0]
    if torch.is_grad_enabled() or w.shape[1] != Cin or KERNEL_FLAGS["gn"] or KERNEL_FLAGS["no_gn_wino"] or H % 4 or W % 4 or not form:
        return plain()
    mean = torch.empty((Bn, G), device=x.device, dtype=torch.float32)
    rstd = torch.empty_like(mean)
    gn = GroupNormArgs()
    gn.x, gn.gamma, gn.beta, gn.mean, gn.rstd = x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), mean.data_ptr(), rstd.data_ptr()
    gn.B, gn.HW, gn.C, gn.G, gn.eps, gn.silu = Bn, H * W, Cin, G, eps, 1
    if x2 is not None:
        _req(x2, "groupnorm x2")
        gn.x2, gn.C1 = x2.data_ptr(), C1
    if not lib.gad_groupnorm_wino4_ok(C.byref(gn), W):
        return plain()
    # the convolution's input is only a shape here: its first stage is the norm's launch
    y, a = _conv_fwd_args(x, (Bn, H, W, Cin), w, bias, 1, (1, 1, 1, 1), False, rowadd, residual, tile_hint, 0)
    V = _offer_wino(a, x.device, w, form, supplied=True)
    if V is None:
        return plain()
    check(lib.gad_groupnorm_silu_wino4(C.byref(gn), V.data_ptr(), W, _stream()), "gad_groupnorm_silu_wino4")
    _launch_gemm(a, x.device)
    return y


def _wino_shadow(src, items, f):
    """The Winograd forms of items [(offset in src, Cout, Cin)]: U, {offset: (offset in U, floats)} and the tile table are built
    once; f = 2 or 4.  `src` is a buffer, or a conv parameter standing for its own storage."""
    launch, npos = (_capi.load().gad_wino_weights, 16) if f == 2 else (_capi.load().gad_wino4_weights, 36)
    rows, where, doff = [], {}, 0
    for off, co, ci in items:
        where[off] = (doff, npos * co * ci)
        rows += [(off, doff, co, ci, a, b) for a in range(0, co, 32) for b in range(0, ci, 32)]
        doff += npos * co * ci
    U = torch.empty(max(doff, 1), device=src.device, dtype=torch.float32)
    table = torch.tensor(rows, dtype=torch.int64, device=src.device)
    return Shadow((U,), lambda home: check(launch(home.data_ptr(), U.data_ptr(), table.data_ptr(), len(rows), _stream()),
                                           "gad_wino_weights"), where)


def wino_weight(w, f=2, offered=False):
    """The Winograd form U = G w G^T of a 3x3 conv weight: [16][Cout][Cin] for F(2x2, 3x3) (`gad_wino_weights`, f = 2) or
    [36][Cout][Cin] for F(4x4, 3x3) (`gad_wino4_weights`, f = 4); None for a weight no forward launch is offered that form of
    (`wino_prefilter`: Cin % 32, Cout % 4, < 64 output channels, bf16-operand mode, the no_wino switches).  A weight living in
    a flat parameter buffer - or in the rotated shadow of one, for the data gradients - is served from ONE transformed shadow of
    that buffer per form, refreshed by a single launch when the weights changed (`Shadow.fresh_for`); any other weight keeps
    its own transform, rewritten in place per version.  `offered`: the caller has asked the pre-filter for this launch."""
    co, ci = w.shape[0], w.shape[1]
    if not offered and wino_prefilter(w.shape[2:], 1, (1, 1, 1, 1), False, co, ci, (f, f))[0] != f:
        return None
    attr = "_gad_wino" if f == 2 else "_gad_wino4"
    if _in_flat_buffer(w):
        flat, off, n = w._gad_flat
        s = getattr(flat, attr, None)
        if s is None:
            s = _wino_shadow(flat, [it for it in _conv3x3_residents(flat) if _wino_ok(it[1], it[2])], f)
            setattr(flat, attr, s)
        if off not in s.where:
            return None
        d0, dn = s.where[off]
        return s.fresh_for(flat, off, w).buffers[0][d0:d0 + dn]
    return cached(w, attr, lambda: _wino_shadow(w, [(0, co, ci)], f), lambda s: s.refresh(weight_krsc(w))).buffers[0]


def refresh_wino(module):
    """Bring the Winograd shadows of every 3x3 weight of `module` up to date NOW - before replaying a captured graph, whose
    launches read the shadow at a fixed address but cannot notice that the weights moved since the capture."""
    for p in module.parameters():
        if p.ndim == 4 and tuple(p.shape[2:]) == (3, 3):
            home = p._gad_flat[0] if _in_flat_buffer(p) else p
            for f, attr in ((2, "_gad_wino"), (4, "_gad_wino4")):
                if getattr(home, attr, None) is not None:            # a shadow some launch has used
                    wino_weight(p, f)


def _dense_1x1(KH, KW, stride, pad, upsample, Cin, Cout) -> bool:
    """A 1x1 / stride-1 convolution (ResNet shortcuts, proj_in / proj_out of the SD transformer blocks) is a dense GEMM over
    the pixel rows: its gradients run on the lean dense loaders instead of the im2col gathers."""
    return (KH == 1 and KW == 1 and stride == 1 and tuple(pad) == (0, 0, 0, 0) and not upsample and Cin % 4 == 0 and Cout % 4 == 0
            and not KERNEL_FLAGS["gemm"] & _capi.GEMM_GENERAL_LOADERS)


def two_source_ok(c1: int, c2: int) -> bool:
    """Can conv2d_fwd_raw(x, ..., x2=) gather this channel split? (32-channel K steps must not straddle it)"""
    return c1 % 32 == 0 and c2 % 32 == 0


def conv2d_dgrad_raw(dy, w, x_shape, stride=1, pad=(1, 1, 1, 1), upsample=False, tile_hint=0, splitk_hint=0):
    """dy [B,Ho,Wo,Cout] -> dx [B,H,W,Cin] (sums the 2x2 replicas if the conv was upsample-fused)."""
    _req(dy, "conv dy")
    Bn, H, W, Cin = x_shape
    wk = weight_krsc(w)
    Cout, KH, KW, _ = wk.shape
    _, Ho, Wo, _ = dy.shape
    He, We = (2 * H, 2 * W) if upsample else (H, W)
    dxe = _out((Bn, He, We, Cin), dy.device)
    if _dense_1x1(KH, KW, stride, pad, upsample, Cin, Cout):      # dx = dy W
        gemm_raw(dy, wk, dxe, A_KC, B_MC, Bn * H * W, Cin, Cout, Cout, Cin, Cin, tile_hint=tile_hint, splitk_hint=splitk_hint)
        return dxe
    g = ConvGeom(Ho, Wo, Cout, Cout, He, We, KH, KW, stride, pad[0], pad[2], 0)
    gemm_raw(dy, wk, dxe, A_CONVT, B_WDGRAD, Bn * He * We, Cin, KH * KW * Cout, 0, 0, Cin, geom=g,
             tile_hint=tile_hint, splitk_hint=splitk_hint)
    return _upsample2x_bwd(dxe, x_shape) if upsample else dxe


def _upsample2x_bwd(dxe, x_shape):
    """dxe [B,2H,2W,C], the gradient on the nearest-2x grid an upsample-fused conv ran on -> dx [B,H,W,C]: sums the 2 x 2 replicas."""
    Bn, H, W, Cin = x_shape
    dx = torch.empty((Bn, H, W, Cin), device=dxe.device, dtype=torch.float32)
    check(_capi.load().gad_upsample2x_bwd(dxe.data_ptr(), dx.data_ptr(), Bn, H, W, Cin, _stream()), "gad_upsample2x_bwd")
    return dx


def conv2d_wgrad_raw(dy, x, w_like, stride=1, pad=(1, 1, 1, 1), upsample=False, tile_hint=0, splitk_hint=0, out=None, wino_v=None):
    """dW with the parameter's logical shape [Cout,Cin,KH,KW] and channels_last storage; `out` = a
    [Cout,Cin,KH,KW] view with that storage to write into (flat gradient slot); `wino_v` = the scratch the forward launch of
    this convolution kept (`conv2d_fwd_raw(keep_v=)`): the Winograd form then reads the transformed input from it."""
    _req(dy, "conv dy")
    _req(x, "conv x")
    Bn, H, W, Cin = x.shape
    Cout, _, KH, KW = w_like.shape
    _, Ho, Wo, _ = dy.shape
    dwk = _out((Cout, KH, KW, Cin), dy.device) if out is None else weight_krsc(out)
    if _dense_1x1(KH, KW, stride, pad, upsample, Cin, Cout):
        gemm_raw(dy, x, dwk, A_MC, B_MC, Cout, Cin, Bn * H * W, Cout, Cin, Cin, tile_hint=tile_hint, splitk_hint=splitk_hint)   # dW = dy^T x
        return dwk.permute(0, 3, 1, 2)
    g = ConvGeom(H, W, Cin, Cin, Ho, Wo, KH, KW, stride, pad[0], pad[2], int(upsample))
    a = gemm_raw(dy, x, dwk, A_MC, B_CONV, Cout, KH * KW * Cin, Bn * Ho * Wo, Cout, 0, KH * KW * Cin, geom=g,
                 tile_hint=tile_hint, splitk_hint=splitk_hint, launch=False)
    if wino_prefilter((KH, KW), stride, pad, False, Cout, Cin, (Ho, Wo), tile_hint, splitk_hint)[1]:
        scratch = _opt_in_wino_wgrad(a, dy.device, wino_v)      # noqa: F841  (held until the launch is enqueued)
    _launch_gemm(a, dy.device)
    return dwk.permute(0, 3, 1, 2)


def colsum_raw(dy2d: torch.Tensor, segments=1, out=None):
    """[S*M, N] -> [S, N] column sums per segment (`out`: contiguous destination of S*N floats)."""
    lib = _capi.load()
    ws = workspace(dy2d.device)
    rows, N = dy2d.shape
    if out is None:
        out = torch.empty((segments, N), device=dy2d.device, dtype=torch.float32)
    check(lib.gad_colsum(dy2d.data_ptr(), out.data_ptr(), segments, rows // segments, N, ws.data_ptr(), ws.numel(),
                         _stream()), "gad_colsum")
    return out


def linear_fwd_raw(x2d, w, bias=None, residual=None, alpha=1.0, force_f32=False):
    M, K = x2d.shape
    N = w.shape[0]
    y = _out((M, N), x2d.device)
    gemm_raw(x2d, w, y, A_KC, B_KC, M, N, K, K, K, N, bias=bias, residual=residual, ldr=N, alpha=alpha, force_f32=force_f32)
    return y


# ---- eval launches of the score-tail networks (gad/inception.py, gad/vgg.py, gad/vit.py): each the one call site of its symbol
def conv_krsc_raw(x, w_krsc, bias, kh, kw, stride, pad_h, pad_w, out=None, c0=0):
    """x [B,H,W,Cin] * weights already laid out [Cout][KH][KW][Cin] -> channels [c0, c0 + Cout) of `out` [B,Ho,Wo,Ctot], or a
    tensor of its own; exact fp32, direct route (no Winograd operand)."""
    Bn, H, W, ci = x.shape
    co = w_krsc.shape[0]
    Ho, Wo = (H + 2 * pad_h - kh) // stride + 1, (W + 2 * pad_w - kw) // stride + 1
    if out is None:
        out = torch.empty((Bn, Ho, Wo, co), device=x.device, dtype=torch.float32)
    gemm_raw(x, w_krsc, out[..., c0:c0 + co], A_CONV, B_KC, Bn * Ho * Wo, co, kh * kw * ci, 0, kh * kw * ci, out.shape[-1],
             geom=ConvGeom(H, W, ci, ci, Ho, Wo, kh, kw, stride, pad_h, pad_w, 0), bias=bias, force_f32=True)
    return out


def relu_raw(t):
    """in place on a contiguous [..., C] tensor"""
    Cn = t.shape[-1]
    check(_capi.load().gad_relu(t.data_ptr(), t.numel() // Cn, Cn, Cn, _stream()), "gad_relu")
    return t


def pool2d_raw(x, out, c0, k, stride, pad, mode, relu_in=False):
    """k x k pool of x [B,H,W,C] into channels [c0, c0 + C) of `out` [B,Ho,Wo,Ctot]; relu_in: of relu(x)"""
    Bn, H, W, Cn = x.shape
    check(_capi.load().gad_pool2d(x.data_ptr(), out[..., c0:].data_ptr(), Bn, H, W, Cn, Cn, out.shape[-1], out.shape[1],
                                  out.shape[2], k, stride, pad, mode, int(relu_in), _stream()), "gad_pool2d")
    return out


def resize_bilinear_raw(x_nchw, R, a, b):
    """[B,C,H,W] -> NHWC [B,R,R,C] = a * bilinear(x) + b (align_corners=False)"""
    Bn, Cn, H, W = x_nchw.shape
    y = torch.empty((Bn, R, R, Cn), device=x_nchw.device, dtype=torch.float32)
    check(_capi.load().gad_resize_bilinear(x_nchw.data_ptr(), y.data_ptr(), Bn, Cn, H, W, R, R, a, b, _stream()),
          "gad_resize_bilinear")
    return y


def gelu_raw(h, kind):
    """in place on a contiguous [rows, C] tensor; kind: _capi.GELU_ERF | GELU_QUICK"""
    check(_capi.load().gad_gelu(h.data_ptr(), h.shape[0], h.shape[1], h.shape[1], kind, _stream()), "gad_gelu")
    return h


def l2_normalize_rows_raw(x2d):
    """in place on a contiguous [rows, C] fp32 device tensor"""
    _req(x2d, "l2_normalize input")
    check(_capi.load().gad_l2_normalize_rows(x2d.data_ptr(), x2d.shape[0], x2d.shape[1], x2d.shape[1], _stream()),
          "gad_l2_normalize_rows")
    return x2d


# ---- eval launches of the autoencoders (gad/vae.py)
def conv_direct_raw(x, w_krsc, bias, stride=1, pad=(1, 1, 1, 1), upsample=False, residual=None):
    """x [B,H,W,Cin] * weights already laid out [Cout][KH][KW][Cin] -> [B,Ho,Wo,Cout] (+ residual of that shape); pad = (top,
    bottom, left, right); `upsample`: the nearest-2x of x is folded into the gather.  Exact fp32, direct route (no Winograd
    operand)."""
    Bn, H, W, ci = x.shape
    co, kh, kw, wc = w_krsc.shape
    if wc != ci:
        raise _capi.GadError(f"conv weight expects {wc} input channels, got {ci}")
    He, We = (2 * H, 2 * W) if upsample else (H, W)
    Ho, Wo = _conv_out_size(He, kh, stride, pad[0], pad[1]), _conv_out_size(We, kw, stride, pad[2], pad[3])
    y = torch.empty((Bn, Ho, Wo, co), device=x.device, dtype=torch.float32)
    if residual is not None and tuple(residual.shape) != tuple(y.shape):
        raise _capi.GadError(f"conv residual {tuple(residual.shape)} does not match the output {tuple(y.shape)}")
    gemm_raw(x, w_krsc, y, A_CONV, B_KC, Bn * Ho * Wo, co, kh * kw * ci, 0, kh * kw * ci, co,
             geom=ConvGeom(H, W, ci, ci, Ho, Wo, kh, kw, stride, pad[0], pad[2], int(upsample)), bias=bias,
             residual=residual, ldr=co, force_f32=True)
    return y


def group_norm_raw(x, gamma, beta, G, eps, silu):
    """[SiLU](GroupNorm(x)) on contiguous NHWC [B, ..., C] (forward only, no autograd)"""
    _req(x, "groupnorm x")
    y = torch.empty_like(x)
    mean = torch.empty((x.shape[0], G), device=x.device, dtype=torch.float32)
    rstd = torch.empty_like(mean)
    a = _gn_args(x, y, gamma, beta, mean, rstd, G, eps, silu)
    check(_capi.load().gad_groupnorm_silu_fwd(C.byref(a), _stream()), "gad_groupnorm_silu_fwd")
    return y


def attention_d512_ok(d: int) -> bool:
    return bool(_capi.load().gad_attention_d512_supported(int(d)))


def _attention_eval_raw(symbol, q, k, v, Bn, heads, Tq, Tk, d, ldq, ldk, ldv, need_lse):
    """The forward-only, exact-fp32 attention entry point `symbol` on [Bn, T, *] views -> (o, lse or None)"""
    o = torch.empty((Bn, Tq, heads * d), device=q.device, dtype=torch.float32)
    lse = torch.empty((Bn, heads, Tq), device=q.device, dtype=torch.float32) if need_lse else None
    a = _attention_args(q, k, v, o, lse, Bn, heads, Tq, Tk, d, ldq, ldk, ldv, Tq * ldq, Tk * ldk, Tk * ldv)
    check(getattr(_capi.load(), symbol)(C.byref(a), _stream()), symbol)
    return o, lse


def attention_fwd_d512_raw(q, k, v, Bn, heads, Tq, Tk, d, ldq, ldk, ldv, need_lse=False):
    """`attention_fwd_raw` for the wide head the autoencoders' mid block has (d = 512): exact fp32, forward only.
    -> (o [Bn, Tq, heads*d], lse [Bn, heads, Tq] or None)"""
    return _attention_eval_raw("gad_attention_fwd_d512", q, k, v, Bn, heads, Tq, Tk, d, ldq, ldk, ldv, need_lse)


# ---- eval launches of the text towers (gad/text.py)
def attention_causal_ok(T: int, d: int) -> bool:
    return bool(_capi.load().gad_attention_causal_supported(int(T), int(d)))


def attention_causal_fwd_raw(q, k, v, Bn, heads, T, d, ldq, ldk, ldv, need_lse=False):
    """Causal self-attention (query i sees keys j <= i) on [Bn, T, *] views, exact fp32, forward only: T <= 128, d in
    {16, 32, 64}; q, k, v may be column blocks of one projection output as for `attention_fwd_raw`.  An unsupported launch is
    an error.  -> (o [Bn, T, heads*d], lse [Bn, heads, T] or None)"""
    return _attention_eval_raw("gad_attention_causal_fwd", q, k, v, Bn, heads, T, T, d, ldq, ldk, ldv, need_lse)


def attention_causal_qkv_raw(qkv, Bn, T, Cq, heads):
    """`attention_causal_fwd_raw` on the output of ONE fused projection [Bn*T, 3*Cq] (q | k | v along the columns), read in place"""
    _req(qkv, "causal attention qkv")
    d, ld = Cq // heads, 3 * Cq
    return attention_causal_fwd_raw(qkv[:, 0:Cq], qkv[:, Cq:2 * Cq], qkv[:, 2 * Cq:3 * Cq], Bn, heads, T, d, ld, ld, ld)[0]


def text_tokens_raw(ids, token_emb, pos):
    """ids [B, T] integers (host or device), token_emb [V, W], pos [T, W] -> [B*T, W] = token_emb[ids] + pos.  An id outside
    [0, V) is refused here, on the host (the kernel only clamps)."""
    _req(token_emb, "text token embedding")
    _req(pos, "text positional embedding")
    Bn, T = ids.shape
    V, W = token_emb.shape
    if tuple(pos.shape) != (T, W):
        raise _capi.GadError(f"text_tokens: {T} tokens of width {W} need a positional embedding [{T}, {W}], got {tuple(pos.shape)}")
    host = ids.detach().cpu()
    lo, hi = int(host.min()), int(host.max())
    if lo < 0 or hi >= V:
        raise _capi.GadError(f"text_tokens: token id {lo if lo < 0 else hi} is outside the vocabulary [0, {V})")
    dev_ids = host.to(torch.int32).contiguous().to(token_emb.device)
    out = torch.empty((Bn * T, W), device=token_emb.device, dtype=torch.float32)
    check(_capi.load().gad_text_tokens(dev_ids.data_ptr(), token_emb.data_ptr(), pos.data_ptr(), out.data_ptr(), Bn, T, W, V, _stream()),
          "gad_text_tokens")
    return out


def gather_rows_raw(x2d, rows, T):
    """x2d [B*T, W] contiguous, rows [B] integers in [0, T) (host or device) -> [B, W]: out[b] = x2d[b*T + rows[b]]"""
    _req(x2d, "gather_rows input")
    Bn, W = x2d.shape[0] // T, x2d.shape[1]
    host = rows.detach().cpu()
    if host.numel() != Bn or int(host.min()) < 0 or int(host.max()) >= T:
        raise _capi.GadError(f"gather_rows: {Bn} row indices in [0, {T}) are required")
    dev_rows = host.to(torch.int32).contiguous().to(x2d.device)
    out = torch.empty((Bn, W), device=x2d.device, dtype=torch.float32)
    check(_capi.load().gad_gather_rows(x2d.data_ptr(), dev_rows.data_ptr(), out.data_ptr(), Bn, T, W, W, _stream()), "gad_gather_rows")
    return out


def vq_lookup_raw(z2d, codebook):
    """z2d [n, D] (a row-strided view is read in place: NHWC latents), codebook [K, D] contiguous
    -> (idx int32 [n] of the nearest code, zq [n, D] = z + (codebook[idx] - z))"""
    n, D = z2d.shape
    if z2d.dtype != torch.float32 or codebook.dtype != torch.float32 or not codebook.is_contiguous() or (D > 1 and z2d.stride(1) != 1):
        raise _capi.GadError("vq_lookup: fp32 rows with unit column stride and a contiguous fp32 codebook are required")
    if codebook.ndim != 2 or codebook.shape[1] != D:
        raise _capi.GadError(f"vq_lookup: codebook {tuple(codebook.shape)} does not hold codes of {D}")
    idx = torch.empty((n,), device=z2d.device, dtype=torch.int32)
    zq = torch.empty((n, D), device=z2d.device, dtype=torch.float32)
    check(_capi.load().gad_vq_lookup(z2d.data_ptr(), z2d.stride(0) if n > 1 else D, codebook.data_ptr(), n, codebook.shape[0], D,
                                     idx.data_ptr(), zq.data_ptr(), D, _stream()), "gad_vq_lookup")
    return idx, zq


def layernorm_fwd_raw(x, gamma, beta, eps):
    """over the last axis of a contiguous tensor -> (y, mean [rows], rstd [rows])"""
    C_ = x.shape[-1]
    rows = x.numel() // C_
    y = torch.empty_like(x)
    stats = torch.empty((2, rows), device=x.device, dtype=torch.float32)
    check(_capi.load().gad_layernorm_fwd(x.data_ptr(), y.data_ptr(), gamma.data_ptr(), beta.data_ptr(), stats[0].data_ptr(),
                                         stats[1].data_ptr(), rows, C_, eps, _stream()), "gad_layernorm_fwd")
    return y, stats[0], stats[1]


def linear_dgrad_raw(dy2d, w):
    M, N = dy2d.shape
    K = w.shape[1]
    dx = _out((M, K), dy2d.device)
    gemm_raw(dy2d, w, dx, A_KC, B_MC, M, K, N, N, K, K)
    return dx


def linear_wgrad_raw(dy2d, x2d, out=None):
    M, N = dy2d.shape
    K = x2d.shape[1]
    dw = _out((N, K), dy2d.device) if out is None else out
    gemm_raw(dy2d, x2d, dw, A_MC, B_MC, N, K, M, N, K, K)
    return dw


# ----------------------------------------------------------------------------------
# autograd functions
# ----------------------------------------------------------------------------------
def _param_grad(param, compute):
    """compute(out) produces the gradient, writing into `out` when given.  With a sink: first gradient of the
    step goes straight into the slot, later ones are added."""
    v, first = _sink(param)
    if v is None:
        return compute(None)
    if first:
        compute(v)
    else:
        v.add_(compute(None))
    return None


def _conv_backward(ctx, dy, x, x_shape, w, stride, pad, upsample, has, need):
    """Backward of y = conv(x) + bias + rowadd[b] + residual for Conv2dFn and GnSiluConv3x3Fn -> (dx, dw, d bias, d rowadd,
    d residual).  `has` / `need`: which of (bias, rowadd, residual) the forward had, and which of
    (x, w, bias, rowadd, residual) want a gradient; `x` (the conv's input) is read only for the weight gradient, which takes the
    transformed input the forward launch kept (`ctx.wino_v`) in its Winograd form."""
    dy = dy.contiguous()
    dx = None
    if need[0]:
        if dgrad_as_forward(w, stride, pad):
            dx = conv2d_fwd_raw(dy, rotated_weight(w), None)
            if upsample:
                dx = _upsample2x_bwd(dx, x_shape)
        else:
            dx = conv2d_dgrad_raw(dy, w, x_shape, stride, pad, upsample)
    V, ctx.wino_v = ctx.wino_v, None
    dw = _param_grad(w, lambda o: conv2d_wgrad_raw(dy, x, w, stride, pad, upsample, out=o, wino_v=V)) if need[1] else None
    db, dr = _conv_epilogue_grads(dy, ctx.bias_ref, has[0] and need[2], has[1] and need[3])
    dres = dy if (has[2] and need[4]) else None
    return dx, dw, db, dr, dres


class Conv2dFn(torch.autograd.Function):
    """y = conv(x) + bias + rowadd[b] (time-embedding add) + residual, all fused in the
    contraction epilogue (ResnetBlock2D / Downsample2D / Upsample2D)."""

    @staticmethod
    def forward(ctx, x, w, bias, rowadd, residual, stride, pad, upsample):
        ctx.save_for_backward(x, w)
        ctx.bias_ref = bias
        ctx.cfg = (stride, pad, upsample, (bias is not None, rowadd is not None, residual is not None))
        # an F(4x4) forward launch leaves the transformed input V in its scratch: kept for the weight gradient, which would make
        # the same image from x again
        keep = [] if ctx.needs_input_grad[1] else None
        y = conv2d_fwd_raw(x, w, bias, stride, pad, upsample, rowadd, residual, keep_v=keep)
        ctx.wino_v = keep[0] if keep else None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        stride, pad, upsample, has = ctx.cfg
        return (*_conv_backward(ctx, dy, x, x.shape, w, stride, pad, upsample, has, ctx.needs_input_grad[:5]), None, None, None)


def _conv_epilogue_grads(dy, bias, need_bias, need_rowadd):
    """-> (d bias, d rowadd) of y = conv(x) + bias + rowadd[b]: column sums of dy, per image for the time-embedding row."""
    Bn, Ho, Wo, Cout = dy.shape
    db = dr = None
    if need_rowadd:
        dr = colsum_raw(dy.view(Bn * Ho * Wo, Cout), segments=Bn)
        if need_bias:
            db = _param_grad(bias, lambda o: colsum_raw(dr, 1, out=o).view(Cout))
    elif need_bias:
        db = _param_grad(bias, lambda o: colsum_raw(dy.view(Bn * Ho * Wo, Cout), 1, out=o).view(Cout))
    return db, dr


class GnSiluConv3x3Fn(torch.autograd.Function):
    """Training form of a ResnetBlock2D half: (y [, alias of x]) = (conv3x3(SiLU(GroupNorm(x))) + bias + rowadd[b] + residual [, x])
    as ONE autograd node over the two ordinary launches, `gad_groupnorm_silu_fwd` then the convolution: the normalised
    activation h is saved only where the weight wants a gradient (a frozen weight: nothing reads it again), and an F(4x4)
    forward launch's transformed input is kept for that weight gradient as in Conv2dFn.  Results are bit-identical to the two
    separate nodes'.  Backward = Conv2dFn's then GroupNormSiluFn's kernels."""

    @staticmethod
    def forward(ctx, x, gamma, beta, w, bias, rowadd, residual, G, eps, bypass):
        _req(x, "groupnorm x")
        Bn = x.shape[0]
        mean = torch.empty((Bn, G), device=x.device, dtype=torch.float32)
        rstd = torch.empty_like(mean)
        keep = [] if ctx.needs_input_grad[3] else None
        h = torch.empty_like(x)
        check(_capi.load().gad_groupnorm_silu_fwd(C.byref(_gn_args(x, h, gamma, beta, mean, rstd, G, eps, True)), _stream()),
              "gad_groupnorm_silu_fwd")
        y = conv2d_fwd_raw(h, w, bias, 1, (1, 1, 1, 1), False, rowadd=rowadd, residual=residual, keep_v=keep)
        ctx.save_for_backward(x, gamma, beta, mean, rstd, w, h if keep is not None else None)     # (a frozen weight: nothing reads h again)
        ctx.wino_v = keep[0] if keep else None
        ctx.bias_ref = bias
        ctx.cfg = (G, eps, (bias is not None, rowadd is not None, residual is not None))
        return (y, x.view_as(x)) if bypass else y

    @staticmethod
    def backward(ctx, dy, dbypass=None):
        x, gamma, beta, mean, rstd, w, h = ctx.saved_tensors
        G, eps, has = ctx.cfg
        need = ctx.needs_input_grad
        if dy is None:                                   # only the alias of x was used downstream
            return (dbypass, *([None] * 9))
        dh, dw, db, dr, dres = _conv_backward(ctx, dy, h, x.shape, w, 1, (1, 1, 1, 1), False, has,
                                              (need[0] or need[1] or need[2], *need[3:7]))
        dx = dgamma = dbeta = None
        if dh is not None:
            dx, dgamma, dbeta = _gn_backward(x, gamma, beta, mean, rstd, G, eps, True, dh, dbypass, need[1] or need[2])
        elif dbypass is not None:
            dx = dbypass
        return dx, dgamma, dbeta, dw, db, dr, dres, None, None, None


def gn_silu_conv3x3(x, gamma, beta, G, eps, w, bias, rowadd=None, residual=None, bypass=False):
    """Differentiable conv3x3(SiLU(GroupNorm(x))) + bias + rowadd + residual (GnSiluConv3x3Fn); with `bypass` also an alias of
    x for the block's residual branch (as `group_norm_bypass`).  Bit-identical to `group_norm` then `conv2d`, which half-precision
    activations and odd shapes take."""
    if x.dtype == torch.bfloat16 or tuple(w.shape[2:]) != (3, 3) or w.shape[1] != x.shape[-1] or x.ndim != 4:
        if bypass:
            h, x = group_norm_bypass(x, gamma, beta, G, eps, True)
        else:
            h = group_norm(x, gamma, beta, G, eps, True)
        y = conv2d(h, w, bias, rowadd, residual)
        return (y, x) if bypass else y
    if bypass and not (torch.is_grad_enabled() and x.requires_grad):
        return GnSiluConv3x3Fn.apply(x, gamma, beta, w, bias, rowadd, residual, G, eps, False), x
    return GnSiluConv3x3Fn.apply(x, gamma, beta, w, bias, rowadd, residual, G, eps, bypass)


def _half():
    from . import half
    return half


def conv2d(x, w, bias=None, rowadd=None, residual=None, stride=1, pad=(1, 1, 1, 1), upsample=False):
    if x.dtype == torch.bfloat16:
        return _half().conv2d(x, w, bias, rowadd, residual, stride, pad, upsample)
    return Conv2dFn.apply(x, w, bias, rowadd, residual, stride, pad, upsample)


class LinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, bias, residual):
        shp = x.shape
        x2 = _req(x, "linear x").view(-1, shp[-1])
        ctx.save_for_backward(x2, w)
        ctx.shp = shp
        ctx.bias_ref = bias
        ctx.flags = (bias is not None, residual is not None)
        r2 = residual.view(-1, w.shape[0]) if residual is not None else None
        return linear_fwd_raw(x2, w, bias, r2).view(*shp[:-1], w.shape[0])

    @staticmethod
    def backward(ctx, dy):
        x2, w = ctx.saved_tensors
        dy2 = dy.contiguous().view(-1, w.shape[0])
        dx = linear_dgrad_raw(dy2, w).view(ctx.shp) if ctx.needs_input_grad[0] else None
        dw = _param_grad(w, lambda o: linear_wgrad_raw(dy2, x2, out=o)) if ctx.needs_input_grad[1] else None
        db = _param_grad(ctx.bias_ref, lambda o: colsum_raw(dy2, 1, out=o).view(-1)) \
            if (ctx.flags[0] and ctx.needs_input_grad[2]) else None
        dres = dy if (ctx.flags[1] and ctx.needs_input_grad[3]) else None
        return dx, dw, db, dres


def linear(x, w, bias=None, residual=None):
    if x.dtype == torch.bfloat16:
        return _half().linear(x, w, bias, residual)
    return LinearFn.apply(x, w, bias, residual)


def lora_fusable(in_features: int, out_features: int, rank: int) -> bool:
    """Can y = x W^T + b + s (x A^T) B^T run as down-GEMM + ONE K-concatenated GEMM (forward and data gradient)?
    The K split points (in_features forward, out_features backward) must be multiples of the 32-wide K step and the rank
    a multiple of 4 (float4 staging); pruned ragged ranks that are not take the two-launch route."""
    return in_features % 32 == 0 and out_features % 32 == 0 and rank % 4 == 0 and rank > 0


class LoraLinearFn(torch.autograd.Function):
    """diffusers LoRACompatibleLinear with a LoRALinearLayer set (text_to_image/train_text_to_image_lora.py:786-820,
    SURVEY A.11): y = x W^T + b + s (x A^T) B^T [+ residual].
    Forward:  mid = s x A^T (alpha epilogue), then ONE launch over the concatenated K axis [x | mid] . [W | B]^T.
    Backward: dmid = s dy B, then ONE launch dx = [dy | dmid] . [W ; A]; dB = dy^T mid, dA = dmid^T x (and dW, db when
    the base is trainable).  Against base GEMM + residual-accumulating side GEMM this drops one launch and one
    read + write pass over y (forward) / dx (backward) per projection - 128 projections in the SD U-Net."""

    @staticmethod
    def forward(ctx, x, w, bias, down, up, s, residual):
        shp = x.shape
        x2 = _req(x, "lora linear x").view(-1, shp[-1])
        M, K = x2.shape
        N, r = up.shape
        mid = torch.empty((M, r), device=x.device, dtype=torch.float32)
        gemm_raw(x2, down, mid, A_KC, B_KC, M, r, K, K, K, r, alpha=s)
        y = torch.empty((M, N), device=x.device, dtype=torch.float32)
        r2 = residual.view(-1, N) if residual is not None else None
        gemm_raw(x2, w, y, A_KC, B_KC, M, N, K + r, K, K, N, bias=bias, residual=r2, ldr=N, A_k2=mid, B_k2=up, k_split=K)
        ctx.save_for_backward(x2, w, down, up, mid)
        ctx.meta = (shp, s, bias, residual is not None)
        return y.view(*shp[:-1], N)

    @staticmethod
    def backward(ctx, dy):
        x2, w, down, up, mid = ctx.saved_tensors
        shp, s, bias, has_res = ctx.meta
        M, K = x2.shape
        N, r = up.shape
        dy2 = dy.contiguous().view(-1, N)
        need_x = ctx.needs_input_grad[0]
        need_lora = ctx.needs_input_grad[3] or ctx.needs_input_grad[4]
        dmid = None
        if need_x or ctx.needs_input_grad[3]:
            dmid = torch.empty((M, r), device=dy2.device, dtype=torch.float32)
            gemm_raw(dy2, up, dmid, A_KC, B_MC, M, r, N, N, r, r, alpha=s)                  # s dy B
        dx = None
        if need_x:
            dx = torch.empty((M, K), device=dy2.device, dtype=torch.float32)
            gemm_raw(dy2, w, dx, A_KC, B_MC, M, K, N + r, N, K, K, A_k2=dmid, B_k2=down, k_split=N)
            dx = dx.view(shp)
        dw = _param_grad(w, lambda o: linear_wgrad_raw(dy2, x2, out=o)) if ctx.needs_input_grad[1] else None
        db = _param_grad(bias, lambda o: colsum_raw(dy2, 1, out=o).view(-1)) if (bias is not None and ctx.needs_input_grad[2]) else None
        dd = _param_grad(down, lambda o: linear_wgrad_raw(dmid, x2, out=o)) if ctx.needs_input_grad[3] else None      # dmid^T x
        du = _param_grad(up, lambda o: linear_wgrad_raw(dy2, mid, out=o)) if ctx.needs_input_grad[4] else None        # dy^T mid
        dres = dy if (has_res and ctx.needs_input_grad[6]) else None
        return dx, dw, db, dd, du, None, dres


def lora_linear(x, w, bias, down, up, s=1.0, residual=None):
    if x.dtype == torch.bfloat16:
        return _half().lora_linear(x, w, bias, down, up, s, residual)
    return LoraLinearFn.apply(x, w, bias, down, up, float(s), residual)


def _gn_args(x, y, gamma, beta, mean, rstd, G, eps, silu):
    a = GroupNormArgs()
    Bn, C_ = x.shape[0], x.shape[-1]
    HW = x.numel() // (Bn * C_)
    ws = workspace(x.device)
    a.x, a.y, a.gamma, a.beta = x.data_ptr(), y.data_ptr(), gamma.data_ptr(), beta.data_ptr()
    a.mean, a.rstd = mean.data_ptr(), rstd.data_ptr()
    a.B, a.HW, a.C, a.G = Bn, HW, C_, G
    a.eps, a.silu = eps, int(silu)
    a.ws, a.ws_bytes = ws.data_ptr(), ws.numel()
    a.flags = KERNEL_FLAGS["gn"]
    return a


def _gn_backward(x, gamma, beta, mean, rstd, G, eps, silu, dy, dbypass, affine_grads):
    """-> (dx, dgamma, dbeta) of y = [SiLU](GroupNorm(x)); `dbypass` (the gradient of an alias of x) is summed in the kernel's
    store; parameter gradients go to their flat-buffer slots where they have one (then returned as None)."""
    dy = dy.contiguous()
    dx = torch.empty_like(x)
    a = _gn_args(x, dx, gamma, beta, mean, rstd, G, eps, silu)
    a.dy = dy.data_ptr()
    if dbypass is not None:
        a.dx_add = _req(dbypass.contiguous(), "groupnorm bypass gradient").data_ptr()
    if not affine_grads:                                 # frozen norm (LoRA training): dx only
        check(_capi.load().gad_groupnorm_silu_bwd(C.byref(a), _stream()), "gad_groupnorm_silu_bwd")
        return dx, None, None
    (sg, fg), (sb, fb) = _sink(gamma), _sink(beta)
    direct_g, direct_b = sg is not None and fg, sb is not None and fb
    dgamma = sg if direct_g else torch.empty_like(gamma)
    dbeta = sb if direct_b else torch.empty_like(beta)
    a.dgamma, a.dbeta = dgamma.data_ptr(), dbeta.data_ptr()
    check(_capi.load().gad_groupnorm_silu_bwd(C.byref(a), _stream()), "gad_groupnorm_silu_bwd")
    if sg is not None:
        if not fg:
            sg.add_(dgamma)
        dgamma = None
    if sb is not None:
        if not fb:
            sb.add_(dbeta)
        dbeta = None
    return dx, dgamma, dbeta


class GroupNormSiluFn(torch.autograd.Function):
    """y = [SiLU](GroupNorm(x)) on NHWC; x is [B, ..., C]."""

    @staticmethod
    def forward(ctx, x, gamma, beta, G, eps, silu):
        _req(x, "groupnorm x")
        y = torch.empty_like(x)
        mean = torch.empty((x.shape[0], G), device=x.device, dtype=torch.float32)
        rstd = torch.empty_like(mean)
        a = _gn_args(x, y, gamma, beta, mean, rstd, G, eps, silu)
        check(_capi.load().gad_groupnorm_silu_fwd(C.byref(a), _stream()), "gad_groupnorm_silu_fwd")
        ctx.save_for_backward(x, gamma, beta, mean, rstd)
        ctx.cfg = (G, eps, silu)
        return y

    @staticmethod
    def backward(ctx, dy, dbypass=None):
        x, gamma, beta, mean, rstd = ctx.saved_tensors
        G, eps, silu = ctx.cfg
        return (*_gn_backward(x, gamma, beta, mean, rstd, G, eps, silu, dy, dbypass,
                              ctx.needs_input_grad[1] or ctx.needs_input_grad[2]), None, None, None)


class GroupNormBypassFn(GroupNormSiluFn):
    """(y, x_bypass) = (GroupNorm(+SiLU)(x), x): the input of ResnetBlock2D / the attention block feeds the norm AND the
    residual branch.  Handing the second consumer this node's own alias of x makes x single-consumer for autograd, and the
    backward receives both gradients at once: dx = gn_bwd(dy) + d(bypass) is one kernel (`gad_groupnorm_args.dx_add`)
    instead of the norm's backward plus an elementwise add launch."""

    @staticmethod
    def forward(ctx, x, gamma, beta, G, eps, silu):
        y = GroupNormSiluFn.forward(ctx, x, gamma, beta, G, eps, silu)
        return y, x.view_as(x)

    @staticmethod
    def backward(ctx, dy, dbypass):
        if dy is None:                                   # only the bypass was used downstream
            return dbypass, None, None, None, None, None
        return GroupNormSiluFn.backward(ctx, dy, dbypass)


def group_norm_bypass(x, gamma, beta, G, eps, silu):
    """-> (GroupNorm(+SiLU)(x), alias of x for the residual branch); see GroupNormBypassFn."""
    if x.dtype == torch.bfloat16:
        return _half().group_norm_bypass(x, gamma, beta, G, eps, silu)
    if not (torch.is_grad_enabled() and x.requires_grad):
        return group_norm(x, gamma, beta, G, eps, silu), x
    return GroupNormBypassFn.apply(x, gamma, beta, G, eps, silu)


def group_norm(x, gamma, beta, G, eps, silu):
    if x.dtype == torch.bfloat16:
        return _half().group_norm(x, gamma, beta, G, eps, silu)
    return GroupNormSiluFn.apply(x, gamma, beta, G, eps, silu)


def _gn2_args(x, x2, y, gamma, beta, mean, rstd, G, eps, silu):
    a = _gn_args(y, y, gamma, beta, mean, rstd, G, eps, silu)      # shapes of the concatenated tensor = y's
    a.x, a.x2, a.C1 = x.data_ptr(), x2.data_ptr(), x.shape[-1]
    return a


def group_norm_two_source_ok(x, x2, G) -> bool:
    """Can the forward of GroupNorm(cat([x, x2], channels)) read both sources in place?  (Both plans can - the one-pass
    slab plan and, since round 3, the two-pass plan the pruned widths' 288 = 192 + 96 channels at 32x32 take -, as long as
    a channel quad never straddles the two sources.)"""
    C_ = x.shape[-1] + x2.shape[-1]
    return C_ % G == 0 and x.shape[-1] % 4 == 0 and x2.shape[-1] % 4 == 0


def group_norm_cat_raw(x, x2, gamma, beta, G, eps, silu):
    """[SiLU](GroupNorm(cat([x, x2], -1))) without the concatenated tensor (forward only, no autograd)."""
    _req(x, "groupnorm x")
    _req(x2, "groupnorm x2")
    y = torch.empty((*x.shape[:-1], x.shape[-1] + x2.shape[-1]), device=x.device, dtype=torch.float32)
    mean = torch.empty((x.shape[0], G), device=x.device, dtype=torch.float32)
    rstd = torch.empty_like(mean)
    a = _gn2_args(x, x2, y, gamma, beta, mean, rstd, G, eps, silu)
    check(_capi.load().gad_groupnorm_silu_fwd(C.byref(a), _stream()), "gad_groupnorm_silu_fwd")
    return y


class SiluFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        _req(x, "silu x")
        y = torch.empty_like(x)
        check(_capi.load().gad_silu_fwd(x.data_ptr(), y.data_ptr(), x.numel(), _stream()), "gad_silu_fwd")
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        dy = dy.contiguous()
        dx = torch.empty_like(x)
        check(_capi.load().gad_silu_bwd(x.data_ptr(), dy.data_ptr(), dx.data_ptr(), x.numel(), _stream()), "gad_silu_bwd")
        return dx


def silu(x):
    return SiluFn.apply(x)


class ConcatFn(torch.autograd.Function):
    """torch.cat([h, skip], dim=channel) for NHWC tensors (UpBlock2D skip connections)."""

    @staticmethod
    def forward(ctx, a, b):
        _req(a, "concat a")
        _req(b, "concat b")
        C1, C2 = a.shape[-1], b.shape[-1]
        out = torch.empty((*a.shape[:-1], C1 + C2), device=a.device, dtype=torch.float32)
        check(_capi.load().gad_concat_channels(a.data_ptr(), b.data_ptr(), out.data_ptr(), a.numel() // C1, C1, C2,
                                               _stream()), "gad_concat_channels")
        ctx.cs = (C1, C2)
        return out

    @staticmethod
    def backward(ctx, d):
        C1, C2 = ctx.cs
        d = d.contiguous()
        da = torch.empty((*d.shape[:-1], C1), device=d.device, dtype=torch.float32)
        db = torch.empty((*d.shape[:-1], C2), device=d.device, dtype=torch.float32)
        check(_capi.load().gad_split_channels(d.data_ptr(), da.data_ptr(), db.data_ptr(), d.numel() // (C1 + C2), C1, C2,
                                              _stream()), "gad_split_channels")
        return da, db


def concat(a, b):
    if a.dtype == torch.bfloat16:
        return _half().concat(a, b)
    return ConcatFn.apply(a, b)


def nchw_to_nhwc_raw(x):
    Bn, C_, H, W = x.shape
    y = torch.empty((Bn, H, W, C_), device=x.device, dtype=torch.float32)
    check(_capi.load().gad_nchw_to_nhwc(x.data_ptr(), y.data_ptr(), Bn, C_, H * W, _stream()), "gad_nchw_to_nhwc")
    return y


def nhwc_to_nchw_raw(x):
    Bn, H, W, C_ = x.shape
    y = torch.empty((Bn, C_, H, W), device=x.device, dtype=torch.float32)
    check(_capi.load().gad_nhwc_to_nchw(x.data_ptr(), y.data_ptr(), Bn, C_, H * W, _stream()), "gad_nhwc_to_nchw")
    return y


class ToNCHWFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return nhwc_to_nchw_raw(_req(x, "to_nchw x"))

    @staticmethod
    def backward(ctx, dy):
        return nchw_to_nhwc_raw(dy.contiguous())


def to_nchw(x):
    return ToNCHWFn.apply(x)


def timestep_embedding(t: torch.Tensor, dim, flip_sin_to_cos, freq_shift, max_period=10000.0):
    t = t.to(torch.int64).contiguous()
    out = torch.empty((t.shape[0], dim), device=t.device, dtype=torch.float32)
    check(_capi.load().gad_timestep_embedding(t.data_ptr(), out.data_ptr(), t.shape[0], dim, int(flip_sin_to_cos),
                                              float(freq_shift), float(max_period), _stream()), "gad_timestep_embedding")
    return out


# ---- attention core: softmax(q k^T / sqrt(d)) v with q,k,v given as [B, T, heads*d] ----
def _attn_gemm(A, B, Cm, a_mode, b_mode, M, N, K, lda, ldb, ldc, Bn, heads, sA, sB, sC, alpha=1.0):
    gemm_raw(A, B, Cm, a_mode, b_mode, M, N, K, lda, ldb, ldc, alpha=alpha, batch=Bn * heads, batch_inner=heads,
             sA=sA, sB=sB, sC=sC)


def fused_attention_ok(d: int, *lds) -> bool:
    """Does the fused (flash-style) attention take this head dim?  Any d <= 256 does; row strides need no alignment
    (an exact instance - 16, 24, 32, 40, 48, 64, 80, 96, 128, 160, 192, 224, 256 - with float4-aligned rows streams by
    LDS-DMA, anything else - the head-grouped-pruned CelebA model's d = 23 - runs the dword-staged RG instance)."""
    return bool(_capi.load().gad_attention_supported(int(d)))


def _attention_args(q, k, v, o, lse, Bn, heads, Tq, Tk, d, ldq, ldk, ldv, sq, sk, sv, scale=None):
    a = _capi.AttentionArgs()
    a.q, a.k, a.v, a.o, a.lse = q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), _ptr(lse)
    a.B, a.heads, a.Tq, a.Tk, a.d = Bn, heads, Tq, Tk, d
    a.ldq, a.ldk, a.ldv, a.ldo = ldq, ldk, ldv, heads * d
    a.stride_q, a.stride_k, a.stride_v, a.stride_o = sq, sk, sv, Tq * heads * d
    a.scale = 1.0 / math.sqrt(d) if scale is None else scale       # (zero-padded heads keep the true head dim's scale)
    if scale is not None:
        a.alg_d = int(round(1.0 / (scale * scale)))
    a.operand_precision = 0
    return a


def _attention_grad_args(a, do, delta, dq, dk, dv, ld, sq, sk):
    """The backward's fields of `a`: gradient pointers, their row stride, batch strides of the query / key side."""
    a.d_o, a.delta, a.dq, a.dk, a.dv = do.data_ptr(), delta.data_ptr(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr()
    a.ld_do = a.ld_dq = a.ld_dk = a.ld_dv = ld
    a.stride_do = a.stride_dq = sq
    a.stride_dk = a.stride_dv = sk
    return a


def attention_fwd_raw(q, k, v, Bn, heads, Tq, Tk, d, ldq, ldk, ldv, need_lse=True, scale=None):
    """Fused attention forward on [Bn, T, *] views (q, k, v may be column blocks of one projection output: their
    data_ptr is the column offset, ld* the row stride).  -> (o [Bn, Tq, heads*d], lse [Bn, heads, Tq] or None)"""
    o = _out((Bn, Tq, heads * d), q.device)
    lse = _out((Bn, heads, Tq), q.device) if need_lse else None
    a = _attention_args(q, k, v, o, lse, Bn, heads, Tq, Tk, d, ldq, ldk, ldv, Tq * ldq, Tk * ldk, Tk * ldv, scale)
    a.operand_precision = 1 if OPERAND_PRECISION[0] else 0         # bf16 modes: bf16-operand instance of the fused kernel
    a.flags = _capi.ATTN_NARROW_FWD if KERNEL_FLAGS["narrow_attn_fwd"] else 0
    if PROFILER is not None:
        PROFILER.attention(_capi.load().gad_attention_fwd, a, "fwd")
    else:
        check(_capi.load().gad_attention_fwd(C.byref(a), _stream()), "gad_attention_fwd")
    return o, lse


class AttentionCoreFn(torch.autograd.Function):
    """F.scaled_dot_product_attention(q, k, v) of AttnProcessor2_0
    (reference src/diffusers/models/attention_processor.py:1314-1325) on [B, T, heads*d] operands: ONE fused kernel
    forward (online softmax, the scores never leave the CU; only the per-row log-sum-exp is kept) and a
    recomputing dQ + dK/dV kernel pair backward (csrc/attention.hip)."""

    @staticmethod
    def forward(ctx, q, k, v, heads, scale=None):
        for t_, n_ in ((q, "q"), (k, "k"), (v, "v")):
            _req(t_, n_)
        Bn, Tq, Cq = q.shape
        Tk = k.shape[1]
        d = Cq // heads
        o, lse = attention_fwd_raw(q, k, v, Bn, heads, Tq, Tk, d, Cq, Cq, Cq, need_lse=True, scale=scale)
        ctx.save_for_backward(q, k, v, o, lse)
        ctx.heads, ctx.prec, ctx.scale = heads, (1 if OPERAND_PRECISION[0] else 0), scale
        return o

    @staticmethod
    def backward(ctx, do):
        q, k, v, o, lse = ctx.saved_tensors
        heads = ctx.heads
        do = do.contiguous()
        Bn, Tq, Cq = q.shape
        Tk = k.shape[1]
        d = Cq // heads
        dq, dk, dv = _out(q.shape, q.device), _out(k.shape, k.device), _out(v.shape, v.device)
        delta = _out(lse.shape, lse.device)
        a = _attention_args(q, k, v, o, lse, Bn, heads, Tq, Tk, d, Cq, Cq, Cq, Tq * Cq, Tk * Cq, Tk * Cq, ctx.scale)
        _attention_grad_args(a, do, delta, dq, dk, dv, Cq, Tq * Cq, Tk * Cq)
        a.operand_precision = ctx.prec                  # the precision the forward's LSE was computed in
        a.flags = _capi.ATTN_TWO_KERNEL_BWD if KERNEL_FLAGS["two_kernel_attn_bwd"] else 0
        need = _capi.load().gad_attention_bwd_workspace_bytes(C.byref(a))
        if need:                                         # dQ partial slabs of the single-pass kernel (one per key block)
            slabs = _scratch("attn_ws", need, q.device)
            a.ws, a.ws_bytes = slabs.data_ptr(), need
        if PROFILER is not None:
            PROFILER.attention(_capi.load().gad_attention_bwd, a, "bwd")
        else:
            check(_capi.load().gad_attention_bwd(C.byref(a), _stream()), "gad_attention_bwd")
        return dq, dk, dv, None, None


class UnfusedAttentionCoreFn(torch.autograd.Function):
    """The same function as three launches (batched Q K^T, row softmax, batched P V; P kept for backward): the route
    for head dims without a fused instance, and the independent implementation the fused kernels are tested against."""

    @staticmethod
    def forward(ctx, q, k, v, heads, scale=None):
        for t_, n_ in ((q, "q"), (k, "k"), (v, "v")):
            _req(t_, n_)
        Bn, Tq, Cq = q.shape
        Tk = k.shape[1]
        d = Cq // heads
        scale = 1.0 / math.sqrt(d) if scale is None else scale
        ctx.scale = scale
        S = torch.empty((Bn, heads, Tq, Tk), device=q.device, dtype=torch.float32)
        _attn_gemm(q, k, S, A_KC, B_KC, Tq, Tk, d, Cq, Cq, Tk, Bn, heads,
                   (Tq * Cq, d), (Tk * Cq, d), (heads * Tq * Tk, Tq * Tk))
        check(_capi.load().gad_softmax_fwd(S.data_ptr(), S.data_ptr(), Bn * heads * Tq, Tk, scale, _stream()),
              "gad_softmax_fwd")
        o = torch.empty((Bn, Tq, Cq), device=q.device, dtype=torch.float32)
        _attn_gemm(S, v, o, A_KC, B_MC, Tq, d, Tk, Tk, Cq, Cq, Bn, heads,
                   (heads * Tq * Tk, Tq * Tk), (Tk * Cq, d), (Tq * Cq, d))
        ctx.save_for_backward(q, k, v, S)
        ctx.heads = heads
        return o

    @staticmethod
    def backward(ctx, do):
        q, k, v, P = ctx.saved_tensors
        heads = ctx.heads
        do = do.contiguous()
        Bn, Tq, Cq = q.shape
        Tk = k.shape[1]
        d = Cq // heads
        scale = ctx.scale
        sP = (heads * Tq * Tk, Tq * Tk)
        sQ, sK = (Tq * Cq, d), (Tk * Cq, d)
        # dV[b,h] = P^T dO   (A = P as [k=Tq][m=Tk], B = dO as [k=Tq][n=d])
        dv = torch.empty_like(v)
        _attn_gemm(P, do, dv, A_MC, B_MC, Tk, d, Tq, Tk, Cq, Cq, Bn, heads, sP, sQ, sK)
        # dP = dO V^T
        dP = torch.empty_like(P)
        _attn_gemm(do, v, dP, A_KC, B_KC, Tq, Tk, d, Cq, Cq, Tk, Bn, heads, sQ, sK, sP)
        # dS = scale * P * (dP - rowsum(dP*P))   (in place into dP)
        check(_capi.load().gad_softmax_bwd(P.data_ptr(), dP.data_ptr(), dP.data_ptr(), Bn * heads * Tq, Tk, scale,
                                           _stream()), "gad_softmax_bwd")
        # dQ = dS K ; dK = dS^T Q
        dq = torch.empty_like(q)
        _attn_gemm(dP, k, dq, A_KC, B_MC, Tq, d, Tk, Tk, Cq, Cq, Bn, heads, sP, sK, sQ)
        dk = torch.empty_like(k)
        _attn_gemm(dP, q, dk, A_MC, B_MC, Tk, d, Tq, Tk, Cq, Cq, Bn, heads, sP, sQ, sK)
        return dq, dk, dv, None, None


class PadHeadsFn(torch.autograd.Function):
    """Zero-pad the per-head blocks of an attention projection parameter from head dim d to dpad (a multiple of 8):
    axis 0 - the rows of to_q / to_k / to_v weights [heads*d, C] and biases [heads*d]; axis 1 - the columns of the to_out
    weight [C, heads*d].  The head-grouped-pruned CelebA model has d = 23 (reference unconditional_generation/prune.py:
    337-342): 322-float rows are not float4-aligned, which puts the four projections on the scalar-gather GEMM path and
    the attention on its dword-staged instances.  With zero-padded heads (d = 24) every launch is back on LDS-DMA and the
    result is the same function: the extra q / k channels are 0 * 0, the extra v / output channels meet zero columns of
    to_out.  The gradient of the padded tensor is sliced back into the parameter (its flat-buffer sink when a
    FusedTrainer step is running)."""

    @staticmethod
    def forward(ctx, w, heads, d, dpad, axis):
        ctx.param, ctx.cfg = w, (heads, d, dpad, axis)
        src = w.detach()
        if axis == 0:
            rest = src.shape[1:]
            out = src.new_zeros((heads, dpad) + tuple(rest))
            out[:, :d] = src.reshape((heads, d) + tuple(rest))
            return out.view((heads * dpad,) + tuple(rest))
        out = src.new_zeros((src.shape[0], heads, dpad))
        out[:, :, :d] = src.reshape(src.shape[0], heads, d)
        return out.view(src.shape[0], heads * dpad)

    @staticmethod
    def backward(ctx, g):
        heads, d, dpad, axis = ctx.cfg
        w = ctx.param
        if axis == 0:
            gs = g.view((heads, dpad) + tuple(w.shape[1:]))[:, :d].reshape(w.shape)
        else:
            gs = g.view(w.shape[0], heads, dpad)[:, :, :d].reshape(w.shape)
        return _deliver(w, gs), None, None, None, None


def pad_heads(w, heads, d, dpad, axis):
    return PadHeadsFn.apply(w, heads, d, dpad, axis)


def attention_core(q, k, v, heads, scale=None):
    if q.dtype == torch.bfloat16:
        return _half().attention_core(q, k, v, heads, scale)
    d = q.shape[-1] // heads
    # Training at one wide head over a short sequence (CIFAR: d = 256 / 192, T <= 256) keeps the three-launch route: S is a
    # few MB there, and the recomputing backward (7 products, 1 wave per SIMD at d >= 192) measured 0.48 ms against
    # 0.32 ms (tools/bench_attention.py).  Everything else - every sampling forward, CelebA's and SD's heads - is fused.
    wide_short = torch.is_grad_enabled() and d > 160 and q.shape[1] * k.shape[1] <= 256 * 256
    if fused_attention_ok(d, q.shape[-1]) and not wide_short:
        return AttentionCoreFn.apply(q, k, v, heads, scale)
    return UnfusedAttentionCoreFn.apply(q, k, v, heads, scale)


def attention_core_fused(q, k, v, heads):
    return AttentionCoreFn.apply(q, k, v, heads)


def attention_core_unfused(q, k, v, heads):
    return UnfusedAttentionCoreFn.apply(q, k, v, heads)


def attention_core_qkv_raw(qkv, Bn, T, Cq, heads, scale=None):
    """Inference form on the output of ONE fused projection: qkv is [Bn*T, 3*Cq] (q | k | v along the columns); the
    fused attention kernel reads q, k, v in place through their row stride 3*Cq.  No autograd."""
    d = Cq // heads
    ld = 3 * Cq
    q, k, v = qkv[:, 0:Cq], qkv[:, Cq:2 * Cq], qkv[:, 2 * Cq:3 * Cq]        # views: data_ptr = column offset
    if fused_attention_ok(d, ld):
        return attention_fwd_raw(q, k, v, Bn, heads, T, T, d, ld, ld, ld, need_lse=False, scale=scale)[0]
    scale = 1.0 / math.sqrt(d) if scale is None else scale
    S = torch.empty((Bn, heads, T, T), device=qkv.device, dtype=torch.float32)
    _attn_gemm(q, k, S, A_KC, B_KC, T, T, d, ld, ld, T, Bn, heads, (T * ld, d), (T * ld, d), (heads * T * T, T * T))
    check(_capi.load().gad_softmax_fwd(S.data_ptr(), S.data_ptr(), Bn * heads * T, T, scale, _stream()), "gad_softmax_fwd")
    o = torch.empty((Bn, T, Cq), device=qkv.device, dtype=torch.float32)
    _attn_gemm(S, v, o, A_KC, B_MC, T, d, T, T, ld, Cq, Bn, heads, (heads * T * T, T * T), (T * ld, d), (T * Cq, d))
    return o


# ----------------------------------------------------------------------------------
# scheduler / loss / optimizer kernels (no autograd)
# ----------------------------------------------------------------------------------
def add_noise_raw(x0, eps, t, alphas_cumprod):
    _req(x0, "add_noise x0")
    _req(eps, "add_noise eps")
    t = t.to(torch.int64).contiguous()
    out = torch.empty_like(x0)
    check(_capi.load().gad_add_noise(x0.data_ptr(), eps.data_ptr(), t.data_ptr(), alphas_cumprod.data_ptr(),
                                     out.data_ptr(), x0.shape[0], x0.numel() // x0.shape[0], _stream()), "gad_add_noise")
    return out


def ddim_step_raw(x, eps, alpha_t: float, alpha_prev: float, clip: float, out=None):
    _req(x, "ddim x")
    _req(eps, "ddim eps")
    out = torch.empty_like(x) if out is None else out
    check(_capi.load().gad_ddim_step(x.data_ptr(), eps.data_ptr(), out.data_ptr(), x.numel(), alpha_t, alpha_prev, clip,
                                     _stream()), "gad_ddim_step")
    return out


_DDPM_VARIANCE = {"fixed_small": _capi.DDPM_FIXED_SMALL, "fixed_large": _capi.DDPM_FIXED_LARGE}


def ddpm_step_raw(x, eps, seeds, t: int, alpha_t: float, alpha_prev: float, clip: float, variance_type="fixed_small", out=None):
    """Ancestral DDPM update of a batch in one launch (gad_ddpm_step): x, eps [B][...] fp32, seeds [B] int64 device (row b's
    64-bit noise key).  Row b's variance noise is a function of (seeds[b], t, element) alone.  `out` may be x (in place)."""
    _req(x, "ddpm x")
    _req(eps, "ddpm eps")
    if variance_type not in _DDPM_VARIANCE:
        raise _capi.GadError(f"ddpm_step: variance_type={variance_type!r}, expected fixed_small or fixed_large")
    B = x.shape[0]
    if eps.shape != x.shape or not (seeds.is_cuda and seeds.dtype == torch.int64 and seeds.is_contiguous() and seeds.numel() == B):
        raise _capi.GadError(f"ddpm_step: eps {tuple(eps.shape)} must match x {tuple(x.shape)} and seeds must be a contiguous "
                             f"int64 device tensor of {B} entries, got {seeds.dtype} {seeds.device} {tuple(seeds.shape)}")
    out = torch.empty_like(x) if out is None else _req(out, "ddpm out")
    if out.shape != x.shape:
        raise _capi.GadError(f"ddpm_step: out {tuple(out.shape)} must match x {tuple(x.shape)}")
    check(_capi.load().gad_ddpm_step(x.data_ptr(), eps.data_ptr(), out.data_ptr(), B, x.numel() // max(B, 1), seeds.data_ptr(),
                                     int(t), alpha_t, alpha_prev, clip, _DDPM_VARIANCE[variance_type], _stream()),
          "gad_ddpm_step")
    return out


def latent_draw_raw(moments, rows, seed: int, step: int, scale: float, sample=True, random_flip=False, out=None, flipped=None):
    """The x0 rows of one SD training step in one launch (gad_latent_draw): moments [N, F, 2L, h, w] fp32 (F = 1 plain, 2 plain |
    flipped; mean | logvar along the channels), rows [B] int64 device -> x0 [B, L, h, w] = scale * (mean + std z) of the slab
    the row's coin picks (`random_flip`), or scale * mean (`sample=False`).  `flipped` (uint8 [B]) receives the slab index.
    A row is a function of (seed, rows[b], step) alone."""
    _req(moments, "latent_draw moments")
    if moments.dim() != 5 or moments.shape[2] % 2:
        raise _capi.GadError(f"latent_draw: moments must be [N, F, 2L, h, w], got {tuple(moments.shape)}")
    N, F, L2, h, w = moments.shape
    if not (rows.is_cuda and rows.dtype == torch.int64 and rows.is_contiguous() and rows.dim() == 1):
        raise _capi.GadError(f"latent_draw: rows must be a contiguous 1-D int64 device tensor, got {rows.dtype} {rows.device} "
                             f"{tuple(rows.shape)}")
    B, shape = rows.numel(), (rows.numel(), L2 // 2, h, w)
    out = torch.empty(shape, dtype=torch.float32, device=moments.device) if out is None else _req(out, "latent_draw out")
    if tuple(out.shape) != shape:
        raise _capi.GadError(f"latent_draw: out {tuple(out.shape)} must be {shape}")
    if flipped is not None and not (flipped.is_cuda and flipped.dtype == torch.uint8 and flipped.is_contiguous()
                                    and flipped.numel() == B):
        raise _capi.GadError(f"latent_draw: flipped must be a contiguous uint8 device tensor of {B} entries, got {flipped.dtype} "
                             f"{flipped.device} {tuple(flipped.shape)}")
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    flags = (_capi.LATENT_SAMPLE if sample else 0) | (_capi.LATENT_RANDOM_FLIP if random_flip else 0)
    check(_capi.load().gad_latent_draw(moments.data_ptr(), N, F, (L2 // 2) * h * w, rows.data_ptr(), B, out.data_ptr(),
                                       _ptr(flipped), seed - (1 << 64) if seed >> 63 else seed, int(step) & 0xFFFFFFFF,
                                       float(scale), flags, _stream()), "gad_latent_draw")
    return out


def pixels_to_nchw_raw(pixels, lut, flip=False, out=None):
    """uint8 [B, H, W, C] device pixels -> fp32 [B, C, H, W] = lut[pixel] (gad_pixels_to_nchw), mirrored along W when `flip`.
    `lut`: 256 fp32 values on the device (gad.similarity.pixel_lut: ToTensor + Normalize([0.5], [0.5]))."""
    if not (pixels.is_cuda and pixels.dtype == torch.uint8 and pixels.is_contiguous() and pixels.dim() == 4):
        raise _capi.GadError(f"pixels_to_nchw: expected a contiguous uint8 [B, H, W, C] device tensor, got {pixels.dtype} "
                             f"{pixels.device} {tuple(pixels.shape)}")
    _req(lut, "pixels_to_nchw lut")
    if lut.numel() != 256:
        raise _capi.GadError(f"pixels_to_nchw: lut must hold 256 values, got {lut.numel()}")
    B, H, W, Cn = pixels.shape
    out = torch.empty((B, Cn, H, W), dtype=torch.float32, device=pixels.device) if out is None else _req(out, "pixels_to_nchw out")
    if tuple(out.shape) != (B, Cn, H, W):
        raise _capi.GadError(f"pixels_to_nchw: out {tuple(out.shape)} must be {(B, Cn, H, W)}")
    check(_capi.load().gad_pixels_to_nchw(pixels.data_ptr(), out.data_ptr(), B, H, W, Cn, lut.data_ptr(), int(bool(flip)),
                                          _stream()), "gad_pixels_to_nchw")
    return out


def plms_step_raw(x, eps, cs: float, cm: float, weights, history=(), push=None, x_saved=None, saved_mode=_capi.PLMS_SAVED_NONE,
                  guidance=None, out=None):
    """One PLMS step in one launch (gad_plms_step): x fp32, eps the U-Net output - of the doubled batch [uncond ; cond] when
    `guidance` is a number, of x's own shape when it is None.  `weights` = (w0, w1, w2, w3) for (e, *history), `history` the stored
    predictions newest first (at most three); `push` receives e; `x_saved` is written (PLMS_SAVE) or takes x's place
    (PLMS_USE_SAVED).  cs, cm and the weights are python floats (fp64), rounded once in the entry point.  `out` may be x."""
    _req(x, "plms x")
    _req(eps, "plms eps")
    n = x.numel()
    if eps.numel() != (n if guidance is None else 2 * n):
        raise _capi.GadError(f"plms_step: eps has {eps.numel()} elements, expected "
                             + (f"{n} (x's own)" if guidance is None else f"{2 * n} (the doubled batch [uncond ; cond])"))
    history = tuple(history)
    w = tuple(float(v) for v in weights)
    if len(w) != 4 or len(history) > 3:
        raise _capi.GadError(f"plms_step: {len(w)} weights and {len(history)} history terms, expected 4 and at most 3")
    for name, t in [(f"plms h{i + 1}", h) for i, h in enumerate(history)] + [("plms push", push), ("plms x_saved", x_saved)]:
        if t is not None and _req(t, name).numel() != n:
            raise _capi.GadError(f"plms_step: {name[5:]} has {t.numel()} elements, x has {n}")
    out = torch.empty_like(x) if out is None else _req(out, "plms out")
    if out.numel() != n:
        raise _capi.GadError(f"plms_step: out {tuple(out.shape)} must match x {tuple(x.shape)}")
    h = [t.data_ptr() for t in history] + [None] * (3 - len(history))
    eps_c = None if guidance is None else eps.data_ptr() + 4 * n
    check(_capi.load().gad_plms_step(x.data_ptr(), eps.data_ptr(), eps_c, 0.0 if guidance is None else float(guidance), h[0], h[1],
                                     h[2], None if push is None else push.data_ptr(),
                                     None if x_saved is None else x_saved.data_ptr(), int(saved_mode), out.data_ptr(), n,
                                     float(cs), float(cm), w[0], w[1], w[2], w[3], _stream()), "gad_plms_step")
    return out


def to_image01_raw(x):
    _req(x, "to_image01 x")
    y = torch.empty_like(x)
    check(_capi.load().gad_to_image01(x.data_ptr(), y.data_ptr(), x.numel(), _stream()), "gad_to_image01")
    return y


def mse_fwd_bwd_raw(pred, target, grad_scale=1.0):
    """(loss [1], dloss/dpred) for nn.MSELoss(reduction='mean') (reference main.py:602,708)."""
    _req(pred, "mse pred")
    _req(target, "mse target")
    ws = workspace(pred.device)
    loss = torch.empty(1, device=pred.device, dtype=torch.float32)
    d = torch.empty_like(pred)
    check(_capi.load().gad_mse_fwd_bwd(pred.data_ptr(), target.data_ptr(), loss.data_ptr(), d.data_ptr(), pred.numel(),
                                       grad_scale, ws.data_ptr(), ws.numel(), _stream()), "gad_mse_fwd_bwd")
    return loss, d


# ---- local model behaviours (csrc/local.hip) ----
def image_metrics_raw(a, b, win=7, data_range=1.0, K1=0.01, K2=0.03):
    """a, b: [N][H][W][C] fp32 images -> [N][3] fp64 (mse, nrmse with `a` as image_true, ssim), scikit-image's definitions."""
    _req(a, "image_metrics a")
    _req(b, "image_metrics b")
    if a.ndim != 4 or a.shape != b.shape:
        raise _capi.GadError(f"image_metrics: expected two [N][H][W][C] tensors of one shape, got {tuple(a.shape)} and {tuple(b.shape)}")
    N, H, W, Cc = a.shape
    lib = _capi.load()
    need = lib.gad_image_metrics_workspace_bytes(N, H, W, Cc, win)
    if need < 0:
        raise _capi.GadError(f"gad_image_metrics: {lib.gad_last_error().decode()}")
    ws = _scratch("metrics_ws", need, a.device)
    out = torch.empty((N, 3), device=a.device, dtype=torch.float64) if OUT_ALLOC_DT is None \
        else OUT_ALLOC_DT((N, 3), a.device, torch.float64)
    check(lib.gad_image_metrics(a.data_ptr(), b.data_ptr(), out.data_ptr(), N, H, W, Cc, win, data_range, K1, K2,
                                ws.data_ptr(), need, _stream()), "gad_image_metrics")
    return out


def add_noise_bcast_raw(x0, eps, t, alphas_cumprod, rows_per_image, out=None):
    """x0 [I][C][H][W], eps [R][C][H][W] (NCHW), t [T] int64 -> xt [R][H][W][C] (NHWC); row r: image r // rows_per_image,
    timestep t[r % T]."""
    _req(x0, "add_noise_bcast x0")
    _req(eps, "add_noise_bcast eps")
    _req(alphas_cumprod, "add_noise_bcast alphas_cumprod")
    if not (t.is_cuda and t.dtype == torch.int64 and t.is_contiguous() and t.ndim == 1):
        raise _capi.GadError("add_noise_bcast t: expected a contiguous 1-D int64 device tensor")
    R, Cc, H, W = eps.shape
    if x0.ndim != 4 or tuple(x0.shape[1:]) != (Cc, H, W) or x0.shape[0] * rows_per_image != R:
        raise _capi.GadError(f"add_noise_bcast: x0 {tuple(x0.shape)} does not hold one image per {rows_per_image} rows of eps {tuple(eps.shape)}")
    out = _out((R, H, W, Cc), eps.device) if out is None else _req(out, "add_noise_bcast out")
    if out.numel() != eps.numel():
        raise _capi.GadError("add_noise_bcast: out does not have the size of eps")
    check(_capi.load().gad_add_noise_bcast(x0.data_ptr(), eps.data_ptr(), t.data_ptr(), alphas_cumprod.data_ptr(), out.data_ptr(),
                                           R, rows_per_image, t.shape[0], Cc, H * W, alphas_cumprod.numel(), _stream()),
          "gad_add_noise_bcast")
    return out


def mse_segments_raw(pred, eps, rows_per_segment, out=None):
    """pred [R][H][W][C] (NHWC), eps [R][C][H][W] (NCHW) -> [R // rows_per_segment] fp32 means of (pred - eps)^2."""
    _req(pred, "mse_segments pred")
    _req(eps, "mse_segments eps")
    R, Cc, H, W = eps.shape
    if tuple(pred.shape) != (R, H, W, Cc):
        raise _capi.GadError(f"mse_segments: pred {tuple(pred.shape)} is not the NHWC shape of eps {tuple(eps.shape)}")
    lib = _capi.load()
    need = lib.gad_mse_segments_workspace_bytes(R, rows_per_segment, Cc, H * W)
    if need < 0:
        raise _capi.GadError(f"gad_mse_segments: {lib.gad_last_error().decode()}")
    ws = _scratch("segments_ws", need, pred.device)
    S = R // max(rows_per_segment, 1)
    out = _out((S,), pred.device) if out is None else _req(out, "mse_segments out")
    if out.numel() != S:
        raise _capi.GadError(f"mse_segments: out holds {out.numel()} values for {S} segments")
    check(lib.gad_mse_segments(pred.data_ptr(), eps.data_ptr(), out.data_ptr(), R, rows_per_segment, Cc, H * W, ws.data_ptr(), need,
                               _stream()), "gad_mse_segments")
    return out


def sumsq_raw(g, out=None):
    ws = workspace(g.device)
    out = torch.empty(1, device=g.device, dtype=torch.float32) if out is None else out
    check(_capi.load().gad_sumsq(g.data_ptr(), out.data_ptr(), g.numel(), ws.data_ptr(), ws.numel(), _stream()), "gad_sumsq")
    return out


def clip_adam_ema_raw(p, g, m, v, ema, sumsq, *, max_norm, lr, betas, eps, weight_decay, adamw, step, ema_decay):
    written(p)        # p is the flat parameter buffer: a raw kernel moves its residents, which no version counter sees (gad/shadows.py)
    a = AdamArgs()
    a.p, a.g, a.m, a.v, a.ema = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), _ptr(ema)
    a.n = p.numel()
    a.sumsq = _ptr(sumsq)
    a.max_norm = max_norm
    a.lr, a.beta1, a.beta2, a.eps, a.weight_decay = lr, betas[0], betas[1], eps, weight_decay
    a.adamw, a.step, a.ema_decay = int(adamw), step, ema_decay
    check(_capi.load().gad_clip_adam_ema(C.byref(a), _stream()), "gad_clip_adam_ema")


def adam8_qmap(signed: bool) -> torch.Tensor:
    """The 256 ascending fp32 code values of the 8-bit optimizer's signed / unsigned map (host tensor; needs no GPU)"""
    buf = (C.c_float * 256)()
    check(_capi.load().gad_adam8_qmap(int(bool(signed)), buf), "gad_adam8_qmap")
    return torch.tensor(list(buf), dtype=torch.float32)


def clip_adam8_ema_raw(p, g, ema, state1, state2, absmax1, absmax2, m32, v32, blocks, sumsq, *, max_norm, lr, betas, eps, step, ema_decay):
    """Fused clip + 8-bit blockwise Adam + EMA (gad_clip_adam8_ema).  `blocks`: uint8 device tensor holding the gad_adam8_block
    table (training.adam8_blocks); each block carries its own decoupled weight decay."""
    written(p)        # as clip_adam_ema_raw: the raw kernel moves the flat buffer's residents
    if state1.dtype != torch.uint8 or state2.dtype != torch.uint8 or state1.numel() != p.numel() or state2.numel() != p.numel():
        raise _capi.GadError("clip_adam8_ema: state1 / state2 must be uint8 buffers as long as the flat parameter buffer")
    if absmax1.numel() != absmax2.numel() or m32.numel() != v32.numel() or g.numel() != p.numel():
        raise _capi.GadError("clip_adam8_ema: buffer lengths do not match")
    if blocks.dtype != torch.uint8 or blocks.numel() % C.sizeof(_capi.Adam8Block) or not blocks.is_contiguous():
        raise _capi.GadError("clip_adam8_ema: blocks is not a contiguous uint8 image of a gad_adam8_block table")
    a = Adam8Args()
    a.p, a.g, a.ema = p.data_ptr(), g.data_ptr(), _ptr(ema)
    a.state1, a.state2, a.absmax1, a.absmax2 = state1.data_ptr(), state2.data_ptr(), absmax1.data_ptr(), absmax2.data_ptr()
    a.m32, a.v32, a.blocks = m32.data_ptr(), v32.data_ptr(), blocks.data_ptr()
    a.n, a.n32, a.n_absmax, a.n_blocks = p.numel(), m32.numel(), absmax1.numel(), blocks.numel() // C.sizeof(_capi.Adam8Block)
    a.sumsq = _ptr(sumsq)
    a.max_norm = max_norm
    a.lr, a.beta1, a.beta2, a.eps = lr, betas[0], betas[1], eps
    a.step, a.ema_decay = step, ema_decay
    check(_capi.load().gad_clip_adam8_ema(C.byref(a), _stream()), "gad_clip_adam8_ema")


def ema_update_raw(ema, p, decay: float):
    check(_capi.load().gad_ema_update(ema.data_ptr(), p.data_ptr(), p.numel(), decay, _stream()), "gad_ema_update")


def wf_dots_raw(o, k, g, dots):
    """dots[0] = o.g, dots[1] = k.g (fp64 device pair) over three equally long fp32 vectors; partials in the stream's workspace"""
    ws = workspace(g.device)
    check(_capi.load().gad_wf_dots(o.data_ptr(), k.data_ptr(), g.data_ptr(), g.numel(), dots.data_ptr(), ws.data_ptr(), ws.numel(),
                                   _stream()), "gad_wf_dots")
    return dots


def wf_update_raw(o, k, dots, N: float):
    """k -= dots[1] / (N + dots[0]) * o;  o -= dots[0] / (N + dots[0]) * o  (both from the old o), in place"""
    check(_capi.load().gad_wf_update(o.data_ptr(), k.data_ptr(), dots.data_ptr(), float(N), o.numel(), _stream()), "gad_wf_update")


def _lora_dropout_args(x2, downs, p, scale, seed, offset, layer, max_blocks=0):
    """gad_lora_dropout_args over tokens x2 [M, C] and the contiguous down matrices [r, C] of the projections that share them,
    with the stream's workspace (csrc/lora.hip)"""
    M, Cc = x2.shape
    a = _capi.LoraDropoutArgs()
    a.x, a.ldx, a.M, a.C = _req_rows(x2, "lora x").data_ptr(), (x2.stride(0) if M > 1 else Cc), M, Cc
    a.r, a.n_proj, a.layer = downs[0].shape[0], len(downs), layer
    for j, d in enumerate(downs):
        a.A[j] = _req(d, "lora down").data_ptr()
    a.p, a.scale, a.seed, a.offset, a.max_blocks = float(p), float(scale), seed & 0xFFFFFFFF, offset & 0xFFFFFFFF, max_blocks
    ws = workspace(x2.device)
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
    return a


def _req_rows(t, name):
    if not (t.is_cuda and t.dtype == torch.float32 and t.ndim == 2 and t.stride(1) == 1):
        raise _capi.GadError(f"{name}: expected an fp32 device matrix with contiguous rows, got {t.dtype} {t.device} strides {t.stride()}")
    return t


def lora_down_dropout_fwd_raw(x2, downs, p, scale, seed, offset, layer, max_blocks=0):
    """mid_j = scale * (x o m_j / (1 - p)) A_j^T for every projection j from one read of x -> [mid_j [M, r]]"""
    a = _lora_dropout_args(x2, downs, p, scale, seed, offset, layer, max_blocks)
    mids = [torch.empty((x2.shape[0], a.r), device=x2.device, dtype=torch.float32) for _ in downs]
    for j, m in enumerate(mids):
        a.mid[j] = m.data_ptr()
    check(_capi.load().gad_lora_down_dropout_fwd(C.byref(a), _stream()), "gad_lora_down_dropout_fwd")
    return mids


def lora_down_dropout_bwd_raw(x2, downs, dmids, dx2, p, seed, offset, layer, outs=None):
    """dA_j = dmid_j^T (x o m_j / (1 - p)) -> [dA_j [r, C]] (into `outs[j]` where given), and dx2 += sum_j (dmid_j A_j) o m_j / (1 - p)
    in place, with the forward's masks"""
    a = _lora_dropout_args(x2, downs, p, 1.0, seed, offset, layer)
    outs = list(outs) if outs is not None else [None] * len(downs)
    for j, d in enumerate(downs):
        if outs[j] is None:
            outs[j] = torch.empty_like(d)
        a.dmid[j], a.dA[j] = _req(dmids[j], "lora dmid").data_ptr(), _req(outs[j], "lora dA").data_ptr()
    a.dx, a.ld_dx = _req_rows(dx2, "lora dx").data_ptr(), (dx2.stride(0) if dx2.shape[0] > 1 else dx2.shape[1])
    check(_capi.load().gad_lora_down_dropout_bwd(C.byref(a), _stream()), "gad_lora_down_dropout_bwd")
    return outs


def lora_merge_raw(w, up, down, alpha):
    """w [N, K] += alpha * up [N, r] @ down [r, K] in place (merge_and_unload; -alpha unmerges)"""
    N, K = w.shape
    check(_capi.load().gad_lora_merge(_req_rows(w, "lora merge W").data_ptr(), w.stride(0) if N > 1 else K, _req(up, "lora up").data_ptr(),
                                      _req(down, "lora down").data_ptr(), N, K, up.shape[1], float(alpha), _stream()), "gad_lora_merge")
    written_everywhere()        # a device-pointer write: whatever is derived from w must refresh


class LoraDropoutQKVFn(torch.autograd.Function):
    """The three LoRA projections of one attention block as ONE autograd node (peft: y_j = x W_j^T + b_j + s (drop_j(x) A_j^T) B_j^T,
    each projection with its own dropout mask; reference unconditional_generation/unlearn.py:410-416).
    Forward:  gad_lora_down_dropout_fwd once (x read once, masks regenerated, never stored), then per projection the
              K-concatenated launch over [x | mid_j] . [W_j | B_j]^T (base + side GEMM where the shapes rule that out).
    Backward: dmid_j = s dy_j B_j and dB_j = dy_j^T mid_j (small GEMMs), the base data gradient sum_j dy_j W_j (each launch adds
              onto the previous one in its epilogue), then gad_lora_down_dropout_bwd for dA_j and the LoRA part of dx.
    The base weights are frozen (get_peft_model): no dW / db is formed."""

    @staticmethod
    def forward(ctx, x, ws_, bs_, meta, *ab):
        n = len(ws_)
        downs, ups = ab[:n], ab[n:]
        p, s, seed, offset, layer = meta
        shp = x.shape
        x2 = _req(x, "lora qkv x").view(-1, shp[-1])
        M, K = x2.shape
        r = downs[0].shape[0]
        mids = lora_down_dropout_fwd_raw(x2, [d.detach() for d in downs], p, s, seed, offset, layer)
        ys = []
        for w, b, up, mid in zip(ws_, bs_, ups, mids):
            N = w.shape[0]
            y = torch.empty((M, N), device=x.device, dtype=torch.float32)
            if lora_fusable(K, N, r):
                gemm_raw(x2, w, y, A_KC, B_KC, M, N, K + r, K, K, N, bias=b, A_k2=mid, B_k2=up, k_split=K)
            else:
                base = linear_fwd_raw(x2, w, b)
                gemm_raw(mid, up, y, A_KC, B_KC, M, N, r, r, r, N, residual=base, ldr=N)
            ys.append(y.view(*shp[:-1], N))
        ctx.save_for_backward(x2, *downs, *ups, *mids)
        ctx.frozen, ctx.meta, ctx.shp, ctx.n = (ws_, bs_), meta, shp, n
        return tuple(ys)

    @staticmethod
    def backward(ctx, *dys):
        n = ctx.n
        saved = ctx.saved_tensors
        x2, downs, ups, mids = saved[0], saved[1:1 + n], saved[1 + n:1 + 2 * n], saved[1 + 2 * n:]
        ws_, _ = ctx.frozen
        p, s, seed, offset, layer = ctx.meta
        M, K = x2.shape
        r = downs[0].shape[0]
        dx = torch.empty((M, K), device=x2.device, dtype=torch.float32)
        dmids, d_ups = [], []
        for j, (w, up, mid) in enumerate(zip(ws_, ups, mids)):
            N = w.shape[0]
            dy2 = dys[j].contiguous().view(-1, N)
            dmid = torch.empty((M, r), device=x2.device, dtype=torch.float32)
            gemm_raw(dy2, up, dmid, A_KC, B_MC, M, r, N, N, r, r, alpha=s)                         # s dy B
            dmids.append(dmid)
            d_ups.append(_param_grad(up, lambda o, dy2=dy2, mid=mid: linear_wgrad_raw(dy2, mid, out=o)))   # dy^T mid
            gemm_raw(dy2, w, dx, A_KC, B_MC, M, K, N, N, K, K, residual=dx if j else None, ldr=K if j else 0)   # dx (+)= dy W
        sinks = [_sink(d) for d in downs]
        outs = [v if (v is not None and first) else None for v, first in sinks]
        dAs = lora_down_dropout_bwd_raw(x2, [d.detach() for d in downs], dmids, dx, p, seed, offset, layer, outs=outs)
        d_downs = []
        for (v, first), g in zip(sinks, dAs):
            if v is None:
                d_downs.append(g)
            else:
                if not first:
                    v.add_(g)
                d_downs.append(None)
        return (dx.view(ctx.shp) if ctx.needs_input_grad[0] else None, None, None, None, *d_downs, *d_ups)


def lora_dropout_qkv(x, ws_, bs_, downs, ups, p, s, seed, offset, layer):
    """(q, k, v) of an attention block under LoRA with dropout; `ws_` / `bs_` the frozen base weights and biases"""
    return LoraDropoutQKVFn.apply(x, tuple(ws_), tuple(bs_), (float(p), float(s), int(seed), int(offset), int(layer)), *downs, *ups)


# ----------------------------------------------------------------------------------
# transformer-block operators (UNet2DConditionModel)
# ----------------------------------------------------------------------------------
class LayerNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, eps):
        y, mean, rstd = layernorm_fwd_raw(_req(x, "layernorm x"), gamma, beta, eps)
        ctx.save_for_backward(x, gamma, mean, rstd)
        ctx.beta_ref = beta
        return y

    @staticmethod
    def backward(ctx, dy, dbypass=None):
        x, gamma, mean, rstd = ctx.saved_tensors
        dy = dy.contiguous()
        C_ = x.shape[-1]
        rows = x.numel() // C_
        dx = torch.empty_like(x)
        want = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]            # frozen LayerNorm (LoRA training): dx only
        dgb = torch.empty(2 * C_, device=x.device, dtype=torch.float32) if want else None
        ws = workspace(x.device)
        add = _req(dbypass.contiguous(), "layernorm bypass gradient") if dbypass is not None else None
        check(_capi.load().gad_layernorm_bwd(x.data_ptr(), dy.data_ptr(), dx.data_ptr(), _ptr(add), gamma.data_ptr(),
                                             mean.data_ptr(), rstd.data_ptr(), _ptr(dgb), rows, C_, ws.data_ptr(), ws.numel(),
                                             _stream()), "gad_layernorm_bwd")
        if not want:
            return dx, None, None, None
        return dx, _deliver(gamma, dgb[:C_]), _deliver(ctx.beta_ref, dgb[C_:]), None


class LayerNormBypassFn(LayerNormFn):
    """(LayerNorm(x), alias of x): the residual branch of a transformer sub-block takes the alias, so the norm's backward
    receives both gradients and adds them in its own store (see GroupNormBypassFn)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps):
        return LayerNormFn.forward(ctx, x, gamma, beta, eps), x.view_as(x)

    @staticmethod
    def backward(ctx, dy, dbypass):
        if dy is None:
            return dbypass, None, None, None
        return LayerNormFn.backward(ctx, dy, dbypass)


def layer_norm(x, gamma, beta, eps=1e-5):
    if x.dtype == torch.bfloat16:
        return _half().layer_norm(x, gamma, beta, eps)
    return LayerNormFn.apply(x, gamma, beta, eps)


def layer_norm_bypass(x, gamma, beta, eps=1e-5):
    if x.dtype == torch.bfloat16:
        return _half().layer_norm_bypass(x, gamma, beta, eps)
    if not (torch.is_grad_enabled() and x.requires_grad):
        return layer_norm(x, gamma, beta, eps), x
    return LayerNormBypassFn.apply(x, gamma, beta, eps)


class GegluFn(torch.autograd.Function):
    """out = h[..., :F] * gelu(h[..., F:])  (diffusers GEGLU after its projection)."""

    @staticmethod
    def forward(ctx, h):
        _req(h, "geglu h")
        F2 = h.shape[-1]
        out = torch.empty((*h.shape[:-1], F2 // 2), device=h.device, dtype=torch.float32)
        check(_capi.load().gad_geglu_fwd(h.data_ptr(), out.data_ptr(), h.numel() // F2, F2 // 2, _stream()), "gad_geglu_fwd")
        ctx.save_for_backward(h)
        return out

    @staticmethod
    def backward(ctx, dout):
        (h,) = ctx.saved_tensors
        dout = dout.contiguous()
        F2 = h.shape[-1]
        dh = torch.empty_like(h)
        check(_capi.load().gad_geglu_bwd(h.data_ptr(), dout.data_ptr(), dh.data_ptr(), h.numel() // F2, F2 // 2, _stream()),
              "gad_geglu_bwd")
        return dh


def geglu(h):
    if h.dtype == torch.bfloat16:
        return _half().geglu(h)
    return GegluFn.apply(h)


def cfg_ddim_step_raw(x, eps_uc, guidance: float, alpha_t: float, alpha_prev: float, clip: float, out=None):
    """x [n...], eps_uc = U-Net output of the doubled batch [uncond ; cond] -> guided DDIM update of x."""
    _req(x, "cfg x")
    _req(eps_uc, "cfg eps")
    if eps_uc.numel() != 2 * x.numel():
        raise _capi.GadError("cfg_ddim_step: eps must hold the doubled batch")
    out = torch.empty_like(x) if out is None else out
    check(_capi.load().gad_cfg_ddim_step(x.data_ptr(), eps_uc.data_ptr(), out.data_ptr(), x.numel(), guidance, alpha_t,
                                         alpha_prev, clip, _stream()), "gad_cfg_ddim_step")
    return out


def _req_half_rows(t, name):
    if not (t.is_cuda and t.dtype == torch.float16 and t.dim() == 2 and t.stride(1) == 1 and t.stride(0) >= t.shape[1]):
        raise _capi.GadError(f"{name}: expected a row-major fp16 device matrix, got {t.dtype} {t.device} strides {tuple(t.stride())}")
    return t


def manifold_radii_raw(features, k):
    """fp16 [N, D] (row stride >= D) -> fp16 [N]: every row's distance to its k-th nearest other row (gad_manifold_radii)."""
    f = _req_half_rows(features, "manifold features")
    lib = _capi.load()
    N, D = f.shape
    nbytes = lib.gad_manifold_radii_workspace_bytes(N, D, f.stride(0), k)
    check(nbytes < 0, "gad_manifold_radii_workspace_bytes")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=f.device)
    kth = torch.empty(N, dtype=torch.float16, device=f.device)
    check(lib.gad_manifold_radii(f.data_ptr(), N, D, f.stride(0), k, kth.data_ptr(), ws.data_ptr(), nbytes, _stream()),
          "gad_manifold_radii")
    return kth


def manifold_cover_raw(probe, target, kth_target):
    """fp16 [Np, D], [Nt, D], fp16 radii [Nt] -> uint8 [Np]: the probe lies inside some target's ball (gad_manifold_cover)."""
    p, t = _req_half_rows(probe, "manifold probes"), _req_half_rows(target, "manifold targets")
    if p.shape[1] != t.shape[1] or kth_target.shape != (t.shape[0],) or kth_target.dtype != torch.float16 \
            or not kth_target.is_contiguous() or kth_target.device != t.device:
        raise _capi.GadError("manifold_cover: probes and targets must share D, radii must be contiguous fp16 [Nt] beside the targets")
    lib = _capi.load()
    (Np, D), Nt = p.shape, t.shape[0]
    nbytes = lib.gad_manifold_cover_workspace_bytes(Np, p.stride(0), Nt, t.stride(0), D)
    check(nbytes < 0, "gad_manifold_cover_workspace_bytes")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=p.device)
    out = torch.empty(Np, dtype=torch.uint8, device=p.device)
    check(lib.gad_manifold_cover(p.data_ptr(), Np, p.stride(0), t.data_ptr(), Nt, t.stride(0), D, kth_target.data_ptr(),
                                 out.data_ptr(), ws.data_ptr(), nbytes, _stream()), "gad_manifold_cover")
    return out
