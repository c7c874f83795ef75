"""The host side of the fp32 convolution launches, traced without a GPU: every public entry of gad/ops.py that launches a
convolution is driven with CPU tensors against a proxy around the REAL library that records the launch symbols instead of
running them and counts the (pure host) route queries it passes through.  tests/golden/make_conv_launch_trace.py records
CASES into tests/golden/conv_launch_trace.json; tests/test_conv_launch_cpu.py replays them against the current ops.py.

A launch is [symbol, argument, ...]: an argument struct is the list of its fields in declaration order, a pointer is null
(None), [name, byte offset] inside an allocation the trace knows - the case's own tensors, the workspace and whatever
ops.SCRATCH_ALLOC / ops.OUT_ALLOC handed out - or "unnamed".  Hook allocations are named `<kind><n>:<bytes>`, n counting the
allocations of that kind in the order the launches first use them, so a scratch region is pinned to its exact size and an
allocation no launch reads changes nothing.  gad_gemm launches also carry the route the library resolves for the arguments
as launched: [kernel id, tile, split, vec, workspace bytes, Winograd bytes]."""
import ctypes as C
from contextlib import contextmanager

import torch

from gad import _capi, ops
from gad.training import flatten_params

QUERIES = ("gad_gemm_kernel_id", "gad_gemm_plan", "gad_gemm_wino_bytes", "gad_gemm_workspace_bytes", "gad_groupnorm_wino4_ok")
P1, P0 = (1, 1, 1, 1), (0, 0, 0, 0)


def _is_host_query(name):
    return name in QUERIES or name.endswith(("_bytes", "_ok", "_supported", "_uses_bf16", "_one_pass")) or name in ("gad_version", "gad_last_error")


class Proxy:
    """libgad_hip.so with its launches recorded (never executed: there is no GPU) and its route queries counted"""

    def __init__(self, lib, env):
        self._lib, self._env = lib, env

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not _is_host_query(name):
            return lambda *args: self._env.launch(name, args)
        if name not in QUERIES:
            return fn

        def counted(*args):
            self._env.queries[name] = self._env.queries.get(name, 0) + 1
            return fn(*args)
        return counted


class Env:
    """One case's world: named allocations, the recorded launches, the query counts."""

    def __init__(self, lib, hooked):
        self.lib, self.hooked = lib, hooked
        self.allocs, self.keep, self.names, self.counts = [], [], {}, {}      # [(first byte, end, kind, bytes)]
        self.launches, self.queries, self.stats = [], {}, None
        self.ws = self.named("ws", torch.empty(ops.WS_BYTES, dtype=torch.uint8), fixed=True)

    # ---- allocations ----
    def named(self, kind, t, fixed=False):
        self.keep.append(t)
        nbytes = t.numel() * t.element_size()
        self.allocs.append((t.data_ptr(), t.data_ptr() + max(nbytes, 1), kind, None if fixed else nbytes))
        return t

    def tensor(self, name, *shape):
        return self.named("in:" + name, torch.empty(shape, dtype=torch.float32), fixed=True)

    def weight(self, name, co, ci, k=3, grad=False):
        """a conv parameter: logical [Cout, Cin, k, k] over [Cout][k][k][Cin] storage"""
        w = self.tensor(name, co, k, k, ci).permute(0, 3, 1, 2)
        return w.requires_grad_(True) if grad else w

    def scratch_alloc(self, kind, nbytes, device):
        return self.named(kind, torch.empty(nbytes, dtype=torch.uint8))

    def out_alloc(self, shape, device):
        return self.named("out", torch.empty(shape, dtype=torch.float32))

    def pointer(self, p):
        if not p:
            return None
        for i, (lo, hi, kind, nbytes) in enumerate(self.allocs):
            if lo <= p < hi:
                if i not in self.names:
                    n = self.counts[kind] = self.counts.get(kind, -1) + 1
                    self.names[i] = kind if nbytes is None else f"{kind}{n}:{nbytes}"
                return [self.names[i], p - lo]
        return "unnamed"

    # ---- launches ----
    def struct(self, s):
        out = []
        for fname, ftype in s._fields_:
            v = getattr(s, fname)
            out.append(self.pointer(v) if ftype is C.c_void_p else self.struct(v) if isinstance(v, C.Structure) else v)
        return out

    def launch(self, name, args):
        rec = [name]
        for t, v in zip(_capi.SIGNATURES[name][1], args):
            if t is C.c_void_p:
                rec.append(self.pointer(v))
            elif isinstance(t, type) and issubclass(t, C._Pointer):
                rec.append(self.struct(v._obj))
            else:
                rec.append(v)
        if name == "gad_gemm":
            a = _capi.GemmArgs.from_buffer_copy(args[0]._obj)
            tile, sk, vec = C.c_int32(), C.c_int32(), C.c_int32()
            lib, r = self.lib, C.byref(a)
            assert lib.gad_gemm_plan(r, C.byref(tile), C.byref(sk), C.byref(vec)) == 0
            rec.append([lib.gad_gemm_kernel_id(r), tile.value, sk.value, vec.value, lib.gad_gemm_workspace_bytes(r), lib.gad_gemm_wino_bytes(r)])
        self.launches.append(rec)
        return 0

    def result(self):
        out = {"launches": self.launches, "queries": dict(sorted(self.queries.items()))}
        if self.stats is not None:
            out["route_stats"] = sorted([list(k), n] for k, n in self.stats.items())
        return out


class StubProfiler:
    """ops.PROFILER without HIP events: the queries GemmProfiler.gemm makes, then the launch"""

    def __init__(self):
        self.batches = []

    def gemm(self, lib, a, batch):
        tile, sk, vec = C.c_int32(), C.c_int32(), C.c_int32()
        _capi.check(lib.gad_gemm_plan(C.byref(a), C.byref(tile), C.byref(sk), C.byref(vec)), "gad_gemm_plan")
        lib.gad_gemm_kernel_id(C.byref(a))
        self.batches.append(batch)
        _capi.check(lib.gad_gemm(C.byref(a), None), "gad_gemm")


@contextmanager
def world(env):
    """ops.py on the CPU: the device checks, the stream and the per-stream workspace are replaced; the library is the proxy"""
    saved = (ops._req, ops._stream, ops.workspace, ops.SCRATCH_ALLOC, ops.OUT_ALLOC, ops.PROFILER, ops.ROUTE_STATS, _capi._lib)
    ops._req, ops._stream, ops.workspace = (lambda t, name: t), (lambda: None), (lambda device: env.ws)
    if env.hooked:
        ops.SCRATCH_ALLOC, ops.OUT_ALLOC = env.scratch_alloc, env.out_alloc
    _capi._lib = Proxy(env.lib, env)
    try:
        yield env
    finally:
        (ops._req, ops._stream, ops.workspace, ops.SCRATCH_ALLOC, ops.OUT_ALLOC, ops.PROFILER, ops.ROUTE_STATS, _capi._lib) = saved


def run_case(lib, fn, hooked):
    env = Env(lib, hooked)
    with world(env):
        fn(env)
    return env.result()


# ---- the drivers: one public entry each ----
def _epilogue(e, B, Ho, Wo, co):
    return dict(rowadd=e.tensor("rowadd", B, co), residual=e.tensor("residual", B, Ho, Wo, co))


def _out_hw(h, k, stride, pad, ups):
    h = 2 * h if ups else h
    return (h + pad[0] + pad[1] - k) // stride + 1


def fwd(B, hw, ci, co, k=3, stride=1, pad=P1, ups=False, hint=0, splitk=0, c2=0, epi=False, keep=None):
    def run(e):
        x = e.tensor("x", B, hw, hw, ci - c2)
        x2 = e.tensor("x2", B, hw, hw, c2) if c2 else None
        w = e.weight("w", co, ci, k)
        Ho = _out_hw(hw, k, stride, pad, ups)
        more = _epilogue(e, B, Ho, Ho, co) if epi else {}
        if keep is not None:
            more["keep_v"] = kept = []
        y = ops.conv2d_fwd_raw(x, w, e.tensor("bias", co) if epi else None, stride, pad, ups, tile_hint=hint, splitk_hint=splitk, x2=x2, **more)
        assert tuple(y.shape) == (B, Ho, Ho, co)
        if keep is not None:
            e.launches.append(["kept", [e.pointer(v.data_ptr()) for v in kept]])
    return run


def dgrad(B, hw, ci, co, k=3, stride=1, pad=P1, ups=False, hint=0, splitk=0):
    def run(e):
        Ho = _out_hw(hw, k, stride, pad, ups)
        dx = ops.conv2d_dgrad_raw(e.tensor("dy", B, Ho, Ho, co), e.weight("w", co, ci, k), (B, hw, hw, ci), stride, pad, ups, hint, splitk)
        assert tuple(dx.shape) == (B, hw, hw, ci)
    return run


def wgrad(B, hw, ci, co, k=3, stride=1, pad=P1, ups=False, hint=0, splitk=0, kept=None, out=False):
    """kept: None, "fwd" (the V a forward launch of the same convolution kept), or a byte count (a V of that size)"""
    def run(e):
        Ho = _out_hw(hw, k, stride, pad, ups)
        x, w = e.tensor("x", B, hw, hw, ci), e.weight("w", co, ci, k)
        V = None
        if kept == "fwd":
            keep = []
            ops.conv2d_fwd_raw(x, w, None, stride, pad, ups, keep_v=keep)
            V = keep[0] if keep else None
        elif kept is not None:
            V = e.named("v", torch.empty(kept, dtype=torch.uint8))
        dw = ops.conv2d_wgrad_raw(e.tensor("dy", B, Ho, Ho, co), x, w, stride, pad, ups, hint, splitk,
                                  out=e.weight("dw", co, ci, k) if out else None, wino_v=V)
        assert tuple(dw.shape) == (co, ci, k, k)
    return run


def gn_conv(B, hw, ci, co, c2=0, hint=0, epi=False, grad=False, G=32):
    def run(e):
        x = e.tensor("x", B, hw, hw, ci - c2)
        x2 = e.tensor("x2", B, hw, hw, c2) if c2 else None
        more = _epilogue(e, B, hw, hw, co) if epi else {}
        with torch.enable_grad() if grad else torch.no_grad():
            y = ops.gn_silu_conv3x3_raw(x, x2, e.tensor("gamma", ci), e.tensor("beta", ci), G, 1e-5, e.weight("w", co, ci),
                                        e.tensor("bias", co), tile_hint=hint, **more)
        assert tuple(y.shape) == (B, hw, hw, co)
    return run


def _weight_home(e, co, ci, k, home):
    """home: "frozen", "trainable" or "flat" (a parameter re-homed in a flat buffer beside a second 3x3 weight)"""
    if home != "flat":
        return e.weight("w", co, ci, k, grad=home == "trainable")
    ps = [torch.nn.Parameter(torch.zeros(c_o, k, k, c_i).permute(0, 3, 1, 2)) for c_o, c_i in ((co, ci), (64, 64))]
    flat, gflat = flatten_params(ps)
    e.named("in:flat", flat, fixed=True)
    e.named("in:flat_grad", gflat, fixed=True)
    return ps[0]


def conv_fn(B, hw, ci, co, k=3, stride=1, pad=P1, ups=False, home="trainable", epi=False, x_grad=True, sinks=False):
    def run(e):
        x = e.tensor("x", B, hw, hw, ci).requires_grad_(x_grad)
        w = _weight_home(e, co, ci, k, home)
        Ho = _out_hw(hw, k, stride, pad, ups)
        bias = e.tensor("bias", co).requires_grad_(True) if epi else None
        rowadd = e.tensor("rowadd", B, co).requires_grad_(True) if epi else None
        y = ops.Conv2dFn.apply(x, w, bias, rowadd, e.tensor("residual", B, Ho, Ho, co) if epi else None, stride, pad, ups)
        if sinks:
            ops.begin_backward_step()
        try:
            y.backward(e.tensor("dy", B, Ho, Ho, co))
        finally:
            ops.end_backward_step()
    return run


def gn_conv_fn(B, hw, ci, co, home="trainable", x_grad=True, bypass=False):
    def run(e):
        x = e.tensor("x", B, hw, hw, ci).requires_grad_(x_grad)
        w = _weight_home(e, co, ci, 3, home)
        gamma, beta = e.tensor("gamma", ci).requires_grad_(x_grad), e.tensor("beta", ci).requires_grad_(x_grad)
        y = ops.gn_silu_conv3x3(x, gamma, beta, 32, 1e-5, w, e.tensor("bias", co), bypass=bypass)
        y = y[0] if bypass else y
        if y.requires_grad:
            y.backward(e.tensor("dy", B, hw, hw, co))
    return run


def flags(fn, **kw):
    def run(e):
        with ops.kernel_flags(**kw):
            fn(e)
    return run


def precision(fn, name):
    def run(e):
        with ops.operand_precision(name):
            fn(e)
    return run


def profiled(fn):
    def run(e):
        ops.PROFILER = prof = StubProfiler()
        fn(e)
        e.launches.append(["profiler batches", prof.batches])
    return run


def counted(fn):
    def run(e):
        ops.ROUTE_STATS = e.stats = {}
        fn(e)
    return run


SWITCHES = ("no_patch", "tap_major_k", "gn_two_pass", "scalar_epilogue", "general_loaders", "native_dgrad", "two_kernel_attn_bwd",
            "narrow_attn_fwd", "no_wino", "no_wino4", "no_gn_wino")
CHANNELS = ((32, 64), (128, 128), (96, 224), (3, 64), (64, 3))
V_BYTES = 36 * (128 * 32 * 32 // 16) * 128 * 4           # the F(4x4) input image of a [128, 32, 32, 128] activation


def _cases():
    c = {}
    # forward: every map x batch with two of the channel pairs, every channel pair at 16 x 16 / B = 128
    for i, hw in enumerate((8, 16, 6, 7, 32)):
        for j, B in enumerate((1, 128, 1024)):
            for n in range(2):
                ci, co = CHANNELS[(2 * (3 * i + j) + n) % 5]
                c[f"fwd {hw}x{hw} B{B} {ci}->{co}"] = fwd(B, hw, ci, co)
    for ci, co in CHANNELS:
        c[f"fwd 16x16 B128 {ci}->{co}"] = fwd(128, 16, ci, co)
        c[f"fwd 8x8 B1024 {ci}->{co} epilogue"] = fwd(1024, 8, ci, co, epi=True)
    c["fwd 32x32 B1024 32->64"] = fwd(1024, 32, 32, 64)
    c["fwd 16x16 B128 128->128 epilogue keep"] = fwd(128, 16, 128, 128, epi=True, keep=True)
    c["fwd 6x6 B128 128->128 keep"] = fwd(128, 6, 128, 128, keep=True)
    c["fwd 8x8 B1 128->128 keep"] = fwd(1, 8, 128, 128, keep=True)
    # geometry
    c["fwd 1x1 16x16 B128 128->128"] = fwd(128, 16, 128, 128, k=1, pad=P0)
    c["fwd 1x1 16x16 B128 96->224 epilogue"] = fwd(128, 16, 96, 224, k=1, pad=P0, epi=True)
    c["fwd stride2 16x16 B128 128->128"] = fwd(128, 16, 128, 128, stride=2, pad=(0, 1, 0, 1))
    c["fwd stride2 pad1 32x32 B8 32->64"] = fwd(8, 32, 32, 64, stride=2)
    c["fwd upsample 8x8 B128 128->128"] = fwd(128, 8, 128, 128, ups=True)
    c["fwd upsample 16x16 B1024 32->64 keep"] = fwd(1024, 16, 32, 64, ups=True, keep=True)
    c["fwd two-source 16x16 B128 64+64->128"] = fwd(128, 16, 128, 128, c2=64)
    c["fwd two-source 1x1 16x16 B128 96+32->64"] = fwd(128, 16, 128, 64, k=1, pad=P0, c2=32)
    c["fwd pad0 16x16 B128 128->128"] = fwd(128, 16, 128, 128, pad=P0)
    # tile and split hints
    for hint in (7, 8, 9, 10, 11):
        c[f"fwd 16x16 B128 128->128 hint{hint}"] = fwd(128, 16, 128, 128, hint=hint, keep=True)
        c[f"fwd 8x8 B1 128->128 hint{hint}"] = fwd(1, 8, 128, 128, hint=hint)
    c["fwd 6x6 B128 128->128 hint7"] = fwd(128, 6, 128, 128, hint=7)
    c["fwd 6x6 B128 128->128 hint8"] = fwd(128, 6, 128, 128, hint=8)
    c["fwd 7x7 B128 128->128 hint7"] = fwd(128, 7, 128, 128, hint=7)
    c["fwd 16x16 B128 128->128 hint1"] = fwd(128, 16, 128, 128, hint=1)
    c["fwd 16x16 B128 128->128 splitk2"] = fwd(128, 16, 128, 128, splitk=2)
    c["fwd 8x8 B1 128->128 splitk2"] = fwd(1, 8, 128, 128, splitk=2)
    # every switch: forward, weight gradient, GroupNorm -> V
    for s in SWITCHES:
        c[f"fwd 16x16 B128 128->128 {s}"] = flags(fwd(128, 16, 128, 128, keep=True), **{s: True})
        c[f"wgrad 32x32 B128 128->128 {s}"] = flags(wgrad(128, 32, 128, 128, kept="fwd"), **{s: True})
    for s in ("gn_two_pass", "general_loaders", "no_wino", "no_wino4", "no_gn_wino"):
        c[f"gn_conv 16x16 B1024 128->128 {s}"] = flags(gn_conv(1024, 16, 128, 128), **{s: True})
    c["fwd 6x6 B128 128->128 no_wino4"] = flags(fwd(128, 6, 128, 128), no_wino4=True)
    c["dgrad 1x1 16x16 B128 128->128 general_loaders"] = flags(dgrad(128, 16, 128, 128, k=1, pad=P0), general_loaders=True)
    c["wgrad 1x1 16x16 B128 128->128 general_loaders"] = flags(wgrad(128, 16, 128, 128, k=1, pad=P0), general_loaders=True)
    # operand precision 1 and 2 where no bf16 weight is made (that branch asks the device for its capture state)
    for name in ("bf16-operands", "bf16"):
        c[f"fwd 16x16 B128 3->64 {name}"] = precision(fwd(128, 16, 3, 64), name)
        c[f"fwd 1x1 16x16 B128 128->128 {name}"] = precision(fwd(128, 16, 128, 128, k=1, pad=P0), name)
        c[f"fwd two-source 16x16 B128 64+64->128 {name}"] = precision(fwd(128, 16, 128, 128, c2=64), name)
        c[f"wgrad 32x32 B128 128->128 {name}"] = precision(wgrad(128, 32, 128, 128, kept=V_BYTES), name)
        c[f"dgrad 16x16 B128 128->128 {name}"] = precision(dgrad(128, 16, 128, 128), name)
        c[f"gn_conv 16x16 B128 48->64 {name}"] = precision(gn_conv(128, 16, 48, 64, G=16), name)
    # data gradient (the native kernels; the forward form on rotated weights is in the autograd cases)
    for B, hw, ci, co in ((128, 16, 128, 128), (1, 8, 32, 64), (1024, 8, 96, 224), (128, 7, 3, 64), (128, 32, 64, 3)):
        c[f"dgrad {hw}x{hw} B{B} {ci}->{co}"] = dgrad(B, hw, ci, co)
    c["dgrad 1x1 16x16 B128 128->128"] = dgrad(128, 16, 128, 128, k=1, pad=P0)
    c["dgrad 1x1 16x16 B128 3->64"] = dgrad(128, 16, 3, 64, k=1, pad=P0)
    c["dgrad 1x1 stride2 16x16 B128 128->128"] = dgrad(128, 16, 128, 128, k=1, stride=2, pad=P0)
    c["dgrad stride2 16x16 B128 128->128"] = dgrad(128, 16, 128, 128, stride=2, pad=(0, 1, 0, 1))
    c["dgrad upsample 8x8 B128 128->128"] = dgrad(128, 8, 128, 128, ups=True)
    c["dgrad 16x16 B128 128->128 hint1 splitk2"] = dgrad(128, 16, 128, 128, hint=1, splitk=2)
    # weight gradient: without a kept V, with the forward launch's, with one of the right size, with one too small
    for B, hw, ci, co in ((128, 16, 128, 128), (128, 32, 128, 128), (1024, 8, 96, 224), (1, 8, 32, 64), (128, 32, 32, 64), (128, 6, 128, 128), (128, 7, 128, 128),
                          (128, 16, 3, 64), (128, 16, 64, 3)):
        c[f"wgrad {hw}x{hw} B{B} {ci}->{co}"] = wgrad(B, hw, ci, co)
        c[f"wgrad {hw}x{hw} B{B} {ci}->{co} kept"] = wgrad(B, hw, ci, co, kept="fwd")
    c["wgrad 32x32 B128 128->128 kept V"] = wgrad(128, 32, 128, 128, kept=V_BYTES)
    c["wgrad 32x32 B128 128->128 kept V too small"] = wgrad(128, 32, 128, 128, kept=V_BYTES - 4)
    c["wgrad 32x32 B128 128->128 kept V out"] = wgrad(128, 32, 128, 128, kept=V_BYTES, out=True)
    c["wgrad 16x16 B128 128->128 out"] = wgrad(128, 16, 128, 128, out=True)
    for hint in (8, 1):
        c[f"wgrad 32x32 B128 128->128 hint{hint} kept V"] = wgrad(128, 32, 128, 128, hint=hint, kept=V_BYTES)
        c[f"wgrad 16x16 B128 128->128 hint{hint} kept"] = wgrad(128, 16, 128, 128, hint=hint, kept="fwd")
        c[f"wgrad 8x8 B1 128->128 hint{hint}"] = wgrad(1, 8, 128, 128, hint=hint)
    c["wgrad 32x32 B128 128->128 splitk2 kept V"] = wgrad(128, 32, 128, 128, splitk=2, kept=V_BYTES)
    c["wgrad 1x1 16x16 B128 128->128"] = wgrad(128, 16, 128, 128, k=1, pad=P0)
    c["wgrad 1x1 16x16 B128 3->64"] = wgrad(128, 16, 3, 64, k=1, pad=P0)
    c["wgrad stride2 16x16 B128 128->128"] = wgrad(128, 16, 128, 128, stride=2, pad=(0, 1, 0, 1))
    c["wgrad upsample 8x8 B128 128->128 kept"] = wgrad(128, 8, 128, 128, ups=True, kept="fwd")
    c["wgrad pad0 16x16 B128 128->128"] = wgrad(128, 16, 128, 128, pad=P0)
    # GroupNorm writes V (the sampler's ResnetBlock2D halves)
    for B, hw, ci, co in ((1024, 16, 128, 128), (1024, 8, 256, 256), (128, 32, 128, 128), (1, 8, 128, 128), (128, 16, 96, 224), (128, 6, 128, 128),
                          (128, 16, 128, 32), (1024, 32, 32, 64)):
        c[f"gn_conv {hw}x{hw} B{B} {ci}->{co}"] = gn_conv(B, hw, ci, co)
    c["gn_conv 16x16 B1024 128->128 epilogue"] = gn_conv(1024, 16, 128, 128, epi=True)
    c["gn_conv two-source 16x16 B1024 128+128->128"] = gn_conv(1024, 16, 256, 128, c2=128, epi=True)
    c["gn_conv two-source 8x8 B1 64+64->128"] = gn_conv(1, 8, 128, 128, c2=64)
    c["gn_conv 16x16 B1024 128->128 grad enabled"] = gn_conv(1024, 16, 128, 128, grad=True)
    for hint in (7, 8, 9, 10, 11, 1):
        c[f"gn_conv 16x16 B1024 128->128 hint{hint}"] = gn_conv(1024, 16, 128, 128, hint=hint)
    # autograd: forward + backward, for the kept V and both forms of the data gradient
    for home in ("trainable", "frozen", "flat"):
        c[f"Conv2dFn 16x16 B128 128->128 {home}"] = conv_fn(128, 16, 128, 128, home=home, epi=True)
        c[f"Conv2dFn 8x8 B1 128->128 {home}"] = conv_fn(1, 8, 128, 128, home=home)
        c[f"GnSiluConv3x3Fn 16x16 B128 128->128 {home}"] = gn_conv_fn(128, 16, 128, 128, home=home)
    c["Conv2dFn 16x16 B128 128->128 flat sinks"] = conv_fn(128, 16, 128, 128, home="flat", sinks=True)
    c["Conv2dFn 16x16 B128 128->128 flat native_dgrad"] = flags(conv_fn(128, 16, 128, 128, home="flat"), native_dgrad=True)
    c["Conv2dFn 16x16 B128 128->128 no x grad"] = conv_fn(128, 16, 128, 128, x_grad=False)
    c["Conv2dFn upsample 8x8 B128 128->128 frozen"] = conv_fn(128, 8, 128, 128, ups=True, home="frozen")
    c["Conv2dFn upsample 8x8 B128 128->128 trainable"] = conv_fn(128, 8, 128, 128, ups=True)
    c["Conv2dFn 1x1 16x16 B128 128->128"] = conv_fn(128, 16, 128, 128, k=1, pad=P0)
    c["Conv2dFn stride2 16x16 B128 128->128"] = conv_fn(128, 16, 128, 128, stride=2, pad=(0, 1, 0, 1))
    c["Conv2dFn 16x16 B128 3->64"] = conv_fn(128, 16, 3, 64)
    c["Conv2dFn 6x6 B128 128->128 frozen"] = conv_fn(128, 6, 128, 128, home="frozen")
    c["Conv2dFn 32x32 B128 32->64"] = conv_fn(128, 32, 32, 64)
    c["Conv2dFn 32x32 B128 128->128"] = conv_fn(128, 32, 128, 128, epi=True)
    c["Conv2dFn 32x32 B128 128->128 flat sinks"] = conv_fn(128, 32, 128, 128, home="flat", sinks=True)
    c["GnSiluConv3x3Fn 32x32 B128 128->128"] = gn_conv_fn(128, 32, 128, 128)
    c["GnSiluConv3x3Fn 16x16 B128 128->128 bypass"] = gn_conv_fn(128, 16, 128, 128, bypass=True)
    c["GnSiluConv3x3Fn 16x16 B128 128->128 frozen no x grad"] = gn_conv_fn(128, 16, 128, 128, home="frozen", x_grad=False)
    c["GnSiluConv3x3Fn 8x8 B1024 96->224"] = gn_conv_fn(1024, 8, 96, 224)
    # the profiler and the route statistics
    c["profiled fwd 16x16 B128 128->128"] = profiled(fwd(128, 16, 128, 128, keep=True))
    c["profiled fwd 6x6 B128 128->128"] = profiled(fwd(128, 6, 128, 128))
    c["profiled wgrad 16x16 B128 128->128 kept"] = profiled(wgrad(128, 16, 128, 128, kept="fwd"))
    c["profiled gn_conv 16x16 B1024 128->128"] = profiled(gn_conv(1024, 16, 128, 128))
    c["profiled dgrad 1x1 16x16 B128 128->128"] = profiled(dgrad(128, 16, 128, 128, k=1, pad=P0))
    c["counted fwd 16x16 B128 128->128"] = counted(fwd(128, 16, 128, 128))
    c["counted fwd 6x6 B128 128->128"] = counted(fwd(128, 6, 128, 128))
    c["counted fwd 8x8 B1 128->128"] = counted(fwd(1, 8, 128, 128))
    c["counted gn_conv 16x16 B1024 128->128"] = counted(gn_conv(1024, 16, 128, 128))
    c["counted gn_conv 8x8 B1 128->128"] = counted(gn_conv(1, 8, 128, 128))
    c["counted Conv2dFn 16x16 B128 128->128"] = counted(conv_fn(128, 16, 128, 128))
    c["counted wgrad 8x8 B1 128->128"] = counted(wgrad(1, 8, 128, 128))
    c["counted Conv2dFn 32x32 B128 128->128"] = counted(conv_fn(128, 32, 128, 128))
    c["counted wgrad 32x32 B128 128->128"] = counted(wgrad(128, 32, 128, 128))
    c["profiled wgrad 32x32 B128 128->128 kept"] = profiled(wgrad(128, 32, 128, 128, kept="fwd"))
    return c


HOOKED = _cases()
# the production path - no allocation hook set, so no canary workspace query: outputs and scratch are "unnamed"
UNHOOKED = {name: HOOKED[name] for name in (
    "fwd 16x16 B128 128->128", "fwd 8x8 B1024 96->224 epilogue", "fwd 6x6 B128 128->128 keep", "fwd 8x8 B1 128->128 keep",
    "fwd 16x16 B128 128->128 epilogue keep", "fwd 7x7 B128 32->64", "fwd 32x32 B1024 32->64", "fwd 1x1 16x16 B128 128->128",
    "fwd two-source 16x16 B128 64+64->128", "fwd upsample 16x16 B1024 32->64 keep", "fwd 16x16 B128 128->128 hint7",
    "fwd 16x16 B128 128->128 hint9", "fwd 16x16 B128 128->128 splitk2", "fwd 16x16 B128 128->128 no_wino4", "fwd 16x16 B128 3->64 bf16-operands",
    "dgrad 16x16 B128 128->128", "dgrad 1x1 16x16 B128 128->128", "dgrad upsample 8x8 B128 128->128",
    "wgrad 16x16 B128 128->128", "wgrad 16x16 B128 128->128 kept", "wgrad 32x32 B128 128->128 kept", "wgrad 32x32 B128 128->128 kept V too small", "wgrad 8x8 B1 32->64",
    "wgrad 1x1 16x16 B128 128->128", "wgrad 32x32 B128 128->128 general_loaders", "Conv2dFn 32x32 B128 128->128", "counted Conv2dFn 32x32 B128 128->128",
    "gn_conv 16x16 B1024 128->128", "gn_conv 8x8 B1 128->128", "gn_conv two-source 16x16 B1024 128+128->128", "gn_conv 16x16 B1024 128->128 hint7",
    "gn_conv 16x16 B128 128->32", "gn_conv 16x16 B1024 128->128 no_gn_wino",
    "Conv2dFn 16x16 B128 128->128 trainable", "Conv2dFn 16x16 B128 128->128 frozen", "Conv2dFn 16x16 B128 128->128 flat",
    "Conv2dFn 16x16 B128 128->128 flat sinks", "GnSiluConv3x3Fn 16x16 B128 128->128 trainable", "GnSiluConv3x3Fn 16x16 B128 128->128 flat",
    "profiled fwd 16x16 B128 128->128", "counted Conv2dFn 16x16 B128 128->128", "counted gn_conv 16x16 B1024 128->128")}
CASES = [(name, fn, True) for name, fn in HOOKED.items()] + [(name + " [no hooks]", fn, False) for name, fn in UNHOOKED.items()]
