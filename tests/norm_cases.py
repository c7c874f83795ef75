"""Inputs, references and the acceptance bound for the norm conditioning tests (tests/test_norm_conditioning_cpu.py,
tests/test_gpu_norm_conditioning.py): GroupNorm / LayerNorm on data whose mean lies far from zero against its spread, where
`E[x^2] - E[x]^2` in fp32 cancels and a centred variance does not.  Nothing here needs a GPU.

Everything is compared with fp64 of the SAME stored values (fp32, or bf16-representable for the half path), so input
rounding is never charged to a kernel.  Tensors are [B, C, HW] (a group = `cpg` consecutive channels); the kernels' layout
is `channels_last(x)`.

The bound.  No absolute tolerance: the achievable error grows with |mean| / std (one input ulp against std).  A quantity is
accepted when

    max |got - want_fp64|  <=  K * max(e_ref, 2^-22 * max |want_fp64|),      K = 8

where e_ref is the error of torch's own fp32 CPU operator (F.group_norm / F.layer_norm; torch.var_mean for mean and rstd;
fp32 autograd for gradients) on the same input.  K covers another fixed summation order, an fp32 Chan merge over up to 128
chunks, rsqrtf and FMA contraction; the floor covers inputs on which torch happens to be exact.  bf16 outputs get one bf16
rounding of the result (2^-8 relative) on top; mean / rstd are fp32 in both paths and get none."""
import torch
import torch.nn.functional as F

K = 8.0
FLOOR = 2.0 ** -22
BF16_ROUNDING = 2.0 ** -8
EPS = 1e-5


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------------------ inputs ----
def offset(mean, std):
    def make(B, C, HW, G, seed=0):
        return mean + std * torch.randn(B, C, HW, generator=_gen(seed))
    return make


MIXED_MEANS = (0.0, 10.0, -10.0, 100.0, -100.0)


def mixed(B, C, HW, G, seed=0):
    """every group draws its own mean from {0, +-10, +-100}; neighbouring groups always differ"""
    g = _gen(seed)
    idx = torch.randint(0, 5, (B, G), generator=g)
    step = torch.randint(1, 5, (B, G), generator=g)
    for j in range(1, G):                                        # a neighbour with the same mean moves on by 1..4
        same = idx[:, j] == idx[:, j - 1]
        idx[:, j] = torch.where(same, (idx[:, j] + step[:, j]) % 5, idx[:, j])
    m = torch.tensor(MIXED_MEANS)[idx]
    x = torch.randn(B, G, C // G, HW, generator=g) + m[:, :, None, None]
    return x.view(B, C, HW)


def exact_shift(c, grid_log2=-10):
    """x0 + c with x0 on a 2^grid_log2 grid in [-4, 4): every sum x0 + c is exact in the storage type, so the fp64
    GroupNorm of x0 + c equals that of x0 and any loss is the kernel's"""
    def make(B, C, HW, G, seed=0):
        return exact_shift_base(B, C, HW, grid_log2, seed) + float(c)
    return make


def exact_shift_base(B, C, HW, grid_log2, seed=0):
    steps = int(round(4 * 2.0 ** -grid_log2))
    return torch.randint(-steps, steps, (B, C, HW), generator=_gen(seed)).float() * 2.0 ** grid_log2


def outlier(first):
    """N(0, 1) with one element per group set to 1000: the group's very first element (first pixel, first channel), or one
    elsewhere.  A statistic shifted by a pivot read from the data fails the first placement."""
    def make(B, C, HW, G, seed=0):
        x = torch.randn(B, G, C // G, HW, generator=_gen(seed))
        if first:
            x[:, :, 0, 0] = 1000.0
        else:
            x[:, :, C // G - 1, (HW * 5) // 7] = 1000.0
        return x.view(B, C, HW)
    return make


def constant(B, C, HW, G, seed=0):
    return torch.full((B, C, HW), 96.0)


# name -> (generator, |mean| / std of a group; 0 where that is not the point of the case)
FP32_CASES = {
    "offset(30,1)": (offset(30.0, 1.0), 30.0),
    "offset(100,1)": (offset(100.0, 1.0), 100.0),
    "offset(300,1)": (offset(300.0, 1.0), 300.0),
    "offset(30,0.1)": (offset(30.0, 0.1), 300.0),
    "offset(-100,1)": (offset(-100.0, 1.0), 100.0),
    "mixed": (mixed, 100.0),
    "exact_shift(0)": (exact_shift(0), 0.0),
    "exact_shift(64)": (exact_shift(64), 64 / 2.31),
    "exact_shift(512)": (exact_shift(512), 512 / 2.31),
    "outlier(first)": (outlier(True), 0.0),
    "outlier(elsewhere)": (outlier(False), 0.0),
    "constant": (constant, 0.0),
}


def _bf16(make):
    def wrapped(B, C, HW, G, seed=0):
        return make(B, C, HW, G, seed).to(torch.bfloat16).float()
    return wrapped


# bf16 storage: the values are bf16-representable and held in fp32
BF16_CASES = {
    "offset(30,1)": (_bf16(offset(30.0, 1.0)), 30.0),
    "offset(100,1)": (_bf16(offset(100.0, 1.0)), 100.0),
    "offset(300,1)": (_bf16(offset(300.0, 1.0)), 300.0),
    "offset(30,0.1)": (_bf16(offset(30.0, 0.1)), 300.0),
    "offset(-100,1)": (_bf16(offset(-100.0, 1.0)), 100.0),
    "mixed": (_bf16(mixed), 100.0),
    "exact_shift(0)": (exact_shift(0, -2), 0.0),
    "exact_shift(32)": (exact_shift(32, -2), 32 / 2.31),
    "exact_shift(64)": (exact_shift(64, -1), 64 / 2.31),
    "exact_shift(128)": (exact_shift(128, 0), 128 / 2.31),
    "outlier(first)": (_bf16(outlier(True)), 0.0),
    "outlier(elsewhere)": (_bf16(outlier(False)), 0.0),
    "constant": (constant, 0.0),
}
EXACT_SHIFTS = {"fp32": [(0, -10), (64, -10), (512, -10)], "bf16": [(0, -2), (32, -2), (64, -1), (128, 0)]}


def channels_last(x):
    """[B, C, HW] -> contiguous [B, HW, C]"""
    return x.transpose(1, 2).contiguous()


def affine(C, seed=0):
    g = _gen(1000 + seed)
    return 1 + 0.3 * torch.randn(C, generator=g), 0.2 * torch.randn(C, generator=g)


# --------------------------------------------------------------------------------------------------- references ----
def _max_err(a, b):
    return (a.double() - b.double()).abs().max().item()


def group_norm_reference(x, G, gamma, beta, eps=EPS, silu=False, dy=None):
    """-> (want, e_ref): fp64 values of y, mean, rstd (and dx, dgamma, dbeta when dy is given) for the fp32-held input
    x [B, C, HW], and the max error of torch's fp32 CPU arithmetic on the same input for each of them"""
    def run(dt):
        xr = x.detach().to(dt, copy=True).requires_grad_(dy is not None)                # (copies: x itself stays a plain tensor)
        ga, be = (t.detach().to(dt, copy=True).requires_grad_(dy is not None) for t in (gamma, beta))
        y = F.group_norm(xr, G, ga, be, eps)
        if silu:
            y = F.silu(y)
        var, mean = torch.var_mean(x.to(dt).view(x.shape[0], G, -1), -1, unbiased=False)
        out = {"y": y.detach(), "mean": mean, "rstd": torch.rsqrt(var + eps)}
        if dy is not None:
            y.backward(dy.to(dt))
            out.update(dx=xr.grad, dgamma=ga.grad, dbeta=be.grad)
        return out
    want = run(torch.float64)
    got32 = run(torch.float32)
    e_ref = {k: _max_err(got32[k], want[k]) for k in want}
    return want, e_ref


def layer_norm_reference(x, gamma, beta, eps=EPS, dy=None):
    """the same for LayerNorm over the last axis of x [rows, C]"""
    def run(dt):
        xr = x.detach().to(dt, copy=True).requires_grad_(dy is not None)                # (copies: x itself stays a plain tensor)
        ga, be = (t.detach().to(dt, copy=True).requires_grad_(dy is not None) for t in (gamma, beta))
        y = F.layer_norm(xr, (x.shape[-1],), ga, be, eps)
        var, mean = torch.var_mean(x.to(dt), -1, unbiased=False)
        out = {"y": y.detach(), "mean": mean, "rstd": torch.rsqrt(var + eps)}
        if dy is not None:
            y.backward(dy.to(dt))
            out.update(dx=xr.grad, dgamma=ga.grad, dbeta=be.grad)
        return out
    want = run(torch.float64)
    got32 = run(torch.float32)
    return want, {k: _max_err(got32[k], want[k]) for k in want}


# -------------------------------------------------------------------------------------------------------- bound ----
def bound(e_ref, want, k=K):
    return k * max(e_ref, FLOOR * want.abs().max().item())


def ratio(got, want, e_ref, bf16_out=False, k=K):
    """worst |got - want| over its allowance; accepted when <= 1.  bf16_out adds one bf16 rounding of the result."""
    g, w = got.detach().cpu().double(), want.detach().cpu().double()
    assert g.shape == w.shape, (g.shape, w.shape)
    tol = torch.full_like(w, bound(e_ref, w, k))
    if bf16_out:
        tol = tol + w.abs() * BF16_ROUNDING
    err = (g - w).abs()
    return torch.where(err == 0, torch.zeros_like(err), err / tol).max().item()        # (0 / 0: exact where the bound is 0)


def check(got, want, e_ref, keys=None, bf16_out=(), label=""):
    """assert every quantity of `got` (dict) inside the bound; prints each figure first.
    A figure is err / (K * max(e_ref, floor)): <= 1 passes, and times K it is the kernel / torch-fp32 ratio."""
    bad = []
    for k in keys or got.keys():
        r = ratio(got[k], want[k], e_ref[k], bf16_out=k in bf16_out)
        err = _max_err(got[k].detach().cpu(), want[k])
        line = f"{label:58s} {k:7s} err {err:9.3e}  torch-fp32 {e_ref[k]:9.3e}  err/bound {r:8.3f}"
        print(line, flush=True)
        if not r <= 1.0:
            bad.append(line)
    assert not bad, "outside K * max(e_ref, 2^-22 max|want|):\n" + "\n".join(bad)


# --------------------------------------------------------------------------- fp32 emulations of the two formulas ----
def emulate_group_norm(x, G, chunk_pixels, centred, eps=EPS):
    """fp32 torch restatement of a chunked GroupNorm statistic on x [B, C, HW]: per chunk of `chunk_pixels` pixels (None:
    the whole group at once) either sums S, SS and m2 = max(SS - S mean, 0)  (centred = False), or the chunk mean first
    and then sum (x - mean)^2  (centred = True); chunks merged in order with Chan's formula in fp32.
    -> dict(y (no affine), mean, rstd)"""
    B, C, HW = x.shape
    cpg = C // G
    xg = x.view(B, G, cpg, HW)
    n = torch.zeros(B, G)
    mean = torch.zeros(B, G)
    m2 = torch.zeros(B, G)
    cp = chunk_pixels or HW
    for p0 in range(0, HW, cp):
        c = xg[..., p0:p0 + cp]
        nb = float(c.shape[-1] * cpg)
        if centred:
            mb = c.sum((2, 3)) / nb
            d0 = c - mb[..., None, None]
            m2b = (d0 * d0).sum((2, 3))
        else:
            S = c.sum((2, 3))
            SS = (c * c).sum((2, 3))
            mb = S / nb
            m2b = (SS - S * mb).clamp_min(0)
        d = mb - mean
        nt = n + nb
        mean = mean + d * (nb / nt)
        m2 = m2 + m2b + d * d * (n * nb / nt)
        n = nt
    rstd = torch.rsqrt(m2 / n + eps)
    y = ((xg - mean[..., None, None]) * rstd[..., None, None]).view(B, C, HW)
    return {"y": y, "mean": mean, "rstd": rstd}
