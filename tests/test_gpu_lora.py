"""GPU tests of LoRA unlearning: the dropout LoRA down-projection kernels and the merge (csrc/lora.hip) against fp64 numpy with
the restated masks (tests/lora_ref.py), one LoRA step and two LoRA+ optimizer steps of the TINY U-Net against the oracle in double
carrying the same masks, merge_and_unload against the un-merged eval forward, and `unlearn.py --method lora` on the HIP backend.

Shapes: M in {1, 63, 64, 65, 1000} (one 16-row block, a ragged one, exactly two, a third begun, many workgroups), 5000 (the
backward's row slabs are two blocks long) and 262 144 + 65 (past the forward's default grid: a second trip); C in {32, 96, 256}
and 30 (ragged: the scalar path); r in {4, 16, 20, 64} (a padded tile, one tile, two tiles, four tiles = more than one pass with
three projections); n_proj in {1, 3}; p in {0, 0.05, 0.5}.  Every raw launch runs with its operands, its outputs and its exactly
sized workspace between poisoned bands."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest
import torch

import lora_ref as LR

pytestmark = pytest.mark.gpu
dev = torch.device("cuda:0")
PAD, POISON = 4096, 0xA5
SEED = 20240531
U = 2.0 ** -24


@pytest.fixture(scope="module")
def lib():
    from gad import _capi
    return _capi.load()


def _stream():
    from gad import ops
    return ops._stream()


class Banded:
    """`nbytes` of device memory between two poisoned bands"""

    def __init__(self, nbytes):
        self.buf = torch.full((PAD + nbytes + PAD,), POISON, dtype=torch.uint8, device=dev)
        self.nbytes = nbytes
        self.ptr = self.buf.data_ptr() + PAD
        assert self.ptr % 16 == 0

    def f32(self):
        return self.buf[PAD:PAD + self.nbytes].view(torch.float32)

    def intact(self):
        return bool((self.buf[:PAD] == POISON).all()) and bool((self.buf[PAD + self.nbytes:] == POISON).all())


def banded(a):
    b = Banded(a.size * 4)
    b.f32().copy_(torch.from_numpy(np.array(a)).reshape(-1))
    return b


@functools.lru_cache(maxsize=None)
def operands(M, C, r, n_proj):
    """seeded fp32 (x, [A_j], [dmid_j], dx0) on the host; computed once per shape and never written"""
    rng = np.random.default_rng(M * 131 + C * 17 + r * 3 + n_proj)
    x = rng.standard_normal((M, C)).astype(np.float32)
    As = tuple((rng.standard_normal((r, C)) / np.sqrt(C)).astype(np.float32) for _ in range(n_proj))
    dm = tuple(rng.standard_normal((M, r)).astype(np.float32) for _ in range(n_proj))
    dx0 = rng.standard_normal((M, C)).astype(np.float32)
    for a in (x, dx0) + As + dm:
        a.setflags(write=False)
    return x, As, dm, dx0


def make_args(M, C, r, n_proj, p, scale, offset, layer, max_blocks=0):
    from gad import _capi
    a = _capi.LoraDropoutArgs()
    a.ldx, a.M, a.C, a.r, a.n_proj, a.layer, a.ld_dx = C, M, C, r, n_proj, layer, C
    a.p, a.scale, a.seed, a.offset, a.max_blocks = p, scale, SEED, offset, max_blocks
    return a


def run_fwd(lib, M, C, r, n_proj, p, scale=2.0, offset=7, layer=3, max_blocks=0):
    x, As, _, _ = operands(M, C, r, n_proj)
    a = make_args(M, C, r, n_proj, p, scale, offset, layer, max_blocks)
    bx, bA, bm = banded(x), [banded(A) for A in As], [Banded(M * r * 4) for _ in As]
    need = lib.gad_lora_down_dropout_workspace_bytes(ctypes.byref(a))
    assert need >= 0, lib.gad_last_error()
    ws = Banded(need)
    a.x, a.workspace, a.workspace_bytes = bx.ptr, ws.ptr, need
    for j in range(n_proj):
        a.A[j], a.mid[j] = bA[j].ptr, bm[j].ptr
    assert lib.gad_lora_down_dropout_fwd(ctypes.byref(a), _stream()) == 0, lib.gad_last_error()
    out = [b.f32().cpu().numpy().reshape(M, r) for b in bm]
    assert all(b.intact() for b in [bx, ws] + bA + bm)
    assert np.array_equal(bx.f32().cpu().numpy().reshape(M, C), x)
    return out, (bx, bA)


FWD = [(1, 32, 4, 1, 0.05), (63, 96, 16, 3, 0.5), (64, 256, 16, 3, 0.05), (65, 30, 20, 1, 0.5), (1000, 256, 64, 3, 0.05),
       (1000, 30, 4, 3, 0.05), (65, 96, 64, 1, 0.05), (1000, 32, 20, 3, 0.5), (64, 96, 4, 3, 0.5), (262144 + 65, 32, 4, 1, 0.05)]


# ---- 1: forward ----
@pytest.mark.parametrize("M,C,r,n_proj,p", FWD)
def test_down_dropout_forward_against_fp64(lib, M, C, r, n_proj, p):
    """|mid - mid_64| <= 2 (C + 2) 2^-24 * s / (1 - p) * sum_c |x m a| per element: the fp32 summation bound of a C-term fmaf chain
    with the roundings of x / (1 - p) and of the scale on top.  One wrong mask bit moves an element by a whole term."""
    s = 2.0
    x, As, _, _ = operands(M, C, r, n_proj)
    got, _ = run_fwd(lib, M, C, r, n_proj, p, scale=s)
    want, mag = LR.down_fwd(x, As, s, p, SEED, 7, 3)
    for j in range(n_proj):
        bound = 2 * (C + 2) * U * s / (1 - p) * mag[j]
        err = np.abs(got[j] - want[j])
        worst = float(np.max(err / np.maximum(bound, 1e-300)))
        print(f"M={M} C={C} r={r} n_proj={n_proj} p={p} j={j}: max err / bound = {worst:.3f}, max |mid| = {np.abs(want[j]).max():.3f}")
        assert np.all(err <= bound)
    # a mask of the wrong stream fails the bound by orders of magnitude
    if p > 0 and M >= 63:
        other, _ = LR.down_fwd(x, As[:1], s, p, SEED, 8, 3)
        assert np.max(np.abs(got[0] - other[0]) / np.maximum(2 * (C + 2) * U * s / (1 - p) * mag[0], 1e-300)) > 100


@pytest.mark.parametrize("M,C,r,n_proj", [(300, 32, 16, 3), (1000, 256, 64, 3), (700, 30, 20, 1)])
def test_forward_does_not_depend_on_the_grid(lib, M, C, r, n_proj):
    """one workgroup walking the rows in several trips, two, and the default grid give equal bits"""
    a, _ = run_fwd(lib, M, C, r, n_proj, 0.05)
    for cap in (1, 2):
        b, _ = run_fwd(lib, M, C, r, n_proj, 0.05, max_blocks=cap)
        assert all(u.tobytes() == v.tobytes() for u, v in zip(a, b))


@pytest.mark.parametrize("M,C,r,n_proj", [(1, 32, 4, 1), (63, 96, 16, 3), (65, 30, 4, 3), (1000, 256, 20, 1), (1000, 256, 64, 3)])
def test_forward_without_dropout_is_the_plain_down_projection(lib, M, C, r, n_proj):
    """p = 0: bit-equal to gemm_raw with alpha = s (and inside the fp64 bound)"""
    from gad import ops
    from gad._capi import A_KC, B_KC
    s = 2.0
    x, As, _, _ = operands(M, C, r, n_proj)
    got, (bx, bA) = run_fwd(lib, M, C, r, n_proj, 0.0, scale=s)
    want, mag = LR.down_fwd(x, As, s, 0.0, SEED, 7, 3)
    for j in range(n_proj):
        mid = torch.empty((M, r), device=dev)
        ops.gemm_raw(bx.f32().view(M, C), bA[j].f32().view(r, C), mid, A_KC, B_KC, M, r, C, C, C, r, alpha=s)
        assert mid.cpu().numpy().tobytes() == got[j].tobytes(), j
        assert np.all(np.abs(got[j] - want[j]) <= 2 * (C + 2) * U * s * mag[j])


# ---- 2: backward ----
def run_bwd(lib, M, C, r, n_proj, p, offset=7, layer=3):
    x, As, dm, dx0 = operands(M, C, r, n_proj)
    a = make_args(M, C, r, n_proj, p, 1.0, offset, layer)
    bx, bdx, bA, bdm = banded(x), banded(dx0), [banded(A) for A in As], [banded(d) for d in dm]
    bdA = [Banded(r * C * 4) for _ in As]
    need = lib.gad_lora_down_dropout_workspace_bytes(ctypes.byref(a))
    ws = Banded(need)
    a.x, a.dx, a.workspace, a.workspace_bytes = bx.ptr, bdx.ptr, ws.ptr, need
    for j in range(n_proj):
        a.A[j], a.dmid[j], a.dA[j] = bA[j].ptr, bdm[j].ptr, bdA[j].ptr
    assert lib.gad_lora_down_dropout_bwd(ctypes.byref(a), _stream()) == 0, lib.gad_last_error()
    dAs = [b.f32().cpu().numpy().reshape(r, C) for b in bdA]
    dx = bdx.f32().cpu().numpy().reshape(M, C)
    assert all(b.intact() for b in [bx, bdx, ws] + bA + bdm + bdA)
    assert np.array_equal(bx.f32().cpu().numpy().reshape(M, C), x)
    return dAs, dx


BWD = [(1, 32, 4, 1, 0.05), (63, 96, 16, 3, 0.5), (64, 256, 16, 3, 0.05), (65, 30, 20, 1, 0.5), (1000, 256, 64, 3, 0.05),
       (1000, 30, 4, 3, 0.05), (5000, 96, 16, 3, 0.05), (1000, 256, 16, 3, 0.0), (65, 30, 4, 3, 0.0), (1000, 320, 20, 3, 0.5)]


@pytest.mark.parametrize("M,C,r,n_proj,p", BWD)
def test_down_dropout_backward_against_fp64(lib, M, C, r, n_proj, p):
    """dA: the forward's form of bound with M terms, 2 (M + 2) 2^-24 / (1 - p) * sum_m |dmid x m|.  dx: n_proj r product terms
    and the incoming gradient as one more term of the same sum, 2 (n_proj r + 2) 2^-24 (|dx0| + sum_j sum_r |dmid a| m / (1 - p)).
    dx0 is non-zero and really accumulated onto; a second launch gives equal bits."""
    x, As, dm, dx0 = operands(M, C, r, n_proj)
    dAs, dx = run_bwd(lib, M, C, r, n_proj, p)
    wA, wx, magA, magx = LR.down_bwd(x, As, dm, dx0, p, SEED, 7, 3)
    for j in range(n_proj):
        bound = 2 * (M + 2) * U / (1 - p) * magA[j]
        err = np.abs(dAs[j] - wA[j])
        print(f"M={M} C={C} r={r} n_proj={n_proj} p={p} dA{j}: max err / bound = {float(np.max(err / np.maximum(bound, 1e-300))):.3f}")
        assert np.all(err <= bound)
    bound = 2 * (n_proj * r + 2) * U * (np.abs(dx0) + magx / (1 - p))
    err = np.abs(dx - wx)
    print(f"M={M} C={C} r={r} n_proj={n_proj} p={p} dx: max err / bound = {float(np.max(err / np.maximum(bound, 1e-300))):.3f}, "
          f"|dx - dx0| max = {np.abs(wx - dx0).max():.3f}")
    assert np.all(err <= bound)
    assert np.abs(wx - dx0).max() > 0.1 and np.abs(dx - (wx - dx0)).max() > 0.1        # neither the sum's part alone
    dAs2, dx2 = run_bwd(lib, M, C, r, n_proj, p)
    assert dx2.tobytes() == dx.tobytes() and all(u.tobytes() == v.tobytes() for u, v in zip(dAs, dAs2))


# ---- 3: merge ----
def test_merge_against_fp64_and_unmerge(lib):
    """W += alpha B A within 2 (r + 2) 2^-24 (|W| + |alpha| sum_r |b a|) (an r-term fmaf chain, the scale and the add); merging and
    unmerging returns W to within 2 ulp (2 * 2^-23) of the magnitudes that met in the two adds, |W| + |alpha| sum_r |b a|."""
    rng = np.random.default_rng(5)
    N, K, ldw, r, alpha = 70, 50, 52, 8, 4.0
    W = rng.standard_normal((N, ldw)).astype(np.float32)
    B, A = rng.standard_normal((N, r)).astype(np.float32), (rng.standard_normal((r, K)) / 8).astype(np.float32)
    bW, bB, bA = banded(W), banded(B), banded(A)
    assert lib.gad_lora_merge(bW.ptr, ldw, bB.ptr, bA.ptr, N, K, r, alpha, _stream()) == 0, lib.gad_last_error()
    got = bW.f32().cpu().numpy().reshape(N, ldw)
    d64, mag = alpha * (B.astype(np.float64) @ A.astype(np.float64)), abs(alpha) * (np.abs(B).astype(np.float64) @ np.abs(A))
    scale = np.abs(W[:, :K]) + mag
    err = np.abs(got[:, :K] - (W[:, :K] + d64))
    print(f"merge: max err / bound = {float(np.max(err / (2 * (r + 2) * U * scale))):.3f}")
    assert np.all(err <= 2 * (r + 2) * U * scale) and np.array_equal(got[:, K:], W[:, K:])      # the row padding is not touched
    assert np.abs(d64).max() > 1.0
    assert lib.gad_lora_merge(bW.ptr, ldw, bB.ptr, bA.ptr, N, K, r, -alpha, _stream()) == 0, lib.gad_last_error()
    back = bW.f32().cpu().numpy().reshape(N, ldw)
    assert np.all(np.abs(back[:, :K] - W[:, :K]) <= 2 * 2.0 ** -23 * scale)
    assert all(b.intact() for b in (bW, bB, bA))


# ---- 4: one LoRA step and two LoRA+ optimizer steps on the TINY U-Net ----
TINY = dict(block_out_channels=[32, 32, 64, 64], norm_num_groups=8)
R_, ALPHA, P_DROP, LR_ = 16, 32, 0.05, 1e-4


def tiny_pair():
    import gad
    from oracle import diffusers_ref as R
    from src.ddpm_config import DDPMConfig
    ucfg = dict(DDPMConfig.cifar100_config["unet_config"], **TINY)
    scfg = DDPMConfig.cifar100_config["scheduler_config"]
    torch.manual_seed(0)
    ref = R.UNet2DModel(**ucfg)
    net = gad.UNet2DModel(**ucfg)
    net.load_state_dict(ref.state_dict())
    net.to(dev)
    ref.double()
    torch.manual_seed(5)
    gad.get_peft_model(net, gad.LoraConfig(r=R_, lora_alpha=ALPHA, lora_dropout=P_DROP, target_modules=["to_q", "to_v", "to_k"]))
    torch.manual_seed(5)
    LR.get_peft_model(ref, R_, ALPHA, P_DROP, torch.initial_seed() & 0xFFFFFFFF)
    g = torch.Generator().manual_seed(9)
    with torch.no_grad():                                            # B = 0 would make every dA zero: the same small B on both sides
        for m, ls in zip(gad.lora.lora_layers(net), LR.lora_layers(ref)):
            for (_, a, b), l in zip(m.lora_qkv.matrices(), ls):
                assert torch.equal(a.detach().cpu().double(), l.A.detach())
                v = 0.02 * torch.randn(b.shape, generator=g)
                b.copy_(v.to(dev))
                l.B.copy_(v.double())
    return net, ref, gad.DDPMScheduler(**scfg), R.DDPMScheduler(**scfg)


def ref_grads(ref, sch_r, x, e, t, offset):
    LR.set_offset(ref, offset)
    ref.train()
    for p in ref.parameters():
        p.grad = None
    out = ref(sch_r.add_noise(x.double(), e.double(), t), t).sample
    torch.nn.functional.mse_loss(out, e.double()).backward()
    layers = [l for ls in LR.lora_layers(ref) for l in ls]
    assert all(p.grad is None for p in ref.parameters() if not p.requires_grad)
    return out.detach(), [l.A.grad.numpy().copy() for l in layers], [l.B.grad.numpy().copy() for l in layers]


def test_lora_step_against_the_oracle_in_double():
    """Train-mode output within 1e-4 and every dA / dB within 2e-3 relative per tensor of the oracle in double with the same masks (the
    project's bounds, as in test_influence_unlearner_against_the_oracle_in_double); no base parameter has a gradient or moves.  Then
    two LoRA+ steps against fp64 Adam at lr (A) and 16 lr (B): per tensor |moved_gpu - moved_64| <= 5 % of |moved_64|.  Adam's first
    updates are lr * g / (|g| + eps): an element moves by about its learning rate whatever the gradient's scale, so a gradient error
    matters only where it flips a sign, |g_i| below the error - a share f of the elements, costing 2 sqrt(f) of the norm; with fp32
    gradients good to 2e-3 per tensor (1e-5 typically) f stays below 6e-4, while a wrong multiplier or clip norm is off by
    a factor."""
    import gad
    net, ref, sch, sch_r = tiny_pair()
    g = torch.Generator().manual_seed(11)
    x, e = torch.rand(4, 3, 32, 32, generator=g) * 2 - 1, torch.randn(4, 3, 32, 32, generator=g)
    t = torch.tensor([11, 977, 500, 3])
    xd, ed, td = x.to(dev), e.to(dev), t.to(dev)
    base = {n: p.detach().clone() for n, p in net.named_parameters() if "lora_qkv" not in n}
    params, groups = gad.lora_parameters(net, 16)
    trainer = gad.FusedTrainer(net, sch, None, lr=LR_, max_grad_norm=1.0, params=params, groups=groups)
    n = len(params) // 2
    net.train()
    with torch.no_grad():
        out = net(sch.add_noise(xd, ed, td), td).sample.cpu()        # this block's first training forward: offset 1
    want, _, _ = ref_grads(ref, sch_r, x, e, t, 1)
    err = float((out.double() - want).abs().max())
    LR.set_offset(ref, 0)
    ref.eval()
    with torch.no_grad():
        moved = float((ref(sch_r.add_noise(x.double(), e.double(), t), t).sample - want).abs().max())
    print(f"train-mode output: max |gpu - oracle| = {err:.3e}; dropout moves the output by {moved:.3e}")
    assert err <= 1e-4 and moved > 10 * err

    trainer._forward_backward(xd, ed, td, (), None)                  # offset 2
    _, gA, gB = ref_grads(ref, sch_r, x, e, t, 2)
    worst = 0.0
    for p, gr in zip(params, gA + gB):
        gg = p._gad_sink.detach().cpu().double().numpy()
        rel = float(np.linalg.norm(gg - gr) / max(np.linalg.norm(gr), 1e-30))
        worst = max(worst, rel)
        assert rel < 2e-3, rel
    print(f"worst per-tensor relative LoRA gradient error: {worst:.3e}")
    for name, p in net.named_parameters():
        if "lora_qkv" not in name:
            assert p.grad is None and not p.requires_grad and torch.equal(p.detach(), base[name]), name

    layers = [l for ls in LR.lora_layers(ref) for l in ls]
    start = [p.detach().cpu().double().numpy().copy() for p in params]
    adam = LR.LoraPlusAdam([l.A.detach().numpy() for l in layers], [l.B.detach().numpy() for l in layers], LR_, 16.0)
    norm64 = adam.step(gA + gB)
    trainer.optimizer_step()
    assert abs(float(trainer.grad_norm()) - norm64) <= 2e-3 * norm64
    with torch.no_grad():
        for l, a, b in zip(layers, adam.p[:n], adam.p[n:]):
            l.A.copy_(torch.from_numpy(a))
            l.B.copy_(torch.from_numpy(b))
    trainer.step(xd, ed, td)                                         # offset 3, through the refreshed weights
    _, gA, gB = ref_grads(ref, sch_r, x, e, t, 3)
    adam.step(gA + gB)
    worst = 0.0
    for i, (p, s0, p64) in enumerate(zip(params, start, adam.p)):
        got, want_d = p.detach().cpu().double().numpy() - s0, p64 - s0
        rel = float(np.linalg.norm(got - want_d) / np.linalg.norm(want_d))
        worst = max(worst, rel)
        assert rel <= 0.05, (i, rel)
        rate = LR_ * (1.0 if i < n else 16.0)
        assert 0.5 * rate <= np.abs(want_d).mean() <= 2.0 * rate      # two steps of about one learning rate each
    print(f"two LoRA+ steps: worst per-tensor |moved - moved_64| / |moved_64| = {worst:.3e}")
    for name, p in net.named_parameters():
        if "lora_qkv" not in name:
            assert torch.equal(p.detach(), base[name]), name


# ---- 5: merge and sampling ----
def test_merge_and_unload_matches_the_unmerged_eval_forward():
    """After merge_and_unload a no-grad forward (the fused no-LoRA sampling route) equals the un-merged eval forward within the
    output tolerance, 1e-4; after putting the layers back, rewriting a B matrix in place and merging again it matches the new
    un-merged forward - which fused [3C, C] projections or other derived weights left over from the first merge would fail."""
    import gad
    net, _, sch, _ = tiny_pair()
    g = torch.Generator().manual_seed(13)
    x = torch.randn(4, 3, 32, 32, generator=g).to(dev)
    t = torch.tensor([11, 977, 500, 3]).to(dev)
    plain = {n: p.detach().clone() for n, p in net.named_parameters() if "lora_qkv" not in n}
    net.eval()
    kept = [(m, m.lora_qkv) for m in gad.lora.lora_layers(net)]
    with torch.no_grad():
        y0 = net(x, t).sample.clone()
    assert gad.merge_and_unload(net) is net and not gad.lora.lora_layers(net)
    assert [n for n, _ in net.named_parameters()] == list(plain)
    with torch.no_grad():
        y1 = net(x, t).sample.clone()
    changed = [n for n, p in net.named_parameters() if not torch.equal(p.detach(), plain[n])]
    assert changed and all(n.split(".")[-2] in ("to_q", "to_k", "to_v") and n.endswith("weight") for n in changed)
    e1 = float((y1 - y0).abs().max())
    for m, lq in kept:                                               # the layers back on, one matrix rewritten in place
        m.lora_qkv = lq
        with torch.no_grad():
            lq.to_q_B.mul_(-40.0)
            lq.to_v_B.data.mul_(25.0)
    with torch.no_grad():
        y2 = net(x, t).sample.clone()
    gad.merge_and_unload(net)
    with torch.no_grad():
        y3 = net(x, t).sample.clone()
    e3, moved = float((y3 - y2).abs().max()), float((y2 - y1).abs().max())
    print(f"merged vs un-merged eval forward: {e1:.3e}; after the rewrite {e3:.3e} (the rewrite moved the output by {moved:.3e})")
    assert e1 <= 1e-4 and e3 <= 1e-4 and moved > 1e-3


# ---- 6: the entry point ----
def test_lora_entry_point_on_the_hip_backend(tmp_path, monkeypatch):
    """train 3 steps on toy2, then `--method lora --gd_steps 3`: one row with the method's fields, the EMA's step counter advanced by
    gd_steps, shadows equal to the merged weights, and no LoRA layer left on the sampled model."""
    import gad
    from src.ddpm_config import DDPMConfig
    cfg = {**DDPMConfig.cifar100_config}
    cfg["unet_config"] = dict(cfg["unet_config"], **TINY)
    cfg["n_samples"] = 4
    cfg["batch_size"] = 16
    for k in ("training_steps", "ckpt_freq", "sample_freq"):
        cfg[k] = dict(cfg[k], retrain=3)
    monkeypatch.setattr(DDPMConfig, "cifar100_config", cfg)
    from unconditional_generation import main as train_main
    from unconditional_generation import unlearn as unlearn_main
    out, db = str(tmp_path / "res"), str(tmp_path / "db.jsonl")
    assert train_main.main(train_main.parse_args(["--dataset", "toy2", "--method", "retrain", "--outdir", out, "--batch_size", "16",
                                                  "--num_inference_steps", "10", "--log_freq", "1"]))
    mdir = os.path.join(out, "toy2", "retrain", "models", "full")
    ck = torch.load(os.path.join(mdir, "ckpt_steps_00000003.pt"), weights_only=False)
    pdir = os.path.join(out, "toy2", "pruned", "models", "pruner=magnitude_pruning_ratio=0.3_threshold=0.05")
    os.makedirs(pdir)
    torch.save({"unet": ck["unet"], "unet_config": ck["unet_config"]}, os.path.join(pdir, "ckpt_steps_00000000.pt"))
    before = ck["unet_ema"]["optimization_step"]
    kept = {}
    store = gad.EMAModel.store

    def recording_store(self, parameters):
        parameters = list(parameters)
        kept["step"] = self.optimization_step
        kept["pairs"] = [(p.detach().clone(), s.detach().clone()) for p, s in zip(parameters, self.shadow_params)]
        kept["n_shadows"] = len(self.shadow_params)
        store(self, parameters)
    monkeypatch.setattr(gad.EMAModel, "store", recording_store)
    argv = ["--dataset", "toy2", "--method", "lora", "--removal_dist", "shapley", "--removal_seed", "1", "--load", mdir, "--outdir", out,
            "--db", db, "--gd_steps", "3", "--lora_rank", "8", "--n_samples", "16", "--batch_size", "8", "--num_inference_steps", "10",
            "--model_behavior", "global"]
    assert unlearn_main.main(unlearn_main.parse_args(argv))
    rows = open(db).readlines()
    assert len(rows) == 1
    row = json.loads(rows[0])
    assert row["method"] == "lora" and row["lora_rank"] == 8 and row["lora_dropout"] == 0.05 and row["gd_steps"] == 3
    assert row["trained_steps"] == 3 and np.isfinite(row["fid_value"]) and row["total_steps_time"] > 0
    names = [n for n, _ in gad.UNet2DModel(**ck["unet_config"]).named_parameters()]
    assert kept["step"] == before + 3 and len(kept["pairs"]) == kept["n_shadows"] == len(names)
    assert all(torch.equal(p, s) for p, s in kept["pairs"])
    moved = [k for k, (p, _) in zip(names, kept["pairs"]) if not torch.equal(ck["unet"][k].to(p.device), p)]
    assert moved and all(k.split(".")[-2] in ("to_q", "to_k", "to_v") and k.endswith("weight") for k in moved)
    assert os.path.exists(os.path.join(out, "toy2", "lora", "samples", "shapley", "shapley_seed=1", "prutirb_ratio_0.5_steps_00000003.png"))
