"""8-bit blockwise Adam on the GPU (csrc/optim8.hip): the fused clip + Adam8bit + EMA launch against the fp64 restatement
(tests/adam8_ref.py), teacher-forced - every reference step starts from the state the device holds - then FusedTrainer(optim_bits=8)
on a small U-Net and on the SD LoRA parameters, and resuming from a state dict.

Tolerances: p and the EMA rtol 1e-6 / atol 1e-6 (those of test_fused_clip_adam_ema_matches_torch); absmax rtol 1e-6; codes equal
except that at most 0.1 % may differ by exactly one level - a cap the restatement keeps against itself between fp32 and fp64
(tests/test_adam8_cpu.py::test_fp32_restatement_keeps_the_cap_against_fp64 measures 0 differing codes on the same inputs)."""
import pytest
import torch

import adam8_ref as R

pytestmark = pytest.mark.gpu
dev = torch.device("cuda:0")
PAD, POISON = 4096, 0x5A
KEYS = ("p", "ema", "state1", "state2", "absmax1", "absmax2", "m32", "v32")


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


class Guarded:
    """device buffers between poisoned bands"""

    def __init__(self):
        self.regions = []

    def put(self, name, cpu):
        nbytes = cpu.numel() * cpu.element_size()
        buf = torch.full((nbytes + 2 * PAD,), POISON, dtype=torch.uint8, device=dev)
        view = buf[PAD:PAD + nbytes].view(cpu.dtype)
        view.copy_(cpu)
        self.regions.append((name, buf, nbytes))
        return view

    def check(self):
        for name, buf, nbytes in self.regions:
            assert (buf[:PAD] == POISON).all() and (buf[PAD + nbytes:] == POISON).all(), f"{name}: wrote outside the buffer"


def _cpu(bufs):
    return {k: (None if bufs.get(k) is None else bufs[k].detach().cpu().clone()) for k in KEYS}


def _launch(ops, bufs, g, blocks, hp, step):
    ss = ops.sumsq_raw(g)
    ops.clip_adam8_ema_raw(bufs["p"], g, bufs["ema"], bufs["state1"], bufs["state2"], bufs["absmax1"], bufs["absmax2"], bufs["m32"],
                           bufs["v32"], blocks, ss, max_norm=hp["max_norm"], lr=hp["lr"], betas=hp["betas"], eps=hp["eps"], step=step,
                           ema_decay=hp["ema_decay"])
    return float(ss.item())


def _compare(got, want, what, atol_p=1e-6):
    """device state `got` (CPU copies) against the fp64 restatement `want`"""
    for k in ("p", "ema"):
        if want[k] is not None:
            err = (got[k].double() - want[k]).abs()
            print(f"{what} {k}: largest error {float(err.max()):.3e}")
            assert torch.allclose(got[k].double(), want[k], rtol=1e-6, atol=atol_p), (what, k, float(err.max()))
    for k in ("absmax1", "absmax2"):
        rel = ((got[k].double() - want[k]).abs() / want[k].abs().clamp_min(1e-300)).max() if want[k].numel() else 0.0
        print(f"{what} {k}: largest relative error {float(rel):.3e}")
        assert torch.allclose(got[k].double(), want[k], rtol=1e-6, atol=0.0), (what, k)
    for k in ("m32", "v32"):     # a moment's error is a few ulps of the larger of beta*m and (1-beta)*g, which may cancel: absolute
        assert torch.allclose(got[k].double(), want[k], rtol=1e-6, atol=1e-6 * float(want[k].abs().max())), (what, k)
    for k in ("state1", "state2"):
        R.codes_agree(got[k], want[k], f"{what} {k}")
    for k in KEYS:
        if got[k] is not None and got[k].is_floating_point():
            assert torch.isfinite(got[k]).all(), (what, k)


@pytest.fixture(scope="module")
def kernel_run():
    """six teacher-forced steps of the launch on adam8_ref.make_case(), every buffer between poisoned bands"""
    from gad import ops
    from gad.training import SLOT, adam8_blocks
    sizes, p0, grads = R.make_case()
    hp = dict(R.CASE_HP)
    lay = adam8_blocks([torch.empty(n) for n in sizes], hp.pop("weight_decay"), no_decay=R.CASE_NO_DECAY)
    st = R.case_state(lay, sizes, p0)
    n = st["p"].numel()
    # sentinels where nothing may ever be written: the padding of every slot, the code bytes under fp32-state parameters
    for small, off, cnt, _, _ in lay.params:
        pad = slice(off + cnt, off + (cnt + SLOT - 1) // SLOT * SLOT)
        st["p"][pad], st["ema"][pad] = 7.0, -7.0
        st["state1"][pad], st["state2"][pad] = 0xAB, 0xAB
        if small:
            st["state1"][off:off + cnt], st["state2"][off:off + cnt] = 0xCD, 0xCD
    guard = Guarded()
    bufs = {k: guard.put(k, st[k]) for k in KEYS}
    blocks = guard.put("blocks", torch.from_numpy(lay.table.view("u1").copy()))
    steps = []
    for t, gs in enumerate(grads, 1):
        g = guard.put(f"g{t}", R.flat_grad(lay, n, gs))
        before = _cpu(bufs)
        ss = _launch(ops, bufs, g, blocks, hp, t)
        torch.cuda.synchronize()
        want = R.adam8_step(before, g.cpu(), lay.table, sumsq=ss, step=t, dtype=torch.float64, **hp)
        steps.append(dict(before=before, after=_cpu(bufs), want=want, sumsq=ss, g=g))
    return dict(lay=lay, hp=hp, steps=steps, guard=guard, bufs=bufs, blocks=blocks, sizes=sizes, SLOT=SLOT)


def test_kernel_matches_the_fp64_restatement(kernel_run):
    lay, steps = kernel_run["lay"], kernel_run["steps"]
    clipped = [s["sumsq"] > 1.0 for s in steps]
    assert any(clipped) and not all(clipped)                                  # the clip is active on some steps and idle on others
    saw126 = saw_underflow = False
    for t, s in enumerate(steps, 1):
        _compare(s["after"], s["want"], f"step {t}")
        got = s["after"]
        (_, off5, n5, first5, nb5), (_, off6, n6, _, _) = lay.params[5], lay.params[6]
        # the tensor that never gets a gradient: absmax 0, zero codes, untouched parameter
        assert (got["state1"][off5:off5 + n5] == 127).all() and (got["state2"][off5:off5 + n5] == 0).all()
        assert (got["absmax1"][first5:first5 + nb5] == 0).all() and (got["absmax2"][first5:first5 + nb5] == 0).all()
        assert torch.equal(got["p"][off5:off5 + n5] , s["before"]["p"][off5:off5 + n5] * (1 - torch.tensor(1e-2) * torch.tensor(1e-6)))
        saw126 |= bool((got["state1"][lay.params[2][1]:lay.params[2][1] + 4096] == 126).any())
        saw_underflow |= bool(((got["state2"][off6:off6 + n6] == 0) & (s["g"].cpu()[off6:off6 + n6] != 0)).any())
    assert saw126 and saw_underflow      # negative moments at code 126; second moments that underflow to code 0 inside a block


def test_guard_bands(kernel_run):
    """SLOT padding of p, ema and both code buffers, the code bytes under fp32-state parameters and the bands around every buffer"""
    kernel_run["guard"].check()
    lay, SLOT = kernel_run["lay"], kernel_run["SLOT"]
    got = kernel_run["steps"][-1]["after"]
    pads = 0
    for small, off, cnt, _, _ in lay.params:
        pad = slice(off + cnt, off + (cnt + SLOT - 1) // SLOT * SLOT)
        pads += pad.stop - pad.start
        assert (got["p"][pad] == 7.0).all() and (got["ema"][pad] == -7.0).all()
        assert (got["state1"][pad] == 0xAB).all() and (got["state2"][pad] == 0xAB).all()
        if small:
            assert (got["state1"][off:off + cnt] == 0xCD).all() and (got["state2"][off:off + cnt] == 0xCD).all()
    assert pads == 1 + 7 + 7
    assert torch.equal(kernel_run["blocks"].cpu(), torch.from_numpy(lay.table.view("u1").copy()))


def test_bit_reproducible(kernel_run):
    from gad import ops
    s = kernel_run["steps"][3]
    outs = []
    for _ in range(2):
        bufs = {k: s["before"][k].to(dev) for k in KEYS}
        _launch(ops, bufs, s["g"], kernel_run["blocks"], kernel_run["hp"], 4)
        outs.append(_cpu(bufs))
    for k in KEYS:
        assert torch.equal(outs[0][k], outs[1][k]), k
        assert torch.equal(outs[0][k], s["after"][k]), k


# ---- FusedTrainer ------------------------------------------------------------------------------------------------------
def _trainer_state(tr):
    return {"p": tr.flat.detach().cpu().clone(), "ema": None if tr.ema_flat is None else tr.ema_flat.detach().cpu().clone(),
            **{k: v.detach().cpu().clone() for k, v in tr.state8.items()}}


def _replay(tr, before, step, ema_decay):
    """the restatement of the optimizer step the trainer has just taken, from its captured gradient and clip scalar"""
    hp = tr.hp
    return R.adam8_step(before, tr.gflat.detach().cpu(), tr.adam8.table, sumsq=float(tr._sumsq.item()), max_norm=tr.max_grad_norm,
                        lr=hp["lr"], betas=hp["betas"], eps=hp["eps"], step=step, ema_decay=ema_decay, dtype=torch.float64)


# the smallest U-Net of the registry's topology that still has every kind of parameter: 3x3 convs and attention projections of at
# least 4096 elements (uint8 state, many blocks, short last blocks), biases, norms and conv_in / conv_out below it (fp32 state)
UNET_SHRINK = dict(block_out_channels=[32, 64, 64, 64], norm_num_groups=8)


def _unet_trainer(optim_bits, **kw):
    import gad
    from src.ddpm_config import DDPMConfig
    cfg = dict(DDPMConfig.cifar100_config["unet_config"], **UNET_SHRINK)
    torch.manual_seed(0)
    net = gad.UNet2DModel(**cfg).to(dev)
    ema = gad.EMAModel(net.parameters())
    ema.optimization_step = 5000
    sch = gad.DDPMScheduler(**DDPMConfig.cifar100_config["scheduler_config"])
    extra = dict(optim_bits=8, no_decay=["bias" in n for n, _ in net.named_parameters()]) if optim_bits == 8 else {}
    return gad.FusedTrainer(net, sch, ema, lr=1e-3, weight_decay=1e-2, max_grad_norm=1.0, **extra, **kw)


def _batch(i):
    return rnd(4, 3, 32, 32, seed=10 + i).to(dev), rnd(4, 3, 32, 32, seed=20 + i).to(dev), torch.tensor([3, 400, 720, 990]).to(dev)


def test_trainer_on_a_small_unet_and_resume():
    def fp32_run():
        tr = _unet_trainer(32)
        for i in range(2):
            tr.step(*_batch(i))
        return tr
    first = fp32_run()
    tr = _unet_trainer(8)
    assert tr.m is None and tr.state8["state1"].dtype == torch.uint8
    kinds = [small for small, *_ in tr.adam8.params]
    tab = tr.adam8.table
    assert any(kinds) and not all(kinds) and ((tab["len"] < 2048) & (tab["fp32"] == 0)).any()      # short last blocks
    sd2 = None
    for i in range(3):
        before = _trainer_state(tr)
        tr.step(*_batch(i))
        want = _replay(tr, before, i + 1, tr.ema.cur_decay_value)
        _compare(_trainer_state(tr), want, f"U-Net step {i + 1}")
        if i == 1:
            sd2 = tr.state_dict()
            weights2 = {k: v.detach().clone() for k, v in tr.model.state_dict().items()}
            ema2 = tr.ema.state_dict()
    assert int((tr.state8["state1"] != 127).sum()) > 0.5 * tr.flat.numel()
    # the fp32 trainer of the same process is what it was: same moments, same weights, bit for bit, before and after the 8-bit one
    again = fp32_run()
    assert again.optim_bits == 32 and not hasattr(again, "state8") and "exp_avg" in again.state_dict()["state"][0]
    assert torch.equal(first.flat, again.flat) and torch.equal(first.m, again.m) and torch.equal(first.v, again.v)
    assert all(torch.equal(a, b) for a, b in zip(first.ema.shadow_params, again.ema.shadow_params))
    # resume: state_dict after step 2 -> fresh trainer -> step 3 is the uninterrupted run's, bit for bit
    st = sd2["state"]
    big = next(i for i, (small, *_) in enumerate(tr.adam8.params) if not small)
    tiny = next(i for i, (small, *_) in enumerate(tr.adam8.params) if small)
    assert set(st[big]) == {"state1", "state2", "absmax1", "absmax2", "qmap1", "qmap2", "step"} and st[big]["state1"].dtype == torch.uint8
    assert tuple(st[big]["state1"].shape) == tuple(tr.params[big].shape) and st[tiny]["state1"].dtype == torch.float32
    fresh = _unet_trainer(8)
    fresh.model.load_state_dict(weights2)
    fresh.ema.load_state_dict(ema2)
    fresh.load_state_dict(sd2)
    assert fresh.step_count == 2
    fresh.step(*_batch(2))
    assert torch.equal(fresh.flat, tr.flat)
    assert all(torch.equal(a, b) for a, b in zip(fresh.ema.shadow_params, tr.ema.shadow_params))
    for k in tr.state8:
        assert torch.equal(fresh.state8[k], tr.state8[k]), k
    with pytest.raises(ValueError, match="8-bit"):
        fresh.load_state_dict(first.state_dict())                             # fp32 Adam moments are not this trainer's state


def test_sd_lora_trainer_step():
    """One SD LoRA step under --use_8bit_adam semantics (params=, adamw=True, decay on every LoRA parameter): matrices of at
    least 4096 elements hold uint8 state, the smaller ones fp32 moments, and the step is the restatement's."""
    import gad
    from test_gpu_sd import SMALL
    sch = gad.DDPMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", num_train_timesteps=1000)
    torch.manual_seed(0)
    net = gad.UNet2DConditionModel(**SMALL).to(dev)
    lora = net.inject_lora(rank=32)
    with torch.no_grad():
        for n, p in net.named_parameters():
            if n.endswith("lora_layer.up.weight"):
                p.copy_(rnd(*p.shape, seed=len(n), scale=0.02).to(dev))
    tr = gad.FusedTrainer(net, sch, None, lr=3e-4, weight_decay=1e-2, adamw=True, max_grad_norm=1.0, params=lora, optim_bits=8)
    kinds = {p.numel(): small for p, (small, *_) in zip(tr.params, tr.adam8.params)}
    assert kinds[32 * 128] is False and kinds[32 * 64] is True and (tr.adam8.table["weight_decay"] > 0).all()
    before = _trainer_state(tr)
    try:
        gad.set_operand_precision("bf16")
        tr.step(rnd(2, 4, 16, 16, seed=1).to(dev), rnd(2, 4, 16, 16, seed=2).to(dev), torch.tensor([5, 800]).to(dev), rnd(2, 77, 96, seed=3).to(dev))
    finally:
        gad.set_operand_precision("no")
    want = _replay(tr, before, 1, 0.0)
    after = _trainer_state(tr)
    _compare(after, want, "SD LoRA step")
    for p, (small, off, n, first, nb) in zip(tr.params, tr.adam8.params):
        if not small:
            assert (after["absmax1"][first:first + nb] > 0).all() and (after["state2"][off:off + n] != 0).any()
    sd = tr.state_dict()["state"]
    assert {v["state1"].dtype for v in sd.values()} == {torch.uint8, torch.float32}
