"""gad/shadows.py without a GPU: the freshness rule of the derived weight copies, the per-parameter cache, the rotated
shadow as the home of further shadows, and that every place which writes weights behind torch's back says so.

What torch sees and what it does not, on a flat buffer `flat` with resident parameters p (training.flatten_params):
an in-place op on `flat.detach()` moves flat's version counter (a detached alias shares it), `p.copy_()` moves only p's,
and a write through `.data` - like a raw kernel's through the device pointer - moves none: that one must be announced."""
import contextlib
from types import SimpleNamespace

import pytest
import torch

from gad import half, ops, shadows
from gad.shadows import Shadow, cached, stamp, weight_key, written, written_everywhere
from gad.training import EMAModel, FusedTrainer, flatten_params


def conv_weight(seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(64, 64, 3, 3, generator=g).contiguous(memory_format=torch.channels_last)


@pytest.fixture
def home():
    """(flat buffer, [two 64x64x3x3 channels-last weights, one 8x16 matrix]) on the CPU"""
    ps = [torch.nn.Parameter(conv_weight(1)), torch.nn.Parameter(conv_weight(2)),
          torch.nn.Parameter(torch.randn(8, 16, generator=torch.Generator().manual_seed(3)))]
    flat, _ = flatten_params(ps)
    return flat, ps


def test_one_rule_decides_when_a_buffer_shadow_refreshes(home):
    flat, ps = home
    offs = [p._gad_flat[1] for p in ps]
    copy, calls = torch.zeros_like(flat), []

    def refresh(src):
        assert src is flat
        calls.append(1)
        copy.copy_(src.detach())
    s = Shadow((copy,), refresh)
    assert s.fresh_for(flat, offs[0], ps[0]) is s and len(calls) == 1 and torch.equal(copy, flat)
    for p, off in zip(ps, offs):                                     # every resident is fresh after the one refresh
        s.fresh_for(flat, off, p)
    assert len(calls) == 1
    # a write that no version counter sees, not announced: served stale - the epoch, not the data, is the signal
    before = flat.detach().clone()
    flat.data.mul_(1.5)
    s.fresh_for(flat, offs[0], ps[0])
    assert len(calls) == 1 and torch.equal(copy, before) and not torch.equal(copy, flat)
    written(flat)                                                    # ... announced: one refresh
    s.fresh_for(flat, offs[0], ps[0])
    s.fresh_for(flat, offs[1], ps[1])
    assert len(calls) == 2 and torch.equal(copy, flat)
    with torch.no_grad():                                            # an in-place op on flat.detach(): torch counts it for flat
        flat.detach().mul_(0.5)
    s.fresh_for(flat, offs[2], ps[2])
    s.fresh_for(flat, offs[2], ps[2])
    assert len(calls) == 3 and torch.equal(copy, flat)
    with torch.no_grad():                                            # through torch, one resident: only ITS version moves
        ps[1].copy_(ps[1] * 0.25)
    s.fresh_for(flat, offs[1], ps[1])
    assert len(calls) == 4 and torch.equal(copy, flat)
    s.fresh_for(flat, offs[0], ps[0])                                # the siblings were covered by that refresh
    s.fresh_for(flat, offs[2], ps[2])
    s.fresh_for(flat, offs[1], ps[1])
    assert len(calls) == 4
    written_everywhere()
    s.fresh_for(flat, offs[0], ps[0])
    s.fresh_for(flat, offs[1], ps[1])
    assert len(calls) == 5
    assert s.buffers[0] is copy                                      # one buffer throughout
    assert s.versions == {o: p._version for p, o in zip(ps, offs)}
    s.fresh_for(flat)                                                # no resident named: the buffer as stamped
    assert len(calls) == 5


def test_stamp_and_weight_key_are_one_spelling(home):
    flat, ps = home
    for change in (lambda: None, lambda: written(flat), written_everywhere, lambda: ps[0].data.mul_(2.0),
                   lambda: ps[0].detach().mul_(2.0)):
        change()
        for p in ps:
            assert stamp(p) == weight_key(p)[1:] == ops.weight_key(p)[1:]
            assert weight_key(p)[0] == p.data_ptr()
            assert stamp(p)[1:] == stamp(flat)[1:]                   # a resident carries its buffer's epochs
    e = stamp(flat)
    written(flat)
    assert stamp(flat) == (e[0], e[1], e[2] + 1) and stamp(ps[2]) == (ps[2]._version, e[1], e[2] + 1)
    written_everywhere()
    assert stamp(flat) == (e[0], e[1] + 1, e[2] + 1)
    lone = torch.nn.Parameter(torch.zeros(3))
    assert weight_key(lone) == (lone.data_ptr(), 0, e[1] + 1, 0)
    assert ops.WEIGHT_EPOCH is shadows.WEIGHT_EPOCH


def test_bf16_weight_follows_every_kind_of_write(home):
    flat, ps = home
    convs = ps[:2]
    views = [ops.bf16_weight(p) for p in convs]
    ptrs = [v.data_ptr() for v in views]
    shadow = flat._gad_bf16.buffers[0]

    def check():
        for p, ptr in zip(convs, ptrs):
            got = ops.bf16_weight(p)
            assert got.data_ptr() == ptr and got.dtype == torch.bfloat16
            assert torch.equal(got, ops.weight_krsc(p).detach().to(torch.bfloat16))
        assert flat._gad_bf16.buffers[0] is shadow
    check()
    flat.data.mul_(1.5)                                              # 1. behind torch's back, one buffer named
    written(flat)
    check()
    with torch.no_grad():                                            # 2. through torch, one resident
        convs[1].copy_(convs[1] * 0.25)
    check()
    for p in convs:                                                  # 3. behind torch's back, no buffer named (EMAModel.copy_to)
        p.data.copy_(p.data * 3.0)
    written_everywhere()
    check()
    with torch.no_grad():                                            # 4. through torch, the whole buffer
        flat.detach().add_(1.0)
    check()


def torch_rotate(flat, out, table, tiles):
    """what gad_rotate_conv3x3 computes: W'[ci][2-r][2-s][co] = W[co][r][s][ci] for every 3x3 resident"""
    for p, off, n in flat._gad_params:
        if p.ndim == 4:
            co, ci = p.shape[:2]
            out[off:off + n].view(ci, 3, 3, co).copy_(flat.detach()[off:off + n].view(co, 3, 3, ci).flip(1, 2).permute(3, 1, 2, 0))


def test_the_rotated_shadow_is_the_home_of_further_shadows(home, monkeypatch):
    flat, ps = home
    launches = []
    monkeypatch.setattr(ops, "_rotate_conv3x3", lambda *a: (launches.append(1), torch_rotate(*a)))
    w = ps[1]
    off, n = w._gad_flat[1:]

    def check(n_launches):
        r = ops.rotated_weight(w)
        assert len(launches) == n_launches
        assert torch.equal(ops.weight_krsc(r), ops.weight_krsc(w).detach().flip(1, 2).permute(3, 1, 2, 0))
        assert torch.equal(ops.bf16_weight(r), ops.weight_krsc(r).to(torch.bfloat16))      # derived from the shadow, follows it
        return r
    r = check(1)
    shadow = flat._gad_rot.buffers[0]
    assert r._gad_flat[0] is shadow and r._gad_flat[1:] == (off, n) and ops._in_flat_buffer(r)
    assert shadow._gad_conv3x3 == [(p._gad_flat[1], 64, 64) for p in ps[:2]]
    casts = []
    cast = shadow._gad_bf16.refresh
    shadow._gad_bf16.refresh = lambda src: (casts.append(1), cast(src))
    assert check(1) is r and ops.rotated_weight(ps[0]) is not r and not casts              # nothing moved: no launch, no cast
    flat.data.mul_(1.5)
    written(flat)
    assert check(2) is r and len(casts) == 1                                               # one launch, then one cast
    with torch.no_grad():
        w.copy_(w * 0.25)
    assert check(3) is r and len(casts) == 2
    ops.rotated_weight(ps[0])                                                              # the sibling: covered
    ops.bf16_weight(ops.rotated_weight(ps[0]))
    assert len(launches) == 3 and len(casts) == 2
    assert flat._gad_rot.buffers[0] is shadow and r._gad_flat[0] is shadow


def test_per_parameter_cache():
    w = conv_weight(4)                                               # frozen, outside any buffer
    r = ops.rotated_weight(w)
    assert ops.rotated_weight(w) is r and w._gad_rot.value is r and w._gad_rot.key == weight_key(w)
    assert torch.equal(ops.weight_krsc(r), ops.weight_krsc(w).flip(1, 2).permute(3, 1, 2, 0))
    w.mul_(2.0)
    r2 = ops.rotated_weight(w)
    assert r2 is not r and torch.equal(ops.weight_krsc(r2), ops.weight_krsc(w).flip(1, 2).permute(3, 1, 2, 0))
    written_everywhere()
    assert ops.rotated_weight(w) is not r2
    b = ops.bf16_weight(w)
    assert ops.bf16_weight(w) is b and torch.equal(b, ops.weight_krsc(w).to(torch.bfloat16))
    # the in-place variant: allocated once, rewritten per version at a fixed address
    made, filled = [], []

    def make():
        made.append(1)
        return torch.empty(w.numel())

    def fill(v):
        filled.append(1)
        v.copy_(ops.weight_krsc(w).reshape(-1))
    v = cached(w, "_test_inplace", make, fill)
    ptr = v.data_ptr()
    assert cached(w, "_test_inplace", make, fill) is v and (len(made), len(filled)) == (1, 1)
    w.mul_(0.5)
    v2 = cached(w, "_test_inplace", make, fill)
    assert v2 is v and v2.data_ptr() == ptr and (len(made), len(filled)) == (1, 2)
    assert torch.equal(v2, ops.weight_krsc(w).reshape(-1))


def test_half_weight_rot_drops_its_stepping_stone(monkeypatch):
    monkeypatch.setattr(half, "to_half", lambda x: x.contiguous().to(torch.bfloat16))
    w = conv_weight(5)
    hr = half.half_weight_rot(w)
    assert not hasattr(w, "_gad_rot") and half.half_weight_rot(w) is hr
    assert torch.equal(hr, ops.weight_krsc(w).flip(1, 2).permute(3, 1, 2, 0).to(torch.bfloat16))
    kept = ops.rotated_weight(w)                                     # one that somebody else made stays
    w.mul_(2.0)
    half.half_weight_rot(w)
    assert hasattr(w, "_gad_rot") and ops.rotated_weight(w) is not kept


# ---- every place that writes weights where torch does not see it announces the write
def global_epoch():
    return shadows.WEIGHT_EPOCH[0]


def epoch_of(buf):
    return stamp(buf)[2]


def test_ema_copy_to_and_restore_announce():
    ps = [torch.nn.Parameter(torch.ones(4)), torch.nn.Parameter(torch.ones(2, 3))]
    ema = EMAModel(ps)
    for s in ema.shadow_params:
        s.mul_(2.0)
    ema.store(ps)
    e, versions = global_epoch(), [p._version for p in ps]
    ema.copy_to(ps)
    assert global_epoch() == e + 1 and [p._version for p in ps] == versions and all((p == 2).all() for p in ps)
    ema.restore(ps)
    assert global_epoch() == e + 2 and [p._version for p in ps] == versions and all((p == 1).all() for p in ps)


def test_the_raw_optimizer_step_announces(home, monkeypatch):
    flat, _ = home
    monkeypatch.setattr(ops._capi, "load", lambda: SimpleNamespace(gad_clip_adam_ema=lambda *a: 0))
    monkeypatch.setattr(ops, "_stream", lambda: None)
    e = epoch_of(flat)
    z = torch.zeros_like(flat)
    ops.clip_adam_ema_raw(flat, z, z, z, None, None, max_norm=0.0, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0,
                          adamw=False, step=1, ema_decay=0.0)
    assert epoch_of(flat) == e + 1


def test_influence_apply_announces(home):
    from gad.influence import InfluenceUnlearner
    flat, _ = home
    e, before = epoch_of(flat), flat.detach().clone()
    InfluenceUnlearner.apply(SimpleNamespace(flat=flat), torch.ones_like(flat), 0.5)
    assert epoch_of(flat) == e + 1 and torch.equal(flat, before + 0.5)


def test_graph_capture_of_the_training_step_announces(home, monkeypatch):
    """FusedTrainer._step_graphed: the launches that refresh the derived weights must be part of the capture"""
    flat, _ = home
    monkeypatch.setattr(torch.cuda, "CUDAGraph", lambda: SimpleNamespace(replay=lambda: None))
    monkeypatch.setattr(torch.cuda, "graph", lambda g: contextlib.nullcontext())
    monkeypatch.setattr(ops, "WS_BYTES", 16)
    t = FusedTrainer.__new__(FusedTrainer)
    t.flat, t._graph, t._graph_failed = flat, None, False
    seen = []
    t._forward_backward = lambda *a: (seen.append(epoch_of(flat)), torch.zeros(1))[1]      # the launches: none
    t.optimizer_step = lambda: None
    e = epoch_of(flat)
    x = torch.zeros(2, 3, 4, 4)
    t._step_graphed(x, x.clone(), torch.zeros(2, dtype=torch.long), [], None)
    assert not t._graph_failed and seen == [e + 1] and epoch_of(flat) == e + 1
    t._step_graphed(x, x.clone(), torch.zeros(2, dtype=torch.long), [], None)                   # a replay captures nothing
    assert seen == [e + 1] and epoch_of(flat) == e + 1


def test_coalition_hand_over_of_the_ema_weights_announces(home, monkeypatch):
    """CoalitionEngine.train_phase ends by copying the EMA buffer over the model's flat buffer"""
    from gad import coalition
    flat, _ = home
    ema_flat = torch.full_like(flat, 7.0)
    monkeypatch.setattr(torch.cuda, "Event", lambda **kw: SimpleNamespace(record=lambda: None))
    monkeypatch.setattr(coalition, "DeviceLoader", lambda *a, **kw: ())
    model = SimpleNamespace(flat=(flat, None), eval=lambda: None)
    engine = SimpleNamespace(coalition=lambda seed: ([0], [1]), opt_seed=0, load_base=lambda: (model, None),
                             make_trainer=lambda m, e: SimpleNamespace(ema_flat=ema_flat), dataset=None, config={"batch_size": 1},
                             device=torch.device("cpu"), train_scheduler=SimpleNamespace(config=SimpleNamespace(num_train_timesteps=10)),
                             gd_steps=0)
    e = global_epoch()
    with pytest.raises(StopIteration) as done:
        next(coalition.CoalitionEngine.train_phase(engine, 0))
    assert done.value.value["model"] is model and torch.equal(flat, ema_flat) and global_epoch() == e + 1


def test_loading_lora_weights_announces():
    from gad.sd import UNet2DConditionModel
    proj = [SimpleNamespace(weight=torch.zeros(8, 16), set_lora_layer=lambda layer, i=i: loaded.__setitem__(i, layer)) for i in range(4)]
    loaded = {}
    attn = SimpleNamespace(to_q=proj[0], to_k=proj[1], to_v=proj[2], to_out=[proj[3]])
    unet = SimpleNamespace(attention_modules=lambda: {"a.processor": attn})
    sd = {"unet.a.processor.to_k_lora.down.weight": torch.ones(4, 16), "unet.a.processor.to_k_lora.up.weight": torch.ones(8, 4)}
    e = global_epoch()
    assert UNet2DConditionModel.load_lora_state_dict(unet, sd) == 1
    assert global_epoch() == e + 1 and list(loaded) == [1] and (loaded[1].up.weight == 1).all()
