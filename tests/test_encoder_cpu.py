"""The pre-LN encoder the image and the text towers share (gad/encoder.py) and the chunked forward every eval network shares
(gad/extractor.py), without a GPU: the seeded weights are pinned by digest (seeded towers stand in for pretrained ones under
tags that database rows carry), the launches of a whole tower are recorded and compared call by call, operand by operand,
and `_chunked` is run through each kind of network."""
import hashlib
from types import SimpleNamespace

import pytest
import torch

from gad import _capi, encoder, extractor, ops, text, vae, vit
from gad._capi import GELU_ERF, GELU_QUICK

VIT_CLIP = vit.Config(32, 8, 32, 2, 2, 64, 16)
VIT_BLIP = vit.Config(32, 8, 32, 2, 2, 64, None, act="gelu", ln_pre=False, patch_bias=True)
TEXT_PROJ = text.TextConfig(64, 8, 32, 2, 2, 64, 16)
TEXT_NOPROJ = text.TextConfig(64, 8, 32, 2, 2, 64, None)


# ---- 1. seeded weights ------------------------------------------------------------------------------------------------------
def _digest(sd):
    h = hashlib.sha256()
    for key, t in sd.items():
        h.update(key.encode())
        h.update(t.contiguous().numpy().tobytes())
    return h.hexdigest()[:16]


# what the towers gave before the rule moved into gad/encoder.py (torch 2.10, CPU generator), all at seed 7
SEEDED = {
    "vit clip": (lambda: vit.seeded_state_dict(VIT_CLIP, 7), "9a0a1ec604550e0a"),
    "vit blip": (lambda: vit.seeded_state_dict(VIT_BLIP, 7), "97461ba163845756"),
    "text openai": (lambda: text.seeded_state_dict(TEXT_PROJ, 7, "openai"), "4dec779c7d80c307"),
    "text hf": (lambda: text.seeded_state_dict(TEXT_PROJ, 7, "hf"), "41451ea863564d68"),
    "text hf, no projection": (lambda: text.seeded_state_dict(TEXT_NOPROJ, 7, "hf"), "e522666c00d2a743"),
}


@pytest.mark.parametrize("case", sorted(SEEDED))
def test_seeded_weights_keep_their_digest(case):
    make, want = SEEDED[case]
    assert _digest(make()) == want


def test_one_table_gives_every_layout_the_same_block():
    W, M = 8, 12
    loaded = {}
    for layout in sorted(encoder.LAYOUTS):
        shapes = encoder.block_shapes(layout, 3, W, M)
        assert len(shapes) == (16 if layout == "hf_split" else 12) and all(k.startswith(encoder.LAYOUTS[layout]["block"].format(3)) for k in shapes)
        g = torch.Generator().manual_seed(0)
        sd = {k: torch.randn(s, generator=g).half() for k, s in shapes.items()}
        blk = encoder.load_block(lambda k: sd[k].detach().float().contiguous(), layout, 3)
        assert list(blk) == ["ln1", "ln2", "qkv", "out", "fc", "proj"]
        assert all(t.dtype == torch.float32 and t.is_contiguous() for pair in blk.values() for t in pair)
        loaded[layout] = {k: tuple(tuple(t.shape) for t in pair) for k, pair in blk.items()}
        if layout == "hf_split":
            p = "encoder.layers.3.self_attn."
            assert torch.equal(blk["qkv"][0], torch.cat([sd[p + f"{n}_proj.weight"] for n in "qkv"], 0).float())
            assert torch.equal(blk["qkv"][1], torch.cat([sd[p + f"{n}_proj.bias"] for n in "qkv"], 0).float())
    assert loaded["openai"] == loaded["hf_fused"] == loaded["hf_split"]
    assert loaded["openai"] == dict(ln1=((W,), (W,)), ln2=((W,), (W,)), qkv=((3 * W, W), (3 * W,)), out=((W, W), (W,)),
                                    fc=((M, W), (M,)), proj=((W, M), (W,)))


# ---- 2. the launch trace ----------------------------------------------------------------------------------------------------
@pytest.fixture
def trace(monkeypatch):
    """every launch the towers make replaced by a recorder that returns zeros of the right shape -> the list of calls"""
    calls = []

    def rec(name, out, **info):
        calls.append(SimpleNamespace(name=name, out=out, **info))
        return out

    def linear(x, w, bias=None, residual=None, alpha=1.0, force_f32=False):
        assert x.shape[1] == w.shape[1] and alpha == 1.0
        return rec("linear", torch.zeros(x.shape[0], w.shape[0]), x=x, w=w, bias=bias, residual=residual, force_f32=force_f32)

    def layernorm(x, gamma, beta, eps):
        return rec("ln", torch.zeros_like(x), x=x, gb=(gamma, beta), eps=eps), None, None

    def attention(name):
        return lambda qkv, Bn, T, Cq, heads: rec(name, torch.zeros(Bn, T, Cq), x=qkv, args=(Bn, T, Cq, heads))

    def resize(x, R, P, rh, rw, oy, ox, a=1.0, b=0.0):
        return rec("resize_patches", torch.zeros(x.shape[0] * (R // P) ** 2, P * P * 3), x=x, args=(R, P, rh, rw, oy, ox, a, b))

    def vit_tokens(emb, cls, pos, g, b, out, Bn, T, W, eps, stream):
        rec("vit_tokens", None, ptrs=(emb, cls, pos, g, b), out_ptr=out, args=(Bn, T, W, eps))
        return 0

    monkeypatch.setattr(ops, "linear_fwd_raw", linear)
    monkeypatch.setattr(ops, "layernorm_fwd_raw", layernorm)
    monkeypatch.setattr(ops, "gelu_raw", lambda h, kind: rec("gelu", h, x=h, kind=kind))                 # in place
    monkeypatch.setattr(ops, "attention_core_qkv_raw", attention("attention_core"))
    monkeypatch.setattr(ops, "attention_causal_qkv_raw", attention("attention_causal"))
    monkeypatch.setattr(ops, "text_tokens_raw", lambda ids, tok, pos: rec("text_tokens", torch.zeros(ids.numel(), tok.shape[1]), ids=ids, tok=tok, pos=pos))
    monkeypatch.setattr(ops, "gather_rows_raw", lambda x, rows, T: rec("gather", torch.zeros(rows.numel(), x.shape[1]), x=x, rows=rows, T=T))
    monkeypatch.setattr(vit, "resize_patches_raw", resize)
    monkeypatch.setattr(ops, "_req", lambda t, name: t)
    monkeypatch.setattr(ops, "_stream", lambda: None)
    lib = _capi.load()

    class Lib:                                                   # the library, but for the one launch VisionTower.tokens makes itself
        gad_vit_tokens = staticmethod(vit_tokens)

        def __getattr__(self, name):
            return getattr(lib, name)
    monkeypatch.setattr(_capi, "load", Lib)
    return calls


def _is_linear(c, x, wb, residual):
    """a force_f32 contraction of `x` with the (weight, bias) pair `wb` (or a bare weight), both by identity"""
    w, b = wb if isinstance(wb, tuple) else (wb, None)
    return c.name == "linear" and c.x is x and c.w is w and c.bias is b and c.residual is residual and c.force_f32 is True


def _is_ln(c, x, gb, eps):
    return c.name == "ln" and c.x is x and c.gb[0] is gb[0] and c.gb[1] is gb[1] and c.eps == eps


def _check_block(c, blk, x_in, attention, Bn, T, cfg):
    """the eight calls `c` of one block on the residual stream `x_in` (None: whatever ln_1 read) -> the block's output"""
    assert [k.name for k in c] == ["ln", "linear", attention, "linear", "ln", "linear", "gelu", "linear"]
    x_in = c[0].x if x_in is None else x_in
    assert x_in.shape == (Bn * T, cfg.width)
    assert _is_ln(c[0], x_in, blk["ln1"], cfg.eps)
    assert _is_linear(c[1], c[0].out, blk["qkv"], None)
    assert c[2].x is c[1].out and c[2].args == (Bn, T, cfg.width, cfg.heads)
    o = c[3].x                                                   # the attention's output, viewed as rows
    assert o.shape == (Bn * T, cfg.width) and o.data_ptr() == c[2].out.data_ptr()
    assert _is_linear(c[3], o, blk["out"], x_in)
    assert _is_ln(c[4], c[3].out, blk["ln2"], cfg.eps)
    assert _is_linear(c[5], c[4].out, blk["fc"], None)
    assert c[6].x is c[5].out and c[6].kind == (GELU_ERF if cfg.act == "gelu" else GELU_QUICK)
    assert _is_linear(c[7], c[5].out, blk["proj"], c[3].out)
    return c[7].out


def _check_blocks(calls, tower, x_in, attention, Bn, T):
    for i in range(tower.cfg.layers):
        x_in = _check_block(calls[8 * i:8 * i + 8], tower.w[i], x_in, attention, Bn, T, tower.cfg)
    return x_in


TEXT_TOWERS = {"openai": (TEXT_PROJ, "openai"), "hf": (TEXT_PROJ, "hf"), "hf, no projection": (TEXT_NOPROJ, "hf"),
               "gelu": (text.TextConfig(64, 8, 32, 2, 2, 64, 16, act="gelu", eps=1e-6), "openai")}


def _ids(Bn, cfg):
    ids = torch.randint(1, cfg.vocab - 1, (Bn, cfg.context), generator=torch.Generator().manual_seed(1))
    for b in range(Bn):
        ids[b, (3 * b + 2) % cfg.context] = cfg.vocab - 1          # the end-of-text token, at another position in each row
    return ids


@pytest.mark.parametrize("case", sorted(TEXT_TOWERS))
def test_text_tower_launch_trace(case, trace):
    cfg, layout = TEXT_TOWERS[case]
    t = text.TextTower(cfg, text.seeded_state_dict(cfg, 7, layout))
    Bn, T = 3, cfg.context
    ids = _ids(Bn, cfg)

    def trunk():
        c = list(trace)
        trace.clear()
        assert c[0].name == "text_tokens" and torch.equal(c[0].ids, ids) and c[0].tok is t.w["tok"] and c[0].pos is t.w["pos"]
        return c[1 + 8 * cfg.layers:], _check_blocks(c[1:], t, c[0].out, "attention_causal", Bn, T)

    out = t.hidden(ids)
    tail, x = trunk()
    assert len(tail) == 1 and _is_ln(tail[0], x, t.w["ln_final"], cfg.eps) and x.shape == (Bn * T, cfg.width)
    assert out.shape == (Bn, T, cfg.width) and out.data_ptr() == tail[0].out.data_ptr()
    fns = [(t.pooled, 2)] + ([(t.embed, 3)] if cfg.embed_dim is not None else [])
    for fn, n in fns:
        out = fn(ids)
        tail, x = trunk()
        assert len(tail) == n and out is tail[-1].out
        assert tail[0].name == "gather" and tail[0].x is x and torch.equal(tail[0].rows, ids.argmax(dim=-1)) and tail[0].T == T
        assert _is_ln(tail[1], tail[0].out, t.w["ln_final"], cfg.eps)
        if n == 3:
            assert _is_linear(tail[2], tail[1].out, t.w["head"], None) and out.shape == (Bn, cfg.embed_dim)


@pytest.mark.parametrize("cfg", [VIT_CLIP, VIT_BLIP], ids=["clip", "blip"])
def test_vision_tower_launch_trace(cfg, trace):
    t = vit.VisionTower.seeded(cfg, 7)
    Bn, T = 3, cfg.tokens
    images = torch.rand(Bn, 3, 40, 56, generator=torch.Generator().manual_seed(0))
    out = t.forward(images)
    c = list(trace)
    assert c[0].name == "resize_patches" and torch.equal(c[0].x, images)
    assert c[0].args == (cfg.image_size, cfg.patch) + vit.resize_geometry(40, 56, cfg.image_size, cfg.layout) + (1.0, 0.0)
    assert _is_linear(c[1], c[0].out, t.w["patch"], None)
    ln_pre = tuple(p.data_ptr() for p in t.w["ln_pre"]) if cfg.ln_pre else (None, None)
    assert c[2].name == "vit_tokens" and c[2].args == (Bn, T, cfg.width, cfg.eps)
    assert c[2].ptrs == (c[1].out.data_ptr(), t.w["cls"].data_ptr(), t.w["pos"].data_ptr()) + ln_pre
    x = _check_blocks(c[3:], t, None, "attention_core", Bn, T)
    assert c[3].x.data_ptr() == c[2].out_ptr                       # the first block reads what gad_vit_tokens wrote
    tail = c[3 + 8 * cfg.layers:]
    assert len(tail) == (2 if cfg.embed_dim is not None else 1) and out is tail[-1].out
    rows = tail[0].x                                               # a copy of the class rows: the first of each image's T
    assert rows.shape == (Bn, cfg.width) and rows.is_contiguous() and rows.data_ptr() != x.data_ptr()
    assert _is_ln(tail[0], rows, t.w["ln_post"], cfg.eps)
    if cfg.embed_dim is not None:
        assert _is_linear(tail[1], tail[0].out, t.w["head"], None) and out.shape == (Bn, cfg.embed_dim)


# ---- 3. the chunked forward -------------------------------------------------------------------------------------------------
def _sizes():
    seen = []

    def chunk(x):
        seen.append(len(x))
        return x.float() + 1
    return seen, chunk


def test_chunked_on_an_extractor_subclass():
    seen, chunk = _sizes()

    class Net(extractor.Extractor):
        owner, dims, max_batch = "Net(x)", 4, 2
        _chunk = staticmethod(chunk)

    net = Net("net-unloaded")
    x = torch.arange(20.0).view(5, 4)
    with pytest.raises(_capi.GadError, match=r"Net\(x\): no weights loaded"):
        net(x)
    net.w = {"b": torch.zeros(1)}
    assert torch.equal(net(x), x + 1) and seen == [2, 2, 1]


def test_chunked_on_a_text_tower():
    seen, chunk = _sizes()
    ids = _ids(5, TEXT_NOPROJ)
    for fn in ("hidden", "pooled", "embed"):                         # a tower with no weights at all says so, whatever is asked
        with pytest.raises(_capi.GadError, match=r"TextTower\(text\): no weights loaded"):
            getattr(text.TextTower(TEXT_NOPROJ), fn)(ids)
    assert seen == []
    t = text.TextTower.seeded(TEXT_NOPROJ, 7)
    with pytest.raises(_capi.GadError, match=r"TextTower\(text\): this tower has no text_projection"):
        t.embed(ids)
    t.max_batch = 2
    t._hidden_chunk = chunk
    out = t.hidden(ids)
    assert seen == [2, 2, 1] and torch.equal(out, ids.float() + 1)


def test_chunked_on_an_autoencoder():
    seen, chunk = _sizes()
    m = vae.VQModel(vae.make_config("vq", (32, 64), 1, 3, 8, num_vq_embeddings=64))
    x = torch.arange(15.0).view(5, 3)
    assert m.max_batch == 8 and m.tag == "vqmodel-unloaded"
    with pytest.raises(_capi.GadError, match="VQModel: no weights loaded"):
        m._chunked(chunk, x)
    assert seen == []
    m.w, m.max_batch = {"b": torch.zeros(1)}, 2
    assert torch.equal(m._chunked(chunk, x), x + 1) and seen == [2, 2, 1]
    assert m.to("cpu") is m and m.device == torch.device("cpu")
