"""The CLIP text towers on the GPU: gad_attention_causal_fwd, gad_text_tokens and gad_gather_rows through the C ABI, gad/text.py
against the float64 restatement of tests/text_ref.py (itself checked against `transformers` in tests/test_text_cpu.py), and
compute_model_behaviors with the text tower in the prompt's place.

The attention bounds are those tests/test_gpu_attention.py uses for the exact-fp32 kernels (3e-5 on o, 1e-4 on lse, unit-normal
operands); the tower bounds are 8 x what float32 arithmetic costs on the SAME inputs, measured on the CPU by the reference
(`text_ref` in float32 against float64) and written next to the constant; the inputs are seeded, so the yardsticks are fixed."""
import ctypes as C
import functools
import json
import math
import os

import numpy as np
import pytest
import torch

import text_ref as R
from gad import _capi, ops, text, vit
from gad.clip_bpe import ClipBPE

pytestmark = pytest.mark.gpu
dev = torch.device("cuda:0")
TAIL = 5                       # rows allocated past the end of every output
SENTINEL = -123.5
B, HEADS = 2, 3


def _lib():
    return _capi.load()


# ---------------------------------------------------------------------------------------------------------------
# gad_attention_causal_fwd
# ---------------------------------------------------------------------------------------------------------------
# a single key; exactly one tile; one tile plus a row; the text towers' 77 = 4 x 16 + 13 (a 13-row tail); the maximum
SHAPES = [(T, d) for T in (1, 16, 17, 77, 128) for d in (16, 64)] + [(77, 32)]


@functools.lru_cache(maxsize=None)
def _qkv(T, d):
    return torch.randn(B * T, 3 * HEADS * d, generator=torch.Generator().manual_seed(1000 * T + d))


@functools.lru_cache(maxsize=None)
def _reference(T, d):
    """float64: (o [B, T, H d], lse [B, H, T] in the log2 domain of gad_attention_fwd)"""
    W = HEADS * d
    q, k, v = (_qkv(T, d).double()[:, i * W:(i + 1) * W].reshape(B, T, HEADS, d).transpose(1, 2) for i in range(3))
    s = q @ k.transpose(-1, -2) / math.sqrt(d)
    s = s.masked_fill(torch.ones(T, T, dtype=torch.bool).triu(1), float("-inf"))
    o = (torch.softmax(s, dim=-1) @ v).transpose(1, 2).reshape(B, T, W)
    return o, torch.logsumexp(s, dim=-1) / math.log(2.0)


def _launch(q, k, v, T, d, ldq, ldk, ldv, want_lse=False, Tk=None, precision=0, expect=0):
    """-> (rc, o [B T + TAIL, H d] with its sentinel rows, lse or None); q, k, v are device tensors or views (data_ptr = column offset)"""
    W = HEADS * d
    o = torch.full((B * T + TAIL, W), SENTINEL, device=dev)
    lse = torch.full((B * HEADS * T + TAIL,), SENTINEL, device=dev) if want_lse else None
    Tk = T if Tk is None else Tk
    a = ops._attention_args(q, k, v, o, lse, B, HEADS, T, Tk, d, ldq, ldk, ldv, T * ldq, Tk * ldk, Tk * ldv)
    a.operand_precision = precision
    rc = _lib().gad_attention_causal_fwd(C.byref(a), ops._stream())
    torch.cuda.synchronize()
    assert rc == expect, _lib().gad_last_error()
    return rc, o, lse


def _fused(qkv_dev, T, d, **kw):
    W = HEADS * d
    return _launch(qkv_dev[:, 0:W], qkv_dev[:, W:2 * W], qkv_dev[:, 2 * W:3 * W], T, d, 3 * W, 3 * W, 3 * W, **kw)


@pytest.mark.parametrize("T,d", SHAPES)
def test_causal_attention_against_float64(T, d):
    lib, W = _lib(), HEADS * d
    assert lib.gad_attention_causal_supported(T, d) == 1
    want_o, want_lse = _reference(T, d)
    qkv = _qkv(T, d).to(dev)
    parts = [qkv[:, i * W:(i + 1) * W].contiguous() for i in range(3)]
    outs = []
    for form in ("fused", "contiguous"):
        for with_lse in (False, True):
            if form == "fused":
                _, o, lse = _fused(qkv, T, d, want_lse=with_lse)
            else:
                _, o, lse = _launch(*parts, T, d, W, W, W, want_lse=with_lse)
            assert bool((o[B * T:] == SENTINEL).all())
            err = float((o[:B * T].cpu().double().view(B, T, W) - want_o).abs().max())
            print(f"causal T={T} d={d} {form} lse={with_lse}: o max abs err {err:.3e} (bound 3e-5)")
            assert err < 3e-5
            if with_lse:
                assert bool((lse[B * HEADS * T:] == SENTINEL).all())
                lerr = float((lse[:B * HEADS * T].cpu().double().view(B, HEADS, T) - want_lse).abs().max())
                print(f"    lse max abs err {lerr:.3e} (bound 1e-4)")
                assert lerr < 1e-4
            outs.append(o)
    for o in outs[1:]:                                             # the operands' strides and the lse store change no bit of o
        assert torch.equal(o, outs[0])
    assert torch.equal(_fused(qkv, T, d)[1], outs[0])              # and a second launch gives the same bits


@pytest.mark.parametrize("d", [16, 64])
@pytest.mark.parametrize("T", [17, 77])
def test_a_later_key_never_enters_an_earlier_row(T, d):
    """keys and values from t0 on become NaN: rows before t0 keep their bits.  A tile that is computed and then masked, a zero
    probability multiplied into a NaN value, or a padded column that leaks would each show here."""
    W = HEADS * d
    clean = _qkv(T, d).to(dev)
    _, o_clean, lse_clean = _fused(clean, T, d, want_lse=True)
    assert bool(torch.isfinite(o_clean[:B * T]).all())
    for t0 in (1, 16, 17, 64):
        if t0 >= T:
            continue
        bad = clean.clone().view(B, T, 3 * W)
        bad[:, t0:, W:] = float("nan")
        _, o, lse = _fused(bad.view(B * T, 3 * W), T, d, want_lse=True)
        got, want = o[:B * T].view(B, T, W)[:, :t0], o_clean[:B * T].view(B, T, W)[:, :t0]
        assert bool(torch.isfinite(got).all()), (T, d, t0)
        assert torch.equal(got, want), (T, d, t0)
        assert torch.equal(lse[:B * HEADS * T].view(B, HEADS, T)[:, :, :t0], lse_clean[:B * HEADS * T].view(B, HEADS, T)[:, :, :t0])
        assert bool((o[B * T:] == SENTINEL).all())
        assert bool(torch.isnan(o[:B * T].view(B, T, W)[:, t0:]).all())        # and the rows that do see them say so


def test_causal_refusals_launch_nothing():
    lib, T, d = _lib(), 32, 16
    W = HEADS * d
    big = torch.zeros(B * 129 + 8, 3 * HEADS * 64, device=dev)

    def refused(why, *args, **kw):
        rc, o, _ = _launch(*args, expect=1, **kw)
        msg = lib.gad_last_error().decode()
        assert "gad_attention_causal_fwd" in msg and why in msg, msg
        assert bool((o == SENTINEL).all())

    q, k, v = big[:, 0:W], big[:, W:2 * W], big[:, 2 * W:3 * W]
    ld = big.shape[1]
    refused("Tq=32 != Tk=31", q, k, v, T, d, ld, ld, ld, Tk=31)
    refused("T=129", q, k, v, 129, d, ld, ld, ld)
    refused("head dim 40", q, k, v, T, 40, ld, ld, ld)
    refused("operand_precision", q, k, v, T, d, ld, ld, ld, precision=1)
    flat = big.view(-1)
    refused("16-byte aligned", flat[1:], k, v, T, d, ld, ld, ld)
    refused("16-byte aligned", q, k, flat[2:], T, d, ld, ld, ld)
    refused("multiples of 4", q, k, v, T, d, ld, ld + 2, ld)
    refused("smaller than heads*d", q, k, v, T, d, W - 4, ld, ld)
    assert lib.gad_attention_causal_supported(129, 64) == 0 and lib.gad_attention_causal_supported(77, 40) == 0
    assert lib.gad_attention_causal_supported(0, 64) == 0 and lib.gad_attention_causal_supported(128, 32) == 1
    with pytest.raises(_capi.GadError, match="head dim 40"):
        ops.attention_causal_qkv_raw(torch.zeros(B * T, 3 * 80, device=dev), B, T, 80, 2)


# ---------------------------------------------------------------------------------------------------------------
# gad_text_tokens, gad_gather_rows
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [32, 516])
def test_text_tokens_and_gather_rows_equal_torch_indexing(W):
    V, T, Bn = 50, 7, 3
    g = torch.Generator().manual_seed(W)
    emb, pos = torch.randn(V, W, generator=g), torch.randn(T, W, generator=g)
    ids = torch.randint(0, V, (Bn, T), generator=g)
    ids[0, 0], ids[2, 6] = 0, V - 1
    got = ops.text_tokens_raw(ids, emb.to(dev), pos.to(dev))
    assert tuple(got.shape) == (Bn * T, W) and torch.equal(got.cpu(), (emb[ids] + pos).view(Bn * T, W))
    assert torch.equal(ops.text_tokens_raw(ids.to(dev).int(), emb.to(dev), pos.to(dev)), got)           # device ids, int32
    rows = torch.tensor([6, 0, 3])
    picked = ops.gather_rows_raw(got, rows, T)
    assert torch.equal(picked.cpu(), got.cpu().view(Bn, T, W)[torch.arange(Bn), rows])
    for bad in (V, -1):
        ids2 = ids.clone()
        ids2[1, 2] = bad
        with pytest.raises(_capi.GadError, match=rf"token id {bad} is outside the vocabulary \[0, {V}\)"):
            ops.text_tokens_raw(ids2, emb.to(dev), pos.to(dev))
    with pytest.raises(_capi.GadError, match="row indices"):
        ops.gather_rows_raw(got, torch.tensor([0, 7, 0]), T)


def test_gather_kernels_clamp_and_refuse():
    """straight through the C ABI: an index outside the table is clamped (never read outside), W % 4 != 0 is refused"""
    lib, V, T, W = _lib(), 5, 3, 8
    emb, pos = torch.arange(V * W, dtype=torch.float32, device=dev).view(V, W), torch.zeros(T, W, device=dev)
    ids = torch.tensor([[-7, 2, 99]], dtype=torch.int32, device=dev)
    out = torch.full((T + TAIL, W), SENTINEL, device=dev)
    assert lib.gad_text_tokens(ids.data_ptr(), emb.data_ptr(), pos.data_ptr(), out.data_ptr(), 1, T, W, V, ops._stream()) == 0
    assert torch.equal(out[:T], emb[[0, 2, V - 1]]) and bool((out[T:] == SENTINEL).all())
    rows = torch.tensor([9], dtype=torch.int32, device=dev)
    one = torch.full((1 + TAIL, W), SENTINEL, device=dev)
    assert lib.gad_gather_rows(out.data_ptr(), rows.data_ptr(), one.data_ptr(), 1, T, W, W, ops._stream()) == 0
    assert torch.equal(one[0], out[T - 1]) and bool((one[1:] == SENTINEL).all())
    assert lib.gad_text_tokens(ids.data_ptr(), emb.data_ptr(), pos.data_ptr(), out.data_ptr(), 1, T, 6, V, ops._stream()) == 1
    assert "multiple of 4" in lib.gad_last_error().decode()
    assert lib.gad_gather_rows(out.data_ptr(), rows.data_ptr(), one.data_ptr(), 1, T, W, 6, ops._stream()) == 1
    assert "ldx" in lib.gad_last_error().decode()
    assert lib.gad_gather_rows(None, rows.data_ptr(), one.data_ptr(), 1, T, W, W, ops._stream()) == 1 and "null" in lib.gad_last_error().decode()
    torch.cuda.synchronize()
    assert bool((one[1:] == SENTINEL).all())


# ---------------------------------------------------------------------------------------------------------------
# the whole tower
# ---------------------------------------------------------------------------------------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "clip_text.npz")
SEEDED = text.TextConfig(64, 77, 128, 2, 2, 512, 48)              # the real T and head dim
SEED = 7
# text_ref in float32 on the CPU against float64 on the same ids (`tower_f32_error`), max abs over last_hidden_state (entries of
# magnitude up to 4.3) and over the projected embedding (up to 2.6): the yardstick; the GPU may take 8 x it (MFMA summation
# orders).
#                          hidden      embed
#   golden (HF layout)     1.21e-06    6.26e-07
#   golden (OpenAI)        1.21e-06    6.26e-07
#   seeded, 3 prompts      2.43e-06    1.75e-06
# The GPU's own error is printed by the tests (`pytest -s`).
TOWER_F32_ERR = {"golden": (1.21e-06, 6.26e-07), "seeded": (2.43e-06, 1.75e-06)}


@functools.lru_cache(maxsize=None)
def _golden():
    z = np.load(GOLDEN)
    cfg = text.TextConfig(*(int(v) for v in z["config"]))
    sd = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd/")}
    return cfg, sd, torch.from_numpy(z["ids"]), torch.from_numpy(z["last_hidden_state"]), torch.from_numpy(z["text_embeds"])


def _seeded_ids():
    g = torch.Generator().manual_seed(SEED)
    ids = torch.randint(0, 62, (3, 77), generator=g)
    ids[:, 0] = 62
    for b, end in enumerate((10, 76, 1)):                         # a short prompt, a full one, start + end only
        ids[b, end:] = 63
    return ids


@functools.lru_cache(maxsize=None)
def _seeded_ref(dtype=torch.float64):
    with torch.no_grad():
        return R.hidden_and_embed(text.seeded_state_dict(SEEDED, SEED), SEEDED, _seeded_ids(), dtype)


def tower_f32_error(which):
    """the yardsticks above, recomputed (CPU only)"""
    if which == "seeded":
        return tuple(float((a.double() - b).abs().max()) for a, b in zip(_seeded_ref(torch.float32), _seeded_ref()))
    cfg, sd, ids, h, e = _golden()
    with torch.no_grad():
        got = R.hidden_and_embed(sd, cfg, ids, torch.float32)
    return float((got[0].double() - h).abs().max()), float((got[1].double() - e).abs().max())


@pytest.mark.parametrize("layout", ["hf", "openai"])
def test_golden_tower_in_both_layouts(layout):
    cfg, sd, ids, want_h, want_e = _golden()
    yh, ye = TOWER_F32_ERR["golden"]
    t = text.TextTower(cfg, sd if layout == "hf" else R.to_openai(sd, cfg.layers)).to(dev)
    h, e = t.hidden(ids), t.embed(ids)
    assert tuple(h.shape) == (3, 20, 32) and tuple(e.shape) == (3, 24) and h.is_cuda
    eh, ee = float((h.cpu().double() - want_h).abs().max()), float((e.cpu().double() - want_e).abs().max())
    print(f"golden tower ({layout}): hidden max abs err {eh:.3e} (yardstick {yh:.3e}), embeds {ee:.3e} (yardstick {ye:.3e})")
    assert eh <= 8 * yh and ee <= 8 * ye
    unit = t.embed_unit(ids.to(dev))                              # device ids are taken too
    assert float((unit.norm(dim=-1) - 1).abs().max()) < 1e-6
    assert float((unit.cpu().double() - want_e / want_e.norm(dim=-1, keepdim=True)).abs().max()) <= 8 * ye
    pooled = t.pooled(ids)                                        # ln_final of the end-of-text row = that row of `hidden`
    assert torch.equal(pooled, h[torch.arange(3), ids.argmax(-1)])
    last, pool2 = text.CLIPTextModel(t)(ids)
    assert torch.equal(last, h) and torch.equal(pool2, pooled)


@pytest.mark.parametrize("Bn,max_batch", [(1, None), (3, None), (3, 2)])
def test_seeded_tower_against_the_float64_reference(Bn, max_batch):
    t = text.TextTower.seeded(SEEDED, SEED).to(dev)
    assert t.tag == f"text-seeded{SEED}"
    if max_batch:
        t.max_batch = max_batch                                   # two chunks, the second of one prompt
    ids = _seeded_ids()[:Bn]
    h, e = t.hidden(ids), t.embed(ids)
    want_h, want_e = (x[:Bn] for x in _seeded_ref())
    assert tuple(h.shape) == (Bn, 77, 128) and tuple(e.shape) == (Bn, 48)
    yh, ye = TOWER_F32_ERR["seeded"]
    eh, ee = float((h.cpu().double() - want_h).abs().max()), float((e.cpu().double() - want_e).abs().max())
    print(f"seeded tower B={Bn} max_batch={max_batch}: hidden max abs err {eh:.3e} (yardstick {yh:.3e}), embed {ee:.3e} (yardstick {ye:.3e})")
    assert eh <= 8 * yh and ee <= 8 * ye
    with pytest.raises(_capi.GadError, match=r"integers \[B, 77\]"):
        t.hidden(ids[:, :20])
    with pytest.raises(_capi.GadError, match="token id 64 is outside"):
        t.hidden(torch.full((1, 77), 64))


# ---------------------------------------------------------------------------------------------------------------
# compute_model_behaviors end to end: the prompt's CLIP embedding comes from the text tower
# ---------------------------------------------------------------------------------------------------------------
MERGES = ["p a", "pa i", "pai n", "pain t", "paint i", "painti n", "paintin g</w>", "a n</w>", "t h", "th e</w>", "' s</w>", "1 9</w>"]


def test_sd_behaviours_take_the_prompt_from_the_text_tower(tmp_path, monkeypatch):
    import gad
    from src.ddpm_config import PromptConfig
    from test_gpu_sd import SMALL, rnd
    from test_gpu_vit import TOWERS, _ToyDecoder
    from text_to_image import compute_model_behaviors as M
    tiny_text = text.TextConfig(526, 77, 64, 2, 2, 256, 32)       # the synthetic vocabulary's 526 ids into the image tower's 32 dims
    monkeypatch.setitem(vit.PRESETS, "clip_vit_b32", TOWERS["t10"][0])
    monkeypatch.setitem(vit.PRESETS, "clip_vit_l14", TOWERS["t50"][0])
    monkeypatch.setitem(text.PRESETS, "clip_text_b32", tiny_text)
    bpe = tmp_path / "merges.txt"
    bpe.write_text("#version: 0.2\n" + "\n".join(MERGES) + "\n", encoding="utf-8")
    torch.manual_seed(0)
    dec = tmp_path / "decoder.pt"
    torch.jit.script(_ToyDecoder().eval()).save(str(dec))
    monkeypatch.setenv("GAD_VAE_DECODER_TS", str(dec))
    monkeypatch.setenv("GAD_SD_SCORER", "clip-seeded")
    monkeypatch.setenv("GAD_CLIP_BPE", str(bpe))
    for v in M.WEIGHT_VARS + ("GAD_VAE_WEIGHTS", "GAD_SD_TEXT_WEIGHTS"):
        monkeypatch.delenv(v, raising=False)
    torch.manual_seed(0)
    net = gad.UNet2DConditionModel(**SMALL).to(dev)
    for i, p in enumerate(net.inject_lora(rank=4)):
        with torch.no_grad():
            p.copy_(rnd(*p.shape, seed=50 + i, scale=0.05))
    lora = tmp_path / "lora"
    net.save_attn_procs(str(lora))
    weights = tmp_path / "unet.pt"
    torch.save({k: v for k, v in net.state_dict().items() if "lora_layer" not in k}, weights)
    pe = tmp_path / "pe.pt"
    torch.save({"cond": rnd(77, 96, seed=1, scale=0.5), "uncond": rnd(77, 96, seed=2, scale=0.5)}, pe)      # no 'clip_prompt'
    db, img_dir = str(tmp_path / "db.jsonl"), tmp_path / "img"
    args = M.parse_args(["--reference_lora_dir", str(lora), "--lora_dir", str(lora), "--db", db, "--num_images", "2", "--resolution", "128",
                         "--seed", "42", "--unet_overrides", json.dumps(SMALL), "--unet_weights", str(weights), "--num_inference_steps", "2",
                         "--n_noises", "1", "--prompt_embeds", str(pe), "--exp_name", "text", "--img_dir", str(img_dir)])
    assert M.main(args)
    (row,) = [json.loads(line) for line in open(db)]
    assert row["feature_extractor"] == "clip_vit_b32-seeded1234;clip_vit_l14-seeded1234;aesthetic-seeded1234;text=clip_text_b32-seeded1234"
    assert "prompt_encoder" not in row                            # cond / uncond came from the file
    # the same cosine by hand: the seeded towers are deterministic, so the prompt's and the images' unit embeddings are these
    prompt = PromptConfig.artbench_config[args.cls]
    ids = ClipBPE(str(bpe)).encode_batch([prompt], 77, pad="zero")
    assert 2 < int(ids[0].argmax()) < 76 and ids[0, int(ids[0].argmax())] == 525 and int(ids[0, -1]) == 0
    unit = text.TextTower.seeded("clip_text_b32").to(dev).embed_unit(torch.from_numpy(ids))[0]
    assert abs(float(unit.norm()) - 1) < 1e-6
    b32 = vit.VisionTower.seeded("clip_vit_b32").to(dev)
    scores = []
    for i in range(2):
        stored = torch.load(img_dir / f"latents_seed=42_sample_{i}.pt", weights_only=False)
        img = (stored["sample_image"].float() / 255).permute(2, 0, 1).unsqueeze(0).contiguous().to(dev)
        scores.append(torch.dot(b32.embed_unit(img)[0], unit).item())
        assert row[f"generated_image_{i}_clip_prompt_score"] == pytest.approx(scores[-1], abs=1e-6)
    assert row["clip_prompt_score_avg"] == pytest.approx(float(np.mean(scores)), abs=1e-6)
    assert abs(scores[0]) <= 1.0 and scores[0] != scores[1]
