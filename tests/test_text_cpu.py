"""Host side of the CLIP text towers (gad/text.py, gad/clip_bpe.py): the float64 restatement of tests/text_ref.py against a golden
made by `transformers` (tests/golden/make_clip_text_golden.py), the state-dict contract, the tokenizer's known answers on a
synthetic vocabulary derived by hand from the published rule, and the environment wiring of the entry points."""
import gzip
import json
import os
import types

import numpy as np
import pytest
import torch

import text_ref as R
from gad import text
from gad.clip_bpe import ClipBPE, bytes_to_unicode

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "clip_text.npz")


def golden():
    z = np.load(GOLDEN)
    V, T, W, L, H, M, E = (int(v) for v in z["config"])
    cfg = text.TextConfig(V, T, W, L, H, M, E)
    sd = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd/")}
    return cfg, sd, torch.from_numpy(z["ids"]), torch.from_numpy(z["last_hidden_state"]), torch.from_numpy(z["text_embeds"])


# ---------------------------------------------------------------------------------------------------------------
# the reference against transformers
# ---------------------------------------------------------------------------------------------------------------
def test_reference_reproduces_the_transformers_golden_in_both_layouts():
    cfg, sd, ids, want_h, want_e = golden()
    assert want_h.dtype == torch.float64 and tuple(want_h.shape) == (3, 20, 32) and tuple(want_e.shape) == (3, 24)
    assert ids[0, 6:].eq(47).all() and ids[1].argmax() == 19 and ids[2, 1:].eq(47).all() and ids[:, 0].eq(46).all()
    with torch.no_grad():
        for name, d in (("hf", sd), ("openai", R.to_openai(sd, cfg.layers))):
            h, e = R.hidden_and_embed(d, cfg, ids)
            eh, ee = float((h - want_h).abs().max()), float((e - want_e).abs().max())
            print(f"text_ref ({name}) against transformers: hidden {eh:.3e}, embeds {ee:.3e}")
            assert eh <= 1e-10 and ee <= 1e-10
    oa = R.to_openai(sd, cfg.layers)
    assert tuple(oa["transformer.resblocks.1.attn.in_proj_weight"].shape) == (96, 32) and tuple(oa["text_projection"].shape) == (32, 24)
    assert set(oa) == set(text.expected_shapes(cfg, "openai"))


def test_reference_is_causal():
    cfg, sd, ids, _, _ = golden()
    ids2 = ids.clone()
    ids2[1, 3] = (ids2[1, 3] + 1) % 46
    with torch.no_grad():
        a, b = R.hidden(sd, cfg, ids), R.hidden(sd, cfg, ids2)
    assert torch.equal(a[1, :3], b[1, :3]) and not torch.equal(a[1, 3], b[1, 3])


# ---------------------------------------------------------------------------------------------------------------
# shapes and state dicts
# ---------------------------------------------------------------------------------------------------------------
def _count(shapes):
    return sum(int(np.prod(s)) for s in shapes.values())


def test_expected_shapes_of_the_presets():
    """hand-written: per block 4 W (two norms) + 3 W^2 + 3 W (qkv) + W^2 + W (out) + 2 W mlp + mlp + W (MLP), which is
    12 W^2 + 9 W + mlp at mlp = 4 W; around them the token table V W, positions T W, ln_final 2 W and the projection W E"""
    b32, sd14 = text.expected_shapes("clip_text_b32"), text.expected_shapes("sd_text_l14")
    assert text.PRESETS["clip_text_b32"] == text.TextConfig(49408, 77, 512, 12, 8, 2048, 512)
    assert text.PRESETS["sd_text_l14"] == text.TextConfig(49408, 77, 768, 12, 12, 3072, None)
    assert b32["token_embedding.weight"] == (49408, 512) and b32["positional_embedding"] == (77, 512)
    assert b32["text_projection"] == (512, 512) and b32["transformer.resblocks.11.attn.in_proj_weight"] == (1536, 512)
    assert b32["ln_final.bias"] == (512,) and "transformer.resblocks.12.ln_1.weight" not in b32
    assert sd14["embeddings.token_embedding.weight"] == (49408, 768) and sd14["embeddings.position_embedding.weight"] == (77, 768)
    assert sd14["encoder.layers.11.self_attn.k_proj.weight"] == (768, 768) and sd14["encoder.layers.0.mlp.fc1.weight"] == (3072, 768)
    assert sd14["final_layer_norm.weight"] == (768,) and "text_projection.weight" not in sd14
    # OpenAI: 2 + 12 blocks x (4 norm + 2 in_proj + 2 out + 4 mlp) + 2 + 1; HF: 2 + 12 x (4 norm + 8 q/k/v/out + 4 mlp) + 2
    assert (len(b32), len(sd14)) == (149, 196)
    block_b, block_s = 12 * 512 * 512 + 9 * 512 + 2048, 12 * 768 * 768 + 9 * 768 + 3072
    assert _count(b32) == 49408 * 512 + 77 * 512 + 2 * 512 + 12 * block_b + 512 * 512 == 63428096
    assert _count(sd14) == 49408 * 768 + 77 * 768 + 2 * 768 + 12 * block_s == 123060480
    cfg = golden()[0]
    assert text.expected_shapes(cfg, "hf")["text_projection.weight"] == (24, 32)
    assert _count(text.expected_shapes(cfg, "hf")) == _count(text.expected_shapes(cfg, "openai"))
    with pytest.raises(ValueError, match="unknown preset 'clip_text_l14'"):
        text.expected_shapes("clip_text_l14")
    with pytest.raises(ValueError, match="head dim 24"):
        text.TextTower(text.TextConfig(64, 77, 48, 1, 2, 96, None))


def test_missing_keys_and_wrong_shapes_are_refused_by_name():
    cfg, sd, _, _, _ = golden()
    bad = dict(sd)
    del bad["text_model.encoder.layers.1.self_attn.v_proj.bias"]
    with pytest.raises(KeyError, match=r"text_model\.encoder\.layers\.1\.self_attn\.v_proj\.bias"):
        text.TextTower(cfg, bad)
    bad = dict(sd)
    del bad["text_projection.weight"]
    with pytest.raises(KeyError, match=r"'text_projection\.weight'"):
        text.TextTower(cfg, bad)
    bad = dict(sd)
    bad["text_model.embeddings.position_embedding.weight"] = torch.zeros(19, 32)
    with pytest.raises(ValueError, match=r"position_embedding\.weight.*\(19, 32\).*\(20, 32\)"):
        text.TextTower(cfg, bad)
    oa = R.to_openai(sd, cfg.layers)
    bad = dict(oa)
    del bad["ln_final.bias"]
    with pytest.raises(KeyError, match=r"ln_final\.bias"):
        text.TextTower(cfg, bad)
    bad = dict(oa)
    bad["text_projection"] = oa["text_projection"].t().contiguous()
    with pytest.raises(ValueError, match=r"text_projection.*\(24, 32\).*\(32, 24\)"):
        text.TextTower(cfg, bad)
    with pytest.raises(KeyError, match="token_embedding.weight"):
        text.TextTower(cfg, {"visual.conv1.weight": torch.zeros(1)})


def _same(a, b):
    if isinstance(a, torch.Tensor):
        return a.dtype == torch.float32 and torch.equal(a, b)
    if isinstance(a, tuple):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)


def test_prefixed_unprefixed_half_and_both_layouts_load_alike():
    cfg, sd, _, _, _ = golden()
    base = text.TextTower(cfg, sd)
    assert tuple(base.w[0]["qkv"][0].shape) == (96, 32) and tuple(base.w[0]["qkv"][1].shape) == (96,)     # q, k, v stacked at load time
    assert torch.equal(base.w[1]["qkv"][0][32:64], sd["text_model.encoder.layers.1.self_attn.k_proj.weight"])
    assert tuple(base.w["head"].shape) == (24, 32) and base.dims == 24
    plain = {(k[len("text_model."):] if k.startswith("text_model.") else k): v for k, v in sd.items()}
    assert "embeddings.token_embedding.weight" in plain and _same(text.TextTower(cfg, plain).w, base.w)
    extra = dict(sd)
    extra["text_model.embeddings.position_ids"] = torch.arange(20).view(1, 20)
    assert _same(text.TextTower(cfg, extra).w, base.w)
    # OpenAI's names inside a whole CLIP archive: the image tower's keys and logit_scale are extra
    oa = R.to_openai(sd, cfg.layers)
    oa.update({"visual.conv1.weight": torch.zeros(8, 3, 4, 4), "visual.proj": torch.zeros(8, 24), "logit_scale": torch.tensor(4.6)})
    assert _same(text.TextTower(cfg, oa).w, base.w)
    # fp16 archives: cast to fp32, so equal to the fp32 load of the rounded values
    half = {k: v.half() for k, v in sd.items()}
    assert _same(text.TextTower(cfg, half).w, text.TextTower(cfg, {k: v.float() for k, v in half.items()}).w)


def test_seeded_towers_and_tags():
    cfg = golden()[0]
    a, b = text.seeded_state_dict(cfg, 3), text.seeded_state_dict(cfg, 3)
    assert set(a) == set(text.expected_shapes(cfg)) and all(torch.equal(a[k], b[k]) for k in a)
    assert abs(float(a["ln_final.weight"].mean()) - 1) < 0.1 and float(a["positional_embedding"].std()) < 0.03
    t = text.TextTower.seeded(cfg, 3)
    assert t.tag == "text-seeded3" and t.max_batch == 256 and text.TextTower("sd_text_l14").tag == "sd_text_l14-unloaded"
    assert text.TextTower("sd_text_l14").max_batch == 128 and text.TextTower("clip_text_b32").max_batch == 256
    import gad
    assert gad.TextTower is text.TextTower and gad.CLIPTextModel is text.CLIPTextModel and gad.CLIPTokenizer is text.CLIPTokenizer


# ---------------------------------------------------------------------------------------------------------------
# the tokenizer, on a synthetic vocabulary.  The published rule: id(c) = position of c in the byte table, which starts at '!'
# (so a single ASCII character c is ord(c) - 33, and c</w> is 256 more), then one id per merge from 512, then start, end.
# ---------------------------------------------------------------------------------------------------------------
MERGES = ["p a", "pa i", "pai n", "pain t", "paint i", "painti n", "paintin g</w>", "a n</w>", "t h", "th e</w>", "' s</w>", "1 9</w>"]
SOT, EOT = 524, 525


def _ch(c, end=False):
    return ord(c) - 33 + (256 if end else 0)


@pytest.fixture(scope="module")
def vocab_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("bpe")
    txt = "#version: 0.2\n" + "\n".join(MERGES) + "\n"
    (d / "merges_plain.txt").write_text(txt, encoding="utf-8")
    with gzip.open(d / "bpe_simple_vocab.txt.gz", "wt", encoding="utf-8") as f:
        f.write(txt)
    # the HF form of the same vocabulary, written from the rule (not from ClipBPE)
    symbols = list(bytes_to_unicode().values())
    names = symbols + [s + "</w>" for s in symbols] + [m.replace(" ", "") for m in MERGES] + ["<|startoftext|>", "<|endoftext|>"]
    hf = d / "hf"
    hf.mkdir()
    (hf / "vocab.json").write_text(json.dumps({s: i for i, s in enumerate(names)}), encoding="utf-8")
    (hf / "merges.txt").write_text(txt, encoding="utf-8")
    return types.SimpleNamespace(txt=str(d / "merges_plain.txt"), gz=str(d / "bpe_simple_vocab.txt.gz"), hf=str(hf), dir=d)


def test_tokenizer_vocabulary_is_built_the_published_way(vocab_files):
    bpe = ClipBPE(vocab_files.gz)
    assert (bpe.sot, bpe.eot, bpe.vocab_size) == (SOT, EOT, 526)
    assert bpe.encoder["!"] == 0 and bpe.encoder["a"] == _ch("a") == 64 and bpe.encoder["a</w>"] == 320
    assert bpe.encoder["pa"] == 512 and bpe.encoder["painting</w>"] == 518 and bpe.encoder["19</w>"] == 523
    assert len(set(bytes_to_unicode().values())) == 256


def test_tokenizer_known_answers(vocab_files):
    bpe = ClipBPE(vocab_files.txt)
    got = bpe.encode("a Painting")
    assert got.dtype == np.int32 and got.shape == (77,)
    assert got[:4].tolist() == [SOT, 320, 518, EOT] and (got[4:] == EOT).all()
    assert bpe.pieces("painting's") == [518, 522]
    assert bpe.pieces("1989") == [272, 280, 279, 280]                   # digits are single-character pieces: `1 9</w>` never fires
    assert bpe.pieces("the") == [521] and bpe.pieces("an") == [519]
    # `t h` merges but `th e</w>` needs the e at the end of the word; `p a` + `pa i` + `pai n` stop at "pain" + s</w>
    assert bpe.pieces("then") == [520, _ch("e"), _ch("n", True)]
    assert bpe.pieces("pains") == [514, _ch("s", True)]
    assert bpe.pieces("a-b") == [320, _ch("-", True), _ch("b", True)]
    assert bpe.pieces("") == [] and bpe.encode("")[:3].tolist() == [SOT, EOT, EOT]


def test_tokenizer_cleaning_truncation_and_padding(vocab_files):
    bpe = ClipBPE(vocab_files.txt)
    assert bpe.pieces("  A   PAINTING \n") == bpe.pieces("a painting") == [320, 518]
    assert bpe.pieces("a &amp;amp; b") == [320, _ch("&", True), _ch("b", True)]            # unescaped twice
    long = " ".join(["painting"] * 40)
    got = bpe.encode(long, context=16)
    assert got.tolist() == [SOT] + [518] * 14 + [EOT]                                     # the end token stays last
    e, z = bpe.encode("the painting", pad="eot"), bpe.encode("the painting", pad="zero")
    assert e[:4].tolist() == z[:4].tolist() == [SOT, 521, 518, EOT] and (e[4:] == EOT).all() and (z[4:] == 0).all()
    assert int(e.argmax()) == int(z.argmax()) == 3                                         # one end-of-text row, whatever the padding
    with pytest.raises(ValueError, match="pad='max'"):
        bpe.encode("x", pad="max")
    batch = bpe.encode_batch(["a painting", ""], context=8)
    assert batch.shape == (2, 8) and batch.dtype == np.int32


def test_tokenizer_forms_agree_and_shims(vocab_files):
    a, b, c = ClipBPE(vocab_files.txt), ClipBPE(vocab_files.gz), ClipBPE(vocab_files.hf)
    for prompt in ("a Painting", "painting's the 1989 pains", "an impressionism-style painting!", ""):
        assert a.encode(prompt).tolist() == b.encode(prompt).tolist() == c.encode(prompt).tolist(), prompt
    tok = text.CLIPTokenizer.from_path(vocab_files.hf)
    assert tok.model_max_length == 77
    ids = tok(["a painting", "the"], max_length=tok.model_max_length, padding="max_length", truncation=True, return_tensors="pt").input_ids
    assert ids.dtype == torch.int64 and tuple(ids.shape) == (2, 77) and ids[0].tolist() == a.encode("a painting", pad="eot").tolist()
    assert tuple(tok("the", max_length=9, padding="max_length", truncation=True, return_tensors="pt").input_ids.shape) == (1, 9)
    empty = vocab_files.dir / "empty"
    empty.mkdir()
    with pytest.raises(FileNotFoundError, match="vocab.json"):
        ClipBPE(str(empty))


# ---------------------------------------------------------------------------------------------------------------
# environment wiring, as pure host code
# ---------------------------------------------------------------------------------------------------------------
SD_VARS = ("GAD_VAE_DECODER_TS", "GAD_VAE_WEIGHTS", "GAD_SD_SCORER", "GAD_CLIP_B32_WEIGHTS", "GAD_CLIP_L14_WEIGHTS", "GAD_AESTHETIC_WEIGHTS",
           "GAD_CLIP_BPE", "GAD_SD_TEXT_WEIGHTS")


@pytest.fixture
def clean_env(monkeypatch):
    for v in SD_VARS:
        monkeypatch.delenv(v, raising=False)
    return monkeypatch


def test_text_weights_without_a_vocabulary_are_refused_by_name(clean_env, tmp_path):
    from text_to_image import compute_model_behaviors as M
    assert text.sd_text_setting() is None
    clean_env.setenv("GAD_SD_TEXT_WEIGHTS", "/nowhere/text_encoder/model.safetensors")
    with pytest.raises(ValueError, match="GAD_SD_TEXT_WEIGHTS is set but GAD_CLIP_BPE is not"):
        text.sd_text_setting()
    with pytest.raises(ValueError, match="GAD_CLIP_BPE"):
        M.scorer_settings(None)
    args = M.parse_args(["--reference_lora_dir", str(tmp_path), "--db", str(tmp_path / "db.jsonl"), "--exp_name", "x"])
    with pytest.raises(ValueError, match="GAD_CLIP_BPE"):
        M.main(args, backend=types.SimpleNamespace())             # before anything loads: the weights' path does not exist
    with pytest.raises(ValueError, match="GAD_CLIP_BPE"):
        text.prompt_context("a painting", None, 768, torch.device("cpu"))
    clean_env.setenv("GAD_CLIP_BPE", "/nowhere/bpe.txt.gz")
    assert text.sd_text_setting() == ("/nowhere/text_encoder/model.safetensors", "/nowhere/bpe.txt.gz")
    assert M.scorer_settings(None) is None                         # the text encoder alone keeps the stand-in scorer
    # a file that carries both keys wins: nothing is loaded (the paths do not exist) and no encoder tag is reported
    pe = {"cond": torch.ones(77, 8), "uncond": torch.zeros(77, 8)}
    cond, uncond, tag = text.prompt_context("a painting", pe, 8, torch.device("cpu"))
    assert torch.equal(cond, pe["cond"]) and torch.equal(uncond, pe["uncond"]) and tag is None


def test_clip_prompt_needs_the_vocabulary_or_the_file(clean_env):
    from text_to_image import compute_model_behaviors as M
    clean_env.setenv("GAD_SD_SCORER", "clip-seeded")
    clean_env.setenv("GAD_VAE_DECODER_TS", "/nowhere/decoder.pt")
    with pytest.raises(ValueError, match="the CLIP text tower is not part of this project.*'clip_prompt'"):
        M.scorer_settings(None)                                    # word for word what it was
    assert M.scorer_settings({"clip_prompt": torch.ones(512)}) == {"weights": None}
    clean_env.setenv("GAD_CLIP_BPE", "/nowhere/bpe.txt.gz")
    assert M.scorer_settings(None) == {"weights": None, "text": True}
    assert M.scorer_settings({"cond": torch.zeros(77, 8)}) == {"weights": None, "text": True}
    assert M.scorer_settings({"clip_prompt": torch.ones(512)}) == {"weights": None}        # the file still wins
    clean_env.delenv("GAD_VAE_DECODER_TS")
    with pytest.raises(ValueError, match="GAD_VAE_DECODER_TS"):
        M.scorer_settings(None)                                    # a vocabulary does not make latents images


def test_nothing_set_keeps_the_stand_ins(clean_env):
    from text_to_image import compute_model_behaviors as M
    assert M.scorer_settings(None) is None
    args = M.parse_args(["--reference_lora_dir", "a", "--db", "b", "--exp_name", "c"])
    lists = {b: [0.5, 0.25] for b in M.BEHAVIOURS}
    row = M.assemble_row(args, lists, lists, [1], [2])
    assert row["feature_extractor"] == "standin-latent-scorer-seed1234" and "prompt_encoder" not in row
    # the seeded stand-in for CLIP-text(prompt) is what the programs drew before: sha256(prompt) seeds two N(0, 0.5^2) draws
    import hashlib
    prompt = "a Post-Impressionist painting"
    g = torch.Generator().manual_seed(int(hashlib.sha256(prompt.encode()).hexdigest()[:8], 16) % (2 ** 31))
    want = torch.randn(77, 8, generator=g) * 0.5, torch.randn(77, 8, generator=g) * 0.5
    cond, uncond, tag = text.prompt_context(prompt, None, 8, torch.device("cpu"))
    assert torch.equal(cond, want[0]) and torch.equal(uncond, want[1]) and tag is None
