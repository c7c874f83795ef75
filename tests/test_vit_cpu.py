"""Host side of the Vision Transformer image towers (gad/vit.py): state-dict contract, the normalisation fold, the bicubic
tap table the resize kernel is built on (the library's own host routine, no GPU), and the environment wiring of the two
entry points that use the towers."""
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import vit_ref as R
from gad import scoring, vit

TINY = vit.Config(24, 8, 64, 2, 2, 256, 32)
TINY_BLIP = vit.Config(16, 4, 64, 1, 1, 128, None, act="gelu", ln_pre=False, patch_bias=True)


def _count(shapes):
    return sum(int(np.prod(s)) for s in shapes.values())


def test_expected_shapes_of_the_presets():
    """hand-written: per block 4 W (two norms) + 3 W^2 + 3 W (qkv) + W^2 + W (out) + 2 W mlp + mlp + W (MLP), which is
    12 W^2 + 9 W + mlp at mlp = 4 W; around them the patch convolution 3 P^2 W (+ W with a bias), class W, positions T W, ln_pre / ln_post 2 W each, proj W E"""
    b32, l14, blip = (vit.expected_shapes(p) for p in ("clip_vit_b32", "clip_vit_l14", "blip_vqa_base"))
    assert b32["positional_embedding"] == (50, 768) and l14["positional_embedding"] == (257, 1024)
    assert blip["embeddings.position_embedding"] == (1, 577, 768)          # HF keeps the leading batch axis
    assert b32["conv1.weight"] == (768, 3, 32, 32) and l14["conv1.weight"] == (1024, 3, 14, 14)
    assert blip["embeddings.patch_embedding.weight"] == (768, 3, 16, 16) and blip["embeddings.patch_embedding.bias"] == (768,)
    assert b32["proj"] == (768, 512) and l14["proj"] == (1024, 768) and "proj" not in blip
    assert b32["transformer.resblocks.11.attn.in_proj_weight"] == (2304, 768)
    assert l14["transformer.resblocks.23.mlp.c_fc.weight"] == (4096, 1024) and "transformer.resblocks.24.ln_1.weight" not in l14
    assert blip["encoder.layers.11.self_attn.qkv.bias"] == (2304,) and "ln_pre.weight" not in blip
    assert "conv1.bias" not in b32 and "pre_layernorm.weight" not in blip
    assert (len(b32), len(l14), len(blip)) == (152, 296, 150)
    block_b, block_l = 12 * 768 * 768 + 9 * 768 + 3072, 12 * 1024 * 1024 + 9 * 1024 + 4096
    assert _count(b32) == 3 * 1024 * 768 + 768 + 50 * 768 + 4 * 768 + 12 * block_b + 768 * 512 == 87849216
    assert _count(l14) == 3 * 196 * 1024 + 1024 + 257 * 1024 + 4 * 1024 + 24 * block_l + 1024 * 768 == 303966208
    assert _count(blip) == 3 * 256 * 768 + 768 + 768 + 577 * 768 + 2 * 768 + 12 * block_b == 86090496


def test_missing_keys_and_wrong_shapes_are_refused_by_name():
    sd = vit.seeded_state_dict(TINY, 0)
    bad = dict(sd)
    del bad["transformer.resblocks.1.mlp.c_fc.bias"]
    with pytest.raises(KeyError, match=r"transformer\.resblocks\.1\.mlp\.c_fc\.bias"):
        vit.VisionTower(TINY, bad)
    bad = dict(sd)
    bad["positional_embedding"] = torch.zeros(9, 64)
    with pytest.raises(ValueError, match=r"positional_embedding.*\(9, 64\).*\(10, 64\)"):
        vit.VisionTower(TINY, bad)
    sdb = vit.seeded_state_dict(TINY_BLIP, 0)
    del sdb["post_layernorm.weight"]
    with pytest.raises(KeyError, match="post_layernorm.weight"):
        vit.VisionTower(TINY_BLIP, sdb)
    head = vit.AestheticHead.seeded(vit.VisionTower(TINY, sd))
    with pytest.raises(ValueError, match=r"'weight'.*\(1, 33\).*\(1, 32\)"):
        head.load_state_dict({"weight": torch.zeros(1, 33), "bias": torch.zeros(1)})
    with pytest.raises(KeyError, match="bias"):
        head.load_state_dict({"weight": torch.zeros(1, 32)})
    with pytest.raises(ValueError, match="unknown preset"):
        vit.VisionTower("clip_vit_h14")


@pytest.mark.parametrize("cfg,prefix", [(TINY, "visual."), (TINY_BLIP, "vision_model.")])
def test_prefixed_unprefixed_and_fp16_state_dicts_load_alike(cfg, prefix):
    sd = {k: v.half() for k, v in vit.seeded_state_dict(cfg, 3).items()}
    plain = vit.VisionTower(cfg, sd)
    extra = {prefix + k: v for k, v in sd.items()}
    extra.update({"logit_scale": torch.ones(()), "text_projection": torch.zeros(4, 4), "text_decoder.x": torch.zeros(1)})
    prefixed = vit.VisionTower(cfg, extra)

    def leaves(w):
        for k in sorted(w, key=str):
            v = w[k]
            for t in (v.values() if isinstance(v, dict) else [v]):
                yield from (t if isinstance(t, tuple) else (t,))
    a, b = list(leaves(plain.w)), list(leaves(prefixed.w))
    assert len(a) == len(b) > 10
    for x, y in zip(a, b):
        assert x.dtype == torch.float32 and x.is_contiguous() and torch.equal(x, y)
    assert plain.w["pos"].shape == (cfg.tokens, cfg.width) and plain.w["cls"].shape == (cfg.width,)
    assert torch.equal(plain.w[0]["qkv"][0], sd[("transformer.resblocks.0.attn.in_proj_weight" if cfg.embed_dim else
                                                 "encoder.layers.0.self_attn.qkv.weight")].float())


@pytest.mark.parametrize("bias", [False, True])
def test_normalisation_folds_into_the_patch_convolution(bias):
    g = torch.Generator().manual_seed(5)
    w = torch.randn(16, 3, 4, 4, generator=g)
    b = torch.randn(16, generator=g) if bias else None
    x = torch.rand(2, 3, 12, 12, generator=g, dtype=torch.float64)
    mean = torch.tensor(vit.CLIP_MEAN, dtype=torch.float64).view(1, 3, 1, 1)
    std = torch.tensor(vit.CLIP_STD, dtype=torch.float64).view(1, 3, 1, 1)
    want = F.conv2d((x - mean) / std, w.double(), None if b is None else b.double(), stride=4)
    w2, b2 = vit.fold_normalisation(w, b, vit.CLIP_MEAN, vit.CLIP_STD)
    assert w2.dtype == b2.dtype == torch.float64
    got = F.conv2d(x, w2, b2, stride=4)
    assert ((got - want).abs().max() / want.abs().max()).item() < 1e-12


# (H, W, rh, rw, oy, ox, R): 32 -> 24; 40 x 56 with the shorter side to 30 and the centre 24 cropped; 16 -> 56 (upscaling);
# 256 -> 224; 37 x 53 -> 64 x 64
TAP_GEOMETRIES = [(32, 32, 24, 24, 0, 0, 24), (40, 56, 30, 42, 3, 9, 24), (16, 16, 56, 56, 0, 0, 56), (256, 256, 224, 224, 0, 0, 224),
                  (37, 53, 64, 64, 0, 0, 64)]


@pytest.mark.parametrize("H,W,rh,rw,oy,ox,R", TAP_GEOMETRIES)
def test_tap_table_equals_antialiased_bicubic_interpolate(H, W, rh, rw, oy, ox, R):
    x = torch.rand(2, 3, H, W, generator=torch.Generator().manual_seed(H + W), dtype=torch.float64)
    want = F.interpolate(x, size=(rh, rw), mode="bicubic", antialias=True, align_corners=False)[:, :, oy:oy + R, ox:ox + R]
    My, Mx = vit.resize_matrix(H, rh, oy, R), vit.resize_matrix(W, rw, ox, R)
    got = My @ x.numpy() @ Mx.T
    assert np.abs(got - want.numpy()).max() < 1e-12
    for n_in, n_out, o, M in ((H, rh, oy, My), (W, rw, ox, Mx)):
        start, count, w = vit.bicubic_taps(n_in, n_out, o, R)
        assert (count >= 1).all() and (start >= 0).all() and (start + count <= n_in).all() and count.max() <= w.shape[1]
        assert np.abs(M.sum(1) - 1).max() < 1e-14
        assert all((w[i, count[i]:] == 0).all() for i in range(R))


def test_resize_geometry_is_torchvisions():
    assert vit.resize_geometry(40, 56, 30, "clip") == (30, 42, 0, 6) and R.geometry(40, 56, 30, True) == (30, 42, 0, 6)
    assert vit.resize_geometry(56, 40, 24, "clip") == (33, 24, 4, 0) == R.geometry(56, 40, 24, True)
    assert vit.resize_geometry(37, 53, 64, "blip") == (64, 64, 0, 0) == R.geometry(37, 53, 64, False)
    assert vit.resize_geometry(512, 512, 224, "clip") == (224, 224, 0, 0)


def test_max_batch_keeps_activations_under_half_a_gigabyte():
    for preset, want in (("clip_vit_b32", 128), ("clip_vit_l14", 32), ("blip_vqa_base", 16)):
        assert vit.VisionTower(preset).max_batch == want


# ---- environment wiring ----
SD_VARS = ("GAD_CLIP_B32_WEIGHTS", "GAD_CLIP_L14_WEIGHTS", "GAD_AESTHETIC_WEIGHTS", "GAD_SD_SCORER", "GAD_VAE_DECODER_TS")


@pytest.fixture
def clean_env(monkeypatch):
    for v in SD_VARS + ("GAD_BLIP_VISION_WEIGHTS", "GAD_DIVERSITY_NET"):
        monkeypatch.delenv(v, raising=False)
    return monkeypatch


def test_unknown_diversity_net_is_refused(clean_env):
    clean_env.setenv("GAD_DIVERSITY_NET", "blip")
    with pytest.raises(ValueError, match="GAD_DIVERSITY_NET='blip'.*blip-seeded"):
        scoring.diversity_against_dataset(None, None, torch.device("cpu"))
    with pytest.raises(ValueError, match="blip-seeded"):
        scoring.diversity_extractor(torch.device("cpu"))
    clean_env.delenv("GAD_DIVERSITY_NET")
    assert scoring.diversity_extractor(torch.device("cpu")) is None


def test_sd_scorer_refusals_and_unchanged_default(clean_env):
    from text_to_image import compute_model_behaviors as M
    assert M.scorer_settings(None) is None and M.scorer_settings({"clip_prompt": torch.ones(512)}) is None
    clean_env.setenv("GAD_VAE_DECODER_TS", "/nowhere/decoder.pt")
    assert M.scorer_settings(None) is None                     # a decoder alone keeps the stand-in scorer
    clean_env.delenv("GAD_VAE_DECODER_TS")
    clean_env.setenv("GAD_SD_SCORER", "clip")
    with pytest.raises(ValueError, match="GAD_SD_SCORER='clip'.*clip-seeded"):
        M.scorer_settings(None)
    clean_env.setenv("GAD_SD_SCORER", "clip-seeded")
    with pytest.raises(ValueError, match="GAD_VAE_DECODER_TS"):
        M.scorer_settings({"clip_prompt": torch.ones(512)})
    clean_env.setenv("GAD_VAE_DECODER_TS", "/nowhere/decoder.pt")
    with pytest.raises(ValueError, match="'clip_prompt'"):
        M.scorer_settings({"cond": torch.zeros(77, 8), "uncond": torch.zeros(77, 8)})
    with pytest.raises(ValueError, match="'clip_prompt'"):
        M.scorer_settings(None)
    assert M.scorer_settings({"clip_prompt": torch.ones(512)}) == {"weights": None}
    clean_env.delenv("GAD_SD_SCORER")
    clean_env.setenv("GAD_CLIP_B32_WEIGHTS", "/nowhere/ViT-B-32.pt")
    with pytest.raises(ValueError, match="GAD_CLIP_L14_WEIGHTS, GAD_AESTHETIC_WEIGHTS"):
        M.scorer_settings({"clip_prompt": torch.ones(512)})
    clean_env.setenv("GAD_CLIP_L14_WEIGHTS", "/nowhere/ViT-L-14.pt")
    clean_env.setenv("GAD_AESTHETIC_WEIGHTS", "/nowhere/sa_0_4_vit_l_14_linear.pth")
    clean_env.delenv("GAD_VAE_DECODER_TS")
    with pytest.raises(ValueError, match="GAD_VAE_DECODER_TS"):
        M.scorer_settings({"clip_prompt": torch.ones(512)})
    clean_env.setenv("GAD_VAE_DECODER_TS", "/nowhere/decoder.pt")
    got = M.scorer_settings({"clip_prompt": torch.ones(512)})
    assert got["weights"]["GAD_CLIP_L14_WEIGHTS"] == "/nowhere/ViT-L-14.pt"


def test_main_refuses_before_it_loads_anything(clean_env, tmp_path):
    """the named errors come out of `main` itself, on a machine without a GPU: nothing has been built by then"""
    from text_to_image import compute_model_behaviors as M
    args = M.parse_args(["--reference_lora_dir", str(tmp_path), "--db", str(tmp_path / "db.jsonl"), "--exp_name", "x"])
    clean_env.setenv("GAD_SD_SCORER", "clip-seeded")
    with pytest.raises(ValueError, match="GAD_VAE_DECODER_TS"):
        M.main(args, backend=types.SimpleNamespace())
    clean_env.setenv("GAD_VAE_DECODER_TS", "/nowhere/decoder.pt")
    pe = tmp_path / "pe.pt"
    torch.save({"cond": torch.zeros(77, 8), "uncond": torch.zeros(77, 8)}, pe)
    args.prompt_embeds = str(pe)
    with pytest.raises(ValueError, match="'clip_prompt'"):
        M.main(args, backend=types.SimpleNamespace())


def test_rows_keep_the_stand_in_tag_when_nothing_is_configured(clean_env):
    from text_to_image import compute_model_behaviors as M
    args = M.parse_args(["--reference_lora_dir", "a", "--db", "b", "--exp_name", "c"])
    lists = {b: [0.5, 0.25] for b in M.BEHAVIOURS}
    row = M.assemble_row(args, lists, lists, [1], [2])
    assert row["feature_extractor"] == M.LatentScorer.TAG == "standin-latent-scorer-seed1234"
    assert M.assemble_row(args, lists, lists, [1], [2], tag="a;b;c")["feature_extractor"] == "a;b;c"
