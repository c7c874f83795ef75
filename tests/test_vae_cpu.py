"""Host side of the autoencoders (gad/vae.py): key grammar, parameter counts, refusals by name, the environment rules, the C
ABI's new symbols - and the YARDSTICK table the GPU bounds of tests/test_gpu_vae.py are multiples of: tests/vae_ref.py in fp32
on the CPU against itself in fp64, on the GPU tests' own inputs (maximum absolute error, outputs of magnitude 2-3).

    config                               this file measures      bound it asserts (the band an fp32 restatement lies in)
    tiny decoders / encoders (5 x 7)     0.7e-6 .. 1.9e-6        1e-7 .. 2e-5 (all model rows)
    SD VAE decoder, 8 x 8 -> 64 x 64     3.4e-6
    CelebA VQ decode, 8 x 8 -> 32 x 32   2.8e-6
    attention, d = 512                   1.2e-7 .. 2.7e-7        1e-8 .. 2e-6

The band is not a tolerance on the product: it only says the yardstick is a float32 rounding effect (above: eps x a few
hundred accumulated terms; below: not identically zero), so that "8 x the yardstick" means something."""
import math
import os
import re

import pytest
import torch

import vae_ref as R
from gad import _capi, vae

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def count(shapes):
    return sum(math.prod(s) for s in shapes.values())


# ---- key sets, shapes, parameter counts --------------------------------------------------------------------------------------
@pytest.mark.parametrize("preset,dec,enc,whole", [("SD_VAE", 49_490_179, 34_163_592, 83_653_863),
                                                  ("CELEBA_VQ", 32_960_771, 22_337_411, 55_322_782)])
def test_preset_parameter_counts(preset, dec, enc, whole):
    cfg = vae.PRESETS[preset]()
    assert count(vae.decoder_shapes(cfg)) == dec
    assert count(vae.encoder_shapes(cfg)) == enc
    assert count(vae.expected_shapes(cfg)) == whole


def test_presets_and_their_key_grammar():
    from src.ddpm_config import DDPMConfig
    sd, vq = vae.sd_vae_config(), vae.celeba_vq_config()
    assert (sd.kind, sd.block_out_channels, sd.layers_per_block, sd.latent_channels, sd.norm_num_groups, sd.scaling_factor) == \
        ("kl", (128, 256, 512, 512), 2, 4, 32, 0.18215)
    c = DDPMConfig.celeba_config["vqvae_config"]
    assert (vq.kind, list(vq.block_out_channels), vq.layers_per_block, vq.latent_channels, vq.num_vq_embeddings, vq.vq_embed_dim) == \
        ("vq", c["block_out_channels"], c["layers_per_block"], c["latent_channels"], c["num_vq_embeddings"], 3)
    ks = vae.expected_shapes(sd)
    assert ks["decoder.conv_in.weight"] == (512, 4, 3, 3) and ks["decoder.conv_out.weight"] == (3, 128, 3, 3)
    assert ks["encoder.conv_out.weight"] == (8, 512, 3, 3) and ks["quant_conv.weight"] == (8, 8, 1, 1)
    assert ks["post_quant_conv.weight"] == (4, 4, 1, 1)
    assert ks["decoder.up_blocks.2.resnets.0.conv_shortcut.weight"] == (256, 512, 1, 1)      # 512 -> 256 at the third up block
    assert "decoder.up_blocks.0.resnets.0.conv_shortcut.weight" not in ks
    assert "decoder.up_blocks.2.upsamplers.0.conv.weight" in ks and "decoder.up_blocks.3.upsamplers.0.conv.weight" not in ks
    assert "encoder.down_blocks.2.downsamplers.0.conv.weight" in ks and "encoder.down_blocks.3.downsamplers.0.conv.weight" not in ks
    assert "encoder.down_blocks.0.resnets.2.conv1.weight" not in ks and "decoder.up_blocks.0.resnets.2.conv1.weight" in ks
    assert ks["decoder.mid_block.attentions.0.to_out.0.weight"] == (512, 512)
    kv = vae.expected_shapes(vq)
    assert kv["quantize.embedding.weight"] == (8192, 3) and kv["encoder.conv_out.weight"] == (3, 512, 3, 3)
    assert kv["quant_conv.weight"] == (3, 3, 1, 1) and "decoder.up_blocks.3.resnets.0.conv1.weight" not in kv


def test_both_attention_grammars_load_to_identical_weights():
    cfg = R.TINY_KL
    sd = vae.seeded_state_dict(cfg, 1)
    old = {}
    for k, v in sd.items():
        for new, was in (("to_q", "query"), ("to_k", "key"), ("to_v", "value"), ("to_out.0", "proj_attn")):
            k = k.replace(f".attentions.0.{new}.", f".attentions.0.{was}.")
        old[k] = v
    assert any(".query." in k for k in old) and not any(".to_q." in k for k in old)
    a, b = vae.AutoencoderKL(cfg, sd), vae.AutoencoderKL(cfg, old)
    assert a.w.keys() == b.w.keys()
    for k in a.w:
        for x, y in zip(a.w[k], b.w[k]):
            assert torch.equal(x, y)
    q = a.w["decoder.mid_block.attentions.0.qkv"]
    assert tuple(q[0].shape) == (192, 64) and tuple(q[1].shape) == (192,)
    assert torch.equal(q[0][64:128], sd["decoder.mid_block.attentions.0.to_k.weight"])


def test_state_dicts_are_refused_by_key():
    cfg = R.TINY_VQ
    sd = vae.seeded_state_dict(cfg, 1)
    missing = {k: v for k, v in sd.items() if k != "quantize.embedding.weight"}
    with pytest.raises(KeyError, match="VQModel: missing key 'quantize.embedding.weight'"):
        vae.VQModel(cfg, missing)
    bad = dict(sd, **{"decoder.conv_out.bias": torch.zeros(4)})
    with pytest.raises(ValueError, match=re.escape("VQModel: 'decoder.conv_out.bias' has shape (4,), expected (3,)")):
        vae.VQModel(cfg, bad)
    extra = dict(sd, **{"loss.logvar": torch.zeros(())})
    with pytest.raises(KeyError, match="VQModel: unexpected key 'loss.logvar'"):
        vae.VQModel(cfg, extra)
    with pytest.raises(ValueError, match="kind 'vq', expected 'kl'"):
        vae.AutoencoderKL(cfg, sd)
    with pytest.raises(_capi.GadError, match="single attention head of 384 has no kernel"):
        vae.AutoencoderKL(R.cfg("kl", (64, 384), 1, 4, 32))
    with pytest.raises(_capi.GadError, match="VQModel: no weights loaded"):
        vae.VQModel(cfg).decode(torch.zeros(1, 3, 4, 4))


def test_constructors_tags_and_the_writable_scaling_factor(tmp_path):
    from safetensors.torch import save_file
    cfg = R.TINY_VQ
    sd = vae.seeded_state_dict(cfg, 7)
    m = vae.VQModel.seeded(cfg, 7)
    assert m.tag == "vqmodel-seeded7" and m.max_batch == 8 and m.config.scaling_factor == 0.18215
    m.config.scaling_factor = 1.0
    assert m.config.scaling_factor == 1.0 and cfg.scaling_factor == 0.18215         # the model's own copy
    torch.save(sd, tmp_path / "vq.pt")
    save_file(sd, str(tmp_path / "vq.safetensors"))
    a, b = vae.VQModel.from_file(tmp_path / "vq.pt", cfg), vae.VQModel.from_file(tmp_path / "vq.safetensors", cfg)
    assert re.fullmatch(r"vqmodel:vq\.pt:[0-9a-f]{12}", a.tag) and re.fullmatch(r"vqmodel:vq\.safetensors:[0-9a-f]{12}", b.tag)
    assert all(torch.equal(x, y) for k in a.w if k != "quantize.embedding" for x, y in zip(a.w[k], b.w[k]))
    assert torch.equal(a.w["quantize.embedding"], sd["quantize.embedding.weight"])
    kl = vae.AutoencoderKL.seeded(R.TINY_KL, 2)
    assert kl.tag == "autoencoder_kl-seeded2"
    w = kl.w["decoder.conv_in"][0]
    assert tuple(w.shape) == (64, 3, 3, 4)                                            # [Cout][KH][KW][Cin]


# ---- environment rules, pure host code ---------------------------------------------------------------------------------------
@pytest.fixture
def clean_env(monkeypatch):
    for v in ("GAD_VAE_DECODER_TS", "GAD_VAE_WEIGHTS", "GAD_VQVAE_WEIGHTS", "GAD_SD_SCORER", "GAD_CLIP_B32_WEIGHTS",
              "GAD_CLIP_L14_WEIGHTS", "GAD_AESTHETIC_WEIGHTS"):
        monkeypatch.delenv(v, raising=False)
    return monkeypatch


def test_sd_decoder_variables(clean_env):
    from text_to_image import baselines as B
    from text_to_image import compute_model_behaviors as M
    assert M.decoder_setting() is None and M.make_decoder(torch.device("cpu")) is None
    assert B.network_settings(["GAD_VAE_DECODER_TS"], None, "pixel") is None
    clean_env.setenv("GAD_VAE_WEIGHTS", "/x/vae.safetensors")
    assert M.decoder_setting() == ("GAD_VAE_WEIGHTS", "/x/vae.safetensors")
    assert M.scorer_settings(None) is None                                          # a decoder alone keeps the stand-in scorer
    assert B.network_settings(["GAD_VAE_DECODER_TS"], "/x/px.npy", "pixel") == {"GAD_VAE_DECODER_TS": "/x/vae.safetensors"}
    with pytest.raises(ValueError, match="not set: --train_pixels"):
        B.network_settings(["GAD_VAE_DECODER_TS"], None, "pixel")
    clean_env.setenv("GAD_SD_SCORER", "clip-seeded")
    assert M.scorer_settings({"clip_prompt": torch.ones(512)}) == {"weights": None}   # accepted where GAD_VAE_DECODER_TS is
    clean_env.setenv("GAD_VAE_DECODER_TS", "/x/decoder.pt")
    for call in (M.decoder_setting, lambda: M.scorer_settings(None), lambda: M.make_decoder(torch.device("cpu")),
                 lambda: B.network_settings(["GAD_VAE_DECODER_TS"], "/x/px.npy", "pixel")):
        with pytest.raises(ValueError, match="GAD_VAE_DECODER_TS and GAD_VAE_WEIGHTS are both set"):
            call()
    clean_env.delenv("GAD_VAE_WEIGHTS")
    assert M.decoder_setting() == ("GAD_VAE_DECODER_TS", "/x/decoder.pt")
    clean_env.delenv("GAD_VAE_DECODER_TS")
    with pytest.raises(ValueError, match="GAD_VAE_DECODER_TS"):                      # the refusal keeps naming the first variable
        M.scorer_settings({"clip_prompt": torch.ones(512)})


def test_main_refuses_both_decoder_variables_before_it_loads_anything(clean_env, tmp_path):
    import types
    from text_to_image import compute_model_behaviors as M
    args = M.parse_args(["--reference_lora_dir", str(tmp_path), "--db", str(tmp_path / "db.jsonl"), "--exp_name", "x"])
    clean_env.setenv("GAD_VAE_DECODER_TS", "/nowhere/decoder.pt")
    clean_env.setenv("GAD_VAE_WEIGHTS", "/nowhere/vae.safetensors")
    with pytest.raises(ValueError, match="both set"):
        M.main(args, backend=types.SimpleNamespace())


def test_celeba_vqvae_variable(clean_env, tmp_path):
    import types
    from src import diffusion_utils as DU
    assert DU.celeba_vqvae(types.SimpleNamespace(), "cpu") is None                  # unset: latent space, as before
    args = types.SimpleNamespace(dataset="celeba", precompute_stage=None, device="cpu")
    with pytest.raises(NotImplementedError, match="pass --precompute_stage reuse"):
        DU.build_pipeline(args, None, types.SimpleNamespace())
    clean_env.setenv("GAD_VQVAE_WEIGHTS", str(tmp_path / "vq.pt"))
    with pytest.raises(NotImplementedError, match="pass --precompute_stage reuse"):  # the variable does not lift that refusal
        DU.build_pipeline(args, None, types.SimpleNamespace())
    with pytest.raises(NotImplementedError, match="GAD_VQVAE_WEIGHTS is set, and this backend has no VQModel"):
        DU.celeba_vqvae(types.SimpleNamespace(), "cpu")
    cfg = vae.celeba_vq_config()
    cfg.block_out_channels, cfg.layers_per_block, cfg.norm_num_groups, cfg.num_vq_embeddings = (32, 64), 1, 8, 16
    torch.save(vae.seeded_state_dict(cfg, 1), tmp_path / "vq.pt")
    backend = types.SimpleNamespace(VQModel=type("VQ", (vae.VQModel,), {
        "from_file": classmethod(lambda cls, path, preset: vae.VQModel.from_file(path, cfg) if preset == "CELEBA_VQ" else None)}))
    vq = DU.celeba_vqvae(backend, "cpu")
    assert vq.config.scaling_factor == 1.0 and vq.tag.startswith("vqmodel:vq.pt:")
    assert DU.celeba_vqvae(backend, "cpu") is vq                                    # one object per file, device and process


# ---- C ABI -----------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "gad.h")).read()
    for name in ("gad_attention_fwd_d512", "gad_attention_d512_supported", "gad_vq_lookup"):
        assert re.search(rf"\b{name}\s*\(", header), name
        assert name in _capi.SIGNATURES
    lib = _capi.load()
    assert lib.gad_attention_d512_supported(512) == 1 and lib.gad_attention_d512_supported(256) == 0
    assert lib.gad_attention_supported(512) == 0 and lib.gad_attention_supported(256) == 1      # the existing query is unchanged
    assert lib.gad_vq_lookup(None, 3, None, 4, 8, 17, None, None, 3, None) == 1
    assert b"gad_vq_lookup: code dim D=17 is outside 1..16" in lib.gad_last_error()
    a = _capi.AttentionArgs()
    a.q = a.k = a.v = a.o = 16
    a.B = a.heads = a.Tq = a.Tk = 1
    a.d = a.ldq = a.ldk = a.ldv = a.ldo = 384
    import ctypes
    assert lib.gad_attention_fwd_d512(ctypes.byref(a), None) == 1                   # refused before any HIP call
    assert b"gad_attention_fwd_d512: head dim 384 is not 512" in lib.gad_last_error()


# ---- the yardstick table -----------------------------------------------------------------------------------------------------
def _yard(fn):
    return R.max_err(fn(torch.float32), fn(torch.float64))


def test_yardsticks_of_the_gpu_test_inputs():
    rows = {}
    for name in ("TINY_KL", "WIDE_KL", "TINY_VQ"):
        cfg = getattr(R, name)
        sd = vae.seeded_state_dict(cfg, 5)
        z, x = R.latent_input(cfg, B=2), R.image_input(cfg, B=2)
        kw = {} if cfg.kind == "kl" else {"force_not_quantize": True}
        rows[name + " decode"] = _yard(lambda dt: R.Net(sd, cfg, dt).decode(z, **kw))
        rows[name + " encode"] = _yard(lambda dt: R.Net(sd, cfg, dt).moments(x))
    for name, cfg in (("SD_VAE decode", R.SD_VAE), ("CELEBA_VQ decode", R.CELEBA_VQ)):
        sd = vae.seeded_state_dict(cfg, 5)
        z = R.latent_input(cfg, B=1, h=8, w=8)
        rows[name] = _yard(lambda dt: R.Net(sd, cfg, dt).decode(z))
    for k, v in rows.items():
        print(f"yardstick {k}: {v:.2e}")
        assert 1e-7 < v < 2e-5, (k, v)
    for B, Tq, Tk in R.ATTN_SHAPES[1:]:
        q, k, v = R.attention_inputs(B, Tq, Tk, 512)
        y = R.max_err(R.sdpa(q, k, v), R.sdpa(q.double(), k.double(), v.double()))
        print(f"yardstick attention d=512 B={B} Tq={Tq} Tk={Tk}: {y:.2e}")
        assert 1e-8 < y < 2e-6, y
    q, k, v = R.attention_inputs(1, 1, 1, 512)                                      # one key: o = v in any arithmetic
    assert R.max_err(R.sdpa(q, k, v), R.sdpa(q.double(), k.double(), v.double())) == 0.0


def test_reference_lookup_is_the_exact_form_with_ties_to_the_lowest_index():
    z, e = R.rnd(50, 3, seed=1), R.rnd(40, 3, seed=2)
    e[30] = e[4]
    z[0] = e[4]
    idx = R.vq_argmin(z, e)
    assert int(idx[0]) == 4 and not bool((idx == 30).any())
    want = ((z[:, None, :] - e[None]) ** 2).sum(-1).argmin(1)
    assert torch.equal(idx, want)
    cfg = R.TINY_VQ
    net = R.Net(vae.seeded_state_dict(cfg, 5), cfg, torch.float32)
    h = R.latent_input(cfg)
    i, zq = net.lookup(h)
    code = net.sd["quantize.embedding.weight"][i].permute(0, 3, 1, 2)
    assert torch.equal(zq, h + (code - h)) and tuple(i.shape) == (1, 5, 7)
