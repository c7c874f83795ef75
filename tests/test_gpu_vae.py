"""The autoencoders on the GPU: the two kernels of their own (gad_attention_fwd_d512, gad_vq_lookup), whole models against
tests/vae_ref.py in fp64, and the pipelines they are wired into.

Bounds.  Every error is a maximum absolute difference against fp64 on O(1) data, and every bound is a multiple of the
YARDSTICK for the same inputs: the error the fp32 CPU run of the same restatement makes (tests/test_vae_cpu.py records the
table).  Whole models: 8 x the yardstick (the project's convention, tests/test_gpu_vit.py: MFMA summation order).  Attention
at d = 512: m x the yardstick with m = max(8, 2 r), r the ratio the EXISTING wide kernel reaches at d = 256 against its own
yardstick on the same seeds (its softmax runs in the exp2 domain; the new instance is held to the same error ratio, twice).

Measured on an MI355X, (B, Tq, Tk): err / yardstick of the d = 512 kernel | r of the d = 256 wide kernel | bound m
  (1, 1, 1)       0 (exact)   | 0 (exact) | 8        (2, 64, 64)     0.96 | 1.01 | 8        (1, 33, 95)   0.83 | 1.15 | 8
  (2, 130, 70)    0.86        | 0.80      | 8        (1, 300, 700)   2.72 | 3.05 | 8
Whole models, err / yardstick: tiny decoders and encoders 0.8-2.0, the SD decoder (8 x 8 -> 64 x 64) 1.15, the CelebA VQ decode
1.30 (0.98 unquantised), the mid-block attention block at 512 2.36 fused (8 x 32 x 64) and 0.92 on three launches (profiles/vae_ab.txt; every test prints its
figures before it asserts)."""
import math

import pytest
import torch

import vae_ref as R

pytestmark = pytest.mark.gpu
dev = torch.device("cuda:0")


# ---- attention at d = 512 -----------------------------------------------------------------------------------------------
def _fwd512(q, k, v):
    from gad import ops
    B, Tq, d = q.shape
    return ops.attention_fwd_d512_raw(q, k, v, B, 1, Tq, k.shape[1], d, d, d, d, need_lse=True)


def _ratio(got, q, k, v):
    """(error of `got` against fp64) / (error of the fp32 CPU restatement against fp64)"""
    want = R.sdpa(q.double(), k.double(), v.double())
    yard = R.max_err(R.sdpa(q, k, v), want)
    err = R.max_err(got, want)
    if yard == 0.0:                 # a single key: the softmax is exactly 1 and o = v in any arithmetic
        return (0.0 if err == 0.0 else math.inf), yard
    return err / yard, yard


@pytest.mark.parametrize("B,Tq,Tk", R.ATTN_SHAPES)
def test_attention_d512_vs_fp64_within_the_wide_kernels_error_ratio(B, Tq, Tk):
    from gad import ops
    q, k, v = R.attention_inputs(B, Tq, Tk, 512)
    o, lse = _fwd512(q.to(dev), k.to(dev), v.to(dev))
    ratio, yard = _ratio(o, q, k, v)
    q2, k2, v2 = R.attention_inputs(B, Tq, Tk, 256)
    with torch.no_grad():
        o2 = ops.attention_fwd_raw(q2.to(dev), k2.to(dev), v2.to(dev), B, 1, Tq, Tk, 256, 256, 256, 256, need_lse=False)[0]
    r, yard2 = _ratio(o2, q2, k2, v2)
    m = max(8.0, 2.0 * r)
    print(f"attention d=512 B={B} Tq={Tq} Tk={Tk}: err/yardstick {ratio:.2f} (yardstick {yard:.2e}); d=256 wide kernel r {r:.2f} "
          f"(yardstick {yard2:.2e}); bound m = {m:.2f}")
    assert ratio <= m, (ratio, m)
    # lse[b][0][q] = log2(sum_k exp2(log2(e) * scale * q.k))
    s = (q.double() @ k.double().transpose(1, 2)) / math.sqrt(512)
    want_lse = torch.logsumexp(s, dim=-1) / math.log(2.0)
    assert (lse.cpu().double()[:, 0] - want_lse).abs().max().item() < 1e-4


def test_attention_d512_reads_q_k_v_in_place_from_one_projection():
    """q | k | v as column blocks of a [B*T, 1536] projection output: bit-equal to separate tensors"""
    from gad import ops
    B, T, C = 2, 70, 512
    qkv = R.rnd(B * T, 3 * C, seed=7, scale=0.6).to(dev)
    q, k, v = qkv[:, 0:C], qkv[:, C:2 * C], qkv[:, 2 * C:]
    fused = ops.attention_fwd_d512_raw(q, k, v, B, 1, T, T, C, 3 * C, 3 * C, 3 * C)[0]
    sq, sk, sv = (t.reshape(B, T, C).contiguous() for t in (q, k, v))
    assert torch.equal(fused, _fwd512(sq, sk, sv)[0])
    want = R.sdpa(sq.cpu().double(), sk.cpu().double(), sv.cpu().double())
    assert R.max_err(fused, want) < 3e-5


def test_attention_d512_late_dominant_key_takes_the_rescale_branch():
    q, k, v = R.late_key_inputs(512)
    o = _fwd512(q.to(dev), k.to(dev), v.to(dev))[0]
    want = R.sdpa(q.double(), k.double(), v.double())
    # query 17's row is one key's value row to ~e^-40: the same 5e-5 the existing kernels' rescale test allows
    assert R.max_err(o, want) < 5e-5
    assert R.max_err(o[0, 17], v[0, 200].double()) < 5e-5


def test_attention_d512_is_bit_reproducible_and_leaves_no_score_tensor():
    B, T = 2, 1024
    q, k, v = (t.to(dev) for t in R.attention_inputs(B, T, T, 512))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    a = _fwd512(q, k, v)[0]
    peak = torch.cuda.max_memory_allocated(dev) - base
    b = _fwd512(q, k, v)[0]
    assert torch.equal(a, b)
    assert peak < 4 * B * T * T, peak


def test_attention_refusals_name_the_head_dim():
    from gad import _capi, ops
    assert ops.attention_d512_ok(512) and not ops.attention_d512_ok(513) and not ops.attention_d512_ok(8)
    for d in (513, 8):
        q = torch.zeros(1, 4, d, device=dev)
        with pytest.raises(_capi.GadError, match=rf"gad_attention_fwd_d512: head dim {d}"):
            ops.attention_fwd_d512_raw(q, q, q, 1, 1, 4, 4, d, d, d, d)
    q = torch.zeros(1, 4, 257, device=dev)
    with pytest.raises(_capi.GadError, match="gad_attention_fwd: head dim 257 is outside 1..256"):
        ops.attention_fwd_raw(q, q, q, 1, 1, 4, 4, 257, 257, 257, 257, need_lse=False)
    assert not ops.fused_attention_ok(512)


# ---- codebook lookup --------------------------------------------------------------------------------------------------------
LOOKUP_SHAPES = [(4096, 8192, 3), (126, 8192, 3), (1000, 300, 3), (513, 8192, 4), (5, 1, 16)]      # n, K, D


@pytest.mark.parametrize("n,K,D", LOOKUP_SHAPES)
def test_vq_lookup_equals_the_fp64_argmin(n, K, D):
    from gad import ops
    z, e = R.rnd(n, D, seed=21), R.rnd(K, D, seed=22)
    gap = R.vq_relative_gap(z.double(), e.double()).min().item()
    assert gap > 1e-5, gap                                     # precondition: no row is a near tie in fp64
    want = R.vq_argmin(z.double(), e.double())
    idx, zq = ops.vq_lookup_raw(z.to(dev), e.to(dev))
    assert idx.dtype == torch.int32 and torch.equal(idx.cpu().long(), want)
    assert torch.equal(zq.cpu(), z + (e[want] - z))


def test_vq_lookup_duplicate_codes_give_the_lower_index():
    from gad import ops
    z, e = R.rnd(300, 3, seed=23), R.rnd(5000, 3, seed=24)
    e[7] = e[3]
    e[4500:] = e[:500]                                         # the second chunk of the codebook repeats codes of the first
    idx = ops.vq_lookup_raw(z.to(dev), e.to(dev))[0].cpu().long()
    want = R.vq_argmin(z, e)                                   # fp32, exact form, first of equal minima
    assert torch.equal(idx, want) and int(idx.max()) < 4500 and not bool((idx == 7).any())
    z[0] = e[3]                                                # distance exactly 0 to codes 3 and 7
    assert int(ops.vq_lookup_raw(z.to(dev), e.to(dev))[0][0]) == 3


def test_vq_lookup_reads_strided_rows_in_place():
    from gad import ops
    wide = R.rnd(200, 8, seed=25).to(dev)
    e = R.rnd(300, 3, seed=26).to(dev)
    idx, zq = ops.vq_lookup_raw(wide[:, 2:5], e)               # ldz = 8 > D = 3
    idx2, zq2 = ops.vq_lookup_raw(wide[:, 2:5].contiguous(), e)
    assert torch.equal(idx, idx2) and torch.equal(zq, zq2)


def test_vq_lookup_nan_row_disturbs_no_other_row():
    from gad import ops
    z, e = R.rnd(130, 3, seed=27), R.rnd(9000, 3, seed=28)
    clean = ops.vq_lookup_raw(z.to(dev), e.to(dev))
    z2 = z.clone()
    z2[64, 1] = float("nan")
    idx, zq = ops.vq_lookup_raw(z2.to(dev), e.to(dev))
    keep = torch.arange(130) != 64
    assert 0 <= int(idx[64]) < 9000
    assert torch.equal(idx.cpu()[keep], clean[0].cpu()[keep]) and torch.equal(zq.cpu()[keep], clean[1].cpu()[keep])


def test_vq_lookup_refusals_name_the_argument():
    from gad import _capi, ops
    with pytest.raises(_capi.GadError, match="gad_vq_lookup: code dim D=17"):
        ops.vq_lookup_raw(torch.zeros(4, 17, device=dev), torch.zeros(8, 17, device=dev))
    with pytest.raises(_capi.GadError, match="gad_vq_lookup: codebook size K=0"):
        ops.vq_lookup_raw(torch.zeros(4, 3, device=dev), torch.zeros(0, 3, device=dev))


# ---- whole models against tests/vae_ref.py in fp64 -----------------------------------------------------------------------------
def _state_dict(cfg, seed=5):
    from gad import vae
    return vae.seeded_state_dict(cfg, seed)


def _bound(name, fn, got):
    """got against fn(float64), within 8 x what fn(float32) on the CPU is off by"""
    want = fn(torch.float64)
    yard = R.max_err(fn(torch.float32), want)
    err = R.max_err(got, want)
    print(f"{name}: err {err:.2e}, yardstick {yard:.2e}, ratio {err / yard:.2f}, output max {want.abs().max().item():.2f}")
    assert tuple(got.shape) == tuple(want.shape)
    assert err <= 8 * yard, (name, err, yard)


@pytest.mark.parametrize("name", ["TINY_KL", "WIDE_KL", "TINY_VQ"])
def test_decoder_and_encoder_on_odd_maps(name):
    """boc (32, 64): the mid block's head of 64 runs gad_attention_fwd; boc (64, 512): the head of 512, at these sizes on its
    three-launch side (the fused side: test_wide_mid_block_routes_by_grid...).  Latent 5 x 7, image 10 x 14: odd, non-square,
    no multiple of any tile."""
    from gad import vae
    cfg = getattr(R, name)
    sd = _state_dict(cfg)
    cls = vae.AutoencoderKL if cfg.kind == "kl" else vae.VQModel
    m = cls(cfg, sd).to(dev)
    z, x = R.latent_input(cfg, B=2), R.image_input(cfg, B=2)
    kw = {} if cfg.kind == "kl" else {"force_not_quantize": True}
    _bound(f"{name} decode", lambda dt: R.Net(sd, cfg, dt).decode(z, **kw), m.decode(z.to(dev), **kw).sample)
    _bound(f"{name} encode", lambda dt: R.Net(sd, cfg, dt).moments(x), m.encode_moments(x.to(dev)))
    enc = m.encode(x.to(dev))
    if cfg.kind == "vq":                                       # not quantised; a 1-tuple without return_dict (encode(x, False)[0])
        assert torch.equal(enc.latents, m.encode(x.to(dev), False)[0]) and tuple(enc.latents.shape) == (2, 3, 5, 7)
        idx, _ = m.lookup(ops_nhwc(z.to(dev)))
        want_idx, _ = R.Net(sd, cfg, torch.float64).lookup(z.double())
        assert torch.equal(idx.cpu().long(), want_idx)
        _bound(f"{name} decode with lookup", lambda dt: R.Net(sd, cfg, dt).decode(z), m.decode(z.to(dev)).sample)


def ops_nhwc(x):
    from gad import ops
    return ops.nchw_to_nhwc_raw(x.contiguous())


def test_wide_mid_block_routes_by_grid_and_both_routes_meet_the_bound(monkeypatch):
    """One head of 512: gad_attention_fwd_d512 from one workgroup per CU (256) upwards, the three-launch route below - the
    shapes profiles/vae_ab.txt measured either side of.  The whole attention block (GroupNorm, fused q | k | v projection read
    in place, attention, out-projection + residual) against fp64 on each side."""
    from gad import ops, vae
    assert vae.d512_route(8, 2048) == "fused" and vae.d512_route(4, 4096) == "fused" and vae.d512_route(1, 16321) == "fused"
    assert vae.d512_route(8, 1024) == "three-launch" and vae.d512_route(1, 4096) == "three-launch"
    assert vae.d512_route(8, 2040) == "fused" and vae.d512_route(8, 1984) == "three-launch"      # 32 / 31 blocks of 64
    cfg = R.WIDE_KL
    sd = _state_dict(cfg)
    m = vae.AutoencoderKL(cfg, sd).to(dev)
    calls = []
    real = ops.attention_fwd_d512_raw
    monkeypatch.setattr(ops, "attention_fwd_d512_raw", lambda *a, **kw: calls.append(a[3:7]) or real(*a, **kw))
    p = "decoder.mid_block.attentions.0."
    for shape, fused in (((8, 512, 32, 64), True), ((2, 512, 9, 11), False)):
        x = R.rnd(*shape, seed=3)
        del calls[:]
        got = ops.nhwc_to_nchw_raw(m._attention(p, ops_nhwc(x.to(dev))))
        assert bool(calls) == fused, (shape, calls)
        _bound(f"mid-block attention at 512, {shape}, {'fused' if fused else 'three-launch'}",
               lambda dt: R.Net(sd, cfg, dt).attention(p, x.to(dt)), got)


def test_full_width_sd_decoder_on_one_latent():
    from gad import vae
    cfg = R.SD_VAE
    sd = _state_dict(cfg)
    m = vae.AutoencoderKL(cfg, sd).to(dev)
    z = R.latent_input(cfg, B=1, h=8, w=8)
    got = m.decode(z.to(dev)).sample
    assert tuple(got.shape) == (1, 3, 64, 64)
    _bound("SD VAE decode 8x8 -> 64x64", lambda dt: R.Net(sd, cfg, dt).decode(z), got)


def test_full_width_vq_decode_with_lookup():
    from gad import vae
    cfg = R.CELEBA_VQ
    sd = _state_dict(cfg)
    m = vae.VQModel(cfg, sd).to(dev)
    z = R.latent_input(cfg, B=1, h=8, w=8)
    ref64 = R.Net(sd, cfg, torch.float64)
    gap = R.vq_relative_gap(z.double().permute(0, 2, 3, 1).reshape(-1, 3), ref64.sd["quantize.embedding.weight"]).min().item()
    assert gap > 1e-5, gap
    idx, _ = m.lookup(ops_nhwc(z.to(dev)))
    assert torch.equal(idx.cpu().long(), ref64.lookup(z.double())[0])
    _bound("CelebA VQ decode 8x8 -> 32x32", lambda dt: R.Net(sd, cfg, dt).decode(z), m.decode(z.to(dev)).sample)
    _bound("CelebA VQ decode, force_not_quantize", lambda dt: R.Net(sd, cfg, dt).decode(z, force_not_quantize=True),
           m.decode(z.to(dev), force_not_quantize=True).sample)


def test_max_batch_chunks_three_images_by_two():
    from gad import vae
    cfg = R.TINY_KL
    sd = _state_dict(cfg)
    m = vae.AutoencoderKL(cfg, sd).to(dev)
    m.max_batch = 2
    z = R.latent_input(cfg, B=3)
    got = m.decode(z.to(dev)).sample
    assert tuple(got.shape) == (3, 3, 10, 14)
    _bound("max_batch = 2 over 3 images", lambda dt: R.Net(sd, cfg, dt).decode(z), got)
    assert isinstance(m.decode(z.to(dev), return_dict=False), tuple)


def test_kl_latent_dist_mean_logvar_mode_sample_and_clamp():
    from gad import vae
    cfg = R.TINY_KL
    sd = _state_dict(cfg)
    sd["quant_conv.bias"][2 * cfg.latent_channels - 1] = 40.0           # the last logvar channel leaves [-30, 20] upwards
    sd["quant_conv.bias"][cfg.latent_channels] = -50.0                  # the first one downwards
    m = vae.AutoencoderKL(cfg, sd).to(dev)
    x = R.image_input(cfg, B=2)
    dist = m.encode(x.to(dev)).latent_dist
    L = cfg.latent_channels

    def mean(dt):
        return R.Net(sd, cfg, dt).moments(x)[:, :L]

    def logvar(dt):
        return R.Net(sd, cfg, dt).moments(x)[:, L:].clamp(-30.0, 20.0)
    _bound("latent_dist.mean", mean, dist.mean)
    _bound("latent_dist.logvar", logvar, dist.logvar)
    assert bool((dist.logvar[:, -1] == 20.0).all()) and bool((dist.logvar[:, 0] == -30.0).all())
    assert not bool((dist.logvar[:, 1:-1].abs() >= 20.0).any())
    assert dist.mode() is dist.mean
    noise = torch.randn(dist.mean.shape, generator=torch.Generator().manual_seed(9)).to(dev)
    got = dist.sample(torch.Generator().manual_seed(9))
    assert torch.equal(got, dist.mean + torch.exp(0.5 * dist.logvar) * noise)
    assert torch.equal(m.encode(x.to(dev), return_dict=False)[0].mean, dist.mean)


# ---- pipelines ------------------------------------------------------------------------------------------------------------
PIPE_VQ = R.cfg("vq", (32, 32, 64), 1, 3, 8, K=64)             # three blocks: 4x the latent side, as CelebA's 64 -> 256


def _tiny_ldm(vq):
    import gad
    from src.ddpm_config import DDPMConfig
    ucfg = dict(DDPMConfig.celeba_config["unet_config"], block_out_channels=[32, 64, 64, 64], attention_head_dim=8,
                norm_num_groups=8, sample_size=8)
    sc = {k: v for k, v in DDPMConfig.celeba_config["scheduler_config"].items() if not k.startswith("_")}
    torch.manual_seed(0)
    unet = gad.UNet2DModel(**ucfg).to(dev).eval()
    return gad.LDMPipeline(unet, vq, gad.DDIMScheduler(**sc))


def test_ldm_pipeline_decodes_through_the_vqmodel():
    import gad
    vq = gad.VQModel.seeded(PIPE_VQ, 3).to(dev)
    vq.config.scaling_factor = 1.0
    pipe = _tiny_ldm(vq)
    img = pipe(batch_size=2, num_inference_steps=3, output_type="numpy", generator=torch.Generator().manual_seed(1)).images
    assert img.shape == (2, 32, 32, 3) and img.min() >= 0.0 and img.max() <= 1.0 and img.std() > 0.0
    assert pipe.decoder.tag == vq.tag == "vqmodel-seeded3"


def test_generate_images_decodes_each_fused_group():
    """generate_images keeps the fused sampler on the latents; its output is the pipeline's decode of those latents, through
    the uint8 round trip"""
    import gad
    from types import SimpleNamespace
    from gad import ops
    from gad.coalition import FusedSampler, _drain
    from src.diffusion_utils import _fused_sampler_for, generate_images
    vq = gad.VQModel.seeded(PIPE_VQ, 3).to(dev)
    vq.config.scaling_factor = 1.0
    pipe = _tiny_ldm(vq)
    assert _fused_sampler_for(pipe, 4, 32).decode is not None
    got = generate_images(SimpleNamespace(batch_size=4, n_samples=10, num_inference_steps=3), pipe)
    fs = FusedSampler(pipe.unet, pipe.scheduler, 4, 32)
    lat = _drain(fs.latent_steps(fs.initial_noise([0, 1, 2], [4, 4, 2]), 3))
    with torch.no_grad():
        img = ops.to_image01_raw(pipe._decode(lat))
        want = img.mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8).permute(0, 3, 1, 2).float().div_(255)
    assert tuple(got.shape) == (10, 3, 32, 32) and torch.equal(got, want)
    assert torch.equal((got * 255).round() / 255, got)
    # no decode argument: the sampler's output is what it was
    plain = FusedSampler(pipe.unet, pipe.scheduler, 4, 32).generate(10, 3)
    assert tuple(plain.shape) == (10, 3, 8, 8)


def test_sd_decoder_object_has_the_scripted_decoders_protocol(tmp_path, monkeypatch):
    from safetensors.torch import save_file
    from gad import vae
    from text_to_image import compute_model_behaviors as cmb
    cfg = R.TINY_KL
    path = tmp_path / "vae.safetensors"
    save_file(_state_dict(cfg), str(path))
    for v in ("GAD_VAE_DECODER_TS", "GAD_VAE_WEIGHTS"):
        monkeypatch.delenv(v, raising=False)
    assert cmb.make_decoder(dev) is None
    dec = cmb.HipDecoder(str(path), dev, preset=vae.make_config("kl", (32, 64), 1, 4, 8))
    lat = R.latent_input(cfg, B=1, h=6, w=6).to(dev)
    u8, img = dec(lat)
    assert u8.dtype.name == "uint8" and u8.shape == (12, 12, 3)
    assert tuple(img.shape) == (1, 3, 12, 12) and torch.equal((img * 255).round() / 255, img)
    assert torch.equal(img[0].permute(1, 2, 0).mul(255).round().to(torch.uint8).cpu(), torch.from_numpy(u8))
    assert dec.tag.startswith("autoencoder_kl:vae.safetensors:")
    want = R.Net(_state_dict(cfg), cfg, torch.float64).decode(lat.cpu().double() / cmb.VAE_SCALING)
    assert (img.cpu().double() - (want / 2 + 0.5).clamp(0, 1)).abs().max().item() <= 0.5 / 255 + 1e-4


def test_celeba_unlearn_row_names_the_decoder(tmp_path, monkeypatch):
    """GAD_VQVAE_WEIGHTS: the CelebA row's diversity is measured on decoded samples against decoded reference latents, and its
    tag says so"""
    import json
    import os
    import pandas as pd
    import src.constants as constants
    from gad import vae
    from src.ddpm_config import DDPMConfig
    cfg = {**DDPMConfig.celeba_config}
    cfg["unet_config"] = dict(cfg["unet_config"], block_out_channels=[32, 64, 64, 64], attention_head_dim=8,
                              norm_num_groups=8, sample_size=8)
    cfg["vqvae_config"] = dict(cfg["vqvae_config"], block_out_channels=[32, 32, 64], layers_per_block=1, norm_num_groups=8,
                               num_vq_embeddings=64)
    cfg["n_samples"] = 4
    cfg["batch_size"] = 8
    for k in ("training_steps", "ckpt_freq", "sample_freq"):
        cfg[k] = dict(cfg[k], retrain=2)
    monkeypatch.setattr(DDPMConfig, "celeba_config", cfg)
    vq_path = tmp_path / "vqvae.pt"
    torch.save(vae.seeded_state_dict(vae.celeba_vq_config(), 3), vq_path)
    root = tmp_path / "datasets" / "celeba_hq_256_50_resized"
    root.mkdir(parents=True)
    names = [f"{i:05d}.jpg" for i in range(40)]
    pd.DataFrame({"filename": names, "celeb": [i % 4 for i in range(40)]}).to_csv(root / "labels.csv", index=False)
    g = torch.Generator().manual_seed(0)
    torch.save({n: torch.randn(3, 8, 8, generator=g) * 0.5 + 0.2 * (i % 4) for i, n in enumerate(names)}, tmp_path / "vqvae_output.pt")
    monkeypatch.setenv("GAD_DATA", "real")
    monkeypatch.setenv("GAD_LATENTS", str(tmp_path / "vqvae_output.pt"))
    monkeypatch.setenv("GAD_VQVAE_WEIGHTS", str(vq_path))
    monkeypatch.setattr(constants, "DATASET_DIR", str(tmp_path / "datasets"))
    from unconditional_generation import main as train_main
    from unconditional_generation import unlearn as unlearn_main
    out, db = str(tmp_path / "res"), str(tmp_path / "db.jsonl")
    a = train_main.parse_args(["--dataset", "celeba", "--method", "retrain", "--outdir", out, "--precompute_stage", "reuse",
                               "--num_inference_steps", "3", "--log_freq", "1"])
    assert train_main.main(a)
    mdir = os.path.join(out, "celeba", "retrain", "models", "full")
    ck = torch.load(os.path.join(mdir, "ckpt_steps_00000002.pt"), weights_only=False)
    pdir = os.path.join(out, "celeba", "pruned", "models", "pruner=magnitude_pruning_ratio=0.3_threshold=0.05")
    os.makedirs(pdir)
    torch.save({"unet": ck["unet"], "unet_config": ck["unet_config"]}, os.path.join(pdir, "ckpt_steps_00000000.pt"))
    u = unlearn_main.parse_args(["--dataset", "celeba", "--method", "gd", "--removal_dist", "shapley", "--removal_seed", "2",
                                 "--load", mdir, "--outdir", out, "--db", db, "--gd_steps", "2", "--n_samples", "12",
                                 "--batch_size", "6", "--num_inference_steps", "3", "--model_behavior", "global",
                                 "--precompute_stage", "reuse"])
    assert unlearn_main.main(u)
    row = json.loads(open(db).readline())
    assert ";dec=vqmodel:vqvae.pt:" in row["feature_extractor"]
    assert len(row["cluster_count"]) == 20 and sum(row["cluster_count"]) == 12
