"""GPU checks of the PNDM (PLMS) sampler: gad_plms_step against fp64 in every mode, its state and memory rules, the scheduler
free-running against tests/pndm_ref.py, the SD latent pipeline under either sampler, and --sampler on two entry points."""
import json
import math

import numpy as np
import pytest
import torch

import pndm_ref
from test_pndm_cpu import GOOD, REFUSALS, plms_call

pytestmark = pytest.mark.gpu
dev = torch.device("cuda:0")
U = 2.0 ** -24                                              # unit roundoff of fp32
NONE, SAVE, USE = 0, 1, 2

# name, weights on (e, h1, h2, h3), stored predictions read, push, saved mode: the five rows of the multistep table
MODES = [("first", (1.0, 0.0, 0.0, 0.0), 0, True, SAVE),
         ("second", (0.5, 0.5, 0.0, 0.0), 1, False, USE),
         ("two", (3 / 2, -1 / 2, 0.0, 0.0), 1, True, NONE),
         ("three", (23 / 12, -16 / 12, 5 / 12, 0.0), 2, True, NONE),
         ("four", (55 / 24, -59 / 24, 37 / 24, -9 / 24), 3, True, NONE)]
# fewer elements than one workgroup's 1024 with a ragged last wave; a few workgroups; more than the grid's 2048 x 256 float4
SHAPES = [(3, 324), (2, 4, 16, 16), (1, 2048 * 256 * 4 + 4 * 300)]


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def f64(t):
    return t.detach().cpu().double().numpy().reshape(-1)


def step_bound(cs, cm, w, xs, hist, eu, ec=None, g=0.0):
    """The per-element bound of one launch, in fp64 from its inputs: 16 u (|cs xs| + |cm| (sum |w_i h_i| + |w0| (|eps_u| +
    2 |g| (|eps_u| + |eps_c|)))).  16 covers the at most 14 roundings: three coefficients rounded once each, the guidance
    expression, four products and three sums, the two outer products and the subtraction (fma contraction only lowers it)."""
    ec = np.zeros_like(eu) if ec is None else ec
    mag = sum(abs(wi * h) for wi, h in zip(w[1:], hist)) + abs(w[0]) * (np.abs(eu) + 2 * abs(g) * (np.abs(eu) + np.abs(ec)))
    return 16 * U * (np.abs(cs * xs) + abs(cm) * mag)


@pytest.mark.parametrize("guided", [False, True], ids=["unguided", "guided"])
@pytest.mark.parametrize("shape", SHAPES, ids=["ragged_wave", "blocks", "grid_stride"])
def test_kernel_every_mode_against_fp64(shape, guided):
    """Teacher-forced: every mode gets fresh seeded operands; the launch is checked out of place against fp64 under the bound,
    then in place and once more out of place for equal bits, and every byte of scheduler state it must not touch is compared."""
    from gad import ops
    from gad.schedulers import plms_coefficients
    n = math.prod(shape)
    ac = pndm_ref.sd_alphas_cumprod()
    cs, cm = plms_coefficients(ac[501], ac[251])
    g = 7.5 if guided else None
    for k, (name, w, nh, push, mode) in enumerate(MODES):
        x = rnd(*shape, seed=10 + k).to(dev)
        eps = rnd(*((2 * shape[0],) + shape[1:]) if guided else shape, seed=20 + k).to(dev)
        ring0 = rnd(3, n, seed=30 + k).to(dev)
        saved0 = rnd(n, seed=40 + k).to(dev)
        slot = nh % 3                                        # nh == 3: the slot read as h3 is the one overwritten

        def run(out_is_x):
            ring, saved, xin = ring0.clone(), saved0.clone(), x.clone()
            out = ops.plms_step_raw(xin, eps, cs, cm, w, history=[ring[i] for i in range(nh)], push=ring[slot] if push else None,
                                    x_saved=saved if mode != NONE else None, saved_mode=mode, guidance=g,
                                    out=xin if out_is_x else None)
            assert (out.data_ptr() == xin.data_ptr()) == out_is_x
            if not out_is_x:
                assert torch.equal(xin, x), name             # out of place leaves the sample alone
            return out, ring, saved

        out, ring, saved = run(False)
        eu = f64(eps)[:n]
        ec = f64(eps)[n:] if guided else None
        e = eu + 7.5 * (ec - eu) if guided else eu
        hist = [f64(ring0[i]) for i in range(nh)]
        xs = f64(saved0) if mode == USE else f64(x)
        want = cs * xs - cm * (w[0] * e + sum(wi * h for wi, h in zip(w[1:], hist)))
        bound = step_bound(cs, cm, w, xs, hist, eu, ec, 7.5 if guided else 0.0)
        err = np.abs(f64(out) - want)
        print(f"{name} n={n} guided={guided}: max err / bound {np.max(err / bound):.3f}")
        assert np.all(err <= bound), (name, float(np.max(err / bound)))
        # state: the pushed slot holds e, the others and x_saved (outside the first step) keep their bits
        for i in range(3):
            if push and i == slot:
                if guided:                                   # three roundings of eps_u + g (eps_c - eps_u), g = 7.5 exact
                    assert np.all(np.abs(f64(ring[i]) - e) <= 4 * U * (np.abs(eu) + 2 * 7.5 * (np.abs(eu) + np.abs(ec)))), name
                else:
                    assert torch.equal(ring[i], eps.reshape(-1)), name
            else:
                assert torch.equal(ring[i], ring0[i]), (name, i)
        assert torch.equal(saved, x.reshape(-1) if mode == SAVE else saved0), name
        for again in (run(True), run(False)):                # in place, and a rerun: equal bits in the result and the state
            for got, first in zip(again, (out, ring, saved)):
                assert torch.equal(got.reshape(-1), first.reshape(-1)), name


def test_host_refusals_are_raised():
    """the C entry point's refusals (the table of the CPU test, before any HIP call) and the wrapper's, on device tensors"""
    from gad import _capi, ops
    lib = _capi.load()
    for bad, word in REFUSALS:
        assert plms_call(lib, dict(GOOD, **bad)) != 0 and word in lib.gad_last_error(), word
    x, e2 = torch.zeros(2, 8, device=dev), torch.zeros(4, 8, device=dev)
    w = (1.0, 0.0, 0.0, 0.0)
    with pytest.raises(_capi.GadError, match="32 .the doubled batch"):
        ops.plms_step_raw(x, x, 1.0, 0.1, w, guidance=7.5)
    with pytest.raises(_capi.GadError, match="16 .x's own"):
        ops.plms_step_raw(x, e2, 1.0, 0.1, w)
    with pytest.raises(_capi.GadError, match="3 weights"):
        ops.plms_step_raw(x, x, 1.0, 0.1, w[:3])
    with pytest.raises(_capi.GadError, match="h1 has 32 elements"):
        ops.plms_step_raw(x, x, 1.0, 0.1, (0.5, 0.5, 0.0, 0.0), history=[e2])
    with pytest.raises(_capi.GadError, match="push has 32 elements"):
        ops.plms_step_raw(x, x, 1.0, 0.1, w, push=e2)
    with pytest.raises(_capi.GadError, match="plms eps: expected a contiguous fp32"):
        ops.plms_step_raw(x, x.double(), 1.0, 0.1, w)
    with pytest.raises(_capi.GadError, match="x_prev aliases eps"):
        ops.plms_step_raw(x, e2, 1.0, 0.1, w, guidance=7.5, out=e2[:2])
    with pytest.raises(_capi.GadError, match="w1=0.5 with a null h1"):
        ops.plms_step_raw(x, x.clone(), 1.0, 0.1, (0.5, 0.5, 0.0, 0.0))
    with pytest.raises(_capi.GadError, match="cs=0"):
        ops.plms_step_raw(x, x.clone(), 0.0, 0.1, w)
    import gad
    sch = gad.sd_scheduler("pndm")
    with pytest.raises(ValueError, match="set_timesteps has not been called"):
        sch.step(x.clone(), 1, x)
    sch.set_timesteps(4)
    sch.step(x.clone(), 751, x)
    with pytest.raises(ValueError, match="another shape or device"):
        sch.step(e2.clone(), 501, e2)
    sch.set_timesteps(4)                                     # a new trajectory may have a new shape
    sch.step(e2.clone(), 751, e2)


def test_scheduler_free_running_against_the_restatement():
    """PNDMScheduler.step over n = 6: seven steps, six pushes, so the three-slot ring wraps.  The model is the closed form
    eps = 0.3 x + 0.1 sin(t / 1000), in fp32 torch ops on the device and in fp64 in the restatement.  Tolerance, from the
    coefficients alone: each step adds its own launch bound (step_bound, evaluated on the restatement's operands) and carries
    what it inherited through its cs - tol_{k+1} = cs_k tol_k + bound_k over the seven steps."""
    import gad
    sch = gad.sd_scheduler("pndm")
    ref = pndm_ref.PNDMRef(sch.alphas_cumprod.double().numpy())
    sch.set_timesteps(6)
    ref.set_timesteps(6)
    x = rnd(2, 4, 16, 16, seed=3).to(dev)
    xr = f64(x)
    tol = np.zeros_like(xr)
    for t in sch.timesteps.tolist():
        c = 0.1 * math.sin(t / 1000)
        x_next = sch.step(0.3 * x + c, t, x).prev_sample
        assert x_next.data_ptr() != x.data_ptr()
        er = 0.3 * xr + c
        xr = ref.step(er, t, xr)
        last = ref.last
        tol = last["cs"] * tol + step_bound(last["cs"], last["cm"], last["weights"], last["xs"], last["history"], er)
        err = np.abs(f64(x_next) - xr)
        print(f"t={t}: max err / tol {np.max(err / tol):.3f}")
        assert np.all(err <= tol), (t, float(np.max(err / tol)))
        x = x_next
    assert (sch.counter, sch.n_stored) == (7, 3)


def _small_pair():
    from test_gpu_sd import _pair
    return _pair()


def test_pipeline_pndm_matches_oracle_loop():
    """StableDiffusionLatentPipeline with the PLMS sampler on the small U-Net of test_gpu_sd against a loop of the oracle U-Net
    and the fp64 restatement, under that file's fp32 U-Net tolerance close(rtol=2e-4, atol=2e-4)"""
    import gad
    from test_gpu_sd import close
    ref, net = _small_pair()
    cond, uncond = rnd(2, 77, 96, seed=5), rnd(1, 77, 96, seed=6).expand(2, -1, -1).contiguous()
    sch = gad.sd_scheduler("pndm")
    pipe = gad.StableDiffusionLatentPipeline(net, sch)
    calls = []
    got = pipe(cond.to(dev), uncond.to(dev), num_inference_steps=6, guidance_scale=7.5, generator=torch.Generator().manual_seed(11),
               height=128, width=128, callback=lambda i, t, lat: calls.append((i, t, tuple(lat.shape)))).latents
    assert len(sch.timesteps) == 7 and sch.timesteps.tolist() == [831, 665, 665, 499, 333, 167, 1]
    assert calls == [(i, t, (2, 4, 16, 16)) for i, t in enumerate(sch.timesteps.tolist())]
    rs = pndm_ref.PNDMRef(sch.alphas_cumprod.double().numpy())
    rs.set_timesteps(6)
    x = torch.randn((2, 4, 16, 16), generator=torch.Generator().manual_seed(11)).double()
    with torch.no_grad():
        for t in rs.timesteps.tolist():
            xf = x.float()
            e = ref(torch.cat([xf, xf]), torch.tensor(t), torch.cat([uncond, cond])).sample.double()
            eu, ec = e.chunk(2)
            x = torch.from_numpy(rs.step((eu + 7.5 * (ec - eu)).numpy(), t, x.numpy()))
    close(got, x, rtol=2e-4, atol=2e-4)


def test_pipeline_ddim_issues_the_same_launches_as_before():
    """the default pipeline and sd_scheduler("ddim") against the loop the pipeline ran before it took a second sampler:
    equal bits"""
    import gad
    from gad import ops
    _, net = _small_pair()
    cond, uncond = rnd(2, 77, 96, seed=5).to(dev), rnd(1, 77, 96, seed=6).expand(2, -1, -1).contiguous().to(dev)
    kw = dict(num_inference_steps=4, guidance_scale=7.5, height=128, width=128)
    got = [gad.StableDiffusionLatentPipeline(net, *s)(cond, uncond, generator=torch.Generator().manual_seed(11), **kw).latents
           for s in ((), (gad.sd_scheduler("ddim"),))]
    sch = gad.DDIMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", clip_sample=False,
                            set_alpha_to_one=False, steps_offset=1)
    sch.set_timesteps(4)
    lat = torch.randn((2, 4, 16, 16), generator=torch.Generator().manual_seed(11), dtype=torch.float32).to(dev)
    x = ops.nchw_to_nhwc_raw((lat * sch.init_noise_sigma).contiguous())
    ctx = torch.cat([uncond, cond], 0).contiguous()
    t2 = torch.empty(4, device=dev, dtype=torch.int64)
    with torch.no_grad():
        for t in sch.timesteps.tolist():
            t2.fill_(t)
            eps = net.forward_nhwc(torch.cat([x, x], 0), t2, ctx)
            a_t, a_p = sch.step_coefficients(t)
            ops.cfg_ddim_step_raw(x, eps, 7.5, a_t, a_p, 0.0, out=x)
    want = ops.nhwc_to_nchw_raw(x)
    assert torch.equal(got[0], want) and torch.equal(got[1], want)


def _lora_dir(tmp_path, rank=4):
    """a LoRA directory and the base weights it belongs to, for the small U-Net"""
    import gad
    from test_gpu_sd import SMALL
    torch.manual_seed(0)
    net = gad.UNet2DConditionModel(**SMALL).to(dev)
    for i, p in enumerate(net.inject_lora(rank=rank)):
        with torch.no_grad():
            p.copy_(rnd(*p.shape, seed=50 + i, scale=0.05))
    net.save_attn_procs(str(tmp_path / "lora"))
    torch.save({k: v for k, v in net.state_dict().items() if "lora_layer" not in k}, tmp_path / "unet.pt")
    return str(tmp_path / "lora"), str(tmp_path / "unet.pt")


def test_model_behaviours_entry_point_with_pndm(tmp_path, monkeypatch):
    """compute_model_behaviors.py --sampler pndm --num_inference_steps 4 on the synthetic cache of
    test_sd_model_behaviours_entry_point (one LoRA trained for one step on it): the usual keys, finite values, a simple loss over
    the sampler's 5 timesteps, and latents that differ from the ddim run of the same seed"""
    import gad
    import pandas as pd
    from test_gpu_sd import SMALL
    from text_to_image import compute_model_behaviors as M
    from text_to_image import train_text_to_image_lora as T
    data = tmp_path / "artbench"
    T.synthetic_cache(str(data / "latent_cache.pt"), n=120, n_artists=10, res=128, ctx_dim=96)
    pd.DataFrame({"artist": sorted({f"artist_{i:03d}" for i in range(10)})}).to_csv(data / "post_impressionism_artists.csv", index=False)
    over = json.dumps(SMALL)
    assert T.main(T.parse_args(["--train_data_dir", str(data), "--output_dir", str(tmp_path / "out"), "--cls_key", "style", "--cls",
                                "post_impressionism", "--train_batch_size", "8", "--unet_overrides", over, "--seed", "42", "--rank", "4",
                                "--method", "retrain", "--max_train_steps", "1", "--learning_rate", "1e-3"]))
    full = tmp_path / "out" / "artbench_post_impressionism" / "retrain" / "models" / "full"
    seen = []
    real = gad.sd_simple_loss

    def spy(unet, scheduler, latents0, prompt_embeds, timesteps, **kw):
        seen.append(timesteps.tolist())
        return real(unet, scheduler, latents0, prompt_embeds, timesteps, **kw)
    monkeypatch.setattr(gad, "sd_simple_loss", spy)
    db = str(tmp_path / "behaviours.jsonl")
    for sampler in ("pndm", "ddim"):
        assert M.main(M.parse_args(["--reference_lora_dir", str(full), "--lora_dir", str(full), "--db", db, "--num_images", "1",
                                    "--resolution", "128", "--seed", "42", "--unet_overrides", over, "--num_inference_steps", "4",
                                    "--n_noises", "1", "--exp_name", f"full_{sampler}", "--sampler", sampler,
                                    "--img_dir", str(tmp_path / sampler)]))
    assert seen == [[751, 501, 501, 251, 1], [751, 501, 251, 1]]
    rows = [json.loads(l) for l in open(db)]
    assert [r["exp_name"] for r in rows] == ["full_pndm", "full_ddim"] and set(rows[0]) == set(rows[1]) and "sampler" not in rows[0]
    r = rows[0]
    for b in M.BEHAVIOURS:
        assert math.isfinite(r[f"generated_image_0_{b}"]) and f"generated_image_0_{b}_time" in r
    assert r["generated_image_0_simple_loss"] > 0 and r["generated_image_0_nrmse"] == 0.0       # the model against itself
    for k in ("aesthetic_score_0.5", "aesthetic_score_0.9", "clip_prompt_score_avg", "aesthetic_score_avg", "seed", "feature_extractor"):
        assert k in r
    lat = {s: torch.load(tmp_path / s / "latents_seed=42_sample_0.pt", weights_only=False)["sample"] for s in ("pndm", "ddim")}
    assert lat["pndm"].shape == lat["ddim"].shape == (1, 4, 16, 16) and torch.isfinite(lat["pndm"]).all()
    assert not torch.equal(lat["pndm"], lat["ddim"])


def test_journey_entry_point_with_pndm(tmp_path):
    """grad_text_to_image_lora.py --source generated_journey --sampler pndm: 8 steps make 9 callbacks, and the journey points
    index that sequence as the reference does (arange(1, 9, 9 // 3))"""
    import pandas as pd
    from test_gpu_sd import SMALL
    from text_to_image import grad_text_to_image_lora as G
    lora, weights = _lora_dir(tmp_path)
    d = 64
    path = G.main(G.parse_args(["--train_data_dir", str(tmp_path / "artbench"), "--output_dir", str(tmp_path / "out"), "--lora_dir", lora,
                                "--proj_dim", str(d), "--num_images", "1", "--num_journey_points", "3", "--num_inference_steps", "8",
                                "--resolution", "128", "--train_batch_size", "4", "--unet_weights", weights, "--unet_overrides",
                                json.dumps(SMALL), "--source", "generated_journey", "--f", "loss", "--sampler", "pndm"]))
    assert list(G.journey_points(9, 3)) == [1, 4, 7]
    emb = torch.load(path, weights_only=False)
    assert emb.shape == (3, d) and torch.isfinite(emb).all() and (emb.abs().sum(1) > 0).all()
    gdf = pd.read_csv(tmp_path / "out" / "artbench_post_impressionism" / "gradients" / "generated_journey" / "group.csv", index_col=0)
    assert list(gdf["step_idx"]) == [1, 4, 7] and list(gdf["generated_image_idx"]) == [0, 0, 0]
