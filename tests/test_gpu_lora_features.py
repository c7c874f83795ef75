"""GPU tests of the SD LoRA gradient features: the segmented token-axis contraction gad_hgemm_tn_seg (csrc/half.hip) against fp64
of the same bf16-rounded operands, its independence of S / determinism / guard bands, the per-sample features of a small SD U-Net
(gad.trak.lora_gradient_features) against per-sample autograd gradients of the oracle, and the kept scripts end to end.

Tolerances: the kernel bar is test_gpu_half.py::test_hgemm_tn's, applied per segment: 2e-5 sqrt(L) max(1, |want|max), twice that
after an accumulate with alpha 0.5."""
import math
import os

import numpy as np
import pytest
import torch

from test_gpu_guards import POISON, guarded
from test_gpu_half import hb, rnd

pytestmark = pytest.mark.gpu
dev = torch.device("cuda:0")
BF = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "group-attribution-for-diffusion-models_amd")


def _operands(S, L, M, N, seed=1):
    """bf16 operands [S L][M8] / [S L][N8] (zero pad columns) on the device + their fp64 values"""
    M8, N8 = (M + 7) // 8 * 8, (N + 7) // 8 * 8
    a, b = torch.zeros(S * L, M8), torch.zeros(S * L, N8)
    a[:, :M], b[:, :N] = rnd(S * L, M, seed=seed), rnd(S * L, N, seed=seed + 1)
    ah, ad = hb(a)
    bh, bd = hb(b)
    return ah, bh, ad[:, :M], bd[:, :N]


def _want(ad, bd, S, L):
    return torch.stack([ad[s * L:(s + 1) * L].T @ bd[s * L:(s + 1) * L] for s in range(S)])


def _windows(buf, S, M, N, ldc, stride, off=0):
    """[S][M][N] view of the S output windows of a flat fp32 buffer"""
    return torch.as_strided(buf, (S, M, N), (stride, ldc, 1), off)


SEG = [  # S, L, M, N, ldc - N, stride - M * ldc, splitk_hint
    (4, 128, 128, 128, 0, 0, 0),            # L a multiple of the 64-row K step
    (8, 256, 320, 256, 0, 0, 0),
    (16, 77, 768, 256, 0, 0, 0),            # the cross-attention context
    (5, 154, 256, 768, 0, 8, 0),
    (64, 16, 1280, 256, 0, 0, 0),           # deepest level: one K step, mostly padding; S = 64
    (3, 1000, 320, 256, 0, 0, 0),           # split along the rows by the plan (16 steps -> 4 slices)
    (1, 1000, 256, 320, 0, 0, 0),           # S = 1
    (6, 200, 6, 72, 0, 0, 0),               # M not a multiple of 8
    (3, 130, 100, 260, 0, 4, 0),            # M, N not multiples of 128
    (4, 77, 37, 21, 3, 5, 0),               # nothing aligned: scalar stores, ldc gap, odd segment stride
    (4, 300, 264, 8, 8, 16, 3),             # forced split, ldc gap
    (4, 64, 320, 256, 0, 10_000_000, 0),    # c_seg_stride much larger than M * ldc (40 MB between segments)
    (2, 640, 200, 136, 4, 2_000_003, 2),    # forced split, far and odd stride: scalar reduce
]


@pytest.mark.parametrize("S,L,M,N,gap,far,sk", SEG)
def test_hgemm_tn_seg(S, L, M, N, gap, far, sk):
    """every segment against fp64, overwrite then accumulate; everything outside the S windows (the ldc - N gap, the space between
    segments, bands before and after) keeps its poison; S = 1 also equals gad_hgemm_tn within the same bar"""
    from gad import half, ops
    ah, bh, ad, bd = _operands(S, L, M, N)
    want = _want(ad, bd, S, L)
    ldc, stride = N + gap, M * (N + gap) + far
    lead = 1024
    total = lead + (S - 1) * stride + M * ldc + 1024
    poison = torch.tensor([POISON * 0x01010101], dtype=torch.int32).view(torch.float32).item()
    buf = torch.full((total,), poison, device=dev)
    out = _windows(buf, S, M, N, ldc, stride, lead)
    split = sk > 1 or (sk == 0 and (L + 63) // 64 >= 8)          # the plan: slices of at least 256 rows, from L alone

    def launch(**kw):
        fn = lambda: half.wgrad_seg_raw(ah, bh, buf[lead:], M, N, S, stride, ldc=ldc, splitk_hint=sk, **kw)  # noqa: E731
        if split:                                                 # the split workspace at its exact size between guard bands
            assert "ws" in guarded(ops, fn)[1].kinds()
        else:
            fn()

    launch()
    got = out.cpu().double()
    for s in range(S):
        tol = 2e-5 * math.sqrt(L) * max(1.0, want[s].abs().max().item())
        err = (got[s] - want[s]).abs().max().item()
        assert err < tol, (s, err, tol)
    mask = torch.ones(total, dtype=torch.bool, device=dev)
    _windows(mask, S, M, N, ldc, stride, lead).fill_(False)
    raw = buf.view(torch.int32)
    assert bool((raw[mask] == POISON * 0x01010101).all()), "a float outside the S x (M x N) output windows was written"
    launch(accumulate=True, alpha=0.5)
    got = out.cpu().double()
    for s in range(S):
        tol = 2 * 2e-5 * math.sqrt(L) * max(1.0, want[s].abs().max().item())
        assert (got[s] - 1.5 * want[s]).abs().max().item() < tol, s
    assert bool((raw[mask] == POISON * 0x01010101).all()), "accumulate wrote outside the output windows"
    if S == 1:
        plain = torch.empty((M, N), device=dev)
        half.wgrad_raw(ah, bh, plain, accumulate=False)
        tol = 2e-5 * math.sqrt(L) * max(1.0, want[0].abs().max().item())
        assert (plain.cpu().double() - want[0]).abs().max().item() < tol
        one = torch.empty((M, N), device=dev)
        half.wgrad_seg_raw(ah, bh, one, M, N, 1, M * N)
        assert (one.cpu().double() - plain.cpu().double()).abs().max().item() < tol


@pytest.mark.parametrize("L,M,N", [(1000, 320, 256), (77, 768, 256), (16, 1280, 256), (256, 256, 640), (154, 100, 36)])
def test_hgemm_tn_seg_independent_of_batch_and_deterministic(L, M, N):
    """exact: segment s of an S = 16 launch == the same rows computed alone (S = 1) == the same rows at another position of
    another S = 16 launch == a second run"""
    from gad import half
    S = 16
    ah, bh, _, _ = _operands(S, L, M, N, seed=5)
    stride = M * N + 24
    full = torch.zeros(S, stride, device=dev)
    half.wgrad_seg_raw(ah, bh, full, M, N, S, stride)
    again = torch.zeros(S, stride, device=dev)
    half.wgrad_seg_raw(ah, bh, again, M, N, S, stride)
    assert torch.equal(full, again), "two runs differ"
    for s in (0, 5, 15):
        alone = torch.zeros(M, N, device=dev)
        half.wgrad_seg_raw(ah[s * L:(s + 1) * L], bh[s * L:(s + 1) * L], alone, M, N, 1, M * N)
        assert torch.equal(alone.view(-1), full[s, :M * N]), f"segment {s} alone differs from its value inside S = 16"
    perm = [(s + 7) % S for s in range(S)]                       # segment s moves to position perm.index(s)
    ap = torch.cat([ah[s * L:(s + 1) * L] for s in perm])
    bp = torch.cat([bh[s * L:(s + 1) * L] for s in perm])
    moved = torch.zeros(S, stride, device=dev)
    half.wgrad_seg_raw(ap, bp, moved, M, N, S, stride)
    for pos, s in enumerate(perm):
        assert torch.equal(moved[pos], full[s]), f"segment {s} differs at position {pos}"


# ---------------------------------------------------------------------------------------------------------------
# per-sample features of a small SD U-Net with LoRA
# ---------------------------------------------------------------------------------------------------------------
SCHED = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", num_train_timesteps=1000)


def _lora_pair(ragged):
    """oracle / engine SD U-Nets (the reduced shape of test_gpu_sd.SMALL) with the same LoRA matrices, rank 8 or ragged 8 / 6 / 4"""
    import gad
    from oracle.diffusers_ref import LoRALinearLayer as RL
    from oracle.sd_unet_ref import CrossAttention as RCA
    from oracle.sd_unet_ref import UNet2DConditionModel as R
    from test_gpu_sd import SMALL
    torch.manual_seed(0)
    ref = R(**SMALL)
    net = gad.UNet2DConditionModel(**SMALL)
    net.load_state_dict(ref.state_dict())
    net.to(dev)
    for p in ref.parameters():
        p.requires_grad_(False)
    layers, i = {}, 0
    for name, m in ref.named_modules():
        if isinstance(m, RCA):
            for proj, lin in (("to_q", m.to_q), ("to_k", m.to_k), ("to_v", m.to_v), ("to_out", m.to_out[0])):
                r = 8 - (i % 3) * 2 if ragged else 8
                i += 1
                layer = RL(lin.in_features, lin.out_features, rank=r)
                with torch.no_grad():
                    layer.up.weight.copy_(rnd(lin.out_features, r, seed=100 + i, scale=0.05))
                lin.set_lora_layer(layer)
                layers[f"{name}.{proj}"] = layer
    net.inject_lora(rank=8, ranks={k: v.rank for k, v in layers.items()})
    for name, attn in net.attention_modules().items():
        base = name[: -len(".processor")]
        for proj, lin in (("to_q", attn.to_q), ("to_k", attn.to_k), ("to_v", attn.to_v), ("to_out", attn.to_out[0])):
            src = layers[f"{base}.{proj}"]
            with torch.no_grad():
                lin.lora_layer.down.weight.copy_(src.down.weight)
                lin.lora_layer.up.weight.copy_(src.up.weight)
    return ref, net


def _rows(n, k, seed=0):
    """n distinct (latent, context, k timesteps, k noises) rows"""
    g = torch.Generator().manual_seed(seed)
    lat = torch.randn(n, 4, 16, 16, generator=g) * 0.8
    ctx = torch.randn(n, 77, 96, generator=g) * 0.5
    ts = torch.randint(0, 1000, (n, k), generator=g)
    eps = torch.randn(n, k, 4, 16, 16, generator=g)
    return lat, ctx, ts, eps


def _oracle_gradients(ref, net, lat, ctx, ts, eps, behaviour):
    """per-row autograd gradients of the oracle U-Net, laid out like the engine's flat gradient buffer: [n][P] fp64"""
    from gad.trak import lora_flat_gradient
    from oracle import diffusers_ref as R
    sch = R.DDPMScheduler(**SCHED)
    params, gflat = lora_flat_gradient(net)
    where = {n: p._gad_flat for n, p in net.named_parameters() if p.requires_grad}
    ref_params = dict(ref.named_parameters())
    assert len(where) == len(params) and set(where) <= set(ref_params)
    out = np.zeros((lat.shape[0], gflat.numel()))
    k = ts.shape[1]
    for i in range(lat.shape[0]):
        ref.zero_grad()
        x = lat[i:i + 1].expand(k, -1, -1, -1)
        pred = ref(sch.add_noise(x, eps[i], ts[i]), ts[i], ctx[i:i + 1].expand(k, -1, -1)).sample
        target = eps[i] if behaviour == "loss" else torch.zeros_like(pred)
        torch.nn.functional.mse_loss(pred, target).backward()                # mean over the k rows of f(row)
        for n, (_, off, cnt) in where.items():
            out[i, off:off + cnt] = ref_params[n].grad.double().flatten().numpy()
    return out


def _rel_rows(got, want):
    return np.linalg.norm(np.asarray(got, dtype=np.float64) - want, axis=1) / np.linalg.norm(want, axis=1)


@pytest.mark.parametrize("ragged", [True, False])
def test_per_sample_features_match_autograd(ragged):
    """A batch of 4 distinct (latent, t, context) rows, `loss` and `mean-squared-l2-norm`, against per-sample autograd gradients of
    the oracle projected with tests/jl_ref.py.

    fp32 route (one sample per backward): relative row error <= 1e-4, the bar of
    test_gpu_trak.py::test_engine_features_match_autograd_per_sample_gradients for the same comparison.
    bf16 segmented route (all 4 samples in one backward): no derivable bar - bf16 activations move the gradient itself - so the
    yardstick is the EXISTING half path run one sample per backward into the flat buffer (B = 1), measured here against the
    same oracle; the segmented route differs from it only in fp32 summation order and in forward tile plans that change with M
    and must stay within 1.5 x its error.  Measured (profiles/ab_per_sample.txt (4)): 0.008 - 0.020 per row on both routes - at this
    reduced shape the two are equal to all printed digits, the segmented launch summing a segment exactly as a plain launch does."""
    import gad
    from gad import ops
    from gad.trak import Projector, lora_flat_gradient, lora_gradient_features
    from jl_ref import jl_project
    ref, net = _lora_pair(ragged)
    lat, ctx, ts, eps = _rows(4, 1, seed=3)
    sch = gad.DDPMScheduler(**SCHED)
    params, gflat = lora_flat_gradient(net)
    d = 64
    proj = Projector(grad_dim=gflat.numel(), proj_dim=d, seed=42, proj_type="normal", device=dev, max_batch_size=4)
    for behaviour in ("loss", "mean-squared-l2-norm"):
        want = jl_project(_oracle_gradients(ref, net, lat, ctx, ts, eps, behaviour), d, 42)
        got32 = lora_gradient_features(net, sch, lat, ctx, ts, behaviour, proj, noise=eps)
        rel32 = _rel_rows(got32.numpy(), want)
        print(f"ragged={ragged} {behaviour}: fp32 one-sample route rel row err {rel32}")
        assert rel32.max() <= 1e-4, (behaviour, rel32)
        try:
            gad.set_operand_precision("bf16")
            assert ops.half_activations()
            seg = lora_gradient_features(net, sch, lat, ctx, ts, behaviour, proj, noise=eps, samples_per_backward=4)
            base = torch.empty(4, d)
            for i in range(4):                                    # the existing path: flat sink, B = 1
                x, e, t = lat[i:i + 1].to(dev), eps[i].to(dev), ts[i].to(dev)
                pred = net(sch.add_noise(x, e, t), t, ctx[i:i + 1].to(dev)).sample.contiguous()
                target = e if behaviour == "loss" else torch.zeros_like(pred)
                _, dd = ops.mse_fwd_bwd_raw(pred, target.contiguous())
                ops.begin_backward_step()
                try:
                    pred.backward(dd)
                finally:
                    ops.end_backward_step()
                base[i] = proj.project(gflat.view(1, -1), 0)[0].cpu()
        finally:
            gad.set_operand_precision("no")
        rel_seg, rel_base = _rel_rows(seg.numpy(), want), _rel_rows(base.numpy(), want)
        print(f"ragged={ragged} {behaviour}: bf16 segmented rel row err {rel_seg}  bf16 one-sample flat-sink {rel_base}")
        assert rel_seg.max() <= 1.5 * rel_base.max(), (behaviour, rel_seg, rel_base)


def test_timestep_average_in_chunks_equals_one_chunk():
    """k = 6 timesteps accumulated as chunks of j = 4 + 2 == one chunk of 6, per matrix within the kernel bar of
    test_hgemm_tn_seg after an accumulate: 2 x 2e-5 sqrt(L) max(1, |want|max), L = 6 x 256 tokens (the longest segment)"""
    import gad
    from gad.trak import lora_per_sample_gradients
    _, net = _lora_pair(True)
    lat, ctx, ts, eps = _rows(3, 6, seed=4)
    sch = gad.DDPMScheduler(**SCHED)
    try:
        gad.set_operand_precision("bf16")
        one = [r.clone() for _, r in lora_per_sample_gradients(net, sch, lat, ctx, ts, "loss", 3, noise=eps, timesteps_per_backward=6)]
        two = [r.clone() for _, r in lora_per_sample_gradients(net, sch, lat, ctx, ts, "loss", 3, noise=eps, timesteps_per_backward=4)]
    finally:
        gad.set_operand_precision("no")
    (one,), (two,) = one, two
    assert one.abs().max() > 0
    worst = 0.0
    for p in net.parameters():
        if p.requires_grad:
            _, off, n = p._gad_flat
            a, b = two[:, off:off + n].double(), one[:, off:off + n].double()
            tol = 2 * 2e-5 * math.sqrt(6 * 256) * max(1.0, b.abs().max().item())
            err = (a - b).abs().max().item()
            worst = max(worst, err / tol)
            assert err < tol, (off, err, tol)
    print(f"chunks 4 + 2 against one chunk of 6: worst error / bar = {worst:.3e}")


def test_training_step_is_untouched_by_a_per_sample_pass():
    """one FusedTrainer step after a per-sample pass == the step of a model that never saw one, bit for bit (the sink is restored)"""
    import gad
    from gad import ops
    from gad.trak import lora_per_sample_gradients
    lat, ctx, ts, eps = _rows(4, 2, seed=5)
    sch = gad.DDPMScheduler(**SCHED)
    result = []
    try:
        gad.set_operand_precision("bf16")
        for with_pass in (True, False):
            _, net = _lora_pair(True)
            lora = [p for p in net.parameters() if p.requires_grad]
            if with_pass:
                for _ in lora_per_sample_gradients(net, sch, lat, ctx, ts, "loss", 4, noise=eps, timesteps_per_backward=2):
                    pass
                assert ops._PER_SAMPLE[0] is None and not ops._SINK_ACTIVE[0]
            tr = gad.FusedTrainer(net, sch, None, lr=3e-4, weight_decay=1e-6, adamw=True, max_grad_norm=1.0, params=lora)
            loss = tr.step(lat.to(dev), eps[:, 0].contiguous().to(dev), ts[:, 0].contiguous().to(dev), ctx.to(dev))
            result.append((float(loss.item()), tr.flat.clone()))
    finally:
        gad.set_operand_precision("no")
    assert result[0][0] == result[1][0] and torch.equal(result[0][1], result[1][1])


# ---------------------------------------------------------------------------------------------------------------
# the kept entry points end to end
# ---------------------------------------------------------------------------------------------------------------
def test_entry_points_end_to_end(tmp_path):
    """grad_text_to_image_lora.py on a synthetic latent cache for train / generated (both --f) and generated_journey (loss), then
    traks.py on its output: all files, finite values; a second run reproduces every feature file bit for bit"""
    import json
    import gad
    from test_gpu_sd import SMALL
    from text_to_image import grad_text_to_image_lora as G
    from text_to_image import traks
    from text_to_image import train_text_to_image_lora as T
    data = tmp_path / "artbench"
    T.synthetic_cache(str(data / "latent_cache.pt"), n=10, n_artists=4, res=128, ctx_dim=96)
    lora_dir = tmp_path / "lora"
    torch.manual_seed(0)
    net = gad.UNet2DConditionModel(**SMALL).to(dev)
    for i, p in enumerate(net.inject_lora(rank=8)):
        with torch.no_grad():
            p.copy_(rnd(*p.shape, seed=50 + i, scale=0.05))
    net.save_attn_procs(str(lora_dir))
    weights = tmp_path / "unet.pt"
    torch.save({k: v for k, v in net.state_dict().items() if "lora_layer" not in k}, weights)
    d, k = 64, 4
    common = ["--train_data_dir", str(data), "--output_dir", str(tmp_path / "out"), "--lora_dir", str(lora_dir), "--proj_dim", str(d),
              "--num_timesteps", str(k), "--num_images", "2", "--num_journey_points", "3", "--num_inference_steps", "8",
              "--resolution", "128", "--train_batch_size", "4", "--unet_weights", str(weights), "--unet_overrides", json.dumps(SMALL)]
    runs = [("train", "loss", 10), ("train", "mean-squared-l2-norm", 10), ("generated", "loss", 2),
            ("generated", "mean-squared-l2-norm", 2), ("generated_journey", "loss", 2 * len(G.journey_points(8, 3)))]

    def run_all():
        out = {}
        for source, f, rows in runs:
            path = G.main(G.parse_args(common + ["--source", source, "--f", f]))
            emb = torch.load(path, weights_only=False)
            assert emb.shape == (rows, d) and torch.isfinite(emb).all() and (emb.abs().sum(1) > 0).all(), (source, f)
            out[(source, f)] = (path, emb.clone())
        return out
    first = run_all()
    root = tmp_path / "out" / "artbench_post_impressionism"
    assert first[("train", "loss")][0] == str(root / "gradients" / "train" / f"emb_f=loss_num_timesteps={k}_proj_dim={d}.pt")
    assert first[("generated_journey", "loss")][0] == str(
        root / "gradients" / "generated_journey" / f"emb_f=loss_num_journey_points=3_num_journey_noises=1_proj_dim={d}.pt")
    assert not torch.equal(first[("train", "loss")][1], first[("train", "mean-squared-l2-norm")][1])
    import pandas as pd
    assert list(pd.read_csv(root / "gradients" / "train" / "group.csv").columns) == ["index", "artist", "filename"]
    gdf = pd.read_csv(root / "gradients" / "generated_journey" / "group.csv", index_col=0)
    assert list(gdf.columns) == ["generated_image_idx", "step_idx"] and list(gdf["step_idx"]) == [1, 3, 5, 7] * 2
    second = run_all()
    for key, (_, emb) in first.items():
        assert torch.equal(emb, second[key][1]), f"{key}: the second run differs"
    assert not ops_active()
    out_dir = traks.main(traks.parse_args(["--output_dir", str(root), "--num_timesteps", str(k), "--proj_dim", str(d),
                                           "--num_journey_points", "3", "--train_data_dir", str(data), "--device", "cuda"]))
    names = ["avg_grad_sim", "max_grad_sim", "trak", "relative_influence", "renorm_influence", "journey_trak", "dtrak"]
    assert sorted(os.listdir(out_dir)) == sorted([f"artist_{m}.npy" for m in names] + [f"all_generated_images_artist_rank_{m}.npy" for m in names])
    for m in names:
        arr = np.load(os.path.join(out_dir, f"artist_{m}.npy"))
        assert arr.shape == (4, 1) and np.isfinite(arr).all(), m
        assert np.array_equal(np.load(os.path.join(out_dir, f"all_generated_images_artist_rank_{m}.npy")),
                              np.argsort(-arr.mean(axis=-1), kind="stable"))


def ops_active():
    from gad import ops
    return ops._PER_SAMPLE[0] is not None or ops._SINK_ACTIVE[0] or ops.half_activations()
