"""Model behaviours of a LoRA-tuned Stable-Diffusion U-Net for the Shapley / LDS evaluators.

Entry point kept from the reference (text_to_image/compute_model_behaviors.py): same flags, duplicate check
(:168-189), reference LoRA vs coalition LoRA (:195-214), per-image loop with checkpoint / resume (:262-283,433-457),
classifier-free-guided 100-step generations (:311-326), the "simple loss" = mean over `n_noises` of the U-Net's MSE on
the reference sample noised at every scheduler timestep (:391-417), per-image `generated_image_{i}_{behaviour}` and
`..._time` columns, the 0.5 / 0.75 / 0.9 quantiles and averages (:460-495), `remaining_idx` / `removal_idx` from the LoRA
directory's removal_idx.csv (:206-214,497-498), one jsonl row per call (:499-501) - which is what
text_to_image/shapley_lds.py::collect_data reads (:105-135).

Only the U-Net half of the pipelines is on the MI355X hot path.  The frozen VAE, CLIP text tower, CLIP / open-CLIP image
towers and the aesthetic head are hub-fetched in the reference and absent here, so this entry point works on
LATENTS: prompts arrive as embeddings (`--prompt_embeds file.pt` with `cond` / `uncond` [77, D], or a seeded synthetic
pair), samples stay latents, and the CLIP / aesthetic scorers are a seeded stand-in embedder (the arithmetic - cosine
scores, quantiles, schema - is the reference's).  SSIM and NRMSE (:336-356, scikit-image's `structural_similarity` /
`normalized_root_mse` on the two uint8 PIL images) are restated here on uint8 pseudo-images of the latents
(`latents_to_uint8`: the pipeline's own (x/2+0.5).clamp(0,1)*255 round, with latents/4 in the VAE decoder's place).
`--sampler pndm` generates with the PLMS sampler that SD-1.x repositories ship instead of DDIM (gad.PNDMScheduler); the simple
loss then runs on its num_inference_steps + 1 timesteps, the repeated one included, as the reference's `pipeline.scheduler.timesteps`.
The row's keys are the same for both; tell the runs apart by --exp_name.

Where the published files exist the stand-ins give way (nothing changes while none of these is set):
  GAD_VAE_DECODER_TS=/path/decoder.pt   a TorchScript module mapping latents [B,4,h,w], already divided by the VAE's scaling
      factor (0.18215) by this caller, to images in [-1, 1]; stock torch ops, off the hand-written path, like
      GAD_FEATURE_NET_TS.  `ssim` and `nrmse` then run on the decoded uint8 images, and --img_dir stores them too.
  GAD_VAE_WEIGHTS=/path/vae.safetensors   the VAE's own state dict (diffusers' AutoencoderKL keys, .pt or .safetensors): the
      same decode on the HIP operators (gad/vae.py), accepted wherever GAD_VAE_DECODER_TS is; setting both is refused.
  GAD_CLIP_B32_WEIGHTS, GAD_CLIP_L14_WEIGHTS, GAD_AESTHETIC_WEIGHTS (all three, with a decoder: four-channel latents are not
      images)   OpenAI CLIP ViT-B/32, open-CLIP ViT-L-14 (openai weights) and LAION's nn.Linear(768, 1) head on the HIP
      operators (gad/vit.py): `clip_similarity` is the B/32 cosine of the two decoded images, `clip_prompt_score` the B/32
      cosine against the prompt embedding - read from the --prompt_embeds file's key `clip_prompt` ([embed_dim], normalised on
      load), or computed by the text tower when GAD_CLIP_BPE is set (below) - and `aesthetic_score` the head on the L/14
      unit embedding.  `feature_extractor` becomes the `;`-joined tags.
  GAD_SD_SCORER=clip-seeded   the same architectures with seeded weights: what the true tail costs, not what it scores.
  GAD_CLIP_BPE=/path   the CLIP tokenizer's vocabulary (gad/clip_bpe.py).  With the CLIP scorers configured and no `clip_prompt` in
      the --prompt_embeds file, the prompt is embedded by the B/32 text tower on the HIP operators (gad/text.py; the same
      archive GAD_CLIP_B32_WEIGHTS names, or seeded) and `;text=<tower tag>` joins `feature_extractor`.
  GAD_SD_TEXT_WEIGHTS=/path (with GAD_CLIP_BPE)   SD's text_encoder weights: `cond` / `uncond` that the --prompt_embeds file does
      not carry are the encoder's hidden states of the prompt and of the empty prompt, and the row gains `prompt_encoder`.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import pandas as pd
import torch

_HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

from src.ddpm_config import PromptConfig  # noqa: E402

BEHAVIOURS = ["ssim", "nrmse", "simple_loss", "clip_similarity", "clip_prompt_score", "aesthetic_score"]


def latents_to_uint8(lat: torch.Tensor) -> np.ndarray:
    """[1,C,h,w] latents -> [h,w,C] uint8, the way StableDiffusionPipeline turns the decoder output into a PIL image
    ((x/2+0.5).clamp(0,1) -> *255 -> round -> uint8) with latents/4 standing in for `vae.decode` (hub-fetched)."""
    x = (lat[0].detach().float().cpu() / 4.0 / 2 + 0.5).clamp(0, 1)
    return (x.permute(1, 2, 0).numpy() * 255).round().astype("uint8")


def structural_similarity_u8(im1: np.ndarray, im2: np.ndarray, data_range=255, win_size=7, K1=0.01, K2=0.03) -> float:
    """skimage.metrics.structural_similarity(im1, im2, channel_axis=-1, data_range=255) as called at
    compute_model_behaviors.py:338-346 (scikit-image is a third-party dependency, not vendored: algorithm restated -
    Wang et al. 2004 with skimage's defaults: 7x7 uniform window via scipy.ndimage.uniform_filter (reflect), sample
    covariance (NP/(NP-1)), float64, borders of (win-1)//2 cropped, mean over pixels then over channels)."""
    from scipy.ndimage import uniform_filter
    a, b = np.asarray(im1), np.asarray(im2)
    if a.shape != b.shape or a.ndim != 3:
        raise ValueError("structural_similarity_u8: two [H, W, C] images of one shape")
    if min(a.shape[:2]) < win_size:
        raise ValueError("win_size exceeds image extent")            # skimage's error, same condition
    NP = win_size ** 2
    cov_norm = NP / (NP - 1.0)
    C1, C2 = (K1 * data_range) ** 2, (K2 * data_range) ** 2
    pad = (win_size - 1) // 2
    out = []
    for ch in range(a.shape[-1]):
        x, y = a[..., ch].astype(np.float64), b[..., ch].astype(np.float64)
        ux, uy = uniform_filter(x, size=win_size), uniform_filter(y, size=win_size)
        uxx, uyy, uxy = uniform_filter(x * x, size=win_size), uniform_filter(y * y, size=win_size), uniform_filter(x * y, size=win_size)
        vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
        S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux ** 2 + uy ** 2 + C1) * (vx + vy + C2))
        out.append(S[pad:-pad, pad:-pad].mean(dtype=np.float64))
    return float(np.mean(out))


def normalized_root_mse_u8(image_true: np.ndarray, image_test: np.ndarray) -> float:
    """skimage.metrics.normalized_root_mse(image_true, image_test) (:350-354; default 'euclidean' normalisation):
    sqrt(mean((t - x)^2)) / sqrt(mean(t^2)) in float64."""
    t, x = np.asarray(image_true, dtype=np.float64), np.asarray(image_test, dtype=np.float64)
    return float(np.sqrt(np.mean((t - x) ** 2)) / np.sqrt(np.mean(t * t)))


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Compare images generated by two LoRA models.")
    p.add_argument("--pretrained_model_name_or_path", type=str, default="lambdalabs/miniSD-diffusers")
    p.add_argument("--revision", type=str, default=None)
    p.add_argument("--variant", type=str, default=None)
    p.add_argument("--reference_lora_dir", type=str, default=None, required=True)
    p.add_argument("--lora_dir", type=str, default=None)
    p.add_argument("--lora_steps", type=int, default=None)
    p.add_argument("--dataset", type=str, choices=["artbench"], default="artbench")
    p.add_argument("--num_images", type=int, default=50)
    p.add_argument("--n_noises", type=int, default=3)
    p.add_argument("--ckpt_freq", type=int, default=10)
    p.add_argument("--ckpt_path", type=str, default=None)
    p.add_argument("--img_dir", type=str, default=None)
    p.add_argument("--clean_up_ckpt", default=False, action="store_true")
    p.add_argument("--resolution", type=int, default=256)
    p.add_argument("--seed", type=int, default=42)
    p.add_argument("--cls", type=str, default="post_impressionism")
    p.add_argument("--db", type=str, default=None, required=True)
    p.add_argument("--exp_name", type=str, default=None, required=True)
    p.add_argument("--no_duplicate", action="store_true")
    # engine extras (not in the reference)
    p.add_argument("--prompt_embeds", type=str, default=None, help=".pt with cond / uncond [77, D] text embeddings")
    p.add_argument("--unet_overrides", type=str, default=None, help="JSON dict of UNet2DConditionModel constructor overrides")
    p.add_argument("--unet_weights", type=str, default=None, help="local state_dict of the base U-Net (optional)")
    p.add_argument("--num_inference_steps", type=int, default=100)
    p.add_argument("--guidance_scale", type=float, default=7.5)
    p.add_argument("--sampler", type=str, default="ddim", choices=["ddim", "pndm"], help="ddim (default) or pndm: the PLMS sampler SD-1.x repositories ship, num_inference_steps + 1 U-Net calls")
    p.add_argument("--device", type=str, default="cuda:0")
    return p.parse_args(argv)


REFERENCE_KEYS = ["pretrained_model_name_or_path", "revision", "variant", "reference_lora_dir", "lora_dir", "lora_steps",
                  "dataset", "num_images", "n_noises", "ckpt_freq", "ckpt_path", "img_dir", "clean_up_ckpt", "resolution",
                  "seed", "cls", "db", "exp_name", "no_duplicate"]


def has_duplicate(args) -> bool:
    """:168-189 - a row with the same arguments (all but no_duplicate / ckpt_freq) is already in the db."""
    if not (args.db is not None and os.path.exists(args.db) and args.no_duplicate):
        return False
    df = pd.read_json(args.db, lines=True)
    for key in REFERENCE_KEYS:
        if key in ("no_duplicate", "ckpt_freq"):
            continue
        if df.shape[0] == 0:
            return False
        val = getattr(args, key)
        df = df[df[key].isna()] if val is None else df[df[key] == val]
    return df.shape[0] > 0


def assemble_row(args, lists: dict, times: dict, remaining_idx, removal_idx, tag=None) -> dict:
    """The jsonl row of :459-498 from the per-image lists (pure host code; text_to_image/shapley_lds.py reads
    `exp_name`, `remaining_idx` and either `{behaviour}` aggregates or `generated_image_{i}_{behaviour}`)."""
    row = {k: getattr(args, k) for k in REFERENCE_KEYS}
    n = len(lists["aesthetic_score"])
    for i in range(n):
        prefix = f"generated_image_{i}"
        for b in BEHAVIOURS:
            row[f"{prefix}_{b}"] = lists[b][i]
        for b in BEHAVIOURS:
            row[f"{prefix}_{b}_time"] = times[b][i]
    for q in (0.5, 0.75, 0.9):
        row[f"aesthetic_score_{q}"] = float(np.quantile(lists["aesthetic_score"], q=q))
        row[f"clip_prompt_score_{q}"] = float(np.quantile(lists["clip_prompt_score"], q=q))
    row["aesthetic_score_avg"] = float(np.mean(lists["aesthetic_score"]))
    row["clip_prompt_score_avg"] = float(np.mean(lists["clip_prompt_score"]))
    row["aesthetic_score_time"] = float(np.sum(times["aesthetic_score"]))
    row["clip_prompt_score_time"] = float(np.sum(times["clip_prompt_score"]))
    row["remaining_idx"] = remaining_idx
    row["removal_idx"] = removal_idx
    row["feature_extractor"] = tag or LatentScorer.TAG        # stand-in scorers: never to be mixed with CLIP / aesthetic-head rows
    return row


VAE_SCALING = 0.18215
WEIGHT_VARS = ("GAD_CLIP_B32_WEIGHTS", "GAD_CLIP_L14_WEIGHTS", "GAD_AESTHETIC_WEIGHTS")


def scorer_settings(prompt_embeds=None):
    """What the environment asks for, checked before anything is loaded (pure host code) -> None while no CLIP variable is set
    (the stand-in scorer, whether or not a decoder is), else {"weights": {variable: path} or None for the seeded towers}.
    `prompt_embeds`: the loaded --prompt_embeds dict or None."""
    from gad.text import sd_text_setting
    sd_text_setting()                                          # (GAD_SD_TEXT_WEIGHTS without GAD_CLIP_BPE: refused here)
    kind = os.environ.get("GAD_SD_SCORER")
    if kind and kind != "clip-seeded":
        raise ValueError(f"GAD_SD_SCORER={kind!r}: the only value is 'clip-seeded'")
    decoder = decoder_setting()                                # (both decoder variables at once: refused here)
    weights = {v: os.environ.get(v) for v in WEIGHT_VARS}
    if not kind and not any(weights.values()):
        return None
    if not kind and not all(weights.values()):
        raise ValueError("the CLIP scorers need all of " + ", ".join(WEIGHT_VARS) + "; not set: "
                         + ", ".join(v for v, p in weights.items() if not p))
    if decoder is None:
        raise ValueError("the CLIP image towers score images, and four-channel latents are not images: set GAD_VAE_DECODER_TS "
                         "to a TorchScript VAE decoder (or GAD_VAE_WEIGHTS to the VAE's state dict)")
    text = prompt_embeds is None or "clip_prompt" not in prompt_embeds     # the prompt's embedding comes from the text tower
    if text and not os.environ.get("GAD_CLIP_BPE"):
        raise ValueError("the CLIP text tower is not part of this project: with the CLIP scorers the --prompt_embeds file must "
                         "carry the prompt's CLIP ViT-B/32 text embedding under the key 'clip_prompt'")
    return {"weights": weights if all(weights.values()) else None, **({"text": True} if text else {})}


def decoder_setting():
    """Which VAE decoder the environment names, as pure host code -> None, ("GAD_VAE_DECODER_TS", path) or
    ("GAD_VAE_WEIGHTS", path); both at once are refused before anything loads."""
    ts, hip = os.environ.get("GAD_VAE_DECODER_TS"), os.environ.get("GAD_VAE_WEIGHTS")
    if ts and hip:
        raise ValueError("GAD_VAE_DECODER_TS and GAD_VAE_WEIGHTS are both set: they name the same decoder twice (a TorchScript "
                         "export and the state dict for the HIP operators) - set one")
    if ts:
        return "GAD_VAE_DECODER_TS", ts
    return ("GAD_VAE_WEIGHTS", hip) if hip else None


def make_decoder(device):
    """the decoder `decoder_setting` names (None: none) - an object with ScriptedDecoder's call protocol and a `tag`"""
    setting = decoder_setting()
    if setting is None:
        return None
    return (ScriptedDecoder if setting[0] == "GAD_VAE_DECODER_TS" else HipDecoder)(setting[1], device)


class HipDecoder:
    """`GAD_VAE_WEIGHTS`: ScriptedDecoder's protocol on gad.AutoencoderKL (the SD VAE preset, HIP operators)."""

    def __init__(self, path, device, preset="SD_VAE"):
        from gad.vae import AutoencoderKL
        self.vae = AutoencoderKL.from_file(path, preset).to(device)
        self.tag = self.vae.tag

    @torch.no_grad()
    def __call__(self, lat):
        x = (self.vae.decode(lat.float() / VAE_SCALING).sample / 2 + 0.5).clamp(0, 1)
        u8 = (x * 255).round()
        return u8[0].permute(1, 2, 0).to(torch.uint8).cpu().numpy(), (u8 / 255).contiguous()


class ScriptedDecoder:
    """`GAD_VAE_DECODER_TS`: latents [1,4,h,w] (as the pipeline returns them) -> the PIL image the reference's pipeline makes
    of them, as uint8 [H,W,3] on the host and as [1,3,H,W] in [0,1] on the device (the uint8 values / 255: the scorers of the
    reference see the PIL image)."""

    def __init__(self, path, device):
        from gad.extractor import file_tag
        self.mod = torch.jit.load(path, map_location=device).eval()
        self.tag = file_tag("torchscript", path)

    @torch.no_grad()
    def __call__(self, lat):
        x = (self.mod(lat.float() / VAE_SCALING).float() / 2 + 0.5).clamp(0, 1)
        u8 = (x * 255).round()
        return u8[0].permute(1, 2, 0).to(torch.uint8).cpu().numpy(), (u8 / 255).contiguous()


class ClipScorer:
    """CLIP ViT-B/32 and open-CLIP ViT-L-14 + aesthetic head on the HIP operators (gad/vit.py, imported only here)."""

    def __init__(self, settings, prompt, device, prompt_text=None):
        from gad import vit
        w = settings["weights"]
        if w:
            self.b32 = vit.VisionTower.from_file(w["GAD_CLIP_B32_WEIGHTS"], "clip_vit_b32").to(device)
            self.l14 = vit.VisionTower.from_file(w["GAD_CLIP_L14_WEIGHTS"], "clip_vit_l14").to(device)
            self.head = vit.AestheticHead.from_file(self.l14, w["GAD_AESTHETIC_WEIGHTS"]).to(device)
        else:
            self.b32 = vit.VisionTower.seeded("clip_vit_b32").to(device)
            self.l14 = vit.VisionTower.seeded("clip_vit_l14").to(device)
            self.head = vit.AestheticHead.seeded(self.l14).to(device)
        text_tag = None
        if prompt is None:                                      # settings["text"]: the B/32 text tower embeds the prompt itself
            from gad.text import clip_prompt_embedding
            prompt, text_tag = clip_prompt_embedding(prompt_text, w["GAD_CLIP_B32_WEIGHTS"] if w else None, device)
        prompt = prompt.detach().float().reshape(-1)
        if prompt.numel() != self.b32.dims:
            raise ValueError(f"--prompt_embeds: 'clip_prompt' has {prompt.numel()} entries, the image tower embeds into {self.b32.dims}")
        self.prompt = torch.nn.functional.normalize(prompt, dim=0).to(device)
        self.tag = ";".join((self.b32.tag, self.l14.tag, self.head.tag) + ((f"text={text_tag}",) if text_tag else ()))

    def embed(self, image01):
        return self.b32.embed_unit(image01)[0]

    def aesthetic(self, image01):
        return self.head(image01)[0].item()


class LatentScorer:
    """Seeded stand-in for the CLIP / open-CLIP image towers + aesthetic head (hub-fetched in the reference,
    compute_model_behaviors.py:243,258-262): latents [1,4,h,w] -> unit embedding; aesthetic = linear head on it."""

    TAG = "standin-latent-scorer-seed1234"

    def __init__(self, device, dim=64, seed=1234):
        g = torch.Generator().manual_seed(seed)
        self.proj = (torch.randn(4 * 8 * 8, dim, generator=g) / 16.0).to(device)
        self.head = torch.randn(dim, generator=g).to(device)
        self.prompt = torch.nn.functional.normalize(torch.randn(dim, generator=g), dim=0).to(device)

    def embed(self, lat):
        pooled = torch.nn.functional.adaptive_avg_pool2d(lat.float(), 8).flatten(1)
        return torch.nn.functional.normalize(pooled @ self.proj, dim=-1).squeeze(0)


def main(args, backend=None):
    if backend is None:
        import gad as backend
    if has_duplicate(args):
        print(f"Found duplicate record in database at {args.db}. Process cancelled.")
        return False
    device = torch.device(args.device)
    pe = torch.load(args.prompt_embeds, map_location="cpu", weights_only=False) if args.prompt_embeds else None
    settings = scorer_settings(pe)                                             # refusals come before anything is loaded
    prompt = PromptConfig.artbench_config[args.cls]                           # :192-194 (kept for the record)
    ucfg = json.loads(args.unet_overrides) if args.unet_overrides else {}

    def load_unet(lora_dir, weight_name):
        # without --unet_weights the base is the random init of `seed`, exactly as train_text_to_image_lora.py builds it
        backend.seed_everything(args.seed)
        unet = backend.UNet2DConditionModel(**ucfg)
        if args.unet_weights:
            unet.load_state_dict(torch.load(args.unet_weights, map_location="cpu", weights_only=False))
        unet.to(device)
        if lora_dir is not None:
            unet.load_attn_procs(lora_dir, weight_name=weight_name)
        return unet.eval()

    ref_unet = load_unet(args.reference_lora_dir, "pytorch_lora_weights.safetensors")
    name = "pytorch_lora_weights" + (f"_{args.lora_steps}" if args.lora_steps is not None else "") + ".safetensors"
    unet = load_unet(args.lora_dir, name)
    remaining_idx = removal_idx = None
    if args.lora_dir is not None:
        f = os.path.join(args.lora_dir, "removal_idx.csv")
        if os.path.exists(f):
            df = pd.read_csv(f)
            remaining_idx = df["idx"][df["remaining"]].to_list()
            removal_idx = df["idx"][~df["remaining"]].to_list()
    else:
        print("Pretrained model is loaded")

    ctx_dim = ref_unet.config.cross_attention_dim
    from gad.text import prompt_context
    cond, uncond, prompt_encoder = prompt_context(prompt, pe, ctx_dim, device)
    cond, uncond = cond.to(device).unsqueeze(0), uncond.to(device).unsqueeze(0)

    # the reference takes the scheduler its model repository ships (:153-164); each pipeline owns one (PNDM keeps state)
    ref_pipe, pipe = (backend.StableDiffusionLatentPipeline(u, backend.sd_scheduler(args.sampler)) for u in (ref_unet, unet))
    noise_sched = backend.DDPMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear",
                                        num_train_timesteps=1000)
    decoder = make_decoder(device)
    scorer = LatentScorer(device) if settings is None else ClipScorer(settings, None if settings.get("text") else pe["clip_prompt"], device, prompt)
    ref_gen = torch.Generator(device=device).manual_seed(args.seed)            # :200-201,216-219
    gen = torch.Generator(device=device).manual_seed(args.seed)
    noise_gen = torch.Generator(device=device).manual_seed(args.seed)
    lists = {b: [] for b in BEHAVIOURS}
    times = {b: [] for b in BEHAVIOURS}
    done = 0
    if args.ckpt_path is not None and os.path.exists(args.ckpt_path):          # :262-283
        ck = torch.load(args.ckpt_path, map_location="cpu", weights_only=False)
        ref_gen.set_state(ck["reference_generator_state"])
        gen.set_state(ck["generator_state"])
        noise_gen.set_state(ck["noise_generator_state"])
        for b in BEHAVIOURS:
            lists[b], times[b] = ck[f"{b}_list"], ck[f"{b}_time_list"]
        done = ck["num_completed_images"]
        print(f"Checkpoint loaded from {args.ckpt_path}")
    if args.img_dir is not None:
        os.makedirs(args.img_dir, exist_ok=True)

    def sync():
        if device.type == "cuda":
            torch.cuda.synchronize(device)

    kw = dict(num_inference_steps=args.num_inference_steps, guidance_scale=args.guidance_scale,
              height=args.resolution, width=args.resolution)
    for i in range(done, args.num_images):
        ref_lat = ref_pipe(cond, uncond, generator=ref_gen, **kw).latents       # :311-317
        sync()
        t_gen = time.time()
        lat = pipe(cond, uncond, generator=gen, **kw).latents                   # :319-326
        sync()
        t_gen = time.time() - t_gen
        if decoder is None:
            ref_u8, u8 = latents_to_uint8(ref_lat), latents_to_uint8(lat)
            stored = {"reference": ref_lat.cpu(), "sample": lat.cpu()}
        else:                                                                   # the decoded images, as the reference's PIL pair
            (ref_u8, ref_img), (u8, img) = decoder(ref_lat), decoder(lat)
            stored = {"reference": ref_lat.cpu(), "sample": lat.cpu(), "reference_image": torch.from_numpy(ref_u8),
                      "sample_image": torch.from_numpy(u8)}
        if args.img_dir is not None:
            torch.save(stored, os.path.join(args.img_dir, f"latents_seed={args.seed}_sample_{i}.pt"))
        t0 = time.time()                                                        # ssim (:336-346)
        lists["ssim"].append(structural_similarity_u8(ref_u8, u8, data_range=255))
        times["ssim"].append(time.time() - t0 + t_gen)
        t0 = time.time()                                                        # nrmse (:348-356), euclidean normalisation
        lists["nrmse"].append(normalized_root_mse_u8(ref_u8, u8))
        times["nrmse"].append(time.time() - t0 + t_gen)
        t0 = time.time()                                                        # clip similarity (:358-378)
        e_ref, e = (scorer.embed(ref_lat), scorer.embed(lat)) if settings is None else (scorer.embed(ref_img), scorer.embed(img))
        lists["clip_similarity"].append(torch.dot(e_ref, e).item())
        times["clip_similarity"].append(time.time() - t0 + t_gen)
        t0 = time.time()                                                        # clip prompt score (:380-388)
        lists["clip_prompt_score"].append(torch.dot(e, scorer.prompt).item())
        times["clip_prompt_score"].append(time.time() - t0 + t_gen)
        t0 = time.time()                                                        # simple loss (:390-417)
        pipe.scheduler.set_timesteps(args.num_inference_steps)
        ts = pipe.scheduler.timesteps.to(device)                                # pndm: num_inference_steps + 1 entries, one twice
        lists["simple_loss"].append(backend.sd_simple_loss(unet, noise_sched, ref_lat, cond, ts, n_noises=args.n_noises,
                                                           generator=noise_gen))
        sync()
        times["simple_loss"].append(time.time() - t0)
        t0 = time.time()                                                        # aesthetic score (:419-431)
        lists["aesthetic_score"].append(torch.dot(e, scorer.head).item() if settings is None else scorer.aesthetic(img))
        times["aesthetic_score"].append(time.time() - t0 + t_gen)
        done += 1
        if args.ckpt_path is not None and done % args.ckpt_freq == 0:            # :433-457
            ck = {"reference_generator_state": ref_gen.get_state(), "generator_state": gen.get_state(),
                  "noise_generator_state": noise_gen.get_state(), "num_completed_images": done}
            for b in BEHAVIOURS:
                ck[f"{b}_list"], ck[f"{b}_time_list"] = lists[b], times[b]
            torch.save(ck, args.ckpt_path)
            print(f"Checkpoint saved tp {args.ckpt_path}")

    row = assemble_row(args, lists, times, remaining_idx, removal_idx, tag=None if settings is None else scorer.tag)
    if prompt_encoder is not None:
        row["prompt_encoder"] = prompt_encoder
    with open(args.db, "a+") as f:
        f.write(json.dumps(row) + "\n")
    print(f"Results saved to the database at {args.db}")
    if args.clean_up_ckpt and args.ckpt_path is not None and os.path.exists(args.ckpt_path):
        os.remove(args.ckpt_path)
    return True


if __name__ == "__main__":
    main(parse_args())
