"""Pixel- and CLIP-similarity baselines for the text-to-image experiment (entry point kept from the reference
text_to_image/baselines.py; pixel_similarity.py and clip_similarity.py are its two halves and run this module's `run`).

The reference's flags, defaults and output files: `{output_dir}/baselines/{group}_{max,avg}_{pixel,clip}_similarity.npy`
([groups, num_images] float64), `generated_image_{i}_{group}_rank_{name}.npy` and `all_generated_images_{group}_rank_{name}.npy`
(baselines.py:263-314).  Its shape is not kept: it re-reads and re-normalises the 5 000 training images - and pushes them through
CLIP again - for each of the 50 generated images.  Here the training pixels stay on the device as uint8, the B/32 tower sees every
image once, and one launch per side (gad.cosine_rows, csrc/similarity.hip) produces every cosine with the norms folded in.

Generated images: one reference-LoRA pipeline, one generator seeded by --seed, --num_images sequential guided generations - the
stream compute_model_behaviors.py draws for `ref_lat`.

Training images: `--train_pixels FILE`, a .npy of uint8 [N, H, W, 3] in the row order of the latent cache's class subset, with
H = W = --resolution (the reference's antialiased bilinear Resize is not restated here, and ArtBench is stored at 256: another
size is refused).  Cosines do not depend on the element order, so rows stay (h, w, c) on both sides.

Networks, as in compute_model_behaviors.py: GAD_VAE_DECODER_TS (TorchScript VAE decoder) and, for the CLIP half,
GAD_CLIP_B32_WEIGHTS - or GAD_SD_SCORER=clip-seeded for the architecture with seeded weights.  A program asks only for what it
uses.  With none of these set and no --train_pixels everything runs on stand-ins (uint8 pseudo-images of the latents on both
sides, `latents_to_uint8`; LatentScorer embeddings) and `baselines/feature_extractor.json` says so; a partial setting is refused
before anything is loaded.  Groups: `{cls}_{group}s.csv` against the cache's `artist` / `filename` column, as traks.py does.

Engine extras (not in the reference): --prompt_embeds, --unet_overrides, --unet_weights, --num_inference_steps,
--guidance_scale, --device, --train_data_dir, --synthetic_cache, --train_pixels; `main(args, backend=None)`.
--dataloader_num_workers is accepted and unused (nothing is loaded per batch).  The prompt: `--prompt_embeds`, else the text encoder
GAD_SD_TEXT_WEIGHTS + GAD_CLIP_BPE name (gad/text.py), else the seeded stand-in."""
import argparse
import json
import os
import sys

import numpy as np
import pandas as pd
import torch

_HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

import src.constants as constants  # noqa: E402
from src.ddpm_config import PromptConfig  # noqa: E402
from text_to_image.compute_model_behaviors import LatentScorer, decoder_setting, latents_to_uint8, make_decoder  # noqa: E402

PIXEL, CLIP = "pixel_similarity", "clip_similarity"
PIXEL_STANDIN_TAG = "standin-latent-pixels"


def parse_args(argv=None, description="Run simple baselines for data attribution.", batch_size=2048, workers=4, generate=True):
    """baselines.py:23-113 (aesthetic_score.py:18-62 with generate=False) plus the engine extras"""
    p = argparse.ArgumentParser(description=description)
    if generate:
        p.add_argument("--pretrained_model_name_or_path", type=str, default="lambdalabs/miniSD-diffusers")
        p.add_argument("--revision", type=str, default=None)
        p.add_argument("--variant", type=str, default=None)
        p.add_argument("--reference_lora_dir", type=str, default=None, required=True)
    p.add_argument("--dataset", type=str, choices=["artbench"], default="artbench")
    if generate:
        p.add_argument("--num_images", type=int, default=50)
        p.add_argument("--resolution", type=int, default=256)
        p.add_argument("--seed", type=int, default=42)
    p.add_argument("--cls", type=str, default="post_impressionism")
    p.add_argument("--group", type=str, default="artist", choices=["artist", "filename"])
    p.add_argument("--output_dir", type=str, default=None, required=True)
    p.add_argument("--dataloader_num_workers", type=int, default=workers)
    p.add_argument("--batch_size", type=int, default=batch_size)
    # engine extras (not in the reference)
    if generate:
        p.add_argument("--prompt_embeds", type=str, default=None, help=".pt with cond / uncond [77, D] text embeddings")
        p.add_argument("--unet_overrides", type=str, default=None, help="JSON dict of UNet2DConditionModel constructor overrides")
        p.add_argument("--unet_weights", type=str, default=None, help="local state_dict of the base U-Net (optional)")
        p.add_argument("--num_inference_steps", type=int, default=100)
        p.add_argument("--guidance_scale", type=float, default=7.5)
        p.add_argument("--sampler", type=str, default="ddim", choices=["ddim", "pndm"], help="ddim (default) or pndm: the PLMS sampler SD-1.x repositories ship, num_inference_steps + 1 U-Net calls")
    else:
        p.add_argument("--resolution", type=int, default=256, help="side of the stand-in latent cache's images")
    p.add_argument("--device", type=str, default="cuda:0")
    p.add_argument("--train_data_dir", type=str, default=None, help="directory of latent_cache.pt and {cls}_{group}s.csv")
    p.add_argument("--synthetic_cache", action="store_true", help="create a seeded stand-in latent cache if missing")
    p.add_argument("--train_pixels", type=str, default=None, help=".npy uint8 [N, H, W, 3]: the class subset's images, cache order")
    return p.parse_args(argv)


def network_settings(file_vars, train_pixels, what):
    """What the environment asks of a program that needs the files `file_vars` (beside --train_pixels), checked before anything
    is loaded (pure host code) -> None for the stand-ins (nothing set), else {variable: path or None}; None as a path is the
    seeded architecture (GAD_SD_SCORER=clip-seeded; GAD_VAE_DECODER_TS has no seeded form).  Anything in between is refused.
    GAD_VAE_WEIGHTS (the VAE's state dict, decoded on the HIP operators) stands wherever GAD_VAE_DECODER_TS does: its path is
    reported under that name, `make_decoder` knows which it is; both at once are refused."""
    kind = os.environ.get("GAD_SD_SCORER")
    if kind and kind != "clip-seeded":
        raise ValueError(f"GAD_SD_SCORER={kind!r}: the only value is 'clip-seeded'")
    decoder = decoder_setting()
    paths = {v: os.environ.get(v) or None for v in file_vars}
    if "GAD_VAE_DECODER_TS" in paths and decoder is not None:
        paths["GAD_VAE_DECODER_TS"] = decoder[1]
    seedable = [v for v in file_vars if v != "GAD_VAE_DECODER_TS"]
    if not kind and not any(paths.values()) and not train_pixels:
        return None
    missing = [v for v, p in paths.items() if not p and not (kind and v in seedable)]
    if not train_pixels:
        missing.append("--train_pixels")
    if missing:
        raise ValueError(f"{what} runs either on stand-ins (none of {', '.join(file_vars)}, GAD_SD_SCORER, --train_pixels) or on "
                         f"all of them; not set: {', '.join(missing)}")
    return paths


def load_training_side(args, unet_ctx_dim=768):
    """The latent cache's class subset and its groups (traks.py:97-99 on the cache's own columns) ->
    (latents [N,4,h,w], group_indices list of index arrays, cache).  Host code."""
    from text_to_image.train_text_to_image_lora import synthetic_cache
    if args.dataset != "artbench":
        raise ValueError(args.dataset)
    data_dir = args.train_data_dir or os.path.join(constants.DATASET_DIR, "artbench-10-imagefolder-split", "train")
    cache_path = os.path.join(data_dir, "latent_cache.pt")
    if not os.path.exists(cache_path):
        if not args.synthetic_cache:
            raise FileNotFoundError(f"{cache_path} not found (pass --synthetic_cache for a seeded stand-in)")
        synthetic_cache(cache_path, res=args.resolution, ctx_dim=unet_ctx_dim)
    cache = torch.load(cache_path, map_location="cpu", weights_only=False)
    keep = np.arange(len(cache["latents"]))
    if "style" in cache:                                                    # baselines.py:146-147
        keep = keep[np.array(cache["style"]) == args.cls]
    group_df = pd.read_csv(os.path.join(data_dir, f"{args.cls}_{args.group}s.csv"))
    names = np.array(cache[args.group])[keep]
    group_indices = [np.where(names == group_df.iloc[i].item())[0] for i in group_df.index]
    return cache["latents"][keep].float(), group_indices, cache


def load_train_pixels(path, n_rows, resolution):
    """--train_pixels -> uint8 [N, H, W, 3] (host), or a refusal by name"""
    px = np.load(path, mmap_mode="r")
    if px.dtype != np.uint8 or px.ndim != 4 or px.shape[-1] != 3:
        raise ValueError(f"--train_pixels {path}: expected uint8 [N, H, W, 3], got {px.dtype} {px.shape}")
    if px.shape[0] != n_rows:
        raise ValueError(f"--train_pixels {path}: {px.shape[0]} images, the latent cache's class subset has {n_rows} "
                         "(one row per cached image, in the cache's order)")
    if px.shape[1] != resolution or px.shape[2] != resolution:
        raise ValueError(f"--train_pixels {path}: images are {px.shape[1]} x {px.shape[2]}, --resolution is {resolution}; the "
                         "reference's antialiased bilinear Resize is not part of this program - store the images at --resolution")
    return np.ascontiguousarray(px)


def images01(u8_nhwc):
    """uint8 [B,H,W,3] on the device -> [B,3,H,W] in [0,1]: what the towers take (the PIL image / 255)"""
    return (u8_nhwc.permute(0, 3, 1, 2).float() / 255).contiguous()


def tower_rows(tower, train_u8, batch_size):
    """the tower once over the resident uint8 images, `batch_size` at a time -> [N, dims] (not normalised)"""
    return torch.cat([tower.forward(images01(train_u8[s:s + batch_size])) for s in range(0, len(train_u8), batch_size)], 0)


def generated_latents(args, backend, device):
    """--num_images sequential guided generations of the reference LoRA from one generator seeded by --seed
    (baselines.py:215-231; compute_model_behaviors.py's `ref_lat` stream)"""
    prompt = PromptConfig.artbench_config[args.cls]
    ucfg = json.loads(args.unet_overrides) if args.unet_overrides else {}
    backend.seed_everything(args.seed)
    unet = backend.UNet2DConditionModel(**ucfg)
    if args.unet_weights:
        unet.load_state_dict(torch.load(args.unet_weights, map_location="cpu", weights_only=False))
    unet.to(device)
    unet.load_attn_procs(args.reference_lora_dir, weight_name="pytorch_lora_weights.safetensors")
    unet.eval()
    from gad.text import prompt_context                                        # file > GAD_SD_TEXT_WEIGHTS' encoder > seeded stand-in
    pe = torch.load(args.prompt_embeds, map_location="cpu", weights_only=False) if args.prompt_embeds else None
    cond, uncond, _ = prompt_context(prompt, pe, unet.config.cross_attention_dim, device)
    cond, uncond = cond.to(device).unsqueeze(0), uncond.to(device).unsqueeze(0)
    pipe = backend.StableDiffusionLatentPipeline(unet, backend.sd_scheduler(args.sampler))
    gen = torch.Generator(device=device).manual_seed(args.seed)
    return [pipe(cond, uncond, generator=gen, num_inference_steps=args.num_inference_steps, guidance_scale=args.guidance_scale,
                 height=args.resolution, width=args.resolution).latents for _ in range(args.num_images)]


def write_tags(out_dir, tags):
    """baselines/feature_extractor.json: name -> the tag of what produced it (merged with what other programs wrote)"""
    path = os.path.join(out_dir, "feature_extractor.json")
    old = {}
    if os.path.exists(path):
        with open(path) as f:
            old = json.load(f)
    old.update(tags)
    with open(path, "w") as f:
        json.dump(old, f, indent=1, sort_keys=True)


def run(args, which, backend=None):
    """`which`: the similarities to compute, of (PIXEL, CLIP).  Returns {name: {"x", "q", "sim"}} (device tensors: the training
    rows, the generated rows and their cosine matrix [N, num_images]) plus "outputs", "group_indices", "dir"."""
    from gad import _capi, similarity
    if backend is None:
        import gad as backend
    needs = ["GAD_VAE_DECODER_TS"] + (["GAD_CLIP_B32_WEIGHTS"] if CLIP in which else [])
    settings = network_settings(needs, args.train_pixels, " + ".join(which))    # refusals come before anything is loaded
    latents, group_indices, _ = load_training_side(args)
    train_px = load_train_pixels(args.train_pixels, len(latents), args.resolution) if settings is not None else None
    device = torch.device(args.device)
    if device.type != "cuda":
        raise _capi.GadError(f"--device {args.device}: the similarity baselines run on the GPU (there is no CPU path)")
    lut = torch.from_numpy(similarity.pixel_lut()).to(device)

    gen_lat = generated_latents(args, backend, device)
    res, tags = {}, {}
    if settings is None:                                                     # stand-ins: pseudo-images of the latents on both sides
        train_u8 = torch.from_numpy(np.stack([latents_to_uint8(latents[i:i + 1]) for i in range(len(latents))])).to(device)
        gen_u8 = torch.from_numpy(np.stack([latents_to_uint8(lat) for lat in gen_lat])).to(device)
        if PIXEL in which:
            tags[PIXEL] = PIXEL_STANDIN_TAG
        if CLIP in which:
            scorer = LatentScorer(device)
            lat_dev = latents.to(device)
            res[CLIP] = {"x": torch.cat([scorer.embed(lat_dev[s:s + args.batch_size]).reshape(-1, scorer.head.numel())
                                         for s in range(0, len(lat_dev), args.batch_size)], 0).contiguous(),
                         "q": torch.stack([scorer.embed(lat) for lat in gen_lat]).contiguous()}
            tags[CLIP] = LatentScorer.TAG
    else:
        decoder = make_decoder(device)
        decoded = [decoder(lat) for lat in gen_lat]                            # (uint8 [H,W,3] host, [1,3,H,W] in [0,1] device)
        gen_u8 = torch.from_numpy(np.stack([u8 for u8, _ in decoded])).to(device)
        if tuple(gen_u8.shape[1:]) != tuple(train_px.shape[1:]):
            raise ValueError(f"{decoder_setting()[0]} decodes to {tuple(gen_u8.shape[1:])}, --train_pixels holds {tuple(train_px.shape[1:])}")
        train_u8 = torch.from_numpy(train_px).to(device)                       # resident as uint8: a quarter of the fp32 bytes
        if PIXEL in which:
            tags[PIXEL] = f"pixels;{decoder.tag}"
        if CLIP in which:
            from gad import vit
            path = settings["GAD_CLIP_B32_WEIGHTS"]
            b32 = (vit.VisionTower.from_file(path, "clip_vit_b32") if path else vit.VisionTower.seeded("clip_vit_b32")).to(device)
            res[CLIP] = {"x": tower_rows(b32, train_u8, args.batch_size),        # the tower once per training image ...
                         "q": torch.cat([b32.forward(img) for _, img in decoded], 0).contiguous()}   # ... and per generated one
            tags[CLIP] = f"{b32.tag};{decoder.tag}"
    if PIXEL in which:
        res[PIXEL] = {"x": train_u8, "q": lut[gen_u8.reshape(len(gen_u8), -1).long()].contiguous()}   # train_transforms(img).flatten()

    outputs = {}
    for name in which:
        r = res[name]
        r["sim"] = similarity.cosine_rows(r["x"], r["q"])
        gmax, gavg = similarity.group_aggregate(r["sim"].cpu().numpy(), group_indices)
        outputs[f"max_{name}"], outputs[f"avg_{name}"] = gmax, gavg
    out_dir = similarity.write_baselines(args.output_dir, args.group, outputs)
    write_tags(out_dir, tags)
    res.update(outputs=outputs, group_indices=group_indices, dir=out_dir)
    return res


def main(args, backend=None):
    return run(args, (PIXEL, CLIP), backend)


if __name__ == "__main__":
    main(parse_args())
    print("Done!")
