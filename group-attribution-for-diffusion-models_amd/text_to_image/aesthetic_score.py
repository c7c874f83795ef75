"""Aesthetic score of every training image as a global baseline (entry point kept from the reference
text_to_image/aesthetic_score.py): same flags, and under `{output_dir}/baselines` the reference's files - `image_aesthetic_score.npy`
(float32 [N]), `aesthetic_score_{group}_indices_dict.pkl` (a plain dict of int -> int64 index array),
`{group}_{max,avg}_aesthetic_score.npy` ([groups, 1] float64) and `all_generated_images_{group}_rank_{name}.npy` (:137-176).

Nothing is generated, so no U-Net and no decoder.  With GAD_CLIP_L14_WEIGHTS + GAD_AESTHETIC_WEIGHTS (or GAD_SD_SCORER=clip-seeded)
and --train_pixels, the open-CLIP ViT-L-14 tower and LAION's head run on the HIP operators (gad/vit.py) over the uint8 images
resident on the device, --batch_size at a time.  With none of them, the LatentScorer stand-in scores the cached latents and
`baselines/feature_extractor.json` says so.  Engine extras: --device, --train_data_dir, --synthetic_cache, --train_pixels,
--resolution (the side of --train_pixels / of a synthetic cache); `main(args, backend=None)`."""
import os
import pickle
import sys

import numpy as np
import torch

_HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

from text_to_image import baselines  # noqa: E402
from text_to_image.compute_model_behaviors import LatentScorer  # noqa: E402

NAME = "aesthetic_score"


def parse_args(argv=None):
    return baselines.parse_args(argv, description="Compute aesthetic score for each training image.", batch_size=1024, workers=2,
                                generate=False)


def main(args, backend=None):
    from gad import _capi, similarity
    settings = baselines.network_settings(["GAD_CLIP_L14_WEIGHTS", "GAD_AESTHETIC_WEIGHTS"], args.train_pixels, NAME)
    latents, group_indices, _ = baselines.load_training_side(args)
    train_px = baselines.load_train_pixels(args.train_pixels, len(latents), args.resolution) if settings is not None else None
    device = torch.device(args.device)
    if device.type != "cuda":
        raise _capi.GadError(f"--device {args.device}: the aesthetic scores run on the GPU (there is no CPU path)")
    with torch.no_grad():
        if settings is None:
            scorer, lat = LatentScorer(device), latents.to(device)
            e = torch.cat([scorer.embed(lat[s:s + args.batch_size]).reshape(-1, scorer.head.numel())
                           for s in range(0, len(lat), args.batch_size)], 0)
            scores, tag = e @ scorer.head, LatentScorer.TAG
        else:
            from gad import vit
            l14_path, head_path = settings["GAD_CLIP_L14_WEIGHTS"], settings["GAD_AESTHETIC_WEIGHTS"]
            l14 = (vit.VisionTower.from_file(l14_path, "clip_vit_l14") if l14_path else vit.VisionTower.seeded("clip_vit_l14")).to(device)
            head = (vit.AestheticHead.from_file(l14, head_path) if head_path else vit.AestheticHead.seeded(l14)).to(device)
            train_u8 = torch.from_numpy(train_px).to(device)
            scores = torch.cat([head(baselines.images01(train_u8[s:s + args.batch_size]))
                                for s in range(0, len(train_u8), args.batch_size)], 0)
            tag = f"{l14.tag};{head.tag}"
    scores = scores.flatten().cpu().numpy().astype(np.float32)
    gmax, gavg = similarity.group_aggregate(scores, group_indices)
    out_dir = similarity.write_baselines(args.output_dir, args.group, {f"max_{NAME}": gmax, f"avg_{NAME}": gavg}, per_image=False)
    np.save(os.path.join(out_dir, "image_aesthetic_score.npy"), scores)
    with open(os.path.join(out_dir, f"aesthetic_score_{args.group}_indices_dict.pkl"), "wb") as handle:
        pickle.dump({int(i): np.asarray(idx, dtype=np.int64) for i, idx in enumerate(group_indices)}, handle)
    baselines.write_tags(out_dir, {NAME: tag})
    return {"scores": scores, "outputs": {f"max_{NAME}": gmax, f"avg_{NAME}": gavg}, "group_indices": group_indices, "dir": out_dir}


if __name__ == "__main__":
    main(parse_args())
    print("Done!")
