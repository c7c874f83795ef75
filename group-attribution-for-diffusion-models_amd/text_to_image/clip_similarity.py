"""CLIP-similarity baseline for the text-to-image experiment (entry point kept from the reference
text_to_image/clip_similarity.py): the CLIP half of baselines.py - same flags, `{group}_{max,avg}_clip_similarity.npy` and
their rank files.  Needs GAD_VAE_DECODER_TS, GAD_CLIP_B32_WEIGHTS (or GAD_SD_SCORER=clip-seeded) and --train_pixels, or none of
them (stand-ins); see baselines.py."""
import os
import sys

_HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

from text_to_image import baselines  # noqa: E402


def parse_args(argv=None):
    return baselines.parse_args(argv, description="Run the CLIP similarity baseline for data attribution.")


def main(args, backend=None):
    return baselines.run(args, (baselines.CLIP,), backend)


if __name__ == "__main__":
    main(parse_args())
    print("Done!")
