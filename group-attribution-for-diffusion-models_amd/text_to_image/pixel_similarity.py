"""Pixel-similarity baseline for the text-to-image experiment (entry point kept from the reference
text_to_image/pixel_similarity.py): the pixel half of baselines.py - same flags, `{group}_{max,avg}_pixel_similarity.npy` and
their rank files.  Needs GAD_VAE_DECODER_TS and --train_pixels, or neither (stand-ins); see baselines.py."""
import os
import sys

_HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

from text_to_image import baselines  # noqa: E402


def parse_args(argv=None):
    return baselines.parse_args(argv, description="Run the pixel similarity baseline for data attribution.")


def main(args, backend=None):
    return baselines.run(args, (baselines.PIXEL,), backend)


if __name__ == "__main__":
    main(parse_args())
    print("Done!")
