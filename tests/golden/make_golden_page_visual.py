"""Golden vectors for the page colouring, produced by the REFERENCE's own ``network_output_to_color_image``
(visualization/utils.py:29-68, reached through the reference's analysis_segmenter module; the function never calls cv2) run in
this container on the CPU, in the plain and in the confidence mode, on two small planes that hold ties between classes,
all-zero pixels, a maximum below 0.01 and a maximum of exactly 1.0.  Data only.

    python tests/golden/make_golden_page_visual.py      -> tests/golden/page_visual.npz
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle.load_reference import load_reference_analysis_segmenter  # noqa: E402

SEED = 20261
CASES = [   # (shape, class -> colour); the background class comes first, as the reference's class-id map has it
    ((1, 3, 24, 40), {"background": "#000000", "printed_text": "#0000FF", "handwritten_text": "#FF0000"}),
    ((1, 4, 17, 9), {"background": "#101010", "printed_text": "#00C800", "handwritten_text": "#FF8000", "stamp": "#7F00FF"}),
]


def make_input(rng, shape):
    _, classes, height, width = shape
    x = rng.rand(*shape).astype(np.float32)
    x[0, :, rng.rand(height, width) < 0.35] = 0.0                       # all-zero pixels
    weak = rng.rand(height, width) < 0.15                               # only the background has a confidence
    x[0, 1:, weak] = 0.0
    ys, xs = np.nonzero(rng.rand(height, width) < 0.12)                 # ties: two (or all) classes share the maximum
    for n, (y, xx) in enumerate(zip(ys, xs)):
        a, b = n % classes, (n + 1 + n // classes) % classes
        top = np.float32(0.25 + 0.5 * rng.rand())
        x[0, :, y, xx] = np.minimum(x[0, :, y, xx], top)
        x[0, a, y, xx] = x[0, b, y, xx] = top
        if n % 5 == 0:
            x[0, :, y, xx] = top
    x[0, :, 1, 1] = 0.0
    x[0, classes - 1, 1, 1] = 0.004                                     # a maximum below 0.01: gradient index -1
    x[0, :, 2, 3] = 0.0
    x[0, 1, 2, 3] = 0.0099999
    x[0, :, 3, 2] = 0.3
    x[0, 1, 3, 2] = 1.0                                                 # a maximum of exactly 1.0: gradient index 99
    x[0, :, 4, 4] = 0.0
    x[0, classes - 1, 4, 4] = 1.0
    x[0, :, 5, 5] = [0.6] + [0.2] * (classes - 1)                       # the background wins, the others still vote
    return x


def main():
    ref = load_reference_analysis_segmenter()
    colour_image = sys.modules["visualization.utils"].network_output_to_color_image
    rng = np.random.RandomState(SEED)
    out = {"seed": np.asarray(SEED), "class_maps_json": np.asarray(json.dumps([colours for _, colours in CASES]))}
    for i, (shape, colours) in enumerate(CASES):
        x = make_input(rng, shape)
        out[f"input_{i}"] = x
        for mode, confidence in (("plain", False), ("confidence", True)):
            image = colour_image(torch.from_numpy(x), colours, show_confidence_in_segmentation=confidence)
            out[f"{mode}_{i}"] = (image[0] * 255).round().to(torch.uint8).permute(1, 2, 0).contiguous().numpy()
    assert ref is not None
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "page_visual.npz"), **out)
    print({k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
