"""Golden vectors for the page evaluation, produced by the REFERENCE's own code run in this container on the CPU:
``VotingAssemblySegmenter.assemble_predictions`` (segmentation/analysis_segmenter.py:198-223) on the five patch-grid cases of
make_golden_analysis.py, and ``calculate_metric`` (segmentation/evaluation/segmentation_metric_calculation.py) for all four
metrics on a handful of confusion matrices.  Data only.

    python tests/golden/make_golden_page_eval.py      -> tests/golden/page_eval.npz
"""
import importlib
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle.load_reference import load_reference_analysis_segmenter  # noqa: E402

CASES = [  # (width, height, patch, overlap or None): as in make_golden_analysis.py
    (700, 500, 256, None), (256, 256, 256, None), (513, 300, 256, None), (1000, 777, 256, 64), (300, 520, 128, 100),
]
SEED = 20240
CLASS_NAMES = ["background", "printed_text", "handwritten_text"]
MATRICES = [   # rows ground truth, columns prediction; every total below 2^24
    [[900, 30, 12], [25, 400, 40], [7, 33, 210]],
    [[5000, 0, 0], [0, 0, 0], [0, 0, 0]],                    # two classes absent from ground truth and prediction
    [[1200, 50, 0], [0, 0, 0], [10, 40, 300]],               # a class without ground truth, but predicted
    [[100, 0, 0], [30, 0, 10], [0, 0, 77]],                  # a class never predicted
    [[4000000, 123456, 7], [98765, 3000000, 54321], [11, 2222, 1000000]],
    [[640, 0, 0], [0, 0, 0], [0, 0, 0]],
    [[0, 0, 0], [0, 17, 3], [0, 5, 29]],                     # no background at all
]
METRICS = ["dice", "iou", "precision", "recall"]


def main():
    ref = load_reference_analysis_segmenter()
    out = {"cases": np.asarray([[w, h, p, -1 if o is None else o] for w, h, p, o in CASES], dtype=np.int64),
           "seed": np.asarray(SEED)}
    rng = np.random.RandomState(SEED)
    for i, (w, h, p, o) in enumerate(CASES):
        me = types.SimpleNamespace(patch_size=p, patch_overlap=o, device="cpu", network=types.SimpleNamespace(num_classes=3),
                                   progress_bar=lambda it, **kw: it)
        boxes = ref.AnalysisSegmenter.calculate_bboxes_for_patches(me, w, h)
        preds = torch.from_numpy(rng.rand(len(boxes), 3, p, p).astype(np.float32))
        if i == 2:   # a band without any confidence left, as after post-processing: the 0 / 0 pixels
            preds[:, :, 40:60, :] = 0.0
        patches = [{"prediction": preds[k], "bbox": boxes[k]} for k in range(len(boxes))]
        voted = ref.VotingAssemblySegmenter.assemble_predictions(me, patches, (w, h))
        out[f"voted_sum_{i}"] = np.asarray(voted.double().sum().item())
        out[f"voted_slice_{i}"] = voted[:, ::37, ::41].numpy()
        out[f"voted_rows_{i}"] = voted[:, 40:60:7, ::5].numpy()
        out[f"labels_slice_{i}"] = torch.argmax(voted, dim=0)[::17, ::19].numpy().astype(np.uint8)

    metric_module = importlib.import_module("segmentation.evaluation.segmentation_metric_calculation")
    scores = []
    for matrix in MATRICES:
        m = torch.tensor(matrix, dtype=torch.float32)   # the reference's matrices are float32
        scores.append({metric: metric_module.calculate_metric(m, CLASS_NAMES, metric) for metric in METRICS})
    out["metric_matrices"] = np.asarray(MATRICES, dtype=np.int64)
    out["metric_class_names"] = np.asarray(CLASS_NAMES)
    out["metric_scores_json"] = np.asarray(json.dumps(scores))
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "page_eval.npz"), **out)
    print({k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
