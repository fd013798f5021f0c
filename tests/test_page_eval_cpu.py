"""Page evaluation, the parts that need no device:
* the restatement's two area formulas -- 2x2 blocks, and the shoelace area of the traced outer border -- agree on hand-made and
  random regions, so the block rule the kernel uses is tested and not assumed;
* the metrics module equals the reference-made golden (tests/golden/page_eval.npz) within 1e-6 relative: the reference divides
  in float32, the module in float64;
* ``create_hyperparam_configs`` and the ``results.json`` layout;
* header / ctypes table agree on the new symbols; the product imports neither scipy nor cv2; CPU tensors raise.
"""
import argparse
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import page_eval_restatement as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "synthesis-in-style_amd")
NEW_SYMBOLS = ["sis_assemble_vote", "sis_confusion_matrix", "sis_color_to_class", "sis_contour_workspace_bytes",
               "sis_remove_small_contours"]


@pytest.mark.parametrize("name", sorted(R.hand_made_masks()))
def test_area_formulas_agree_on_hand_made_masks(name):
    mask = R.hand_made_masks()[name]
    labels, count = R.regions(mask)
    assert count == 1
    region = labels == 1
    blocks, shoelace = R.twice_area_blocks(region), R.twice_area_shoelace(region)
    assert blocks == shoelace
    expected = {"single": 0, "line": 0, "diagonal": 0, "ring_with_island": 2 * 11 * 11, "edge": None}[name]
    if expected is not None:
        assert blocks == expected
    if name == "ring_with_island":   # the hole and the island in it belong to the region
        assert region.sum() == 12 * 12


@pytest.mark.parametrize("seed", range(6))
def test_area_formulas_agree_on_random_regions(seed):
    rng = np.random.RandomState(seed)
    checked = 0
    for trial in range(12):
        if trial % 3 == 0:
            mask = R.closed_mask(R.smooth_noise_planes(rng, (48, 48), 0.15, 1.5))
        else:
            mask = rng.rand(40, 40) < rng.choice([0.1, 0.3, 0.45, 0.6])
        labels, count = R.regions(mask)
        for k in range(1, count + 1):
            assert R.twice_area_blocks(labels == k) == R.twice_area_shoelace(labels == k), (seed, trial, k)
            checked += 1
    assert checked > 50


def test_restated_filter_on_a_known_plane():
    """A 3x3 square (area 4) goes at threshold 5 and stays at 4; a thin line goes at any positive threshold; the background
    plane only gets the confidence threshold."""
    pred = np.zeros((1, 2, 32, 32), dtype=np.float32)
    pred[0, 1, 4:7, 4:7] = 0.9
    pred[0, 1, 26, 3:29] = 0.8
    pred[0, 1, 10:20, 10:20] = 0.75
    pred[0, 1, 30, 30] = 0.5   # below the confidence threshold
    pred[0, 0] = 0.6
    out = R.remove_small_contours(pred, 0.7, 5, 0).numpy()
    assert (out[0, 0] == 0).all()
    assert (out[0, 1, 4:7, 4:7] == 0).all() and (out[0, 1, 26] == 0).all() and out[0, 1, 30, 30] == 0
    assert (out[0, 1, 10:20, 10:20] == np.float32(0.75)).all()
    out = R.remove_small_contours(pred, 0.7, 4, 0).numpy()
    assert (out[0, 1, 4:7, 4:7] == np.float32(0.9)).all() and (out[0, 1, 26] == 0).all()
    out = R.remove_small_contours(pred, 0.7, 5, 1).numpy()   # class 1 is the background now: untouched by the filter
    assert (out[0, 1, 4:7, 4:7] == np.float32(0.9)).all() and (out[0, 1, 26, 3:29] == np.float32(0.8)).all()


def _close(got, want, path=""):
    if isinstance(want, dict):
        assert sorted(got) == sorted(want), path
        for k in want:
            _close(got[k], want[k], f"{path}/{k}")
    else:
        assert got == pytest.approx(want, rel=1e-6, abs=0.0), path


def test_metrics_match_the_reference_golden(golden_dir):
    from segmentation.evaluation.segmentation_metric_calculation import IMPLEMENTED_METRICS, calculate_metric
    g = np.load(os.path.join(golden_dir, "page_eval.npz"))
    names = [str(n) for n in g["metric_class_names"]]
    want = json.loads(str(g["metric_scores_json"]))
    assert sorted(IMPLEMENTED_METRICS) == ["dice", "iou", "precision", "recall"]
    for matrix, scores in zip(g["metric_matrices"], want):
        assert matrix.sum() < 2 ** 24
        for metric in IMPLEMENTED_METRICS:
            got = calculate_metric(torch.from_numpy(matrix), names, metric)
            assert list(got)[:2] == ["weighted_avg", "weighted_text_avg"] and list(got)[2:] == names
            _close(got, scores[metric], metric)
            assert got == R.calculate_metric(matrix, names, metric)
            for k, name in enumerate(names):
                assert IMPLEMENTED_METRICS[metric](torch.from_numpy(matrix), k) == got[name]["score"]


def test_metrics_count_exactly_above_two_to_the_24():
    from segmentation.evaluation.segmentation_metric_calculation import calculate_metric
    big = torch.tensor([[2 ** 24 + 1, 1], [0, 1]], dtype=torch.int64)
    got = calculate_metric(big, ["background", "text"], "precision")
    assert got["background"]["score"] == 1.0 and got["text"]["score"] == 0.5
    assert got["background"]["weight"] == (2 ** 24 + 2) / (2 ** 24 + 3)
    with pytest.raises(AssertionError):
        calculate_metric(big, ["background", "text"], "accuracy")


def test_hyperparam_configs_are_the_reference_product():
    from segmentation.evaluation.analyze_image_segments import build_parser, create_hyperparam_configs
    args = build_parser().parse_args(["pages", "-cds", "-gt", "gt", "--min-confidence", "0.5", "0.7", "--min-contour-area", "0",
                                      "55", "--patch-overlap-factor", "0.25", "0.5"])
    configs = create_hyperparam_configs(args)
    assert configs == tuple({"min_confidence": c, "min_contour_area": a, "patch_overlap": (0, f)}
                            for c in (0.5, 0.7) for a in (0, 55) for f in (0.25, 0.5))
    defaults = create_hyperparam_configs(build_parser().parse_args(["pages"]))
    assert defaults == ({"min_confidence": 0.7, "min_contour_area": 55, "patch_overlap": (0, 0.0)},)
    args = build_parser().parse_args(["pages", "--absolute-patch-overlap", "32", "64"])
    assert [c["patch_overlap"] for c in create_hyperparam_configs(args)] == [(32, 0.0), (64, 0.0)]
    with pytest.raises(SystemExit):
        build_parser().parse_args(["pages", "--absolute-patch-overlap", "32", "--patch-overlap-factor", "0.5"])


def test_visual_flags_raise_and_metrics_are_required():
    from segmentation.evaluation.analyze_image_segments import parse_and_check_arguments
    with pytest.raises(NotImplementedError, match="--visualize-segmentation"):
        parse_and_check_arguments(["pages", "-cds", "-gt", "gt", "-vis"])
    with pytest.raises(NotImplementedError, match="--save-contours"):
        parse_and_check_arguments(["pages", "-cds", "-gt", "gt", "--save-contours"])
    with pytest.raises(SystemExit):
        parse_and_check_arguments(["pages", "-gt", "gt"])
    with pytest.raises(SystemExit):
        parse_and_check_arguments(["pages", "-cio"])
    args = parse_and_check_arguments(["pages", "-cio", "-cre", "-gt", "gt", "-o", "out", "--handle-existing", "append", "--resize",
                                      "-1", "800", "-bw"])
    assert args.calculate_iou and args.calculate_recall and not args.calculate_dice_score and args.resize == [-1, 800]


def test_results_json_layout(tmp_path):
    from segmentation.evaluation.analyze_image_segments import prepare_results
    path = tmp_path / "results.json"
    colors = {"background": [0, 0, 0], "printed_text": [255, 0, 0]}
    results = prepare_results("abort", path, {"checkpoint": "a.pt"}, {"network": "DocUFCN"}, colors)
    assert results == {"general_config": {"experiment_config": {"checkpoint": "a.pt"}, "model_config": {"network": "DocUFCN"},
                                          "class_to_color_map": colors}, "runs": []}
    results["runs"].append({"hyperparams": {"min_confidence": 0.7}})
    path.write_text(json.dumps(results))
    with pytest.raises(AssertionError):
        prepare_results("abort", path, {"checkpoint": "a.pt"}, {"network": "DocUFCN"}, colors)
    again = prepare_results("append", path, {"checkpoint": "a.pt"}, {"network": "DocUFCN"}, colors)
    assert len(again["runs"]) == 1
    with pytest.raises(AssertionError):
        prepare_results("append", path, {"checkpoint": "b.pt"}, {"network": "DocUFCN"}, colors)
    assert prepare_results("overwrite", path, {"checkpoint": "b.pt"}, {}, colors)["runs"] == []


def test_class_id_map():
    from utils.segmentation_utils import get_class_id_map
    colors = {"printed_text": [255, 0, 0], "background": [0, 0, 0], "handwritten_text": [0, 0, 255]}
    assert get_class_id_map("background", colors) == {"background": 0, "printed_text": 1, "handwritten_text": 2}
    assert get_class_id_map("background", colors) == R.class_id_map("background", colors)
    with pytest.raises(KeyError):
        get_class_id_map("paper", colors)


def test_header_and_ctypes_table_agree_on_the_new_symbols():
    import sis_hip
    text = open(os.path.join(ROOT, "include", "sis_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(sis_[a-z0-9_]+)\s*\(", text))
    for name in NEW_SYMBOLS:
        assert name in declared and name in sis_hip.exported_symbols(), name
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, text).group(1)
        assert len(sis_hip._SIGNATURES[name][0]) == len([a for a in decl.split(",") if a.strip()]), name
        assert hasattr(sis_hip.lib(), name)


PAGE_EVAL_MODULES = ["networks/base_segmenter.py", "segmentation/analysis_segmenter.py", "utils/segmentation_utils.py",
                     "segmentation/evaluation/__init__.py", "segmentation/evaluation/segmentation_metric_calculation.py",
                     "segmentation/evaluation/analyze_image_segments.py", "sis_hip/__init__.py"]


def test_product_imports_neither_scipy_nor_cv2():
    """Every module the page evaluation runs through.  cv2 is named nowhere in the product; scipy only by the ViT checkpoint
    import (networks/trans_u_net/npz_import.py, a lazy import for resizing position embeddings), which is not on this path."""
    for rel in PAGE_EVAL_MODULES:
        text = open(os.path.join(SRC, rel)).read()
        assert not re.search(r"^\s*(from|import)\s+(scipy|cv2)\b", text, flags=re.M), rel
    for dirpath, _, files in os.walk(SRC):
        for f in files:
            if f.endswith(".py"):
                text = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+cv2\b", text, flags=re.M), os.path.join(dirpath, f)
    code = ("import sys; import networks.base_segmenter, segmentation.analysis_segmenter, utils.segmentation_utils, "
            "segmentation.evaluation.analyze_image_segments; "
            "assert not [m for m in sys.modules if m.split('.')[0] in ('scipy', 'cv2')]")
    import subprocess
    subprocess.run([sys.executable, "-c", code], check=True, cwd=SRC, env={**os.environ, "PYTHONPATH": SRC})


def test_cpu_tensors_raise_instead_of_falling_back():
    import sis_hip
    from networks.base_segmenter import BaseSegmenter
    from segmentation.analysis_segmenter import AnalysisSegmenter, VotingAssemblySegmenter
    x = torch.rand(1, 3, 16, 16)
    with pytest.raises(NotImplementedError):
        BaseSegmenter(min_contour_area=55).postprocess(x)
    kept = BaseSegmenter(min_confidence=0.5).postprocess(x)   # the threshold alone stays a tensor op on any device
    assert torch.equal(kept, torch.where(x < 0.5, torch.zeros_like(x), x))
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        sis_hip.remove_small_contours(x, 0.5, 55, 0)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        sis_hip.assemble_vote(x, [0], [0], 16, 16)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        sis_hip.confusion_matrix(x[0], torch.zeros(16, 16, dtype=torch.uint8), 3)
    assert issubclass(VotingAssemblySegmenter, AnalysisSegmenter)
