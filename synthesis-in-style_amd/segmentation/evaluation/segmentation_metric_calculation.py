"""Scores from a confusion matrix (reference: segmentation/evaluation/segmentation_metric_calculation.py).

Rows of the matrix are ground-truth classes, columns predicted classes.  The reference fills a float32 matrix with one masked
reduction and one device-to-host copy per cell, adds the pages' matrices in float32 (which stops counting exactly above 2^24
pixels in a cell) and divides in float32.  Here the matrix is the int64 one ``sis_hip.confusion_matrix`` accumulates on the
device; it crosses to the host once and every score is computed in float64 from the integers.  Names, the returned layout and
the rule "0 / 0 is a correct prediction, score 1.0" are the reference's.
"""
from typing import Dict, List

import torch

import sis_hip


def _counts(confusion_matrix):
    """[C][C] Python ints (exact for every pixel count)."""
    return torch.as_tensor(confusion_matrix).detach().cpu().to(torch.int64).tolist()


def _ratio(numerator: int, denominator: int) -> float:
    if denominator == 0:   # the class is neither in the ground truth nor in the prediction: the prediction was correct
        return 1.0
    return float(numerator) / float(denominator)


def _parts(confusion_matrix, class_idx: int):
    m = _counts(confusion_matrix)
    true_positives = m[class_idx][class_idx]
    predicted_positives = sum(row[class_idx] for row in m)
    actual_positives = sum(m[class_idx])
    return true_positives, predicted_positives, actual_positives


def calculate_dice_score(confusion_matrix, class_idx: int) -> float:
    tp, predicted, actual = _parts(confusion_matrix, class_idx)
    return _ratio(2 * tp, predicted + actual)


def calculate_iou(confusion_matrix, class_idx: int) -> float:
    tp, predicted, actual = _parts(confusion_matrix, class_idx)
    return _ratio(tp, predicted + actual - tp)


def calculate_precision(confusion_matrix, class_idx: int) -> float:
    tp, predicted, _ = _parts(confusion_matrix, class_idx)
    return _ratio(tp, predicted)


def calculate_recall(confusion_matrix, class_idx: int) -> float:
    tp, _, actual = _parts(confusion_matrix, class_idx)
    return _ratio(tp, actual)


IMPLEMENTED_METRICS = {
    "dice": calculate_dice_score,
    "iou": calculate_iou,
    "precision": calculate_precision,
    "recall": calculate_recall,
}


def calculate_confusion_matrix(assembled_prediction: torch.Tensor, ground_truth_classes: torch.Tensor, num_classes: int,
                               out: torch.Tensor = None) -> torch.Tensor:
    """int64 [C, C] on the device from [C, H, W] confidences (first maximal class, like ``torch.argmax``) and a uint8 [H, W]
    ground-truth class map; ``out`` accumulates."""
    assert tuple(assembled_prediction.shape[-2:]) == tuple(ground_truth_classes.shape), \
        'Shapes of prediction and ground truth do not match'
    return sis_hip.confusion_matrix(assembled_prediction, ground_truth_classes, num_classes, out=out)


def calculate_metric(confusion_matrix, class_names: List[str], metric: str = "dice") -> Dict[str, Dict[str, float]]:
    assert metric in IMPLEMENTED_METRICS.keys(), \
        f"Metric to calculate must be in {', '.join(m for m in IMPLEMENTED_METRICS.keys())}"
    m = _counts(confusion_matrix)
    total = sum(sum(row) for row in m)
    scores = {"weighted_avg": {"score": 0.0}, "weighted_text_avg": {"score": 0.0}}
    text_weight = 0.0
    for class_idx, name in enumerate(class_names):
        score = IMPLEMENTED_METRICS[metric](m, class_idx)
        weight = float(sum(m[class_idx])) / float(total)
        if "text" in name:
            text_weight += weight
        scores["weighted_avg"]["score"] += score * weight
        scores[name] = {"score": score, "weight": weight}
    for name in class_names:
        if "text" in name:
            if text_weight > 0:
                scores["weighted_text_avg"]["score"] += scores[name]["score"] * scores[name]["weight"] / text_weight
            else:
                scores["weighted_text_avg"]["score"] = 1.0
    return scores
