"""Validation of a segmenter during training: one fused pass per batch (``sis_hip.seg_eval``, csrc/seg_eval.h), one copy to the
host per run.

The reference has the hook (``get_evaluator``, train.py:122-124) and leaves it empty for the segmenters
(training_builder/base_train_builder.py:64-65); this goes beyond it.

What is validated is the argmax of the network's RAW logits against the labels of the validation loader.  ``min_confidence`` and
``min_contour_area`` are NOT applied: they belong to the page evaluation (``analyze_image_segments.py``), which thresholds and
filters assembled pages; a validation number during training is about the network alone.

The pass leaves training where it was: it runs under ``torch.no_grad()`` in ``eval()`` mode (no BatchNorm running statistics, no
dropout draws, no dropout counter), never calls an optimizer, never writes ``emau.mu`` (only ``EMANetUpdater`` does), writes no
parameter (so no packed-weight cache goes stale), and restores the previous mode afterwards, also when a batch raises.
"""
import json
from pathlib import Path
from typing import Dict, List, Optional

import torch

import sis_hip
from segmentation.evaluation.segmentation_metric_calculation import IMPLEMENTED_METRICS, calculate_metric
from training.loop import get_current_reporter, reduce_sum

DICE_SMOOTH = 1e-5   # csrc/loss_ops.hip, networks/trans_u_net/utils.py: DiceLoss
REPORT_PREFIX = 'validation'
LOWER_IS_BETTER = ('ce', 'dice_loss')


def scores_from_state(counts, sums, class_names: List[str]) -> Dict[str, float]:
    """The flat dict of a validation run from the accumulated state of ``sis_hip.seg_eval`` (host or device tensors):
    ``<metric>/<class name>``, ``<metric>/weighted_avg`` and ``<metric>/weighted_text_avg`` for dice, iou, precision and recall
    (``calculate_metric`` on the integer matrix), ``pixel_accuracy``, ``ce`` = sums[0] / counted, ``dice_loss`` = the DiceLoss of
    csrc/loss_ops.hip on the accumulated sums in float64, ``counted`` and ``ignored``.  With nothing counted (every label
    ignored) ``ce`` and ``pixel_accuracy`` are 0, every class scores 1.0 by the 0 / 0 rule and the weighted averages, which have
    no weight to go by, are 0."""
    classes = len(class_names)
    counts = torch.as_tensor(counts).detach().cpu().to(torch.int64)
    sums = torch.as_tensor(sums).detach().cpu().to(torch.float64).tolist()
    if counts.numel() != classes * classes + 2 or len(sums) != 1 + 3 * classes:
        raise ValueError(f"state of {counts.numel()} counts and {len(sums)} sums does not belong to {classes} classes")
    matrix = counts[:classes * classes].view(classes, classes)
    counted, ignored = int(counts[classes * classes]), int(counts[classes * classes + 1])
    out = {}
    for metric in IMPLEMENTED_METRICS:
        if counted:
            for name, entry in calculate_metric(matrix, class_names, metric).items():
                out[f"{metric}/{name}"] = float(entry["score"])
        else:
            for class_idx, name in enumerate(class_names):
                out[f"{metric}/{name}"] = IMPLEMENTED_METRICS[metric](matrix, class_idx)
            out[f"{metric}/weighted_avg"] = out[f"{metric}/weighted_text_avg"] = 0.0
    out["pixel_accuracy"] = float(int(matrix.diagonal().sum())) / counted if counted else 0.0
    out["ce"] = sums[0] / counted if counted else 0.0
    dice = 0.0
    for c in range(classes):
        intersect, p_sum, t_sum = sums[1 + 3 * c:4 + 3 * c]
        dice += 1.0 - (2.0 * intersect + DICE_SMOOTH) / (p_sum + t_sum + DICE_SMOOTH)
    out["dice_loss"] = dice / classes
    out["counted"], out["ignored"] = counted, ignored
    return out


def better(metric: str, value: float, best: Optional[float]) -> bool:
    """Does ``value`` STRICTLY improve on ``best``?  ``ce`` and ``dice_loss``: lower is better; every score: higher."""
    if best is None:
        return True
    return value < best if metric in LOWER_IS_BETTER else value > best


def default_eval_iter(config: dict, iterations_per_epoch: int) -> int:
    """``eval_iter`` when given, else ``snapshot_save_iter`` when that is positive, else one epoch."""
    if config.get('eval_iter'):
        return int(config['eval_iter'])
    if config.get('snapshot_save_iter') and config['snapshot_save_iter'] > 0:
        return int(config['snapshot_save_iter'])
    return max(int(iterations_per_epoch), 1)


def validation_due(iteration: int, eval_iter: int, max_iter: int) -> bool:
    """Every ``eval_iter`` iterations and once after the last one -- once, not twice, where the two coincide."""
    return iteration % eval_iter == 0 or iteration == max_iter


class ValidationLog:
    """What rank 0 does with the scores of a run: one line on stdout, one JSON line appended to ``<log_dir>/validation.jsonl``,
    and ``<log_dir>/best.pt`` (snapshot layout) whenever ``best_metric`` strictly improves."""
    LINE_KEYS = ('dice/weighted_avg', 'iou/weighted_avg', 'pixel_accuracy', 'ce')

    def __init__(self, log_dir, best_metric: str = 'dice/weighted_avg', snapshotter=None):
        self.log_dir, self.best_metric, self.snapshotter = Path(log_dir), best_metric, snapshotter
        self.best = None

    def record(self, iteration: int, scores: Dict[str, float], final: bool = False) -> bool:
        """-> whether ``best.pt`` was written."""
        if self.best_metric not in scores:
            raise KeyError(f"best_metric '{self.best_metric}' is not a validation score ({', '.join(sorted(scores))})")
        print(f"validation iter {iteration} " + " ".join(f"{k}={scores[k]:.5f}" for k in self.LINE_KEYS), flush=True)
        self.log_dir.mkdir(parents=True, exist_ok=True)
        with open(self.log_dir / 'validation.jsonl', 'a') as f:
            f.write(json.dumps({'iteration': iteration, 'final': bool(final), **scores}) + '\n')
        improved = better(self.best_metric, scores[self.best_metric], self.best)
        if improved:
            self.best = scores[self.best_metric]
            if self.snapshotter is not None:
                self.snapshotter.save_as('best.pt')
        return improved


def _unwrap(network):
    return network.module if hasattr(network, 'module') and isinstance(network.module, torch.nn.Module) else network


class SegmentationValidator:
    """``run()``: the whole validation loader through the network in evaluation mode, one ``seg_eval`` per batch, no host
    synchronisation inside the loop, the state summed over the ranks and copied to the host once -> ``scores_from_state``,
    reported under ``validation/``.  Every run starts the loader at its epoch 0, so all runs of a training see the same pages."""

    def __init__(self, network, loader, class_names, device, amp=None):
        self.network, self.loader, self.class_names = network, loader, list(class_names)
        self.device = torch.device(device)
        self.amp_dtype = {'bf16': torch.bfloat16, 'fp16': torch.float16}.get(amp)
        self.last_counts = self.last_sums = None   # the summed state of the last run, on the host

    def batch_logits(self, network, images):
        """The logits ``seg_eval`` is given: EMANet's at their native 1 / 8 size (the kernel interpolates them, as the training
        loss does), the full-size output of the others in the dtype their head wrote."""
        from networks.ema_net.network import EMANet
        if isinstance(network, EMANet):
            return network.eval_logits(images)
        with torch.autocast(device_type='cuda', dtype=self.amp_dtype or torch.bfloat16, enabled=self.amp_dtype is not None):
            return network(images)

    def run(self) -> Dict[str, float]:
        network = _unwrap(self.network)
        was_training = network.training
        classes = len(self.class_names)
        counts, sums = sis_hip.seg_eval_state(classes, self.device)
        if hasattr(self.loader, 'set_epoch'):
            self.loader.set_epoch(0)
        # A replayed step hipGraph moves the weights without moving their stamps (training/graph_step.py): whatever a layer
        # derived from them in an earlier eager forward (bf16 copies nobody else keeps current) is declared out of date here.
        sis_hip.mark_written(network)
        network.eval()
        try:
            with torch.no_grad():
                for batch in self.loader:
                    images = batch['images'].to(self.device, non_blocking=True)
                    labels = batch['segmented'].to(self.device, non_blocking=True)
                    logits = self.batch_logits(network, images)
                    if logits.shape[1] != classes:
                        raise RuntimeError(f"the network predicts {logits.shape[1]} classes, the colour map names {classes}")
                    if logits.dtype not in (torch.float32, torch.bfloat16):
                        logits = logits.float()
                    sis_hip.seg_eval(logits, labels, counts=counts, sums=sums)
        finally:
            network.train(was_training)
        counts, sums = reduce_sum(counts), reduce_sum(sums)
        packed = torch.cat([counts, sums.view(torch.int64)]).cpu()   # the one copy to the host: the doubles travel as their bits
        self.last_counts, self.last_sums = packed[:counts.numel()], packed[counts.numel():].view(torch.float64)   # on the host
        scores = scores_from_state(self.last_counts, self.last_sums, self.class_names)
        get_current_reporter().add_observation(scores, REPORT_PREFIX)
        return scores
