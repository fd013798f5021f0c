"""Validation during training, the parts that need no device: the ``--eval-iter`` option and its default, the
direction of ``best_metric``, the ``validation/`` reporter keys and the rank-0 log, ``get_evaluator``, the restatement against
torch's float64 operators on the exact-scale cases, and the two new entries of the C ABI."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import seg_eval_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = {"sis_seg_eval_workspace_bytes", "sis_seg_eval"}
NEW_KERNELS = {"seg_eval_kernel", "seg_eval_finish_kernel"}
NAMES = ["background", "printed_text", "handwritten_text", "stamp"]
METRICS = ("dice", "iou", "precision", "recall")
DOCUMENTED_KEYS = {f"{m}/{n}" for m in METRICS for n in NAMES + ["weighted_avg", "weighted_text_avg"]} | \
    {"pixel_accuracy", "ce", "dice_loss", "counted", "ignored"}


def test_parse_args_knows_eval_iter():
    import train
    args = train.parse_args(["cfg.yaml", "--val-images", "val.json", "--eval-iter", "7"])
    assert args.eval_iter == 7 and args.validation_json == "val.json"
    assert train.parse_args(["cfg.yaml"]).eval_iter is None
    config = train.merge_config_and_args({"eval_iter": 3, "best_metric": "ce"}, train.parse_args(["cfg.yaml"]))
    assert config["eval_iter"] == 3 and config["best_metric"] == "ce"      # the config key stands when the flag is absent


def test_default_interval_rule():
    from training.validation import default_eval_iter
    assert default_eval_iter({"eval_iter": 5, "snapshot_save_iter": 100}, 40) == 5
    assert default_eval_iter({"eval_iter": None, "snapshot_save_iter": 100}, 40) == 100
    assert default_eval_iter({"snapshot_save_iter": 0}, 40) == 40
    assert default_eval_iter({"snapshot_save_iter": -1}, 40) == 40
    assert default_eval_iter({}, 40) == 40 and default_eval_iter({}, 0) == 1


def test_validation_schedule():
    """Every ``eval_iter`` iterations and once after the last: --eval-iter 2 gives 2, 4 and the final 5 of five iterations, and
    2, 4 of four -- the pass after the last iteration is not run twice."""
    from training.validation import validation_due
    assert [it for it in range(1, 6) if validation_due(it, 2, 5)] == [2, 4, 5]
    assert [it for it in range(1, 5) if validation_due(it, 2, 4)] == [2, 4]
    assert [it for it in range(1, 4) if validation_due(it, 100, 3)] == [3]


def test_best_metric_direction():
    from training.validation import better
    assert better("dice/weighted_avg", 0.1, None) and better("ce", 5.0, None)
    assert better("dice/weighted_avg", 0.6, 0.5) and not better("dice/weighted_avg", 0.5, 0.5) and not better("iou/stamp", 0.4, 0.5)
    assert better("ce", 0.4, 0.5) and not better("ce", 0.5, 0.5) and not better("ce", 0.6, 0.5)
    assert better("dice_loss", 0.1, 0.2) and better("pixel_accuracy", 0.9, 0.8)


def _state(rng, classes=4, shape=(2, 9, 11)):
    logits = rng.standard_normal((shape[0], classes) + shape[1:]).astype(np.float32)
    labels = R.labels_with_ignored(rng, shape, classes)
    return logits, labels, R.reference(logits, labels)


def test_scores_from_state():
    from segmentation.evaluation.segmentation_metric_calculation import calculate_metric
    from training.validation import scores_from_state
    logits, labels, ref = _state(np.random.default_rng(1))
    scores = scores_from_state(torch.from_numpy(ref.counts), torch.from_numpy(ref.sums), NAMES)
    assert set(scores) == DOCUMENTED_KEYS
    matrix = ref.counts[:16].reshape(4, 4)
    for metric in METRICS:
        for name, entry in calculate_metric(torch.from_numpy(matrix), NAMES, metric).items():
            assert scores[f"{metric}/{name}"] == entry["score"]
    assert scores["counted"] == ref.counts[16] and scores["ignored"] == ref.counts[17] and scores["ignored"] > 0
    assert scores["pixel_accuracy"] == np.trace(matrix) / ref.counts[16]
    x, lab = torch.from_numpy(logits).double(), torch.from_numpy(np.where((labels >= 0) & (labels < 4), labels, -100))
    assert scores["ce"] == pytest.approx(torch.nn.functional.cross_entropy(x, lab, ignore_index=-100).item(), rel=1e-12)
    p = torch.softmax(x, dim=1)
    onehot = torch.stack([torch.from_numpy(labels == c) for c in range(4)], dim=1).double()
    dice = sum(1 - (2 * (p[:, c] * onehot[:, c]).sum() + 1e-5) / ((p[:, c] ** 2).sum() + onehot[:, c].sum() + 1e-5) for c in range(4)) / 4
    assert scores["dice_loss"] == pytest.approx(dice.item(), rel=1e-12)
    # every label ignored: nothing is counted, ce is 0 and nothing is NaN
    empty = R.reference(logits, np.full(labels.shape, 255))
    scores = scores_from_state(empty.counts, empty.sums, NAMES)
    assert scores["ce"] == 0.0 and scores["pixel_accuracy"] == 0.0 and scores["counted"] == 0 and scores["dice/weighted_avg"] == 0.0
    assert scores["dice/stamp"] == 1.0 and all(np.isfinite(v) for v in scores.values())
    with pytest.raises(ValueError, match="3 classes"):
        scores_from_state(ref.counts, ref.sums, NAMES[:3])


class _Head(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Conv2d(3, 4, 1)
        self.drop = torch.nn.Dropout(0.5)
        self.modes = []

    def forward(self, x):
        self.modes.append((self.training, torch.is_grad_enabled()))
        return self.drop(self.conv(x))


def _fake_seg_eval(logits, labels, size=None, counts=None, sums=None):
    ref = R.reference(logits.numpy(), labels[:, 0].numpy())
    counts += torch.from_numpy(ref.counts)
    sums += torch.from_numpy(ref.sums)
    return counts, sums


def test_validator_plumbing_and_reporter_keys(monkeypatch):
    """``SegmentationValidator.run()`` on the CPU with the kernel call replaced by the restatement: evaluation mode under no_grad,
    the previous mode restored (also when a batch raises), the loader rewound, the scalars under ``validation/``."""
    import sis_hip
    from training.loop import get_current_reporter
    from training.validation import SegmentationValidator
    monkeypatch.setattr(sis_hip, "seg_eval", _fake_seg_eval)
    rng = np.random.default_rng(2)
    batches = [{"images": torch.from_numpy(rng.standard_normal((2, 3, 5, 7)).astype(np.float32)),
                "segmented": torch.from_numpy(R.labels_with_ignored(rng, (2, 1, 5, 7), 4))} for _ in range(3)]

    class Loader(list):
        epochs = []

        def set_epoch(self, epoch):
            self.epochs.append(epoch)

    net = _Head().train()
    validator = SegmentationValidator(net, Loader(batches), NAMES, "cpu")
    get_current_reporter().observations.clear()
    scores = validator.run()
    assert net.modes == [(False, False)] * 3 and net.training and Loader.epochs == [0]
    assert set(scores) == DOCUMENTED_KEYS and scores["counted"] + scores["ignored"] == 3 * 2 * 5 * 7
    assert set(get_current_reporter().scalars()) == {f"validation/{k}" for k in DOCUMENTED_KEYS}
    with torch.no_grad():
        want = np.zeros(18, dtype=np.int64)
        for b in batches:
            want += R.reference(net.eval().conv(b["images"]).numpy(), b["segmented"][:, 0].numpy()).counts
    assert scores["counted"] == want[16] and scores["pixel_accuracy"] == want[:16].reshape(4, 4).trace() / want[16]
    net.eval()
    validator.run()
    assert not net.training                                        # an evaluation-mode network stays in evaluation mode
    net.train()
    monkeypatch.setattr(sis_hip, "seg_eval", lambda *a, **k: (_ for _ in ()).throw(RuntimeError("batch failed")))
    with pytest.raises(RuntimeError, match="batch failed"):
        validator.run()
    assert net.training
    get_current_reporter().observations.clear()


def test_validation_log(tmp_path, capsys):
    from training.validation import ValidationLog, scores_from_state
    _, _, ref = _state(np.random.default_rng(3))
    scores = scores_from_state(ref.counts, ref.sums, NAMES)

    class Snap:
        saved = []

        def save_as(self, name):
            self.saved.append(name)

    log = ValidationLog(tmp_path / "logs", "ce", Snap())
    assert log.record(2, scores) and not log.record(4, scores) and log.record(5, {**scores, "ce": scores["ce"] / 2}, final=True)
    assert Snap.saved == ["best.pt", "best.pt"]
    lines = [json.loads(line) for line in (tmp_path / "logs" / "validation.jsonl").read_text().splitlines()]
    assert [(r["iteration"], r["final"]) for r in lines] == [(2, False), (4, False), (5, True)]
    assert set(lines[0]) == DOCUMENTED_KEYS | {"iteration", "final"}
    out = capsys.readouterr().out.splitlines()
    assert len(out) == 3 and re.fullmatch(r"validation iter 2 dice/weighted_avg=\S+ iou/weighted_avg=\S+ pixel_accuracy=\S+ ce=\S+", out[0])
    with pytest.raises(KeyError, match="accuracy"):
        ValidationLog(tmp_path, "accuracy").record(1, scores)


def test_get_evaluator(tmp_path):
    from training.validation import SegmentationValidator
    from training_builder.base_train_builder import BaseTrainBuilder, Snapshotter
    from training_builder.trans_u_net_train_builder import TransUNetTrainBuilder
    colors = tmp_path / "colors.json"
    colors.write_text(json.dumps({"stamp": [0, 255, 0], "background": [0, 0, 0], "printed_text": [255, 0, 0]}))
    config = {"num_classes": 3, "class_to_color_map": str(colors), "amp": "bf16"}
    assert BaseTrainBuilder(config, [], None, build=False).get_evaluator() is None
    assert BaseTrainBuilder(config, [], None, build=False).get_evaluator(logger=None) is None
    evaluator = TransUNetTrainBuilder(config, [], [], build=False).get_evaluator()
    assert isinstance(evaluator, SegmentationValidator) and evaluator.class_names == ["stamp", "background", "printed_text"]
    assert evaluator.amp_dtype is torch.bfloat16
    assert BaseTrainBuilder({"num_classes": 2}, [], [], build=False).get_evaluator().class_names == ["class_0", "class_1"]
    net = torch.nn.Linear(2, 2)
    snap = Snapshotter({"segmentation_network": net}, tmp_path / "snaps", 0)
    snap.maybe_save(10)
    assert not (tmp_path / "snaps").exists()
    snap.save_as("best.pt")
    assert set(torch.load(tmp_path / "snaps" / "best.pt")["segmentation_network"]) == {"weight", "bias"}


@pytest.mark.parametrize("scale", R.EXACT_SCALES, ids=lambda s: f"{s[0][0]}x{s[0][1]}-{s[1][0]}x{s[1][1]}")
def test_restatement_equals_torch_float64_on_exact_scales(scale):
    (h, w), (oh, ow) = scale
    rng = np.random.default_rng(h + oh)
    logits = R.tie_logits(rng, (3, 5, h, w))
    labels = R.labels_with_ignored(rng, (3, oh, ow), 5)
    ref = R.reference(logits, labels, (oh, ow))
    up = torch.nn.functional.interpolate(torch.from_numpy(logits).double(), size=(oh, ow), mode="bilinear", align_corners=True)
    assert torch.equal(up, torch.from_numpy(ref.values))            # exact: power-of-two lambdas on small integers
    pred, lab = torch.argmax(up, dim=1).numpy(), labels
    valid = (lab >= 0) & (lab < 5)
    assert np.array_equal(ref.counts[:25], np.bincount(lab[valid] * 5 + pred[valid], minlength=25))
    assert ref.counts[25] == valid.sum() and ref.counts[26] == (~valid).sum() > 0
    ce = torch.nn.functional.cross_entropy(up, torch.from_numpy(np.where(valid, lab, -100)), ignore_index=-100, reduction="sum")
    assert ref.sums[0] == pytest.approx(ce.item(), rel=1e-12)
    p = torch.softmax(up, dim=1).numpy()
    for c in range(5):
        assert ref.sums[1 + 3 * c] == pytest.approx(p[:, c][lab == c].sum(), rel=1e-12)
        assert ref.sums[2 + 3 * c] == pytest.approx((p[:, c] ** 2).sum(), rel=1e-12) and ref.sums[3 + 3 * c] == (lab == c).sum()


def test_general_scale_cases_have_no_undecided_pixel():
    """The cap the GPU test asserts (1 in 1000), on the inputs it draws: the restatement alone gives 0."""
    for (h, w), (oh, ow) in R.GENERAL_SCALES:
        rng = np.random.default_rng(0)
        batch = 1 if oh * ow > 4096 else 2
        logits = rng.standard_normal((batch, 4, h, w)).astype(np.float32)
        labels = R.labels_with_ignored(rng, (batch, oh, ow), 4)
        assert R.reference(logits, labels, (oh, ow)).undecided.sum() == 0


def test_check_counts_excuses_only_undecided_pixels():
    rng = np.random.default_rng(4)
    logits = np.zeros((1, 3, 2, 2), dtype=np.float32)
    logits[0, 0], logits[0, 1] = [[1, 0], [0, 1]], [[0, 1], [1, 0]]      # the centre of 2x2 -> 3x3 is an exact tie of classes 0 and 1
    labels = rng.integers(0, 3, size=(1, 3, 3))
    ref = R.reference(logits, labels, (3, 3))
    assert ref.undecided[0, 1, 1] and ref.undecided.sum() == 5     # the centre and the four edge midpoints
    moved = ref.counts.copy()
    l = labels[0, 1, 1]
    moved[l * 3 + 0] -= 1
    moved[l * 3 + 1] += 1
    assert R.check_counts(moved, ref, labels) == 5
    with pytest.raises(AssertionError):
        R.check_counts(moved, ref, labels, exact=True)
    wrong = ref.counts.copy()
    wrong[l * 3 + 0] -= 1
    wrong[l * 3 + 2] += 1                                           # class 2 is nobody's second choice
    with pytest.raises(AssertionError):
        R.check_counts(wrong, ref, labels)


def test_c_abi_has_the_new_entries():
    import sis_hip
    header = open(os.path.join(ROOT, "include", "sis_hip.h")).read()
    declared = set(re.findall(r"\b(sis_[a-z0-9_]+)\s*\(", header))
    assert NEW_SYMBOLS <= declared and NEW_SYMBOLS <= set(sis_hip.exported_symbols())
    assert declared >= set(sis_hip.exported_symbols())
    lib = ctypes.CDLL(sis_hip.LIB_PATH)
    for name in NEW_SYMBOLS:
        decl = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, header).group(1)
        assert decl.count(",") + 1 == len(sis_hip._SIGNATURES[name][0]), name
        assert hasattr(lib, name), name
    assert sis_hip._SIGNATURES["sis_seg_eval_workspace_bytes"][1] is sis_hip._i64
    assert NEW_KERNELS <= sis_hip.own_kernel_names()
    L = sis_hip.lib()
    assert L.sis_seg_eval_workspace_bytes(16, 4, 256, 256) == 512 * 13 * 8     # 1 048 576 pixels: the launch's 512 workgroups
    assert L.sis_seg_eval_workspace_bytes(3, 5, 5, 7) == 1 * 16 * 8 and L.sis_seg_eval_workspace_bytes(1, 17, 8, 8) == 0
    assert L.sis_seg_eval_workspace_bytes(512, 4, 32768, 32768) == 512 * 13 * 8     # 2^39 pixels: 2^30 per workgroup, an int's worth
    assert L.sis_seg_eval_workspace_bytes(513, 4, 32768, 32768) == 0 and L.sis_seg_eval_workspace_bytes(1, 4, 32768, 32769) == 0
    assert L.sis_seg_eval(None, None, None, None, 0, None, 1, 4, 8, 8, 8, 8, None) != 0    # declines before any device call
    assert "null pointer" in L.sis_last_error().decode()
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        sis_hip.seg_eval(torch.zeros(1, 4, 8, 8), torch.zeros(1, 8, 8, dtype=torch.int64))
