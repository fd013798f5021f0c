"""GPU: validation during training (training/validation.py) on a tiny PNG dataset: ``SegmentationValidator.run()``
for the three segmenters against ``torch.argmax`` of their own evaluation forward, training left exactly where it was (hipGraph
step included), and ``train.main`` end to end with and without ``--val-images``."""
import json
import os
import re

import numpy as np
import pytest
import torch
import yaml

import seg_eval_restatement as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "synthesis-in-style_amd")
COLORS = {"background": [0, 0, 0], "printed_text": [255, 0, 0], "handwritten_text": [0, 0, 255], "stamp": [0, 255, 0]}
NAMES = list(COLORS)
METRICS = ("dice", "iou", "precision", "recall")
DOCUMENTED_KEYS = {f"{m}/{n}" for m in METRICS for n in NAMES + ["weighted_avg", "weighted_text_avg"]} | \
    {"pixel_accuracy", "ce", "dice_loss", "counted", "ignored"}


@pytest.fixture(scope="module")
def png_dataset(tmp_path_factory):
    """Six 40 x 40 [image | label] pairs in four classes: train.json lists all, val.json the last five (one short of a
    multiple of the batch size, so the last validation batch is a smaller one)."""
    from PIL import Image
    root = tmp_path_factory.mktemp("validation_pairs")
    rng = np.random.default_rng(8)
    table = np.array(list(COLORS.values()), dtype=np.uint8)
    ys, xs = np.arange(40)[:, None] * 3 // 40, np.arange(40)[None, :] * 4 // 40
    for i in range(6):
        image = rng.integers(0, 256, (40, 40, 3), dtype=np.uint8)
        label = ((ys * 4 + xs + rng.integers(0, 4)) % 4).astype(np.uint8)
        Image.fromarray(np.concatenate([image, table[label]], axis=1)).save(str(root / f"{i:04d}.png"))
    (root / "train.json").write_text(json.dumps([{"file_name": f"{i:04d}.png"} for i in range(6)]))
    (root / "val.json").write_text(json.dumps([{"file_name": f"{i:04d}.png"} for i in range(1, 6)]))
    (root / "colors.json").write_text(json.dumps(COLORS))
    return root


def _val_loader(root, device, image_size, batch_size=4):
    from data.device_dataset import DeviceSegmentationLoader
    from data.segmentation_dataset import AugmentedSegmentationDataset
    dataset = AugmentedSegmentationDataset(root / "val.json", root=str(root), class_to_color_map_path=root / "colors.json",
                                           image_size=image_size, num_augmentations=2, device=device)
    return DeviceSegmentationLoader(dataset, batch_size, shuffle=False, drop_last=False, seed=3)


def _state_bits(network, optimizer=None):
    state = {k: v.detach().clone() for k, v in network.state_dict().items()}
    if optimizer is not None:
        for i, p in enumerate(p for g in optimizer.param_groups for p in g["params"]):
            for key, value in optimizer.state.get(p, {}).items():
                if torch.is_tensor(value):
                    state[f"optimizer.{i}.{key}"] = value.detach().clone()
    return state


def _assert_same_bits(a, b):
    assert a.keys() == b.keys()
    bits = lambda t: t.reshape(-1).contiguous().view(torch.uint8)   # noqa: E731  (bit patterns: a NaN equals itself)
    differing = [k for k in a if a[k].shape != b[k].shape or not torch.equal(bits(a[k]), bits(b[k]))]
    assert not differing, f"{len(differing)} of {len(a)} tensors differ, first {differing[:5]}"


def _network(which, device):
    """-> (network on the device, image size, amp)"""
    torch.manual_seed(0)
    if which == "DocUFCN":
        from networks.doc_ufcn import get_doc_ufcn
        return get_doc_ufcn("base")(4, 3, min_confidence=0.0, min_contour_area=0).to(device), 48, None
    if which == "EMANet":
        from networks.ema_net.network import EMANet
        return EMANet(4, 50, use_pretrained_resnet=False).to(device), 64, None
    from training_builder.trans_u_net_train_builder import TransUNetTrainBuilder
    cfg = yaml.safe_load(open(os.path.join(SRC, "configs", "segmenter", "trans_u_net_r50_vit_b16_512.yaml")))
    cfg.update(num_classes=4, image_size=64, batch_size=4)   # 64 = 4 x 4 tokens of 16: the smallest grid the builder's tests train
    return TransUNetTrainBuilder(cfg, [], [], rank=0, world_size=1).get_network(), 64, cfg["amp"]


@pytest.mark.parametrize("which", ["DocUFCN", "EMANet", "TransUNet"])
def test_validator_equals_argmax_of_the_evaluation_forward(device, png_dataset, which):
    from segmentation.evaluation.segmentation_metric_calculation import calculate_metric
    from training.loop import get_current_reporter
    from training.validation import SegmentationValidator
    network, size, amp = _network(which, device)
    network.train()
    loader = _val_loader(png_dataset, device, size)
    validator = SegmentationValidator(network, loader, NAMES, device, amp=amp)
    before = _state_bits(network)
    get_current_reporter().observations.clear()
    scores = validator.run()
    assert network.training and all(m.training for m in network.modules())
    _assert_same_bits(before, _state_bits(network))                   # every parameter and buffer, emau.mu included
    assert set(scores) == DOCUMENTED_KEYS
    assert set(get_current_reporter().scalars()) == {f"validation/{k}" for k in DOCUMENTED_KEYS}
    counts = validator.last_counts.numpy()
    assert scores["counted"] == 10 * size * size and scores["ignored"] == 0     # 5 files x 2 indices

    loader.set_epoch(0)
    network.eval()
    aten = np.zeros(18, dtype=np.int64)
    ref_counts, undecided = np.zeros(18, dtype=np.int64), 0
    with torch.no_grad():
        batches = list(loader)
        assert [b["images"].shape[0] for b in batches] == [4, 4, 2]
        for batch in batches:
            labels = batch["segmented"][:, 0]
            with torch.autocast(device_type="cuda", dtype=torch.bfloat16, enabled=amp is not None):
                full = network(batch["images"])                           # EMANet: interpolated to the image size by ATen
            pred = torch.argmax(full, dim=1)
            aten[:16] += torch.bincount((labels * 4 + pred).flatten(), minlength=16).cpu().numpy()
            if which == "EMANet":
                low = network.logits(batch["images"])[0]
                assert tuple(low.shape[-2:]) == (size // 8, size // 8)
                ref = R.reference(low.cpu().numpy(), labels.cpu().numpy(), (size, size))
                # ATen's interpolation rounds like the kernel's, not in the same places: it gets the same allowance
                R.check_counts(np.concatenate([torch.bincount((labels * 4 + pred).flatten(), minlength=16).cpu().numpy(),
                                               ref.counts[16:]]), ref, labels.cpu().numpy())
                ref_counts += ref.counts
                undecided += int(ref.undecided.sum())
    network.train()
    if which == "EMANet":
        assert undecided * 1000 <= 10 * size * size
        moved = np.abs(counts[:16] - ref_counts[:16]).sum()
        assert moved <= 2 * undecided and counts[:16].sum() == ref_counts[:16].sum()
        if undecided == 0:
            assert np.array_equal(counts[:16], aten[:16])
    else:
        assert full.dtype == (torch.bfloat16 if amp else torch.float32)
        assert np.array_equal(counts[:16], aten[:16])
    matrix = torch.from_numpy(counts[:16].reshape(4, 4))
    for metric in METRICS:
        for key, entry in calculate_metric(matrix, NAMES, metric).items():
            assert scores[f"{metric}/{key}"] == entry["score"]
    assert scores["pixel_accuracy"] == counts[:16].reshape(4, 4).trace() / counts[16]
    assert np.isfinite(scores["ce"]) and scores["ce"] > 0 and 0 < scores["dice_loss"] < 1


def _train(device, png_dataset, which, validate_after, iterations=5, size=None):
    """``iterations`` updater iterations from a fixed seed, the step hipGraph on (two eager iterations, the third is captured,
    the rest are replays), a validation pass after the iterations in ``validate_after`` -> (state bits, updater)."""
    import sis_hip
    from networks.doc_ufcn import get_doc_ufcn
    from networks.ema_net.network import EMANet
    from networks.ema_net.utils import get_params
    from training.fused_adam import GradientClipAdam
    from training.fused_sgd import FusedSGD
    from training.validation import SegmentationValidator
    from updater.segmentation_updater import EMANetUpdater, StandardUpdater
    torch.manual_seed(0)
    sis_hip._drop_seeds.clear()      # the dropout seed word is drawn from torch's seed when first asked for
    gen = torch.Generator().manual_seed(1)
    size = size or (EMANET_TRAIN_SIZE if which == "EMANet" else 48)
    batches = [{"images": torch.rand(2, 3, size, size, generator=gen) * 2 - 1,
                "segmented": torch.randint(0, 4, (2, 1, size, size), generator=gen)} for _ in range(iterations)]
    if which == "EMANet":
        net = EMANet(4, 50, use_pretrained_resnet=False).to(device).train()
        lr = 2e-5
        opt = FusedSGD([{"params": list(get_params(net, "1x")), "lr": lr, "weight_decay": 1e-4},
                        {"params": list(get_params(net, "1y")), "lr": lr, "weight_decay": 0},
                        {"params": list(get_params(net, "2x")), "lr": 2 * lr, "weight_decay": 0.0}], momentum=0.9)
        updater = EMANetUpdater(em_mom=0.9, iterators={"images": batches}, networks={"segmentation": net},
                                optimizers={"main": opt}, device=device)
    else:
        net = get_doc_ufcn("base")(4, 3, min_confidence=0.0, min_contour_area=0).to(device).train()
        assert any(isinstance(m, torch.nn.Dropout) and m.p > 0 for m in net.modules())
        opt = GradientClipAdam(net.parameters(), lr=1e-3, betas=(0.5, 0.999), weight_decay=1e-4)
        updater = StandardUpdater(iterators={"images": batches}, networks={"segmentation": net}, optimizers={"main": opt},
                                  device=device, class_weights=[1.0, 2.0, 2.0, 2.0])
    assert updater._step_graph.enabled
    validator = SegmentationValidator(net, _val_loader(png_dataset, device, size), NAMES, device)
    # the vendor library's convolutions (EMANet's 3-channel stem) are asked for their repeatable solvers, in every run alike
    with torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True):
        for it in range(1, iterations + 1):
            updater.update()
            if it in validate_after:
                validator.run()
        torch.cuda.synchronize()
    assert updater._step_graph.graph is not None and updater._step_graph.capture_error is None
    return _state_bits(net, opt)


EMANET_TRAIN_SIZE = 256


@pytest.mark.parametrize("which", ["EMANet", "DocUFCN"])
def test_training_is_undisturbed(device, png_dataset, which):
    """Five iterations with a validation pass after the second (before the capture of the third) and after the fourth (between
    two replays) against the same five with none: weights, BatchNorm statistics, EM bases and optimizer state bit for bit.

    EMANet runs at 256 x 256, the shipped config's size, with the vendor library asked for its repeatable solvers, because that
    is where two runs of its training step are comparable at all.  Measured on the MI355X, in one process, seed, initial weights
    and batches the same, bit patterns compared: at 64 x 64 and 128 x 128 one training-mode forward repeated on the same
    weights first differs at ``extractor.7.1.conv2`` / ``extractor.7.2.conv2`` (layer4's 3x3 layers whose dilation, 8 / 16, is
    the whole side of the 8 x 8 / 16 x 16 feature map), and two five-iteration runs WITHOUT validation differ in 450 to 459 of
    the 529 tensors; at 256 x 256 the forward repeats and one gradient does not, that of the 3-channel stem convolution, which
    runs on the vendor library (432 of 529 tensors after five iterations); with ``cudnn.deterministic`` two runs without
    validation are bit-equal, and so this test can see what a validation pass changes.  DocUFCN (48 x 48, dropout on) has no
    library layer and needs neither."""
    plain = _train(device, png_dataset, which, validate_after=())
    validated = _train(device, png_dataset, which, validate_after=(2, 4))
    assert any("running_mean" in k for k in plain) and any(k.startswith("optimizer.") for k in plain)
    assert which != "EMANet" or "emau.mu" in plain
    _assert_same_bits(plain, validated)


def _main(png_dataset, tmp_path, capsys, validation):
    import train
    from training.loop import get_current_reporter
    cfg = yaml.safe_load(open(os.path.join(SRC, "configs", "segmenter", "ema_net_resnet50_256.yaml")))
    cfg.update(batch_size=2, image_size=64, iterations_per_epoch=2, epochs=3, snapshot_save_iter=4, log_iter=1, num_classes=4,
               num_augmentations=2)
    path = tmp_path / "config.yaml"
    path.write_text(yaml.safe_dump(cfg))
    argv = [str(path), "--images", str(png_dataset / "train.json"), "--class-to-color-map", str(png_dataset / "colors.json"),
            "--max-iter", "4", "-l", str(tmp_path / "logs")]
    if validation:
        argv += ["--val-images", str(png_dataset / "val.json"), "--eval-iter", "2"]
    get_current_reporter().observations.clear()
    capsys.readouterr()
    train.main(0, train.parse_args(argv), 1)
    return capsys.readouterr().out.splitlines(), sorted(os.listdir(tmp_path / "logs"))


ITER_LINE = r"iter \d+ loss/softmax=\S+ images/s=\S+"


def test_train_main_with_validation(device, png_dataset, tmp_path, capsys):
    from networks.ema_net.network import EMANet
    out, files = _main(png_dataset, tmp_path, capsys, validation=True)
    assert files == ["000004.pt", "best.pt", "validation.jsonl"]
    records = [json.loads(line) for line in (tmp_path / "logs" / "validation.jsonl").read_text().splitlines()]
    # --eval-iter 2, 4 iterations: after iterations 2 and 4; the pass after the last iteration IS the one of iteration 4
    assert [(r["iteration"], r["final"]) for r in records] == [(2, False), (4, True)]
    assert all(set(r) == DOCUMENTED_KEYS | {"iteration", "final"} for r in records)
    assert all(r["counted"] == 10 * 64 * 64 and r["ignored"] == 0 and np.isfinite(r["ce"]) for r in records)
    shown = [line for line in out if line.startswith("validation")]
    assert len(shown) == 2 and all(re.fullmatch(r"validation iter [24] dice/weighted_avg=\S+ iou/weighted_avg=\S+ "
                                                r"pixel_accuracy=\S+ ce=\S+", line) for line in shown)
    assert f"dice/weighted_avg={records[0]['dice/weighted_avg']:.5f}" in shown[0]
    assert [line for line in out if not line.startswith("validation")] == [line for line in out if re.fullmatch(ITER_LINE, line)]
    assert len(out) == 6 and out.index(shown[0]) == 2 and out.index(shown[1]) == 5      # right after iterations 2 and 4
    best = torch.load(tmp_path / "logs" / "best.pt", map_location="cpu")
    assert set(best) == {"segmentation_network", "main"}
    EMANet(4, 50, use_pretrained_resnet=False).load_state_dict(best["segmentation_network"], strict=True)


def test_train_main_without_validation_is_unchanged(device, png_dataset, tmp_path, capsys):
    out, files = _main(png_dataset, tmp_path, capsys, validation=False)
    assert files == ["000004.pt"]                                   # no validation.jsonl, no best.pt
    assert len(out) == 4 and all(re.fullmatch(ITER_LINE, line) for line in out)
