"""The validation pass on one MI355X.

* ``sis_hip.seg_eval`` (two launches) per batch against the same quantities in ATen in this process: ``F.interpolate`` where the
  logits are smaller than the labels, ``argmax``, ``bincount`` over ``label * C + prediction`` (which synchronises with the host to
  size its result), ``cross_entropy(reduction='sum', ignore_index)``, ``softmax`` and the three Dice sums.  Batch and size are read
  off the shipped configs, the class count is the four of the document colour maps:
    EMANet     B = 16, 4 x 32 x 32 float32 logits -> 256 x 256 labels   (the interpolated route)
    TransUNet  B = 8, 4 x 512 x 512 bfloat16 logits, labels at that size (``amp: bf16``)
  The two variants alternate, ``--runs`` rounds each after warm-up, device events around a window of at least 0.2 s; median and
  range.  Every call takes the next of several input sets that together exceed the 256 MiB Infinity Cache.
* bytes per second next to the HBM roofline, the only bound this pass has: the logits and the int64 labels read once, over the
  measured time of a call, against the achievable 6.3 TB/s (MI355X_MICROARCH: 8 TB/s peak).  The figure is the call's (two
  launches issued from Python), not a kernel's.
* a whole ``SegmentationValidator.run()`` over ``--val-batches`` batches next to the training step of the same EMANet at the
  shipped config (hipGraph step after its warm-up), both in images per second.

Writes profiles/seg_eval_bench.json and prints it.

    python tools/bench_seg_eval.py [--runs 5] [--val-batches 8] [--out profiles/seg_eval_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "synthesis-in-style_amd")
sys.path.insert(0, SRC)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
import yaml  # noqa: E402

CLASSES = 4
HBM_ACHIEVABLE = 6.3e12
WINDOW_SECONDS = 0.2


def aten_eval(logits, labels, classes=CLASSES):
    x = logits.float()
    if x.shape[-2:] != labels.shape[-2:]:
        x = F.interpolate(x, size=labels.shape[-2:], mode="bilinear", align_corners=True)
    pred = x.argmax(dim=1)
    valid = (labels >= 0) & (labels < classes)
    cells = torch.bincount(torch.where(valid, labels * classes + pred, classes * classes).flatten(), minlength=classes * classes + 1)
    ce = F.cross_entropy(x, torch.where(valid, labels, -100), ignore_index=-100, reduction="sum")
    p = torch.softmax(x, dim=1)
    onehot = (labels[:, None] == torch.arange(classes, device=labels.device).view(1, -1, 1, 1)).float()
    return cells, ce, (p * onehot).sum(dim=(0, 2, 3)), (p * p).sum(dim=(0, 2, 3)), onehot.sum(dim=(0, 2, 3))


def timed(fn, sets, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for i in range(iters):
        fn(*sets[i % len(sets)])
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def measure(variants, sets, runs):
    iters = {}
    for name, fn in variants.items():
        timed(fn, sets, 3)
        iters[name] = int(min(20000, max(5, WINDOW_SECONDS * 1e3 / max(timed(fn, sets, 5), 1e-3))))
    samples = {name: [] for name in variants}
    for _ in range(runs):
        for name, fn in variants.items():
            samples[name].append(timed(fn, sets, iters[name]))
    return {name: {"median_ms": round(statistics.median(v), 5), "min_ms": round(min(v), 5), "max_ms": round(max(v), 5), "iters": iters[name]}
            for name, v in samples.items()}


def bench_shape(sis_hip, device, gen, batch, low, size, dtype, runs):
    logits_bytes = batch * CLASSES * low * low * (2 if dtype == torch.bfloat16 else 4)
    set_bytes = logits_bytes + batch * size * size * 8
    n_sets = -(-(288 << 20) // set_bytes)
    sets = []
    for _ in range(n_sets):
        labels = torch.randint(0, CLASSES, (batch, size, size), generator=gen, device=device)
        labels[torch.rand((batch, size, size), generator=gen, device=device) < 0.02] = 255
        sets.append((torch.randn((batch, CLASSES, low, low), generator=gen, device=device).to(dtype), labels))
    counts, sums = sis_hip.seg_eval_state(CLASSES, device)
    times = measure({"kernel": lambda x, lab: sis_hip.seg_eval(x, lab, counts=counts, sums=sums), "aten": aten_eval}, sets, runs)
    k_counts, k_sums = sis_hip.seg_eval(*sets[0])
    cells, ce, inter, psum, tsum = aten_eval(*sets[0])
    moved = int((k_counts[:CLASSES * CLASSES] - cells[:CLASSES * CLASSES]).abs().sum())
    roofline_ms = set_bytes / HBM_ACHIEVABLE * 1e3
    times["kernel"]["bytes_per_s"] = round(set_bytes / (times["kernel"]["median_ms"] * 1e-3), 1)
    times["kernel"]["share_of_hbm_roofline"] = round(roofline_ms / times["kernel"]["median_ms"], 4)
    return {"batch": batch, "classes": CLASSES, "logits": [low, low], "labels": [size, size], "dtype": str(dtype).replace("torch.", ""),
            "input_sets": n_sets, "bytes_read_per_call": set_bytes, "roofline_ms_reading_once": round(roofline_ms, 5), **times,
            "kernel_over_aten": round(times["kernel"]["median_ms"] / times["aten"]["median_ms"], 4),
            "kernel_against_aten_float32": {"pixels_in_another_cell": moved, "pixels": batch * size * size,
                                            "ce_relative": abs(float(k_sums[0]) - float(ce)) / float(ce),
                                            "dice_sums_max_relative": float(((k_sums[1:].view(-1, 3).t().float() - torch.stack([inter, psum, tsum]))
                                                                             .abs() / torch.stack([inter, psum, tsum]).clamp_min(1e-30)).max())}}


def bench_pass(device, cfg, runs, val_batches):
    """images/s of the EMANet training step (hipGraph, after warm-up) and of a whole validation pass over ``val_batches`` batches."""
    from training.validation import SegmentationValidator
    from training_builder.ema_net_train_builder import EMANetTrainBuilder
    from utils.synthetic_data import SyntheticSegmentationLoader
    batch, size = cfg["batch_size"], cfg["image_size"]
    train_loader = SyntheticSegmentationLoader(batch, size, cfg["num_classes"], seed=1234, device=device, num_batches=None)
    val = list(SyntheticSegmentationLoader(batch, size, cfg["num_classes"], seed=99, device=device, num_batches=val_batches))
    builder = EMANetTrainBuilder(dict(cfg), train_loader, val, rank=0, world_size=1)
    updater = builder.get_updater()
    validator = SegmentationValidator(builder.get_network(), val, [f"class_{i}" for i in range(cfg["num_classes"])], device)

    def steps(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            updater.update()
        torch.cuda.synchronize()
        return n * batch / (time.perf_counter() - t0)

    def passes(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            validator.run()      # ends in the one copy to the host
        return n * batch * len(val) / (time.perf_counter() - t0)

    steps(6)      # two eager iterations, the capture, three replays
    passes(1)
    train, valid = [], []
    for _ in range(runs):
        train.append(steps(20))
        valid.append(passes(2))
    summary = lambda v: {"median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1)}   # noqa: E731
    return {"network": "EMANet-50", "batch": batch, "size": size, "classes": cfg["num_classes"], "validation_batches": len(val),
            "step_graph": updater._step_graph.graph is not None, "training_images_per_s": summary(train),
            "validation_images_per_s": summary(valid),
            "validation_pass_in_training_steps": round(statistics.median(train) / statistics.median(valid) * len(val), 2)}


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--runs", type=int, default=5)
    parser.add_argument("--val-batches", type=int, default=8)
    parser.add_argument("--skip-pass", action="store_true", help="only the per-batch comparison")
    parser.add_argument("--out", default=os.path.join(ROOT, "profiles", "seg_eval_bench.json"))
    args = parser.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_seg_eval: a HIP device is required (no CPU timing is meaningful)")
    import sis_hip
    device = torch.device("cuda:0")
    gen = torch.Generator(device=device).manual_seed(0)
    ema = yaml.safe_load(open(os.path.join(SRC, "configs", "segmenter", "ema_net_resnet50_256.yaml")))
    tun = yaml.safe_load(open(os.path.join(SRC, "configs", "segmenter", "trans_u_net_r50_vit_b16_512.yaml")))
    result = {"device": torch.cuda.get_device_name(0), "hbm_achievable_bytes_per_s": HBM_ACHIEVABLE, "runs": args.runs, "per_batch": {
        "ema_net": bench_shape(sis_hip, device, gen, ema["batch_size"], ema["image_size"] // 8, ema["image_size"], torch.float32, args.runs),
        "trans_u_net": bench_shape(sis_hip, device, gen, tun["batch_size"], tun["image_size"], tun["image_size"],
                                   torch.bfloat16 if tun.get("amp") == "bf16" else torch.float32, args.runs)}}
    if not args.skip_pass:
        result["whole_pass"] = bench_pass(device, ema, args.runs, args.val_batches)
    text = json.dumps(result, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
