"""DatasetGAN ensemble training on one MI355X (training/ensemble_step.py, csrc/pixel_ensemble_train.h).

One Generator(256, channel_multiplier=2)-shaped activation set (14 layers, F = 5888) of one image is resident; N = 3 members,
3 classes.  Timed per step at P = 4, 4096 and 65536 pixels of that image:
  * fused: ``FusedEnsembleStep.step`` -- gather, the two layer-1 GEMMs, the tail, the N optimizers;
  * baseline, the only way the code before this stage could do a step: ``scale_activations`` builds the [1, 256, 256, 5888]
    feature tensor, the P rows are taken from it, then the ATen loop over the members with the same optimizers.
Both run in one process, alternating, five runs each (a run = ``--steps`` timed steps after ``--warmup``); the median run is
reported.  Executed TFLOP/s: the operations of the two layer-1 GEMMs (2 * 2 * P * F * N * 128) over the WHOLE fused step's time,
against the 157.3 TFLOP/s fp32 matrix peak.  Launches per step are the fused path's own count by construction (gather 1,
layer-1 forward 1, tail 9, weight gradient 3 and 1 more when P > 2048 splits it into slabs, 2 per optimizer).
Writes profiles/ensemble_train_bench.json and prints it.

    python tools/bench_ensemble_train.py [--steps 5] [--warmup 2]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "synthesis-in-style_amd"))

import torch  # noqa: E402
from torch import nn  # noqa: E402

PEAK_TF = 157.3
GEN256 = [(512, 4)] * 2 + [(512, 8)] * 2 + [(512, 16)] * 2 + [(512, 32)] * 2 + [(512, 64)] * 2 + [(256, 128)] * 2 + \
    [(128, 256)] * 2
SIZE, MEMBERS, CLASSES = 256, 3, 3
ADAM = dict(lr=5e-4, betas=(0.5, 0.999), weight_decay=1e-4)


class _Resident:
    def __init__(self, layers):
        self.layers, self.image_size = layers, SIZE


def _events_ms(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def _ensemble(dev, features):
    from networks.pixel_classifier.model import PixelEnsembleClassifier
    from training.fused_adam import GradientClipAdam
    torch.manual_seed(0)
    e = PixelEnsembleClassifier(CLASSES, features, MEMBERS)
    for m in e.get_networks().values():
        m.to(dev)
    opts = {f"optimizer_{i}": GradientClipAdam(m.parameters(), **ADAM) for i, m in enumerate(e.get_networks().values())}
    return e, opts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--pixels", type=int, nargs="*", default=[4, 4096, 65536])
    args = ap.parse_args()
    from data.dataset_gan_dataset import scale_activations
    from training.ensemble_step import FusedEnsembleStep
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(11)
    layers = [torch.randn(1, c, r, r, device=dev, generator=gen) for c, r in GEN256]
    features = sum(c for c, _ in GEN256)
    dataset = _Resident(layers)
    upsamplers = [nn.Upsample(scale_factor=SIZE / r, mode="bilinear") for _, r in GEN256]
    fused_e, fused_opts = _ensemble(dev, features)
    fused = FusedEnsembleStep(fused_e, fused_opts)
    base_e, base_opts = _ensemble(dev, features)
    ce = nn.CrossEntropyLoss()
    out = {"workload": f"DatasetGAN ensemble training step, Generator(256) activations (F = {features}), N = {MEMBERS} members, "
                       f"{CLASSES} classes, fp32", "device": torch.cuda.get_device_name(0), "runs": 5, "steps_per_run": args.steps,
           "fp32_mfma_peak_tflops": PEAK_TF, "pixels": {}}
    for npix in args.pixels:
        g = torch.Generator().manual_seed(npix)
        flat = torch.randperm(SIZE * SIZE, generator=g)[:npix]
        pixels = torch.stack([torch.zeros_like(flat), flat // SIZE, flat % SIZE], 1).int().to(dev)
        labels = torch.randint(0, CLASSES, (npix,), generator=g).to(dev)

        def fused_step():
            fused.step(pixels, labels, dataset)

        def baseline_step():
            feats = scale_activations([{i: t for i, t in enumerate(layers)}], upsamplers)[0]
            x = feats[pixels[:, 0].long(), pixels[:, 1].long(), pixels[:, 2].long()]
            del feats
            for i, m in enumerate(base_e.get_networks().values()):
                opt = base_opts[f"optimizer_{i}"]
                opt.zero_grad()
                ce(m(x), labels).backward()
                opt.step()

        fused_ms, base_ms = [], []
        for _ in range(5):   # alternating: both legs see the same clocks and the same neighbours
            fused_ms.append(_events_ms(fused_step, args.steps, args.warmup))
            base_ms.append(_events_ms(baseline_step, args.steps, args.warmup))
        f, b = statistics.median(fused_ms), statistics.median(base_ms)
        gemm_flops = 2 * 2.0 * npix * features * MEMBERS * 128
        out["pixels"][str(npix)] = {
            "fused_ms_per_step": round(f, 4), "fused_runs_ms": [round(v, 4) for v in fused_ms],
            "baseline_ms_per_step": round(b, 4), "baseline_runs_ms": [round(v, 4) for v in base_ms],
            "speedup": round(b / f, 2), "layer1_gemm_tflops_over_step": round(gemm_flops / f / 1e9, 3),
            "fraction_of_fp32_mfma_peak": round(gemm_flops / f / 1e9 / PEAK_TF, 4),
            "fused_launches_per_step": 14 + (1 if npix > 2048 else 0) + 2 * MEMBERS,
        }
        print(npix, out["pixels"][str(npix)], flush=True)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "ensemble_train_bench.json"), "w") as fh:
        json.dump(out, fh)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
