"""DatasetGAN labelling on one MI355X (segmentation/dataset_gan_segmenter.py, csrc/pixel_ensemble.hip).

Measured in one process, on Generator(256, channel_multiplier=2)-shaped activations (14 layers, F = 5888) and a seeded
ensemble of N = 3 members with 3 classes (the shipped dataset-creation config):
  * the fused label pass alone at B = 32: ms per batch, executed TFLOP/s (operations counted from shapes below), share of
    the fp32 matrix peak (157.3 TFLOP/s);
  * the dataset loop (synthesis -> label pass on the side stream -> uint8 images) in images/s with the DatasetGAN labeller,
    next to the k-means labeller (one catalogue of 5 centres on layer 13) and bare synthesis;
  * the reference's ATen formulation (``scale_activations`` + each member's nn.Sequential + ``torch.mode``) at B = 8, per
    image, next to the fused pass on the same activations and weights, and the agreement of their labels.
Every timed shape is warmed up first; times come from device events.  Writes profiles/dataset_gan_bench.json and prints it.
``--label-only``: just the warmed-up label pass at B = 32 (for a kernel-trace run of its own).

    python tools/bench_dataset_gan.py [--steps 10] [--warmup 3] [--loop-batches 12]
"""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "synthesis-in-style_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

PEAK_TF = 157.3
GEN256 = [(512, 4)] * 2 + [(512, 8)] * 2 + [(512, 16)] * 2 + [(512, 32)] * 2 + [(512, 64)] * 2 + [(256, 128)] * 2 + \
    [(128, 256)] * 2
COLOURS = {"background": "#000000", "printed_text": "#0000FF", "handwritten_text": "#FF0000"}


def label_flops(layout, size, members, h1=128, h2=32, cp=32):
    """Operations the fused pass executes per image: the first layer at each activation's own resolution, the bilinear
    interpolate-and-add of every lower group (8 per output element: 4 products, 4 sums), the two tail layers (padded to
    the kernel's class tile)."""
    m = members * h1
    first = sum(2.0 * m * c * r * r for c, r in layout)
    groups = len({r for _, r in layout if r < size})
    interp = 8.0 * size * size * m * groups
    tail = 2.0 * size * size * members * (h1 * h2 + h2 * cp)
    return first + interp + tail


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


def _segmenter(tmp, members, classes=3, seed=100):
    import make_golden_dataset_gan as G
    from segmentation.dataset_gan_segmenter import DatasetGANSegmenter
    dim = sum(c for c, _ in GEN256)
    path = os.path.join(tmp, f"ens{members}.pth")
    torch.save({f"network_{i}": G.seeded_member(classes, dim, seed=seed + i) for i in range(members)}, path)
    return DatasetGANSegmenter(base_dir=tmp, image_size=256, class_to_color_map=COLOURS, classifier_path=path,
                               feature_size=dim, upsamplers=[torch.nn.Upsample(scale_factor=256 / r, mode='bilinear')
                                                             for _, r in GEN256])


def _acts(batch, dev, seed=11):
    g = torch.Generator(device=dev).manual_seed(seed)
    return {k: torch.randn(batch, c, r, r, device=dev, generator=g) for k, (c, r) in enumerate(GEN256)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--loop-batches", type=int, default=12)
    ap.add_argument("--label-only", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_dataset_gan needs a HIP device: there is no CPU measurement")
    dev = torch.device("cuda:0")
    tmp = tempfile.mkdtemp()
    seg = _segmenter(tmp, 3)
    out = {"workload": "DatasetGAN labels of Generator(256) activations, N = 3 members, 3 classes, fp32",
           "device": torch.cuda.get_device_name(0)}

    # ---- label pass alone, B = 32
    acts32 = _acts(32, dev)
    ms32 = _events_ms(lambda: seg.predict_labels_from_activations(acts32), args.steps, args.warmup)
    flops = 32 * label_flops(GEN256, 256, 3)
    out["label_pass_b32"] = {"ms_per_batch": round(ms32, 3), "images_per_s": round(32e3 / ms32, 1),
                             "gflop_per_image": round(flops / 32 / 1e9, 2),
                             "executed_tflops": round(flops / ms32 / 1e9, 2),
                             "fraction_of_fp32_mfma_peak": round(flops / ms32 / 1e9 / PEAK_TF, 3)}
    if args.label_only:
        print(json.dumps(out))
        return
    del acts32

    # ---- reference ATen formulation against the fused pass, B = 8, same activations and weights
    from data.dataset_gan_dataset import scale_activations
    acts8 = _acts(8, dev, seed=12)
    own8 = _events_ms(lambda: seg.predict_labels_from_activations(acts8), args.steps, args.warmup)

    def reference():
        with torch.no_grad():
            return seg.predict_labels(scale_activations([acts8], seg.upsamplers)[0])

    ref_ms = _events_ms(reference, 2, 1)
    agree = (reference().long() == seg.predict_labels_from_activations(acts8)).double().mean().item()
    out["reference_vs_own_b8"] = {"reference_ms_per_image": round(ref_ms / 8, 3), "own_ms_per_image": round(own8 / 8, 3),
                                  "speedup": round(ref_ms / own8, 2), "label_agreement": round(agree, 6)}
    del acts8
    torch.cuda.empty_cache()

    # ---- dataset loop: synthesis + label pass on the side stream, three labellers in the same process
    from networks.stylegan2.model import Generator
    from segmentation.gan_local_edit.factor_catalog import FactorCatalog
    from utils.dataset_creation import label_and_encode, seeded_latents
    torch.manual_seed(0)
    g = Generator(256, 512, 8, channel_multiplier=2).to(dev).eval()
    catalog = {13: FactorCatalog(cluster_centers=np.random.RandomState(0).randn(5, 128).astype(np.float32))}
    noise = g.make_noise()

    def loop(catalogs, dg, batches):
        pending = None
        with torch.no_grad():
            for _ in range(batches):
                z = seeded_latents(32, 512, dev)
                image, acts = g([z.to(dev, non_blocking=True)], noise=noise, return_intermediate_activations=True)
                job = label_and_encode(image, acts, catalogs, dg)
                if pending is not None and pending[2] is not None:
                    pending[2].synchronize()
                pending = job
        if pending is not None and pending[2] is not None:
            pending[2].synchronize()

    rates = {}
    for name, cats, dg in (("synthesis_only", {}, None), ("kmeans", catalog, None), ("dataset_gan", {}, seg)):
        loop(cats, dg, 2)
        ms = _events_ms(lambda: loop(cats, dg, args.loop_batches), 1, 0)
        rates[name] = round(32e3 * args.loop_batches / ms, 1)
    out["dataset_loop_images_per_s_b32"] = rates

    path = os.path.join(ROOT, "profiles", "dataset_gan_bench.json")
    with open(path, "w") as f:
        f.write(json.dumps(out) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
