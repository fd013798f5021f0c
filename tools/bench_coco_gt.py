"""Dataset ground truth on one MI355X at the dataset workload's shape: B = 32 label images of 256 x 256, the
two annotated classes of the cluster-based labeller (setup of tools/bench_cluster_segmenter.py: Generator(256), random
weights, random unit centres).

* (a) ``sis_hip.label_regions`` in listing mode per batch, on the labeller's own label images and on smooth-noise planes
  (tests/page_eval_restatement.py), device events after warm-up, five alternating runs, the median; the labeller's own time
  per batch from profiles/cluster_segmenter_bench.json stands beside it;
* (b) the dataset loop with ``--png-encoder device`` -- synthesis, label pass, PNG encode and the copy to pinned memory, the
  file writes left out -- with and without the listing of ``--ground-truth``, wall clock, five alternating runs, the median;
* (c) full annotations (regions, run lengths, strings, dictionaries) for label images that are resident on the device, in
  images/s, against tests/coco_gt_restatement.py on 16 host workers, with equal annotations.

Writes profiles/coco_gt_bench.json and prints it.

    python tools/bench_coco_gt.py [--steps 20] [--warmup 5] [--out profiles/coco_gt_bench.json]
"""
import argparse
import json
import multiprocessing
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "synthesis-in-style_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

from bench_cluster_segmenter import BATCH, COLOURS, SIZE, event_ms, setup  # noqa: E402

ROUNDS = 5


def _host_annotations(labels):
    import coco_gt_restatement as R
    from segmentation.evaluation.coco_gt import COCOGtCreator
    creator = COCOGtCreator(COLOURS, region_provider=R.provider)
    return [creator.annotations_of_label_images(label[None], 0, 0)[0] for label in labels]


def smooth_noise_labels(colours):
    import coco_gt_restatement as R
    import page_eval_restatement as E
    noise = E.smooth_noise_planes(np.random.RandomState(11), (BATCH, len(colours), SIZE, SIZE), 0.2)
    masks = np.stack([(noise[:, k] > 0.7) & (noise.argmax(axis=1) == k) for k in range(len(colours))], axis=1)
    return R.planes_to_label(masks, colours)


def loop_ms(g, segmenter, colours, with_listing, steps, warmup):
    import torch
    from utils.dataset_creation import encode_pairs_on_device, label_and_encode, list_classes_on_device, seeded_latents
    device = torch.device("cuda:0")

    def issue():
        with torch.no_grad():
            z = seeded_latents(BATCH, g.style_dim, device).to(device, non_blocking=True)
            image, acts = g([z], noise=g.make_noise(), return_intermediate_activations=True)
            pixels, labels, ready = label_and_encode(image, acts, {}, None, segmenter)
            label_image, listed = (lambda: labels["cluster_segmenter"][1]), None
            if with_listing:
                lab, listed, ready = list_classes_on_device(pixels, label_image, colours, ready)
                label_image = lambda: lab  # noqa: E731
            return encode_pairs_on_device(pixels, label_image, ready), listed

    def run(n):
        pending = None
        for _ in range(n):
            job = issue()
            if pending is not None:
                pending[0][2].synchronize()
            pending = job
        pending[0][2].synchronize()

    run(warmup)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run(steps)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coco_gt_bench.json"))
    args = ap.parse_args()
    pool = multiprocessing.get_context("fork").Pool(args.workers)   # forked before this process opens the device
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_coco_gt needs a HIP device: nothing is measured without one")
    import sis_hip
    from segmentation.evaluation.coco_gt import COCOGtCreator
    g, segmenter, _, _, acts = setup(0.75)
    creator = COCOGtCreator(COLOURS)
    colours = creator.colours
    labeller_images = segmenter.label_activations(acts)[1].contiguous()
    noise_images = torch.from_numpy(smooth_noise_labels(colours)).cuda()
    inputs = {"labeller_label_images": labeller_images, "smooth_noise_planes": noise_images}

    # (a) listing mode, alternating between the two inputs
    listing = {name: [] for name in inputs}
    for _ in range(ROUNDS):
        for name, images in inputs.items():
            listing[name].append(event_ms(lambda: sis_hip.label_regions(images, colours, runs=False, max_regions=0), args.steps, args.warmup))
    result = {"device": torch.cuda.get_device_name(0), "shape": {"batch": BATCH, "p": SIZE, "annotated_classes": len(colours)}}
    result["listing_ms_per_batch"] = {}
    for name, images in inputs.items():
        found = sis_hip.label_regions(images, colours, runs=False)
        result["listing_ms_per_batch"][name] = {
            "median": round(statistics.median(listing[name]), 4), "runs": [round(v, 4) for v in listing[name]],
            "regions_per_plane": round(float(found.region_count.float().mean()), 1),
            "counts_per_plane": round(float(found.run_total.float().mean()), 1),
            "planes_with_a_class": int(found.has.sum())}
    try:
        with open(os.path.join(ROOT, "profiles", "cluster_segmenter_bench.json")) as f:
            result["labeller_on_finished_maps_ms"] = json.load(f)["label_pass_ms"]["labeller_on_finished_maps"]
    except OSError:
        result["labeller_on_finished_maps_ms"] = None

    # (b) the loop, alternating between without and with the listing
    loops = {"without": [], "with_ground_truth": []}
    for _ in range(ROUNDS):
        loops["without"].append(loop_ms(g, segmenter, colours, False, args.steps, args.warmup))
        loops["with_ground_truth"].append(loop_ms(g, segmenter, colours, True, args.steps, args.warmup))
    medians = {k: statistics.median(v) for k, v in loops.items()}
    result["dataset_loop_device_encoder"] = {
        k: {"ms_per_batch": round(medians[k], 3), "images_per_s": round(BATCH / medians[k] * 1e3, 1), "runs": [round(x, 3) for x in v]}
        for k, v in loops.items()}
    result["dataset_loop_device_encoder"]["listing_costs_ms_per_batch"] = round(medians["with_ground_truth"] - medians["without"], 3)

    # (c) full annotations of resident label images against the restatement on host workers
    annotations = {}
    for name, images in inputs.items():
        times = []
        for _ in range(ROUNDS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            found, _ = creator.annotations_of_label_images(images, 0, 0)
            times.append((time.perf_counter() - t0) * 1e3)
        host_images = images.cpu().numpy()
        chunks = [list(range(BATCH))[i::args.workers] for i in range(args.workers) if list(range(BATCH))[i::args.workers]]
        host_times, done = [], None
        for _ in range(2):
            t0 = time.perf_counter()
            done = pool.map(_host_annotations, [host_images[chunk] for chunk in chunks])
            host_times.append((time.perf_counter() - t0) * 1e3)
        per_image = {}
        for chunk, lists in zip(chunks, done):
            for b, items in zip(chunk, lists):
                per_image[b] = [{k: v for k, v in a.items() if k not in ("id", "image_id")} for a in items]
        device_per_image = {b: [] for b in range(BATCH)}
        for a in found:
            device_per_image[a["image_id"]].append({k: v for k, v in a.items() if k not in ("id", "image_id")})
        ms = statistics.median(times)
        annotations[name] = {"annotations": len(found), "device_ms_per_batch": round(ms, 2), "device_images_per_s": round(BATCH / ms * 1e3, 1),
                             "host_workers": args.workers, "host_ms_per_batch": round(min(host_times), 1),
                             "host_images_per_s": round(BATCH / min(host_times) * 1e3, 1),
                             "equal_annotations": device_per_image == per_image}
    pool.close()
    pool.join()
    result["full_annotations"] = annotations
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
