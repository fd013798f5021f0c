"""Cluster-based labeller on one MI355X at the shipped config's shape: Generator(256), B = 32, class
determination on layers 8 / 9 (64 x 64), fine-grained segmentation on layers 12 / 13 (256 x 256), three classes.

* the label pass alone (k-means maps + labeller, and the labeller on finished maps), device events after warm-up;
* per-kernel times from a ``rocprofv3 --kernel-trace --stats`` run of its own (a child process started before this one opens
  the device; ``--no-profile`` skips it);
* the dataset loop's images/s with this labeller, with the k-means maps only, and bare synthesis, in this process, alternating,
  the best window of each;
* the definition's restatement (tests/cluster_segmenter_restatement.py) on 16 host workers for the same cluster maps.

The generator has random weights and the catalogs random unit centres (24 per layer, as bench.py's dataset workload), so the
class of a cluster is made up: per layer the clusters are ranked by how many pixels of one probe batch they take, the largest
are background until ``--background`` of the pixels is covered, the others alternate between the two text classes.
Writes profiles/cluster_segmenter_bench.json and prints it.

    python tools/bench_cluster_segmenter.py [--steps 20] [--warmup 5] [--out profiles/cluster_segmenter_bench.json]
"""
import argparse
import csv
import glob
import json
import multiprocessing
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "synthesis-in-style_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

SIZE, BATCH, CLUSTERS = 256, 32, 24
CHANNELS = {"8": 512, "9": 512, "12": 128, "13": 128}
COLOURS = {"background": "#000000", "printed_text": "#0000FF", "handwritten_text": "#FF0000"}
CONFIG = {"keys_for_class_determination": ["8", "9"], "keys_for_finegrained_segmentation": ["12", "13"], "keys_to_merge": {},
          "only_keep_overlapping": False, "min_class_contour_area": 50}   # the reference's stylegan2_cluster_based_bw_hwp_wpi.json


def setup(background_share):
    """(generator, segmenter, k-means-only catalogs, spec for the restatement, probe activations)."""
    import torch
    import cluster_segmenter_restatement as R
    from networks.stylegan2.model import Generator
    from segmentation.black_white_handwritten_printed_text_segmenter import BlackWhiteHandwrittenPrintedTextDatasetSegmenter
    from segmentation.gan_local_edit.factor_catalog import FactorCatalog
    device = torch.device("cuda:0")
    torch.manual_seed(0)
    g = Generator(SIZE, 512, 8, channel_multiplier=2)   # as bench.py's dataset workload: random weights, noise weights that matter
    with torch.no_grad():
        for name, p in g.named_parameters():
            if name.endswith("noise.weight"):
                p.normal_(0.0, 0.1)
    g = g.to(device).eval()
    rng = np.random.RandomState(7)
    centres = {}
    for key, channels in CHANNELS.items():
        c = rng.randn(CLUSTERS, channels).astype(np.float32)
        centres[key] = c / np.linalg.norm(c, axis=1, keepdims=True)
    catalogs = {int(k): FactorCatalog(cluster_centers=c) for k, c in centres.items()}
    torch.random.manual_seed(1)
    with torch.no_grad():
        _, acts = g([torch.randn(BATCH, g.style_dim).to(device)], noise=g.make_noise(), return_intermediate_activations=True)
    table = {}
    for key in CHANNELS:
        counts = torch.bincount(catalogs[int(key)].predict(acts[int(key)]).flatten(), minlength=CLUSTERS).cpu().numpy()
        order, covered, names, text = np.argsort(-counts), 0, {}, 0
        for cluster in order:
            if covered < background_share * counts.sum():
                names[int(cluster)] = "background"
            else:
                names[int(cluster)] = ("printed_text", "handwritten_text")[text % 2]
                text += 1
            covered += counts[cluster]
        table[key] = names
    spec = R.make_spec(size=SIZE, clusters_to_class=table, keys=tuple(CHANNELS), **CONFIG)
    base = tempfile.mkdtemp(prefix="cluster_segmenter_bench_")
    os.makedirs(os.path.join(base, "catalogs", str(CLUSTERS)))
    files = {}
    for key, c in centres.items():
        files[key] = os.path.join(str(CLUSTERS), f"centres_{key}.npy")
        np.save(os.path.join(base, "catalogs", files[key]), c)
    with open(os.path.join(base, "catalogs", f"{CLUSTERS}.json"), "w") as f:
        json.dump({"catalogs": files}, f)
    with open(os.path.join(base, f"merged_classes_{CLUSTERS}.json"), "w") as f:
        json.dump(spec["clusters_to_class"], f)
    from pathlib import Path
    segmenter = BlackWhiteHandwrittenPrintedTextDatasetSegmenter(
        base_dir=Path(base), image_size=SIZE, class_to_color_map=COLOURS, num_clusters=CLUSTERS, **CONFIG)
    return g, segmenter, catalogs, spec, acts


def event_ms(fn, steps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def label_only(launches, background_share):
    """What the profiler child runs: the label pass on one batch's activations, a few times."""
    import torch
    _, segmenter, _, _, acts = setup(background_share)
    for _ in range(launches):
        segmenter.label_activations(acts)
    torch.cuda.synchronize()


def kernel_stats(launches, background_share):
    """{kernel: {calls, mean_us, us_per_label_pass}} of the label pass's own kernels, from a rocprofv3 child process."""
    out = tempfile.mkdtemp(prefix="cluster_segmenter_prof_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--", sys.executable,
           os.path.abspath(__file__), "--label-only", str(launches), "--background", str(background_share)]
    done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    found = glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True)
    if done.returncode != 0 or not found:
        return {"error": f"rocprofv3 exit {done.returncode}", "output_tail": done.stdout[-600:]}
    rows = {}
    for row in csv.DictReader(open(found[0])):
        name = row["Name"]
        if not any(tag in name for tag in ("cluster_", "contour_", "kmeans")):
            continue
        short = name.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
        calls, total_ns = int(row["Calls"]), float(row["TotalDurationNs"])
        rows[short] = {"calls": calls, "mean_us": round(total_ns / calls / 1e3, 2), "us_per_label_pass": round(total_ns / launches / 1e3, 2)}
    return dict(sorted(rows.items(), key=lambda kv: -kv[1]["us_per_label_pass"]))


def _host_images(job):
    import cluster_segmenter_restatement as R
    maps, spec = job
    return [R.segment_image({k: v[b] for k, v in maps.items()}, spec) for b in range(len(next(iter(maps.values()))))]


def loops(g, segmenter, catalogs, steps, warmup, rounds=3):
    import torch
    from utils.dataset_creation import label_and_encode, seeded_latents
    device = torch.device("cuda:0")

    def batch_of(kind):
        with torch.no_grad():
            z = seeded_latents(BATCH, g.style_dim, device).to(device, non_blocking=True)
            image, acts = g([z], noise=g.make_noise(), return_intermediate_activations=True)
            if kind == "synthesis":
                return image
            if kind == "kmeans_only":
                return label_and_encode(image, acts, catalogs)
            return label_and_encode(image, acts, {}, None, segmenter)

    best = {}
    for _ in range(rounds):
        for kind in ("synthesis", "kmeans_only", "cluster_segmenter"):
            for _ in range(warmup):
                batch_of(kind)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                batch_of(kind)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) / steps * 1e3
            best[kind] = min(best.get(kind, ms), ms)
    return {k: {"ms_per_batch": round(v, 3), "images_per_s": round(BATCH / v * 1e3, 1)} for k, v in best.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--background", type=float, default=0.75, help="share of a layer's pixels whose clusters are background")
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--label-only", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cluster_segmenter_bench.json"))
    args = ap.parse_args()
    if args.label_only:
        return label_only(args.label_only, args.background)
    # the workers are forked and the profiler child has finished before this process opens the device
    pool = multiprocessing.get_context("fork").Pool(args.workers) if args.workers > 0 else None
    stats = None if args.no_profile else kernel_stats(10, args.background)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_cluster_segmenter needs a HIP device: nothing is measured without one")
    import cluster_segmenter_restatement as R
    g, segmenter, catalogs, spec, acts = setup(args.background)
    maps = {k: segmenter.catalog[k].predict(acts[int(k)]) for k in CHANNELS}
    class_map, colour, drop = segmenter.label_cluster_maps(maps)
    result = {"device": torch.cuda.get_device_name(0),
              "shape": {"generator": SIZE, "batch": BATCH, "clusters_per_layer": CLUSTERS, "classes": 3, **CONFIG,
                        "resolutions": {k: int(m.shape[-1]) for k, m in maps.items()}, "background_share": args.background},
              "labelled_share_of_pixels": round(float((class_map != 0).float().mean()), 4),
              "dropped_of_probe_batch": int(drop.sum()),
              "label_pass_ms": {
                  "kmeans_maps_and_labeller": round(event_ms(lambda: segmenter.label_activations(acts), args.steps, args.warmup), 4),
                  "labeller_on_finished_maps": round(event_ms(lambda: segmenter.label_cluster_maps(maps), args.steps, args.warmup), 4),
                  "kmeans_maps_only": round(event_ms(lambda: [c.predict(acts[k]) for k, c in catalogs.items()], args.steps,
                                                     args.warmup), 4)},
              "kernels_rocprofv3": stats}
    if pool is not None:
        host_maps = {k: m.cpu().numpy() for k, m in maps.items()}
        chunks = [list(range(BATCH))[i::args.workers] for i in range(args.workers) if list(range(BATCH))[i::args.workers]]
        times, done = [], None
        for _ in range(2):
            t0 = time.perf_counter()
            done = pool.map(_host_images, [({k: v[chunk] for k, v in host_maps.items()}, spec) for chunk in chunks])
            times.append((time.perf_counter() - t0) * 1e3)
        pool.close()
        pool.join()
        host_classes = np.zeros((BATCH, SIZE, SIZE), dtype=np.uint8)
        for chunk, images in zip(chunks, done):
            for b, (classes, _) in zip(chunk, images):
                host_classes[b] = classes
        result["host_restatement"] = {"workers": args.workers, "ms_per_batch": round(min(times), 1),
                                      "equals_device_class_map": bool(np.array_equal(host_classes, class_map.cpu().numpy()))}
        result["host_restatement"]["over_device_labeller"] = round(
            min(times) / result["label_pass_ms"]["labeller_on_finished_maps"], 1)
    result["dataset_loop"] = loops(g, segmenter, catalogs, args.steps, args.warmup)
    loop = result["dataset_loop"]
    result["dataset_loop"]["labeller_over_kmeans_only_ms"] = round(
        loop["cluster_segmenter"]["ms_per_batch"] - loop["kmeans_only"]["ms_per_batch"], 3)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
