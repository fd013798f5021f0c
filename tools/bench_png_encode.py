"""The dataset's PNG pairs on one MI355X: device encoder against PIL, at the dataset loop's shape -- B = 32 real
generator pairs of 256 x 512 (Generator(256) with random weights, label half = the grey cluster-id map of layer 13).

* device encode ms per batch (device events after warm-up), and per launch from a ``rocprofv3 --kernel-trace --stats`` run of its
  own (a child process started before this one opens the device; ``--no-profile`` skips it);
* ``Image.save`` of the same pairs on one host thread and on the writer pool's thread count;
* the copy of the encoded batch to pinned memory, and writing its files, each alone;
* ``create_dataset_for_segmentation.build_dataset`` images/s with ``-s DIR`` under ``--png-encoder pil`` (the loop as it was) and
  ``device``, beside the same loop without ``-s``: the variants alternate in this process, five runs, median and range;
* bytes per file of both encoders on the same generator output.

Writes profiles/png_encode_bench.json and prints it.

    python tools/bench_png_encode.py [--images 256] [--runs 5] [--out profiles/png_encode_bench.json]
"""
import argparse
import csv
import glob
import io
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "synthesis-in-style_amd"))

import numpy as np  # noqa: E402

SIZE, BATCH, CLUSTERS, LABEL_LAYER = 256, 32, 24, 13
CHANNELS = {8: 512, 9: 512, 12: 128, 13: 128}


def setup(workdir):
    """(generator, creation config, one batch of uint8 pairs on the device)."""
    import torch
    import sis_hip
    from networks.stylegan2.model import Generator
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
    files = {}
    for layer, channels in CHANNELS.items():
        files[str(layer)] = os.path.join(workdir, f"centres_{layer}.npy")
        np.save(files[str(layer)], rng.randn(CLUSTERS, channels).astype(np.float32))
    config = {"image_size": SIZE, "latent_size": 512, "n_mlp": 8, "seed": 1, "catalogs": files, "label_layer": LABEL_LAYER}
    torch.random.manual_seed(1)
    with torch.no_grad():
        image, acts = g([torch.randn(BATCH, g.style_dim).to(device)], noise=g.make_noise(), return_intermediate_activations=True)
        pixels = sis_hip.make_image_u8(image)
        labels = FactorCatalog(cluster_centers=np.load(files[str(LABEL_LAYER)])).predict(acts[LABEL_LAYER])
        grey = (labels * 255 // (CLUSTERS - 1)).to(torch.uint8)
        label = grey[..., None].expand(-1, -1, -1, 3).contiguous()
    return g, config, pixels, label


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


def spread(values, digits=3):
    return {"median": round(statistics.median(values), digits), "min": round(min(values), digits), "max": round(max(values), digits)}


def encode_only(launches):
    """What the profiler child runs: the encoder on one batch of pairs, a few times."""
    import torch
    import sis_hip
    workdir = tempfile.mkdtemp(prefix="png_encode_prof_")
    _, _, pixels, label = setup(workdir)
    for _ in range(launches):
        sis_hip.png_encode_pairs(pixels, label)
    torch.cuda.synchronize()
    shutil.rmtree(workdir, ignore_errors=True)


def kernel_stats(launches):
    """{kernel: {calls, mean_us, us_per_batch}} of the encoder's launches, from a rocprofv3 child process."""
    out = tempfile.mkdtemp(prefix="png_encode_prof_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--", sys.executable,
           os.path.abspath(__file__), "--encode-only", str(launches)]
    done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    found = glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True)
    if done.returncode != 0 or not found:
        return {"error": f"rocprofv3 exit {done.returncode}", "output_tail": done.stdout[-600:]}
    rows = {}
    for row in csv.DictReader(open(found[0])):
        name = row["Name"]
        if "png_" not in name and "fill" not in name.lower() and "memset" not in name.lower():
            continue
        short = name.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
        calls, total_ns = int(row["Calls"]), float(row["TotalDurationNs"])
        rows[short] = {"calls": calls, "mean_us": round(total_ns / calls / 1e3, 2), "us_per_batch": round(total_ns / launches / 1e3, 2)}
    shutil.rmtree(out, ignore_errors=True)
    return dict(sorted(rows.items(), key=lambda kv: -kv[1]["us_per_batch"]))


def pil_save(pairs, directory, threads):
    from PIL import Image

    def one(i):
        Image.fromarray(pairs[i]).save(os.path.join(directory, f"{i:04d}.png"))

    t0 = time.perf_counter()
    if threads == 1:
        for i in range(len(pairs)):
            one(i)
    else:
        with ThreadPoolExecutor(max_workers=threads) as pool:
            list(pool.map(one, range(len(pairs))))
    return (time.perf_counter() - t0) * 1e3


def write_files(buffer, sizes, directory, threads):
    def one(i):
        with open(os.path.join(directory, f"{i:04d}.png"), "wb") as f:
            f.write(memoryview(buffer[i, :int(sizes[i])]))

    t0 = time.perf_counter()
    with ThreadPoolExecutor(max_workers=threads) as pool:
        list(pool.map(one, range(buffer.shape[0])))
    return (time.perf_counter() - t0) * 1e3


def dataset_loop(g, config, images, encoder, save_to, writers):
    """images/s of build_dataset (the generator is handed over as built: loading a checkpoint is not what is timed)."""
    import torch
    import create_dataset_for_segmentation as cds
    cds.load_generator = lambda *a, **k: g
    args = argparse.Namespace(checkpoint=None, num_images=images, save_to=save_to, batch_size=BATCH, truncate=False,
                              png_encoder=encoder, png_writers=writers)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    done, _ = cds.build_dataset(args, config)
    elapsed = time.perf_counter() - t0
    assert done == images
    return images / elapsed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=256, help="images per run of the dataset loop")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--writers", type=int, default=4)
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--encode-only", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "png_encode_bench.json"))
    args = ap.parse_args()
    if args.encode_only:
        return encode_only(args.encode_only)
    stats = None if args.no_profile else kernel_stats(10)   # the profiler child has finished before this process opens the device
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_png_encode needs a HIP device: nothing is measured without one")
    import sis_hip
    workdir = tempfile.mkdtemp(prefix="png_encode_bench_")
    g, config, pixels, label = setup(workdir)
    buffer, sizes = sis_hip.png_encode_pairs(pixels, label)
    host_buffer = torch.empty(buffer.shape, dtype=torch.uint8, pin_memory=True)
    pairs = np.concatenate([pixels.cpu().numpy(), label.cpu().numpy()], axis=2)
    from PIL import Image
    sizes_host = sizes.cpu().numpy()
    for i in (0, BATCH - 1):
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(buffer[i, :sizes_host[i]].cpu().numpy().tobytes()))), pairs[i])
    scratch = os.path.join(workdir, "files")
    os.makedirs(scratch)
    pil_bytes = []
    for i in range(BATCH):
        out = io.BytesIO()
        Image.fromarray(pairs[i]).save(out, format="PNG")
        pil_bytes.append(out.tell())
    result = {"device": torch.cuda.get_device_name(0),
              "shape": {"batch": BATCH, "height": SIZE, "image_width": SIZE, "label_width": SIZE, "label": f"grey cluster ids of layer {LABEL_LAYER}",
                        "buffer_stride_bytes": int(buffer.shape[1])},
              "bytes_per_file": {"device": spread([int(s) for s in sizes_host], 0), "pil": spread(pil_bytes, 0),
                                 "device_over_pil": round(float(sizes_host.mean()) / float(np.mean(pil_bytes)), 3)},
              "kernels_rocprofv3": stats}
    encode, copy, save1, savep, write1, writep = [], [], [], [], [], []
    for _ in range(args.runs):   # the variants alternate
        encode.append(event_ms(lambda: sis_hip.png_encode_pairs(pixels, label), args.steps, args.warmup))
        copy.append(event_ms(lambda: host_buffer.copy_(buffer, non_blocking=True), args.steps, 2))
        save1.append(pil_save(pairs, scratch, 1))
        savep.append(pil_save(pairs, scratch, args.writers))
        write1.append(write_files(host_buffer.numpy(), sizes_host, scratch, 1))
        writep.append(write_files(host_buffer.numpy(), sizes_host, scratch, args.writers))
    result["per_batch_ms"] = {"device_encode": spread(encode), "copy_whole_buffer_to_pinned": spread(copy),
                              "pil_save_one_thread": spread(save1, 1), f"pil_save_{args.writers}_threads": spread(savep, 1),
                              "write_device_files_one_thread": spread(write1, 2),
                              f"write_device_files_{args.writers}_threads": spread(writep, 2)}
    result["host_cpus_visible"] = len(os.sched_getaffinity(0))
    loops = {"no_save": [], "save_pil": [], "save_device": []}
    for kind in loops:   # one warm-up run each
        dataset_loop(g, config, 2 * BATCH, "device" if kind == "save_device" else "pil", None if kind == "no_save" else os.path.join(workdir, "warm"),
                     args.writers)
    for run in range(args.runs):
        for kind in loops:
            save_to = None if kind == "no_save" else os.path.join(workdir, f"{kind}_{run}")
            loops[kind].append(dataset_loop(g, config, args.images, "device" if kind == "save_device" else "pil", save_to, args.writers))
            if save_to:
                shutil.rmtree(save_to, ignore_errors=True)
    base = statistics.median(loops["no_save"])
    result["dataset_loop_images_per_s"] = {k: spread(v, 1) for k, v in loops.items()}
    result["dataset_loop_images_per_s"]["images_per_run"] = args.images
    result["dataset_loop_images_per_s"]["share_of_no_save"] = {k: round(statistics.median(v) / base, 3) for k, v in loops.items() if k != "no_save"}
    result["dataset_loop_images_per_s"]["device_over_pil"] = round(statistics.median(loops["save_device"]) / statistics.median(loops["save_pil"]), 2)
    shutil.rmtree(workdir, ignore_errors=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
