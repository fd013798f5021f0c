"""GAN training patches from one scanned page on one MI355X: the device path of
scripts/create_stylegan_train_dataset.py against its Pillow path, which is the yardstick.

The page is a synthetic A4 scan at 300 dpi (2480 x 3508, RGB).  With the tool's defaults (--max-size 3000, --min-size 1000,
--image-size 256) it is first shrunk to 2121 x 3000 and then, for the drawn downsample factor, left alone (factor 1: 108
patches) or shrunk to 707 x 1000 (factor 4: 12 patches).

* per page and factor, ms of the three steps -- thumbnail, gather (crop), PNG encode -- on the device (device events after
  warm-up; the host-side tap tables are cached after the first page and timed apart) and with Pillow in this process on one
  host thread and on 16 (16 pages at once, wall time / 16).  File writes are left out on both sides.  The variants alternate,
  five runs, median and range.
* the whole tool on a directory of 16 such pages (PNG files), decode and file writes included: pages/s of both pixel paths,
  alternating runs, and the share of the run that decoding the files alone takes.

Writes profiles/scan_patches_bench.json and prints it.

    python tools/bench_scan_patches.py [--runs 5] [--tool-runs 3] [--out profiles/scan_patches_bench.json]
"""
import argparse
import io
import json
import os
import shutil
import statistics
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "synthesis-in-style_amd"))

import numpy as np  # noqa: E402

WIDTH, HEIGHT, MAX_SIZE, MIN_SIZE, IMAGE_SIZE, PAGES, WORKERS = 2480, 3508, 3000, 1000, 256, 16, 16


def synthetic_scan(seed):
    """Paper-like ground with noise, and dark text-like strokes in lines."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:HEIGHT, 0:WIDTH]
    ground = (228 + 12 * np.sin(x / 310.0) * np.cos(y / 270.0)).astype(np.float32)
    a = ground[:, :, None] + rng.normal(0, 3, (HEIGHT, WIDTH, 3)).astype(np.float32)
    for line in range(200, HEIGHT - 200, 60):
        xs = 200
        while xs < WIDTH - 250:
            w = int(rng.integers(8, 60))
            a[line:line + int(rng.integers(18, 34)), xs:xs + w] = rng.integers(10, 70)
            xs += w + int(rng.integers(6, 30))
    return np.clip(a, 0, 255).astype(np.uint8)


def spread(values, digits=3):
    return {"median": round(statistics.median(values), digits), "min": round(min(values), digits), "max": round(max(values), digits)}


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


def pil_steps(array, factor):
    """(thumbnail ms, crop ms, encode ms) of one page with Pillow on the calling thread."""
    from PIL import Image
    from scripts.create_stylegan_train_dataset import crop_patches
    from utils.scan_patches import random_resize_size
    image = Image.fromarray(array)
    t0 = time.perf_counter()
    image.thumbnail((MAX_SIZE, MAX_SIZE))
    side = random_resize_size(image.width, image.height, factor, MIN_SIZE)
    image.thumbnail((side, side))
    t1 = time.perf_counter()
    patches = crop_patches(image, IMAGE_SIZE)
    for patch in patches:
        patch.load()
    t2 = time.perf_counter()
    for patch in patches:
        patch.save(io.BytesIO(), format="PNG")
    t3 = time.perf_counter()
    return (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3


def pil_pool(array, factor, pool):
    """Wall ms per page of the three steps together with WORKERS pages in flight."""
    t0 = time.perf_counter()
    list(pool.map(lambda _: pil_steps(array, factor), range(WORKERS)))
    return (time.perf_counter() - t0) * 1e3 / WORKERS


def tool_run(root, out, pixel_path):
    from scripts import create_stylegan_train_dataset as tool
    import torch
    args = tool.build_parser().parse_args([root, out, str(PAGES), "--seed", "1", "--pixel-path", pixel_path, "--decode-workers", str(WORKERS)])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    train, val = tool.main(args)
    elapsed = time.perf_counter() - t0
    shutil.rmtree(out, ignore_errors=True)
    return PAGES / elapsed, len(train) + len(val)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--tool-runs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scan_patches_bench.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_scan_patches needs a HIP device: nothing is measured without one")
    import sis_hip
    from PIL import Image
    from scripts.create_stylegan_train_dataset import decode_page
    from utils import scan_patches as tables
    device = torch.device("cuda:0")
    array = synthetic_scan(0)
    page = torch.from_numpy(array).to(device)
    result = {"device": torch.cuda.get_device_name(0), "host_cpus_visible": len(os.sched_getaffinity(0)), "pillow": Image.__version__,
              "page": {"width": WIDTH, "height": HEIGHT, "max_size": MAX_SIZE, "min_size": MIN_SIZE, "image_size": IMAGE_SIZE},
              "per_page_ms": {}}
    pool = ThreadPoolExecutor(max_workers=WORKERS)
    for factor in (1, 4):
        def shrink():
            p = sis_hip.scan_thumbnail(page, MAX_SIZE)
            return sis_hip.scan_thumbnail(p, tables.random_resize_size(int(p.shape[1]), int(p.shape[0]), factor, MIN_SIZE))

        tables.axis_table.cache_clear()
        t0 = time.perf_counter()
        small = shrink()
        torch.cuda.synchronize()
        first_call_ms = (time.perf_counter() - t0) * 1e3   # with the host tables built (Python floats), uploaded, and the launches
        origins = tables.patch_origins(int(small.shape[1]), int(small.shape[0]), IMAGE_SIZE)
        patches = sis_hip.scan_patches(small, origins, IMAGE_SIZE)
        want = Image.fromarray(array)
        want.thumbnail((MAX_SIZE, MAX_SIZE))
        side = tables.random_resize_size(want.width, want.height, factor, MIN_SIZE)
        want.thumbnail((side, side))
        assert np.array_equal(small.cpu().numpy(), np.asarray(want)), "the device page is not Pillow's"
        rows = {k: [] for k in ("device_thumbnail", "device_gather", "device_encode", "pil_thumbnail_1", "pil_crop_1", "pil_encode_1",
                                "pil_all_steps_1", f"pil_all_steps_{WORKERS}_workers")}
        for _ in range(args.runs):   # the variants alternate
            rows["device_thumbnail"].append(event_ms(shrink, args.steps, args.warmup))
            rows["device_gather"].append(event_ms(lambda: sis_hip.scan_patches(small, origins, IMAGE_SIZE), args.steps, args.warmup))
            rows["device_encode"].append(event_ms(lambda: sis_hip.png_encode_pairs(patches), args.steps, args.warmup))
            a, b, c = pil_steps(array, factor)
            rows["pil_thumbnail_1"].append(a)
            rows["pil_crop_1"].append(b)
            rows["pil_encode_1"].append(c)
            rows["pil_all_steps_1"].append(a + b + c)
            rows[f"pil_all_steps_{WORKERS}_workers"].append(pil_pool(array, factor, pool))
        entry = {k: spread(v) for k, v in rows.items()}
        device_all = sum(statistics.median(rows[k]) for k in ("device_thumbnail", "device_gather", "device_encode"))
        entry["device_all_steps_median"] = round(device_all, 3)
        entry["device_first_thumbnail_with_host_tables"] = round(first_call_ms, 2)
        entry["size_after_thumbnail"] = [int(small.shape[1]), int(small.shape[0])]
        entry["patches"] = len(origins)
        entry["pil_1_over_device"] = round(statistics.median(rows["pil_all_steps_1"]) / device_all, 2)
        entry[f"pil_{WORKERS}_workers_over_device"] = round(statistics.median(rows[f"pil_all_steps_{WORKERS}_workers"]) / device_all, 2)
        result["per_page_ms"][f"factor_{factor}"] = entry
    pool.shutdown()

    workdir = tempfile.mkdtemp(prefix="scan_patches_bench_")
    scans = os.path.join(workdir, "scans")
    os.makedirs(scans)
    for i in range(PAGES):   # the same scan moved down by a few lines: other bytes, the same statistics
        Image.fromarray(np.roll(array, 41 * i, axis=0)).save(os.path.join(scans, f"page_{i:02d}.png"), compress_level=1)
    files = sorted(os.path.join(scans, name) for name in os.listdir(scans))
    decode = []
    loops = {"pil": [], "device": []}
    tool_run(scans, os.path.join(workdir, "warm"), "device")   # one warm-up run of the device path (the Pillow path has nothing to warm)
    for run in range(args.tool_runs):
        with ThreadPoolExecutor(max_workers=WORKERS) as decoders:
            t0 = time.perf_counter()
            list(decoders.map(decode_page, files))
            decode.append(time.perf_counter() - t0)
        for kind in loops:
            rate, count = tool_run(scans, os.path.join(workdir, f"{kind}_{run}"), kind)
            loops[kind].append(rate)
    shutil.rmtree(workdir, ignore_errors=True)
    tool = {k: spread(v, 2) for k, v in loops.items()}
    tool.update({"pages": PAGES, "patches_written": count, "decode_workers": WORKERS, "source_files": "PNG, compress_level 1",
                 "decode_alone_seconds": spread(decode, 3),
                 "decode_share_of_run": {k: round(statistics.median(decode) / (PAGES / statistics.median(v)), 3) for k, v in loops.items()},
                 "device_over_pil": round(statistics.median(loops["device"]) / statistics.median(loops["pil"]), 2)})
    result["whole_tool_pages_per_s"] = tool
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
