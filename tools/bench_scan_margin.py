"""Scanner-margin removal on one MI355X: ``sis_hip.scan_content_box`` against the numpy / scipy restatement
of the same statement (tests/scan_margin_restatement.py, one host thread, equal output asserted), and
scripts/create_stylegan_train_dataset.py with and without ``--margin-remove`` on the same files.  The protocol is that of
tools/bench_scan_patches.py: warm-up, then five alternating runs, every run reported.

* ms per ``scan_content_box`` (device events, ``--steps`` calls per window) on two analysis images: the 1000 x 707 scan case of
  tests/scan_margin_cases.py, and the synthetic A4 page of tools/bench_scan_patches.py (2480 x 3508 at 300 dpi) laid on a
  scanner bed and thumbnailed to 1000 (707 x 1000); the restatement's ms for the same images.
* the one host read: per page, the wall time the host waits for the four integers of the box after everything is enqueued.
* the whole tool on 16 bed-margined A4 pages (PNG files), pages/s with and without the flag in alternating runs, and the
  share of the run with the flag that the waits for the box add up to.
* ``--trace-calls N``: nothing but N calls per image after a warm-up, for a kernel trace taken in a run of its own; its
  per-kernel statistics go into the result with ``--kernel-stats FILE`` (the trace tool's kernel statistics as CSV).

Writes profiles/scan_margin_bench.json and prints it.

    python tools/bench_scan_margin.py [--runs 5] [--tool-runs 5] [--kernel-stats stats.csv] [--out profiles/scan_margin_bench.json]
"""
import argparse
import csv
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "synthesis-in-style_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

PAGES, WORKERS, BED = 16, 16, 25


def bedded(array, seed=0):
    """The page on a scanner bed: 6 % of the page's width free on every side, +-3 noise on the bed."""
    h, w = array.shape[:2]
    m = round(0.06 * w)
    rng = np.random.RandomState(seed)
    out = np.clip(BED + rng.randint(-3, 4, size=(h + 2 * m, w + 2 * m, 3)), 0, 255).astype(np.uint8)
    out[m:m + h, m:m + w] = array
    return out


def runs_of(values, digits=3):
    return {"runs": [round(v, digits) for v in values], "median": round(statistics.median(values), digits)}


def tool_run(root, out, margin_remove):
    from scripts import create_stylegan_train_dataset as tool
    import torch
    args = tool.build_parser().parse_args([root, out, str(PAGES), "--seed", "1", "--pixel-path", "device", "--decode-workers", str(WORKERS)]
                                          + (["--margin-remove"] if margin_remove else []))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    train, val = tool.main(args)
    elapsed = time.perf_counter() - t0
    shutil.rmtree(out, ignore_errors=True)
    return PAGES / elapsed, len(train) + len(val)


def kernel_stats(path):
    """Rows of the trace tool's kernel statistics (CSV with Name, Calls, TotalDurationNs, AverageNs, Percentage) that name
    one of this library's kernels."""
    import sis_hip
    rows = []
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("KernelName") or ""
            if sis_hip.is_own_kernel(name):
                rows.append({"kernel": name.split("(")[0][-60:], "calls": int(row["Calls"]), "average_us": round(float(row["AverageNs"]) / 1e3, 2),
                             "total_us": round(float(row["TotalDurationNs"]) / 1e3, 1)})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--tool-runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--trace-calls", type=int, default=0)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scan_margin_bench.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_scan_margin needs a HIP device: nothing is measured without one")
    import sis_hip
    from PIL import Image
    import bench_scan_patches as B
    import scan_margin_cases as K
    import scan_margin_restatement as R
    device = torch.device("cuda:0")
    a4 = bedded(B.synthetic_scan(0))
    a4_page = torch.from_numpy(a4).to(device)
    images = {"scan_case_1000x707": torch.from_numpy(K.scan(K.TOOL_SCAN[0], K.TOOL_SCAN[1], 0)).to(device),
              "a4_300dpi_on_bed_thumbnail_1000": sis_hip.scan_thumbnail(a4_page, 1000)}
    if args.trace_calls:
        for image in images.values():
            for _ in range(args.warmup + args.trace_calls):
                sis_hip.scan_content_box(image)
        torch.cuda.synchronize()
        print(json.dumps({"trace_calls": args.trace_calls, "warmup": args.warmup, "images": list(images)}))
        return

    result = {"device": torch.cuda.get_device_name(0), "host_cpus_visible": len(os.sched_getaffinity(0)), "per_call_ms": {}}
    rows = {name: {"device": [], "restatement_1_thread": []} for name in images}
    for name, image in images.items():
        got = sis_hip.scan_content_box(image, edges=True, max_contours=4096)
        want = R.content_box(image.cpu().numpy())
        assert got.box.tolist() == want.box and got.info.tolist() == want.info, (name, got.box.tolist(), want.box, got.info.tolist(), want.info)
        assert np.array_equal(got.edges.cpu().numpy(), want.edges), name
        assert np.array_equal(got.contours[:want.info[0]].cpu().numpy(), want.contours), name
        rows[name].update(size=[int(image.shape[1]), int(image.shape[0])], box=want.box, info=want.info,
                          workspace_bytes=int(sis_hip.lib().sis_scan_content_box_workspace_bytes(int(image.shape[0]), int(image.shape[1]))))
    for _ in range(args.runs):   # the variants alternate
        for name, image in images.items():
            rows[name]["device"].append(B.event_ms(lambda: sis_hip.scan_content_box(image), args.steps, args.warmup))
            host = image.cpu().numpy()
            t0 = time.perf_counter()
            R.content_box(host)
            rows[name]["restatement_1_thread"].append((time.perf_counter() - t0) * 1e3)
    for name, row in rows.items():
        row["device"], row["restatement_1_thread"] = runs_of(row["device"], 4), runs_of(row["restatement_1_thread"], 1)
        row["restatement_over_device"] = round(row["restatement_1_thread"]["median"] / row["device"]["median"], 1)
        result["per_call_ms"][name] = row

    # the one host read of scan_remove_margin on the full page: enqueue everything, then wait for the box
    waits, device_ms = [], []
    for _ in range(args.warmup):
        sis_hip.scan_remove_margin(a4_page)
    for _ in range(args.runs):
        torch.cuda.synchronize()
        found = sis_hip.scan_content_box(sis_hip.scan_thumbnail(a4_page, 1000))
        t1 = time.perf_counter()
        found.box.tolist()
        t2 = time.perf_counter()
        waits.append((t2 - t1) * 1e3)
        device_ms.append(B.event_ms(lambda: sis_hip.scan_content_box(sis_hip.scan_thumbnail(a4_page, 1000)), 10, 2))
    cropped, box, crop = sis_hip.scan_remove_margin(a4_page)
    want_cropped, want_box, want_crop = R.remove_margin(a4)
    assert (box, crop) == (want_box, want_crop) and np.array_equal(cropped.cpu().numpy(), want_cropped)
    result["remove_margin_a4_on_bed"] = {"page": [int(a4.shape[1]), int(a4.shape[0])], "box": box, "crop": crop,
                                         "thumbnail_plus_content_box_device_ms": runs_of(device_ms, 3),
                                         "host_wait_for_the_box_ms": runs_of(waits, 3)}

    workdir = tempfile.mkdtemp(prefix="scan_margin_bench_")
    scans = os.path.join(workdir, "scans")
    os.makedirs(scans)
    base = B.synthetic_scan(0)
    for i in range(PAGES):   # bench_scan_patches.py's pages, each on the bed
        Image.fromarray(bedded(np.roll(base, 41 * i, axis=0), i)).save(os.path.join(scans, f"page_{i:02d}.png"), compress_level=1)
    loops, counts = {"without_flag": [], "with_margin_remove": []}, {}
    tool_run(scans, os.path.join(workdir, "warm0"), False)
    tool_run(scans, os.path.join(workdir, "warm1"), True)
    for run in range(args.tool_runs):
        for kind, flag in (("without_flag", False), ("with_margin_remove", True)):
            rate, counts[kind] = tool_run(scans, os.path.join(workdir, f"{kind}_{run}"), flag)
            loops[kind].append(rate)
    shutil.rmtree(workdir, ignore_errors=True)
    tool = {k: runs_of(v, 2) for k, v in loops.items()}
    with_seconds = PAGES / tool["with_margin_remove"]["median"]
    tool.update({"pages": PAGES, "patches_written": counts, "decode_workers": WORKERS, "source_files": "PNG, compress_level 1, A4 at 300 dpi on a bed",
                 "with_over_without": round(tool["with_margin_remove"]["median"] / tool["without_flag"]["median"], 3),
                 "host_wait_share_of_run_with_flag": round(PAGES * statistics.median(waits) / 1e3 / with_seconds, 4)})
    result["whole_tool_pages_per_s"] = tool
    if args.kernel_stats:
        result["kernel_trace_of_its_own"] = kernel_stats(args.kernel_stats)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
