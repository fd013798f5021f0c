"""Page evaluation on one MI355X: the contour filter per launch against the HBM roofline and against the host
restatement (tests/page_eval_restatement.py on 16 worker processes, plus the two PCIe transfers a host path needs), and one
2480 x 3508 page end to end through DocUFCN + VotingAssemblySegmenter + confusion matrix with ``min_contour_area`` 55 and 0.

Times are device events after warm-up.  An untrained DocUFCN answers about 1/3 everywhere, so the confidence threshold is set
to a quantile of its own outputs on the page (``--keep``: the share of non-background confidences that survive); the filter
then sees speckle and blobs instead of empty planes.  Writes profiles/page_eval_bench.json and prints it.

    python tools/bench_page_eval.py [--steps 20] [--warmup 3] [--out profiles/page_eval_bench.json]
"""
import argparse
import json
import multiprocessing
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "synthesis-in-style_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

HBM_ACHIEVABLE = 6.3e12   # bytes/s, float4 copy on this part
FILTER_SHAPES = [(16, 3, 256, 256), (8, 3, 512, 512)]


def _host_planes(job):
    import page_eval_restatement as R
    planes, min_area = job
    return np.stack([p * R.keep_mask(p, min_area) for p in planes])


def host_filter(pool, pred, min_confidence, min_area, background, workers):
    """The restatement, planes spread over the worker processes."""
    import page_eval_restatement as R
    q = R.threshold(pred, min_confidence)
    out = q.copy()
    todo = [(b, c) for b in range(q.shape[0]) for c in range(q.shape[1]) if c != background]
    chunks = [todo[i::workers] for i in range(workers) if todo[i::workers]]
    done = pool.map(_host_planes, [(np.stack([q[b, c] for b, c in chunk]), min_area) for chunk in chunks])
    for chunk, planes in zip(chunks, done):
        for (b, c), plane in zip(chunk, planes):
            out[b, c] = plane
    return out


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


def bench_filter(pool, workers, steps, warmup):
    import torch
    import page_eval_restatement as R
    import sis_hip
    dev = torch.device("cuda:0")
    rows = []
    for shape in FILTER_SHAPES:
        rng = np.random.RandomState(shape[2])
        pred = R.smooth_noise_planes(rng, shape, 0.15, sigma=4.0)
        x = torch.from_numpy(pred).to(dev)
        got = sis_hip.remove_small_contours(x, 0.7, 55, 0)
        ms = event_ms(lambda: sis_hip.remove_small_contours(x, 0.7, 55, 0), steps, warmup)
        threshold_ms = event_ms(lambda: torch.where(x < 0.7, torch.zeros_like(x), x), steps, warmup)
        row = {"shape": list(shape), "min_confidence": 0.7, "min_contour_area": 55,
               "device_ms_per_launch": round(ms, 4), "threshold_only_torch_where_ms": round(threshold_ms, 4),
               "algorithmic_bytes": 8.0 * x.numel(),   # one read of the predictions, one write of the result
               "achieved_GBps": round(8.0 * x.numel() / (ms * 1e-3) / 1e9, 1),
               "share_of_achievable_hbm": round(8.0 * x.numel() / (ms * 1e-3) / HBM_ACHIEVABLE, 4)}
        rows.append(row)
        if pool is None:   # --workers 0 (profiler runs): the device side alone
            continue
        pinned_in, pinned_out = torch.empty(shape, dtype=torch.float32).pin_memory(), torch.empty(shape, dtype=torch.float32).pin_memory()
        host = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pinned_in.copy_(x)                                            # device -> host
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            out = host_filter(pool, pinned_in.numpy(), 0.7, 55, 0, workers)
            t2 = time.perf_counter()
            pinned_out.copy_(torch.from_numpy(out))
            x.new_empty(shape).copy_(pinned_out, non_blocking=False)      # host -> device
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            host.append(((t3 - t0) * 1e3, (t1 - t0 + t3 - t2) * 1e3))
        host_ms, transfer_ms = min(host)
        if not torch.equal(got.cpu(), torch.from_numpy(out)):
            raise RuntimeError(f"device and host filter differ at {shape}")
        row.update({"host_restatement_ms": round(host_ms, 2), "host_transfers_ms": round(transfer_ms, 2), "host_workers": workers,
                    "host_over_device": round(host_ms / ms, 1), "outputs_equal": True})
    return rows


def synthetic_page(width, height, seed=0):
    """Light paper with dark strokes of two inks; the ground truth is the ink map."""
    rng = np.random.RandomState(seed)
    truth = np.zeros((height, width), dtype=np.uint8)
    for _ in range(1500):
        cls = rng.randint(1, 3)
        h, w = rng.randint(4, 28), rng.randint(30, 260)
        top, left = rng.randint(0, height - h), rng.randint(0, width - w)
        truth[top:top + h, left:left + w] = cls
    ink = np.asarray([[242, 240, 232], [30, 30, 60], [40, 60, 160]], dtype=np.int64)
    page = np.clip(ink[truth] + rng.randint(-12, 13, size=(height, width, 3)), 0, 255).astype(np.uint8)
    return page, truth


def bench_page(steps, warmup, keep):
    import torch
    import torch.nn.functional as F
    import sis_hip
    from networks.doc_ufcn import DocUFCN
    from segmentation.analysis_segmenter import VotingAssemblySegmenter
    dev = torch.device("cuda:0")
    width, height, patch, batch = 2480, 3508, 256, 16
    page_np, truth_np = synthetic_page(width, height)
    page, truth = torch.from_numpy(page_np).to(dev), torch.from_numpy(truth_np).to(dev)
    torch.manual_seed(0)
    net = DocUFCN(3, 3).to(dev).eval()
    seg = VotingAssemblySegmenter(net, patch, dev, batch_size=batch, patch_overlap_factor=0.25)
    xs, ys = seg.patch_grid(width, height)
    with torch.no_grad():
        first = F.softmax(net(sis_hip.crop_patches_u8(page, xs, ys, patch)[:batch]), dim=1)
    net.min_confidence = float(first[:, 1:].flatten()[::97].quantile(1.0 - keep))
    matrix = torch.zeros((3, 3), dtype=torch.int64, device=dev)

    def step():
        assembled = seg.segment_image(page)
        sis_hip.confusion_matrix(assembled, truth, 3, out=matrix)

    def staged(stages):
        """The same step with an event pair around every stage."""
        def ev():
            return torch.cuda.Event(enable_timing=True)
        marks = []

        def timed(name, fn):
            a, b = ev(), ev()
            a.record()
            r = fn()
            b.record()
            marks.append((name, a, b))
            return r
        with torch.no_grad():
            patches = timed("crop", lambda: sis_hip.crop_patches_u8(page, xs, ys, patch))
            outs = []
            for i in range(0, patches.shape[0], batch):
                soft = timed("network+softmax", lambda: F.softmax(net(patches[i:i + batch]), dim=1))
                outs.append(timed("postprocess", lambda: net.postprocess(soft)))
            preds = timed("concatenate", lambda: torch.cat(outs, dim=0))
            assembled = timed("vote", lambda: seg.assemble_predictions(preds, (width, height)))
            timed("confusion_matrix", lambda: sis_hip.confusion_matrix(assembled, truth, 3, out=matrix))
        torch.cuda.synchronize()
        for name, a, b in marks:
            stages[name] = stages.get(name, 0.0) + a.elapsed_time(b)

    out = {"page": [width, height], "patch": patch, "patch_overlap_factor": 0.25, "batch": batch, "patches": len(xs) * len(ys),
           "network": "DocUFCN(3, 3) untrained, eval", "min_confidence": round(net.min_confidence, 6), "kept_share": keep}
    for area in (55, 0, 55, 0):   # alternating, the better of two windows each
        net.min_contour_area = area
        with torch.no_grad():
            ms = event_ms(step, steps, warmup)
        key = f"min_contour_area_{area}"
        if key not in out or ms < out[key]["page_ms"]:
            out[key] = {"page_ms": round(ms, 3), "pages_per_s": round(1e3 / ms, 3)}
    for area in (55, 0):
        net.min_contour_area = area
        stages = {}
        staged({})
        for _ in range(3):
            staged(stages)
        total = sum(stages.values())
        out[f"min_contour_area_{area}"]["stage_ms"] = {k: round(v / 3, 3) for k, v in stages.items()}
        out[f"min_contour_area_{area}"]["stage_share"] = {k: round(v / total, 4) for k, v in stages.items()}
    out["slowdown_55_over_0"] = round(out["min_contour_area_55"]["page_ms"] / out["min_contour_area_0"]["page_ms"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--page-steps", type=int, default=3)
    ap.add_argument("--keep", type=float, default=0.15)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--skip-page", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "page_eval_bench.json"))
    args = ap.parse_args()
    # the workers are forked before the device is opened and never touch it
    pool = multiprocessing.get_context("fork").Pool(args.workers) if args.workers > 0 else None
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_page_eval needs a HIP device: nothing is measured without one")
    result = {"device": torch.cuda.get_device_name(0), "hbm_achievable_Bps": HBM_ACHIEVABLE,
              "contour_filter": bench_filter(pool, args.workers, args.steps, args.warmup)}
    if pool is not None:
        pool.close()
        pool.join()
    if not args.skip_page:
        result["page"] = bench_page(args.page_steps, 1, args.keep)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
