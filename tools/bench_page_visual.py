"""Page visualisation on one MI355X at the size of a real page: one synthetic A4 scan at 300 dpi, 2480 x 3508
pixels, three classes, smooth-noise confidences (tests/page_eval_restatement.py) thresholded at 0.7.

* ``sis_hip.page_regions`` (tables and label maps), ``sis_hip.page_render`` with all four pictures, region and patch boxes, in
  the plain and in the confidence mode, and ``sis_hip.page_crops`` in both modes over every kept region: device events after
  warm-up, five alternating runs, the median;
* beside them the numpy / scipy / PIL restatement of the same outputs on the host (tests/page_visual_restatement.py for the
  regions, the colouring, the overlay and the crops, ``ImageDraw.rectangle`` for the outlines), wall clock, one run.  Its
  confidence colouring is VECTORISED; the reference walks every non-background pixel of the page in a Python loop, which is
  slower still;
* whether the device's tables, label maps, colouring and overlay equal the restatement's at this size.

Writes profiles/page_visual_bench.json and prints it.

    python tools/bench_page_visual.py [--steps 5] [--warmup 2] [--out profiles/page_visual_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "synthesis-in-style_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

WIDTH, HEIGHT, CLASSES, PATCH = 2480, 3508, 3, 256
COLOURS = [(0, 0, 0), (0, 0, 255), (255, 0, 0)]
ROUNDS = 5


def event_ms(fn, steps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(steps):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / steps


def wall_ms(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


def host_boxes(base, region_boxes, patch_boxes):
    from PIL import Image, ImageDraw
    image = Image.fromarray(base)
    draw = ImageDraw.Draw(image)
    for box in region_boxes:
        draw.rectangle(box, outline=(0, 255, 0), width=3)
    for box in patch_boxes:
        draw.rectangle(box, outline=(255, 0, 0), width=1)
    return np.array(image)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "page_visual_bench.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_page_visual needs a HIP device: nothing is measured without one")
    import page_eval_restatement as E
    import page_visual_restatement as V
    import sis_hip
    from segmentation.analysis_segmenter import AnalysisSegmenter

    device = torch.device("cuda:0")
    pred = E.threshold(E.smooth_noise_planes(np.random.RandomState(3), (CLASSES, HEIGHT, WIDTH), 0.15), 0.7)
    scan = np.random.RandomState(4).randint(0, 256, (HEIGHT, WIDTH, 3)).astype(np.uint8)
    patches = [tuple(int(v) for v in b)
               for b in AnalysisSegmenter(torch.nn.Identity(), PATCH, device).calculate_bboxes_for_patches(WIDTH, HEIGHT)]
    x, page = torch.from_numpy(pred).to(device), torch.from_numpy(scan).to(device)
    patch_boxes = torch.tensor(patches, dtype=torch.int32).to(device)
    table = torch.tensor(sis_hip.page_confidence_table(COLOURS), dtype=torch.uint8).to(device)

    counts = sis_hip.page_regions(x, max_regions=0, labels=False).region_count.cpu()
    capacity = int(counts.max())
    found = sis_hip.page_regions(x, max_regions=capacity)
    host_rows = found.regions.cpu().numpy()
    rows = [host_rows[k, :int(counts[k])] for k in range(CLASSES)]
    crop_rows = np.asarray([(k, *(int(v) for v in r[:5])) for k in range(CLASSES) for r in rows[k] if r[6]], dtype=np.int64)

    def render(confidence):
        return sis_hip.page_render(x, page, COLOURS, confidence_table=table if confidence else None, regions=found.regions,
                                   region_count=found.region_count, patch_boxes=patch_boxes)

    steps = {"regions": lambda: sis_hip.page_regions(x, max_regions=capacity),
             "render_plain": lambda: render(False), "render_confidence": lambda: render(True),
             "crops_bbox": lambda: sis_hip.page_crops(page, crop_rows, "bbox"),
             "crops_contour": lambda: sis_hip.page_crops(page, crop_rows, "contour", found.region_labels)}
    times = {name: [] for name in steps}
    for _ in range(ROUNDS):
        for name, fn in steps.items():
            times[name].append(event_ms(fn, args.steps, args.warmup))

    # the restatement on the host, one run each
    want, regions_ms = wall_ms(lambda: V.page_regions(pred, 0, (), 10))
    boxes = V.kept_boxes(want["rows"])
    host = {"regions": regions_ms}
    pictures = {}
    for mode, confidence in (("render_plain", False), ("render_confidence", True)):
        def draw():
            segmented = V.colour_image(pred, COLOURS, 0, confidence)
            return {"segmented": segmented, "overlay": V.overlay(segmented, scan, COLOURS[0]),
                    "boxes_on_page": host_boxes(scan, boxes, patches), "boxes_on_segmented": host_boxes(segmented, boxes, patches)}
        pictures[mode], host[mode] = wall_ms(draw)
    for mode in ("bbox", "contour"):
        _, host[f"crops_{mode}"] = wall_ms(lambda: [V.crop(scan, k, row, want["labels"], mode) for k in range(CLASSES)
                                                    for row in want["rows"][k] if row[6]])

    equal = {"region_tables": all(np.array_equal(rows[k], want["rows"][k]) for k in range(CLASSES)),
             "label_maps": bool(np.array_equal(found.region_labels.cpu().numpy(), want["labels"]))}
    for mode, confidence in (("render_plain", False), ("render_confidence", True)):
        got = render(confidence)
        equal[f"{mode}_segmented"] = bool(np.array_equal(got.segmented.cpu().numpy(), pictures[mode]["segmented"]))
        equal[f"{mode}_overlay"] = bool(np.array_equal(got.overlay.cpu().numpy(), pictures[mode]["overlay"]))
    thin = sum(1 for x0, y0, x1, y1 in boxes if x1 - x0 < 3 or y1 - y0 < 3)
    if thin == 0:   # every kept box is at least as thick as the stroke: PIL's outlines are the rule's
        got = render(False)
        equal["boxes_on_page_vs_pil"] = bool(np.array_equal(got.boxes_on_page.cpu().numpy(), pictures["render_plain"]["boxes_on_page"]))

    result = {"device": torch.cuda.get_device_name(0),
              "page": {"width": WIDTH, "height": HEIGHT, "classes": CLASSES, "patch_boxes": len(patches),
                       "regions_per_plane": [int(c) for c in counts], "kept_regions": len(crop_rows), "kept_boxes_thinner_than_stroke": thin,
                       "crop_bytes": int(sum(3 * r[4] * r[5] for r in crop_rows))},
              "device_ms": {name: {"median": round(statistics.median(v), 4), "runs": [round(t, 4) for t in v]} for name, v in times.items()},
              "host_restatement_ms": {name: round(v, 1) for name, v in host.items()},
              "host_confidence_colouring": "vectorised numpy; the reference's per-pixel Python loop is slower still",
              "equal_to_restatement": equal}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
