"""Test infrastructure shared by tests/test_page_visual_gpu.py and tests/test_page_visual_guard_bands_gpu.py: one page through
the three wrappers of csrc/page_visual.h, every result compared byte for byte with tests/page_visual_restatement.py.  ``run``
calls a wrapper (directly, or between guard bands), ``put`` places an input on the device."""
import functools

import numpy as np
import torch

import page_visual_restatement as V

COLOURS = [(0, 0, 0), (0, 0, 255), (255, 0, 0), (0, 200, 0)]
MIN_AREA = 10


@functools.lru_cache(maxsize=None)
def noise_case(seed):
    """(pred, scan, restated regions) of a noise case, computed once and shared."""
    _, shape, density = next(c for c in V.NOISE_CASES if c[0] == seed)
    pred = V.noise_page(seed, shape, density)
    scan = V.noise_scan(seed, shape[1], shape[2], 3 if seed % 2 else 1)
    want = V.page_regions(pred, 0, (), MIN_AREA)
    for arr in (pred, scan, want["labels"]):
        arr.setflags(write=False)
    return pred, scan, want


def patch_grid(height, width, device):
    """``calculate_bboxes_for_patches`` for a patch of 32 and an overlap of 8: boxes that reach past the page."""
    from segmentation.analysis_segmenter import AnalysisSegmenter
    boxes = AnalysisSegmenter(torch.nn.Identity(), 32, device, patch_overlap=8).calculate_bboxes_for_patches(width, height)
    assert any(right > width or bottom > height for _, _, right, bottom in boxes)
    return [tuple(int(v) for v in box) for box in boxes]


def assert_regions(found, want, max_regions=None):
    counts = found.region_count.cpu().numpy()
    assert np.array_equal(counts, want["region_count"]), (counts, want["region_count"])
    assert np.array_equal(found.kept_count.cpu().numpy(), want["kept_count"])
    table = found.regions.cpu().numpy()
    for k, rows in enumerate(want["rows"]):
        stored = len(rows) if max_regions is None else min(len(rows), max_regions)
        assert np.array_equal(table[k, :stored], rows[:stored]), f"class {k}"
    if found.region_labels is not None:
        assert np.array_equal(found.region_labels.cpu().numpy(), want["labels"])


def assert_render(got, want):
    for name, image in want.items():
        mine = getattr(got, name)
        assert mine is not None and mine.dtype == torch.uint8 and np.array_equal(mine.cpu().numpy(), image), name


def check_page(run, put, pred, scan, want, device, background=0, colours=None, max_regions=None):
    """Regions, the four pictures in both modes and both crop modes of one page against the restatement.  Returns the device
    regions."""
    import sis_hip
    colours = COLOURS[:pred.shape[0]] if colours is None else colours
    height, width = pred.shape[1:]
    x, page = put(torch.from_numpy(np.array(pred))), put(torch.from_numpy(np.array(scan)))
    found = run(sis_hip.page_regions, x, background, (), MIN_AREA, max_regions=max_regions)
    assert_regions(found, want, max_regions)
    rows = want["rows"] if max_regions is None else [r[:max_regions] for r in want["rows"]]
    boxes = patch_grid(height, width, device)
    patch_boxes = put(torch.tensor(boxes, dtype=torch.int32))
    table = put(torch.tensor(sis_hip.page_confidence_table(colours), dtype=torch.uint8))
    for confidence in (False, True):
        got = run(sis_hip.page_render, x, page, colours, background_class_id=background,
                  confidence_table=table if confidence else None, regions=found.regions, region_count=found.region_count,
                  patch_boxes=patch_boxes)
        assert_render(got, V.render(pred, scan, colours, background, confidence, rows, boxes))
    crop_rows = [(k, *(int(v) for v in r[:5])) for k, table_k in enumerate(rows) for r in table_k if r[6]]
    assert crop_rows
    for mode in ("bbox", "contour"):
        packed, offsets = run(sis_hip.page_crops, page, crop_rows, mode, found.region_labels)
        host = packed.cpu().numpy()
        assert len(offsets) == len(crop_rows) and host.size == sum(3 * r[4] * r[5] for r in crop_rows)
        for (k, root, x0, y0, w, h), offset in zip(crop_rows, offsets):
            piece = host[offset:offset + 3 * w * h].reshape(h, w, 3)
            assert np.array_equal(piece, V.crop(scan, k, (root, x0, y0, w, h), want["labels"], mode)), (mode, k, root)
    return found
