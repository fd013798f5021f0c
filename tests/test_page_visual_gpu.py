"""GPU parity of the page visualisation (csrc/page_visual.h) against the independent restatement
(tests/page_visual_restatement.py: numpy + scipy.ndimage) and the reference-made golden colouring
(tests/golden/page_visual.npz).  Every comparison is of integers or bytes and exact."""
import argparse
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import page_visual_checks as C  # noqa: E402
import page_visual_restatement as V  # noqa: E402

pytestmark = pytest.mark.gpu


def _direct(fn, *args, **kwargs):
    return fn(*args, **kwargs)


def _put(device):
    return lambda t: t.to(device)


@pytest.mark.parametrize("seed", [c[0] for c in V.NOISE_CASES])
def test_noise_pages(device, seed):
    pred, scan, want = C.noise_case(seed)
    for k in range(1, pred.shape[0]):   # no case passes on empty tables
        assert want["kept_count"][k] >= 2 and want["region_count"][k] - want["kept_count"][k] >= 1
    C.check_page(_direct, _put(device), pred, scan, want, device)


@pytest.mark.parametrize("channels", [1, 3])
def test_hand_made_page(device, channels):
    pred = V.hand_made_page()
    want = V.page_regions(pred, 0, (), C.MIN_AREA)
    assert want["region_count"].tolist() == [0, 6] and want["kept_count"].tolist() == [0, 4]
    found = C.check_page(_direct, _put(device), pred, V.noise_scan(9, 45, 70, channels), want, device)
    areas = found.regions[1, :6, 5].cpu().tolist()
    assert sorted(areas)[:2] == [0, 0] and 20 in areas   # the single pixel, the line, the 2 x 11 bar


@pytest.mark.parametrize("case", [0, 1])
def test_colouring_equals_the_reference_bytes(device, golden_dir, case):
    import sis_hip
    from PIL import ImageColor
    golden = np.load(os.path.join(golden_dir, "page_visual.npz"))
    colours = [ImageColor.getrgb(c) for c in json.loads(str(golden["class_maps_json"]))[case].values()]
    pred = torch.from_numpy(golden[f"input_{case}"][0]).to(device)
    table = torch.tensor(sis_hip.page_confidence_table(colours), dtype=torch.uint8).to(device)
    plain = sis_hip.page_render(pred, None, colours, outputs=("segmented",))
    assert plain.overlay is None and plain.boxes_on_page is None and plain.boxes_on_segmented is None
    assert np.array_equal(plain.segmented.cpu().numpy(), golden[f"plain_{case}"])
    shaded = sis_hip.page_render(pred, None, colours, confidence_table=table, outputs=("segmented",))
    assert np.array_equal(shaded.segmented.cpu().numpy(), golden[f"confidence_{case}"])


def test_filter_classes_and_another_background(device):
    import sis_hip
    pred, scan, _ = C.noise_case(5)   # four classes
    x = torch.from_numpy(np.array(pred)).to(device)
    want = V.page_regions(pred, 2, (1,), C.MIN_AREA)
    assert want["region_count"][1] == 0 and want["region_count"][2] == 0 and want["region_count"][0] > 0 and want["region_count"][3] > 0
    found = sis_hip.page_regions(x, 2, (1,), C.MIN_AREA)
    C.assert_regions(found, want)
    assert not found.region_labels[1].any() and not found.region_labels[2].any()
    colours = [(10, 20, 30), (0, 0, 255), (250, 250, 250), (0, 200, 0)]
    page = torch.from_numpy(np.array(scan)).to(device)
    table = torch.tensor(sis_hip.page_confidence_table(colours), dtype=torch.uint8).to(device)
    for confidence in (False, True):
        got = sis_hip.page_render(x, page, colours, background_class_id=2, confidence_table=table if confidence else None,
                                  regions=found.regions, region_count=found.region_count)
        C.assert_render(got, V.render(pred, scan, colours, 2, confidence, want["rows"]))
    other = V.page_regions(pred, 0, (), 3)   # another minimum area moves rows between kept and dropped
    C.assert_regions(sis_hip.page_regions(x, 0, (), 3), other)
    assert not np.array_equal(other["kept_count"], V.page_regions(pred, 0, (), C.MIN_AREA)["kept_count"])


def test_truncating_capacity_keeps_the_true_counts(device):
    pred, scan, want = C.noise_case(1)
    assert want["region_count"][1:].min() > 3
    found = C.check_page(_direct, _put(device), pred, scan, want, device, max_regions=3)
    assert tuple(found.regions.shape) == (3, 3, 8)
    import sis_hip
    counts_only = sis_hip.page_regions(torch.from_numpy(np.array(pred)).to(device), max_regions=0, labels=False)
    assert counts_only.regions is None and counts_only.region_labels is None
    assert np.array_equal(counts_only.region_count.cpu().numpy(), want["region_count"])
    assert np.array_equal(counts_only.kept_count.cpu().numpy(), want["kept_count"])


def test_two_runs_are_byte_identical(device):
    import sis_hip
    pred, scan, want = C.noise_case(2)
    x, page = torch.from_numpy(np.array(pred)).to(device), torch.from_numpy(np.array(scan)).to(device)
    runs = []
    for _ in range(2):
        found = sis_hip.page_regions(x, max_regions=int(want["region_count"].max()))
        drawn = sis_hip.page_render(x, page, C.COLOURS[:3], regions=found.regions, region_count=found.region_count)
        stored = [found.regions[k, :int(want["region_count"][k])] for k in (1, 2)]   # rows past a plane's count are not written
        runs.append([*stored, found.region_count, found.kept_count, found.region_labels, *drawn])
    for a, b in zip(*runs):
        assert a.data_ptr() != b.data_ptr() and torch.equal(a, b)


def test_regions_and_render_inside_a_graph(device):
    import sis_hip
    pred, scan, want = C.noise_case(1)
    other = V.noise_page(11, pred.shape, 0.15)
    static = torch.from_numpy(np.array(pred)).to(device)
    page = torch.from_numpy(np.array(scan)).to(device)
    colours = C.COLOURS[:3]
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):   # warm-up outside the capture
        sis_hip.page_regions(static)
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        found = sis_hip.page_regions(static)
        drawn = sis_hip.page_render(static, page, colours, regions=found.regions, region_count=found.region_count)
    for source, expected in ((pred, want), (other, V.page_regions(other, 0, (), C.MIN_AREA))):
        static.copy_(torch.from_numpy(np.array(source)))
        graph.replay()
        torch.cuda.synchronize()
        C.assert_regions(found, expected)
        C.assert_render(drawn, V.render(source, scan, colours, 0, False, expected["rows"]))


class _NoiseNetwork(torch.nn.Module):
    """Stands in for a trained segmenter: ``predict`` returns thresholded smooth noise, patch after patch."""
    num_input_channels = 3

    def __init__(self, classes, seed):
        super().__init__()
        self.classes, self.rng = classes, np.random.RandomState(seed)
        self.min_confidence, self.min_contour_area = 0.7, 0

    def predict(self, images):
        b, _, p, _ = images.shape
        noise = V.E.threshold(V.E.smooth_noise_planes(self.rng, (b, self.classes, p, p), 0.15), 0.7)
        return torch.from_numpy(noise).to(images.device)


@pytest.mark.parametrize("show_confidence", [False, True])
def test_visualize_segmentation_end_to_end(device, tmp_path, show_confidence):
    from PIL import Image
    from segmentation.analysis_segmenter import AnalysisSegmenter
    from segmentation.evaluation.segmentation_visualization import get_bounding_boxes, visualize_segmentation
    class_map = {"background": "#000000", "printed_text": "#0000FF", "handwritten_text": "#FF0000"}
    colours = [(0, 0, 0), (0, 0, 255), (255, 0, 0)]
    segmenter = AnalysisSegmenter(_NoiseNetwork(3, 17), 64, device, batch_size=4, patch_overlap=8, class_to_color_map=class_map,
                                  show_confidence_in_segmentation=show_confidence)
    scan = V.noise_scan(17, 300, 200, 3)   # 200 wide, 300 high
    image = Image.fromarray(scan)
    assembled = segmenter.segment_image(image)
    assert tuple(assembled.shape) == (3, 300, 200)
    args = argparse.Namespace(output_dir=tmp_path, overlay_segmentation=True, extract_bboxes=True, draw_patches=True,
                              draw_bboxes_on_segmentation=True, save_bboxes=True, save_contours=True)
    visualize_segmentation(assembled, image, image, segmenter, args, class_map, "page_a")

    pred = assembled.cpu().numpy()
    want = V.page_regions(pred, 0, (), 10)
    assert all(want["kept_count"][k] >= 2 for k in (1, 2))
    patches = [tuple(box) for box in segmenter.calculate_bboxes_for_patches(200, 300)]
    pictures = V.render(pred, scan, colours, 0, show_confidence, want["rows"], patches)
    files = {"page_a_segmented_no_bboxes.png": pictures["segmented"], "page_a_overlayed.png": pictures["overlay"],
             "page_a_bboxes.png": pictures["boxes_on_page"], "page_a_segmented.png": pictures["boxes_on_segmented"]}
    for k in (1, 2):
        kept = [r for r in want["rows"][k] if r[6]]
        for i, row in enumerate(kept):
            files[f"bboxes/page_a_class_{k}_bbox_{i}.png"] = V.crop(scan, k, row, want["labels"], "bbox")
            files[f"contours/page_a_class_{k}_contour_{i}.png"] = V.crop(scan, k, row, want["labels"], "contour")
    root = tmp_path / "images"
    written = {str(p.relative_to(root)) for p in root.rglob("*") if p.is_file()}
    assert written == set(files)
    for name, expected in files.items():
        with Image.open(root / name) as picture:
            assert picture.mode == "RGB" and np.array_equal(np.array(picture), expected), name
    boxes = get_bounding_boxes(assembled)
    assert sorted(boxes) == [1, 2]
    for k in (1, 2):
        assert [tuple(b) for b in boxes[k]] == [(int(r[1]), int(r[2]), int(r[1] + r[3]), int(r[2] + r[4])) for r in want["rows"][k] if r[6]]
    assert np.array_equal(np.array(segmenter.prediction_to_color_image(assembled)), pictures["segmented"])
