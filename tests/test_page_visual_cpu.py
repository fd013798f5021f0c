"""The page visualisation without a device: the restatement's colouring against the reference's golden bytes, the gradient table
against ``linear_gradient``'s formula entry for entry, the outline rule against PIL's ``ImageDraw.rectangle``, the hand-made
regions, the C ABI's declarations and argument checks, the new command's flags and ``BBox``."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import page_visual_restatement as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = {"sis_page_regions_workspace_bytes", "sis_page_regions", "sis_page_render", "sis_page_crops"}
NEW_KERNELS = {"pv_rank_kernel", "pv_box_kernel", "pv_finish_kernel", "pv_colour_kernel", "pv_region_boxes_kernel",
               "pv_patch_boxes_kernel", "pv_crops_kernel"}


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "page_visual.npz"))


# ---- colouring -----------------------------------------------------------------------------------------------------------------------
def _colours(class_map):
    from PIL import ImageColor
    return [ImageColor.getrgb(c) for c in class_map.values()]


@pytest.mark.parametrize("case", [0, 1])
@pytest.mark.parametrize("mode", ["plain", "confidence"])
def test_restatement_colouring_equals_the_reference(golden, case, mode):
    class_map = json.loads(str(golden["class_maps_json"]))[case]
    assert list(class_map)[0] == "background"
    pred = golden[f"input_{case}"][0]
    want = golden[f"{mode}_{case}"]
    got = V.colour_image(pred, _colours(class_map), 0, confidence=mode == "confidence")
    assert got.dtype == np.uint8 and np.array_equal(got, want)


def test_golden_inputs_hold_the_edge_cases(golden):
    for case in (0, 1):
        pred = golden[f"input_{case}"][0]
        top = pred.max(axis=0)
        assert ((pred == top).sum(axis=0) >= 2)[top > 0].sum() >= 5          # ties between classes, above zero
        assert (top == 0).sum() >= 20                                        # all-zero pixels
        assert ((top > 0) & (top < 0.01)).sum() >= 2 and (top == 1.0).sum() >= 2
        assert ((pred.argmax(axis=0) == 0) & (pred[1:].sum(axis=0) > 0)).sum() >= 1   # the background wins, the others vote
        assert not np.array_equal(golden[f"plain_{case}"], golden[f"confidence_{case}"])


def test_gradient_table_equals_linear_gradient():
    import sis_hip
    colours = [(0, 0, 0), (0, 0, 255), (255, 0, 0), (16, 16, 16), (0, 200, 0), (255, 128, 0), (127, 0, 255), (255, 255, 255), (1, 2, 3)]

    def linear_gradient(start_rgb, finish_rgb, n=10):   # the formula of the reference's visualization/utils.py:9-26
        out = [start_rgb]
        for t in range(1, n):
            out.append(tuple(int(start_rgb[j] + (float(t) / (n - 1)) * (finish_rgb[j] - start_rgb[j])) for j in range(3)))
        return out

    want = [linear_gradient((255, 255, 255), c, 100) for c in colours]
    table = sis_hip.page_confidence_table(colours)
    restated = V.gradient_table(colours)
    assert restated.shape == (len(colours), 100, 3)
    for k in range(len(colours)):
        for t in range(100):
            assert tuple(table[k][t]) == tuple(restated[k, t]) == tuple(want[k][t]), (k, t)
        assert tuple(table[k][0]) == (255, 255, 255) and tuple(table[k][99]) == colours[k]


# ---- outlines --------------------------------------------------------------------------------------------------------------------------
def _pil_outline(height, width, box, colour, stroke):
    from PIL import Image, ImageDraw
    image = Image.new("RGB", (width, height), (9, 9, 9))
    ImageDraw.Draw(image).rectangle(tuple(int(v) for v in box), outline=colour, width=stroke)
    return np.array(image)


@pytest.mark.parametrize("stroke,colour", [(1, V.RED), (3, V.GREEN)])
def test_outline_rule_equals_pil_on_boxes_of_at_least_the_stroke(stroke, colour):
    rng = np.random.RandomState(7 + stroke)
    height, width = 37, 53
    outside = 0
    for _ in range(1500):
        x0, y0 = int(rng.randint(-12, width + 4)), int(rng.randint(-12, height + 4))
        x1, y1 = x0 + int(rng.randint(stroke, 40)), y0 + int(rng.randint(stroke, 40))
        got = np.full((height, width, 3), 9, np.uint8)
        V.outline(got, (x0, y0, x1, y1), colour, stroke)
        assert np.array_equal(got, _pil_outline(height, width, (x0, y0, x1, y1), colour, stroke)), (x0, y0, x1, y1)
        outside += x0 < 0 or y0 < 0 or x1 >= width or y1 >= height
    assert outside > 300   # boxes partly (or wholly) outside the image


def test_thin_boxes_are_filled_where_pil_paints_outside():
    """The documented difference: a box thinner than the stroke is filled by the rule and nothing else is painted; PIL's
    outline of such a box leaves it."""
    height, width, stroke = 30, 30, 3
    bled = 0
    for w, h in [(0, 0), (1, 7), (7, 1), (0, 9), (2, 2), (1, 1), (11, 1), (2, 11)]:
        x0, y0 = 10, 12
        got = np.full((height, width, 3), 9, np.uint8)
        V.outline(got, (x0, y0, x0 + w, y0 + h), V.GREEN, stroke)
        painted = (got != 9).any(axis=2)
        want = np.zeros((height, width), bool)
        want[y0:y0 + h + 1, x0:x0 + w + 1] = True
        assert np.array_equal(painted, want), (w, h)
        pil = (_pil_outline(height, width, (x0, y0, x0 + w, y0 + h), V.GREEN, stroke) != 9).any(axis=2)
        bled += bool((pil & ~want).any())
    assert bled >= 1


# ---- regions -----------------------------------------------------------------------------------------------------------------------------
def test_hand_made_page():
    pred = V.hand_made_page()
    assert pred.shape == (2, 45, 70)
    found = V.page_regions(pred, 0, (), 10)
    rows = found["rows"][1]
    assert found["region_count"].tolist() == [0, 6] and found["kept_count"].tolist() == [0, 4] and len(found["rows"][0]) == 0
    by_root = {int(r[0]): [int(v) for v in r] for r in rows}
    assert [r[0] for r in rows.tolist()] == sorted(by_root)                       # ascending root order
    assert by_root[0][1:7] == [0, 0, 7, 9, 2 * 28 + 1, 1]                         # the edge shape, in the plane's corner
    assert by_root[5 * 70 + 40][1:] == [40, 5, 1, 1, 0, 0, 0]                     # a single pixel
    assert by_root[8 * 70 + 22][1:] == [22, 8, 9, 1, 0, 0, 0]                     # a one-pixel line: area 0
    assert by_root[14 * 70 + 18][1:] == [18, 14, 11, 2, 20, 1, 0]                 # the 2 x 11 bar: twice_area exactly 20
    ring = by_root[27 * 70 + 22]
    assert ring[1:5] == [22, 27, 12, 12] and ring[5] == 2 * 11 * 11 and ring[6] == 1   # hole and island filled
    spanning = by_root[18 * 70 + 48]
    assert spanning[1:5] == [48, 18, 19, 24] and spanning[1] < 64 <= spanning[1] + spanning[3] and spanning[2] < 32 <= spanning[2] + spanning[4]
    labels = found["labels"]
    assert not labels[0].any() and labels[1][30, 27] == 27 * 70 + 22 + 1 and labels[1][44, 69] == 0
    assert sorted(set(labels[1].ravel().tolist())) == [0] + [r + 1 for r in sorted(by_root)]
    # a filtered class and another background: the skipped planes swap
    other = V.page_regions(pred, 1, (), 10)
    assert other["region_count"][1] == 0 and other["region_count"][0] >= 1
    assert V.page_regions(pred, 0, (1,), 10)["region_count"].tolist() == [0, 0]


def test_noise_cases_have_kept_and_dropped_regions():
    for seed, shape, density in V.NOISE_CASES:
        found = V.page_regions(V.noise_page(seed, shape, density), 0, (), 10)
        for k in range(1, shape[0]):
            count, kept = int(found["region_count"][k]), int(found["kept_count"][k])
            assert 5 <= count <= 145 and 2 <= kept <= 67 and 1 <= count - kept <= 78, (seed, k, count, kept)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_header_ctypes_table_and_library_agree():
    import sis_hip
    text = open(os.path.join(ROOT, "include", "sis_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert NEW_SYMBOLS <= set(re.findall(r"\b(sis_[a-z0-9_]+)\s*\(", header)) and NEW_SYMBOLS <= set(sis_hip.exported_symbols())
    L = sis_hip.lib()
    for name in NEW_SYMBOLS:
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, header).group(1)
        assert decl.count(",") + 1 == len(sis_hip._SIGNATURES[name][0]), name
        assert hasattr(L, name)
        assert re.search(r"%s \((segmentation_utils|segmentation_visualization|visualization/utils)\.py:\d+-\d+" % name, text), name
    assert "NOT pinned against OpenCV's\n * findContours / boundingRect / drawContours" in text
    assert NEW_KERNELS <= sis_hip.own_kernel_names()
    csrc = os.path.join(ROOT, "synthesis-in-style_amd", "csrc")
    assert "page_visual.hip" not in os.listdir(csrc) and '#include "page_visual.h"' in open(os.path.join(csrc, "contour_ops.hip")).read()
    assert sis_hip.PAGE_MAX_EDGE == 8192 and sis_hip.PAGE_MAX_CLASSES == 16


def test_entries_decline_bad_arguments_before_any_launch():
    import sis_hip
    L = sis_hip.lib()
    ptr = ctypes.c_void_p(4096)   # never dereferenced: every case returns at its check
    colours = (ctypes.c_uint8 * 48)()
    assert L.sis_page_regions_workspace_bytes(3, 33, 70) == 9 * 3 * 33 * 70
    assert L.sis_page_regions_workspace_bytes(16, 8192, 8192) == 9 * 16 * 8192 * 8192
    bad_shapes = [(1, 33, 70), (17, 33, 70), (3, 0, 70), (3, 33, 0), (3, 8193, 70), (3, 33, 8193), (3, -1, 70)]
    assert [L.sis_page_regions_workspace_bytes(*a) for a in bad_shapes] == [0] * len(bad_shapes)
    ws = L.sis_page_regions_workspace_bytes(3, 33, 70)

    def regions(regions=ptr, counts=ptr, kept=ptr, pred=ptr, classes=3, height=33, width=70, background=0, filter_classes=0,
                min_area=10, max_regions=8, workspace=ptr, workspace_bytes=ws):
        return L.sis_page_regions(regions, counts, kept, None, pred, classes, height, width, background, filter_classes, min_area,
                                  max_regions, workspace, workspace_bytes, None)

    def render(segmented=ptr, overlay=ptr, pred=ptr, page=ptr, channels=3, colours=colours, regions=ptr, counts=ptr, max_regions=8,
               patch_boxes=ptr, patches=2, classes=3, height=33, width=70, background=0):
        return L.sis_page_render(segmented, overlay, None, None, pred, page, channels, colours, None, regions, counts, max_regions,
                                 patch_boxes, patches, classes, height, width, background, None)

    def crops(out=ptr, out_bytes=64, table=ptr, rows=1, page=ptr, channels=3, labels=ptr, classes=3, height=33, width=70, mode=1):
        return L.sis_page_crops(out, out_bytes, table, rows, page, channels, labels, classes, height, width, mode, None)

    shape_cases = [(dict(classes=1), "classes 1"), (dict(classes=17), "classes 17"), (dict(height=0), "page 0 x 70"),
                   (dict(width=0), "page 33 x 0"), (dict(height=8193), "page 8193 x 70"), (dict(width=8193), "page 33 x 8193")]
    cases = [(regions, kw, text) for kw, text in shape_cases] + [(render, kw, text) for kw, text in shape_cases] \
        + [(crops, kw, text) for kw, text in shape_cases]
    cases += [(regions, kw, text) for kw, text in [
        (dict(counts=None), "null"), (dict(kept=None), "null"), (dict(pred=None), "null"), (dict(workspace=None), "null"),
        (dict(background=-1), "background class -1"), (dict(background=3), "background class 3"), (dict(filter_classes=8), "filter_classes"),
        (dict(min_area=-1), "min_contour_area"), (dict(max_regions=-1), "max_regions"), (dict(regions=None), "max_regions without"),
        (dict(max_regions=1 << 27), "max_regions"), (dict(workspace_bytes=ws - 1), "workspace too small"),
        (dict(workspace=ctypes.c_void_p(4098)), "aligned")]]
    cases += [(render, kw, text) for kw, text in [
        (dict(pred=None), "null"), (dict(colours=None), "null"), (dict(segmented=None, overlay=None), "no output"),
        (dict(page=None), "null page"), (dict(channels=2), "2 channels"), (dict(background=3), "background class 3"),
        (dict(max_regions=-1), "max_regions"), (dict(regions=None), "without tables"), (dict(counts=None), "without tables"),
        (dict(patches=-1), "negative"), (dict(patch_boxes=None), "patch boxes missing")]]
    cases += [(crops, kw, text) for kw, text in [
        (dict(out=None), "null"), (dict(table=None), "null"), (dict(page=None), "null"), (dict(mode=2), "mode 2"),
        (dict(labels=None), "without region labels"), (dict(channels=4), "4 channels"), (dict(rows=0), "non-positive"),
        (dict(out_bytes=0), "non-positive")]]
    for call, kw, text in cases:
        assert call(**kw) != 0, (call.__name__, kw)
        assert text in L.sis_last_error().decode(), (call.__name__, kw, L.sis_last_error().decode())


def test_wrappers_decline_host_tensors_and_bad_shapes():
    import torch
    import sis_hip
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        sis_hip.page_regions(torch.zeros(3, 8, 8))
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        sis_hip.page_render(torch.zeros(3, 8, 8), None, [(0, 0, 0)] * 3, outputs=("segmented",))
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        sis_hip.page_crops(torch.zeros(8, 8, 3, dtype=torch.uint8), [(1, 0, 0, 0, 2, 2)], "bbox")
    with pytest.raises(RuntimeError, match="mode"):
        sis_hip.page_crops(torch.zeros(8, 8, 3, dtype=torch.uint8), [], "polygon")
    assert sis_hip.page_regions_capacity(33, 70) == 17 * 35


# ---- the Python surface -------------------------------------------------------------------------------------------------------------------
def test_command_parses_the_reference_flags():
    from segmentation.evaluation import segmentation_visualization as S
    args = S.parse_and_check_arguments(
        ["pages", "-f", "cfg.json", "-op", "train.yaml", "-o", "out", "--resize", "-1", "800", "-bw", "--absolute-patch-overlap", "8", "16",
         "--min-confidence", "0.5", "0.7", "--min-contour-area", "30", "-vis", "--overlay-segmentation", "--extract-bboxes",
         "--draw-patches", "--draw-bboxes-on-segmentation", "--save-bboxes", "--save-contours", "--show-confidence"])
    assert args.visualize_segmentation and args.overlay_segmentation and args.extract_bboxes and args.draw_patches
    assert args.draw_bboxes_on_segmentation and args.save_bboxes and args.save_contours and args.show_confidence
    assert str(args.image_dir) == "pages" and str(args.config_file) == "cfg.json" and str(args.output_dir) == "out"
    assert args.resize == [-1, 800] and args.convert_to_black_white and args.absolute_patch_overlap == [8, 16]
    assert args.min_confidence == [0.5, 0.7] and args.min_contour_area == [30]
    plain = S.parse_and_check_arguments(["pages"])   # -vis is implied, nothing else is
    assert plain.visualize_segmentation and not plain.extract_bboxes and not plain.show_confidence
    from segmentation.evaluation.analyze_image_segments import create_hyperparam_configs
    names = [S.get_string_representation_of_config(c) for c in create_hyperparam_configs(args)]
    assert len(names) == 4 and names[0] == "min_confidence_0_5_min_contour_area_30_patch_overlap_8__0_0"
    for name in ("get_bounding_boxes", "draw_segmentation", "save_overlayed_segmentation_image", "extract_and_save_bounding_boxes",
                 "extract_and_save_contours", "visualize_segmentation"):
        assert callable(getattr(S, name)), name
    assert "OpenCV's contour order" in S.__doc__ and "thinner than the stroke" in S.__doc__


def test_bbox_behaves_as_the_reference():
    from utils.segmentation_utils import BBox
    box = BBox.from_opencv_bounding_rect(3, 4, 10, 20)
    assert box == (3, 4, 13, 24) and isinstance(box, tuple) and box._fields == ("left", "top", "right", "bottom")
    assert (box.left, box.top, box.right, box.bottom, box.width, box.height) == (3, 4, 13, 24, 10, 20)
    assert box.top_left() == (3, 4) and box.bottom_right() == (13, 24)
    assert box.as_points() == ((3, 4), (13, 4), (13, 24), (3, 24))
    assert box.is_overlapping_with(BBox(12, 23, 30, 30)) and not box.is_overlapping_with(BBox(13, 4, 20, 24))
    assert box.get_mutual_bbox(BBox(0, 10, 5, 40)) == BBox(0, 4, 13, 40)
    left, top, right, bottom = box   # the tuple alias of analysis_segmenter.py: four integers
    assert (left, top, right, bottom) == (3, 4, 13, 24)
    from segmentation.analysis_segmenter import AnalysisSegmenter
    import inspect
    params = list(inspect.signature(AnalysisSegmenter.__init__).parameters)
    assert params[-2:] == ["class_to_color_map", "show_confidence_in_segmentation"] and hasattr(AnalysisSegmenter, "prediction_to_color_image")
