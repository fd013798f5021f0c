"""Host side of the scanner-margin removal: the restatement (tests/scan_margin_restatement.py) on the
constructed cases of tests/scan_margin_cases.py, ``scale_bounding_box`` against the reference's arithmetic, the two entries'
declarations and their refusals, and the tool's wiring as far as it goes without a device."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scan_margin_cases as K  # noqa: E402
import scan_margin_restatement as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = {"sis_scan_content_box_workspace_bytes", "sis_scan_content_box"}
NEW_KERNELS = {"margin_clear_kernel", "margin_front_kernel", "margin_flag_kernel", "margin_close_kernel", "margin_roots_kernel",
               "margin_boxes_kernel", "margin_areas_kernel", "margin_decide_kernel", "margin_keep_kernel", "margin_finish_kernel",
               "margin_table_kernel"}


def _tool():
    sys.path.insert(0, os.path.join(ROOT, "synthesis-in-style_amd"))
    from scripts import create_stylegan_train_dataset as tool
    return tool


# ---- the restatement on the constructions

@pytest.mark.parametrize("size,paper,box", K.SCANS + [K.TOOL_SCAN])
def test_a_scan_is_cut_to_the_paper_grown_by_one_pixel(size, paper, box):
    for seed in K.SCAN_SEEDS if size[0] * size[1] < 600000 else (0,):
        r = R.content_box(K.scan(size, paper, seed))
        assert r.box == box and r.info[3:5] == [2, 0], (seed, r.box, r.info)   # two contours kept: the paper's edge and its hole
        assert r.info[2] == r.info[5] == (box[2] - box[0]) * (box[3] - box[1])
        assert r.edges.shape == (size[1], size[0]) and set(np.unique(r.edges)) == {0, 255}


def test_whole_image_decisions():
    for image, contours, decision in ((K.small_paper(), None, 2), (K.no_margin(), None, 2), (K.uniform(), 0, 1), (K.one_contour(), 1, 1)):
        r = R.content_box(image)
        h, w = image.shape[:2]
        assert r.box == [0, 0, w, h] and r.info[4] == decision and r.info[3] == r.info[5] == 0, r.info
        assert contours is None or r.info[0] == contours
    assert R.content_box(K.small_paper()).info[0] > 1


def test_nested_squares_give_six_contours_cut_after_two():
    r = R.content_box(K.nested())
    assert r.info[:5] == [6, 3, 101 * 101, 2, 0] and r.box == [9, 9, 110, 110]
    assert r.contours[:, 0].tolist() == [0, 0, 0, 1, 1, 1]
    assert r.contours[:, 4].tolist() == [101, 61, 21, 101, 61, 21]            # an island in a hole is a contour of its own
    assert all(np.all(np.diff(r.contours[r.contours[:, 0] == k, 1]) > 0) for k in (0, 1))   # ascending roots within a kind


def test_equal_areas():
    r = R.content_box(K.two_squares())
    assert r.info[:5] == [4, 2, 49, 0, 2] and (r.contours[:, 4] * r.contours[:, 5]).tolist() == [49] * 4
    r = R.content_box(K.two_squares(**K.TWO_SQUARES_GROWN))   # decision 0 with ONE area: only the first contour is kept
    areas = (r.contours[:, 4] * r.contours[:, 5]).tolist()
    assert r.info[0] == 2 and len(set(areas)) == 1 and r.info[3:6] == [1, 0, areas[0]]
    assert r.box == [r.contours[0, 2], r.contours[0, 3], r.contours[0, 2] + r.contours[0, 4], r.contours[0, 3] + r.contours[0, 5]]


def test_the_cut_takes_the_first_of_equal_gaps():
    def c(area, root):
        return R.Contour(0, root, root, 0, area, 1)
    found = [c(100, 0), c(90, 200), c(80, 400), c(80, 600), c(70, 800)]   # gaps 10, 10, 0, 10: the one at the top wins
    box, kept, decision, threshold, largest = R.decide(found, 10, 16)     # 96 > largest is false: decision 0
    assert (kept, decision, threshold, largest) == (1, 0, 100, 100) and box == [0, 0, 100, 1]
    found = [c(100, 0), c(95, 200), c(60, 400), c(60, 600)]
    assert R.decide(found, 10, 16)[1:4] == (2, 0, 95)


def test_a_weak_edge_hangs_on_its_strong_end_across_tiles():
    def lines(image, axis):
        return int((R.content_box(image).edges.max(axis=axis) > 0).sum())
    assert lines(K.chain(), 0) == 160 and lines(K.chain(ramp=False), 0) == 0
    assert lines(K.chain(transpose=True), 1) == 160 and lines(K.chain(ramp=False, transpose=True), 1) == 0
    assert lines(K.diagonal_chain(), 0) == 99 and lines(K.diagonal_chain(ramp=False), 0) == 0


def test_the_strongest_channel_decides():
    both = R.content_box(K.channel_step(True)), R.content_box(K.channel_step(False))
    assert both[0].info[6] > 0 and np.array_equal(both[0].edges, both[1].edges) and both[0].info == both[1].info


def test_random_bytes_give_dense_contours_and_ties():
    for size in K.RANDOM_SIZES[1:]:
        r = R.content_box(K.random_bytes(size))
        areas = (r.contours[:, 4] * r.contours[:, 5]).tolist()
        assert r.info[0] >= 10 and len(set(areas)) < len(areas)
    assert R.content_box(K.random_bytes((3, 3))).info[0] <= 1


def test_blur_rounds_to_nearest_and_mirrors_without_the_edge():
    a = np.zeros((3, 4, 3), dtype=np.uint8)
    a[0, 0] = 90
    b = R.blur(a)
    assert b[0, 0, 0] == 10 and b[1, 1, 0] == 10 and b[0, 2, 0] == 0   # (90 + 4) // 9; the corner is counted once
    a[:] = 0
    a[1, 1] = 9
    assert R.blur(a)[0, 0, 0] == 4                                      # mirrored: (1, 1) is seen four times from the corner


# ---- step 8

def test_scale_bounding_box_is_the_references_arithmetic():
    from utils.scan_patches import ANALYSIS_SIZE, scale_bounding_box
    assert ANALYSIS_SIZE == 1000
    assert scale_bounding_box([10, 20, 90, 180], (100, 200), (1000, 2000)) == [100, 200, 900, 1800]
    # 2480 x 3508 analysed at 707 x 1000: factors 3.5077793493635077 and 3.508
    assert scale_bounding_box([59, 39, 651, 971], (707, 1000), (2480, 3508)) == [206, 136, 2283, 3406]
    assert scale_bounding_box([1, 1, 3, 3], (3, 3), (10, 10)) == [3, 3, 10, 10]   # 3.33..: truncated, not rounded
    assert scale_bounding_box([0, 0, 707, 1000], (707, 1000), (2480, 3508)) == [0, 0, 2480, 3508]
    for box, small, large in (([59, 39, 651, 971], (707, 1000), (2480, 3508)), ([7, 9, 640, 333], (1000, 707), (3000, 2121))):
        assert scale_bounding_box(box, small, large) == R.scale_bounding_box(box, small, large)


# ---- the entries

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
        assert re.search(r"%s \(scripts/create_stylegan_train_dataset\.py:\d+" % name, text), name   # the reference lines it replaces
    assert NEW_KERNELS <= sis_hip.own_kernel_names()
    for wrapper in ("scan_content_box", "scan_remove_margin"):
        assert callable(getattr(sis_hip, wrapper))


def test_workspace_bytes_are_zero_outside_the_limits():
    import sis_hip
    L = sis_hip.lib()
    assert L.sis_scan_content_box_workspace_bytes(3, 3) > 0 and L.sis_scan_content_box_workspace_bytes(4096, 4096) > 0
    for h, w in ((2, 100), (100, 2), (4097, 100), (100, 4097), (0, 0), (-5, 100)):
        assert L.sis_scan_content_box_workspace_bytes(h, w) == 0, (h, w)
    small, large = L.sis_scan_content_box_workspace_bytes(100, 100), L.sis_scan_content_box_workspace_bytes(200, 100)
    assert large > small and small % 4 == 0


def test_entry_declines_bad_arguments_before_any_launch():
    import sis_hip
    L = sis_hip.lib()
    p = ctypes.c_void_p(4096)   # never dereferenced: every case returns at its check
    odd = ctypes.c_void_p(4098)
    ws = L.sis_scan_content_box_workspace_bytes(100, 120)

    def call(box=p, info=p, edges=p, contours=p, max_contours=4, page=p, h=100, w=120, low=20, high=150, workspace=p, workspace_bytes=ws):
        return L.sis_scan_content_box(box, info, edges, contours, max_contours, page, h, w, low, high, workspace, workspace_bytes, None)

    for kw, text in [(dict(box=None), "null"), (dict(info=None), "null"), (dict(page=None), "null"), (dict(workspace=None), "null"),
                     (dict(box=odd), "aligned"), (dict(info=odd), "aligned"), (dict(contours=odd), "aligned"),
                     (dict(workspace=odd), "aligned"), (dict(workspace_bytes=ws - 1), "workspace of"), (dict(h=2), "outside 3..4096"),
                     (dict(w=4097), "outside 3..4096"), (dict(low=-1), "low -1"), (dict(low=30, high=29), "high 29"),
                     (dict(max_contours=-1), "max_contours -1")]:
        assert call(**kw) != 0 and text in L.sis_last_error().decode(), (kw, L.sis_last_error().decode())


# ---- the tool

def test_margin_remove_on_the_device_path_reaches_device_selection(tmp_path, monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)   # where a device is present, tests/test_scan_margin_gpu.py runs the tool
    tool = _tool()
    args = tool.build_parser().parse_args([str(tmp_path), str(tmp_path / "out"), "5", "--margin-remove", "--pixel-path", "device"])
    assert tool.resolve_paths(args) == ("device", "device")
    with pytest.raises(RuntimeError, match="no HIP device"):
        tool.main(args)
    args = tool.build_parser().parse_args([str(tmp_path), str(tmp_path / "out"), "5", "--margin-remove", "--pixel-path", "pil"])
    with pytest.raises(NotImplementedError):
        tool.resolve_paths(args)
    assert "device" in [a for a in tool.build_parser()._actions if a.dest == "margin_remove"][0].help
