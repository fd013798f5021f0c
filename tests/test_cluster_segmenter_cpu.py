"""CPU part of the cluster-based labeller's tests:

* the definition (restatement 1) against the reference's pairwise merging on pixel sets (restatement 2) on seeded random
  images: the share of differing images is printed and capped, and every differing image contains a gap that borders two or
  more groups (difference (a));
* hand-made cases with the outcome asserted directly;
* host logic: label-map inversion, the sanity assertion, a missing ``printed_text``, a resolution above the image size, CPU
  tensors, header / ctypes table, and that the product modules import neither scipy nor cv2.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cluster_segmenter_restatement as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "synthesis-in-style_amd")
MODULES = ("segmentation/base_cluster_based_dataset_segmenter.py",
           "segmentation/black_white_handwritten_printed_text_segmenter.py", "segmentation/base_dataset_segmenter.py",
           "segmentation/gan_local_edit/factor_catalog.py", "utils/dataset_creation.py", "create_dataset_for_segmentation.py")
MAX_DIFFERING_SHARE = 0.05
PRINTED, HANDWRITTEN = 1, 2   # class ids of the default colour-map order


# ---- restatement 1 against restatement 2 ---------------------------------------------------------------------------------------
def test_group_merging_against_pairwise_merging():
    rng = np.random.RandomState(20261017)
    images, differing, differing_without_shared_gap = 0, 0, 0
    for keys in (2, 3):
        for n in range(160):
            regions_per_key = []
            for k in range(keys):
                r = (16, 32, 64)[(n + k) % 3]
                mask = R.enlarge(R.smooth_mask(rng, r, coverage=0.15 + 0.10 * rng.rand()), 64)
                regions_per_key.append(R.plane_regions(mask))
            ours, shared_gaps = R.merge(regions_per_key, False)
            theirs = R.merge_pairwise(regions_per_key, False)
            images += 1
            if not R.same_groups(ours, theirs):
                differing += 1
                differing_without_shared_gap += shared_gaps == 0
            else:   # then the overlapping-only selection agrees too
                assert R.same_groups(R.merge(regions_per_key, True)[0], R.merge_pairwise(regions_per_key, True))
    share = differing / images
    print(f"group merging vs pairwise merging: {differing} of {images} images differ ({100 * share:.2f} %), "
          f"{differing_without_shared_gap} of them without a gap that borders two or more groups")
    assert images >= 300
    assert differing_without_shared_gap == 0
    assert share <= MAX_DIFFERING_SHARE


# ---- hand-made cases -----------------------------------------------------------------------------------------------------------
def test_ring_with_blob_in_its_hole_is_one_filled_group():
    s = R.shapes()
    groups, shared = R.merge([R.plane_regions(s["ring"]), R.plane_regions(s["blob"])], True)
    assert len(groups) == 1 and groups[0][1] == 2 and shared == 0
    assert np.array_equal(groups[0][0], R.plane_regions(R.box(10, 40, 10, 40))[0])   # the dilated square, hole filled
    assert R.same_groups(groups, R.merge_pairwise([R.plane_regions(s["ring"]), R.plane_regions(s["blob"])], True))
    class_map, _, drop = R.segment(*R.hand_made_cases()["ring_and_blob"])
    assert np.array_equal(class_map[0] == PRINTED, s["in_hole"]) and not drop[0]


def test_c_closed_by_a_touching_piece_stays_two_groups():
    s = R.shapes()
    c, bar = R.plane_regions(s["c_shape"]), R.plane_regions(s["touching_bar"])
    assert len(c) == 1 and len(bar) == 1 and not (c[0] & bar[0]).any()
    groups, shared = R.merge([c, bar], False)
    assert len(groups) == 2 and shared == 1 and [n for _, n in groups] == [1, 1]
    assert not any(m[25, 27] for m, _ in groups)   # the enclosed area belongs to nobody
    assert R.merge([c, bar], True)[0] == []
    assert R.same_groups(groups, R.merge_pairwise([c, bar], False))
    class_map, _, _ = R.segment(*R.hand_made_cases()["c_closed_by_touching_piece"])
    assert not class_map.any()


def test_overlapping_halves_take_the_gap_they_enclose():
    s = R.shapes()
    halves = [R.plane_regions(s["left_half"]), R.plane_regions(s["right_half"])]
    groups, shared = R.merge(halves, True)
    assert len(groups) == 1 and groups[0][1] == 2 and shared == 0
    assert groups[0][0][25, 27] and np.array_equal(groups[0][0], R.plane_regions(R.box(10, 40, 10, 46))[0])
    assert R.same_groups(groups, R.merge_pairwise(halves, True))
    class_map, _, _ = R.segment(*R.hand_made_cases()["halves_enclosing_a_gap"])
    assert np.array_equal(class_map[0] == PRINTED, s["inside"])


def test_one_empty_key_leaves_nothing():
    s = R.shapes()
    assert R.merge([R.plane_regions(s["ring"]), []], False) == ([], 0)
    assert R.merge_pairwise([R.plane_regions(s["ring"]), []], False) == []
    class_map, _, _ = R.segment(*R.hand_made_cases()["one_key_empty"])
    assert not class_map.any()


def test_single_key_keeps_its_regions_whatever_the_flag():
    s = R.shapes()
    regions = R.plane_regions(s["blob"] | R.box(50, 52, 50, 52))
    groups, _ = R.merge([regions], True)
    assert len(groups) == 2 and all(n == 1 for _, n in groups)
    class_map, _, _ = R.segment(*R.hand_made_cases()["single_key_flag_set"])
    assert np.array_equal(class_map[0] == PRINTED, s["inside"])


def test_score_tie_goes_to_the_first_class_of_the_colour_map():
    cases = R.hand_made_cases()
    maps, spec = cases["score_tie"]
    classes = [n for n in spec["class_to_color_map"] if n != "background"]
    masks = R.class_masks({k: v[0] for k, v in maps.items()}, spec["label_map"], classes, 64)
    fine = R.merge([R.plane_regions(masks[k]["printed_text"]) for k in ("12", "13")], True)[0]
    text = {c: R.merge([R.plane_regions(masks[k][c]) for k in ("8", "9")], False)[0] for c in classes}
    scores = [int((fine[0][0] & text[c][0][0]).sum()) for c in classes]
    assert len(fine) == 1 and scores[0] == scores[1] > 0
    class_map, _, _ = R.segment(maps, spec)
    assert set(np.unique(class_map)) == {0, PRINTED}
    class_map, colour, _ = R.segment(*cases["score_tie_other_order"])   # handwritten_text is class 1 there
    assert set(np.unique(class_map)) == {0, 1} and (colour[class_map == 1] == (255, 0, 0)).all()


def test_area_equal_to_the_minimum_is_kept_and_one_less_is_not():
    maps, spec, twice_area = R.area_threshold_case()
    assert twice_area % 2 == 0
    spec["min_class_contour_area"] = twice_area // 2
    assert R.segment(maps, spec)[0].any()
    spec["min_class_contour_area"] = twice_area // 2 + 1
    assert not R.segment(maps, spec)[0].any()


def test_drop_flag_needs_a_tall_and_a_wide_region_of_one_class():
    cases = R.hand_made_cases()
    class_map, _, drop = R.segment(*cases["drop_same_class"])
    assert drop[0] == 1 and set(np.unique(class_map)) == {0, PRINTED}
    class_map, _, drop = R.segment(*cases["no_drop_different_classes"])
    assert drop[0] == 0 and set(np.unique(class_map)) == {0, PRINTED, HANDWRITTEN}


# ---- host logic ----------------------------------------------------------------------------------------------------------------
def _segmenter(tmp_path, spec, clusters=3):
    from segmentation.black_white_handwritten_printed_text_segmenter import BlackWhiteHandwrittenPrintedTextDatasetSegmenter
    R.write_segmenter_files(str(tmp_path), spec, clusters)
    return BlackWhiteHandwrittenPrintedTextDatasetSegmenter(**R.segmenter_arguments(tmp_path, spec, clusters))


def test_label_map_inversion_and_tables(tmp_path):
    table = {k: {0: "background", 1: "printed_text", 2: "handwritten_text", 3: "printed_text"} for k in R.KEYS}
    spec = R.make_spec(clusters_to_class=table, keys_to_merge={"both": ["12", "13"]},
                       keys_for_finegrained_segmentation=["12", "both"])
    seg = _segmenter(tmp_path, spec, clusters=4)
    assert seg.class_label_map["12"] == {"background": [0], "printed_text": [1, 3], "handwritten_text": [2]}
    assert seg.class_label_map == spec["label_map"]
    assert seg.base_keys == ["8", "9", "12", "13"] and seg.sources_of == {"8": 1, "9": 2, "12": 4, "both": 12}
    lut = seg.lookup_table(seg.base_keys)
    assert lut.shape == (4, 256) and lut[2, :5].tolist() == [0, 1, 2, 1, 0] and not lut[:, 4:].any()
    assert sorted(seg.catalog) == ["12", "13", "8", "9"] and seg.catalog["8"].cluster_centers.shape == (4, 4)
    assert seg.check_sanity_of_class_label_map(set(R.KEYS)) == {}
    with pytest.raises(NotImplementedError):
        seg.render_debug_contours({}, "x")


def test_sanity_assertion_names_the_unknown_classes(tmp_path):
    table = {k: {0: "background", 1: "printed_text", 2: "stamp"} for k in R.KEYS}
    with pytest.raises(AssertionError, match="stamp"):
        _segmenter(tmp_path, R.make_spec(clusters_to_class=table))


def test_missing_printed_text_raises(tmp_path):
    spec = R.make_spec()
    spec["class_to_color_map"] = {"background": (0, 0, 0), "handwritten_text": (255, 0, 0)}
    with pytest.raises(ValueError, match="printed_text"):
        _segmenter(tmp_path, spec)


def test_resolution_above_image_size_and_cpu_tensors_raise(tmp_path):
    seg = _segmenter(tmp_path, R.make_spec(size=32))
    maps = {k: torch.zeros((1, 32, 32), dtype=torch.int64) for k in R.KEYS}
    with pytest.raises(NotImplementedError):
        seg.label_cluster_maps(maps)
    with pytest.raises(NotImplementedError):
        seg.create_segmentation_image({int(k): torch.zeros((1, 4, 16, 16)) for k in R.KEYS})
    maps["9"] = torch.zeros((1, 64, 64), dtype=torch.int64)
    with pytest.raises(ValueError, match="64"):
        seg.label_cluster_maps(maps)
    with pytest.raises(ValueError, match="64"):
        seg.label_activations({int(k): torch.zeros((1, 4, 64, 64)) for k in R.KEYS})
    with pytest.raises(ValueError):
        R.enlarge(np.zeros((64, 64)), 32)


def test_header_and_ctypes_table_agree_on_the_new_symbols():
    import sis_hip
    text = open(os.path.join(ROOT, "include", "sis_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("sis_cluster_segment", "sis_cluster_segment_workspace_bytes"):
        assert name in sis_hip.exported_symbols(), name
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, text).group(1)
        assert len(sis_hip._SIGNATURES[name][0]) == len([a for a in decl.split(",") if a.strip()]), name


def test_product_imports_neither_scipy_nor_cv2():
    for rel in MODULES:
        text = open(os.path.join(SRC, rel)).read()
        assert not re.search(r"^\s*(from|import)\s+(scipy|cv2)\b", text, flags=re.M), rel
    code = ("import sys; import segmentation.black_white_handwritten_printed_text_segmenter, utils.dataset_creation; "
            "assert not [m for m in sys.modules if m.split('.')[0] in ('scipy', 'cv2')]")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=SRC, env={**os.environ, "PYTHONPATH": SRC})
