"""GPU parity of the scanner-margin kernels (csrc/scan_margin.h) with the restatement
(tests/scan_margin_restatement.py): every comparison is of bytes and exact.  The cases are those of tests/scan_margin_cases.py,
whose constructed results tests/test_scan_margin_cpu.py holds against the restatement on the host."""
import json
import os
import random
import sys

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scan_margin_cases as K  # noqa: E402
import scan_margin_checks as C  # noqa: E402
import scan_margin_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu
NAMES = [name for name, _ in K.all_cases()]
TOOL_OPTIONS = ["--image-size", "64", "--min-size", "100", "--max-size", "300"]


def _direct(fn, *args, **kwargs):
    return fn(*args, **kwargs)


def _put(device):
    return lambda t: t.to(device)


@pytest.mark.parametrize("name", NAMES)
def test_edges_contours_info_and_box_equal_the_restatement(device, name):
    C.check_case(_direct, _put(device), name)
    C.check_case(_direct, _put(device), name, outputs=False)


@pytest.mark.parametrize("name", [name for name in NAMES if C.want(name).info[0] >= 2])
def test_a_short_table_holds_the_prefix_and_moves_nothing_else(device, name):
    C.check_truncated_table(device, name)


@pytest.mark.parametrize("name", NAMES)
def test_two_calls_give_the_same_bytes(device, name):
    page = torch.from_numpy(C.cases()[name]).to(device)
    rows = C.want(name).info[0] + 1
    first, second = C.entry(page, rows, rows), C.entry(page, rows, rows)
    for a, b in zip(first, second):
        assert torch.equal(a, b), name


def test_thresholds_are_arguments_of_the_entry(device):
    import sis_hip
    a = K.chain(ramp=False)   # a step of 10 grey levels, spread by the blur over rows of 100, 103, 107, 110: magnitude 4 * 7 = 28
    page = torch.from_numpy(a).to(device)
    for low, high in ((20, 150), (20, 27), (20, 28), (27, 27), (28, 150), (0, 0)):
        got = sis_hip.scan_content_box(page, low=low, high=high, edges=True)
        want = R.content_box(a, low, high)
        C.same(got.edges, want.edges, f"edges at {low}, {high}")
        C.same(got.info, want.info, f"info at {low}, {high}")
    # both comparisons are strict: 28 is strong above a high of 27 and not above 28, a candidate above a low of 27 and not of 28
    assert R.content_box(a, 20, 27).info[6] == R.content_box(a, 27, 27).info[6] == 160
    assert R.content_box(a, 20, 28).info[6] == R.content_box(a, 28, 150).info[6] == R.content_box(a, 20, 150).info[6] == 0


@pytest.mark.parametrize("index", range(len(K.TOOL_PAGES)))
def test_remove_margin_returns_the_restatements_crop(device, index):
    _, width, height = K.TOOL_PAGES[index]
    box, crop = C.check_remove_margin(_direct, _put(device), K.margin_page(width, height, index))
    assert crop != [0, 0, width, height]   # a margin was found


def test_wrappers_refuse_what_the_entry_does_not_take(device):
    import sis_hip
    page = torch.from_numpy(K.uniform())
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        sis_hip.scan_content_box(page)
    with pytest.raises(RuntimeError, match="outside 3..4096"):
        sis_hip.scan_content_box(torch.zeros((2, 10, 3), dtype=torch.uint8, device=device))
    with pytest.raises(RuntimeError, match="0 <= low <= high"):
        sis_hip.scan_content_box(page.to(device), low=30, high=20)


def test_tool_with_margin_remove_cuts_the_cropped_pages(device, tmp_path):
    """--margin-remove on the device path: every patch equals Pillow's sequence on the page cropped at the restatement's box,
    and the names and both lists are those of a run without the flag."""
    from scripts import create_stylegan_train_dataset as tool
    root = K.write_tool_pages(tmp_path / "scans")
    lists = {}
    for flag in (True, False):
        out = tmp_path / ("with" if flag else "without")
        args = tool.build_parser().parse_args([str(root), str(out), "10", "--seed", "5", "--pixel-path", "device", "--png-encoder", "pil"]
                                              + TOOL_OPTIONS + (["--margin-remove"] if flag else []))
        tool.main(args)
        lists[flag] = [json.load(open(out / name)) for name in ("train.json", "val.json")]
    rng = random.Random(5)
    files = sorted(root / name for name, _, _ in K.TOOL_PAGES)
    rng.shuffle(files)
    with_flag, without_flag = [], []
    for path in files:
        image = Image.open(path).convert("RGB")
        factor = rng.randint(1, 4)
        cropped, box, crop = R.remove_margin(np.asarray(image))
        assert np.array_equal(cropped, np.asarray(image.crop(crop))) and crop != [0, 0, image.width, image.height]
        stem = str((path.parent / path.stem).relative_to(root))
        for flag, page, names in ((True, Image.fromarray(cropped), with_flag), (False, image, without_flag)):
            patches = tool.page_patches_pil(page, factor, 64, 300, 100)
            names += [f"{stem}_{i}.png" for i in range(len(patches))]
            if flag:
                for i, patch in enumerate(patches):
                    got = np.asarray(Image.open(tmp_path / "with" / f"{stem}_{i}.png"))
                    assert np.array_equal(got, np.asarray(patch)), (stem, i)
    # one stream: the same files in the same order with the same factors, and (by the construction of the pages) as many
    # windows on a cropped page as on the whole one -- so the names and both lists are those of the run without the flag
    assert with_flag == without_flag and len(with_flag) == len(set(with_flag)) > 10
    rng.shuffle(with_flag)
    cut = int(len(with_flag) * 0.9)
    assert lists[True] == lists[False] == [with_flag[:cut], with_flag[cut:]]
    written = sorted(str(p.relative_to(tmp_path / "with")) for p in (tmp_path / "with").glob("**/*.png"))
    assert written == sorted(with_flag)
