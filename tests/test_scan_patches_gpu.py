"""GPU parity of the scan-patch kernels (csrc/scan_patches.h) with Pillow itself: every comparison is of bytes
and exact.  The shapes are the lists of tests/scan_patches_restatement.py, which tests/test_scan_patches_cpu.py holds against
Pillow on the host."""
import argparse
import json
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scan_patches_checks as C  # noqa: E402
import scan_patches_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu
KINDS = ("random", "binary")


def _direct(fn, *args, **kwargs):
    return fn(*args, **kwargs)


def _put(device):
    return lambda t: t.to(device)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape,size", R.RESIZE_CASES)
def test_resample_equals_pillow_resize(device, shape, size, kind):
    C.check_resample(_direct, _put(device), shape, size, kind)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape,s", R.THUMBNAIL_CASES)
def test_thumbnail_equals_pillow_thumbnail(device, shape, s, kind):
    C.check_thumbnail(_direct, _put(device), shape, s, kind)


def test_thumbnail_leaves_a_fitting_page_alone(device):
    page = torch.from_numpy(R.page(40, 30, "random")).to(device)
    import sis_hip
    assert sis_hip.scan_thumbnail(page, 40) is page


@pytest.mark.parametrize("shape,size", [((2, 300), (2, 40)), ((2, 300), (1, 40)), ((3, 1000), (1, 100))])
def test_very_tall_pages_take_pillows_vertical_first_order(device, shape, size):
    """More than a hundred times taller than wide and losing rows: Pillow resamples the rows first, in a call of its own."""
    C.check_resample(_direct, _put(device), shape, size, "random")
    C.check_thumbnail(_direct, _put(device), shape, size[1], "binary")


def test_more_than_one_tile_in_both_directions(device):
    """200 output columns are four horizontal tiles (the last ragged), 70 rows five row groups; 1030 output bytes per row are
    two workgroups of the vertical pass."""
    C.check_resample(_direct, _put(device), (700, 70), (200, 33), "random")
    C.check_resample(_direct, _put(device), (1100, 40), (344, 40), "binary")
    C.check_resample(_direct, _put(device), (344, 90), (344, 31), "random")


@pytest.mark.parametrize("shape", [(403, 297), (5, 3)])
@pytest.mark.parametrize("factors", [(2, 2), (3, 1), (7, 8)])
def test_reduce_equals_pillow_reduce(device, shape, factors):
    import sis_hip
    a = R.page(shape[0], shape[1], "random")
    got = sis_hip.scan_reduce(torch.from_numpy(a).to(device), *factors)
    C.same_bytes(got, np.asarray(Image.fromarray(a).reduce(factors)), f"reduce {shape} {factors}")


@pytest.mark.parametrize("shape,size", R.CROP_CASES[:3] + [((512, 256), 256)])
def test_patches_equal_pillow_crop(device, shape, size):
    C.check_patches(_direct, _put(device), shape, size)


def test_two_calls_give_the_same_bytes(device):
    import sis_hip
    page = torch.from_numpy(R.page(403, 297, "random")).to(device)
    first, second = sis_hip.scan_thumbnail(page, 100), sis_hip.scan_thumbnail(page, 100)
    assert torch.equal(first, second)
    origins = [(0, 0), (150, 0), (-3, 290)]
    assert torch.equal(sis_hip.scan_patches(page, origins, 64), sis_hip.scan_patches(page, origins, 64))


def test_wrappers_refuse_what_the_entries_do_not_take(device):
    import sis_hip
    page = torch.from_numpy(R.page(40, 30, "random"))
    for call in (lambda: sis_hip.scan_reduce(page, 2, 2), lambda: sis_hip.scan_resample(page, (10, 10)),
                 lambda: sis_hip.scan_thumbnail(page, 10), lambda: sis_hip.scan_patches(page, [(0, 0)], 8)):
        with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
            call()
    on_device = page.to(device)
    with pytest.raises(RuntimeError, match="uint8"):
        sis_hip.scan_reduce(on_device.float(), 2, 2)
    with pytest.raises(RuntimeError, match="product <= 65536"):
        sis_hip.scan_reduce(on_device, 300, 300)
    with pytest.raises(RuntimeError, match="odd and <= 67"):   # 1000 -> 10 columns in one call: 401 taps
        sis_hip.scan_resample(torch.zeros((4, 1000, 3), dtype=torch.uint8, device=device), (10, 4))
    with pytest.raises(RuntimeError, match="size 5000 outside"):
        sis_hip.scan_patches(on_device, [(0, 0)], 5000)


@pytest.fixture(scope="module")
def page_dir(tmp_path_factory):
    import scan_patches_pages as P
    return P.write_pages(tmp_path_factory.mktemp("scan_pages"))


def test_tool_on_the_device_writes_the_pil_paths_dataset(device, page_dir, tmp_path):
    from scripts import create_stylegan_train_dataset as tool
    import scan_patches_pages as P
    lists = {}
    for pixel_path, encoder in (("pil", "pil"), ("device", "device")):
        out = tmp_path / pixel_path
        args = tool.build_parser().parse_args([str(page_dir), str(out), "10", "--seed", "5", "--pixel-path", pixel_path, "--png-encoder",
                                               encoder] + P.TOOL_OPTIONS)
        tool.main(args)
        lists[pixel_path] = [json.load(open(out / name)) for name in ("train.json", "val.json")]
    assert lists["device"] == lists["pil"]
    names = lists["pil"][0] + lists["pil"][1]
    assert len(names) == len(set(names)) > 20
    for name in names:
        want = np.asarray(Image.open(tmp_path / "pil" / name))
        got = np.asarray(Image.open(tmp_path / "device" / name))
        assert want.shape == (64, 64, 3) and np.array_equal(got, want), name
    written = sorted(str(p.relative_to(tmp_path / "device")) for p in (tmp_path / "device").glob("**/*.png"))
    assert written == sorted(names)
