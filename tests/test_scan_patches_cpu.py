"""Host side of the scan patches: the yardstick (tests/scan_patches_restatement.py) against Pillow itself, the
host tables (utils/scan_patches.py) against the yardstick, and scripts/create_stylegan_train_dataset.py on its Pillow path."""
import ctypes
import json
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scan_patches_pages as P  # noqa: E402
import scan_patches_restatement as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = {"sis_scan_reduce", "sis_scan_resample_workspace_bytes", "sis_scan_resample", "sis_scan_patches"}
NEW_KERNELS = {"scan_reduce_kernel", "scan_hpass_kernel", "scan_vpass_kernel", "scan_patches_kernel"}
KINDS = ("random", "binary")
TALL_CASES = [((2, 300), (2, 40)), ((2, 300), (1, 40)), ((3, 1000), (1, 100))]


def _pil_thumbnail_size(width, height, s):
    image = Image.new("RGB", (width, height))
    image.thumbnail((s, s))
    return image.size


# ---- the size rule

def test_thumbnail_size_rule_against_pillow():
    from utils import scan_patches as U
    cases = [(w, h, s) for w in range(1, 41) for h in range(1, 41) for s in (1, 7, 16)] + [(w, h, s) for (w, h), s in R.THUMBNAIL_CASES]
    cases += [(2480, 3508, 877.0), (2480, 3508, 1169.3333333333333), (3000, 2121, 1000), (300, 214, 100.0)]
    for w, h, s in cases:
        want = _pil_thumbnail_size(w, h, s)
        for rule in (U.thumbnail_size, R.thumbnail_size):
            got = rule(w, h, s)
            assert (got or (w, h)) == want, (w, h, s, got, want)
            assert (got is None) == (math.floor(s) >= w and math.floor(s) >= h)


# ---- the yardstick against Pillow

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape,size", R.RESIZE_CASES + TALL_CASES)
def test_restatement_resample_equals_pillow(shape, size, kind):
    a = R.page(shape[0], shape[1], kind)
    want = np.asarray(Image.fromarray(a).resize(size, Image.BICUBIC, reducing_gap=None))
    assert np.array_equal(R.resample(a, size), want)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape,s", R.THUMBNAIL_CASES)
def test_restatement_thumbnail_equals_pillow(shape, s, kind):
    a = R.page(shape[0], shape[1], kind)
    image = Image.fromarray(a)
    image.thumbnail((s, s))
    got = R.thumbnail(a, s)
    assert got.shape == np.asarray(image).shape and np.array_equal(got, np.asarray(image))


def test_binary_pages_reach_both_ends_of_the_clip():
    """0 / 255 pages drive the negative lobes below 0 and the overshoot above 255: without the clip the sums leave the byte."""
    a = R.page(131, 97, "binary").astype(np.int64)
    coef, first, count = R.axis_tables(131, 0, 131, 40)
    sums = [(1 << 21) + (a[:, first[x]:first[x] + count[x], 0] * coef[x, :count[x]]).sum(axis=1) for x in range(40)]
    values = np.concatenate(sums) >> 22
    assert values.min() < 0 and values.max() > 255


@pytest.mark.parametrize("factors", [(2, 2), (3, 1), (7, 8), (1, 5), (16, 16)])
@pytest.mark.parametrize("shape", [(403, 297), (5, 3)])
def test_restatement_reduce_equals_pillow(shape, factors):
    a = R.page(shape[0], shape[1], "random")
    assert np.array_equal(R.reduce(a, *factors), np.asarray(Image.fromarray(a).reduce(factors)))


# ---- the host tables against the yardstick

def test_axis_tables_equal_the_restatements():
    from utils import scan_patches as U
    spans = [(w, 0.0, float(w), ow) for (w, _), (ow, _) in R.RESIZE_CASES] + [(h, 0.0, float(h), oh) for (_, h), (_, oh) in R.RESIZE_CASES]
    spans += [(135, 0.0, 403 / 3, 100), (87, 0.0, 603 / 7, 38), (250, 0.0, 999 / 4, 100), (1240, 0.0, 1240.0, 620)]
    for in_size, in0, in1, out_size in spans:
        table = U.axis_table(in_size, in0, in1, out_size)
        coef, first, count = R.axis_tables(in_size, in0, in1, out_size)
        assert table.ksize == coef.shape[1] and table.ksize % 2 == 1
        assert np.array_equal(np.array(table.coef), coef) and table.first == first.tolist() and table.count == count.tolist()
        # what the kernels rely on: 24 signed bits per coefficient, the sum of |k| * 255 inside int32, taps inside the source,
        # first indices that do not decrease, and a tile's span inside the staging bound of csrc/scan_patches.h
        assert np.abs(coef).max() < 1 << 23 and np.abs(coef).sum(axis=1).max() < 1.4 * (1 << 22)
        assert first.min() >= 0 and (first + count).max() <= in_size and (np.diff(first) >= 0).all()
        cap = (63 * (table.ksize - 1) + 3) // 4 + table.ksize + 2
        for x0 in range(0, out_size, 64):
            assert (first + count)[x0:x0 + 64].max() - first[x0] <= cap


def test_thumbnail_plans_follow_pillows_steps():
    from utils import scan_patches as U
    want = {((403, 297), 100): ((100, 74), (2, 2)), ((801, 603), 50): ((50, 38), (8, 7)), ((999, 1), 100): ((100, 1), (4, 1)),
            ((130, 97), 120): ((120, 90), (1, 1)), ((640, 480), 80): ((80, 60), (4, 4))}
    for (shape, s), (size, factors) in want.items():
        plan = U.thumbnail_plan(shape[0], shape[1], s)
        assert (plan.size, plan.factors) == (size, factors)
        assert plan.reduced == (-(-shape[0] // factors[0]), -(-shape[1] // factors[1]))
    assert U.thumbnail_plan(999, 1, 100).resamples[0].vertical is None      # one row stays one row: Pillow skips the pass
    assert U.thumbnail_plan(40, 30, 40) is None and U.thumbnail_plan(40, 30, 64) is None
    tall = U.resize_plans(2, 300, (1, 40))
    assert len(tall) == 2 and tall[0].horizontal is None and tall[0].size == (2, 40) and tall[1].vertical is None


# ---- windows

@pytest.mark.parametrize("shape,size", R.CROP_CASES)
def test_window_origins_and_patches_against_pillow_crop(shape, size):
    from utils import scan_patches as U
    width, height = shape
    a = R.page(width, height, "random")
    image = Image.fromarray(a)
    origins = U.patch_origins(width, height, size)
    assert origins == R.crop_origins(width, height, size)
    nx, ny = math.ceil(width / size), math.ceil(height / size)
    assert len(origins) == nx * ny
    patches = R.crop(a, origins, size)
    index = 0
    for y_idx in range(ny):   # the reference's formula, its float boxes handed to Pillow
        start_y = y_idx * (size - (ny * size - height) / ny)
        for x_idx in range(nx):
            start_x = x_idx * (size - (nx * size - width) / nx)
            assert origins[index] == (int(round(start_x)), int(round(start_y)))
            want = np.asarray(image.crop((start_x, start_y, start_x + size, start_y + size)))
            assert np.array_equal(patches[index], want), (shape, index)
            index += 1


def test_half_pixel_origins_go_to_even_and_short_pages_are_filled_black():
    from utils import scan_patches as U
    assert [x for x, _ in U.patch_origins(301, 260, 256)[:2]] == [0, 150]     # 150.5 -> 150
    assert [x for x, _ in U.patch_origins(303, 257, 256)[:2]] == [0, 152]     # 151.5 -> 152
    assert U.patch_origins(1000, 200, 256) == [(0, 0), (250, 0), (500, 0), (750, 0)]
    a = R.page(1000, 200, "random")
    patches = R.crop(a, U.patch_origins(1000, 200, 256), 256)
    assert not patches[:, 200:].any() and np.array_equal(patches[1, :200], a[:, 250:506])
    assert U.patch_origins(512, 256, 256) == [(0, 0), (256, 0)]


# ---- the tool

def _tool():
    from scripts import create_stylegan_train_dataset as tool
    return tool


def test_parser_takes_the_references_options_and_the_new_ones():
    parser = _tool().build_parser()
    args = parser.parse_args(["scans", "out", "100", "--image-size", "128", "--only-jsons", "--max-size", "2000", "--margin-remove",
                              "--filter", "page"])
    assert (args.root_dir, args.destination, args.max_num_samples) == ("scans", "out", 100)
    assert (args.image_size, args.only_jsons, args.max_size, args.margin_remove, args.filter) == (128, True, 2000, True, "page")
    args = parser.parse_args(["scans", "out", "100"])
    assert (args.image_size, args.only_jsons, args.max_size, args.margin_remove, args.filter) == (256, False, 3000, False, None)
    assert (args.seed, args.min_size, args.pixel_path, args.png_encoder) == (None, 1000, "device", None)
    assert _tool().resolve_paths(args) == ("device", "device")
    args = parser.parse_args(["scans", "out", "100", "--seed", "3", "--min-size", "500", "--pixel-path", "pil"])
    assert (args.seed, args.min_size) == (3, 500) and _tool().resolve_paths(args) == ("pil", "pil")
    assert _tool().decode_worker_count(64) == 16 and _tool().decode_worker_count(0) == 1
    help_text = parser.format_help()
    assert "decoded in full" in help_text and "OpenCV" in help_text


def test_margin_remove_raises(tmp_path):
    tool = _tool()
    args = tool.build_parser().parse_args([str(tmp_path), str(tmp_path / "out"), "5", "--margin-remove", "--pixel-path", "pil"])
    with pytest.raises(NotImplementedError, match="Canny.*contour hierarchy.*OpenCV is not a dependency"):
        tool.main(args)
    assert tool.MARGIN_REMOVE_MESSAGE.count(".") == 1   # one sentence


def test_import_needs_no_opencv_tqdm_or_pytorch_training():
    code = ("import sys; sys.path[:0] = [%r]; from scripts import create_stylegan_train_dataset as t; "
            "bad = [m for m in ('cv2', 'pytorch_training') if m in sys.modules]; assert not bad, bad; print('clean')"   # (torch itself loads tqdm)
            % os.path.join(ROOT, "synthesis-in-style_amd"))
    assert subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, check=True).stdout.strip() == "clean"
    source = open(os.path.join(ROOT, "synthesis-in-style_amd", "scripts", "create_stylegan_train_dataset.py")).read()
    assert not re.search(r"^\s*(import|from)\s+(cv2|tqdm|pytorch_training)\b", source, flags=re.M)


@pytest.fixture(scope="module")
def pil_run(tmp_path_factory):
    tool = _tool()
    root = P.write_pages(tmp_path_factory.mktemp("scan_pages"))
    out = tmp_path_factory.mktemp("scan_out")
    args = tool.build_parser().parse_args([str(root), str(out), "10", "--seed", "5", "--pixel-path", "pil"] + P.TOOL_OPTIONS)
    return root, out, tool.main(args)


def test_pil_path_end_to_end(pil_run):
    import random
    root, out, (train, val) = pil_run
    assert [json.load(open(out / name)) for name in ("train.json", "val.json")] == [train, val]
    # the same stream, drawn here: the shuffle of the sorted files, one factor per page, the shuffle before the split
    rng = random.Random(5)
    files = sorted(root / name for name, _, _ in P.PAGES)
    rng.shuffle(files)
    expected = []
    for path in files:
        image = Image.open(path).convert("RGB")
        if max(image.size) > 300:
            image.thumbnail((300, 300))
        factor = rng.randint(1, 4)
        image.thumbnail((max(max(image.size) / factor, 100),) * 2)
        count = math.ceil(image.width / 64) * math.ceil(image.height / 64)
        expected += [str((path.parent / f"{path.stem}_{i}.png").relative_to(root)) for i in range(count)]
        first = np.asarray(Image.open(out / path.parent.relative_to(root) / f"{path.stem}_0.png"))
        assert np.array_equal(first, np.asarray(image.crop((0, 0, 64, 64))))
    assert sorted(train + val) == sorted(expected) and len(expected) == len(set(expected)) > 20
    rng.shuffle(expected)
    split = int(len(expected) * 0.9)
    assert (train, val) == (expected[:split], expected[split:])
    written = sorted(str(p.relative_to(out)) for p in out.glob("**/*.png"))
    assert written == sorted(expected)
    assert all(Image.open(out / name).size == (64, 64) for name in expected)
    assert any(name.startswith(os.path.join("a", "b", "tall_")) for name in expected)
    from data.gan_image_dataset import DeviceImageDataset   # the list is what train_stylegan_2.py --images reads
    listed = DeviceImageDataset(str(out / "train.json"), 64, load=False)
    assert listed.image_data == train and all(os.path.isfile(os.path.join(listed.root, name)) for name in train)


def test_only_jsons_lists_what_the_destination_holds(pil_run, tmp_path):
    tool = _tool()
    _, out, (train, val) = pil_run
    before = sorted(train + val)
    args = tool.build_parser().parse_args([str(tmp_path / "unused"), str(out), "7", "--only-jsons", "--seed", "2"])
    new_train, new_val = tool.main(args)
    assert sorted(new_train + new_val) == before[:7] and len(new_train) == 6 and len(new_val) == 1
    assert json.load(open(out / "train.json")) == new_train
    args = tool.build_parser().parse_args([str(tmp_path / "unused"), str(out), "1000", "--only-jsons", "--seed", "5"])
    all_train, all_val = tool.main(args)
    assert sorted(all_train + all_val) == before and len(all_train) == int(len(before) * 0.9)
    assert not (tmp_path / "unused").exists()


def test_an_undecodable_page_is_printed_and_skipped(tmp_path, capsys):
    tool = _tool()
    root = tmp_path / "scans"
    root.mkdir()
    Image.fromarray(P.synthetic_page(130, 97, 9)).save(root / "good.png")
    (root / "broken.png").write_bytes(b"not a png")
    args = tool.build_parser().parse_args([str(root), str(tmp_path / "out"), "10", "--seed", "1", "--pixel-path", "pil"] + P.TOOL_OPTIONS)
    train, val = tool.main(args)
    assert "cannot identify image file" in capsys.readouterr().out
    assert train + val and all(os.path.basename(name).startswith("good_") for name in train + val)


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
    for wrapper in ("scan_reduce", "scan_resample", "scan_thumbnail", "scan_patches"):
        assert callable(getattr(sis_hip, wrapper))


def test_entries_decline_bad_arguments_before_any_launch():
    import sis_hip
    L = sis_hip.lib()
    p = ctypes.c_void_p(4096)   # never dereferenced: every case returns at its check
    odd = ctypes.c_void_p(4098)

    def error():
        return L.sis_last_error().decode()

    for kw, text in [(dict(h=0), "page 0 x"), (dict(w=16385), "outside 1..16384"), (dict(fx=0), "factors (0"), (dict(fx=300, fy=300), "product"),
                     (dict(out=None), "null")]:
        a = dict(out=p, h=10, w=10, fx=2, fy=2)
        a.update(kw)
        assert L.sis_scan_reduce(a["out"], p, a["h"], a["w"], a["fx"], a["fy"], None) != 0 and text in error(), (kw, error())

    assert L.sis_scan_resample_workspace_bytes(97, 131, 31, 40) == 97 * 120 and L.sis_scan_resample_workspace_bytes(97, 131, 31, 41) == 97 * 124
    assert L.sis_scan_resample_workspace_bytes(0, 131, 31, 40) == 0 and L.sis_scan_resample_workspace_bytes(97, 131, 31, 16385) == 0
    ws = L.sis_scan_resample_workspace_bytes(97, 131, 31, 40)

    def resample(in_h=97, in_w=131, out_h=31, out_w=40, kx=15, ky=15, tx=p, ty=p, workspace=p, workspace_bytes=ws, out=p):
        return L.sis_scan_resample(out, p, in_h, in_w, out_h, out_w, tx, tx, tx, kx, ty, ty, ty, ky, workspace, workspace_bytes, None)

    for kw, text in [(dict(in_h=0), "every side"), (dict(out_w=16385), "every side"), (dict(kx=69), "ksize_x 69"), (dict(ky=14), "ksize_y 14"),
                     (dict(kx=0, tx=None), "no horizontal pass"), (dict(ky=0, ty=None), "no vertical pass"), (dict(tx=None), "horizontal tables"),
                     (dict(ky=0, ty=p, out_h=97), "vertical tables"), (dict(workspace_bytes=ws - 1), "workspace of"),
                     (dict(workspace=None), "aligned workspace"), (dict(workspace=odd), "aligned workspace"), (dict(out=None), "null")]:
        assert resample(**kw) != 0 and text in error(), (kw, error())

    def patches(n=4, size=64, h=100, w=100, out=p, origins=p):
        return L.sis_scan_patches(out, p, origins, n, size, h, w, None)

    for kw, text in [(dict(n=0), "0 windows"), (dict(n=65536), "65536 windows"), (dict(size=0), "size 0"), (dict(size=4097), "size 4097"),
                     (dict(h=0), "page 0 x"), (dict(origins=None), "null"), (dict(out=odd), "aligned")]:
        assert patches(**kw) != 0 and text in error(), (kw, error())
