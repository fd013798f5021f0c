"""The dataset's ground truth on the device (csrc/coco_gt.h) against tests/coco_gt_restatement.py: every
output is an integer and is compared exactly.  Shapes: p = 1, 5, 31, 32, 33 (one tile, a tile border) and 70 (3x3 ragged
tiles); B = 3, K = 3 with one class absent from one image and one colour of the image in no class."""
import argparse
import json

import numpy as np
import pytest
import torch

import coco_gt_restatement as R
import page_eval_restatement as E

pytestmark = pytest.mark.gpu

COLOURS = [[0, 0, 255], [255, 0, 0], [0, 200, 7]]


def _call(device, label, colours=COLOURS, **kw):
    import sis_hip
    return sis_hip.label_regions(torch.from_numpy(label).to(device), colours, **kw)


def _check(device, label, colours=COLOURS):
    """Full mode with the default capacities, listing mode, and the same bytes on a second run."""
    full = _call(device, label, colours)
    want = R.assert_equal_to_device(full, label, colours)
    worst_regions, worst_runs = ((label.shape[1] + 1) // 2) ** 2, label.shape[1] ** 2 + 1 + ((label.shape[1] + 1) // 2) ** 2
    assert full.regions.shape[2] == worst_regions and full.runs.shape[2] == worst_runs   # the defaults never truncate
    assert want["region_count"].max() <= worst_regions and want["run_total"].max() <= worst_runs
    listing = _call(device, label, colours, runs=False)
    assert listing.runs is None
    R.assert_equal_to_device(listing, label, colours, runs=False, want=want)
    R.assert_equal_to_device(_call(device, label, colours), label, colours, want=want)
    return want


def _random_masks(rng, p, density):
    """[3][3][p][p] disjoint class masks; class 1 is absent from image 1."""
    pick = rng.rand(3, p, p)
    which = rng.randint(0, 3, size=(3, p, p))
    masks = np.stack([(pick < density) & (which == k) for k in range(3)], axis=1)
    masks[1, 1] = False
    return masks


@pytest.mark.parametrize("p", [1, 5, 31, 32, 33, 70])
@pytest.mark.parametrize("density", [0.1, 0.5, 0.9])
def test_random_planes(device, p, density):
    rng = np.random.RandomState(1000 * p + int(10 * density))
    label = R.planes_to_label(_random_masks(rng, p, density), COLOURS)
    want = _check(device, label)
    assert want["region_count"][1, 1] == 0 and want["has"][1, 1] == 0
    if p >= 31:
        assert (label == 9).all(axis=3).any()   # the colour that is in no class


@pytest.mark.parametrize("p", [33, 70])
def test_smooth_noise_planes(device, p):
    """Regions that span several tiles, with holes and islands."""
    rng = np.random.RandomState(p)
    noise = E.smooth_noise_planes(rng, (3, 3, p, p), 0.25)
    winner = noise.argmax(axis=1)
    masks = np.stack([(noise[:, k] > 0.7) & (winner == k) for k in range(3)], axis=1)
    want = _check(device, R.planes_to_label(masks, COLOURS))
    assert want["has"].any() and max(len(t) for img in want["tables"] for t in img) >= 2


@pytest.mark.parametrize("p", [33, 70])
def test_hand_made_planes_at_tile_borders(device, p):
    """Every hand-made plane across the tile border at 32 (p = 70: also at 64), three shapes per image at three corners."""
    planes = R.hand_made_planes()
    names = sorted(planes)
    label = np.zeros((3, p, p, 3), np.uint8)
    placed = {}
    for j, name in enumerate(names + names[:2]):
        s = planes[name][0].shape[0]
        o, o2 = min(32 - s // 2, p - s), (min(64 - s // 2, p - s) if p > 64 else 0)
        y, x = [(o, o), (o, o2), (o2, o)][j % 3]
        label[j // 3][R.embed(planes[name][0], p, y, x)] = COLOURS[j % 3]
        placed[(j // 3, j % 3)] = (name, y, x)
    want = _check(device, label)
    for (b, k), (name, y, x) in placed.items():
        rows = np.asarray(planes[name][1])   # box, area and "is a stroke" move with the shape; the runs depend on the plane
        got = want["tables"][b][k]
        assert np.array_equal(got[:, 3:6], rows[:, 3:6]) and np.array_equal(got[:, 7] > 0, rows[:, 7] > 0), name
        assert np.array_equal(got[:, 1], rows[:, 1] + x) and np.array_equal(got[:, 2], rows[:, 2] + y), name


def test_hand_made_planes_alone(device):
    """The written-out tables themselves, each plane at its own size."""
    for name, (mask, rows, runs) in R.hand_made_planes().items():
        label = np.zeros(mask.shape + (3,), np.uint8)
        label[mask] = COLOURS[0]
        got = _call(device, label[None], COLOURS[:1])
        n = len(rows)
        assert int(got.region_count[0, 0]) == n and int(got.run_total[0, 0]) == len(runs), name
        assert got.regions[0, 0, :n].cpu().tolist() == rows and got.runs[0, 0, :len(runs)].cpu().tolist() == runs, name
        assert int(got.has[0, 0]) == int(len(runs) > 0), name


def test_serpentine_and_full_plane(device):
    """One region through all nine tiles of p = 70, the full plane, the lattices of most regions and of many kept regions."""
    p = 70
    masks = np.stack([R.serpentine(p), np.ones((p, p), bool), R.isolated_lattice(p)])[:, None]
    label = np.zeros((3, p, p, 3), np.uint8)
    label[masks[:, 0]] = COLOURS[0]
    want = _check(device, label, COLOURS[:1])
    assert [int(c) for c in want["region_count"][:, 0]] == [1, 1, 35 * 35]
    assert list(want["runs"][1][0]) == [0, p * p] and want["has"][2, 0] == 0


def test_capacities_truncate_and_report_the_true_totals(device):
    p = 33
    label = np.zeros((2, p, p, 3), np.uint8)
    label[0][R.l_lattice(p)] = COLOURS[0]
    label[1][R.l_lattice(p).T] = COLOURS[1]
    want = R.label_regions(label, COLOURS[:2])
    need_regions, need_runs = int(want["region_count"].max()), int(want["run_total"].max())
    assert need_regions == 121 and need_runs == 605
    small = _call(device, label, COLOURS[:2], max_regions=need_regions // 2, max_runs=need_runs // 2)
    assert small.regions.shape[2] == need_regions // 2 and small.runs.shape[2] == need_runs // 2
    R.assert_equal_to_device(small, label, COLOURS[:2], want=want)
    exact = _call(device, label, COLOURS[:2], max_regions=int(small.region_count.max()), max_runs=int(small.run_total.max()))
    R.assert_equal_to_device(exact, label, COLOURS[:2], want=want)
    assert exact.regions.shape[2] == need_regions and exact.runs.shape[2] == need_runs
    none = _call(device, label, COLOURS[:2], runs=False, max_regions=0)
    assert none.regions is None and none.runs is None
    R.assert_equal_to_device(none, label, COLOURS[:2], runs=False, want=want)


def test_wrapper_checks(device):
    import sis_hip
    good = torch.zeros((1, 4, 4, 3), dtype=torch.uint8, device=device)
    for label, colours in [(good.cpu(), COLOURS), (good.float(), COLOURS), (good[:, :3], COLOURS), (good, []), (good, [[1, 2]]),
                           (good, [[0, 0, 0]] * 9), (good, [[0, 0, 256]])]:
        with pytest.raises(RuntimeError):
            sis_hip.label_regions(label, colours)


# ---------------------------------------------------------------------------------------------------- the dataset tool

CLASS_COLOURS = {"background": "#000000", "printed_text": "#0000FF", "handwritten_text": "#FF0000"}


def _expected_from_pngs(directory, names):
    """has_* keys and annotations of the written PNGs by the restatement."""
    from segmentation.evaluation.coco_gt import COCOGtCreator
    creator = COCOGtCreator(CLASS_COLOURS, image_root=directory, region_provider=R.provider)
    listing = creator.determine_classes_in_images([directory / n for n in names["all"]])
    coco = creator.create_coco_gt_from_image_paths([directory / n for n in names["val"]])
    return dict(zip(names["all"], listing)), coco


def _strip_dates(coco):
    for image in coco["images"]:
        image.pop("date_captured")
    coco["info"].pop("year")
    return coco


@pytest.mark.parametrize("encoder", ["device", "pil"])
def test_tool_writes_listing_and_coco_gt(device, tmp_path, encoder):
    import create_dataset_for_segmentation as cds
    from segmentation.evaluation.coco_gt import COCOGtCreator
    from test_png_encode_gpu import _branch, _tiny_generator
    ckpt, _ = _tiny_generator(tmp_path)
    cfg, extra = _branch("dataset_gan", tmp_path)
    common = dict(checkpoint=str(ckpt), config=None, num_images=11, batch_size=4, truncate=False, png_encoder=encoder, png_writers=2,
                  **extra)
    plain, with_gt = tmp_path / "plain", tmp_path / "gt"
    assert cds.build_dataset(argparse.Namespace(save_to=str(plain), **common), cfg) == (11, (0, 11))
    cds.create_train_val_split(plain, cfg["seed"])
    args = argparse.Namespace(save_to=str(with_gt), ground_truth=True, **common)
    assert cds.build_dataset(args, cfg) == (11, (0, 11))
    creator = COCOGtCreator(cfg["class_to_color_map"], image_root=with_gt)
    cds.create_train_val_split(with_gt, cfg["seed"], ground_truth=creator)
    sidecar = with_gt / "class_listing.rank0.jsonl"
    assert len(sidecar.read_text().splitlines()) == 11

    # the flag changes no PNG and not the split; without it the directory is what it was
    files = sorted(f.relative_to(plain) for f in plain.rglob("*") if f.is_file())
    assert files == sorted(f.relative_to(with_gt) for f in with_gt.rglob("*") if f.is_file() and f.name not in
                           ("coco_gt.json", sidecar.name))
    for rel in files:
        if rel.suffix == ".png":
            assert (plain / rel).read_bytes() == (with_gt / rel).read_bytes(), rel
    train, val = json.loads((with_gt / "train.json").read_text()), json.loads((with_gt / "val.json").read_text())
    assert [e["file_name"] for e in train] == [e["file_name"] for e in json.loads((plain / "train.json").read_text())]
    assert all(set(e) == {"file_name"} for e in json.loads((plain / "val.json").read_text()))

    names = {"all": [e["file_name"] for e in train + val], "val": [e["file_name"] for e in val]}
    listing, coco = _expected_from_pngs(with_gt, names)
    for entry in train + val:
        assert {k: v for k, v in entry.items() if k != "file_name"} == listing[entry["file_name"]], entry
        assert set(entry) == {"file_name", "has_printed_text", "has_handwritten_text"}
    got = json.loads((with_gt / "coco_gt.json").read_text())
    assert _strip_dates(got) == _strip_dates(json.loads(json.dumps(coco)))
    assert [i["file_name"] for i in got["images"]] == names["val"] and got["images"][0]["width"] == 32
    assert any(v for entry in listing.values() for v in entry.values()) and len(got["annotations"]) > 0   # there is something to list

    # the split alone, on the same directory without its sidecars, gives the same files
    before = {n: (with_gt / n).read_text() for n in ("train.json", "val.json")}
    sidecar.unlink()
    cfg_path = tmp_path / "cfg.json"
    cfg_path.write_text(json.dumps(cfg))
    cds.main(argparse.Namespace(config=str(cfg_path), save_to=str(with_gt), only_create_train_val_split=True, ground_truth=True))
    assert {n: (with_gt / n).read_text() for n in before} == before
    assert _strip_dates(json.loads((with_gt / "coco_gt.json").read_text())) == got
