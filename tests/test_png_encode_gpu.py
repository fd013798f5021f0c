"""sis_hip.png_encode_pairs on the device: the file bytes EQUAL those of tests/png_restatement.py (and the sizes too), on the
smallest shapes at which each mechanism can go wrong; PIL decodes every device file to the input pixels; the dataset tool
writes the same dataset with ``--png-encoder device`` as with ``pil``."""
import argparse

import numpy as np
import pytest
import torch

import png_cases as K
import png_restatement as P

pytestmark = pytest.mark.gpu


def _encode(device, image, label=None, **kw):
    import sis_hip
    buffer, sizes = sis_hip.png_encode_pairs(torch.from_numpy(image).to(device), None if label is None else torch.from_numpy(label).to(device), **kw)
    torch.cuda.synchronize()
    assert buffer.dtype == torch.uint8 and sizes.dtype == torch.int32 and tuple(sizes.shape) == (image.shape[0],)
    return buffer.cpu().numpy(), sizes.cpu().numpy()


def _check(device, image, label=None):
    buffer, sizes = _encode(device, image, label)
    K.assert_files_equal(buffer, sizes, image, label)
    return buffer, sizes


def test_row_edge_one_pixel(device):
    """(H, W) = (1, 1): a 4-byte row, only the i < 3 edge of the filter."""
    _check(device, np.array([[[[7, 200, 143]]]], dtype=np.uint8))


@pytest.mark.parametrize("h,w,wl", [(3, 5, 0), (2, 87, 0), (3, 5, 2), (2, 87, 87)])
def test_unaligned_rows(device, h, w, wl):
    """Row lengths that are no multiple of 4, odd H; with a label the second half of a row starts at an odd address."""
    _check(device, *K.random_pair(h * 100 + w + wl, 2, h, w, wl))


@pytest.mark.parametrize("w", K.FLAT_WIDTHS)
def test_flat_row_258_cap_and_remainder(device, w):
    image = K.flat_row(w)
    tokens = P.tokens_closed_form(P.filtered_rows(image[0])[0])
    assert ("match", 258) in tokens   # the case is what it claims to be
    _check(device, image)


def test_length_code_boundaries(device):
    image = K.planted_runs()
    lengths = {v for kind, v in P.tokens_closed_form(P.filtered_rows(image[0])[0]) if kind == "match"}
    assert {3, 10, 11, 114, 115, 130, 131, 226, 227, 257, 258} <= lengths
    _check(device, image)


def test_literal_code_boundary(device):
    _check(device, K.literal_boundary())


def test_row_seams_in_a_batch_of_three(device):
    image, label = K.seam_batch()
    _, sizes = _check(device, image, label)
    assert len(set(sizes.tolist())) == 3


def test_stream_ending_on_and_off_a_byte_boundary(device):
    for image in K.byte_boundary_pair():
        _check(device, image)


def test_no_label_equals_label_none_and_wrapper_checks(device):
    import sis_hip
    image, label = K.random_pair(3, 2, 4, 6, 3)
    _check(device, image, None)
    with pytest.raises(RuntimeError):
        sis_hip.png_encode_pairs(torch.from_numpy(image).to(device), torch.from_numpy(label[:, :3]).to(device))
    with pytest.raises(RuntimeError):
        sis_hip.png_encode_pairs(torch.from_numpy(image))


def test_caller_buffer_and_two_encodes_are_byte_equal(device):
    """``out=``: a wider buffer that arrives full of 0xFF; the files are the same bytes as into a fresh one, twice."""
    import sis_hip
    image, label = K.random_pair(4, 3, 6, 9, 5)
    stride = sis_hip.png_capacity(6, 14) + 32
    out = torch.full((3, stride), 255, dtype=torch.uint8, device=device)
    buffer, sizes = _encode(device, image, label, out=out)
    assert buffer.shape[1] == stride
    K.assert_files_equal(buffer, sizes, image, label)
    again, sizes2 = _encode(device, image, label, out=out)
    fresh, sizes3 = _encode(device, image, label)
    assert np.array_equal(buffer, again) and np.array_equal(sizes, sizes2) and np.array_equal(sizes, sizes3)
    assert np.array_equal(buffer[:, :fresh.shape[1]], fresh)
    with pytest.raises(RuntimeError, match="out_stride"):
        sis_hip.png_encode_pairs(torch.from_numpy(image).to(device), torch.from_numpy(label).to(device), out=out[:, :64].contiguous())


def test_workload_shape(device):
    """The dataset's real shape, once: 256 rows of 1537 filtered bytes."""
    image, label, expected = K.workload_case()
    buffer, sizes = _encode(device, image, label)
    K.assert_files_equal(buffer, sizes, image, label, expected)


# ---------------------------------------------------------------------------------------------------- the dataset tool

def _tiny_generator(tmp_path):
    from networks import get_stylegan2_generator
    torch.manual_seed(0)
    g = get_stylegan2_generator(32, 512, n_mlp=2)
    ckpt = tmp_path / "g.pt"
    torch.save({"g_ema": g.state_dict()}, ckpt)
    centres = tmp_path / "c.npy"
    np.save(centres, np.random.RandomState(0).standard_normal((5, 512)).astype(np.float32))
    return ckpt, {"image_size": 32, "latent_size": 512, "n_mlp": 2, "seed": 3, "catalogs": {"7": str(centres)}, "label_layer": 7}


@pytest.fixture(scope="module")
def datasets(device, tmp_path_factory):
    """The tiny generator of tests/test_dataset_ops_gpu.py, the same 7 images written with both encoders."""
    import create_dataset_for_segmentation as cds
    tmp_path = tmp_path_factory.mktemp("png_datasets")
    ckpt, cfg = _tiny_generator(tmp_path)
    out = {}
    for encoder in ("pil", "device"):
        args = argparse.Namespace(checkpoint=str(ckpt), config=None, num_images=7, save_to=str(tmp_path / encoder), batch_size=3,
                                  truncate=False, png_encoder=encoder, png_writers=2)
        assert cds.build_dataset(args, cfg) == (7, (0, 7))
        cds.create_train_val_split(tmp_path / encoder, cfg["seed"])
        out[encoder] = (tmp_path / encoder, args.dropped_image_ids)
    return out


def test_build_dataset_device_encoder_writes_the_same_dataset(datasets):
    from PIL import Image
    (pil_dir, pil_dropped), (dev_dir, dev_dropped) = datasets["pil"], datasets["device"]
    assert pil_dropped == dev_dropped
    pil_files = sorted(p.relative_to(pil_dir) for p in pil_dir.rglob("*.png"))
    assert pil_files == sorted(p.relative_to(dev_dir) for p in dev_dir.rglob("*.png")) and len(pil_files) == 7
    for rel in pil_files:
        a, b = Image.open(pil_dir / rel), Image.open(dev_dir / rel)
        assert a.mode == b.mode == "RGB" and np.array_equal(np.asarray(a), np.asarray(b)), rel
    assert (dev_dir / "train.json").read_text() == (pil_dir / "train.json").read_text()
    # the device files are the format's bytes
    pixels = np.asarray(Image.open(dev_dir / pil_files[3]))
    assert (dev_dir / pil_files[3]).read_bytes() == P.encode_png(pixels[:, :32], pixels[:, 32:])


def _branch(branch, tmp_path):
    """(creation config, extra arguments) of the other three label branches of ``flush``, set up as the existing end-to-end
    tests of each labeller do."""
    base = {"image_size": 32, "latent_size": 512, "n_mlp": 2, "seed": 3}
    colours = {"background": "#000000", "printed_text": "#0000FF", "handwritten_text": "#FF0000"}
    if branch == "zeros":
        return base, {}
    if branch == "dataset_gan":
        from test_dataset_gan_gpu import G
        torch.save({**{f"network_{i}": G.seeded_member(3, 512 * 8, seed=40 + i) for i in range(3)}, **{f"optimizer_{i}": {} for i in range(3)}},
                   tmp_path / "ens.pth")
        return {**base, "segmenter_type": "dataset_gan", "class_to_color_map": colours}, {"classifier_path": str(tmp_path / "ens.pth")}
    from test_cluster_segmenter_gpu import CLUSTERS, E2E_KEYS, R, e2e_spec
    R.write_segmenter_files(str(tmp_path / "ssd"), e2e_spec(), CLUSTERS, {k: 512 for k in E2E_KEYS})
    cfg = {**base, "segmenter_type": "black_white_handwritten_printed", "class_to_color_map": colours,
           "keys_for_class_determination": ["4", "5"], "keys_for_finegrained_segmentation": ["6", "7"], "keys_to_merge": {},
           "only_keep_overlapping": False, "min_class_contour_area": 2}
    return cfg, {"num_clusters": CLUSTERS, "semantic_segmentation_base_dir": tmp_path / "ssd"}


@pytest.mark.parametrize("branch", ["zeros", "dataset_gan", "cluster_segmenter"])
def test_build_dataset_other_label_branches(device, tmp_path, monkeypatch, branch):
    """The label image built on the device in the branches the fixture above does not take; with the cluster-based labeller
    two images are flagged on top of its own decisions, so that ``keep`` is exercised: neither encoder writes them."""
    from PIL import Image
    import create_dataset_for_segmentation as cds
    ckpt, _ = _tiny_generator(tmp_path)
    cfg, extra = _branch(branch, tmp_path)
    original = cds.label_and_encode

    def flag_two(image, acts, catalogs, dataset_gan=None, cluster_segmenter=None):
        pixels, labels, ready = original(image, acts, catalogs, dataset_gan, cluster_segmenter)
        if ready is not None:
            ready.synchronize()
        labels["cluster_segmenter"][2][1:] = 1
        torch.cuda.synchronize()
        return pixels, labels, ready

    if branch == "cluster_segmenter":
        monkeypatch.setattr(cds, "label_and_encode", flag_two)
    dropped, files = {}, {}
    for encoder in ("pil", "device"):
        args = argparse.Namespace(checkpoint=str(ckpt), config=None, num_images=5, save_to=str(tmp_path / encoder), batch_size=3,
                                  truncate=False, png_encoder=encoder, png_writers=3, **extra)
        assert cds.build_dataset(args, cfg) == (5, (0, 5))
        dropped[encoder] = args.dropped_image_ids
        files[encoder] = {f.name: np.asarray(Image.open(f)) for f in (tmp_path / encoder).rglob("*.png")}
    assert dropped["pil"] == dropped["device"] and sorted(files["pil"]) == sorted(files["device"])
    if branch == "cluster_segmenter":
        assert {1, 2, 4} <= set(dropped["device"]) and len(files["device"]) == 5 - len(dropped["device"])
    else:
        assert dropped["device"] == [] and len(files["device"]) == 5
    for name, pixels in files["pil"].items():
        assert pixels.shape == (32, 64, 3) and np.array_equal(pixels, files["device"][name]), name
    if branch == "zeros":
        assert not files["device"]["0000.png"][:, 32:].any() and files["device"]["0000.png"][:, :32].any()


def test_device_written_directory_loads_to_the_same_tensors(device, datasets):
    """The resident dataset (data/segmentation_dataset.py) and the batches data/device_dataset.py deals from it."""
    import json
    from data.device_dataset import DeviceSegmentationLoader
    from data.segmentation_dataset import SegmentationDataset
    colours = {"background": [0, 0, 0], "b": [63, 63, 63], "c": [127, 127, 127], "d": [191, 191, 191], "e": [255, 255, 255]}
    loaded = []
    for encoder in ("pil", "device"):
        root = datasets[encoder][0]
        (root / "colors.json").write_text(json.dumps(colours))
        loaded.append(SegmentationDataset(root / "train.json", root=str(root), class_to_color_map_path=root / "colors.json", device=device))
    a, b = loaded
    assert len(a) == len(b) == 6
    assert torch.equal(a.pixels, b.pixels) and torch.equal(a.classes, b.classes)
    for x, y in zip(DeviceSegmentationLoader(a, 3, shuffle=False), DeviceSegmentationLoader(b, 3, shuffle=False)):
        assert torch.equal(x["images"], y["images"]) and torch.equal(x["segmented"], y["segmented"])
