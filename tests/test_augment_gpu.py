"""GPU: on-device augmentation and the device-resident PNG loader against the numpy / scipy restatement of DESIGN.md §12
(tests/augment_restatement.py).  The restatement is of the project's own statement; nothing here is compared with imgaug.

Shapes: B = 3 slots, a 45 x 83 source (odd sizes, 3-byte rows that are no multiple of 4, partial tiles; output at the same size
takes the scalar stores and S = 32 the 16-byte ones and the folded resize), one 40 x 40 square for the exact cases and the
loader, sigma = 9 (radius 36: a mirror halo wider than half of the 45 rows).
"""
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "synthesis-in-style_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import augment_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0") if torch.cuda.is_available() else None
IDENTITY_LUT = np.arange(256, dtype=np.uint8)
FIELDS = [(5.0, 25.0, 0x1234ABCD), (9.0, 5.0, 0xFEDCBA98)]   # (sigma, alpha, seed word)


def _blocks(rng, height, width, count=4):
    """A class map of `count` classes in rectangular blocks."""
    ys, xs = np.arange(height)[:, None] * 3 // height, np.arange(width)[None, :] * 4 // width
    return ((ys * 4 + xs + rng.integers(0, count)) % count).astype(np.uint8)


def _warp(pixels, classes, cases, fields=None, out_size=None, quantize=True, index=None):
    """cases: [(minv [2,3], lut [256], field slot)] -> (images [B,3,h,w] float32, segmented [B,h,w] int64) as numpy."""
    import sis_hip
    dev = lambda a, dtype: torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)   # noqa: E731
    b = len(cases)
    out = sis_hip.augment_warp(
        dev(pixels, torch.uint8), dev(classes, torch.uint8), dev(list(range(b)) if index is None else index, torch.int32),
        dev(np.stack([c[0] for c in cases]), torch.float32), dev(np.stack([c[1] for c in cases]), torch.uint8),
        dev([c[2] for c in cases], torch.int32), fields, out_size=out_size, quantize=quantize)
    assert out["images"].dtype == torch.float32 and out["segmented"].dtype == torch.int64 and out["segmented"].shape[1] == 1
    return out["images"].cpu().numpy(), out["segmented"][:, 0].cpu().numpy()


@pytest.fixture(scope="module")
def square():
    rng = np.random.default_rng(40)
    return rng.integers(0, 256, (1, 40, 40, 3), dtype=np.uint8), _blocks(rng, 40, 40)[None]


@pytest.fixture(scope="module")
def general():
    """The 45 x 83 inputs, the device-computed fields and one reference per (output size, slot), computed once."""
    import sis_hip
    from utils.augment_dataset import _resize, _translation, inverse_map, rotation_matrix, shear_matrix
    rng = np.random.default_rng(4583)
    h, w = 45, 83
    pixels = rng.integers(0, 256, (3, h, w, 3), dtype=np.uint8)
    classes = np.stack([_blocks(rng, h, w) for _ in range(3)])
    fields = sis_hip.elastic_field(h, w, [f[0] for f in FIELDS], [f[1] for f in FIELDS], seeds=[f[2] for f in FIELDS], device=DEV)
    fields_host = fields.cpu().numpy()
    forward = rotation_matrix(7.5, w, h) @ _translation(3.3, -2.1) @ shear_matrix(20.0, w, h)   # shear first
    data = {"pixels": pixels, "classes": classes, "fields": fields, "sizes": {}}
    for name, (out_h, out_w) in {"same": (h, w), "s32": (32, 32)}.items():
        minv = inverse_map(_resize(w, h, out_w, out_h) @ forward)
        cases = [(minv, IDENTITY_LUT, -1), (minv, IDENTITY_LUT, 0), (minv, IDENTITY_LUT, 1)]
        want = [R.warp(pixels[b], classes[b], minv, IDENTITY_LUT, out_h, out_w, None if slot < 0 else fields_host[slot])
                for b, (_, _, slot) in enumerate(cases)]
        data["sizes"][name] = {"out": (out_h, out_w), "cases": cases, "want": want}
    return data


# ---------------------------------------------------------------------------------------------------- 1. exact cases

@pytest.mark.parametrize("quantize", [True, False])
def test_exact_cases_are_bit_equal(square, quantize):
    from data.device_dataset import encode_batch
    from utils.augment_dataset import gamma_lut, inverse_map, rot90_matrix
    pixels, classes = square
    identity = np.array([[1, 0, 0], [0, 1, 0]], dtype=np.float32)
    shift = np.array([[1, 0, -3], [0, 1, 5]], dtype=np.float32)     # forward translation by (+3, -5)
    invert, gamma2 = (255 - IDENTITY_LUT).astype(np.uint8), gamma_lut(2.0)
    cases = [(identity, IDENTITY_LUT, -1), (shift, IDENTITY_LUT, -1), (inverse_map(rot90_matrix(1, 40, 40)), IDENTITY_LUT, -1),
             (inverse_map(rot90_matrix(3, 40, 40)), IDENTITY_LUT, -1), (identity, invert, -1), (identity, gamma2, -1)]
    images, segmented = _warp(pixels, classes, cases, quantize=quantize, index=[0] * len(cases))

    want = encode_batch(torch.from_numpy(pixels).to(DEV), torch.from_numpy(classes.astype(np.int64)).to(DEV))
    assert np.array_equal(images[0], want["images"][0].cpu().numpy())
    assert np.array_equal(segmented[0], want["segmented"][0, 0].cpu().numpy())

    def expect(image, label):
        return R.encode(image.astype(np.float32).transpose(2, 0, 1)), label.astype(np.int64)

    shifted, shifted_label = np.zeros_like(pixels[0]), np.zeros_like(classes[0])
    shifted[:35, 3:], shifted_label[:35, 3:] = pixels[0][5:, :37], classes[0][5:, :37]   # 0 / background in the uncovered band
    for slot, (image, label) in {1: (shifted, shifted_label),
                                 2: (np.rot90(pixels[0], -1), np.rot90(classes[0], -1)),
                                 3: (np.rot90(pixels[0], -3), np.rot90(classes[0], -3)),
                                 4: (invert[pixels[0]], classes[0]), 5: (gamma2[pixels[0]], classes[0])}.items():
        want_image, want_label = expect(image, label)
        assert np.array_equal(images[slot], want_image), slot
        assert np.array_equal(segmented[slot], want_label), slot
    assert (images[1][:, 35:] == -1.0).all() and (images[1][:, :, :3] == -1.0).all()


def test_sample_ids_outside_the_dataset_and_background_id(square):
    """A slot whose id is outside the resident arrays reads nothing: zero image, background label; the background id is the caller's."""
    import sis_hip
    pixels, classes = square
    dev = lambda a, dtype: torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)   # noqa: E731
    identity = np.tile(np.array([[1, 0, 0], [0, 1, 10]], dtype=np.float32), (3, 1, 1))   # output rows 30.. lie below the source
    out = sis_hip.augment_warp(dev(pixels, torch.uint8), dev(classes, torch.uint8), dev([0, 1, -1], torch.int32),
                               dev(identity, torch.float32), dev(np.tile(IDENTITY_LUT, (3, 1)), torch.uint8),
                               dev([-1, 7, -1], torch.int32), None, background_id=2)
    images, segmented = out["images"].cpu().numpy(), out["segmented"][:, 0].cpu().numpy()
    assert (images[1:] == -1.0).all() and (segmented[1:] == 2).all()
    assert (segmented[0, 30:] == 2).all() and np.array_equal(segmented[0, :-10], classes[0, 10:].astype(np.int64))
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        sis_hip.augment_warp(torch.zeros(1, 4, 4, 3, dtype=torch.uint8), dev(classes, torch.uint8), dev([0], torch.int32),
                             dev(identity[:1], torch.float32), dev(IDENTITY_LUT[None], torch.uint8), dev([-1], torch.int32))


# ---------------------------------------------------------------------------------------------------- 2. general warp

@pytest.mark.parametrize("size", ["same", "s32"])
def test_general_warp_unquantized(general, size):
    """Image values within 0.5 (of 255) of the float64 restatement: fp32 coordinates are good to ~3e-4 px, the steepest slope is
    255 per px in each axis -> ~0.15; a wrong tap on random pixels is off by tens.  Labels equal except within 1e-3 px of a
    rounding boundary in float64, at most 2 % of the pixels."""
    spec = general["sizes"][size]
    images, segmented = _warp(general["pixels"], general["classes"], spec["cases"], general["fields"], spec["out"], quantize=False)
    for b, (values, labels, (sx, sy)) in enumerate(spec["want"]):
        error = np.abs(R.decode(images[b]) - values).max()
        unsure = R.near_rounding_boundary(sx, sy, 1e-3)
        print(f"general warp {size} slot {b}: max |value error| {error:.4f} of 255, {100 * unsure.mean():.2f} % of labels left out")
        assert error <= 0.5, (size, b, error)
        assert unsure.mean() <= 0.02
        assert np.array_equal(segmented[b][~unsure], labels[~unsure]), (size, b)
        inside = (values.sum(0) > 0).mean()
        assert 0.3 < inside <= 1.0   # the case is not vacuous: a good part of the output shows the source


# ---------------------------------------------------------------------------------------------------- 3. quantised bytes

@pytest.mark.parametrize("size", ["same", "s32"])
def test_general_warp_quantized(general, size):
    spec = general["sizes"][size]
    images, _ = _warp(general["pixels"], general["classes"], spec["cases"], general["fields"], spec["out"], quantize=True)
    for b, (values, _, _) in enumerate(spec["want"]):
        decoded = R.decode(images[b])
        got = np.rint(decoded)
        assert np.abs(decoded - got).max() < 1e-3    # bytes came out
        want = np.rint(values)                       # half to even, as the kernel's rintf
        assert np.abs(got - want).max() <= 1, (size, b)
        clear = np.abs(values - np.floor(values) - 0.5) > 0.2
        print(f"quantised warp {size} slot {b}: {100 * clear.mean():.1f} % of the values checked exactly")
        assert clear.mean() >= 0.5
        assert np.array_equal(got[clear], want[clear]), (size, b)


# ---------------------------------------------------------------------------------------------------- 4. elastic field

def test_elastic_noise_equals_the_restated_hash():
    import sis_hip
    seeds = [0x1234ABCD, 0xFFFFFFFF]
    field, noise = sis_hip.elastic_field(45, 83, [5.0, 5.0], [1.0, 1.0], seeds=seeds, device=DEV, return_noise=True)
    noise = noise.cpu().numpy()
    for f, seed in enumerate(seeds):
        want = R.elastic_noise(seed, 45, 83)
        assert np.array_equal(noise[f], want)
        assert want.min() >= -1.0 and want.max() < 1.0 and abs(want.mean()) < 0.05
    assert not np.array_equal(noise[0], noise[1]) and not np.array_equal(noise[0, 0], noise[0, 1])
    again = sis_hip.elastic_field(45, 83, [5.0, 5.0], [1.0, 1.0], noise=torch.from_numpy(noise).to(DEV))
    assert torch.equal(again, field)   # the blur of the generated noise is the blur of the same noise supplied


def test_elastic_field_matches_gaussian_filter():
    import scipy.ndimage  # noqa: F401  (the restatement's Gaussian: a missing library fails the test)
    import sis_hip
    rng = np.random.default_rng(9)
    noise = rng.uniform(-1, 1, (2, 2, 45, 83)).astype(np.float32)
    field = sis_hip.elastic_field(45, 83, [f[0] for f in FIELDS], [f[1] for f in FIELDS], noise=torch.from_numpy(noise).to(DEV))
    field = field.cpu().numpy()
    for f, (sigma, alpha, _) in enumerate(FIELDS):
        want = R.elastic_field(noise[f], sigma, alpha)
        error = np.abs(field[f] - want).max()
        print(f"elastic field sigma {sigma} alpha {alpha}: max error {error:.2e} px, max |field| {np.abs(want).max():.2f} px")
        assert error <= 1e-4, (sigma, alpha, error)
        assert np.abs(want).max() > 0.05


def test_elastic_field_refuses_an_image_within_the_radius():
    import sis_hip
    with pytest.raises(ValueError, match="radius 36"):
        sis_hip.elastic_field(30, 83, [9.0], [5.0], seeds=[1], device=DEV)
    with pytest.raises(ValueError):
        sis_hip.elastic_field(45, 83, [9.5], [5.0], seeds=[1], device=DEV)
    assert sis_hip.elastic_radius(9.0) == 36 and sis_hip.elastic_radius(5.0) == 20


# ---------------------------------------------------------------------------------------------------- 5. loader end to end

COLORS = {"background": [0, 0, 0], "printed_text": [255, 0, 0], "handwritten_text": [0, 0, 255], "stamp": [0, 255, 0]}


@pytest.fixture(scope="module")
def png_dataset(tmp_path_factory):
    from PIL import Image
    root = tmp_path_factory.mktemp("pairs")
    rng = np.random.default_rng(6)
    table = np.array(list(COLORS.values()), dtype=np.uint8)
    samples = []
    for i in range(6):
        image, label = rng.integers(0, 256, (40, 40, 3), dtype=np.uint8), _blocks(rng, 40, 40)
        (root / str(i // 3)).mkdir(exist_ok=True)
        Image.fromarray(np.concatenate([image, table[label]], axis=1)).save(str(root / str(i // 3) / f"{i:04d}.png"))
        samples.append((image, label))
    (root / "train.json").write_text(json.dumps([{"file_name": f"{i // 3}/{i:04d}.png"} for i in range(6)]))
    (root / "colors.json").write_text(json.dumps(COLORS))
    return root, samples


def _dataset(root, **kwargs):
    from data.segmentation_dataset import AugmentedSegmentationDataset
    return AugmentedSegmentationDataset(root / "train.json", root=str(root), class_to_color_map_path=root / "colors.json",
                                        num_augmentations=3, device=DEV, **kwargs)


def test_loader_epoch(png_dataset):
    from data.device_dataset import DeviceSegmentationLoader, encode_batch
    root, samples = png_dataset
    dataset = _dataset(root)
    assert len(dataset) == 18 and dataset.resident and dataset.pixels.is_cuda and dataset.pixels.dtype == torch.uint8
    assert tuple(dataset.pixels.shape) == (6, 40, 40, 3) and tuple(dataset.classes.shape) == (6, 40, 40)
    ordered = list(DeviceSegmentationLoader(dataset, 4, shuffle=False, seed=3))
    assert len(ordered) == 18 // 4 == len(DeviceSegmentationLoader(dataset, 4, shuffle=False))
    for batch in ordered:
        assert batch["images"].dtype == torch.float32 and tuple(batch["images"].shape) == (4, 3, 40, 40)
        assert batch["segmented"].dtype == torch.int64 and tuple(batch["segmented"].shape) == (4, 1, 40, 40)
        assert batch["images"].is_cuda and not batch["images"].requires_grad and torch.is_grad_enabled()
        assert batch["images"].min() >= -1 and batch["images"].max() <= 1 and 0 <= batch["segmented"].min() <= batch["segmented"].max() < 4
    # indices 0..5 are the originals: encode_batch of the file bytes, bit for bit
    want = encode_batch(torch.from_numpy(np.stack([s[0] for s in samples])).to(DEV),
                        torch.from_numpy(np.stack([s[1] for s in samples]).astype(np.int64)).to(DEV))
    got_images = torch.cat([ordered[0]["images"], ordered[1]["images"][:2]])
    got_labels = torch.cat([ordered[0]["segmented"], ordered[1]["segmented"][:2]])
    assert torch.equal(got_images, want["images"]) and torch.equal(got_labels, want["segmented"])
    assert not torch.equal(ordered[1]["images"][2], want["images"][0])   # index 6: an augmented draw of sample 0
    item = dataset[2]
    assert torch.equal(item["images"], want["images"][2]) and torch.equal(item["segmented"], want["segmented"][2])

    def epoch(seed, **kwargs):
        return list(DeviceSegmentationLoader(_dataset(root, **kwargs), 4, seed=seed))

    first, second, other = epoch(3), epoch(3), epoch(4)
    assert all(torch.equal(a[k], b[k]) for a, b in zip(first, second) for k in a)
    assert not all(torch.equal(a["images"], b["images"]) for a, b in zip(first, other))
    spilled = epoch(3, max_resident_bytes=0)   # the pinned-host fallback yields the same batches
    assert all(torch.equal(a[k], b[k]) for a, b in zip(first, spilled) for k in a)
    loader = DeviceSegmentationLoader(dataset, 4, seed=3)
    one, two = list(loader), list(loader)      # a second pass is the next epoch
    assert not all(torch.equal(a["images"], b["images"]) for a, b in zip(one, two))
    ranks = [DeviceSegmentationLoader(dataset, 4, rank=r, world_size=2, seed=3) for r in range(2)]
    assert sorted(ranks[0].indices(0) + ranks[1].indices(0)) == list(range(18))
    assert len(list(ranks[1])) == len(ranks[1]) == 2


def test_loader_refuses_mixed_sizes_and_train_builds_it(png_dataset, tmp_path):
    import train
    from PIL import Image
    from data.device_dataset import DeviceSegmentationLoader
    root, _ = png_dataset
    Image.fromarray(np.zeros((40, 64, 3), dtype=np.uint8)).save(str(tmp_path / "small.png"))
    (tmp_path / "mixed.json").write_text(json.dumps([{"file_name": str(root / "0" / "0000.png")}, {"file_name": str(tmp_path / "small.png")}]))
    from data.segmentation_dataset import SegmentationDataset
    with pytest.raises(ValueError, match="small.png"):
        SegmentationDataset(tmp_path / "mixed.json", class_to_color_map_path=root / "colors.json", device=DEV)
    args = train.parse_args(["cfg.yaml", "--images", str(root / "train.json"), "--class-to-color-map", str(root / "colors.json")])
    config = {"train_json": args.train_json, "batch_size": 4, "image_size": 32, "num_classes": 4, "num_augmentations": 5}
    loader = train.get_data_loader(config, 0, DEV, args)
    assert isinstance(loader, DeviceSegmentationLoader) and len(loader.dataset) == 30 and len(loader) == 7
    batch = next(iter(loader))
    assert tuple(batch["images"].shape) == (4, 3, 32, 32) and tuple(batch["segmented"].shape) == (4, 1, 32, 32)
    assert train.get_data_loader(config, 0, DEV, args, validation=True) is None


def test_shipped_config_builds_an_augmented_loader(png_dataset):
    """``train.py configs/segmenter/ema_net_resnet50_256.yaml --images train.json --val-images train.json --class-to-color-map
    colors.json`` as documented: five indices per file, four of them augmented, for training and -- as in the reference -- for
    validation; the 40 x 40 pairs are served at the config's 256."""
    import train
    import yaml
    from data.device_dataset import DeviceSegmentationLoader
    root, _ = png_dataset
    path = os.path.join(ROOT, "synthesis-in-style_amd", "configs", "segmenter", "ema_net_resnet50_256.yaml")
    args = train.parse_args([path, "--images", str(root / "train.json"), "--val-images", str(root / "train.json"),
                             "--class-to-color-map", str(root / "colors.json")])
    config = train.merge_config_and_args(yaml.safe_load(open(path)), args)
    loader = train.get_data_loader(config, 0, DEV, args)
    assert isinstance(loader, DeviceSegmentationLoader) and loader.shuffle and loader.drop_last
    assert len(loader.dataset) == 5 * 6 and sum(loader.dataset.is_augmented(i) for i in range(30)) == 24
    assert len(loader) == 30 // 16
    batch = next(iter(loader))
    assert tuple(batch["images"].shape) == (16, 3, 256, 256) and tuple(batch["segmented"].shape) == (16, 1, 256, 256)
    validation = train.get_data_loader(config, 0, DEV, args, validation=True)
    assert len(validation.dataset) == 30 and not validation.shuffle and not validation.drop_last and len(validation) == 2
    del config["num_augmentations"]
    with pytest.raises(KeyError, match="num_augmentations"):
        train.get_data_loader(config, 0, DEV, args)


def test_doc_ufcn_step_on_a_loader_batch(png_dataset):
    """One updater step of DocUFCN on a batch of the 40 x 40 pairs.  DocUFCN's own kernels refuse 40 x 40 inputs ((H / 8) (W / 8) must
    be a multiple of 4), so the loader serves the pairs at ``image_size`` 48, the smallest size above 40 they take: the resize
    is folded into the warp, as for every dataset whose files are not of the training size."""
    from data.device_dataset import DeviceSegmentationLoader
    from networks.doc_ufcn import get_doc_ufcn
    from training.fused_adam import GradientClipAdam
    from training.loop import get_current_reporter
    from updater.segmentation_updater import StandardUpdater
    root, _ = png_dataset
    torch.manual_seed(0)
    net = get_doc_ufcn("base")(4, 3, min_confidence=0.0, min_contour_area=0).to(DEV).train()
    loader = DeviceSegmentationLoader(_dataset(root, image_size=48), 4, seed=1)
    opt = GradientClipAdam(net.parameters(), lr=5e-3, betas=(0.5, 0.999), weight_decay=1e-4)
    updater = StandardUpdater(iterators={'images': loader}, networks={'segmentation': net}, optimizers={'main': opt}, device=DEV,
                              class_weights=[1.0, 2.0, 2.0, 2.0], hip_graph=False)
    assert tuple(next(iter(loader))["images"].shape) == (4, 3, 48, 48)
    updater.update()
    torch.cuda.synchronize()
    losses = {k: v for k, v in get_current_reporter().scalars().items() if "loss" in k}
    assert losses and all(np.isfinite(v) for v in losses.values()), losses
    assert all(torch.isfinite(p).all() for p in net.parameters())


def test_synthesis_loader_augments_all_but_one_in_num_augmentations():
    """``SynthesisSegmentationLoader(num_augmentations=k)``: a slot stays unaugmented with probability 1 / k -- those slots are the
    plain loader's, bit for bit -- and the others pass through the warp; with None the loader is the plain one."""
    from data.device_dataset import SynthesisSegmentationLoader
    from networks.stylegan2.model import Generator
    from segmentation.gan_local_edit.factor_catalog import FactorCatalog
    torch.manual_seed(4)
    g = Generator(64, 64, 2, channel_multiplier=1).to(DEV).eval()
    layer = 7   # [B, C, 32, 32]: the label map is resized to the image's 64 x 64 before the warp
    with torch.no_grad():
        _, acts = g([torch.randn(1, 64, device=DEV)], return_intermediate_activations=True)
    rng = np.random.RandomState(9)
    catalogs = {layer: FactorCatalog(cluster_centers=rng.randn(6, acts[layer].shape[1]).astype(np.float32))}

    def first_batch(**kwargs):
        loader = SynthesisSegmentationLoader(g, catalogs, layer, batch_size=8, class_of_cluster=torch.tensor([0, 1, 2, 1, 0, 2]),
                                             image_size=64, seed=13, num_batches=1, **kwargs)
        torch.manual_seed(21)   # make_noise() draws from the device RNG
        return next(iter(loader))

    plain, augmented = first_batch(), first_batch(num_augmentations=3)
    assert augmented["images"].dtype == torch.float32 and tuple(augmented["images"].shape) == (8, 3, 64, 64)
    assert augmented["segmented"].dtype == torch.int64 and tuple(augmented["segmented"].shape) == (8, 1, 64, 64)
    assert torch.is_grad_enabled() and augmented["segmented"].max() <= 2 and augmented["images"].abs().max() <= 1
    kept = np.random.default_rng([13, 0x617567]).random(8) < 1.0 / 3   # the loader's first draw: seed 13 keeps slots 0, 3, 5, 6
    assert 0 < kept.sum() < 8
    for b in range(8):
        same = torch.equal(plain["images"][b], augmented["images"][b]) and torch.equal(plain["segmented"][b], augmented["segmented"][b])
        assert same == bool(kept[b]), b
