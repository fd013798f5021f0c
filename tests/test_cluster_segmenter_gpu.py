"""Cluster-based labeller on the device (csrc/cluster_segment.hip) against the definition's restatement
(tests/cluster_segmenter_restatement.py, numpy + scipy.ndimage), byte for byte: class map, colour image and drop flags."""
import argparse
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cluster_segmenter_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu

CLUSTERS = 6
RESOLUTIONS = {"8": 16, "9": 32, "12": 32, "13": 64}


def build(base_dir, spec, clusters=CLUSTERS, channels=None):
    from segmentation.black_white_handwritten_printed_text_segmenter import BlackWhiteHandwrittenPrintedTextDatasetSegmenter
    R.write_segmenter_files(str(base_dir), spec, clusters, channels)
    return BlackWhiteHandwrittenPrintedTextDatasetSegmenter(**R.segmenter_arguments(base_dir, spec, clusters))


def on_device(segmenter, maps, device):
    out = segmenter.label_cluster_maps({k: torch.from_numpy(np.ascontiguousarray(v)).to(device) for k, v in maps.items()})
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def check(segmenter, maps, spec, device):
    class_map, colour, drop = on_device(segmenter, maps, device)
    want = R.segment(maps, spec)
    assert class_map.dtype == colour.dtype == drop.dtype == np.uint8
    assert np.array_equal(drop, want[2]), (drop, want[2])
    assert np.array_equal(class_map, want[0]), f"{int((class_map != want[0]).sum())} pixels of the class map differ"
    assert np.array_equal(colour, want[1])
    return class_map, colour, drop


@pytest.fixture(scope="module")
def random_maps():
    rng = np.random.RandomState(7)
    maps = {k: R.smooth_cluster_maps(rng, 3, r, CLUSTERS) for k, r in RESOLUTIONS.items()}
    return maps, R.random_class_table(rng, RESOLUTIONS, CLUSTERS)


@pytest.mark.parametrize("min_area", [1, 4, 50])
@pytest.mark.parametrize("only_keep_overlapping", [False, True])
def test_random_maps(device, tmp_path, random_maps, only_keep_overlapping, min_area):
    """S = 64 is 2 x 2 labelling tiles: cross-tile merges, the plane edge and the nearest enlargement from 16 and 32."""
    maps, table = random_maps
    spec = R.make_spec(clusters_to_class=table, only_keep_overlapping=only_keep_overlapping, min_class_contour_area=min_area)
    class_map, _, _ = check(build(tmp_path, spec), maps, spec, device)
    assert len(np.unique(class_map)) == 3   # the inputs exercise both text classes


@pytest.mark.parametrize("name", sorted(R.hand_made_cases()))
def test_hand_made_cases(device, tmp_path, name):
    maps, spec = R.hand_made_cases()[name]
    check(build(tmp_path, spec, clusters=3), maps, spec, device)


def test_area_threshold(device, tmp_path):
    maps, spec, twice_area = R.area_threshold_case()
    for area, painted in ((twice_area // 2, True), (twice_area // 2 + 1, False)):
        spec["min_class_contour_area"] = area
        class_map, _, _ = check(build(tmp_path / str(area), spec, clusters=3), maps, spec, device)
        assert class_map.any() == painted


def test_keys_to_merge(device, tmp_path, random_maps):
    """A new key made of two layers of different resolution, a key replaced by its union with another, and a merge of a merge."""
    maps, table = random_maps
    spec = R.make_spec(clusters_to_class=table, keys_to_merge={"fine": ["12", "13"], "9": ["8", "9"], "all": ["fine", "9"]},
                       keys_for_class_determination=["8", "9", "all"], keys_for_finegrained_segmentation=["12", "fine"],
                       only_keep_overlapping=True, min_class_contour_area=4)
    segmenter = build(tmp_path, spec)
    assert segmenter.sources_of == {"8": 1, "9": 3, "all": 15, "12": 4, "fine": 12}
    class_map, _, _ = check(segmenter, maps, spec, device)
    assert class_map.any()


def test_shipped_shape(device, tmp_path):
    rng = np.random.RandomState(11)
    resolutions = {"8": 64, "9": 64, "12": 256, "13": 256}
    maps = {k: R.smooth_cluster_maps(rng, 2, r, CLUSTERS) for k, r in resolutions.items()}
    spec = R.make_spec(size=256, clusters_to_class=R.random_class_table(rng, resolutions, CLUSTERS), min_class_contour_area=50)
    class_map, _, _ = check(build(tmp_path, spec), maps, spec, device)
    assert class_map.any()


def test_two_runs_are_byte_identical(device, tmp_path, random_maps):
    maps, table = random_maps
    spec = R.make_spec(clusters_to_class=table, only_keep_overlapping=True)
    segmenter = build(tmp_path, spec)
    first, second = on_device(segmenter, maps, device), on_device(segmenter, maps, device)
    assert all(np.array_equal(a, b) for a, b in zip(first, second))


def test_graph_replay_on_new_maps_equals_eager(device, tmp_path, random_maps):
    maps, table = random_maps
    spec = R.make_spec(clusters_to_class=table)
    segmenter = build(tmp_path, spec)
    rng = np.random.RandomState(13)
    other = {k: R.smooth_cluster_maps(rng, 3, r, CLUSTERS) for k, r in RESOLUTIONS.items()}
    eager = on_device(segmenter, other, device)   # also uploads the lookup table before the capture
    static = {k: torch.from_numpy(v).to(device) for k, v in maps.items()}
    stream = torch.cuda.Stream(device)
    stream.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(stream):
        segmenter.label_cluster_maps(static)
    torch.cuda.current_stream(device).wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = segmenter.label_cluster_maps(static)
    for k, v in other.items():
        static[k].copy_(torch.from_numpy(v))
    graph.replay()
    torch.cuda.synchronize()
    assert all(np.array_equal(t.cpu().numpy(), e) for t, e in zip(captured, eager))
    assert eager[0].any()


# ---- end to end ------------------------------------------------------------------------------------------------------------------
E2E_KEYS = {"4": 16, "5": 16, "6": 32, "7": 32}   # activation layers of Generator(32) and their resolutions


def e2e_spec():
    table = {"4": {0: "background", 1: "printed_text", 2: "handwritten_text", 3: "background", 4: "printed_text", 5: "background"},
             "5": {0: "printed_text", 1: "background", 2: "background", 3: "handwritten_text", 4: "printed_text", 5: "background"},
             "6": {0: "background", 1: "printed_text", 2: "background", 3: "printed_text", 4: "background", 5: "printed_text"},
             "7": {0: "printed_text", 1: "background", 2: "printed_text", 3: "background", 4: "printed_text", 5: "background"}}
    return R.make_spec(size=32, clusters_to_class=table, keys=tuple(E2E_KEYS), keys_for_class_determination=["4", "5"],
                       keys_for_finegrained_segmentation=["6", "7"], min_class_contour_area=2)


def small_generator():
    from networks import get_stylegan2_generator
    torch.manual_seed(0)
    return get_stylegan2_generator(32, 512, n_mlp=2)


def test_create_segmentation_image_on_generator_activations(device, tmp_path):
    spec = e2e_spec()
    segmenter = build(tmp_path, spec, channels={k: 512 for k in E2E_KEYS})
    g = small_generator().to(device).eval()
    torch.manual_seed(1)
    with torch.no_grad():
        _, acts = g([torch.randn(3, 512, device=device)], noise=g.make_noise(), return_intermediate_activations=True)
    maps = {k: segmenter.catalog[k].predict(acts[int(k)]).cpu().numpy() for k in E2E_KEYS}
    assert all(maps[k].shape == (3, r, r) for k, r in E2E_KEYS.items())
    want = R.segment(maps, spec)
    colour, to_drop = segmenter.create_segmentation_image(acts)
    assert isinstance(colour, np.ndarray) and colour.dtype == np.uint8 and np.array_equal(colour, want[1])
    assert to_drop == [int(i) for i in np.nonzero(want[2])[0]]
    masks = segmenter.predict_clusters(acts, segmenter.class_label_map)
    assert masks["6"]["printed_text"].dtype == torch.bool
    assert np.array_equal(masks["6"]["printed_text"].cpu().numpy(), np.isin(maps["6"], [1, 3, 5]))


def test_build_dataset_writes_colour_labels_and_skips_dropped_ids(device, tmp_path, monkeypatch):
    from PIL import Image
    import create_dataset_for_segmentation as cds
    spec = e2e_spec()
    R.write_segmenter_files(str(tmp_path / "ssd"), spec, CLUSTERS, {k: 512 for k in E2E_KEYS})
    torch.save({"g_ema": small_generator().state_dict()}, tmp_path / "g.pt")
    cfg = {"image_size": 32, "latent_size": 512, "n_mlp": 2, "seed": 3, "segmenter_type": "black_white_handwritten_printed",
           "class_to_color_map": {"background": "#000000", "printed_text": "#0000FF", "handwritten_text": "#FF0000"},
           "keys_for_class_determination": ["4", "5"], "keys_for_finegrained_segmentation": ["6", "7"], "keys_to_merge": {},
           "only_keep_overlapping": False, "min_class_contour_area": 2}
    args = argparse.Namespace(checkpoint=str(tmp_path / "g.pt"), config=None, num_images=7, save_to=str(tmp_path / "out"),
                              batch_size=3, truncate=False, num_clusters=CLUSTERS,
                              semantic_segmentation_base_dir=tmp_path / "ssd")
    seen = []   # (cluster maps of a batch) in the loop's order, from the very activations the loop labels
    original = cds.label_and_encode

    def spy(image, acts, catalogs, dataset_gan=None, cluster_segmenter=None):
        seen.append({k: cluster_segmenter.catalog[k].predict(acts[int(k)]).cpu().numpy() for k in E2E_KEYS})
        return original(image, acts, catalogs, dataset_gan, cluster_segmenter)

    monkeypatch.setattr(cds, "label_and_encode", spy)
    assert cds.build_dataset(args, cfg) == (7, (0, 7))
    want_colour = np.concatenate([R.segment(maps, spec)[1] for maps in seen])
    want_drop = np.concatenate([R.segment(maps, spec)[2] for maps in seen])
    assert len(want_colour) == 7 and args.dropped_image_ids == [int(i) for i in np.nonzero(want_drop)[0]]
    written = {f.name: f for f in (tmp_path / "out").rglob("*.png")}
    assert sorted(written) == [f"{i:04d}.png" for i in range(7) if not want_drop[i]]
    for i in range(7):
        if not want_drop[i]:
            pair = np.asarray(Image.open(written[f"{i:04d}.png"]))
            assert pair.shape == (32, 64, 3) and np.array_equal(pair[:, 32:], want_colour[i]), i
    assert want_colour.any()

    # without the segmenter_type the label half is still the grey cluster-id map
    monkeypatch.setattr(cds, "label_and_encode", original)
    centres = str(tmp_path / "ssd" / "catalogs" / str(CLUSTERS) / "centres_7.npy")
    plain = {"image_size": 32, "latent_size": 512, "n_mlp": 2, "seed": 3, "catalogs": {"7": centres}, "label_layer": 7}
    args.save_to = str(tmp_path / "plain")
    assert cds.build_dataset(args, plain) == (7, (0, 7)) and args.dropped_image_ids == []
    files = sorted((tmp_path / "plain").rglob("*.png"))
    assert [f.name for f in files] == [f"{i:04d}.png" for i in range(7)]
    right = np.asarray(Image.open(files[2]))[:, 32:]
    assert set(np.unique(right)) <= {0, 51, 102, 153, 204, 255} and (right[..., 0] == right[..., 1]).all()
    assert np.array_equal(right[..., 0], seen[0]["7"][2] * 255 // 5)
