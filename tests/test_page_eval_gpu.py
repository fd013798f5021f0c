"""GPU parity of the page evaluation (csrc/contour_ops.hip, csrc/page_ops.hip) against the independent
restatement (tests/page_eval_restatement.py: numpy + scipy.ndimage) and the reference-made golden vectors
(tests/golden/page_eval.npz).  The contour filter, the confusion matrix and the class map are integer decisions: bit-exact, no
tolerance, no excluded pixel.  Voting assembly: rtol 1e-6 (at most C + 1 float32 roundings separate two orders of the class
sum and the division, C <= 16), exact zeros where nothing voted."""
import json
import os
import sys
from unittest import mock

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import page_eval_restatement as R  # noqa: E402
from oracle import analysis_ref as A  # noqa: E402

pytestmark = pytest.mark.gpu

#        P,  B, C, density, min_contour_area, min_confidence, background_class_id
FILTER_CASES = [
    (64, 16, 4, 0.10, 1, 0.0, 0),
    (64, 16, 4, 0.25, 55, 0.7, 2),
    (64, 3, 3, 0.45, 400, 0.7, 0),
    (250, 4, 3, 0.15, 55, 0.7, 0),
    (250, 2, 3, 0.30, 400, 0.0, 2),
    (250, 2, 4, 0.05, 1, 0.7, 2),
    (256, 4, 3, 0.05, 55, 0.7, 0),
    (256, 2, 4, 0.20, 400, 0.7, 2),
    (256, 2, 3, 0.40, 1, 0.0, 0),
    (512, 2, 3, 0.15, 55, 0.7, 0),
    (512, 1, 3, 0.30, 400, 0.0, 2),
    (512, 1, 4, 0.08, 1, 0.7, 2),
]


def _noise(p, b, c, density, seed):
    rng = np.random.RandomState(seed)
    pred = R.smooth_noise_planes(rng, (b, c, p, p), density, sigma=2.0 + 0.01 * p)
    edge = rng.rand(b, c, p, p) < 0.001   # values on both sides of the mask rule's boundary (q * 255 >= 1 in float32)
    pred[edge] = (np.float32(1.0) / np.float32(255.0)) * rng.choice(np.asarray([0.9999999, 1.0, 1.0000001], dtype=np.float32),
                                                                      size=int(edge.sum()))
    return pred


def _filter_twice(pred, min_confidence, min_contour_area, background, device):
    import sis_hip
    x = torch.from_numpy(pred).to(device)
    first = sis_hip.remove_small_contours(x, min_confidence, min_contour_area, background)
    second = sis_hip.remove_small_contours(x, min_confidence, min_contour_area, background)
    assert first.data_ptr() != second.data_ptr()
    assert torch.equal(first.view(torch.int32), second.view(torch.int32)), "two runs differ"
    return first.cpu()


@pytest.mark.parametrize("p,b,c,density,min_area,min_conf,background", FILTER_CASES)
def test_contour_filter_bit_exact_on_smooth_noise(device, p, b, c, density, min_area, min_conf, background):
    pred = _noise(p, b, c, density, seed=p + 7 * min_area + b)
    got = _filter_twice(pred, min_conf, min_area, background, device)
    want = R.remove_small_contours(pred, min_conf, min_area, background)
    removed = (want == 0) & (torch.from_numpy(R.threshold(pred, min_conf)) != 0)
    print(f"P={p} B={b} C={c} density={density} area={min_area} conf={min_conf}: "
          f"{int(removed.sum())} pixels removed, {int((got != want).sum())} differ")
    assert torch.equal(got, want)
    assert got.dtype == torch.float32 and tuple(got.shape) == (b, c, p, p)
    q = torch.from_numpy(R.threshold(pred, min_conf))
    assert torch.equal(got[:, background], q[:, background])   # the background plane only gets the threshold


def _hand_made_planes(p):
    """One plane per hand-made mask (placed away from, and on, the plane's edge), a full plane, an empty one, a spiral that
    crosses every tile many times (long label chains) and a ring around the whole plane with islands in it."""
    planes = []
    for name, mask in sorted(R.hand_made_masks().items()):
        for top, left in [(20, 23), (0, 0), (p - mask.shape[0], p - mask.shape[1]), (31, 30)]:
            plane = np.zeros((p, p), dtype=np.float32)
            plane[top:top + mask.shape[0], left:left + mask.shape[1]] = mask * np.float32(0.9)
            planes.append(plane)
    planes.append(np.full((p, p), 0.8, dtype=np.float32))
    planes.append(np.zeros((p, p), dtype=np.float32))
    spiral = np.zeros((p, p), dtype=np.float32)
    lo, hi = 1, p - 2
    while hi - lo > 16:   # concentric open squares joined into one stroke, 3 pixels wide, 8 apart
        spiral[lo:lo + 3, lo:hi + 1] = 0.9
        spiral[lo:hi + 1, hi - 2:hi + 1] = 0.9
        spiral[hi - 2:hi + 1, lo:hi + 1] = 0.9
        spiral[lo + 11:hi + 1, lo:lo + 3] = 0.9
        spiral[lo + 11:lo + 14, lo:lo + 14] = 0.9
        lo, hi = lo + 11, hi - 11
    planes.append(spiral)
    ring = np.zeros((p, p), dtype=np.float32)
    ring[0:4, :] = ring[-4:, :] = 0.7
    ring[:, 0:4] = ring[:, -4:] = 0.7
    ring[p // 2 - 3:p // 2 + 3, p // 2 - 3:p // 2 + 3] = 0.9   # islands in the hole: part of the ring's region
    ring[10:12, 40:43] = 0.9
    planes.append(ring)
    broken = ring.copy()
    broken[0:4, 17] = 0.0   # the same ring with a one-pixel-wide gap: the closing shuts it again
    planes.append(broken)
    open_ring = ring.copy()
    open_ring[0:4, 17:27] = 0.0   # a gap the closing leaves open: the inside is outside now, the islands are on their own
    planes.append(open_ring)
    return np.stack(planes)


@pytest.mark.parametrize("p", [64, 250])
@pytest.mark.parametrize("min_area", [1, 55, 400])
def test_contour_filter_bit_exact_on_hand_made_masks(device, p, min_area):
    planes = _hand_made_planes(p)
    pred = np.stack([np.full_like(planes, 0.3), planes], axis=1)   # class 0: background plane
    got = _filter_twice(pred, 0.0, min_area, 0, device)
    want = R.remove_small_contours(pred, 0.0, min_area, 0)
    differ = (got != want).flatten(1).sum(1)
    print(f"P={p} area={min_area}: planes with differences {differ.nonzero().flatten().tolist()}")
    assert torch.equal(got, want)
    if min_area == 400 and p == 64:
        spiral = len(R.hand_made_masks()) * 4 + 2
        assert (got[spiral, 1] != 0).any()   # the spiral is one long region and stays


def test_contour_filter_inside_a_graph(device):
    import sis_hip
    pred = _noise(256, 2, 3, 0.2, seed=99)
    static = torch.from_numpy(pred).to(device)
    side = torch.cuda.Stream(device=device)
    side.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(side):
        sis_hip.remove_small_contours(static, 0.7, 55, 0)
    torch.cuda.current_stream(device).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = sis_hip.remove_small_contours(static, 0.7, 55, 0)
    graph.replay()
    torch.cuda.synchronize(device)
    assert torch.equal(out.cpu(), R.remove_small_contours(pred, 0.7, 55, 0))
    other = _noise(256, 2, 3, 0.35, seed=100)
    static.copy_(torch.from_numpy(other))
    graph.replay()
    torch.cuda.synchronize(device)
    assert torch.equal(out.cpu(), R.remove_small_contours(other, 0.7, 55, 0))


@pytest.mark.parametrize("settings", ["default", "speckle"])
def test_doc_ufcn_predicts_at_its_default_settings(device, settings):
    """``DocUFCN.predict`` at ``min_contour_area = 55`` (raised NotImplementedError before the contour filter existed): equal to
    the restatement applied to the GPU's own softmax output."""
    from networks.doc_ufcn import DocUFCN
    torch.manual_seed(3)
    net = DocUFCN(3, 3).eval().to(device)
    assert net.min_contour_area == 55 and net.min_confidence == 0.7
    x = torch.randn(2, 3, 128, 128, device=device)
    if settings == "speckle":   # untrained softmax outputs sit near 1/3: a threshold among them leaves speckle to clean up
        with torch.no_grad():
            net.min_confidence = float(torch.softmax(net(x), dim=1)[:, 1:].flatten().quantile(0.6))
    with torch.no_grad(), mock.patch.object(net, "postprocess", wraps=net.postprocess) as spy:
        got = net.predict(x)
    softmax = spy.call_args[0][0]
    want = R.remove_small_contours(softmax.cpu(), net.min_confidence, 55, 0)
    kept = float((want != 0).float().mean())
    print(f"min_confidence={net.min_confidence}: {kept:.3f} of the confidences kept")
    assert torch.equal(got.cpu(), want)
    with torch.no_grad():
        classes = net.predict_classes(x)
    assert tuple(classes.shape) == (2, 1, 128, 128)


def test_voting_assembly_matches_reference_golden_and_restatement(device, golden_dir):
    from segmentation.analysis_segmenter import VotingAssemblySegmenter
    g = np.load(os.path.join(golden_dir, "page_eval.npz"))
    rng = np.random.RandomState(int(g["seed"]))
    for i, (w, h, p, o) in enumerate(g["cases"].tolist()):
        o = None if o < 0 else o
        boxes = A.calculate_bboxes_for_patches(w, h, p, o)
        preds = torch.from_numpy(rng.rand(len(boxes), 3, p, p).astype(np.float32))
        if i == 2:
            preds[:, :, 40:60, :] = 0.0
        seg = VotingAssemblySegmenter(torch.nn.Identity(), p, device, patch_overlap=o or 0)
        out, labels = seg.assemble_predictions(preds.to(device), (w, h), with_labels=True)
        out, labels = out.cpu(), labels.cpu()
        np.testing.assert_allclose(out[:, ::37, ::41].numpy(), g[f"voted_slice_{i}"], rtol=1e-6, atol=0)
        np.testing.assert_allclose(out[:, 40:60:7, ::5].numpy(), g[f"voted_rows_{i}"], rtol=1e-6, atol=0)
        want = R.assemble_vote(preds, boxes, w, h)
        np.testing.assert_allclose(out.numpy(), want.numpy(), rtol=1e-6, atol=0)
        assert abs(out.double().sum().item() - float(g[f"voted_sum_{i}"])) <= 1e-6 * float(g[f"voted_sum_{i}"])
        nothing = want.sum(dim=0) == 0
        assert bool((out[:, nothing] == 0).all())
        if i == 2:
            assert int(nothing.sum()) == 20 * w
        else:
            assert not bool(nothing.any())
        top2 = torch.topk(want, 2, dim=0)[0]
        decided = (top2[0] - top2[1]) > 1e-5
        assert decided[~nothing].float().mean() > 0.99
        assert torch.equal(labels.long()[decided], R.first_max_labels(want)[decided])
        assert bool((labels[nothing] == 0).all())   # all confidences equal (0): the first class
        gl = g[f"labels_slice_{i}"]
        d = decided[::17, ::19].numpy()
        np.testing.assert_array_equal(labels[::17, ::19].numpy()[d], gl[d])
        assert torch.equal(seg.assemble_predictions(preds.to(device), (w, h)).cpu(), out)


@pytest.mark.parametrize("classes", [2, 3, 5, 16])
def test_confusion_matrix_is_exact(device, classes):
    import sis_hip
    rng = np.random.RandomState(classes)
    total = torch.zeros((classes, classes), dtype=torch.int64, device=device)
    want_total = np.zeros((classes, classes), dtype=np.int64)
    for h, w in [(37, 53), (301, 199), (1, 4099)]:
        gt = rng.randint(0, classes, size=(h, w)).astype(np.uint8)
        conf = (rng.randint(0, 12, size=(classes, h, w)) / 11.0).astype(np.float32)   # few levels: many ties, first class wins
        labels = torch.argmax(torch.from_numpy(conf), dim=0)
        want = R.confusion_matrix(labels.numpy(), gt, classes)
        assert want.sum() == h * w
        gt_d = torch.from_numpy(gt).to(device)
        from_conf = sis_hip.confusion_matrix(torch.from_numpy(conf).to(device), gt_d, classes)
        from_labels = sis_hip.confusion_matrix(labels.to(torch.uint8).to(device), gt_d, classes)
        assert from_conf.dtype == torch.int64 and from_conf.is_cuda
        np.testing.assert_array_equal(from_conf.cpu().numpy(), want)
        np.testing.assert_array_equal(from_labels.cpu().numpy(), want)
        assert sis_hip.confusion_matrix(torch.from_numpy(conf).to(device), gt_d, classes, out=total) is total
        want_total += want
    np.testing.assert_array_equal(total.cpu().numpy(), want_total)   # accumulated over three pages


COLORS = {"printed_text": [255, 0, 0], "background": [0, 0, 0], "handwritten_text": "#0000ff"}


def test_ground_truth_color_image_to_class_map(device):
    from utils.segmentation_utils import segmentation_image_to_class_image
    rng = np.random.RandomState(4)
    palette = np.asarray([[0, 0, 0], [255, 0, 0], [0, 0, 255], [255, 0, 1], [12, 200, 7], [0, 0, 254]], dtype=np.uint8)
    image = palette[rng.randint(0, len(palette), size=(123, 77))]
    got = segmentation_image_to_class_image(torch.from_numpy(image).to(device), "background", COLORS)
    numeric = {**COLORS, "handwritten_text": [0, 0, 255]}
    want = R.color_to_class(image, "background", numeric)
    assert got.dtype == torch.uint8 and got.is_cuda
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    assert set(np.unique(want)) == {0, 1, 2}   # printed_text 1, handwritten_text 2, unmatched colours background
    assert torch.equal(segmentation_image_to_class_image(image, "background", COLORS, device=device), got)


def _synthetic_page(rng, h, w):
    """(page uint8 [H,W,3], true class map): paper with printed (blue) and handwritten (red) blobs of many sizes."""
    truth = np.zeros((h, w), dtype=np.uint8)
    for _ in range(60):
        cls = rng.randint(1, 3)
        bh, bw = rng.randint(1, 28), rng.randint(1, 40)
        top, left = rng.randint(0, h - bh), rng.randint(0, w - bw)
        truth[top:top + bh, left:left + bw] = cls
    ink = np.asarray([[245, 245, 240], [25, 30, 200], [205, 35, 30]], dtype=np.int64)
    page = np.clip(ink[truth] + rng.randint(-3, 4, size=(h, w, 3)), 0, 255).astype(np.uint8)
    return page, truth


def test_evaluate_pages_end_to_end(device):
    """A point-wise segmenter with wide margins between the classes (no confidence near a threshold or a tie, so the host
    softmax may stand in for the device's), two pages, a 2x2 hyper-parameter grid: the runs are EQUAL to the ones assembled
    from the restatements."""
    from networks.base_segmenter import BaseSegmenter
    from segmentation.analysis_segmenter import VotingAssemblySegmenter
    from segmentation.evaluation.analyze_image_segments import evaluate_pages

    class Pointwise(BaseSegmenter):
        num_classes = 3

        def forward(self, x):   # x in [-1, 1]: paper is bright everywhere, printed ink blue, handwriting red
            return torch.stack([2.0 * (x[:, 0] + x[:, 1] + x[:, 2]) - 1.0, 3.0 * (x[:, 2] - x[:, 0]) - 2.0,
                                3.0 * (x[:, 0] - x[:, 2]) - 4.0], dim=1)

    rng = np.random.RandomState(8)
    names = ["background", "printed_text", "handwritten_text"]
    pages, truths, gts = {}, {}, {}
    for name, (h, w) in {"page_a": (333, 450), "page_b": (300, 261)}.items():
        pages[name], truths[name] = _synthetic_page(rng, h, w)
        gt = truths[name].copy()
        gt[rng.rand(h, w) < 0.03] = 0   # the annotation disagrees with the ink here and there
        gts[name] = gt
    configs = [{"min_confidence": c, "min_contour_area": a, "patch_overlap": (32, 0.0)} for c in (0.0, 0.5) for a in (0, 30)]
    metrics = ["dice", "iou", "precision", "recall"]
    net = Pointwise()
    seg = VotingAssemblySegmenter(net.to(device), 128, device, batch_size=5)
    got = evaluate_pages(seg, pages, {k: torch.from_numpy(v).to(device) for k, v in gts.items()}, names, configs, metrics)

    want = {"runs": []}
    for config in configs:
        run = {"confusion_matrices": {}}
        total = np.zeros((3, 3), dtype=np.int64)
        for name, page in pages.items():
            h, w = page.shape[:2]
            boxes = A.calculate_bboxes_for_patches(w, h, 128, 32)
            with torch.no_grad():
                softmax = torch.softmax(net.forward(A.crop_patches(page, boxes)), dim=1)
            top2 = torch.topk(softmax, 2, dim=1)[0]
            assert float((top2[:, 0] - top2[:, 1]).min()) > 0.2 and float((softmax - 0.5).abs().min()) > 0.05
            assert float((softmax * 255.0 - 1.0).abs().min()) > 1e-4   # and none near the mask rule's boundary
            if config["min_contour_area"] > 0:
                preds = R.remove_small_contours(softmax, config["min_confidence"], config["min_contour_area"], 0)
            else:
                preds = torch.from_numpy(R.threshold(softmax.numpy(), config["min_confidence"]))
            voted = R.assemble_vote(preds, boxes, w, h)
            matrix = R.confusion_matrix(R.first_max_labels(voted).numpy(), gts[name], 3)
            total += matrix
            run["confusion_matrices"][name] = [float(v) for v in matrix.reshape(-1)]
            for metric in metrics:
                run.setdefault(f"detailed_{metric}_scores", {})[name] = R.calculate_metric(matrix, names, metric)
        for metric in metrics:
            run[f"average_{metric}_scores"] = R.calculate_metric(total, names, metric)
        run["hyperparams"] = config
        want["runs"].append(run)
    for k, (a, b) in enumerate(zip(got["runs"], want["runs"])):
        print(f"run {k} {a['hyperparams']}: matrix page_a {a['confusion_matrices']['page_a']} / {b['confusion_matrices']['page_a']}")
    assert got == want
    assert json.loads(json.dumps(got))["runs"][3]["hyperparams"]["patch_overlap"] == [32, 0.0]
    matrices = [run["confusion_matrices"]["page_a"] for run in got["runs"]]
    assert matrices[0] != matrices[1] and matrices[2] != matrices[3]   # the contour filter changes the outcome
    assert net.min_contour_area == 30 and net.min_confidence == 0.5   # set_hyperparams reached the network
