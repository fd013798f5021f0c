"""Guard-band cases (tests/guard_bands.py) of the ground-truth kernels (csrc/coco_gt.h): the label images, the five outputs and
the workspace between 0xFF bands.  Outputs and workspace are born 0xFF here, so every row, count and table field that is read
has to be written by the kernels first; the results are compared with tests/coco_gt_restatement.py as in
tests/test_coco_gt_gpu.py."""
import numpy as np
import pytest
import torch

import coco_gt_restatement as R
import guard_bands as G
import page_eval_restatement as E
from test_guard_bands_gpu import T

pytestmark = pytest.mark.gpu

COLOURS = [[0, 0, 255], [255, 0, 0]]


@pytest.fixture(autouse=True)
def _fresh_session():
    G.reset()
    yield
    G.reset()


def _run(device, monkeypatch, label, want=None, **kw):
    import sis_hip
    t = T(device, monkeypatch)
    result = t.run(sis_hip.label_regions, t.put(torch.from_numpy(label)), COLOURS, **kw)
    return R.assert_equal_to_device(result, label, COLOURS, runs=kw.get("runs", True), want=want), result


def _small_label():
    p = 33
    label = np.zeros((2, p, p, 3), np.uint8)
    label[0][R.l_lattice(p)] = COLOURS[0]
    label[0][R.embed(R.hand_made_planes()["ring_with_island"][0], p, 24, 24) & ~R.l_lattice(p)] = COLOURS[1]
    label[1][R.serpentine(p)] = COLOURS[1]
    label[1][32, 32] = (7, 7, 7)
    return label


@pytest.mark.parametrize("mode", ["full", "listing", "truncating"])
def test_small_shape(device, monkeypatch, mode):
    label = _small_label()
    kw = {"full": {}, "listing": {"runs": False}, "truncating": {"max_regions": 60, "max_runs": 300}}[mode]
    want, result = _run(device, monkeypatch, label, **kw)
    assert want["region_count"].max() > 60 and want["run_total"].max() > 300 and want["has"].sum() >= 3
    if mode == "truncating":   # what lies behind the stored prefixes of the last plane is still as it was born
        assert result.regions.shape[2] == 60 and result.runs.shape[2] == 300


def test_workload_shape(device, monkeypatch):
    rng = np.random.RandomState(4)
    noise = E.smooth_noise_planes(rng, (4, 2, 256, 256), 0.2)
    masks = np.stack([(noise[:, k] > 0.7) & (noise.argmax(axis=1) == k) for k in range(2)], axis=1)
    _run(device, monkeypatch, R.planes_to_label(masks, COLOURS))
