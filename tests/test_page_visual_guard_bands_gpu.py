"""Guard-band cases (tests/guard_bands.py) of the page visualisation kernels (csrc/page_visual.h): the confidences, the scan,
the tables, every output and the workspace between 0xFF bands.  Outputs and workspace are born 0xFF here, so every count, row,
label and pixel that is read has to be written by the kernels first; the results are compared with
tests/page_visual_restatement.py as in tests/test_page_visual_gpu.py."""
import numpy as np
import pytest
import torch

import guard_bands as G
import page_visual_checks as C
from test_guard_bands_gpu import T

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _fresh_session():
    G.reset()
    yield
    G.reset()


@pytest.mark.parametrize("seed", [1, 4])   # (3, 33, 70) and (2, 40, 1100)
def test_page_between_bands(device, monkeypatch, seed):
    pred, scan, want = C.noise_case(seed)
    t = T(device, monkeypatch)
    C.check_page(t.run, t.put, pred, scan, want, device)


def test_truncating_capacity_between_bands(device, monkeypatch):
    pred, scan, want = C.noise_case(1)
    assert want["region_count"][1:].min() > 3
    t = T(device, monkeypatch)
    found = C.check_page(t.run, t.put, pred, scan, want, device, max_regions=3)
    assert tuple(found.regions.shape) == (3, 3, 8)
    skipped = found.regions[0].cpu().numpy()   # the background plane's rows: still as they were born
    assert np.array_equal(skipped, np.full_like(skipped, -1))
    assert torch.equal(found.region_count.cpu(), torch.from_numpy(want["region_count"]))
