"""Guard-band cases (tests/guard_bands.py) of the PNG encoder (csrc/png_encode.h): images, labels, the file buffer, the sizes
and the workspace between 0xFF bands.  The file buffer is born 0xFF here, so the entry's own clearing is what makes the
ORed stores right; the bytes are compared with tests/png_restatement.py as in tests/test_png_encode_gpu.py."""
import pytest
import torch

import guard_bands as G
import png_cases as K
from test_guard_bands_gpu import T

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _fresh_session():
    G.reset()
    yield
    G.reset()


def _run(device, monkeypatch, image, label, expected=None):
    import sis_hip
    t = T(device, monkeypatch)
    buffer, sizes = t.run(sis_hip.png_encode_pairs, t.put(torch.from_numpy(image)), None if label is None else t.put(torch.from_numpy(label)))
    K.assert_files_equal(buffer.cpu().numpy(), sizes.cpu().numpy(), image, label, expected)


@pytest.mark.parametrize("h,w,wl", [(3, 5, 2), (5, 87, 0)])   # rows of 22 and 262 bytes: no multiple of 4, label at an odd offset
def test_odd_shapes(device, monkeypatch, h, w, wl):
    _run(device, monkeypatch, *K.random_pair(h + w + wl, 3, h, w, wl))


def test_workload_shape(device, monkeypatch):
    _run(device, monkeypatch, *K.workload_case())
