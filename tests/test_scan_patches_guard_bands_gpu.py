"""Guard-band cases (tests/guard_bands.py) of the scan-patch kernels (csrc/scan_patches.h): the page, the tap tables, the
workspace of the horizontal pass and every output between 0xFF bands.  Outputs and workspace are born 0xFF here, so every byte
that is read has to be written by the kernels first; the results are compared with Pillow as in tests/test_scan_patches_gpu.py."""
import pytest

import guard_bands as G
import scan_patches_checks as C
from test_guard_bands_gpu import T

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _fresh_session():
    G.reset()
    yield
    G.reset()


@pytest.mark.parametrize("kind", ["random", "binary"])
def test_resample_between_bands(device, monkeypatch, kind):
    t = T(device, monkeypatch)
    C.check_resample(t.run, t.put, (131, 97), (40, 31), kind)   # rows of 393 and 120 bytes: no row but the first starts on a word


def test_thumbnail_between_bands(device, monkeypatch):
    t = T(device, monkeypatch)
    C.check_thumbnail(t.run, t.put, (403, 297), 100, "random")   # reduce (2, 2) with a ragged edge, then both passes from a float box


def test_single_row_between_bands(device, monkeypatch):
    t = T(device, monkeypatch)
    C.check_thumbnail(t.run, t.put, (999, 1), 100, "binary")    # reduce (4, 1), the horizontal pass straight into the output


def test_zero_fill_gather_between_bands(device, monkeypatch):
    t = T(device, monkeypatch)
    C.check_patches(t.run, t.put, (1000, 200), 256)             # 56 rows of every window lie below the page
    C.check_patches(t.run, t.put, (303, 257), 256)
