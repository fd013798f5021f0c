"""Guard-band cases (tests/guard_bands.py) of the scanner-margin kernels (csrc/scan_margin.h): the page, the workspace and
every output between 0xFF bands.  Outputs and workspace are born 0xFF here, so every byte that is read has to be written by the
kernels first; the results are compared with the restatement as in tests/test_scan_margin_gpu.py, with and without the edge
image and the contour table."""
import pytest

import guard_bands as G
import scan_margin_checks as C
from test_guard_bands_gpu import T

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _fresh_session():
    G.reset()
    yield
    G.reset()


@pytest.mark.parametrize("outputs", [True, False])
@pytest.mark.parametrize("name", ["scan_97x131_s0", "chain", "random_33x31"])   # ragged tiles; five tiles in a row; dense contours
def test_content_box_between_bands(device, monkeypatch, name, outputs):
    t = T(device, monkeypatch)
    got = C.check_case(t.run, t.put, name, outputs=outputs)
    if outputs:   # the two spare rows of the table are as they were born
        assert bool((got.contours[C.want(name).info[0]:] == -1).all())
