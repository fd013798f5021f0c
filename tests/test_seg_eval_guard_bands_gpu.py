"""Guard-band cases (tests/guard_bands.py) of the validation pass (csrc/seg_eval.h, included by seg_ops.hip): logits, labels, the
workspace, ``counts`` and ``sums`` between 0xFF bands, on both routes, at the unaligned 3 x 5 x 7 shape (35 pixels per image:
element loads, a last lane with three pixels, label rows off 16-byte alignment) and at 2 x 4 x 4 (16-byte loads that end at the
last byte before the band).  The workspace is born NaN: a row of partial sums the kernel did not write would reach ``sums``.
Reference and bounds as in tests/test_seg_eval_gpu.py."""
import numpy as np
import pytest
import torch

import guard_bands as G
import seg_eval_restatement as R
from test_guard_bands_gpu import T
from test_seg_eval_gpu import N_THREAD, TORCH_DTYPE

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _fresh_session():
    G.reset()
    yield
    G.reset()


def _guarded(device, monkeypatch, logits, labels, dtype, size, own_state):
    import sis_hip
    t = T(device, monkeypatch)
    classes = logits.shape[1]
    x = t.put(torch.from_numpy(logits).to(TORCH_DTYPE[dtype]))
    lab = t.put(torch.from_numpy(labels))
    state = {}
    if own_state:   # the caller's state, accumulated into: banded as an in-place operand
        state = dict(counts=t.put(torch.zeros(classes * classes + 2, dtype=torch.int64), inplace=True),
                     sums=t.put(torch.zeros(1 + 3 * classes, dtype=torch.float64), inplace=True))
    counts, sums = t.run(sis_hip.seg_eval, x, lab, size=size, **state)
    ref = R.reference(logits, labels, size)
    R.check_counts(counts.cpu().numpy(), ref, labels, exact=True)
    sums = sums.cpu().numpy()
    assert np.isfinite(sums).all() and (np.abs(sums - ref.sums) <= R.sums_bound(ref, N_THREAD)).all()


@pytest.mark.parametrize("own_state", [False, True], ids=["fresh", "accumulate"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("shape", [(3, 5, 7), (2, 4, 4)], ids=["3x5x7", "2x4x4"])
def test_full_resolution(device, monkeypatch, shape, dtype, own_state):
    rng = np.random.default_rng(1)
    logits = R.tie_logits(rng, (shape[0], 5) + shape[1:])
    _guarded(device, monkeypatch, logits, R.labels_with_ignored(rng, shape, 5), dtype, None, own_state)


@pytest.mark.parametrize("own_state", [False, True], ids=["fresh", "accumulate"])
@pytest.mark.parametrize("low,shape", [((3, 4), (3, 5, 7)), ((3, 4), (2, 5, 4))], ids=["3x4-5x7", "3x4-5x4"])
def test_low_resolution(device, monkeypatch, low, shape, own_state):
    """Scales 1/2 (3 -> 5, 4 -> 7) and 1 (4 -> 4): small integers interpolate exactly.  5 x 4 = 20 pixels per image: the label
    quads are 16-byte loads, the logits come from the 2 x 2 neighbourhoods of a 3 x 4 plane whose last row and column are clamped."""
    rng = np.random.default_rng(2)
    logits = R.tie_logits(rng, (shape[0], 4) + low)
    _guarded(device, monkeypatch, logits, R.labels_with_ignored(rng, shape, 4), "f32", shape[1:], own_state)
