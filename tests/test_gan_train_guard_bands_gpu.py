"""Guard-band cases (tests/guard_bands.py) of the GAN-training kernels (csrc/gan_train_ops.h) at the shapes of
tests/test_train_stylegan2_gpu.py: operands and results between 0xFF bands, results born NaN.  References and bounds as there."""
import math

import pytest
import torch
import torch.nn.functional as F

import gan_train_checks as C
import guard_bands as G
from test_guard_bands_gpu import T, _mk

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _fresh_session():
    G.reset()
    yield
    G.reset()


@pytest.mark.parametrize("size", [8, 6, 5])   # 5: 75 bytes per sample, the one-element-per-thread kernel
def test_gan_image_batch(device, monkeypatch, size):
    import sis_hip
    t = T(device, monkeypatch)
    gen = torch.Generator().manual_seed(size)
    images = torch.randint(0, 256, (7, 3, size, size), generator=gen, dtype=torch.uint8)
    ids = torch.tensor([6, 0, 6, 3, 1], dtype=torch.int32)   # the last sample of the list, twice
    out = t.run(sis_hip.gan_image_batch, t.put(images), t.put(ids))
    assert torch.equal(out.cpu(), C.ref_image_batch(images, ids))


@pytest.mark.parametrize("shape", [(2, 8, 8, 8), (1, 3, 6, 10), (3, 24, 4, 8)])
def test_phase_split_and_merge(device, monkeypatch, shape):
    import sis_hip
    t = T(device, monkeypatch)
    gen = torch.Generator().manual_seed(sum(shape))
    x = _mk(gen, *shape)
    split = t.run(sis_hip.phase_split, t.put(x))
    assert torch.equal(split.cpu(), F.pixel_unshuffle(x, 2))
    p = _mk(gen, *split.shape)
    merged = t.run(sis_hip.phase_merge, t.put(p))
    assert torch.equal(merged.cpu(), F.pixel_shuffle(p, 2))


@pytest.mark.parametrize("cout,cin", [(16, 8), (5, 3), (64, 300)])   # (5, 3): 15 pairs, a partial workgroup; (64, 300): 75 workgroups
def test_compose_and_adjoint(device, monkeypatch, cout, cin):
    import sis_hip
    t = T(device, monkeypatch)
    gen = torch.Generator().manual_seed(cout + cin)
    w, g = _mk(gen, cout, cin, 3, 3), _mk(gen, cout, 4 * cin, 3, 3)
    fir, scale = C.fir_taps(dtype=torch.float32), 1 / math.sqrt(cin * 9)
    composed = t.run(sis_hip.down_weight_compose, t.put(w), t.put(fir), scale)
    ref = C.ref_compose(w, fir, scale)
    assert C.max_abs(composed, ref) <= 1e-6 * ref.abs().max().item()
    adjoint = t.run(sis_hip.down_weight_compose_adjoint, t.put(g), t.put(fir), scale)
    ref = C.ref_compose_adjoint(g, fir, scale)
    assert C.max_abs(adjoint, ref) <= 1e-6 * ref.abs().max().item()
