"""Guard-band cases (tests/guard_bands.py) of the evaluation kernels (csrc/eval_ops.h) at the shapes of
tests/test_psnr_ssim_gpu.py and tests/test_autoencoder_dataset_gpu.py: operands, results, the SSIM map and the workspace between
0xFF bands, results born NaN.  References and bounds as there."""
import numpy as np
import pytest
import torch

import guard_bands as G
import psnr_ssim_restatement as R
from test_guard_bands_gpu import T

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _fresh_session():
    G.reset()
    yield
    G.reset()


@pytest.mark.parametrize("content", ["noisy", "mixed_range"])   # mixed_range: the minima launch decides per sample
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_psnr_ssim(device, monkeypatch, shape, content):
    import sis_hip
    t = T(device, monkeypatch)
    shape = R.resolve_shape(shape, sis_hip.psnr_ssim_tile())
    x, y = R.case(shape, content)
    ref_psnr, ref_ssim, ref_s = R.reference(shape, content)
    e_map, e_ssim, e_psnr = R.aten_error(shape, content)
    psnr, ssim, smap = t.run(sis_hip.psnr_ssim, t.put(torch.from_numpy(x)), t.put(torch.from_numpy(y)), window=shape[4], return_map=True)
    assert np.abs(smap.double().cpu().numpy() - ref_s).max() <= R.bound(e_map)
    assert np.abs(ssim.double().cpu().numpy() - ref_ssim).max() <= R.bound(e_ssim)
    assert np.abs(psnr.double().cpu().numpy() - ref_psnr).max() <= R.bound(e_psnr)
    psnr2, ssim2 = t.run(sis_hip.psnr_ssim, t.put(torch.from_numpy(x)), t.put(torch.from_numpy(y)), window=shape[4])   # no map
    assert torch.equal(psnr2, psnr) and torch.equal(ssim2, ssim)


@pytest.mark.parametrize("size", [8, 6, 5])   # 5: 25 pixels per plane, the one-pixel-per-thread kernel
def test_autoencoder_batch(device, monkeypatch, size):
    import sis_hip
    t = T(device, monkeypatch)
    rng = np.random.default_rng(size)
    images = rng.integers(0, 256, (7, 3, size, size), dtype=np.uint8)
    ids, scale, per_channel, seed, grey = [6, 0, 6, 3, 1], [50.0, 0.0, 5.0, 25.0, 10.0], [1, 0, 0, 1, 1], [1, 2, 3, 4, 5], [0, 0, 1, 1, 0]
    i32 = lambda v: t.put(torch.tensor(v, dtype=torch.int32))   # noqa: E731
    inp, out = t.run(sis_hip.autoencoder_batch, t.put(torch.from_numpy(images)), i32(ids), t.put(torch.tensor(scale)), i32(per_channel),
                     i32(seed), i32(grey))
    levels, outputs, ambiguous = R.autoencoder_batch(images, ids, scale, per_channel, seed, grey)
    assert torch.equal(out.cpu(), torch.from_numpy(R.encode(outputs)))
    diff = np.abs(R.decode(inp.cpu().numpy()) - levels)
    assert np.all(diff[~ambiguous] == 0) and diff.max() <= 1
