"""``sis_hip.autoencoder_batch`` (csrc/eval_ops.h) against the numpy restatement of DESIGN.md §15, and the three datasets of
data/autoencoder_dataset.py.

The noisy levels are compared exactly wherever the restatement's value before rounding is farther than 2^-8 from a half-integer
and within one level elsewhere: the fp32 logf, sqrtf and cospif of the kernel put scale * z within about 3e-4 of the float64
value (|z| <= 5.8, scale <= 50, a few ulp of 290 plus the rounding of the sum, half an ulp of 512), well inside 2^-8.
tests/test_psnr_ssim_cpu.py checks that at most 2 % of the pixels of every case are left out that way."""
import json

import numpy as np
import pytest
import torch

import psnr_ssim_restatement as R

pytestmark = pytest.mark.gpu


def _params(device, scale, per_channel, seed, grey):
    as_i32 = lambda v: torch.from_numpy(np.asarray(v, dtype=np.uint32).view(np.int32).copy()).to(device)   # noqa: E731
    return (torch.tensor(scale, dtype=torch.float32, device=device), as_i32(per_channel), as_i32(seed), as_i32(grey))


def _batch(device, images, ids, scale, per_channel, seed, grey):
    import sis_hip
    return sis_hip.autoencoder_batch(torch.from_numpy(images).to(device), torch.tensor(ids, dtype=torch.int32, device=device),
                                     *_params(device, scale, per_channel, seed, grey))


@pytest.mark.parametrize("size", R.NOISE_SIZES)   # 5: 25 pixels per plane, the one-pixel-per-thread kernel
def test_output_and_zero_scale(device, size):
    import sis_hip
    images = R.noise_images(size)
    ids = torch.tensor(R.NOISE_IDS, dtype=torch.int32, device=device)
    plain = sis_hip.gan_image_batch(torch.from_numpy(images).to(device), ids)
    for grey in (0, 1):
        inp, out = _batch(device, images, R.NOISE_IDS, [25.0, 0.0, 50.0], [1, 1, 0], [11, 12, 13], [grey] * 3)
        assert torch.equal(out, plain)
    inp, out = _batch(device, images, R.NOISE_IDS, [0.0] * 3, [1, 0, 1], [21, 22, 23], [0] * 3)
    assert torch.equal(inp, out) and torch.equal(out, plain)
    assert torch.equal(out.cpu(), torch.from_numpy(R.encode(images[R.NOISE_IDS])))


@pytest.mark.parametrize("size,per_channel,grey,scales,seeds", R.noise_cases())
def test_noisy_input_against_the_restatement(device, size, per_channel, grey, scales, seeds):
    images = R.noise_images(size)
    levels, _, ambiguous = R.autoencoder_batch(images, R.NOISE_IDS, scales, [per_channel] * 3, seeds, [grey] * 3)
    inp, _ = _batch(device, images, R.NOISE_IDS, list(scales), [per_channel] * 3, list(seeds), [grey] * 3)
    got = R.decode(inp.cpu().numpy())
    assert torch.equal(inp.cpu(), torch.from_numpy(R.encode(got)))   # every value is the encoding of a level
    diff = np.abs(got - levels)
    print(f"autoencoder_batch S={size} per_channel={per_channel} grey={grey} scales={scales}: {int((diff != 0).sum())} of {diff.size} "
          f"levels differ, {int(ambiguous.sum())} near a rounding boundary")
    assert ambiguous.mean() <= 0.02
    assert np.all(diff[~ambiguous] == 0) and diff.max() <= 1
    if grey:
        assert np.array_equal(got[:, 0], got[:, 1]) and np.array_equal(got[:, 0], got[:, 2])
    if size == 8 and not grey:
        assert got[0].min() == 0 and got[0].max() == 255   # image 3's plateaux: the clip


def test_an_id_outside_the_list_yields_nan(device):
    images = R.noise_images(8)
    inp, out = _batch(device, images, [1, 4, -1], [5.0] * 3, [0] * 3, [1, 2, 3], [0] * 3)
    assert torch.isfinite(inp[0]).all() and torch.isfinite(out[0]).all()
    assert torch.isnan(inp[1:]).all() and torch.isnan(out[1:]).all()


def test_noise_statistics(device):
    """Mid-grey 64 x 64 at scale 50: the 12288 recovered z have |mean| <= 4 / sqrt(n) and |var - 1| <= 4 sqrt(2 / n) (four standard
    errors of a standard normal sample; the levels' rounding adds 3e-5 to the variance and the clip at |z| > 2.54 takes 0.02 of
    the bound's 0.051 away); without per_channel the three channels are equal."""
    images = np.full((1, 3, 64, 64), 128, dtype=np.uint8)
    inp, _ = _batch(device, images, [0, 0], [50.0, 50.0], [1, 0], [R.STATISTICS_SEED, R.STATISTICS_SEED], [0, 0])
    levels = R.decode(inp.cpu().numpy())
    z = (levels[0] - 128) / 50.0
    n = z.size
    print(f"noise statistics: n {n} mean {z.mean():+.4f} (bound {4 / np.sqrt(n):.4f}) var {z.var():.4f} (bound 1 +- {4 * np.sqrt(2 / n):.4f})")
    assert n == 12288 and abs(z.mean()) <= 4 / np.sqrt(n) and abs(z.var() - 1) <= 4 * np.sqrt(2 / n)
    assert not np.array_equal(levels[0, 0], levels[0, 1])
    assert np.array_equal(levels[1, 0], levels[1, 1]) and np.array_equal(levels[1, 0], levels[1, 2])
    assert np.array_equal(levels[1, 0], levels[0, 0])   # the shared z is channel 0's


# ------------------------------------------------------------------------------------------------------------- datasets

@pytest.fixture(scope="module")
def image_list(tmp_path_factory):
    from PIL import Image
    root = tmp_path_factory.mktemp("autoencoder_images")
    rng = np.random.default_rng(23)
    names = []
    for i in range(5):
        names.append(f"{i}.png")
        Image.fromarray(rng.integers(0, 256, (16, 16, 3), dtype=np.uint8)).save(root / names[-1])
    (root / "images.json").write_text(json.dumps(names))
    return str(root / "images.json")


def test_the_three_dataset_classes(device, image_list):
    from data.autoencoder_dataset import AutoencoderDataset, BlackAndWhiteDenoisingAutoencoderDataset, DenoisingAutoencoderDataset
    from data.gan_image_dataset import DeviceImageDataset, DeviceImageLoader
    plain_images = DeviceImageDataset(image_list, 16, device=device).get_batch([4, 0, 4])['image']
    for cls in (AutoencoderDataset, DenoisingAutoencoderDataset, BlackAndWhiteDenoisingAutoencoderDataset):
        first, again, other = (cls(image_list, 16, device=device, noise_seed=s) for s in (5, 5, 6))
        batches = [d.get_batch([4, 0, 4]) for d in (first, again, other)]
        batches.append(first.get_batch([4, 0, 4]))   # the next draw of the same dataset
        for batch in batches:
            assert set(batch) == {'input_image', 'output_image'}
            for t in batch.values():
                assert t.shape == (3, 3, 16, 16) and t.dtype == torch.float32 and t.device == device
                assert t.min() >= -1 and t.max() <= 1
        assert all(torch.equal(batches[0][k], batches[1][k]) for k in batches[0])   # the same noise_seed, the same batches
        if cls is AutoencoderDataset:
            assert torch.equal(batches[0]['input_image'], batches[0]['output_image'])
            assert torch.equal(batches[0]['output_image'], plain_images)
        else:
            assert not torch.equal(batches[0]['input_image'], batches[0]['output_image'])
            assert not torch.equal(batches[0]['input_image'], batches[2]['input_image'])
            assert not torch.equal(batches[0]['input_image'], batches[3]['input_image'])
            assert torch.equal(batches[0]['output_image'], batches[2]['output_image'])
        if cls is BlackAndWhiteDenoisingAutoencoderDataset:
            for t in batches[0].values():
                assert torch.equal(t[:, 0], t[:, 1]) and torch.equal(t[:, 0], t[:, 2])
        elif cls is DenoisingAutoencoderDataset:
            assert torch.equal(batches[0]['output_image'], plain_images)
        item = first[2]
        assert set(item) == {'input_image', 'output_image'} and item['output_image'].shape == (3, 16, 16)
    loader = DeviceImageLoader(DenoisingAutoencoderDataset(image_list, 16, device=device), 2, shuffle=False, drop_last=False)
    assert [len(b['input_image']) for b in loader] == [2, 2, 1]
