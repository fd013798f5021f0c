"""The autoencoder's datasets, resident on the device (reference: data/autoencoder_dataset.py).

The reference decodes a file per ``__getitem__``, adds imgaug's ``AdditiveGaussianNoise`` on the host, converts to grey through
PIL where asked, and runs the torchvision transforms twice (input and output).  Here the files are decoded once
(``DeviceImageDataset``) and a batch is ONE launch of ``sis_hip.autoencoder_batch``: gather, noise, grey conversion, ToTensor +
Normalize(0.5, 0.5) of both ``input_image`` and ``output_image``.  Following DESIGN.md §12's rule the random CHOICES are drawn on
the host and applied on the device: per sample the noise scale (uniformly one of ``DENOISING_VARIANCES``, as imgaug samples a
list parameter), the per-channel bit (p = 1/2: the reference's ``OneOf`` of a shared-noise and a per-channel augmenter) and a
32-bit seed for the kernel's counter-hash normal generator, all from one ``numpy.random.Generator`` seeded by ``noise_seed``.

Not reproduced: imgaug's own noise stream (its global ``imgaug.seed(666)``), and the order of resize and noise for files whose
size is not ``image_size`` -- the reference adds noise to the file's pixels and resizes afterwards, here the resident pixels are
already resized.  For files of the training size the two agree in distribution.
"""
from typing import Dict, Sequence

import numpy
import torch

import sis_hip
from data.gan_image_dataset import DeviceImageDataset, resilient_loader

DENOISING_VARIANCES = [5, 10, 15, 25, 35, 50]


class AutoencoderDataset(DeviceImageDataset):
    """{'input_image', 'output_image'}: the image twice (noise scale 0)."""

    grey = 0

    def __init__(self, *args, noise_seed: int = 666, **kwargs):
        super().__init__(*args, **kwargs)
        self.noise_rng = numpy.random.Generator(numpy.random.PCG64(noise_seed))

    def draw_noise(self, batch: int) -> numpy.ndarray:
        """int32 [3, batch]: the bits of the float32 scale, the per-channel flag, the seed word."""
        return numpy.zeros((3, batch), dtype=numpy.int32)

    def get_batch(self, indices: Sequence[int]) -> Dict[str, torch.Tensor]:
        indices = [int(i) for i in indices]
        if not indices or any(not 0 <= i < len(self) for i in indices):
            raise IndexError(f"dataset index outside 0..{len(self) - 1}")
        pixels = self.pixels
        if not self.resident:
            pixels = pixels[torch.tensor(indices, dtype=torch.int64)].pin_memory().to(self.device, non_blocking=True)
            indices = list(range(len(indices)))
        batch = len(indices)
        # one upload: ids, scale bits, per-channel flags, seed words, grey flags
        host = numpy.empty((5, batch), dtype=numpy.int32)
        host[0] = indices
        host[1:4] = self.draw_noise(batch)
        host[4] = self.grey
        params = torch.from_numpy(host).to(self.device, non_blocking=True)
        input_image, output_image = sis_hip.autoencoder_batch(pixels, params[0], params[1].view(torch.float32), params[2], params[3], params[4])
        return {'input_image': input_image, 'output_image': output_image}

    def __getitem__(self, index: int) -> Dict[str, torch.Tensor]:
        return {key: value[0] for key, value in self.get_batch([index]).items()}


class DenoisingAutoencoderDataset(AutoencoderDataset):

    def draw_noise(self, batch: int) -> numpy.ndarray:
        rng = self.noise_rng
        scale = rng.choice(numpy.asarray(DENOISING_VARIANCES, dtype=numpy.float32), size=batch)
        per_channel = rng.integers(0, 2, size=batch, dtype=numpy.int32)
        seed = rng.integers(0, 1 << 32, size=batch, dtype=numpy.uint32)
        return numpy.stack([scale.astype(numpy.float32).view(numpy.int32), per_channel, seed.view(numpy.int32)])


class BlackAndWhiteDenoisingAutoencoderDataset(DenoisingAutoencoderDataset):
    """Grey images: converted once at load through PIL, and again after the noise by the kernel."""

    grey = 1

    def __init__(self, *args, **kwargs):
        loader = kwargs.get('loader') or resilient_loader
        kwargs['loader'] = lambda path: loader(path).convert('L').convert('RGB')
        super().__init__(*args, **kwargs)

