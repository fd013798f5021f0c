"""JSON-listed training images of the GAN, resident on the device (reference: ``build_data_loader(config['images'], config,
False, dataset_class=JSONDataset, loader_func=resilient_loader)``, train_stylegan_2.py:42-50 with utils/data_loading.py:27-76).

The reference decodes one file per ``__getitem__`` in ``num_workers`` processes: PIL decode -> ``transforms.Resize((S, S))`` ->
``ToTensor`` -> ``Normalize(0.5, 0.5)`` -> ``{'image': tensor}``, collated by a ``DataLoader``.  Here every file is decoded ONCE, at
construction, resized on the host where its size is not ``S x S`` (``PIL.Image.resize((S, S), BILINEAR)`` -- what
``transforms.Resize`` does to a PIL image) and kept as uint8 ``[N, 3, S, S]`` in device memory (a 256^2 image is 192 KB; 100 000
of them are 19 GB).  A batch is one launch of ``sis_hip.gan_image_batch``, which gathers the listed samples and applies the two
normalisations with the reference's arithmetic, bit for bit.  Above ``max_resident_bytes`` the array stays in pinned host memory
and a batch's samples are uploaded before the launch.

The JSON is the list ``scripts/create_stylegan_train_dataset.py`` of the reference writes: image paths relative to the JSON's
directory.  An unreadable file becomes the reference's black image with one printed warning (``resilient_loader``).
"""
import json
import os
from typing import Dict, Iterator, List, Optional, Sequence

import numpy
import torch

import sis_hip
from data.device_dataset import epoch_indices
from data.segmentation_dataset import DEFAULT_MAX_RESIDENT_BYTES, default_loader


def resilient_loader(path):
    """utils/data_loading.py:27-32 of the reference: a file that cannot be decoded is a black 256 x 256 image, not an error."""
    try:
        return default_loader(path)
    except Exception as e:
        from PIL import Image
        print(f"Could not load {path} with exception: {e}", flush=True)
        return Image.new('RGB', (256, 256))


def to_chw_u8(image, size: int) -> numpy.ndarray:
    """PIL RGB image -> uint8 [3, size, size]; other sizes are resized as ``transforms.Resize((size, size))`` resizes a PIL image."""
    from PIL import Image
    if image.size != (size, size):
        image = image.resize((size, size), Image.BILINEAR)
    return numpy.ascontiguousarray(numpy.asarray(image, dtype=numpy.uint8).transpose(2, 0, 1))


class DeviceImageDataset:

    def __init__(self, json_file, image_size: int, input_dim: int = 3, root=None, loader=None, device=None,
                 max_resident_bytes: int = DEFAULT_MAX_RESIDENT_BYTES, load: bool = True):
        if int(input_dim) != 3:
            raise ValueError(f"input_dim {input_dim}: the image loader decodes RGB (3 channels) only")
        self.image_size = int(image_size)
        self.root = os.path.dirname(os.path.abspath(json_file)) if root is None else root
        self.loader = loader if loader is not None else resilient_loader
        with open(json_file) as f:
            self.image_data = [str(name) for name in json.load(f)]
        if not self.image_data:
            raise ValueError(f"{json_file} lists no images")
        if load:   # False: only the file list (no decode, no device)
            self.device = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
            self._load(max_resident_bytes)

    def _load(self, max_resident_bytes: int):
        n, s = len(self.image_data), self.image_size
        pixels = torch.empty((n, 3, s, s), dtype=torch.uint8, pin_memory=self.device.type == 'cuda')
        for i, name in enumerate(self.image_data):
            pixels[i] = torch.from_numpy(to_chw_u8(self.loader(os.path.join(self.root, name)), s))
        self.resident = pixels.numel() <= max_resident_bytes
        self.pixels = pixels.to(self.device) if self.resident else pixels

    def __len__(self) -> int:
        return len(self.image_data)

    def get_batch(self, indices: Sequence[int]) -> Dict[str, torch.Tensor]:
        """{'image': float32 [B, 3, S, S] in [-1, 1]} for dataset indices, on the device: one ``sis_gan_image_batch`` launch."""
        indices = [int(i) for i in indices]
        if not indices or any(not 0 <= i < len(self) for i in indices):
            raise IndexError(f"dataset index outside 0..{len(self) - 1}")
        pixels = self.pixels
        if not self.resident:
            pixels = pixels[torch.tensor(indices, dtype=torch.int64)].pin_memory().to(self.device, non_blocking=True)
            indices = list(range(len(indices)))
        ids = torch.tensor(indices, dtype=torch.int32).to(self.device, non_blocking=True)
        return {'image': sis_hip.gan_image_batch(pixels, ids)}

    def __getitem__(self, index: int) -> Dict[str, torch.Tensor]:
        return {'image': self.get_batch([index])['image'][0]}


class DeviceImageLoader:
    """Iterable of ``{'image'}`` batches of a ``DeviceImageDataset``; one pass is one epoch, and every new pass takes the next
    epoch's permutation (``data.device_dataset.epoch_indices``: seeded, the same on every rank, split by stride)."""

    def __init__(self, dataset, batch_size: int, shuffle: bool = True, drop_last: bool = True, rank: int = 0, world_size: int = 1,
                 seed: int = 0):
        if not 0 <= rank < world_size:
            raise ValueError(f"rank {rank} outside 0..{world_size - 1}")
        self.dataset, self.batch_size, self.shuffle, self.drop_last = dataset, int(batch_size), shuffle, drop_last
        self.rank, self.world_size, self.seed, self.epoch = rank, world_size, seed, 0

    def set_epoch(self, epoch: int):
        self.epoch = epoch

    def indices(self, epoch: Optional[int] = None) -> List[int]:
        return epoch_indices(len(self.dataset), self.epoch if epoch is None else epoch, self.shuffle, self.seed, self.rank,
                             self.world_size)

    def __len__(self):
        per_rank = -(-len(self.dataset) // self.world_size)
        return per_rank // self.batch_size if self.drop_last else -(-per_rank // self.batch_size)

    def __iter__(self) -> Iterator[Dict[str, torch.Tensor]]:
        epoch, self.epoch = self.epoch, self.epoch + 1
        order = self.indices(epoch)
        for lo in range(0, len(order), self.batch_size):
            chunk = order[lo:lo + self.batch_size]
            if len(chunk) < self.batch_size and self.drop_last:
                break
            yield self.dataset.get_batch(chunk)
