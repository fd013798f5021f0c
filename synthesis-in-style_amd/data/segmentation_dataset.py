"""JSON-listed ``[image | label]`` PNG datasets, resident on the device (reference: data/segmentation_dataset.py:16-107).

The reference decodes one PNG per ``__getitem__`` with PIL, augments it with imgaug and hands single samples to a
``DataLoader``.  Here every PNG is decoded ONCE, at construction: the left halves are kept as uint8 pixels [N, H, W, 3], the
right halves are turned into class maps uint8 [N, H, W] with ``sis_hip.color_to_class``, and both stay in device memory (a 256^2
sample is 256 KB; 90 000 of them are 24 GB).  A batch is then one launch of ``sis_hip.augment_warp`` that gathers its samples by
id (utils/augment_dataset.py).  Above ``max_resident_bytes`` the two arrays stay in pinned host memory and a batch's samples
are uploaded before the warp.

Index arithmetic as the reference's ``AugmentedSegmentationDataset`` (:77-95): ``num_augmentations * N`` indices, an index
below N is the original sample, every other index is an augmented draw of sample ``index % N``.  The augmentation itself is
the one stated in DESIGN.md §12; it is not pinned against imgaug.
"""
import json
import os
from pathlib import Path
from typing import Dict, Optional, Sequence

import numpy
import torch

import sis_hip
from utils.augment_dataset import augment_batch
from utils.segmentation_utils import _rgb, get_class_id_map

IMAGE_SUFFIXES = (".png", ".jpg", ".jpeg", ".bmp", ".tif", ".tiff", ".gif", ".webp")
DEFAULT_MAX_RESIDENT_BYTES = 64 << 30
_CHUNK_BYTES = 256 << 20   # colour halves uploaded per color_to_class launch


def is_image(path) -> bool:
    return str(path).lower().endswith(IMAGE_SUFFIXES)


def default_loader(path):
    from PIL import Image   # host decode, once per file; not imported with the module
    with Image.open(path) as image:
        return image.convert("RGB")


class SegmentationDataset:

    def __init__(self, json_file, root=None, transforms=None, loader=None, class_to_color_map_path: Path = None,
                 background_class_name: str = 'background', image_size: int = None, device=None,
                 max_resident_bytes: int = DEFAULT_MAX_RESIDENT_BYTES, seed: int = 0, load: bool = True):
        # ``transforms`` is accepted for the reference's call sites and unused: Resize / ToTensor / Normalize(0.5, 0.5) are what
        # the warp kernel does
        self.root, self.loader = root, loader if loader is not None else default_loader
        self.background_class_name, self.image_size, self.seed = background_class_name, image_size, seed
        if class_to_color_map_path is None:
            raise ValueError("class_to_color_map_path is required: the label halves are colour images")
        with Path(class_to_color_map_path).open() as f:
            self.class_to_color_map = json.load(f)
        if background_class_name not in self.class_to_color_map:
            raise ValueError(f"the colour map {class_to_color_map_path} has no class '{background_class_name}' (the background)")
        self.class_ids = get_class_id_map(background_class_name, self.class_to_color_map)
        with open(json_file) as f:
            self.load_json_data(json.load(f))
        if load:   # False: only the file list and the index arithmetic (no decode, no device)
            self.device = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
            self._load(max_resident_bytes)

    def load_json_data(self, json_data):
        self.image_data = [entry['file_name'] for entry in json_data if is_image(entry['file_name'])]

    def _load(self, max_resident_bytes: int):
        n = len(self.image_data)
        if n == 0:
            raise ValueError("the dataset lists no images")
        pixels = colours = None
        for i, name in enumerate(self.image_data):
            path = os.path.join(self.root, name) if self.root is not None else name
            image = numpy.asarray(self.loader(path))
            if image.ndim != 3 or image.shape[2] != 3 or image.shape[1] % 2:
                raise ValueError(f"{path}: expected an RGB [image | label] pair of even width, got shape {image.shape}")
            half = image.shape[1] // 2
            if pixels is None:
                self.height, self.width = image.shape[0], half
                pixels = torch.empty((n, self.height, self.width, 3), dtype=torch.uint8, pin_memory=True)
                colours = numpy.empty((n, self.height, self.width, 3), dtype=numpy.uint8)
            if (image.shape[0], half) != (self.height, self.width):
                raise ValueError(f"{path}: sample size {image.shape[0]}x{half} differs from the dataset's "
                                 f"{self.height}x{self.width} ({self.image_data[0]}); all samples must have one size")
            pixels[i] = torch.from_numpy(numpy.ascontiguousarray(image[:, :half]))
            colours[i] = image[:, half:]
        self.resident = n * self.height * self.width * 4 <= max_resident_bytes
        names = [name for name in self.class_to_color_map if name != self.background_class_name]
        table = [_rgb(self.class_to_color_map[name]) for name in names]
        ids = [self.class_ids[name] for name in names]
        classes = torch.empty((n, self.height, self.width), dtype=torch.uint8,
                              device=self.device if self.resident else 'cpu', pin_memory=not self.resident)
        per_chunk = max(1, _CHUNK_BYTES // (self.height * self.width * 3))
        for lo in range(0, n, per_chunk):   # colour -> class is per pixel: a chunk of images is one tall image
            chunk = torch.from_numpy(colours[lo:lo + per_chunk]).to(self.device)
            ids_map = sis_hip.color_to_class(chunk.view(-1, self.width, 3), table, ids,
                                             background_id=self.class_ids[self.background_class_name])
            classes[lo:lo + per_chunk] = ids_map.view(-1, self.height, self.width).to(classes.device)
        self.pixels = pixels.to(self.device) if self.resident else pixels
        self.classes = classes

    def original_length(self) -> int:
        return len(self.image_data)

    def __len__(self) -> int:
        return self.original_length()

    def is_augmented(self, index: int) -> bool:
        return False

    def out_size(self):
        return (self.image_size, self.image_size) if self.image_size is not None else (self.height, self.width)

    def sample_rng(self, index: int, epoch: int = 0, seed: Optional[int] = None) -> numpy.random.Generator:
        """The stream an augmented index draws from: a function of (seed, epoch, index), not of the batch it lands in."""
        return numpy.random.default_rng([self.seed if seed is None else seed, epoch, index])

    def get_batch(self, indices: Sequence[int], epoch: int = 0, seed: Optional[int] = None) -> Dict[str, torch.Tensor]:
        """{"images": float32 [B, 3, S, S], "segmented": int64 [B, 1, S, S]} for dataset indices, on the device."""
        n = self.original_length()
        indices = [int(i) for i in indices]
        if any(not 0 <= i < len(self) for i in indices):
            raise IndexError(f"dataset index outside 0..{len(self) - 1}")
        samples = [i % n for i in indices]
        augment = [self.is_augmented(i) for i in indices]
        rngs = [self.sample_rng(i, epoch, seed) if a else None for i, a in zip(indices, augment)]
        pixels, classes = self.pixels, self.classes
        if not self.resident:
            pick = torch.tensor(samples, dtype=torch.int64)
            pixels = pixels[pick].pin_memory().to(self.device, non_blocking=True)
            classes = classes[pick].pin_memory().to(self.device, non_blocking=True)
            samples = list(range(len(indices)))
        return augment_batch(pixels, classes, samples, rngs, out_size=self.out_size(), augment=augment,
                             background_id=self.class_ids[self.background_class_name])

    def __getitem__(self, index: int) -> Dict[str, torch.Tensor]:
        batch = self.get_batch([index])
        return {"images": batch["images"][0], "segmented": batch["segmented"][0]}


class AugmentedSegmentationDataset(SegmentationDataset):
    """``num_augmentations * N`` indices over N files: one pass yields every original once (indices below N) and
    ``num_augmentations - 1`` augmented draws of each file (index ``i`` draws from file ``i % N``)."""

    def __init__(self, *args, num_augmentations, **kwargs):
        if isinstance(num_augmentations, bool) or not isinstance(num_augmentations, int) or num_augmentations < 1:
            raise TypeError(f"num_augmentations must be a positive int, got {num_augmentations!r}")
        self.num_augmentations = num_augmentations
        super().__init__(*args, **kwargs)

    def __len__(self) -> int:
        return self.num_augmentations * self.original_length()

    def is_augmented(self, index: int) -> bool:
        return index // self.original_length() != 0
