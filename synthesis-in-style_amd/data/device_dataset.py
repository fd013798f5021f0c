"""Tensor hand-off from synthesis to segmentation training.

The reference writes every synthetic sample as a side-by-side ``[image | label]`` PNG
(create_dataset_for_segmentation.py:84-99) and ``SegmentationDataset.__getitem__``
(data/segmentation_dataset.py:44-63) splits it again: left half -> ``ToTensor`` + ``Normalize(0.5, 0.5)``
(u8 / 255, then (x - 0.5) / 0.5), right half -> colours -> class ids -> nearest-neighbour resize to ``image_size`` ->
int64 ``[1, S, S]``.  PNG is lossless, so the batch the trainer sees is a pure function of the uint8 pixels and the
label map that ``utils.dataset_creation.label_and_encode`` leaves ON THE DEVICE.  ``encode_batch`` is that function
(same arithmetic, same order, bit for bit -- tests/test_dataset_ops_gpu.py round-trips a PNG through PIL against it)
and ``SynthesisSegmentationLoader`` feeds an updater straight from a generator: no PNG, no PIL, no host copy.

``DeviceSegmentationLoader`` is the loader of the written dataset: batches of a device-resident ``SegmentationDataset`` /
``AugmentedSegmentationDataset`` (data/segmentation_dataset.py), one ``sis_hip.augment_warp`` launch each, in the place of the
reference's ``DataLoader`` + ``DistributedSampler`` (utils/data_loading.py:52-75).
"""
from typing import Dict, Iterator, List, Optional

import numpy
import torch
import torch.nn.functional as F

from utils.dataset_creation import label_and_encode


def encode_batch(pixels: torch.Tensor, labels: torch.Tensor, class_of_cluster: Optional[torch.Tensor] = None,
                 image_size: Optional[int] = None) -> Dict[str, torch.Tensor]:
    """pixels uint8 [B,H,W,3] (``make_image``), labels int64 [B,h,w] cluster ids -> the reference loaders' batch contract
    (``images`` float32 [B,3,H,W] in [-1,1], ``segmented`` int64 [B,1,S,S]).  ``class_of_cluster`` [K] maps cluster ids to
    class ids (the reference's cluster -> class merge + colour map, applied as a lookup); ``image_size`` resizes the label
    map with nearest neighbours exactly as ``class_image_to_tensor`` does (segmentation_dataset.py:37-42)."""
    # divisors as tensors: ATen turns a division by a Python scalar into a multiplication by its reciprocal on the device,
    # which is one ulp off the true division ToTensor performs on the host for some of the 256 byte values
    d255 = torch.full((), 255.0, dtype=torch.float32, device=pixels.device)
    images = pixels.permute(0, 3, 1, 2).to(torch.float32).div(d255).sub(0.5).div(0.5).contiguous()
    classes = labels if class_of_cluster is None else class_of_cluster.to(labels.device)[labels]
    classes = classes.unsqueeze(1)
    size = image_size if image_size is not None else images.shape[-1]
    if classes.shape[-1] != size or classes.shape[-2] != size:
        classes = F.interpolate(classes.to(torch.float32), (size, size)).to(torch.int64)  # default mode: nearest
    return {"images": images, "segmented": classes.to(torch.int64)}


class SynthesisSegmentationLoader:
    """Endless iterable of training batches synthesised on the fly: seeded latents (CPU RNG stream of
    utils/dataset_creation.py:32-37) -> ``Generator.forward`` with activations -> k-means label map of ``label_layer`` +
    uint8 pixels on the side stream -> ``encode_batch``.  Everything after the latents stays in HBM."""

    def __init__(self, generator, catalogs: Dict, label_layer: int, batch_size: int, class_of_cluster=None,
                 image_size: Optional[int] = None, seed: int = 1, truncation_latent=None, num_batches: Optional[int] = None,
                 num_augmentations: Optional[int] = None):
        self.generator, self.catalogs, self.label_layer = generator, catalogs, label_layer
        self.batch_size, self.class_of_cluster, self.image_size = batch_size, class_of_cluster, image_size
        self.seed, self.truncation_latent, self.num_batches = seed, truncation_latent, num_batches
        # the reference trains on ``num_augmentations * N`` indices of which N are originals (segmentation_dataset.py:77-95):
        # a slot stays unaugmented with probability 1 / num_augmentations.  None: no augmentation, the batches of before.
        # Every slot of an augmenting loader goes through the warp, whose resize to ``image_size`` is bilinear for the image and
        # pixel-centre nearest for the labels: its unaugmented slots equal the plain loader's only when ``image_size`` is the
        # generator's size (the plain loader never resizes the image and resizes labels with F.interpolate's nearest).
        self.num_augmentations = num_augmentations

    def __len__(self):
        return self.num_batches if self.num_batches is not None else 1 << 30

    def __iter__(self) -> Iterator[Dict[str, torch.Tensor]]:
        g = self.generator
        device = g.input.input.device
        rng = torch.Generator().manual_seed(self.seed)
        augment_rng = numpy.random.default_rng([self.seed, 0x617567]) if self.num_augmentations is not None else None
        i = 0
        while self.num_batches is None or i < self.num_batches:
            z = torch.randn(self.batch_size, g.style_dim, generator=rng).to(device, non_blocking=True)
            with torch.no_grad():
                image, acts = g([z], noise=g.make_noise(), return_intermediate_activations=True,
                                truncation=0.7 if self.truncation_latent is not None else 1,
                                truncation_latent=self.truncation_latent)
                pixels, labels, ready = label_and_encode(image, {self.label_layer: acts[self.label_layer]},
                                                         {self.label_layer: self.catalogs[self.label_layer]})
                if ready is not None:
                    torch.cuda.current_stream(device).wait_event(ready)
                if augment_rng is None:
                    batch = encode_batch(pixels, labels[self.label_layer], self.class_of_cluster, self.image_size)
                else:
                    batch = self._augmented(pixels, labels[self.label_layer], augment_rng)
            # yielded OUTSIDE the no_grad block: a generator suspended inside it would leave grad mode off in the consumer
            # (the updater keeps this iterator alive across its forward / backward)
            yield batch
            i += 1

    def _augmented(self, pixels, labels, rng):
        from utils.augment_dataset import augment_batch
        classes = labels if self.class_of_cluster is None else self.class_of_cluster.to(labels.device)[labels]
        if tuple(classes.shape[-2:]) != tuple(pixels.shape[1:3]):   # the label layer's resolution -> the image's, nearest
            classes = F.interpolate(classes.unsqueeze(1).to(torch.float32), tuple(pixels.shape[1:3])).squeeze(1)
        keep = rng.random(self.batch_size) < 1.0 / self.num_augmentations
        return augment_batch(pixels.contiguous(), classes.to(torch.uint8).contiguous(), list(range(self.batch_size)), rng,
                             out_size=self.image_size, augment=[not k for k in keep])


def epoch_indices(length: int, epoch: int, shuffle: bool, seed: int, rank: int = 0, world_size: int = 1) -> List[int]:
    """The dataset indices of one rank in one epoch, as ``DistributedSampler`` deals them: a permutation seeded by (seed, epoch)
    -- the same on every rank --, padded from its own start to a multiple of the world size, split by stride."""
    order = numpy.random.default_rng([seed, epoch]).permutation(length) if shuffle else numpy.arange(length)
    total = -(-length // world_size) * world_size
    order = numpy.resize(order, total)   # repeats from the start, as the sampler's padding
    return [int(i) for i in order[rank:total:world_size]]


class DeviceSegmentationLoader:
    """Iterable of {"images", "segmented"} batches of a device-resident dataset; one pass is one epoch, and every new pass
    takes the next epoch's permutation and augmentation draws."""

    def __init__(self, dataset, batch_size: int, shuffle: bool = True, drop_last: bool = True, rank: int = 0, world_size: int = 1,
                 seed: int = 0):
        if not 0 <= rank < world_size:
            raise ValueError(f"rank {rank} outside 0..{world_size - 1}")
        self.dataset, self.batch_size, self.shuffle, self.drop_last = dataset, batch_size, shuffle, drop_last
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
            with torch.no_grad():
                batch = self.dataset.get_batch(chunk, epoch=epoch, seed=self.seed)
            # yielded OUTSIDE the no_grad block, as SynthesisSegmentationLoader does and for the same reason
            yield batch
