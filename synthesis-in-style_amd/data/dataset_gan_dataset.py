"""``scale_activations`` of the reference (data/dataset_gan_dataset.py:12-34): the [B, S, S, F] per-pixel feature tensor of
DatasetGAN.  Kept for API completeness and as the formulation the fused label pass is checked and timed against; the dataset
loop never builds this tensor (segmentation/dataset_gan_segmenter.py).  Differences: the tensor is allocated on the
activations' device (the reference hard-codes 'cuda', :22) and no singleton axis is squeezed (the reference's ``squeeze()``,
:26, also dropped the batch axis of a batch of one)."""
from typing import Dict, List

import torch
from torch.nn import Upsample


def scale_activations(activations: List[Dict[int, torch.Tensor]], upsamplers: List[Upsample]) -> List[torch.Tensor]:
    scaled_activations = []
    for entry_activation in activations:
        assert len(entry_activation) == len(upsamplers), \
            f"uneven size of activations {len(entry_activation)} to upsamplers {len(upsamplers)}"

        first = next(iter(entry_activation.values()))
        batch_size = first.shape[0]
        image_size = entry_activation[0].shape[2] * int(upsamplers[0].scale_factor)
        feature_size = sum([e.shape[1] for e in entry_activation.values()])

        image_activations = torch.empty((batch_size, image_size, image_size, feature_size), device=first.device)

        feature_index = 0
        for idx, activation in entry_activation.items():
            upscaled_feature_maps = upsamplers[idx](activation)
            new_index = feature_index + upscaled_feature_maps.shape[1]
            image_activations[:, :, :, feature_index:new_index] = torch.moveaxis(upscaled_feature_maps, 1, -1)
            feature_index = new_index

        scaled_activations.append(image_activations)
    return scaled_activations


# ---------------------------------------------------------------------------------------------------- training input
import json   # noqa: E402
from pathlib import Path   # noqa: E402
from typing import Optional, Sequence, Union   # noqa: E402

import numpy   # noqa: E402


def class_image_on_host(image: numpy.ndarray, background_class_name: str, class_to_color_map: dict) -> numpy.ndarray:
    """``utils.segmentation_utils.segmentation_image_to_class_image`` for a dataset kept on CPU tensors (the rehearsal path):
    the same rule -- unknown colours are background, of two classes with one colour the later one wins."""
    from utils.segmentation_utils import _rgb, get_class_id_map
    ids = get_class_id_map(background_class_name, class_to_color_map)
    out = numpy.full(image.shape[:2], ids[background_class_name], dtype=numpy.uint8)
    for name, colour in class_to_color_map.items():
        if name != background_class_name:
            out[(image[..., :3] == numpy.asarray(_rgb(colour), dtype=image.dtype)).all(-1)] = ids[name]
    return out


class DeviceDatasetGANDataset:
    """The reference's ``DatasetGANDataset`` / ``DatasetGANGenerationDataset`` (data/base_dataset_gan_dataset.py,
    data/dataset_gan_dataset.py, data/dataset_gan_generation_dataset.py) without the feature tensor.

    Reads the reference's files: a JSON list of ``{image, label, activations | latent}`` (paths relative to the directory of
    ``tensor_path``), ``tensors.npz`` with ``activations`` (a pickled list of ``{layer: [C, r, r]}``) and ``latent_codes``, and
    colour label PNGs.  Kept resident on ``device``: the raw activations, one ``[images, C, r, r]`` tensor per layer in feature
    order (``layers``), and the class maps (``class_maps`` uint8 [images, S, S]).  The reference upsamples every layer to
    [S, S] and stores [images, S, S, F] floats on the host; here a pixel's features are sampled when it is drawn
    (``sis_hip.pe_train_gather``, or ``features`` in plain torch for the ATen loop).

    ``generate=True``: ``reset_dataset()`` runs the stored latent codes through ``generator`` with fresh noise and keeps the new
    activations (the reference's generation dataset); ``generate=False``: the stored activations.

    Sampling is drawn on the HOST from ``numpy.random.default_rng(seed + epoch)`` (the reference: a ``DataLoader``'s shuffle, and
    an unseeded generator per item for ``random_sampling``), see ``PixelBatchLoader``.
    """

    def __init__(self, json_file, tensor_path, class_to_color_map_path, image_size: int, background_class_name: str = 'background',
                 class_probabilities: Union[float, Sequence[float]] = 0.5, random_sampling: bool = False, generate: bool = False,
                 generator=None, device=None, loader=None, upsample_mode: str = 'bilinear'):
        if upsample_mode != 'bilinear':
            raise NotImplementedError(f"upsample_mode '{upsample_mode}': only 'bilinear' is implemented")
        self.device = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
        self.image_size, self.random_sampling, self.generate, self.generator = int(image_size), random_sampling, generate, generator
        self.tensor_path, self.dataset_path = Path(tensor_path), Path(tensor_path).parent
        self.background_class_name = background_class_name
        with Path(class_to_color_map_path).open() as f:
            self.class_to_color_map = json.load(f)
        if isinstance(class_probabilities, float):
            class_probabilities = [class_probabilities, 1 - class_probabilities]
        self.class_probabilities = [float(p) for p in class_probabilities]
        with open(json_file) as f:
            self.json_data = json.load(f)
        if not self.json_data:
            raise ValueError("the dataset lists no images")
        if loader is None:
            from data.segmentation_dataset import default_loader as loader
        self.image_paths = [self.dataset_path / entry["image"] for entry in self.json_data]
        maps = []
        for entry in self.json_data:
            label = numpy.array(loader(str(self.dataset_path / entry["label"])))
            if label.shape[:2] != (self.image_size, self.image_size):
                raise ValueError(f"label {entry['label']} is {label.shape[:2]}, the image size {self.image_size}")
            if self.device.type == 'cuda':
                from utils.segmentation_utils import segmentation_image_to_class_image
                maps.append(segmentation_image_to_class_image(numpy.ascontiguousarray(label[..., :3]), background_class_name,
                                                              self.class_to_color_map, device=self.device).cpu().numpy())
            else:
                maps.append(class_image_on_host(label, background_class_name, self.class_to_color_map))
        self.pixel_labels = numpy.stack(maps)                                  # host copy: buckets and the labels of a batch
        self.class_maps = torch.from_numpy(self.pixel_labels).to(self.device)  # resident copy
        tensors = numpy.load(self.tensor_path, allow_pickle=True)
        self.layers = None
        if generate:
            if generator is None:
                raise ValueError("generate=True needs the generator")
            codes = tensors["latent_codes"]
            self.latents = [torch.as_tensor(numpy.asarray(codes[entry["latent"]]), dtype=torch.float32) for entry in self.json_data]
            self.reset_dataset()
        else:
            stored = tensors["activations"]
            self._keep([stored[entry["activations"]] for entry in self.json_data])
        self.sampling_buckets = []
        if random_sampling:
            flat = self.pixel_labels.reshape(-1)
            self.sampling_buckets = [numpy.flatnonzero(flat == i) for i in range(len(self.class_probabilities))]
            for i, (bucket, p) in enumerate(zip(self.sampling_buckets, self.class_probabilities)):
                if p > 0 and bucket.size == 0:
                    raise ValueError(f"random_sampling: class {i} has probability {p} and no pixel")

    def _keep(self, per_image):
        """[{layer: [C, r, r] or [1, C, r, r]}] per image -> one resident [images, C, r, r] tensor per layer."""
        keys = list(per_image[0].keys())
        layers = []
        for key in keys:
            stack = torch.stack([torch.as_tensor(numpy.asarray(a[key]) if not torch.is_tensor(a[key]) else a[key]).float()
                                .reshape(tuple(a[key].shape[-3:])) for a in per_image])
            res = stack.shape[-1]
            if stack.shape[-2] != res or res > self.image_size or self.image_size % res or (self.image_size // res) & (self.image_size // res - 1):
                raise ValueError(f"layer {key}: resolution {tuple(stack.shape[-2:])} is no power-of-two fraction of {self.image_size}")
            layers.append(stack.to(self.device).contiguous())
        self.layer_keys, self.layers = keys, layers
        self.feature_vector_length = sum(t.shape[1] for t in layers)

    @torch.no_grad()
    def reset_dataset(self):
        if not self.generate:
            return
        per_image = []
        for latent in self.latents:
            latent = latent.to(self.device)
            noise = self.generator.make_noise()
            is_w = latent.dim() >= 2   # [n_latent, style_dim]: a projected W+ code; [style_dim]: z
            _, acts = self.generator([latent.unsqueeze(0)], input_is_latent=is_w, noise=noise, return_intermediate_activations=True)
            per_image.append({k: v[0] for k, v in acts.items()})
        self._keep(per_image)

    def get_feature_vector_length(self) -> int:
        return self.feature_vector_length

    def num_pixels(self) -> int:
        return int(self.pixel_labels.size)

    def __len__(self):
        return int(sum(len(b) for b in self.sampling_buckets)) if self.random_sampling else self.num_pixels()

    def batch(self, flat_indices: numpy.ndarray):
        """Flat pixel indices (image-major, then row, then column) -> the loaders' batch on the device."""
        s = self.image_size
        flat_indices = numpy.asarray(flat_indices, dtype=numpy.int64)
        pixels = numpy.stack([flat_indices // (s * s), flat_indices // s % s, flat_indices % s], 1).astype(numpy.int32)
        labels = self.pixel_labels.reshape(-1)[flat_indices].astype(numpy.int64)
        return {'pixels': torch.from_numpy(pixels).to(self.device, non_blocking=True),
                'label': torch.from_numpy(labels).to(self.device, non_blocking=True)}

    def features(self, pixels: torch.Tensor) -> torch.Tensor:
        """[P, F] features of pixels [P, 3] in plain torch (the ATen loop's input; the fused step gathers them in its own
        kernel): per layer the four bilinear taps of ``nn.Upsample(mode='bilinear')``, align_corners=False."""
        img, y, x = (pixels[:, i].long() for i in range(3))
        out = []
        for t in self.layers:
            res = t.shape[-1]
            if res == self.image_size:
                out.append(t[img, :, y, x])
                continue
            scale = res / self.image_size

            def src(d):
                s = ((d.to(t.dtype) + 0.5) * scale - 0.5).clamp_(min=0)
                i0 = s.floor().long()
                return i0, (i0 + 1).clamp_(max=res - 1), (s - i0.to(t.dtype))[:, None]

            y0, y1, ly = src(y)
            x0, x1, lx = src(x)
            out.append((1 - ly) * ((1 - lx) * t[img, :, y0, x0] + lx * t[img, :, y0, x1])
                       + ly * ((1 - lx) * t[img, :, y1, x0] + lx * t[img, :, y1, x1]))
        return torch.cat(out, 1)


class PixelBatchLoader:
    """Batches ``{'pixels': int32 [P, 3], 'label': int64 [P]}`` of a ``DeviceDatasetGANDataset``; one pass = one epoch.

    Ordinary sampling: one permutation of all pixels per epoch from ``default_rng(seed + epoch)``, cut into batches, the last
    partial one dropped (``drop_last``); ``shuffle=False`` (validation): index order, the partial batch kept.
    ``dataset.random_sampling``: per pixel a class drawn by ``class_probabilities``, then a pixel uniformly from that class's
    bucket; an epoch has ``len(dataset) // batch_size`` batches.  ``epoch_length`` caps the pixels per epoch."""

    def __init__(self, dataset: DeviceDatasetGANDataset, batch_size: int, shuffle: bool = True, drop_last: bool = True, seed: int = 0,
                 epoch_length: Optional[int] = None):
        self.dataset, self.batch_size, self.shuffle, self.drop_last, self.seed = dataset, int(batch_size), shuffle, drop_last, seed
        self.epoch_length, self.epoch = epoch_length, 0

    def _pixels_per_epoch(self) -> int:
        n = len(self.dataset)
        return min(n, self.epoch_length) if self.epoch_length else n

    def __len__(self):
        n = self._pixels_per_epoch()
        return n // self.batch_size if self.drop_last else -(-n // self.batch_size)

    def __iter__(self):
        rng = numpy.random.default_rng(self.seed + self.epoch)
        self.epoch += 1
        ds, b, n = self.dataset, self.batch_size, self._pixels_per_epoch()
        if ds.random_sampling and self.shuffle:
            probabilities = numpy.asarray(ds.class_probabilities) / sum(ds.class_probabilities)
            for _ in range(len(self)):
                classes = rng.choice(len(probabilities), size=b, p=probabilities)
                flat = numpy.empty(b, dtype=numpy.int64)
                for c, bucket in enumerate(ds.sampling_buckets):
                    mine = numpy.flatnonzero(classes == c)
                    if mine.size:
                        flat[mine] = bucket[rng.integers(0, bucket.size, size=mine.size)]
                yield ds.batch(flat)
            return
        order = rng.permutation(ds.num_pixels())[:n] if self.shuffle else numpy.arange(n)
        for lo in range(0, n, b):
            if lo + b > n and self.drop_last:
                return
            yield ds.batch(order[lo:lo + b])
