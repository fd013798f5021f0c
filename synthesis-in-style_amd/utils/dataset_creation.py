"""Synthesis driver: the seeded latent/noise stream and the batched generator call.

Mirrors utils/dataset_creation.py:32-58 of the reference (the two functions the hot loop of
create_dataset_for_segmentation.py:129-148 calls).  Same observable behaviour:

* ``build_latent_and_noise_generator``: ``torch.random.manual_seed(seed)`` once, then per batch
  ``z = randn(B, latent_size)`` from the CPU RNG and ``decoder.make_noise()`` on the generator's device;
* ``generate_images``: move the batch to the device, run ``decoder([z], input_is_latent=False,
  noise=..., return_intermediate_activations=True, truncation=0.7 iff a mean latent is given)`` under
  ``torch.no_grad()``, return ``(activations, image)``.

A dict batch ``{'input_image': ...}`` takes the reference's image-encoding branch: ``autoencoder.encode`` (the projection
encoders, networks/encoder/), then the decoder with ``input_is_latent=autoencoder.is_wplus(latents)``.
"""
import os
from typing import Dict, Iterable, Optional, Tuple

import torch

import sis_hip

from latent_projecting import Latents


def seeded_latents(batch: int, dim: int, device) -> torch.Tensor:
    """``torch.randn(batch, dim)`` from the CPU generator (the reference's latent stream, same values) drawn into PINNED host
    memory when it is headed for a HIP device: the copy that follows (``.to(device, non_blocking=True)``) is then a true
    asynchronous transfer (from pageable memory the runtime stages it through a bounce buffer on the calling thread).  Measured
    on the dataset loop: no difference (15.88 ms per batch of 32 either way, profiles/r05_dataset_vs_synthesis.txt) -- the loop's
    0.9 ms over bare synthesis is the label pass itself: 2.7 GB of activations re-read while the next batch's convolutions
    run, which slows those by what the pass would have cost alone (profiles/r05_dataset_timeline.txt)."""
    device = torch.device(device)
    return torch.randn(batch, dim, pin_memory=device.type == 'cuda' and torch.cuda.is_available())


def build_latent_and_noise_generator(autoencoder, config: Dict, seed=1) -> Iterable:
    torch.random.manual_seed(seed)
    decoder = autoencoder.decoder
    while True:
        device = next(decoder.parameters()).device
        yield Latents(seeded_latents(config['batch_size'], config['latent_size'], device), decoder.make_noise())


def shard_range(num_images: int, rank: int, world_size: int) -> Tuple[int, int]:
    """Image-id range [lo, hi) of one rank: contiguous blocks, remainder spread over the first ranks
    (multi-GPU synthesis is embarrassingly parallel -- SURVEY.md §8e; the reference is single-GPU)."""
    base, rem = divmod(num_images, world_size)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def generate_images(batch: Latents, autoencoder, device='cuda', mean_latent: Optional[torch.Tensor] = None) \
        -> Tuple[Dict[int, torch.Tensor], torch.Tensor]:
    with torch.no_grad():
        if isinstance(batch, Latents):
            latents, input_is_latent = batch.to(device), False
        elif isinstance(batch, dict) and 'input_image' in batch:
            # the reference's image batches (:44-47): encode, then decode W+ latents as latents and W latents through the mapping
            latents = autoencoder.encode(batch['input_image'].to(device))
            input_is_latent = autoencoder.is_wplus(latents)
        else:
            raise NotImplementedError("a batch is a Latents object or a dict holding 'input_image'")
        image, activations = autoencoder.decoder(
            [latents.latent], input_is_latent=input_is_latent, noise=latents.noise, return_intermediate_activations=True,
            truncation=0.7 if mean_latent is not None else 1, truncation_latent=mean_latent)
    return activations, image


_LABEL_STREAMS = {}  # device -> side stream of the label / uint8 pass


def label_and_encode(image: torch.Tensor, activations: Dict[int, torch.Tensor], catalogs: Dict, dataset_gan=None,
                     cluster_segmenter=None) -> Tuple[torch.Tensor, Dict, Optional[torch.cuda.Event]]:
    """What the reference does with a batch after ``generate_images`` (create_dataset_for_segmentation.py:131-135 ->
    ``predict_clusters`` -> ``FactorCatalog.predict``; ``make_image``): nearest-centre label maps of the catalogued
    activation layers and the uint8 NHWC image, here issued on a side stream.  Both passes are HBM-bound
    readers of finished tensors, so they overlap the MFMA-bound first layers of the NEXT batch, whose small grids
    leave most compute units idle.  Returns (pixels u8 [B,H,W,3], {layer: labels}, event): wait for / synchronise on
    the event before touching the results from another stream or the host.  SIS_LABEL_STREAM=0 keeps everything on the
    current stream (event None).  ``dataset_gan``: a DatasetGANSegmenter whose fused pass also runs there; its uint8
    [B,H,W,3] class-colour image is returned under the key "dataset_gan".  ``cluster_segmenter``: a cluster-based labeller
    (segmentation/black_white_handwritten_printed_text_segmenter.py) whose device pass runs there too; its
    (class map, colour image, drop flags) triple is returned under the key "cluster_segmenter"."""
    device = image.device

    def labels_of():
        labels = {k: cat.predict(activations[k]) for k, cat in catalogs.items()}
        if dataset_gan is not None:
            labels["dataset_gan"] = dataset_gan.label_activations(activations)[1]
        if cluster_segmenter is not None:
            labels["cluster_segmenter"] = cluster_segmenter.label_activations(activations)
        return labels

    if os.environ.get("SIS_LABEL_STREAM", "1") == "0" or not image.is_cuda:
        return sis_hip.make_image_u8(image), labels_of(), None
    if device not in _LABEL_STREAMS:
        _LABEL_STREAMS[device] = sis_hip.side_stream(device)
    side, main = _LABEL_STREAMS[device], torch.cuda.current_stream(device)
    side.wait_event(main.record_event())
    with torch.cuda.stream(side):
        labels = labels_of()
        pixels = sis_hip.make_image_u8(image)
    read = list(activations.values()) if dataset_gan is not None or cluster_segmenter is not None \
        else [activations[k] for k in catalogs]
    for t in [image] + read:
        t.record_stream(side)  # the caching allocator must not hand these blocks out again before the side pass has read them
    return pixels, labels, side.record_event()


def encode_pairs_on_device(pixels: torch.Tensor, label_image, ready: Optional[torch.cuda.Event] = None):
    """The PNG files of ``[pixels | label_image()]`` (create_dataset_for_segmentation.py:84-90 of the reference, save_image)
    encoded on the device and copied to PINNED host memory.  ``pixels``: uint8 [B, H, W, 3] as ``label_and_encode`` returns
    them, ``label_image``: a callable that builds the uint8 [B, H, W, 3] label half on the device, ``ready``: the event
    ``label_and_encode`` returned.  With an event everything is issued on the label side stream, behind the label pass, so it
    runs beside the next batch's forward like that pass; without one (SIS_LABEL_STREAM=0) on the current stream.  Returns
    (buffer uint8 [B, stride] host, sizes int32 [B] host, event): synchronise on the event, then ``buffer[i, :sizes[i]]``
    is file i."""
    device = pixels.device
    side = _LABEL_STREAMS.get(device) if ready is not None else None
    stream = side if side is not None else torch.cuda.current_stream(device)
    with torch.cuda.stream(stream):
        buffer, sizes = sis_hip.png_encode_pairs(pixels, label_image())
        host_buffer = torch.empty(buffer.shape, dtype=torch.uint8, pin_memory=True)
        host_sizes = torch.empty(sizes.shape, dtype=torch.int32, pin_memory=True)
        host_buffer.copy_(buffer, non_blocking=True)
        host_sizes.copy_(sizes, non_blocking=True)
        return host_buffer, host_sizes, stream.record_event()


def list_classes_on_device(pixels: torch.Tensor, label_image, colours, ready: Optional[torch.cuda.Event] = None):
    """Which annotated classes every label image holds (the reference's determine_classes_in_image,
    segmentation/evaluation/coco_gt.py:51-65): ``sis_hip.label_regions`` in listing mode on the uint8 [B, p, p, 3] label images
    that the callable ``label_image`` builds on the device, and its ``has`` bytes copied to PINNED host memory.  Issued like
    ``encode_pairs_on_device``: with ``ready`` (the event ``label_and_encode`` returned) on the label side stream, behind the
    label pass; without one on the current stream.  Returns (label images, has uint8 [B, K] host, event): synchronise on the
    event before reading ``has``; the event also stands for the label pass before it."""
    device = pixels.device
    side = _LABEL_STREAMS.get(device) if ready is not None else None
    stream = side if side is not None else torch.cuda.current_stream(device)
    with torch.cuda.stream(stream):
        labels = label_image()
        has = sis_hip.label_regions(labels, colours, runs=False, max_regions=0).has
        host_has = torch.empty(has.shape, dtype=torch.uint8, pin_memory=True)
        host_has.copy_(has, non_blocking=True)
        return labels, host_has, stream.record_event()
