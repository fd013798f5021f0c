"""Synthetic (image, label) dataset generation: the hot loop of the reference's
create_dataset_for_segmentation.py:109-148, sharded over GPUs.

What runs per batch: seeded latents (CPU RNG, as utils/dataset_creation.py:32-37) -> ``Generator.forward`` with
intermediate activations on the MI355X kernels -> nearest k-means centre per pixel of the configured activation
layers on the device (FactorCatalog.predict) -> uint8 images on the device -> side-by-side ``[image | label]`` PNGs
in the reference's directory layout ``<id // 100000>/<id // 1000>/<id>.png`` (save_image, :84-90).

Without a ``segmenter_type`` the label half of the PNG is the raw cluster-id map of ``label_layer``
(id * 255 // (K-1) grey levels).  Not reproduced: debug images.

``--ground-truth`` (opt-in; needs ``class_to_color_map`` in the config; without it every output is what it was): the
reference's ground truth (:151-206).  In the loop the label image of every batch goes through ``sis_hip.label_regions`` in
listing mode on the label side stream (csrc/coco_gt.h), and when the batch is flushed the ``has_<class>`` truth
values of the written images are appended, one JSON line per image, to ``class_listing.rank<r>.jsonl`` below the save
directory.  The split then carries these keys in every entry of ``train.json`` / ``val.json`` (files the sidecars do not cover
are listed from their PNGs) and writes ``coco_gt.json`` for the validation images in ``val.json`` order: one annotation per
outermost contour of a class, holes filled, with RLE, area and bbox (segmentation/evaluation/coco_gt.py).
``--only-create-train-val-split --ground-truth`` does the same on a finished directory, with or without sidecars, which is
also the way after a run on several ranks.  ``scripts/balance_segmentation_train_gt.py`` consumes the keys.

Train / validation split (the reference's :180-202): after a normal run with ``--save-to`` (rank 0), or alone behind
``--only-create-train-val-split``, the PNGs below the save directory are shuffled with ``random.seed(config['seed'])`` and
written as ``train.json`` (90 %) / ``val.json`` (10 %), lists of ``{"file_name": path relative to the save directory}`` --
what ``train.py --images train.json --val-images val.json`` reads (data/segmentation_dataset.py).  The files are listed in
sorted order before the shuffle, so that the split depends on the seed and not on the file system.  With several ranks the
split is not written (the ranks do not synchronise): run it alone afterwards.

``segmenter_type: "black_white_handwritten_printed"`` (the reference's default labeller, :52-65, with its config keys
``class_to_color_map``, ``keys_for_class_determination``, ``keys_for_finegrained_segmentation``, ``keys_to_merge``,
``only_keep_overlapping``, ``min_class_contour_area``, and ``--num-clusters K`` / ``-ssd DIR`` naming
``DIR/catalogs/K.json`` and ``DIR/merged_classes_K.json``): class merging, contour extraction, merging across layers,
classification, area filter and rendering of the reference's BlackWhiteHandwrittenPrintedTextDatasetSegmenter run on the
device (csrc/cluster_segment.hip, DESIGN.md §11 with the stated differences) on the label side stream; the label half of
the PNG is the class-colour image.  Images the labeller flags (a class with a region taller and one wider than 95 % of the
image) are not written: their ids stay unused, so that the bytes behind an id do not depend on batch or world size (the
reference shifts the later ids instead).

``segmenter_type: "dataset_gan"`` in the config (with ``class_to_color_map`` and ``--classifier-path``, as the
reference's :52-81) labels every image with a trained PixelEnsembleClassifier instead
(segmentation/dataset_gan_segmenter.py, fused on the device); the label half of the PNG is then the class-colour image.

``--png-encoder device`` (default ``pil``: the loop above, unchanged): the label image is built on the device in every branch
and ``sis_hip.png_encode_pairs`` turns each ``[image | label]`` pair into a complete PNG file on the label side stream
(csrc/png_encode.h, DESIGN.md §14: filter Sub, one fixed-Huffman deflate block with run-length matches -- larger files than
PIL's, the same pixels); the host copies the finished files to pinned memory and only writes them, on ``--png-writers``
threads (default 4, at most 8), under the same directory layout and file names.  The writers are drained before the split
files are written and when the loop ends; an exception of a writer is raised in the main thread.

Multi-GPU (BASELINE.json configs[2]: 100k images on 8 GPUs): one process per GPU (``torch.distributed.run`` or
manual RANK/WORLD_SIZE), rank r generates the image-id range ``shard_range(num_images, r, world)``; no collective.
The latent stream is one global seeded stream: every rank draws the whole stream in batch order and keeps its own
rows; the per-batch noise maps ([1,1,h,h], shared by the batch's samples) are likewise drawn from the seeded device RNG
for EVERY batch on every rank, also the batches a rank skips.  So the image an id maps to does not depend on the world
size: the union over ranks equals the single-GPU dataset (tests/test_dataset_ops_gpu.py).
"""
import argparse
import json
import os
import random
from pathlib import Path

import numpy
import torch

import sis_hip  # noqa: F401  (fails loudly at import when libsis_hip.so is missing: there is no CPU path)
from networks import get_stylegan2_generator
from segmentation.gan_local_edit.factor_catalog import FactorCatalog
from utils.dataset_creation import encode_pairs_on_device, label_and_encode, list_classes_on_device, seeded_latents, shard_range

PNG_ENCODERS = ("pil", "device")
MAX_PNG_WRITERS = 8
CLASS_LISTING = "class_listing.rank{rank}.jsonl"


def ground_truth_creator(creation_config, image_root):
    """The COCOGtCreator of ``--ground-truth`` (the reference's :185)."""
    from segmentation.evaluation.coco_gt import COCOGtCreator
    if 'class_to_color_map' not in creation_config:
        raise ValueError('--ground-truth needs "class_to_color_map" in the config file')
    return COCOGtCreator(creation_config['class_to_color_map'], image_root=Path(image_root))


def png_writer_count(requested) -> int:
    """``--png-writers`` clamped to 1 .. 8 (a fixed small pool: never sized by the host's CPU count)."""
    return max(1, min(MAX_PNG_WRITERS, int(4 if requested is None else requested)))


def image_path(image_id: int, base_dir: Path, name_format: str = "{id}.png") -> Path:
    return base_dir / str(image_id // 100000) / str(image_id // 1000) / name_format.format(id=image_id)


def write_file(dest: Path, data) -> None:
    dest.parent.mkdir(exist_ok=True, parents=True)
    with open(dest, "wb") as f:
        f.write(data)


class PngWriterPool:
    """A few threads that write finished files; ``drain`` waits for all of them and re-raises a writer's exception in the
    caller.  ``keep_in_flight`` bounds the backlog (and with it the pinned buffers that are alive)."""

    def __init__(self, writers: int):
        from concurrent.futures import ThreadPoolExecutor
        self.pool = ThreadPoolExecutor(max_workers=png_writer_count(writers), thread_name_prefix="png-writer")
        self.futures = []

    def submit(self, dest: Path, data) -> None:
        self.futures.append(self.pool.submit(write_file, dest, data))

    def drain(self, keep_in_flight: int = 0) -> None:
        while len(self.futures) > keep_in_flight:
            self.futures.pop(0).result()

    def close(self) -> None:
        try:
            self.drain()
        finally:
            self.pool.shutdown(wait=True)


def save_image(image: numpy.ndarray, image_id: int, base_dir: Path, name_format: str = "{id}.png"):
    from PIL import Image
    dest = image_path(image_id, base_dir, name_format)
    dest.parent.mkdir(exist_ok=True, parents=True)
    Image.fromarray(image).save(str(dest))


def save_generated_images(generated_images, label_images, first_id: int, base_dir: Path, num_images: int, keep=None):
    images = numpy.concatenate([generated_images, label_images], axis=2)
    fmt = f"{{id:0{max(4, len(str(num_images)))}d}}.png"
    for idx, image in enumerate(images):
        if keep is None or keep[idx]:
            save_image(image, first_id + idx, base_dir, name_format=fmt)


def load_generator(checkpoint, size, latent_size, n_mlp, channel_multiplier, device):
    """Generator-only branch of ``load_autoencoder_or_generator`` (networks/__init__.py:415-423: key 'g_ema', strict)."""
    g = get_stylegan2_generator(size, latent_size, n_mlp=n_mlp, channel_multiplier=channel_multiplier,
                                init_ckpt=checkpoint or None, ckpt_key='g_ema', strict=True)
    return g.to(device).eval()


GENERATOR_PRECISIONS = ("fp32", "bf16")


def add_generator_precision_argument(parser):
    parser.add_argument("--generator-precision", choices=GENERATOR_PRECISIONS, default="fp32",
                        help="fp32: every generator layer on the fp32 kernels (the parity contract); bf16: the stride-1 3x3 "
                             "layers round their operands to bf16 and accumulate in fp32 (faster, images differ slightly)")


def apply_generator_precision(g, args):
    """--generator-precision on a loaded generator; one line names the mode.  (Callers without the flag: nothing changes.)"""
    precision = getattr(args, 'generator_precision', None)
    if precision is None:
        return g
    g.set_matrix_precision(precision)
    what = "stride-1 3x3 layers with bf16 operands, fp32 accumulation" if precision == "bf16" else "all layers fp32"
    print(f"generator precision: {precision} ({what})", flush=True)
    return g


def dataset_gan_segmenter(g, classifier_path, creation_config, mean_latent, device):
    """The reference's get_dataset_gan_params + get_dataset_segmenter (:28-81): one probe forward (B = 1, before the
    dataset's seed is set) gives the activation layout, i.e. the feature size and one bilinear upsampler per layer."""
    from segmentation.dataset_gan_segmenter import DatasetGANSegmenter, dataset_gan_upsamplers
    if not classifier_path:
        raise ValueError('segmenter_type "dataset_gan" needs --classifier-path (the trained ensemble checkpoint)')
    with torch.no_grad():
        _, acts = g([torch.randn(1, g.style_dim, device=device)], noise=g.make_noise(), return_intermediate_activations=True,
                    truncation=0.7 if mean_latent is not None else 1, truncation_latent=mean_latent)
    return DatasetGANSegmenter(base_dir=None, image_size=g.size, class_to_color_map=creation_config['class_to_color_map'],
                               classifier_path=classifier_path, feature_size=sum(a.shape[1] for a in acts.values()),
                               upsamplers=dataset_gan_upsamplers(acts, g.size))


def cluster_based_segmenter(args, creation_config, image_size):
    """The 'black_white_handwritten_printed' branch of the reference's get_dataset_segmenter (:52-65, :76-81)."""
    from segmentation.black_white_handwritten_printed_text_segmenter import BlackWhiteHandwrittenPrintedTextDatasetSegmenter
    if 'only_keep_overlapping' not in creation_config:
        raise ValueError('The key "only_keep_overlapping" must be specified in the config file.')
    num_clusters, base_dir = getattr(args, 'num_clusters', -1), getattr(args, 'semantic_segmentation_base_dir', None)
    if num_clusters is None or num_clusters < 1 or base_dir is None:
        raise ValueError('segmenter_type "black_white_handwritten_printed" needs --num-clusters and '
                         '-ssd/--semantic-segmentation-base-dir (catalogs/K.json and merged_classes_K.json)')
    return BlackWhiteHandwrittenPrintedTextDatasetSegmenter(
        base_dir=Path(base_dir), image_size=image_size, class_to_color_map=creation_config['class_to_color_map'],
        keys_to_merge=creation_config.get('keys_to_merge', {}), only_keep_overlapping=creation_config['only_keep_overlapping'],
        keys_for_class_determination=creation_config['keys_for_class_determination'],
        keys_for_finegrained_segmentation=creation_config['keys_for_finegrained_segmentation'],
        num_clusters=num_clusters, min_class_contour_area=creation_config['min_class_contour_area'])


def build_dataset(args, creation_config, rank=0, world_size=1):
    encoder = getattr(args, 'png_encoder', None) or 'pil'
    if encoder not in PNG_ENCODERS:
        raise ValueError(f"--png-encoder {encoder!r}: one of {PNG_ENCODERS}")
    device = torch.device('cuda', rank % max(torch.cuda.device_count(), 1))
    torch.cuda.set_device(device)
    g = load_generator(args.checkpoint, creation_config.get('image_size', 256), creation_config.get('latent_size', 512),
                       creation_config.get('n_mlp', 8), creation_config.get('channel_multiplier', 2), device)
    apply_generator_precision(g, args)
    catalogs = {}
    for layer, path in creation_config.get('catalogs', {}).items():  # {"13": "centres_13.npy", ...}
        catalogs[int(layer)] = FactorCatalog(cluster_centers=numpy.load(path))
    label_layer = int(creation_config.get('label_layer', max(catalogs) if catalogs else -1))
    mean_latent = g.mean_latent(4096) if args.truncate else None
    dataset_gan = None
    if creation_config.get('segmenter_type') == 'dataset_gan':
        dataset_gan = dataset_gan_segmenter(g, getattr(args, 'classifier_path', None), creation_config, mean_latent, device)
    cluster_segmenter = None
    if creation_config.get('segmenter_type') == 'black_white_handwritten_printed':
        cluster_segmenter = cluster_based_segmenter(args, creation_config, g.size)
    lo, hi = shard_range(args.num_images, rank, world_size)
    dropped = []
    save_dir = Path(args.save_to) if args.save_to else None
    on_device = encoder == 'device' and save_dir is not None
    writers = PngWriterPool(getattr(args, 'png_writers', None)) if on_device else None
    name_format = f"{{id:0{max(4, len(str(args.num_images)))}d}}.png"
    listing = None   # --ground-truth: (creator, the open sidecar) of this rank
    if getattr(args, 'ground_truth', False) and save_dir is not None:
        creator = ground_truth_creator(creation_config, save_dir)
        save_dir.mkdir(exist_ok=True, parents=True)
        listing = (creator, (save_dir / CLASS_LISTING.format(rank=rank)).open('w'))
    torch.random.manual_seed(creation_config.get('seed', 1))
    done = 0

    def label_image_on_device(pixels, labels):
        """The label half of the pair as uint8 [B, H, W, 3] on the device: the four branches of ``flush`` below."""
        if cluster_segmenter is not None:
            return labels["cluster_segmenter"][1]
        if dataset_gan is not None:
            return labels["dataset_gan"]
        if label_layer in labels:
            k = catalogs[label_layer].cluster_centers.shape[0]
            lab = labels[label_layer]
            if lab.shape[-1] != pixels.shape[2]:
                lab = torch.nn.functional.interpolate(lab[:, None].float(), size=pixels.shape[1:3], mode='nearest')[:, 0].long()
            grey = (lab * 255 // max(k - 1, 1)).to(torch.uint8)
            return grey[..., None].expand(-1, -1, -1, 3).contiguous()
        return torch.zeros_like(pixels)

    def flush(job):
        """Host side of a finished batch: wait for its label pass, then encode / write the files."""
        first_id, pixels, labels, ready, files, listed = job
        if ready is not None:
            ready.synchronize()
        keep = None
        if cluster_segmenter is not None:
            keep = ~labels["cluster_segmenter"][2].cpu().numpy().astype(bool)
            dropped.extend(first_id + int(i) for i in numpy.nonzero(~keep)[0])
        if save_dir is None:
            return
        if listed is not None:   # its copy was issued on the label stream before the event(s) this function waits for
            if ready is None:
                listed[1].synchronize()
            creator, sidecar = listing
            for idx, row in enumerate(listed[0].numpy()):
                if keep is None or keep[idx]:
                    name = str(image_path(first_id + idx, save_dir, name_format).relative_to(save_dir))
                    sidecar.write(json.dumps({"file_name": name, **creator.classes_from_has(row)}) + "\n")
        if files is not None:   # encoded on the device: the host only writes buffer[i, :sizes[i]]
            buffer, sizes, encoded = files
            encoded.synchronize()
            buffer, sizes = buffer.numpy(), sizes.numpy()
            for idx in range(buffer.shape[0]):
                if keep is None or keep[idx]:
                    writers.submit(image_path(first_id + idx, save_dir, name_format), memoryview(buffer[idx, :int(sizes[idx])]))
            writers.drain(keep_in_flight=2 * args.batch_size)
            return
        rgb = pixels.cpu().numpy()
        if cluster_segmenter is not None:
            lab_img = labels["cluster_segmenter"][1].cpu().numpy()
        elif dataset_gan is not None:
            lab_img = labels["dataset_gan"].cpu().numpy()
        elif label_layer in labels:
            k = catalogs[label_layer].cluster_centers.shape[0]
            lab = labels[label_layer]
            if lab.shape[-1] != rgb.shape[2]:
                lab = torch.nn.functional.interpolate(lab[:, None].float(), size=rgb.shape[1:3], mode='nearest')[:, 0].long()
            grey = (lab * 255 // max(k - 1, 1)).to(torch.uint8).cpu().numpy()
            lab_img = numpy.repeat(grey[..., None], 3, axis=3)
        else:
            lab_img = numpy.zeros_like(rgb)
        save_generated_images(rgb, lab_img, first_id, save_dir, args.num_images, keep)

    def run_batches():
        nonlocal done
        pending = None
        for first in range(0, args.num_images, args.batch_size):
            n = min(args.batch_size, args.num_images - first)
            z = seeded_latents(args.batch_size, g.style_dim, device)[:n]  # the whole stream is drawn on every rank (pinned) ...
            noise = g.make_noise()  # ... and so are the batch's noise maps (device RNG, same seed on every rank)
            a, b = max(first, lo), min(first + n, hi)
            if a >= b:
                continue
            # A batch that straddles a shard boundary is synthesised WHOLE by both of its owners and then cut: the kernels'
            # split-K / tile plans follow the batch size, so only the same batch gives the same bits -- the bytes an image id
            # maps to must not depend on the world size (at most one redundant partial batch per shard boundary).
            image, acts = g([z.to(device, non_blocking=True)], noise=noise, return_intermediate_activations=True,
                            truncation=0.7 if mean_latent is not None else 1, truncation_latent=mean_latent)
            if (a, b) != (first, first + n):
                image = image[a - first:b - first]
                acts = {k: v[a - first:b - first] for k, v in acts.items()}
            # side stream; the next batch's forward is issued first.  Without a cluster-based labeller the call is the one it
            # always was (callers wrap label_and_encode with its earlier signature).
            extra = {} if cluster_segmenter is None else {"cluster_segmenter": cluster_segmenter}
            pixels, labels, ready = label_and_encode(image, acts, catalogs, dataset_gan, **extra)
            # device encoder: label image, PNG files and their copy to pinned memory follow the label pass on its stream
            label_image, listed = (lambda: label_image_on_device(pixels, labels)), None
            if listing is not None:   # the class listing follows the label image on the same stream; the label image is built once
                lab, has, listed_event = list_classes_on_device(pixels, label_image, listing[0].colours, ready)
                label_image, listed = (lambda: lab), (has, listed_event)
                if ready is not None:
                    ready = listed_event   # later on the same stream: flush waits once, as before
            files = encode_pairs_on_device(pixels, label_image, ready) if on_device else None
            job = (a, pixels, labels, ready, files, listed)
            if pending is not None:
                flush(pending)
            pending = job
            done += b - a
        if pending is not None:
            flush(pending)

    try:
        with torch.no_grad():
            run_batches()
    finally:
        if writers is not None:
            writers.close()   # drained here: before the caller writes the split files, and on every way out
        if listing is not None:
            listing[1].close()
    torch.cuda.synchronize()
    args.dropped_image_ids = dropped   # the labeller's drop decisions of this rank (empty without a cluster-based labeller)
    return done, (lo, hi)


def read_class_listings(image_save_base_dir: Path) -> dict:
    """file name -> its ``has_<class>`` keys, from the sidecars the ranks of a ``--ground-truth`` run left."""
    listed = {}
    for sidecar in sorted(Path(image_save_base_dir).glob(CLASS_LISTING.format(rank='*'))):
        with sidecar.open() as f:
            for line in f:
                if line.strip():
                    entry = json.loads(line)
                    listed[entry.pop("file_name")] = entry
    return listed


def create_train_val_split(image_save_base_dir: Path, seed: int, ground_truth=None):
    """train.json / val.json below ``image_save_base_dir``: seeded shuffle of its PNGs, the first 90 % train, the rest validation.
    ``ground_truth`` (a COCOGtCreator rooted at the directory): every entry also carries the image's ``has_<class>`` keys -- from
    the sidecars of the run where they cover the file, from its PNG otherwise -- and ``coco_gt.json`` is written for the
    validation images in ``val.json`` order (the reference's :180-206)."""
    image_save_base_dir = Path(image_save_base_dir)
    generated_images = sorted(image_save_base_dir.glob('**/*.png'))
    random.seed(seed)
    random.shuffle(generated_images)
    n_train = len(generated_images) * 9 // 10   # nine tenths train, the rest validation (floor, as int(0.9 n))
    parts = {'train.json': generated_images[:n_train], 'val.json': generated_images[n_train:]}
    classes = {}
    if ground_truth is not None:
        keys = {f"has_{name}" for _, name, _ in ground_truth.annotated}
        classes = {name: entry for name, entry in read_class_listings(image_save_base_dir).items() if set(entry) == keys}
        missing = [path for path in generated_images if str(path.relative_to(image_save_base_dir)) not in classes]
        for path, entry in zip(missing, ground_truth.determine_classes_in_images(missing)):
            classes[str(path.relative_to(image_save_base_dir))] = entry
    for name, paths in parts.items():
        with (image_save_base_dir / name).open('w') as f:
            json.dump([{"file_name": str(path.relative_to(image_save_base_dir)), **classes.get(str(path.relative_to(image_save_base_dir)), {})}
                       for path in paths], f)
    if ground_truth is not None:
        with (image_save_base_dir / 'coco_gt.json').open('w') as f:
            json.dump(ground_truth.create_coco_gt_from_image_paths(parts['val.json']), f)
    return len(parts['train.json']), len(parts['val.json'])


def main(args):
    creation_config = json.load(open(args.config)) if args.config else {}
    rank, world = int(os.environ.get('RANK', '0')), int(os.environ.get('WORLD_SIZE', '1'))
    with_gt = {}
    if getattr(args, 'ground_truth', False) and args.save_to:
        with_gt = {"ground_truth": ground_truth_creator(creation_config, args.save_to)}
    if getattr(args, 'only_create_train_val_split', False):
        if not args.save_to:
            raise ValueError('--only-create-train-val-split needs --save-to (the directory that holds the PNG pairs)')
        n_train, n_val = create_train_val_split(Path(args.save_to), creation_config.get('seed', 1), **with_gt)
        print(f"split: {n_train} training and {n_val} validation images", flush=True)
        return
    done, (lo, hi) = build_dataset(args, creation_config, rank, world)
    if args.save_to and world == 1:
        create_train_val_split(Path(args.save_to), creation_config.get('seed', 1), **with_gt)
    elif args.save_to and rank == 0:   # no collective in this tool: the other ranks may still be writing
        print("several ranks: train.json / val.json are NOT written; run --only-create-train-val-split once all ranks are done",
              flush=True)
    note = ""
    if creation_config.get('segmenter_type') == 'black_white_handwritten_printed':
        note = f", {len(args.dropped_image_ids)} of them dropped by the labeller and not written"
    print(f"rank {rank}/{world}: generated image ids [{lo}, {hi}) = {done} images{note}", flush=True)


def build_parser():
    parser = argparse.ArgumentParser(description="Generate a synthetic dataset with a StyleGAN2 generator on MI355X")
    parser.add_argument("checkpoint", nargs='?', default=None, help="generator checkpoint holding 'g_ema' (omit: random weights)")
    parser.add_argument("config", nargs='?', default=None, help="json: image_size, latent_size, seed, catalogs{layer: centres.npy}, label_layer; "
                        "or segmenter_type 'dataset_gan' with class_to_color_map")
    parser.add_argument("-n", "--num-images", type=int, default=100)
    parser.add_argument("-s", "--save-to", help="directory for the PNG pairs (omit: generate only)")
    parser.add_argument("-b", "--batch-size", default=10, type=int)
    parser.add_argument("--only-create-train-val-split", action='store_true', default=False,
                        help="do not create a dataset: build train.json / val.json from the PNG pairs below --save-to")
    parser.add_argument("--truncate", action='store_true', default=False, help="truncation trick (psi 0.7, mean of 4096 latents)")
    parser.add_argument("--classifier-path", help="trained PixelEnsembleClassifier checkpoint (segmenter_type \"dataset_gan\")")
    parser.add_argument("--num-clusters", type=int, default=-1, help="K of catalogs/K.json and merged_classes_K.json "
                        "(segmenter_type \"black_white_handwritten_printed\")")
    parser.add_argument("--png-encoder", choices=PNG_ENCODERS, default="pil", help="pil: PIL on the host, one file at a time; "
                        "device: the PNG files are encoded on the device (fixed-Huffman deflate: larger files, the same pixels) "
                        "and the host only writes them")
    parser.add_argument("--png-writers", type=png_writer_count, default=4, help="file-writer threads of --png-encoder device "
                        "(clamped to 1..8)")
    parser.add_argument("--ground-truth", action='store_true', default=False, help="also write the has_<class> keys of train.json / "
                        "val.json and coco_gt.json for the validation images (needs class_to_color_map in the config)")
    parser.add_argument("-ssd", "--semantic-segmentation-base-dir", type=Path, help="directory that holds catalogs/ and "
                        "merged_classes_K.json, as create_semantic_segmentation.py and the annotation step leave it")
    add_generator_precision_argument(parser)
    return parser


if __name__ == "__main__":
    main(build_parser().parse_args())
