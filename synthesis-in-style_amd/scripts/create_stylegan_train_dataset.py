"""Cut GAN training patches from document scans (the reference's scripts/create_stylegan_train_dataset.py).

Every image under ``root_dir`` is shrunk to ``--max-size`` where a side exceeds it, shrunk again by a random factor 1..4 (but
not below ``--min-size``), cut into ``--image-size`` windows that cover it with an even overlap, and every window is saved as
``destination/<relative dir>/<stem>_<patch idx>.png``.  ``train.json`` and ``val.json`` list the patches, shuffled and split
90 / 10: the lists ``train_stylegan_2.py`` trains from.

Two pixel paths give the same pixels:

* ``--pixel-path device`` (default): pages are decoded on the host by a small thread pool, uploaded through pinned memory, and
  shrunk (``sis_hip.scan_thumbnail``) and cut (``sis_hip.scan_patches``) by the kernels of csrc/scan_patches.h, whose 8-bit
  arithmetic is Pillow's, byte for byte.  With ``--png-encoder device`` (the default of this path) the
  patches are encoded by ``sis_hip.png_encode_pairs`` and the host only writes finished files, on the writer pool of
  create_dataset_for_segmentation.py; these files decode to the same pixels as Pillow's but are not its bytes.
* ``--pixel-path pil``: the reference's sequence with Pillow alone -- ``thumbnail``, ``random_resize``, ``crop_patches``,
  ``save``.  The fallback for a host without a device, and the yardstick of the tests.

Both paths draw from the host ``random`` alike -- the shuffle of the files, one factor per decoded page, the shuffle before
the split -- so one ``--seed`` gives one set of names, factors and lists.  File listings are sorted before they are shuffled.

What differs from the reference:

* Files are decoded IN FULL and converted to RGB before anything else, on both paths.  The reference calls ``thumbnail`` on
  the still lazy file, where Pillow's ``draft`` lets a JPEG decode at a DCT scale when it is to shrink 2x or more: JPEG
  sources give other pixels than the reference there, PNG and TIFF sources the same.
* ``--margin-remove`` runs on the device path only: ``sis_hip.scan_remove_margin`` finds the content box of every decoded page
  on its 1000-pixel thumbnail (blur, Canny, closing, contour boxes and the largest-gap cut of the reference's
  ``get_content_box``, stated in integers in DESIGN.md §20 and run by csrc/scan_margin.h) and crops the page before anything
  else, as the reference does.  The statement follows OpenCV's documented behaviour; OpenCV is not a dependency and nothing was
  compared with it.  With ``--pixel-path pil`` the option still raises: there is no host implementation.  The random stream
  does not see the option: one ``--seed`` gives the same names, factors and lists with and without it.
* No progress bars (tqdm is not a dependency).
"""
import argparse
import json
import os
import random
import sys
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

if __name__ == "__main__":   # run as a file: the package root is the directory above scripts/
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from data.segmentation_dataset import is_image
from utils.scan_patches import ANALYSIS_SIZE, patch_origins, random_resize_size, window_starts

PIXEL_PATHS = ("device", "pil")
PNG_ENCODERS = ("device", "pil")
MAX_DECODE_WORKERS = 16
MARGIN_REMOVE_MESSAGE = ("--margin-remove is not built: margin removal needs Canny edge detection and a contour hierarchy, "
                         "and OpenCV is not a dependency of this repository.")


def decode_worker_count(requested=None) -> int:
    """``--decode-workers`` clamped to 1 .. 16 (a fixed small pool: never sized by the host's CPU count)."""
    return max(1, min(MAX_DECODE_WORKERS, int(8 if requested is None else requested)))


def decode_page(path):
    """The file decoded in full, as an RGB Pillow image."""
    from PIL import Image
    with Image.open(str(path)) as image:
        return image.convert("RGB")


def crop_patches(image, image_size: int):
    """The windows of the reference's crop_patches (:18-34), cut by Pillow's crop at the FLOAT boxes (it rounds them itself)."""
    columns = window_starts(image.width, image_size)
    return [image.crop((x, y, x + image_size, y + image_size)) for y in window_starts(image.height, image_size) for x in columns]


def page_patches_pil(image, factor: int, image_size: int, max_size: int, min_size: int):
    """One decoded page -> its patches as Pillow images: thumbnail(max_size), random_resize with the drawn ``factor``, crop."""
    if any(side > max_size for side in image.size):
        image.thumbnail((max_size, max_size))
    new_size = random_resize_size(image.width, image.height, factor, min_size)
    image.thumbnail((new_size, new_size))
    return crop_patches(image, image_size)


def page_patches_device(image, factor: int, image_size: int, max_size: int, min_size: int, device, margin_remove: bool = False):
    """One decoded page -> its patches as uint8 [n, size, size, 3] on the device, the same pixels as ``page_patches_pil``.
    ``margin_remove``: the scanner margin is cropped off first (``sis_hip.scan_remove_margin``, one host read of four integers)."""
    import numpy
    import torch
    import sis_hip
    host = torch.empty((image.height, image.width, 3), dtype=torch.uint8, pin_memory=True)
    numpy.copyto(host.numpy(), numpy.asarray(image, dtype=numpy.uint8))
    page = host.to(device, non_blocking=True)
    if margin_remove:
        page = sis_hip.scan_remove_margin(page, ANALYSIS_SIZE)[0]
    if any(side > max_size for side in (page.shape[1], page.shape[0])):
        page = sis_hip.scan_thumbnail(page, max_size)
    new_size = random_resize_size(int(page.shape[1]), int(page.shape[0]), factor, min_size)
    page = sis_hip.scan_thumbnail(page, new_size)
    return sis_hip.scan_patches(page, patch_origins(int(page.shape[1]), int(page.shape[0]), image_size), image_size)


class DecodedPages:
    """The files decoded ahead of the loop by ``workers`` threads, handed out in order as (path, image or exception)."""

    def __init__(self, files, workers: int):
        self.files = list(files)
        self.workers = decode_worker_count(workers)
        self.pool = ThreadPoolExecutor(max_workers=self.workers, thread_name_prefix="page-decode")
        self.futures = []
        self.submitted = 0

    def _fill(self):
        while self.submitted < len(self.files) and len(self.futures) < 2 * self.workers:
            self.futures.append(self.pool.submit(decode_page, self.files[self.submitted]))
            self.submitted += 1

    def __iter__(self):
        for index, path in enumerate(self.files):
            self._fill()
            future = self.futures.pop(0)
            try:
                yield index, path, future.result()
            except Exception as e:   # the reference prints a page's exception and goes on
                yield index, path, e

    def close(self):
        for future in self.futures:
            future.cancel()
        self.pool.shutdown(wait=True)


def list_images(directory: Path, pattern: str):
    return sorted(file_name for file_name in directory.glob(pattern) if is_image(file_name))


def resolve_paths(args):
    """(pixel path, PNG encoder) of the arguments; the encoder defaults to the device where the pixels are there."""
    pixel_path = getattr(args, "pixel_path", None) or "device"
    png_encoder = getattr(args, "png_encoder", None) or ("device" if pixel_path == "device" else "pil")
    if pixel_path not in PIXEL_PATHS or png_encoder not in PNG_ENCODERS:
        raise ValueError(f"pixel path {pixel_path!r}, PNG encoder {png_encoder!r}: each must be one of {PIXEL_PATHS}")
    if getattr(args, "margin_remove", False) and pixel_path != "device":
        raise NotImplementedError(MARGIN_REMOVE_MESSAGE)
    return pixel_path, png_encoder


def cut_patches(args, root_dir: Path, destination: Path, rng):
    """Patches of up to ``max_num_samples`` pages written under ``destination``; returns their paths relative to it."""
    pixel_path, png_encoder = resolve_paths(args)
    device = writers = None
    if "device" in (pixel_path, png_encoder):
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("no HIP device: --pixel-path device and --png-encoder device run on one; use --pixel-path pil")
        import sis_hip
        sis_hip.lib()   # fails loudly when the extension is missing
        device = torch.device("cuda", torch.cuda.current_device())
    if png_encoder == "device":
        from create_dataset_for_segmentation import PngWriterPool
        from utils.dataset_creation import encode_pairs_on_device
        writers = PngWriterPool(getattr(args, "png_writers", None))

    glob_filter = f"**/*{args.filter}*" if args.filter is not None else "**/*"
    files_in_root = list_images(root_dir, glob_filter)
    num_files_to_use = min(len(files_in_root), args.max_num_samples)
    rng.shuffle(files_in_root)
    image_size, max_size, min_size = args.image_size, args.max_size, getattr(args, "min_size", 1000)
    margin_remove = bool(getattr(args, "margin_remove", False))

    patch_paths = []
    pending = None   # (names, host buffer, host sizes, event) of the page before: written while this page's kernels run

    def flush(entry):
        if entry is not None:
            names, buffer, sizes, event = entry
            event.synchronize()
            for i, name in enumerate(names):
                writers.submit(name, memoryview(buffer[i, :int(sizes[i])].numpy()))
            writers.drain(keep_in_flight=4 * len(names))

    pages = DecodedPages(files_in_root, getattr(args, "decode_workers", None))
    try:
        for idx, file_path, image in pages:
            dest_dir = destination / file_path.parent.relative_to(root_dir)
            dest_dir.mkdir(exist_ok=True, parents=True)
            if isinstance(image, Exception):   # a page that cannot be decoded is printed and skipped, as in the reference;
                print(image)                   # any other failure (a kernel, a write) ends the run
            else:
                factor = rng.randint(1, 4)   # random_resize's draw: one per decoded page, on both paths
                if pixel_path == "pil":
                    patches = page_patches_pil(image, factor, image_size, max_size, min_size)
                    count = len(patches)
                else:
                    pixels = page_patches_device(image, factor, image_size, max_size, min_size, device, margin_remove)
                    count = int(pixels.shape[0])
                names = [dest_dir / f"{file_path.stem}_{patch_idx}.png" for patch_idx in range(count)]
                if png_encoder == "pil":
                    if pixel_path == "device":
                        from PIL import Image
                        patches = [Image.fromarray(patch) for patch in pixels.cpu().numpy()]
                    for name, patch in zip(names, patches):
                        patch.save(str(name))
                else:
                    if pixel_path == "pil":
                        import numpy
                        import torch
                        stacked = numpy.stack([numpy.asarray(patch, dtype=numpy.uint8) for patch in patches])
                        pixels = torch.from_numpy(stacked).pin_memory().to(device, non_blocking=True)
                    entry = (names,) + tuple(encode_pairs_on_device(pixels, lambda: None))
                    flush(pending)
                    pending = entry
                patch_paths.extend(str(name.relative_to(destination)) for name in names)
                idx += 1
            if idx >= num_files_to_use:
                break
        flush(pending)
        pending = None
    finally:
        pages.close()
        if writers is not None:
            writers.close()   # drained here: before the caller writes the split files, and on every way out
    return patch_paths


def main(args: argparse.Namespace):
    resolve_paths(args)   # declines what is not built (--margin-remove off the device path) before anything is written
    seed = getattr(args, "seed", None)
    rng = random.Random(seed) if seed is not None else random
    root_dir = Path(args.root_dir)
    destination = Path(args.destination)
    destination.mkdir(exist_ok=True, parents=True)

    if not args.only_jsons:
        patch_paths = cut_patches(args, root_dir, destination, rng)
    else:   # list what the destination already holds
        patch_paths = [str(path.relative_to(destination)) for path in list_images(destination, "**/*")[:args.max_num_samples]]

    rng.shuffle(patch_paths)
    cut = int(len(patch_paths) * 0.9)   # 90 % train, the rest validation
    train_patches, validation_patches = patch_paths[:cut], patch_paths[cut:]
    for name, listed in (("train.json", train_patches), ("val.json", validation_patches)):
        with (destination / name).open("w") as f:
            json.dump(listed, f)
    return train_patches, validation_patches


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description="Cut GAN training patches from a directory of document scans")
    parser.add_argument("root_dir", help="directory that holds the scans (searched recursively)")
    parser.add_argument("destination", help="directory the patches, train.json and val.json are written to")
    parser.add_argument("max_num_samples", type=int, help="use at most this many scans")
    parser.add_argument("--image-size", type=int, default=256, help="side of the square patches")
    parser.add_argument("--only-jsons", action='store_true', default=False, help="cut nothing: write the two lists from the patches the destination already holds")
    parser.add_argument("--max-size", type=int, default=3000, help="a scan with a longer side is shrunk to this side first")
    parser.add_argument("--margin-remove", action='store_true', default=False,
                        help="crop the scanner margin off every page first (the reference does it with OpenCV's Canny and findContours; here "
                        "--pixel-path device does it with the kernels of csrc/scan_margin.h, DESIGN.md §20; --pixel-path pil raises)")
    parser.add_argument("--filter", help="use only scans whose path contains this expression")
    parser.add_argument("--seed", type=int, default=None, help="seed of the host random stream: the shuffle of the files, the downsample "
                        "factor 1..4 of every page, the shuffle before the 90/10 split")
    parser.add_argument("--min-size", type=int, default=1000, help="a page is not shrunk below this longer side (the constant inside the "
                        "reference's random_resize)")
    parser.add_argument("--pixel-path", choices=PIXEL_PATHS, default="device", help="device: shrink and cut the pages with the kernels of "
                        "csrc/scan_patches.h (Pillow's pixels, byte for byte); pil: Pillow on the host.  Files are decoded in full on both "
                        "paths, so JPEG sources that shrink 2x or more differ from the reference, which lets Pillow decode them at a DCT scale")
    parser.add_argument("--png-encoder", choices=PNG_ENCODERS, default=None, help="device: sis_hip.png_encode_pairs, the host only writes "
                        "files (default with --pixel-path device); pil: Pillow's save (default with --pixel-path pil)")
    parser.add_argument("--decode-workers", type=decode_worker_count, default=8, help="host threads that decode files (at most 16)")
    parser.add_argument("--png-writers", type=int, default=4, help="file-writer threads of --png-encoder device (at most 8)")
    return parser


if __name__ == "__main__":
    main(build_parser().parse_args())
