"""Ground truth of a directory of ``[image | label]`` PNG pairs: which classes an image holds (the ``has_<class>`` keys of
train.json / val.json) and COCO annotations (``coco_gt.json``), with the names of the reference's
segmentation/evaluation/coco_gt.py.

Per annotated class (every entry of ``class_to_color_map`` but ``background``) the label half is compared with the class colour
and the outermost contours of that mask, holes filled, become one annotation each: RLE, area and bbox.  The regions, their
boxes, areas and run lengths come from ``sis_hip.label_regions`` (csrc/coco_gt.h, DESIGN.md §16 states the contract); the host
decodes the PNGs, turns run lengths into COCO's compressed strings with numpy and assembles the JSON.  There is no host
implementation of the regions: without a device the default provider raises.  The contract is stated exactly and tested against
an independent restatement; it is NOT pinned against OpenCV's ``findContours`` or ``pycocotools`` (the reference rasterises the
contour polygon, which can differ from the filled region by boundary pixels, and ``findContours`` treats plane-edge pixels in
its own way).

A region provider is a callable ``(label uint8 [B, p, p, 3] numpy, colours [[r, g, b]], runs: bool) -> (has, tables, runs)``:
``has`` [B][K] truth values, ``tables[b][k]`` the int rows (root, x0, y0, w, h, area, run_offset, run_count) of plane (b, k) and
``runs[b][k]`` its concatenated counts (None without ``runs``).

CLI: ``python -m segmentation.evaluation.coco_gt image_root class_to_color_map.json`` writes ``image_root/coco_gt.json``.
"""
import argparse
import datetime
import json
from pathlib import Path
from typing import Dict, Iterable, List, Tuple

import numpy

DEFAULT_BATCH = 32


# ---- COCO's compressed RLE string (rleToString / rleFrString of the published cocoapi) ------------------------------------------
def coco_rle_string(counts, lengths=None):
    """Run lengths -> COCO's compressed string.  ``counts``: the concatenated counts of any number of RLEs, ``lengths``: how many
    counts each RLE has (None: one RLE; a single string is returned).  Works on all counts at once: per count, from the third
    on, the difference to the count two before is written in 5-bit groups, low group first, bit 5 flags a continuation and bit
    4 of the last group is the sign."""
    given = numpy.asarray(counts, dtype=numpy.int64).ravel()
    single = lengths is None
    lengths = numpy.asarray([given.size] if single else lengths, dtype=numpy.int64).ravel()
    if int(lengths.sum()) != given.size:
        raise ValueError(f"{given.size} counts for RLEs of {int(lengths.sum())} counts in all")
    starts = numpy.cumsum(lengths) - lengths
    within = numpy.arange(given.size, dtype=numpy.int64) - numpy.repeat(starts, lengths)
    x = given.copy()
    late = numpy.nonzero(within > 2)[0]
    x[late] -= given[late - 2]
    groups = 13   # 64 bits in groups of five
    chars = numpy.zeros((x.size, groups), dtype=numpy.uint8)
    used = numpy.zeros((x.size, groups), dtype=bool)
    active = numpy.ones(x.size, dtype=bool)
    for g in range(groups):
        if not active.any():
            break
        c = x & 0x1F
        x = x >> 5   # arithmetic
        more = numpy.where((c & 0x10) != 0, x != -1, x != 0)
        chars[:, g] = numpy.where(more, c | 0x20, c) + 48
        used[:, g] = active
        active = active & more
    text = chars[used].tobytes().decode("ascii")   # row-major: count after count, group after group
    first_char = numpy.concatenate([[0], numpy.cumsum(used.sum(axis=1))])   # of every count, and the end behind the last
    out = [text[int(first_char[s]):int(first_char[s + n])] for s, n in zip(starts, lengths)]
    return out[0] if single else out


def coco_rle_counts(text: str) -> List[int]:
    """The inverse of ``coco_rle_string`` for one RLE."""
    counts, at = [], 0
    while at < len(text):
        x, k, more = 0, 0, True
        while more:
            c = ord(text[at]) - 48
            x |= (c & 0x1F) << (5 * k)
            more = bool(c & 0x20)
            at += 1
            k += 1
            if not more and c & 0x10:
                x |= -1 << (5 * k)
        if len(counts) > 2:
            x += counts[-2]
        counts.append(x)
    return counts


# ---- region providers ----------------------------------------------------------------------------------------------------------
def device_regions(label, colours, runs=True):
    """The default provider: ``sis_hip.label_regions`` on the current HIP device, one upload, one call, and one copy of the used
    prefixes behind a copy of the totals."""
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("coco_gt: the regions are computed on a HIP device and none is available (there is no host path)")
    import sis_hip
    if not isinstance(label, torch.Tensor):   # (a tensor: label images that are resident on the device already)
        label = torch.from_numpy(numpy.ascontiguousarray(label)).cuda()
    result = sis_hip.label_regions(label, colours, runs=runs)
    small = torch.stack([result.has.to(torch.int32), result.region_count, result.run_total]).cpu().numpy()
    has, region_count, run_total = small[0], small[1], small[2]
    rows = result.regions[:, :, :max(int(region_count.max()), 1)].cpu().numpy()
    counts = result.runs[:, :, :max(int(run_total.max()), 1)].cpu().numpy() if runs else None
    b, k = has.shape
    tables = [[rows[i, j, :region_count[i, j]] for j in range(k)] for i in range(b)]
    seqs = [[counts[i, j, :run_total[i, j]] for j in range(k)] for i in range(b)] if runs else None
    return has, tables, seqs


class COCOGtCreator:

    def __init__(self, class_to_color_map: Dict, image_root: Path = Path('/'), region_provider=None, batch_size: int = DEFAULT_BATCH):
        from PIL import ImageColor
        self.class_to_color_map = class_to_color_map
        self.categories = self.build_categories()
        self.image_root = Path(image_root)
        self.region_provider = device_regions if region_provider is None else region_provider
        self.batch_size = max(1, int(batch_size))
        # the annotated classes, in map order: (category id with the background counted, name, rgb)
        self.annotated = [(category_id, name, tuple(ImageColor.getrgb(color))[:3])
                          for category_id, (name, color) in enumerate(class_to_color_map.items()) if name != 'background']
        self.colours = [list(rgb) for _, _, rgb in self.annotated]

    def build_categories(self) -> List[dict]:
        return [{"id": category_id, "name": name, "supercategory": name, "color": color}
                for category_id, (name, color) in enumerate(self.class_to_color_map.items())]

    @staticmethod
    def get_label_image(image_data) -> numpy.ndarray:
        """The right half of a pair as uint8 [p, p, 3]."""
        pair = numpy.asarray(image_data.convert("RGB") if hasattr(image_data, "convert") else image_data)
        if pair.ndim != 3 or pair.shape[2] != 3 or pair.shape[1] != 2 * pair.shape[0]:
            raise ValueError(f"the label half of a {pair.shape[1]} x {pair.shape[0]} pair is not square")
        return numpy.ascontiguousarray(pair[:, pair.shape[1] // 2:])

    # -- class listing
    def classes_from_has(self, has_row) -> Dict[str, bool]:
        return {f"has_{name}": bool(flag) for (_, name, _), flag in zip(self.annotated, has_row)}

    def determine_classes_in_label_images(self, labels: numpy.ndarray) -> List[Dict[str, bool]]:
        """uint8 [B, p, p, 3] label halves -> one ``{"has_<class>": bool}`` per image (one provider call, listing mode)."""
        if not self.annotated:
            return [{} for _ in range(len(labels))]
        has, _, _ = self.region_provider(labels, self.colours, False)
        return [self.classes_from_has(row) for row in has]

    def determine_classes_in_image(self, image_data) -> Dict[str, bool]:
        return self.determine_classes_in_label_images(self.get_label_image(image_data)[None])[0]

    def determine_classes_in_images(self, image_paths: Iterable[Path]) -> List[Dict[str, bool]]:
        """The batched form over PNG files; images of different sizes go to different calls."""
        out = []
        for _, _, labels in self.batches(image_paths):
            out.extend(self.determine_classes_in_label_images(labels))
        return out

    # -- annotations
    def annotations_of_label_images(self, labels: numpy.ndarray, first_image_id: int, annotation_id: int) -> Tuple[List[dict], int]:
        """uint8 [B, p, p, 3] -> the annotations of images first_image_id .., classes in map order, regions in root order."""
        annotations = []
        if not self.annotated or len(labels) == 0:
            return annotations, annotation_id
        p = int(labels.shape[1])
        _, tables, runs = self.region_provider(labels, self.colours, True)
        kept, counts, lengths = [], [], []
        for b in range(len(labels)):
            for k, (category_id, _, _) in enumerate(self.annotated):
                rows = numpy.asarray(tables[b][k]).reshape(-1, 8)
                rows = rows[rows[:, 7] > 0]
                if len(rows):   # the kept regions' counts lie one after the other in the plane's run array
                    kept.extend((first_image_id + b, category_id, row) for row in rows)
                    counts.append(numpy.asarray(runs[b][k], dtype=numpy.int64)[:int(rows[-1, 6] + rows[-1, 7])])
                    lengths.append(rows[:, 7])
        if not kept:
            return annotations, annotation_id
        strings = coco_rle_string(numpy.concatenate(counts), numpy.concatenate(lengths))
        for (image_id, category_id, row), text in zip(kept, strings):
            annotations.append({
                "id": annotation_id,
                "image_id": image_id,
                "category_id": category_id,
                "segmentation": {"size": [p, p], "counts": text},
                "area": int(row[5]),
                "bbox": [float(row[1]), float(row[2]), float(row[3]), float(row[4])],
                "iscrowd": 0,
            })
            annotation_id += 1
        return annotations, annotation_id

    def build_annotations_for_image(self, image_data, image_id: int, annotation_id: int) -> Tuple[List[dict], int]:
        return self.annotations_of_label_images(self.get_label_image(image_data)[None], image_id, annotation_id)

    def batches(self, image_paths: Iterable[Path]):
        """(paths, PNG sizes, uint8 [B, p, p, 3]) of consecutive files of one size, ``batch_size`` at most."""
        from PIL import Image
        paths, sizes, labels = [], [], []
        for path in image_paths:
            with Image.open(str(path)) as the_image:
                size = (the_image.width, the_image.height)
                label = self.get_label_image(the_image)
            if labels and (label.shape != labels[0].shape or len(labels) == self.batch_size):
                yield paths, sizes, numpy.stack(labels)
                paths, sizes, labels = [], [], []
            paths.append(Path(path))
            sizes.append(size)
            labels.append(label)
        if labels:
            yield paths, sizes, numpy.stack(labels)

    def create_coco_gt_from_image_paths(self, image_paths: Iterable[Path]) -> dict:
        images, annotations, annotation_id = [], [], 0
        for paths, sizes, labels in self.batches(image_paths):
            first = len(images)
            for path, (width, height) in zip(paths, sizes):
                images.append({
                    "id": len(images),
                    "width": width // 2,
                    "height": height,
                    "file_name": str(path.relative_to(self.image_root)),
                    "license": 0,
                    "flickr_url": "",
                    "coco_url": "",
                    "date_captured": str(datetime.datetime.utcnow()),
                })
            found, annotation_id = self.annotations_of_label_images(labels, first, annotation_id)
            annotations.extend(found)
        return {
            "info": {"year": datetime.date.today().year, "version": "1",
                     "description": "COCO GT for evaluation of semantic segmentation", "contributor": "yourself",
                     "url": "http://example.com"},
            "images": images,
            "annotations": annotations,
            "categories": self.categories,
            "licenses": [{"id": 0, "name": "none", "url": "http://example.com"}],
        }


def iter_through_images_in(image_root: Path, extension: str = 'png') -> Iterable[Path]:
    """Sorted, so that image ids do not depend on the file system."""
    return sorted(Path(image_root).glob(f'**/*.{extension}'))


def create_coco_gt_from_image_root(image_root: Path, class_to_color_map, region_provider=None):
    """``class_to_color_map``: the map itself or the path of a JSON file that holds it (or a config with that key)."""
    image_root = Path(image_root)
    if not isinstance(class_to_color_map, dict):
        with open(class_to_color_map) as f:
            class_to_color_map = json.load(f)
        class_to_color_map = class_to_color_map.get('class_to_color_map', class_to_color_map)
    creator = COCOGtCreator(class_to_color_map, image_root=image_root, region_provider=region_provider)
    coco_gt = creator.create_coco_gt_from_image_paths(iter_through_images_in(image_root))
    with (image_root / 'coco_gt.json').open('w') as f:
        json.dump(coco_gt, f)
    return coco_gt


if __name__ == "__main__":
    parser = argparse.ArgumentParser("Provide an Image Root with Segmentation images and create COCO GT")
    parser.add_argument("image_root")
    parser.add_argument("class_to_color_map")
    args = parser.parse_args()
    create_coco_gt_from_image_root(Path(args.image_root), Path(args.class_to_color_map))
