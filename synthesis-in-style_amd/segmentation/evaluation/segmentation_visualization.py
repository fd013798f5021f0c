"""What a user of the segmenter looks at (reference: segmentation/evaluation/segmentation_visualization.py and the visual
flags of analyze_image_segments.py): the colour-coded page, its overlay on the scan, the bounding boxes of the text regions and
the cut-out regions, under the reference's function and file names.

Where the work happens differs from the reference, which runs ``cv2.findContours`` per class, a Python loop per pixel for
``--show-confidence`` and PIL drawing on the host.  Here one ``sis_hip.page_regions`` call finds every region of the assembled
page with its box and area, one ``sis_hip.page_render`` call colours the page, overlays it and draws the outlines, and one
``sis_hip.page_crops`` call per mode cuts the regions out (csrc/page_visual.h, DESIGN.md §17 states the contract).  The region
tables come to the host once per page -- the file names need them -- and the images are written as RGB PNG through PIL.

Differences that show in the output:

* Regions are listed in the order of their first pixel (smallest ``y * width + x``), the reference's in OpenCV's contour order:
  the ``i`` in ``..._bbox_<i>.png`` / ``..._contour_<i>.png`` numbers the same regions differently.
* The overlay and the boxes are drawn on the page the segmenter saw (after ``--resize`` / ``-bw`` and the segmenter's
  thumbnailing, grey shown as RGB).  The reference indexes the untouched original with the prediction's coordinates, which only
  works when the sizes agree; it warns when they differ, and so does this module.
* A box thinner than the stroke is filled; PIL's ``rectangle`` paints outside such a box.
* Contour crops are written through PIL as RGB PNG like every other picture (the reference writes them with ``cv2.imwrite``).

Not pinned against OpenCV: regions that touch the page's edge and degenerate regions.

    python -m segmentation.evaluation.segmentation_visualization <image_dir> -f config.json -o out --extract-bboxes ...
"""
import argparse
import json
import re
import warnings
from pathlib import Path
from typing import Dict, List, Optional, Tuple, Union

import numpy
import torch

import sis_hip
from utils.segmentation_utils import BBox

Color = Tuple[int, int, int]
MIN_CONTOUR_AREA = 10   # find_class_contours' default (reference utils/segmentation_utils.py:105), which the visual half uses


def _rgb(color) -> Color:
    if isinstance(color, str):
        from PIL import ImageColor
        color = ImageColor.getrgb(color)
    return tuple(int(v) for v in color)[:3]


def page_palette(segmenter):
    """(colours [classes][3], background class id, confidence table on the device or None) of a segmenter; the table is built
    and uploaded once per segmenter and colour map."""
    color_map = segmenter.class_to_color_map
    if not color_map:
        raise ValueError("the segmenter has no class_to_color_map")
    colours = [_rgb(c) for c in color_map.values()]
    background = list(color_map).index("background")
    if not segmenter.show_confidence_in_segmentation:
        return colours, background, None
    cached = getattr(segmenter, "_confidence_table", None)
    if cached is None or cached[0] != colours:
        table = torch.tensor(sis_hip.page_confidence_table(colours), dtype=torch.uint8).to(segmenter.device)
        cached = segmenter._confidence_table = (colours, table)
    return colours, background, cached[1]


class PageRegionTables:
    """The regions of one assembled page: ``device`` (a ``sis_hip.PageRegions``) and ``rows``, per class the int32 [n, 8] host
    copy of its table (root, x0, y0, w, h, twice_area, kept, 0) in root order."""

    def __init__(self, device, rows):
        self.device, self.rows = device, rows

    def kept(self, class_id: int) -> numpy.ndarray:
        table = self.rows[class_id]
        return table[table[:, 6] != 0]

    def bounding_boxes(self) -> Dict[int, List[BBox]]:
        boxes = {}
        for class_id in range(len(self.rows)):
            kept = self.kept(class_id)
            if len(kept):   # the reference's dict has no entry for a class without contours
                boxes[class_id] = [BBox.from_opencv_bounding_rect(*(int(v) for v in row[1:5])) for row in kept]
        return boxes


def find_page_regions(prediction: torch.Tensor, filter_classes: Tuple[int, ...] = (), background_class_id: int = 0,
                      labels: bool = False) -> PageRegionTables:
    """``find_class_contours`` + ``cv2.boundingRect`` of the reference on the device; the tables are copied to the host once.
    A page with more regions in a plane than the default capacity is labelled a second time with room for all of them."""
    found = sis_hip.page_regions(prediction, background_class_id, filter_classes, MIN_CONTOUR_AREA, labels=labels)
    counts = found.region_count.cpu().numpy()
    if counts.max() > found.regions.shape[1]:
        found = sis_hip.page_regions(prediction, background_class_id, filter_classes, MIN_CONTOUR_AREA,
                                     max_regions=int(counts.max()), labels=labels)
    host = found.regions.cpu().numpy()
    return PageRegionTables(found, [host[k, :counts[k]] for k in range(host.shape[0])])


def get_bounding_boxes(prediction: torch.Tensor, filter_classes: Tuple = ()) -> Dict[int, List[BBox]]:
    """Class id -> boxes (x, y, x + w, y + h) of the regions of at least ``MIN_CONTOUR_AREA``, in root order."""
    return find_page_regions(prediction, filter_classes).bounding_boxes()


def _page_tensor(image, device) -> torch.Tensor:
    """uint8 [H, W, 1 or 3] on the device from a PIL image (grey stays one channel), an array or a tensor."""
    if hasattr(image, "convert"):
        image = numpy.array(image if image.mode in ("L", "RGB") else image.convert("RGB"))
    page = torch.as_tensor(image)
    if page.dim() == 2:
        page = page.unsqueeze(-1)
    return page.to(device).contiguous()


def _to_pil(image: torch.Tensor):
    from PIL import Image
    return Image.fromarray(image.cpu().numpy())


def _patch_box_tensor(bboxes_for_patches, device) -> Optional[torch.Tensor]:
    if bboxes_for_patches is None or len(bboxes_for_patches) == 0:
        return None
    return torch.tensor([list(box) for box in bboxes_for_patches], dtype=torch.int32).to(device)


def save_overlayed_segmentation_image(segmented_image, original_image, class_to_color_map: dict, image_save_dir: Path,
                                      image_prefix: str, overlay: Optional[torch.Tensor] = None) -> None:
    """Writes ``<prefix>_overlayed.png``.  ``visualize_segmentation`` hands in the ``overlay`` that ``sis_hip.page_render``
    made; called with two images only, as in the reference (:22-32), the pixels are chosen on the host."""
    from PIL import Image
    if overlay is not None:
        overlayed = _to_pil(overlay)
    else:
        segmented = numpy.array(segmented_image.convert("RGB"))
        original = numpy.array(original_image.convert("RGB"))
        coloured = (segmented != numpy.asarray(_rgb(class_to_color_map["background"]), dtype=numpy.uint8)).any(axis=2)
        original[coloured] = segmented[coloured]
        overlayed = Image.fromarray(original)
    overlayed.save(Path(image_save_dir) / f"{image_prefix}_overlayed.png")


def draw_segmentation(original_image, assembled_predictions: torch.Tensor, original_segmented_image,
                      bboxes_for_patches: Union[Tuple[BBox], None] = None, filter_classes: Tuple[int, ...] = (),
                      return_bboxes: bool = False, regions: Optional[PageRegionTables] = None):
    """(image with boxes, segmented image with boxes[, class id -> boxes]): region boxes in green, stroke 3, then the patch
    boxes in red, stroke 1, drawn by ``sis_hip.page_render`` on both images (reference :55-78)."""
    if original_image.size != original_segmented_image.size:
        warnings.warn("Sizes of original_image and original_segmented_image do not match. It could be that there is "
                      "something wrong with the preprocessing of these images.")
    device = assembled_predictions.device
    if regions is None:
        regions = find_page_regions(assembled_predictions, filter_classes)
    patch_boxes = _patch_box_tensor(bboxes_for_patches, device)
    colours = [(0, 0, 0)] * assembled_predictions.shape[0]   # only the outlines are taken from these two calls
    drawn = []
    for base in (original_image, original_segmented_image):
        rendered = sis_hip.page_render(assembled_predictions, _page_tensor(base, device), colours, regions=regions.device.regions,
                                       region_count=regions.device.region_count, patch_boxes=patch_boxes,
                                       outputs=("boxes_on_page",))
        drawn.append(_to_pil(rendered.boxes_on_page))
    if return_bboxes:
        return drawn[0], drawn[1], regions.bounding_boxes()
    return drawn[0], drawn[1]


def _save_crops(image, regions: PageRegionTables, directory: Path, image_prefix: str, mode: str, kind: str) -> None:
    from PIL import Image
    directory.mkdir(exist_ok=True)
    rows, names = [], []
    for class_id in range(len(regions.rows)):
        for i, row in enumerate(regions.kept(class_id)):
            rows.append((class_id, *(int(v) for v in row[:5])))
            names.append(directory / f"{image_prefix}_class_{class_id}_{kind}_{i}.png")
    if not rows:
        return
    device = regions.device.region_count.device
    packed, offsets = sis_hip.page_crops(_page_tensor(image, device), rows, mode, regions.device.region_labels)
    host = packed.cpu().numpy()
    for (_, _, _, _, w, h), offset, name in zip(rows, offsets, names):
        Image.fromarray(host[offset:offset + 3 * w * h].reshape(h, w, 3)).save(name)


def extract_and_save_bounding_boxes(image, assembled_predictions: torch.Tensor, output_dir: Path, image_prefix: str,
                                    filter_classes: Tuple[int, ...] = (), regions: Optional[PageRegionTables] = None) -> None:
    """``bboxes/<prefix>_class_<c>_bbox_<i>.png``: the page cut to every kept region's box (reference :88-96)."""
    if regions is None:
        regions = find_page_regions(assembled_predictions, filter_classes)
    _save_crops(image, regions, Path(output_dir) / "bboxes", image_prefix, "bbox", "bbox")


def extract_and_save_contours(image, assembled_predictions: torch.Tensor, output_dir: Path, image_prefix: str,
                              regions: Optional[PageRegionTables] = None) -> None:
    """``contours/<prefix>_class_<c>_contour_<i>.png``: the page inside every kept region's filled outer contour, white
    around it (reference :99-133)."""
    if regions is None or regions.device.region_labels is None:
        regions = find_page_regions(assembled_predictions, labels=True)
    _save_crops(image, regions, Path(output_dir) / "contours", image_prefix, "contour", "contour")


def visualize_segmentation(assembled_prediction: torch.Tensor, image, original_image, segmenter, args: argparse.Namespace,
                           class_to_color_map: Dict, image_prefix: str) -> None:
    """Every picture the visual flags ask for, below ``<output_dir>/images`` (reference :136-166): one region call, one
    render call and one crop call per mode for the page."""
    image_save_dir = Path(args.output_dir) / "images"
    image_save_dir.mkdir(exist_ok=True, parents=True)
    if segmenter.class_to_color_map is None:
        segmenter.class_to_color_map = class_to_color_map
    page = segmenter._page_tensor(image)   # the page the segmenter saw
    if hasattr(original_image, "size") and tuple(original_image.size) != (page.shape[1], page.shape[0]):
        warnings.warn("Sizes of original_image and original_segmented_image do not match. It could be that there is "
                      "something wrong with the preprocessing of these images.")
    colours, background, table = page_palette(segmenter)
    need_regions = args.extract_bboxes or args.save_bboxes or args.save_contours
    regions = find_page_regions(assembled_prediction, labels=bool(args.save_contours)) if need_regions else None
    outputs = ["segmented"]
    if args.overlay_segmentation:
        outputs.append("overlay")
    patch_boxes = None
    if args.extract_bboxes:
        outputs.append("boxes_on_page")
        if args.draw_bboxes_on_segmentation:
            outputs.append("boxes_on_segmented")
        if args.draw_patches:
            patch_boxes = _patch_box_tensor(segmenter.calculate_bboxes_for_patches(page.shape[1], page.shape[0]), page.device)
    rendered = sis_hip.page_render(assembled_prediction, page, colours, background_class_id=background, confidence_table=table,
                                   regions=regions.device.regions if args.extract_bboxes else None,
                                   region_count=regions.device.region_count if args.extract_bboxes else None,
                                   patch_boxes=patch_boxes, outputs=tuple(outputs))
    segmented_image = _to_pil(rendered.segmented)
    segmented_image.save(image_save_dir / f"{image_prefix}_segmented_no_bboxes.png")
    if args.overlay_segmentation:
        save_overlayed_segmentation_image(segmented_image, original_image, class_to_color_map, image_save_dir, image_prefix,
                                          overlay=rendered.overlay)
    if args.extract_bboxes:
        _to_pil(rendered.boxes_on_page).save(image_save_dir / f"{image_prefix}_bboxes.png")
        if args.draw_bboxes_on_segmentation:
            _to_pil(rendered.boxes_on_segmented).save(image_save_dir / f"{image_prefix}_segmented.png")
    if args.save_bboxes:
        extract_and_save_bounding_boxes(page, assembled_prediction, image_save_dir, image_prefix, regions=regions)
    if args.save_contours:
        extract_and_save_contours(page, assembled_prediction, image_save_dir, image_prefix, regions=regions)


# ---- command line -----------------------------------------------------------------------------------------------------------------
def get_string_representation_of_config(hyperparam_config: dict) -> str:
    """{"min_confidence": 0.7, "patch_overlap": (0, 0.5)} -> min_confidence_0_7_patch_overlap_0__0_5 (reference
    analyze_image_segments.py:175-180): the part of the file names that tells the runs apart."""
    return "_".join(re.sub(r"[,\s.]", "_", re.sub("[()]", "", f"{k}_{v}")) for k, v in hyperparam_config.items())


def parse_and_check_arguments(argv=None) -> argparse.Namespace:
    """The reference tool's file, preprocessing, hyper-parameter and visual flags; ``-vis`` is implied."""
    from segmentation.evaluation.analyze_image_segments import build_parser
    parser = build_parser()
    parser.prog = "python -m segmentation.evaluation.segmentation_visualization"
    parser.description = "Visualize the segmentation of the given images: colour-coded pages, overlays, bounding boxes and " \
                         "cut-out regions of the text the specified segmentation model finds."
    args = parser.parse_args(argv)
    args.visualize_segmentation = True
    return args


def main(args: argparse.Namespace) -> None:
    from PIL import Image, UnidentifiedImageError
    from segmentation.evaluation.analyze_image_segments import (IMAGE_SUFFIXES, create_hyperparam_configs, load_segmenter,
                                                                preprocess_image)
    with args.config_file.open() as f:
        model_config = json.load(f)
    segmenter, _, class_to_color_map = load_segmenter(model_config, args.original_config_path)
    segmenter.class_to_color_map = class_to_color_map
    segmenter.show_confidence_in_segmentation = args.show_confidence
    image_paths = sorted(p for p in args.image_dir.glob("**/*") if p.suffix.lower() in IMAGE_SUFFIXES)
    assert len(image_paths) > 0, "There are no images in the given directory."
    for hyperparam_config in create_hyperparam_configs(args):
        segmenter.set_hyperparams(hyperparam_config)
        for image_path in image_paths:
            try:
                original_image = Image.open(image_path)
                original_image.load()
            except UnidentifiedImageError:
                print(f"File {image_path} is not an image.")
                continue
            image = preprocess_image(original_image, args)
            assembled_prediction = segmenter.segment_image(image)
            image_prefix = f"{image_path.stem}_{get_string_representation_of_config(hyperparam_config)}"
            visualize_segmentation(assembled_prediction, image, original_image, segmenter, args, class_to_color_map, image_prefix)


if __name__ == "__main__":
    main(parse_and_check_arguments())
