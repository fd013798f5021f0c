"""Evaluate a trained segmenter on document pages (reference: segmentation/evaluation/analyze_image_segments.py).

For every hyper-parameter combination (minimum confidence x minimum contour area x patch overlap) every page is segmented by
``VotingAssemblySegmenter`` and compared with its ground-truth class map; ``results.json`` holds, per run, the pages' confusion
matrices, the per-page and the accumulated scores and the hyper-parameters, in the layout the reference's table printer reads.

Where the work happens differs from the reference: the page, its patches, the post-processing (confidence threshold and
small-contour removal), the vote, the ground-truth class map and the confusion matrices stay on the device, and one run copies
its matrices to the host once.  ``main`` is a thin layer of file handling over ``evaluate_pages``.

The drawing half of the reference tool (``-vis``, bounding boxes, contour export, overlays) is a command of its own,
``python -m segmentation.evaluation.segmentation_visualization``, which takes the same flags; here those flags
raise.
"""
import argparse
import itertools
import json
from pathlib import Path
from typing import Dict, Iterable, Mapping, Sequence

import numpy
import torch

from segmentation.evaluation.segmentation_metric_calculation import (IMPLEMENTED_METRICS, calculate_confusion_matrix,
                                                                     calculate_metric)

VISUAL_FLAGS = ("visualize_segmentation", "extract_bboxes", "draw_patches", "draw_bboxes_on_segmentation", "save_bboxes",
                "save_contours", "show_confidence", "overlay_segmentation")
IMAGE_SUFFIXES = {".png", ".jpg", ".jpeg", ".bmp", ".tif", ".tiff", ".gif", ".webp"}


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(
        description="Analyze the given images using the specified segmentation model: dice score, intersection over union, "
                    "precision and recall against ground-truth images.",
        formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    mode = parser.add_argument_group("Management of evaluation modes")
    mode.add_argument("-cds", "--calculate-dice-score", action="store_true", default=False)
    mode.add_argument("-cio", "--calculate-iou", action="store_true", default=False)
    mode.add_argument("-cpr", "--calculate-precision", action="store_true", default=False)
    mode.add_argument("-cre", "--calculate-recall", action="store_true", default=False)
    mode.add_argument("-vis", "--visualize-segmentation", action="store_true", default=False, help="see segmentation_visualization")

    files = parser.add_argument_group("File management")
    files.add_argument("image_dir", type=Path, help="directory that contains the images that should be analyzed")
    files.add_argument("-f", "--config-file", default="config.json", type=Path,
                       help="JSON file with the segmenter configuration: 'checkpoint' (a snapshot of the training, key "
                            "'segmentation_network'), 'class_to_color_map' (JSON file, class name -> colour), optionally "
                            "'max_image_size', 'batch_size', 'background_class_name'")
    files.add_argument("-op", "--original-config-path", type=Path, default=None,
                       help="YAML file of the segmenter's training (network, image_size, ...); default: "
                            "<checkpoint dir>/../config/config.yaml")
    files.add_argument("-gt", "--ground-truth-dir", type=Path, help="directory with <image stem>_gt.png ground-truth images")
    files.add_argument("-o", "--output-dir", default="images", type=Path)
    files.add_argument("--handle-existing", default="abort", type=str, choices=["abort", "append", "overwrite"],
                       help="what to do if there is already a results.json in the output directory")

    pre = parser.add_argument_group("Input image preprocessing")
    pre.add_argument("--resize", nargs=2, type=int, help="[height width]; -1 keeps the aspect ratio for that side")
    pre.add_argument("-bw", "--convert-to-black-white", action="store_true", default=False)

    hyper = parser.add_argument_group("Hyperparameter determination")
    overlap = hyper.add_mutually_exclusive_group()
    overlap.add_argument("--absolute-patch-overlap", nargs="+", type=int, default=[0])
    overlap.add_argument("--patch-overlap-factor", nargs="+", type=float, default=[0.0])
    hyper.add_argument("--min-confidence", nargs="+", type=float, default=[0.7])
    hyper.add_argument("--min-contour-area", nargs="+", type=int, default=[55])

    visual = parser.add_argument_group("Visual output determination (python -m segmentation.evaluation.segmentation_visualization)")
    for flag in ("--extract-bboxes", "--draw-patches", "--draw-bboxes-on-segmentation", "--save-bboxes", "--save-contours",
                 "--show-confidence", "--overlay-segmentation"):
        visual.add_argument(flag, action="store_true", default=False)
    return parser


def parse_and_check_arguments(argv=None) -> argparse.Namespace:
    args = build_parser().parse_args(argv)
    asked = [flag for flag in VISUAL_FLAGS if getattr(args, flag)]
    if asked:
        raise NotImplementedError("visualisation, bounding-box and contour export are not part of this command (use python -m "
                                  "segmentation.evaluation.segmentation_visualization, which takes the same flags): "
                                  f"{', '.join('--' + f.replace('_', '-') for f in asked)}")
    if not any(selected_metrics(args).values()):
        raise SystemExit("No metric selected (-cds, -cio, -cpr, -cre): there would be no output.")
    if args.ground_truth_dir is None:
        raise SystemExit("The metrics need --ground-truth-dir.")
    return args


def selected_metrics(args) -> Dict[str, bool]:
    return {"dice": args.calculate_dice_score, "iou": args.calculate_iou, "precision": args.calculate_precision,
            "recall": args.calculate_recall}


def create_hyperparam_configs(args) -> tuple:
    """Every combination of minimum confidence, minimum contour area and (absolute overlap, overlap factor), confidence
    slowest, overlap fastest."""
    overlaps = itertools.product(args.absolute_patch_overlap, args.patch_overlap_factor)
    return tuple({"min_confidence": confidence, "min_contour_area": area, "patch_overlap": overlap}
                 for confidence, area, overlap in itertools.product(args.min_confidence, args.min_contour_area, overlaps))


def prepare_results(handle_existing: str, output_json_path: Path, model_config: dict, segmenter_config: dict,
                    class_to_color_map: dict) -> dict:
    general = {"experiment_config": model_config, "model_config": segmenter_config, "class_to_color_map": class_to_color_map}
    if output_json_path.exists() and handle_existing != "overwrite":
        assert handle_existing != "abort", f"{output_json_path} already exists and --handle-existing is set to 'abort'"
        with open(output_json_path, "r") as old_json:
            results = json.load(old_json)
        for key, value in general.items():
            assert results["general_config"][key] == json.loads(json.dumps(value)), \
                f"The previously saved {key} does not match the current one. Use a new output dir instead of setting " \
                "--handle-existing to append."
        return results
    return {"general_config": general, "runs": []}


def evaluate_pages(segmenter, pages, ground_truths, class_names: Sequence[str], hyperparam_configs: Iterable[dict],
                   metrics: Iterable[str]) -> dict:
    """``{"runs": [...]}``: one entry of ``results.json``'s ``runs`` per hyper-parameter combination.

    ``pages``: name -> image (anything ``segmenter.segment_image`` takes) or a sequence of images (named by position);
    ``ground_truths``: the same names / positions -> uint8 [H, W] class maps on the segmenter's device.  A run keeps its
    confusion matrices on the device and copies them to the host together, once."""
    metrics = [m for m in metrics]
    for metric in metrics:
        assert metric in IMPLEMENTED_METRICS, f"Metric to calculate must be in {', '.join(IMPLEMENTED_METRICS)}"
    if not isinstance(pages, Mapping):
        pages = {str(i): page for i, page in enumerate(pages)}
    if not isinstance(ground_truths, Mapping):
        ground_truths = {str(i): gt for i, gt in enumerate(ground_truths)}
    num_classes = len(class_names)
    runs = []
    for config in hyperparam_configs:
        segmenter.set_hyperparams(config)
        total = torch.zeros((num_classes, num_classes), dtype=torch.int64, device=segmenter.device)
        per_page = []
        for name, page in pages.items():
            assembled = segmenter.segment_image(page)
            matrix = calculate_confusion_matrix(assembled, ground_truths[name], num_classes)
            total += matrix
            per_page.append(matrix)
        host = torch.stack(per_page + [total]).cpu()
        run = {"confusion_matrices": {}}
        for name, matrix in zip(pages, host[:-1]):
            run["confusion_matrices"][name] = [float(v) for v in matrix.reshape(-1).tolist()]
            for metric in metrics:
                run.setdefault(f"detailed_{metric}_scores", {})[name] = calculate_metric(matrix, class_names, metric)
        for metric in metrics:
            run[f"average_{metric}_scores"] = calculate_metric(host[-1], class_names, metric)
        run["hyperparams"] = config
        runs.append(run)
    return {"runs": runs}


def preprocess_image(image, args):
    if args.resize:
        from PIL import Image
        height, width = args.resize
        assert height > 0 or width > 0, "One of the given resize dimensions has to be greater than 0."
        if height == -1:
            height = int(width * image.height / image.width)
        elif width == -1:
            width = int(height * image.width / image.height)
        image = image.resize((width, height), Image.LANCZOS)
    if args.convert_to_black_white:
        image = image.convert("L")
    return image


def load_segmenter(model_config: dict, original_config_path, device="cuda"):
    """(VotingAssemblySegmenter, training config, class-to-colour map) from the tool's JSON config."""
    import yaml
    from segmentation.analysis_segmenter import VotingAssemblySegmenter
    from training_builder.base_train_builder import load_weights
    from training_builder.train_builder_selection import get_train_builder_class

    checkpoint = Path(model_config["checkpoint"])
    config_path = Path(original_config_path) if original_config_path else checkpoint.parent.parent / "config" / "config.yaml"
    with open(config_path) as f:
        config = yaml.safe_load(f)
    if config.get("network") == "base":   # old config files, where DocUFCN was the only model
        config["network"] = "DocUFCN"
    network = get_train_builder_class(config)(config).get_network()
    load_weights(network, checkpoint, key="segmentation_network")
    with open(model_config["class_to_color_map"]) as f:
        class_to_color_map = json.load(f)
    segmenter = VotingAssemblySegmenter(network.to(device), int(config["image_size"]), device,
                                        batch_size=int(model_config.get("batch_size", config.get("batch_size", 1))),
                                        max_image_size=int(model_config.get("max_image_size", 0)))
    return segmenter, config, class_to_color_map


def main(args: argparse.Namespace) -> None:
    from PIL import Image, UnidentifiedImageError
    from utils.segmentation_utils import segmentation_image_to_class_image

    with args.config_file.open() as f:
        model_config = json.load(f)
    segmenter, config, class_to_color_map = load_segmenter(model_config, args.original_config_path)
    class_names = list(class_to_color_map.keys())
    num_classes = config.get("num_classes", getattr(segmenter.network, "num_classes", len(class_names)))
    assert len(class_names) == num_classes, "Number of classes in color map and segmenter differs."
    background = model_config.get("background_class_name", "background")

    args.output_dir.mkdir(parents=True, exist_ok=True)
    output_json_path = args.output_dir / "results.json"
    results = prepare_results(args.handle_existing, output_json_path, model_config, config, class_to_color_map)

    pages, ground_truths = {}, {}
    for path in sorted(p for p in args.image_dir.glob("**/*") if p.suffix.lower() in IMAGE_SUFFIXES):
        try:
            image = Image.open(path)
            image.load()
        except UnidentifiedImageError:
            print(f"File {path} is not an image.")
            continue
        gt_path = args.ground_truth_dir / f"{path.stem}_gt.png"
        assert gt_path.exists(), f"The following ground truth image does not exist: {gt_path}. Is it a png?"
        page = segmenter._page_tensor(preprocess_image(image, args))
        gt = torch.from_numpy(numpy.array(Image.open(gt_path).convert("RGB")))
        classes = segmentation_image_to_class_image(gt, background, class_to_color_map, device=segmenter.device)
        if tuple(classes.shape) != tuple(page.shape[:2]):
            print(f"Shapes of prediction and ground truth do not match; {path} will be skipped.")
            continue
        pages[path.stem], ground_truths[path.stem] = page, classes
    assert len(pages) > 0, "There are no images in the given directory."

    metrics = [name for name, selected in selected_metrics(args).items() if selected]
    for config_ in create_hyperparam_configs(args):   # one run at a time: results.json is complete after every run
        results["runs"] += evaluate_pages(segmenter, pages, ground_truths, class_names, [config_], metrics)["runs"]
        with open(output_json_path, "w") as out_json:
            json.dump(results, out_json, indent=4)


if __name__ == "__main__":
    main(parse_and_check_arguments())
