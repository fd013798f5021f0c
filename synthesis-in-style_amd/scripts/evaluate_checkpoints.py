"""Reconstruction quality of trained autoencoder checkpoints over datasets (reference: scripts/evaluate_checkpoints.py, same
command line and result files).

    python scripts/evaluate_checkpoints.py checkpoints.txt datasets.json [--skip-fid] [--skip-reconstruction] [--batch-size 32]

``checkpoints.txt`` lists one checkpoint per line (``<run>/checkpoints/<name>``, the run's ``config/{config,args}.json`` beside
it); ``datasets.json`` is a list of ``{"name": ..., "test": <image list>, "train": <image list>}``.  Each (checkpoint, dataset)
pair adds ``{checkpoint name: {dataset name: {"psnr": ..., "ssim": ...}}}`` to ``<run>/evaluation/reconstruction.json``; a pair
that file already holds is skipped.

The reference scores one image per step and reads two numbers back each time.  Here the test images are resident on the device
(``data.autoencoder_dataset``), a step reconstructs ``--batch-size`` of them and scores every one with a single
``PSNRSSIMEvaluator.psnr_and_ssim_batch`` call; the per-image values stay on the device and are read back once per dataset.
Their mean is the mean the per-image loop would report.

FID is not built (it needs the pretrained Inception weights): asked for, the script says so in one
line and goes on with the reconstruction metrics.
"""
import argparse
import copy
import itertools
import json
import os
import sys
from pathlib import Path
from typing import Dict

import torch

if __name__ == "__main__":   # run as a file: the package root is the directory above scripts/
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from data import get_dataset_class
from data.gan_image_dataset import DeviceImageLoader
from evaluation.psnr_ssim import PSNRSSIMEvaluator
from networks import get_autoencoder, load_weights
from utils.config import load_config

EVAL_TYPES = ("fid", "reconstruction")
FID_NOT_BUILT = "FID is not built here (it needs the pretrained Inception network's weights, which this tree does not ship): skipped"


def save_eval_result(eval_result: dict, eval_type: str, dest_dir: Path, dataset_name: str, checkpoint_name: str):
    """Merge one result into ``<dest_dir>/<eval_type>.json`` under [checkpoint name][dataset name]."""
    dest_file = dest_dir / f"{eval_type}.json"
    results = json.loads(dest_file.read_text()) if dest_file.exists() else {}
    results.setdefault(checkpoint_name, {})[dataset_name] = eval_result
    with dest_file.open("w") as f:
        json.dump(results, f, indent='\t')


def has_not_been_evaluated(checkpoint_name: str, dataset_name: str, evaluation_root: Path) -> Dict[str, bool]:
    """{eval type: True where its result file holds nothing for this checkpoint and dataset}."""
    todo = {}
    for eval_type in EVAL_TYPES:
        dest_file = evaluation_root / f"{eval_type}.json"
        done = json.loads(dest_file.read_text()) if dest_file.exists() else {}
        todo[eval_type] = dataset_name not in done.get(checkpoint_name, {})
    return todo


def evaluate_reconstruction(autoencoder, data_loaders: dict) -> dict:
    evaluator = PSNRSSIMEvaluator()
    psnr, ssim = [], []
    for batch in data_loaders['test']:
        with torch.no_grad():
            reconstructed = autoencoder(batch['input_image'])
        p, s = evaluator.psnr_and_ssim_batch(reconstructed, batch['output_image'])
        psnr.append(p)
        ssim.append(s)
    # one transfer per dataset; the mean over the per-image values, in double as statistics.mean of the reference's floats
    values = torch.stack([torch.cat(psnr), torch.cat(ssim)]).double().cpu()
    return {'psnr': float(values[0].mean()), 'ssim': float(values[1].mean())}


def build_data_loaders(dataset: dict, config: dict, batch_size: int) -> dict:
    dataset_class = get_dataset_class(argparse.Namespace(**config))
    return {
        key: DeviceImageLoader(dataset_class(str(path), config['image_size'], input_dim=config.get('input_dim', 3)),
                               batch_size, shuffle=False, drop_last=False)
        for key, path in dataset.items()
    }


def evaluate_checkpoint(checkpoint: str, dataset: dict, args: argparse.Namespace):
    checkpoint = Path(checkpoint)
    evaluation_root = checkpoint.parent.parent / 'evaluation'
    evaluation_root.mkdir(exist_ok=True)

    dataset_name = dataset.pop('name')
    to_evaluate = has_not_been_evaluated(checkpoint.name, dataset_name, evaluation_root)
    if not args.fid:
        to_evaluate['fid'] = False
    if not args.reconstruction:
        to_evaluate['reconstruction'] = False
    if to_evaluate['fid']:
        print(FID_NOT_BUILT, flush=True)
        to_evaluate['fid'] = False
    if not to_evaluate['reconstruction']:
        return

    config = load_config(str(checkpoint), None)
    autoencoder = get_autoencoder(config).to('cuda')
    autoencoder = load_weights(autoencoder, checkpoint, key='autoencoder', strict=True)
    autoencoder.eval()

    # the reconstruction metrics read the test list only (the train list is FID's)
    data_loaders = build_data_loaders({'test': Path(dataset['test'])}, config, args.batch_size)
    result = evaluate_reconstruction(autoencoder, data_loaders)
    save_eval_result(result, "reconstruction", evaluation_root, dataset_name, checkpoint.name)


def main(args):
    with Path(args.checkpoint_list).open() as f:
        checkpoints = [line.rstrip() for line in f if line.strip()]
    with Path(args.dataset_file).open() as f:
        datasets = json.load(f)

    failed_combinations = []
    try:
        for checkpoint, dataset in itertools.product(checkpoints, datasets):
            try:
                evaluate_checkpoint(checkpoint, copy.deepcopy(dataset), args)
            except Exception as e:
                failed_combinations.append({"combination": (checkpoint, dataset), "reason": str(e)})
    finally:
        for failed in failed_combinations:
            print(f"The following eval combination failed: {failed['combination']}, with reason: {failed['reason']}")
    return failed_combinations


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description="Tool that takes a list of checkpoints and datasets and runs evaluation")
    parser.add_argument("checkpoint_list", help="path to file that contains the path to a trained checkpoint in each line")
    parser.add_argument("dataset_file", help="path to json file that contains the paths to datasets each model is to be evaluated on")
    parser.add_argument("--skip-fid", dest="fid", action='store_false', default=True, help="skip fid during evaluation")
    parser.add_argument("--skip-reconstruction", dest="reconstruction", action='store_false', default=True,
                        help="skip calculation of reconstruction metrics such as PSNR and SSIM")
    parser.add_argument("--batch-size", type=int, default=32, help="images reconstructed and scored per step")
    return parser


if __name__ == "__main__":
    main(build_parser().parse_args())
