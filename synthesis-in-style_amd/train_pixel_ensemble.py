"""Train the DatasetGAN pixel-classifier ensemble (reference: ``train.py`` with ``network: PixelEnsemble`` and ``dataset:
dataset_gan``).  The result -- ``{network_i, optimizer_i}`` snapshots under the log directory -- is what
``create_dataset_for_segmentation.py --classifier-path`` loads for ``segmenter_type: "dataset_gan"``.

    python train_pixel_ensemble.py configs/pixel_ensemble/dataset_gan_ensemble.yaml --images train.json \\
        --class-to-color-map map.json -l logs

Dataset, builder and updater are built directly (the ensemble's batches are pixel indices into resident activations, which
``train.py``'s image loaders and builder lookup do not produce): ``DeviceDatasetGANDataset`` -> ``PixelBatchLoader`` ->
``PixelEnsembleTrainBuilder`` -> ``DatasetGANUpdater``, then ``epochs`` passes with the clamped-cosine schedule and the
snapshotter of ``train.py``.  Single process, one device.
"""
import argparse
import logging
import time
from pathlib import Path

import torch

from train import get_scheduler, load_yaml_config, merge_config_and_args
from training.loop import get_current_reporter


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description='Train the DatasetGAN pixel-classifier ensemble')
    parser.add_argument('config', help='path to the config (configs/pixel_ensemble/dataset_gan_ensemble.yaml)')
    parser.add_argument('--images', dest='train_json', help='json file listing {image, label, activations | latent} entries')
    parser.add_argument('--val-images', dest='validation_json', help='json file with validation entries (loaded in order)')
    parser.add_argument('--class-to-color-map', help='json file: class name -> colour of the label images')
    parser.add_argument('-l', '--log-dir', default='logs', help='where to write snapshots')
    parser.add_argument('--max-iter', dest='max_iter', type=int, help='stop after this many iterations')
    return parser.parse_args(argv)


def load_generator_for(config: dict, device):
    from create_dataset_for_segmentation import load_generator
    return load_generator(config['checkpoint'], config['image_size'], config.get('latent_size', 512), config.get('n_mlp', 8),
                          config.get('channel_multiplier', 2), device)


def build_loader(config: dict, json_path, device, validation: bool = False, generator=None):
    from data.dataset_gan_dataset import DeviceDatasetGANDataset, PixelBatchLoader
    dataset = DeviceDatasetGANDataset(
        json_path, config['tensor_path'], Path(config['class_to_color_map']), config['image_size'],
        background_class_name=config.get('background_class_name', 'background'),
        class_probabilities=config.get('class_probability', 0.5), random_sampling=bool(config.get('random_sampling')) and not validation,
        generate=bool(config.get('generate')), generator=generator, device=device, upsample_mode=config.get('upsample_mode', 'bilinear'))
    return PixelBatchLoader(dataset, config['batch_size'], shuffle=not validation, drop_last=not validation,
                            seed=int(config.get('seed', 0)), epoch_length=config.get('epoch_length'))


def main(args: argparse.Namespace):
    config = merge_config_and_args(load_yaml_config(args.config), args)
    if not config.get('train_json') or not config.get('class_to_color_map'):
        raise ValueError("--images and --class-to-color-map are required")
    device = torch.device('cuda', torch.cuda.current_device()) if torch.cuda.is_available() else torch.device('cpu')
    generator = load_generator_for(config, device) if config.get('generate') else None
    loader = build_loader(config, config['train_json'], device, generator=generator)
    val_loader = build_loader(config, config['validation_json'], device, True, generator) if config.get('validation_json') else None
    from training_builder.pixel_ensemble_train_builder import PixelEnsembleTrainBuilder
    builder = PixelEnsembleTrainBuilder(config, loader, val_loader)
    updater = builder.get_updater()
    logging.info('ensemble step: %s', 'fused kernels' if updater.fused_step is not None else f'ATen loop ({updater.fused_reason})')
    per_epoch = len(loader)
    if per_epoch == 0:
        raise ValueError(f"batch_size {config['batch_size']} is larger than the dataset ({len(loader.dataset)} pixels)")
    schedulers = get_scheduler(config, per_epoch, builder.get_optimizers())
    snapshotter = builder.get_snapshotter()
    t0, it = time.perf_counter(), 0
    for epoch in range(config['epochs']):
        if epoch:
            updater.reset()
        for _ in range(per_epoch):
            it += 1
            updater.update()
            for sched in schedulers.values():
                sched.step()
            if snapshotter is not None:
                snapshotter.maybe_save(it)
            if it % config.get('log_iter', 10) == 0:
                obs = get_current_reporter().scalars()
                rate = it * config['batch_size'] / (time.perf_counter() - t0)
                print(f"iter {it} " + " ".join(f"{k}={v:.5f}" for k, v in obs.items()) + f" pixels/s={rate:.1f}", flush=True)
            if config.get('max_iter') and it >= config['max_iter']:
                break
        if config.get('max_iter') and it >= config['max_iter']:
            break
    if snapshotter is not None and (not snapshotter.every or it % snapshotter.every):
        snapshotter.every = it   # the final state is always written
        snapshotter.maybe_save(it)
    logging.info('Training finished')


if __name__ == '__main__':
    logging.basicConfig(level=logging.INFO)
    main(parse_args())
