"""Loader construction for segmentation training (reference: utils/data_loading.py:123-156 ``get_data_loader``).

Only the reference's ``'wpi'`` branch exists here: JSON-listed ``[image | label]`` PNG pairs -> ``AugmentedSegmentationDataset``
kept on the device -> ``DeviceSegmentationLoader`` (shuffled and ``drop_last`` for training, in index order and complete for
validation, which is inflated by ``num_augmentations`` like the training set, as in the reference; split across ranks by stride as the reference's ``DistributedSampler``).  The DatasetGAN branches of the reference
read activation tensors from disk; they are not loaded here but by ``train_pixel_ensemble.py`` (data/dataset_gan_dataset.py,
``DeviceDatasetGANDataset``), whose batches are pixel indices, not images.
"""
import argparse
import os
from pathlib import Path
from typing import Optional


def get_data_loader(dataset_json_path: Path, dataset_name: str, args: argparse.Namespace, config: dict,
                    validation: bool = False, original_generator_config_path: Optional[Path] = None, rank: int = 0,
                    world_size: int = 1, device=None):
    if dataset_name != 'wpi':
        hint = " ('dataset_gan' is loaded by train_pixel_ensemble.py: data/dataset_gan_dataset.py)" if dataset_name == 'dataset_gan' else ""
        raise NotImplementedError(f"dataset '{dataset_name}': only 'wpi' (JSON-listed PNG pairs) is loaded here{hint}")
    if not getattr(args, 'class_to_color_map', None):
        raise ValueError("a PNG dataset needs --class-to-color-map (class name -> colour of the label halves)")
    if 'num_augmentations' not in config:   # the reference reads config['num_augmentations']; a default of 1 would train unaugmented
        raise KeyError("num_augmentations: the config of a PNG dataset must set it (the reference's segmenter configs use 5; "
                       "1 trains on the originals alone)")
    from data.device_dataset import DeviceSegmentationLoader
    from data.segmentation_dataset import AugmentedSegmentationDataset
    dataset_json_path = Path(dataset_json_path)
    dataset = AugmentedSegmentationDataset(
        dataset_json_path, root=os.path.dirname(dataset_json_path), class_to_color_map_path=Path(args.class_to_color_map),
        background_class_name=config.get('background_class_name', 'background'), image_size=config['image_size'],
        num_augmentations=int(config['num_augmentations']), device=device,
        **({'max_resident_bytes': config['max_resident_bytes']} if 'max_resident_bytes' in config else {}))
    return DeviceSegmentationLoader(dataset, config['batch_size'], shuffle=not validation, drop_last=not validation, rank=rank,
                                    world_size=world_size, seed=int(config.get('seed', 0)))
