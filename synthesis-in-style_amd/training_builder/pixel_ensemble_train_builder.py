"""Train builder of the DatasetGAN pixel-classifier ensemble (reference: training_builder/pixel_ensemble_train_builder.py).

Same method names as the reference.  The ensemble is ``PixelEnsembleClassifier(numpy_class, feature_vector_length, num_models)``
with the feature length asked of the loader's dataset; every member gets its own ``GradientClipAdam`` (``optimizer_{i}``, from
``lr`` / ``beta1`` / ``beta2`` / ``weight_decay``); the snapshot is ``{network_i: state_dict, optimizer_i: state_dict}``, the
layout ``DatasetGANSegmenter.load_ensemble`` reads.  As in the other builders here the optimizers are created once (the
reference builds new ones on every ``get_optimizers()`` call), and the evaluator (Dice on a validation set) and the image
plotter are not part of the step: both return ``None``.

This builder is not registered in ``train_builder_selection`` -- its batches are pixel indices, not images, so ``train.py``'s
loop does not fit; ``train_pixel_ensemble.py`` is its entry point.  Single rank only.
"""
from typing import Dict

import torch

from networks.pixel_classifier.model import PixelEnsembleClassifier
from training.fused_adam import GradientClipAdam
from training_builder.base_train_builder import BaseTrainBuilder, Snapshotter
from updater.dataset_gan_updater import DatasetGANUpdater


class PixelEnsembleTrainBuilder(BaseTrainBuilder):
    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self._initialize_segmentation_network()
        self.segmentation_network = self._prepare_segmentation_network(self.segmentation_network)
        self.optimizer_opts = {
            'betas': (self.config['beta1'], self.config['beta2']),
            'weight_decay': self.config['weight_decay'],
            'lr': float(self.config['lr']),
        }
        self._updater = None

    def _initialize_segmentation_network(self):
        try:
            feature_vector_length = self.train_data_loader.dataset.get_feature_vector_length()
        except AttributeError:
            raise RuntimeError('The given dataset does not seem to implement the "get_feature_vector_length" method. '
                               'However, this is required for initializing the PixelEnsemble classifier') from None
        self.segmentation_network = PixelEnsembleClassifier(self.config['numpy_class'], feature_vector_length,
                                                            self.config['num_models'])

    def _prepare_segmentation_network(self, segmentation_network, network_name: str = 'segmentation_network'):
        if self.world_size > 1:
            raise NotImplementedError("multi-rank training of the pixel ensemble is not provided")
        device = self.device()
        for sub_network_name, network in segmentation_network.get_networks().items():
            network.to(device)
            if self.fine_tune is not None:
                checkpoint = torch.load(self.fine_tune, map_location='cpu')
                network.load_state_dict(checkpoint[sub_network_name])
            segmentation_network.set_network(sub_network_name, network)
        return segmentation_network

    def get_networks_for_updater(self) -> Dict:
        return self.segmentation_network.get_networks()

    def get_optimizers(self) -> Dict:
        if self._optimizers is None:
            self._optimizers = {f'optimizer_{i}': GradientClipAdam(sub_network.parameters(), **self.optimizer_opts)
                                for i, sub_network in enumerate(self.segmentation_network.get_networks().values())}
        return self._optimizers

    def get_updater(self):
        if self._updater is None:
            self._updater = DatasetGANUpdater(
                iterators={'feature_vectors': self.train_data_loader}, networks=self.get_networks_for_updater(),
                optimizers=self.get_optimizers(), device=self.device(), copy_to_device=(self.world_size == 1),
                fused=self.config.get('fused'))
        return self._updater

    def get_evaluator(self, logger=None):
        return None   # the DatasetGAN evaluator scores whole activation stacks with the reference's own id-valued "Dice": not
        # the pixel-batch pass of training/validation.py

    def get_snapshotter(self):
        if self.rank != 0:
            return None
        return Snapshotter({**self.segmentation_network.get_networks(), **self.get_optimizers()},
                           self.config.get('log_dir', 'logs'), self.config.get('snapshot_save_iter', 0))
