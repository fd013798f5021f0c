"""One training iteration of the DatasetGAN pixel-classifier ensemble (reference: updater/dataset_gan_updater.py).

The reference's ``update_core`` walks the members: ``network(batch['activations'])`` -> ``nn.CrossEntropyLoss()`` -> backward ->
``optimizer_{i}.step()``, reporting ``loss/CrossEntropyLoss_network_{i}``.  Here a batch is ``{'pixels': int32 [P, 3], 'label':
int64 [P]}`` (data/dataset_gan_dataset.py): the features are gathered from the resident activations, never stored.

* On a HIP device, at world size 1 and for a shape ``FusedEnsembleStep`` covers, the whole iteration runs on the kernels of
  csrc/pixel_ensemble_train.h, all members per launch (training/ensemble_step.py).
* On CPU tensors, at world size above 1, or for the wide variant, it is the reference's per-member ATen loop on features
  built by ``dataset.features(pixels)``.  ``self.fused_reason`` says which and why; ``fused=True`` makes an unsupported shape an
  error instead.

The reported losses stay on the device (no host synchronisation in ``update_core``).
"""
import torch
from torch import nn

import sis_hip
from training.ensemble_step import FusedEnsembleStep
from training.loop import GradientApplier, Updater, get_current_reporter, get_world_size


class DatasetGANUpdater(Updater):
    def __init__(self, *args, **kwargs):
        fused = kwargs.pop('fused', None)   # None: where supported; True: required; False: the ATen loop
        super().__init__(*args, **kwargs)
        self.loss = nn.CrossEntropyLoss()
        self.data_loaders = self.loaders   # the reference's name
        self.dataset = getattr(self.loaders['feature_vectors'], 'dataset', None)
        self.fused_step, self.fused_reason = None, None
        if fused is not False:
            self.fused_reason = self._why_not_fused()
            if self.fused_reason is None:
                self.fused_step = FusedEnsembleStep(_EnsembleView(self.networks), self.optimizers)
            elif fused:
                raise ValueError(f"DatasetGANUpdater(fused=True): {self.fused_reason}")
        else:
            self.fused_reason = "fused=False"

    def _why_not_fused(self):
        if torch.device(self.device).type != 'cuda':
            return "the updater's device is not a HIP device"
        if any(not p.is_cuda for net in self.networks.values() for p in net.parameters()):
            return "the members are not on a HIP device"
        if get_world_size() > 1:
            return "multi-rank training of the ensemble runs the per-member loop"
        if self.dataset is None or not hasattr(self.dataset, 'layers'):
            return "the loader's dataset holds no resident activation layers"
        return FusedEnsembleStep.unsupported(_EnsembleView(self.networks))

    def update_core(self):
        batch = self.next_batch('feature_vectors')
        batch = {key: value.to(self.device, non_blocking=True) for key, value in batch.items()}
        reporter = get_current_reporter()
        if self.fused_step is not None:
            losses = self.fused_step.step(batch['pixels'], batch['label'], self.dataset)
            for i, key in enumerate(self.networks):
                reporter.add_observation({"CrossEntropyLoss_{}".format(key): losses[i]}, 'loss')
            return
        if 'activations' in batch:
            activations = batch['activations']
        else:
            if next(iter(self.networks.values())).layers[0].weight.is_cuda:
                sis_hip.library_call('dataset_gan_updater.aten_loop', intended=True)
            activations = self.dataset.features(batch['pixels'])
        for i, (key, network) in enumerate(self.networks.items()):
            with GradientApplier([network], [self.optimizers[f'optimizer_{i}']]):
                segmentation_prediction = network(activations)
                loss = self.loss(segmentation_prediction, batch['label'].long())
                loss.backward()
            reporter.add_observation({"CrossEntropyLoss_{}".format(key): loss.detach()}, 'loss')

    def reset(self):
        """Epoch boundary: a generating dataset draws fresh activations; the iterators start over."""
        for data_loader in self.data_loaders.values():
            try:
                data_loader.dataset.reset_dataset()
            except AttributeError:
                pass
        self.iterators = {k: iter(v) for k, v in self.loaders.items()}


class _EnsembleView:
    """The updater holds the members as a dict; ``FusedEnsembleStep`` asks an ensemble for ``get_networks()``."""

    def __init__(self, networks):
        self._networks = networks

    def get_networks(self):
        return self._networks
