"""DocUFCN declaration for the shared train builder (reference: training_builder/doc_ufcn_train_builder.py:12-46).

``get_doc_ufcn('base')(3, 3)`` as the reference builds it (:25-27), ``GradientClipAdam(lr, betas=(beta1, beta2), weight_decay)``
from the config (:18-23, :29-31; training/fused_adam.py states the assumed clip rule), the class-weighted cross-entropy updater
(:33-43).  Data parallelism, fine-tuning and snapshots come from the base class."""
from networks.doc_ufcn import get_doc_ufcn
from training.fused_adam import GradientClipAdam
from training_builder.base_train_builder import BaseTrainBuilder, strip_parallel_module
from updater.segmentation_updater import StandardUpdater


class DocUFCNTrainBuilder(BaseTrainBuilder):
    updater_class = StandardUpdater

    def build_network(self):
        segmentation_network_class = get_doc_ufcn('base')
        return segmentation_network_class(3, 3)

    def get_optimizers(self):
        if self._optimizers is None:
            cfg = self.config
            optimizer = GradientClipAdam(strip_parallel_module(self.segmentation_network).parameters(), lr=float(cfg['lr']),
                                         betas=(cfg['beta1'], cfg['beta2']), weight_decay=cfg['weight_decay'])
            self._optimizers = {'main': optimizer}
        return self._optimizers

    def updater_options(self):
        return {'class_weights': list(self.config['class_weights'])}
