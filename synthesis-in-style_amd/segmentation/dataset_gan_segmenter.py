"""DatasetGAN labeller (reference: segmentation/dataset_gan_segmenter.py): a PixelEnsembleClassifier classifies every pixel
of the generator's activations, upsampled to image resolution.

``predict_labels`` keeps the reference's formulation ([B, S, S, F] features, ATen, also on CPU tensors).
``create_segmentation_image`` and ``predict_labels_from_activations`` run the fused device pass instead
(csrc/pixel_ensemble.hip): the first Linear of every member is applied to each activation at its own resolution and only
its result is interpolated (bilinear upsampling commutes with it), so neither the feature tensor nor a full-resolution
hidden tensor is formed.  There is no ATen fallback on that path: unsupported shapes raise."""
from typing import Dict, List, Optional, Tuple

import numpy
import torch
from torch import nn

import sis_hip
from networks.pixel_classifier.model import PixelClassifier, PixelEnsembleClassifier
from segmentation.base_dataset_segmenter import BaseDatasetSegmenter


class DatasetGANSegmenter(BaseDatasetSegmenter):
    def __init__(self, *args, classifier_path: str, feature_size: int, upsamplers: List[nn.Upsample], **kwargs):
        super().__init__(*args, **kwargs)
        self.ensemble = self.load_ensemble(classifier_path, feature_size)
        self.upsamplers = upsamplers
        self._luts = {}

    def load_ensemble(self, path: str, feature_size: int) -> PixelEnsembleClassifier:
        """Every checkpoint entry whose key contains "network" and not "optimizer" is a member's state_dict (strict)."""
        device = torch.device('cuda') if torch.cuda.is_available() else torch.device('cpu')
        ensemble = PixelEnsembleClassifier(len(self.class_to_color_map.keys()), self.image_size, 0)
        checkpoint = torch.load(path, map_location='cpu')
        for key in checkpoint.keys():
            if "network" in key and "optimizer" not in key:
                model = PixelClassifier(len(self.class_to_color_map.keys()), feature_size)
                model.load_state_dict(checkpoint[key])
                model.to(device)
                model.eval()
                ensemble.add_network(model)
        return ensemble

    @torch.no_grad()
    def predict_labels(self, activations: torch.Tensor) -> torch.Tensor:
        b, w, h, f = activations.shape
        activations_batch = activations.reshape([b * w * h, f])
        labels = self.ensemble.predict_classes(activations_batch)
        return labels.reshape([b, self.image_size, self.image_size])

    def label_images_to_color_images(self, label_images: torch.Tensor) -> numpy.ndarray:
        batch_size, _, height, width = label_images.shape
        color_images = numpy.zeros((batch_size, height, width, 3), dtype='uint8')
        color_images[:, :, :] = self.class_to_color_map['background']
        for class_id, (class_name, color) in enumerate(self.class_to_color_map.items()):
            if class_name == 'background':
                continue
            class_mask = (label_images == class_id).cpu().numpy().squeeze()
            color_images[class_mask] = color
        return color_images

    def _layout(self, activations: Dict[int, torch.Tensor]) -> Tuple[List[Tuple[int, int]], List[torch.Tensor]]:
        tensors = list(activations.values())
        if len(self.upsamplers) != len(tensors):
            raise ValueError(f"{len(tensors)} activation layers for {len(self.upsamplers)} upsamplers")
        layout = []
        for key, t in activations.items():
            up = self.upsamplers[key]
            if getattr(up, 'mode', None) != 'bilinear' or getattr(up, 'align_corners', None):
                raise NotImplementedError(f"upsampler of layer {key}: only mode='bilinear' with align_corners=False is implemented")
            if t.dim() != 4 or t.shape[2] != t.shape[3]:
                raise ValueError(f"layer {key}: square [B, C, H, W] activations are required, got {tuple(t.shape)}")
            res = t.shape[-1]
            if res > self.image_size or self.image_size % res or (self.image_size // res) & (self.image_size // res - 1) \
                    or float(up.scale_factor) * res != self.image_size:
                raise ValueError(f"layer {key}: resolution {res} is not a power-of-two fraction of {self.image_size} matching "
                                 f"its upsampler (scale {up.scale_factor})")
            layout.append((t.shape[1], res))
        return layout, tensors

    def _colour_lut(self, device) -> torch.Tensor:
        key = str(device)
        if key not in self._luts:
            self._luts[key] = torch.from_numpy(self.colour_table()).to(device)
        return self._luts[key]

    @torch.no_grad()
    def label_activations(self, activations: Dict[int, torch.Tensor], colours: bool = True, want_logits: bool = False) \
            -> Tuple[torch.Tensor, Optional[torch.Tensor], Optional[torch.Tensor]]:
        """Fused device pass -> (labels int64 [B, S, S], colour image uint8 [B, S, S, 3] or None,
        member logits [N, B, S, S, C] (tests) or None)."""
        layout, tensors = self._layout(activations)
        device = tensors[0].device
        if device.type != 'cuda':
            raise RuntimeError("the fused DatasetGAN label pass needs activations on a HIP device")
        fw = self.ensemble.fused_weights(layout, self.image_size, device)
        return sis_hip.pixel_ensemble_label(
            [tensors[i] for i in fw["full"]], [([tensors[i] for i in idx], wt) for idx, wt in fw["groups"]], fw["w1f"],
            fw["b1"], fw["w2t"], fw["b2"], fw["w3t"], fw["b3"], fw["classes"], fw["hidden1"], self.image_size,
            lut=self._colour_lut(device) if colours else None, want_logits=want_logits)

    def predict_labels_from_activations(self, activations: Dict[int, torch.Tensor]) -> torch.Tensor:
        return self.label_activations(activations, colours=False)[0]

    def create_segmentation_image(self, activations: Dict[int, torch.Tensor]) -> Tuple[numpy.ndarray, List[int]]:
        """The reference's result (colour images, no image dropped) from the fused pass instead of ``scale_activations``."""
        return self.label_activations(activations)[1].cpu().numpy(), []


def dataset_gan_upsamplers(activations: Dict[int, torch.Tensor], image_size: int) -> List[nn.Upsample]:
    """The reference's upsamplers (create_dataset_for_segmentation.py:28-49): one ``nn.Upsample(scale_factor=S / h,
    mode='bilinear')`` per activation layer, in the dict's order."""
    return [nn.Upsample(scale_factor=image_size / a.shape[-1], mode='bilinear') for a in activations.values()]
