"""Common base of the segmentation networks (reference: networks/base_segmenter.py:11-65).

On the hot path only two things matter: it is the nn.Module base class of EMANet / TransUNet, and
``predict_classes`` yields the argmax label map.  The reference's inference-time clean-up is a confidence
threshold, then OpenCV contour removal below ``min_contour_area`` on the host, per patch and per class.  Here
the threshold alone is a tensor op; with ``min_contour_area > 0`` both run in ``sis_hip.remove_small_contours``
(csrc/contour_ops.hip) on the device.  There is no host implementation: CPU tensors raise.
"""
from typing import Any

import torch
import torch.nn.functional as F
from torch import nn


class BaseSegmenter(nn.Module):
    def __init__(self, background_class_id: int = 0, min_confidence: float = 0.0, min_contour_area: int = 0,
                 num_input_channels: int = 3):
        super().__init__()
        self.background_class_id = background_class_id
        self.min_confidence = min_confidence
        self.min_contour_area = min_contour_area
        self.num_input_channels = num_input_channels

    def postprocess(self, predictions: torch.Tensor) -> torch.Tensor:
        if self.min_contour_area > 0:
            if not predictions.is_cuda:
                raise NotImplementedError("contour-area filtering runs on the device only (sis_hip.remove_small_contours)")
            import sis_hip
            return sis_hip.remove_small_contours(predictions, self.min_confidence, self.min_contour_area,
                                                 self.background_class_id)
        return torch.where(predictions < self.min_confidence, torch.zeros_like(predictions), predictions)

    def predict(self, x: torch.Tensor) -> torch.Tensor:
        return self.postprocess(F.softmax(self.forward(x), dim=1))

    def predict_classes(self, x: torch.Tensor) -> torch.Tensor:
        return torch.argmax(self.predict(x), dim=1, keepdim=True)

    def forward(self, x: Any):
        raise NotImplementedError
