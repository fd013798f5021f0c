"""PSNR and SSIM of reconstructions, on the device (reference: evaluation/psnr_ssim.py, which calls kornia once per image).

``PSNRSSIMEvaluator`` keeps the reference's constructor, method names and batch-size-1 assertion; every method is one
``sis_hip.psnr_ssim`` call (csrc/eval_ops.h, three launches, no host sync), which also takes the reference's ``unnormalize``
decision -- a tensor whose minimum is negative is mapped by (clamp(x, -1, 1) + 1) / 2, image and target independently -- on
the device.  ``psnr_and_ssim_batch`` scores every sample of a batch as the reference scores it alone.

``psnr`` is the positive metric 10 log10(max_value^2 / mse): ``kornia.psnr_loss`` returned that in the version the reference was
written against and its negative later; the metric is what is reported.  The definitions are restated, not pinned
against kornia's own output.
"""
from typing import Tuple

import torch

import sis_hip


class PSNRSSIMEvaluator:

    def __init__(self, max_value: int = 1, ssim_kernel_size: int = 5):
        self.max_value = max_value
        self.ssim_kernel_size = ssim_kernel_size

    def psnr_and_ssim_batch(self, image: torch.Tensor, target: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """float32 [B, C, H, W] twice -> (psnr [B], ssim [B]) on the device; nothing is read back."""
        return sis_hip.psnr_ssim(image, target, window=self.ssim_kernel_size, max_val=float(self.max_value))

    def psnr(self, image: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        assert len(image) == 1, "Batch size of images must be one in order to get a meaningful psnr result"
        return self.psnr_and_ssim_batch(image, target)[0][0]

    def ssim(self, image: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        assert len(image) == 1, "Batch size of images must be one in order to get a meaningful ssim result"
        return self.psnr_and_ssim_batch(image, target)[1][0]

    def psnr_and_ssim(self, image: torch.Tensor, target: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        assert len(image) == 1, "Batch size of images must be one in order to get a meaningful psnr / ssim result"
        psnr, ssim = self.psnr_and_ssim_batch(image, target)
        return psnr[0], ssim[0]
