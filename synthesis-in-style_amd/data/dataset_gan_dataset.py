"""``scale_activations`` of the reference (data/dataset_gan_dataset.py:12-34): the [B, S, S, F] per-pixel feature tensor of
DatasetGAN.  Kept for API completeness and as the formulation the fused label pass is checked and timed against; the dataset
loop never builds this tensor (segmentation/dataset_gan_segmenter.py).  Differences: the tensor is allocated on the
activations' device (the reference hard-codes 'cuda', :22) and no singleton axis is squeezed (the reference's ``squeeze()``,
:26, also dropped the batch axis of a batch of one)."""
from typing import Dict, List

import torch
from torch.nn import Upsample


def scale_activations(activations: List[Dict[int, torch.Tensor]], upsamplers: List[Upsample]) -> List[torch.Tensor]:
    scaled_activations = []
    for entry_activation in activations:
        assert len(entry_activation) == len(upsamplers), \
            f"uneven size of activations {len(entry_activation)} to upsamplers {len(upsamplers)}"

        first = next(iter(entry_activation.values()))
        batch_size = first.shape[0]
        image_size = entry_activation[0].shape[2] * int(upsamplers[0].scale_factor)
        feature_size = sum([e.shape[1] for e in entry_activation.values()])

        image_activations = torch.empty((batch_size, image_size, image_size, feature_size), device=first.device)

        feature_index = 0
        for idx, activation in entry_activation.items():
            upscaled_feature_maps = upsamplers[idx](activation)
            new_index = feature_index + upscaled_feature_maps.shape[1]
            image_activations[:, :, :, feature_index:new_index] = torch.moveaxis(upscaled_feature_maps, 1, -1)
            feature_index = new_index

        scaled_activations.append(image_activations)
    return scaled_activations
