"""The default cluster-based labeller (same module path, class name and constructor arguments as the reference's
segmentation/black_white_handwritten_printed_text_segmenter.py): black-and-white pages with printed and handwritten text.

Text regions come from the class-determination layers, fine-grained regions of ``printed_text`` from the fine-grained layers;
every fine-grained region takes the class of the text regions it overlaps most and is painted where the last fine-grained
layer's own ``printed_text`` mask is set.  DESIGN.md §11 states the computation exactly, with its differences from the
reference; all of it runs in csrc/cluster_segment.hip.  There is no host path: CPU tensors raise."""
from typing import Dict, List, Tuple

import numpy
import torch

import sis_hip
from segmentation.base_cluster_based_dataset_segmenter import BaseClusterBasedDatasetSegmenter

FINE_GRAINED_CLASS = 'printed_text'   # the reference's default argument of classify_fine_grained_contours
MAX_KEYS, MAX_CLASSES, MAX_IMAGE_SIZE = 8, 7, 1024


class BlackWhiteHandwrittenPrintedTextDatasetSegmenter(BaseClusterBasedDatasetSegmenter):

    def __init__(self, *args, keys_to_merge: Dict[str, List[str]] = None, **kwargs):
        self.keys_to_merge = {str(dest): [str(s) for s in sources] for dest, sources in (keys_to_merge or {}).items()}
        super().__init__(*args, **kwargs)
        self.keys_for_generation = sorted(set(self.catalog_keys()), key=self.catalog_keys().index)
        if 'background' not in self.class_to_color_map or FINE_GRAINED_CLASS not in self.class_to_color_map:
            raise ValueError(f"class_to_color_map needs the classes 'background' and '{FINE_GRAINED_CLASS}'")
        if len(self.non_background_classes()) > MAX_CLASSES:
            raise ValueError(f"at most {MAX_CLASSES} non-background classes are supported")
        if self.image_size > MAX_IMAGE_SIZE:
            raise ValueError(f"image size {self.image_size} above {MAX_IMAGE_SIZE}")
        self.base_keys, self.sources_of = self.resolve_keys_to_merge()
        unlabelled_clusters = self.check_sanity_of_class_label_map(set(self.base_keys))
        assert not unlabelled_clusters, "Some of the activation maps were not labelled completely " \
                                        f"(map_id: class names without a colour):\n{unlabelled_clusters}"
        self._tables = {}

    def catalog_keys(self) -> List[str]:
        merged_from = [s for sources in self.keys_to_merge.values() for s in sources]
        return self.keys_for_class_determination + self.keys_for_finegrained_segmentation + merged_from

    def resolve_keys_to_merge(self) -> Tuple[List[str], Dict[str, int]]:
        """``keys_to_merge`` applied in dict order, on names: every key ends up as the set of catalogued layers whose masks are
        OR-ed into its own.  Returns the catalogued layers the label pass reads and, per key of the two steps, a bitmask over
        that list."""
        made_of = {key: [key] for key in self.catalog}
        for dest, sources in self.keys_to_merge.items():
            missing = [s for s in sources if s not in made_of]
            if missing or not sources:
                raise ValueError(f"keys_to_merge['{dest}']: no catalog or earlier merge for {missing or 'an empty list'}")
            made_of[dest] = sorted({layer for s in sources for layer in made_of[s]})
        in_use = self.keys_for_class_determination + self.keys_for_finegrained_segmentation
        missing = [k for k in in_use if k not in made_of]
        if missing:
            raise ValueError(f"keys {missing} have neither a catalog in catalogs/{self.num_clusters}.json nor a keys_to_merge entry")
        base_keys = [k for k in self.catalog if any(k in made_of[u] for u in in_use)]
        unmapped = [k for k in base_keys if k not in self.class_label_map]
        if unmapped:
            raise ValueError(f"merged_classes_{self.num_clusters}.json has no entry for the keys {unmapped}")
        if len(base_keys) > MAX_KEYS or len(self.keys_for_class_determination) > MAX_KEYS \
                or len(self.keys_for_finegrained_segmentation) > MAX_KEYS:
            raise ValueError(f"at most {MAX_KEYS} catalogued layers and {MAX_KEYS} keys per step are supported")
        return base_keys, {u: sum(1 << base_keys.index(layer) for layer in made_of[u]) for u in in_use}

    def _device_table(self, device) -> torch.Tensor:
        if str(device) not in self._tables:
            self._tables[str(device)] = torch.from_numpy(self.lookup_table(self.base_keys)).to(device)
        return self._tables[str(device)]

    def label_cluster_maps(self, cluster_maps: Dict[str, torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """{key: int64 [B, r, r]} of the catalogued layers -> (class_map uint8 [B,S,S], colour uint8 [B,S,S,3], drop uint8 [B]),
        all on the device, nothing read back."""
        maps = [cluster_maps[k] for k in self.base_keys]
        for key, m in zip(self.base_keys, maps):
            if m.shape[-1] > self.image_size or self.image_size % m.shape[-1]:
                raise ValueError(f"key {key}: resolution {m.shape[-1]} does not divide the image size {self.image_size}")
        if any(not m.is_cuda for m in maps):
            raise NotImplementedError("the cluster-based label pass runs on a HIP device only; there is no host path")
        classes = self.non_background_classes()
        order = ['background'] + classes
        return sis_hip.cluster_segment(
            maps, self._device_table(maps[0].device),
            [self.sources_of[k] for k in self.keys_for_class_determination],
            [self.sources_of[k] for k in self.keys_for_finegrained_segmentation],
            classes.index(FINE_GRAINED_CLASS), [self.class_id_map[name] for name in order],
            [self.class_to_color_map[name][:3] for name in order], self.image_size, self.only_keep_overlapping,
            self.min_class_contour_area)

    @torch.no_grad()
    def label_activations(self, activations: Dict[int, torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        by_name = {str(k): v for k, v in activations.items()}
        for key in self.base_keys:
            if by_name[key].shape[-1] > self.image_size:
                raise ValueError(f"key {key}: activations of edge {by_name[key].shape[-1]} are larger than the image "
                                 f"size {self.image_size}")
        if any(not by_name[key].is_cuda for key in self.base_keys):
            raise NotImplementedError("the cluster-based label pass runs on a HIP device only; there is no host path")
        return self.label_cluster_maps({key: self.catalog[key].predict(by_name[key]) for key in self.base_keys})

    def create_segmentation_image(self, activations: Dict[int, torch.Tensor]) -> Tuple[numpy.ndarray, List[int]]:
        """(colour images uint8 [B,S,S,3], ids within the batch of the images to drop), as the reference returns."""
        _, colour, drop = self.label_activations(activations)
        return colour.cpu().numpy(), [int(i) for i in torch.nonzero(drop.cpu()).flatten()]
