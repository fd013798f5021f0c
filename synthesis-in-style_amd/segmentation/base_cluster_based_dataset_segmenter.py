"""Cluster-based dataset labellers (same module path, class name and constructor arguments as the reference's
segmentation/base_cluster_based_dataset_segmenter.py): the k-means catalogs of the generator's activation layers, the hand-made
``merged_classes_{K}.json`` that names a class for every cluster, and the class masks that follow from the two.

What the reference does next with those masks on the host (OpenCV contours, pairwise merging, classification, rendering) runs
on the device in one fixed launch sequence (csrc/cluster_segment.hip); this class only prepares its tables:
the ``cluster -> class bits`` lookup table per catalog.  Debug rendering of contours is not ported."""
import json
from pathlib import Path
from typing import Dict, List, Set

import numpy
import torch

from segmentation.base_dataset_segmenter import BaseDatasetSegmenter
from segmentation.gan_local_edit.factor_catalog import FactorCatalog

MAX_CLUSTERS = 256   # one byte of class bits per cluster id (csrc/cluster_segment.hip)


class BaseClusterBasedDatasetSegmenter(BaseDatasetSegmenter):

    def __init__(self, *args, keys_for_class_determination: List[str], keys_for_finegrained_segmentation: List[str],
                 num_clusters: int, min_class_contour_area: int, only_keep_overlapping: bool = True, **kwargs):
        super().__init__(*args, **kwargs)
        self.base_dir = Path(self.base_dir)
        self.keys_for_class_determination = [str(k) for k in keys_for_class_determination]
        self.keys_for_finegrained_segmentation = [str(k) for k in keys_for_finegrained_segmentation]
        if not self.keys_for_class_determination or not self.keys_for_finegrained_segmentation:
            raise ValueError("keys_for_class_determination and keys_for_finegrained_segmentation need at least one key each")
        self.keys_for_generation = self.keys_for_class_determination + self.keys_for_finegrained_segmentation
        self.num_clusters = num_clusters
        self.min_class_contour_area = int(min_class_contour_area)
        self.only_keep_overlapping = bool(only_keep_overlapping)
        self.debug = False
        self.catalog = self.load_catalog()
        self.class_label_map = self.load_class_label_map()

    def catalog_keys(self) -> List[str]:
        return self.keys_for_generation

    def load_catalog(self) -> Dict[str, FactorCatalog]:
        """``catalogs/{num_clusters}.json`` as create_semantic_segmentation.py writes it: its "catalogs" entry maps a layer to
        the .npy file of that layer's unit centres (a relative path counts from the json's directory).  Only the layers in
        ``catalog_keys()`` are loaded."""
        index = self.base_dir / 'catalogs' / f'{self.num_clusters}.json'
        with index.open() as f:
            files = json.load(f)["catalogs"]
        catalogs = {}
        for layer, name in files.items():
            if str(layer) not in self.catalog_keys():
                continue
            path = Path(name)
            centres = numpy.load(str(path if path.is_absolute() else index.parent / path))
            catalogs[str(layer)] = FactorCatalog(cluster_centers=centres)
        return catalogs

    def load_class_label_map(self) -> Dict[str, Dict[str, List[int]]]:
        """``merged_classes_{num_clusters}.json`` holds {key: {cluster id: class name}}; the labeller wants the other
        direction, {key: {class name: [cluster ids]}}, ids in the file's order."""
        with (self.base_dir / f"merged_classes_{self.num_clusters}.json").open() as f:
            by_cluster = json.load(f)
        by_class = {}
        for key, names in by_cluster.items():
            ids_of = {}
            for cluster_id, class_name in names.items():
                ids_of.setdefault(class_name, []).append(int(cluster_id))
            by_class[str(key)] = ids_of
        return by_class

    def check_sanity_of_class_label_map(self, relevant_keys: Set) -> Dict[str, List[str]]:
        """{key: [class names its label map uses that the colour map does not know]}; empty when everything is labelled."""
        unknown = {}
        for key in relevant_keys:
            strangers = [name for name in self.class_label_map[key] if name not in self.class_to_color_map]
            if strangers:
                unknown[key] = strangers
        return unknown

    def render_debug_contours(self, contours, name: str):
        raise NotImplementedError("debug rendering of contours is not ported (DESIGN.md §11, difference (d))")

    def predict_cluster_maps(self, activations: Dict[int, torch.Tensor]) -> Dict[str, torch.Tensor]:
        """{key: int64 [B, r, r]}: nearest centre per pixel of every catalogued layer (FactorCatalog.predict, on the device)."""
        by_name = {str(k): v for k, v in activations.items()}
        return {key: catalog.predict(by_name[key]) for key, catalog in self.catalog.items()}

    def predict_clusters(self, activations: Dict[int, torch.Tensor], class_label_map: Dict[str, Dict[str, list]]) \
            -> Dict[str, Dict[str, torch.Tensor]]:
        """The reference's layout {key: {class name: bool [B, r, r]}} in plain torch, for callers that want the masks; the
        label pass itself does not go through it."""
        result = {}
        for key, cluster_map in self.predict_cluster_maps(activations).items():
            result[key] = {}
            for class_name, cluster_ids in class_label_map[key].items():
                wanted = torch.as_tensor(list(cluster_ids), dtype=cluster_map.dtype, device=cluster_map.device)
                result[key][class_name] = torch.isin(cluster_map, wanted)
        return result

    # ---- tables of the device pass ------------------------------------------------------------------------------------------
    def non_background_classes(self) -> List[str]:
        return [name for name in self.class_to_color_map if name != 'background']

    def lookup_table(self, keys: List[str]) -> numpy.ndarray:
        """uint8 [len(keys), 256]: bit c of entry (k, id) is set when cluster ``id`` of key ``k`` belongs to the c-th
        non-background class of the colour map."""
        classes = self.non_background_classes()
        table = numpy.zeros((len(keys), MAX_CLUSTERS), dtype=numpy.uint8)
        for row, key in enumerate(keys):
            for class_name, cluster_ids in self.class_label_map[key].items():
                if class_name not in classes:
                    continue
                for cluster_id in cluster_ids:
                    if not 0 <= cluster_id < MAX_CLUSTERS:
                        raise ValueError(f"key {key}: cluster id {cluster_id} outside 0..{MAX_CLUSTERS - 1}")
                    table[row, cluster_id] |= 1 << classes.index(class_name)
        return table

    def create_segmentation_image(self, activations: Dict[int, torch.Tensor]):
        raise NotImplementedError
