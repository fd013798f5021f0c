"""The part of the reference's BaseDatasetSegmenter (segmentation/base_dataset_segmenter.py:15-30) a labeller needs: the
class-to-colour map (``PIL.ImageColor.getrgb`` per entry, in the config's order) and the class-id map (position in that
order).  Its OpenCV helpers are CPU post-processing of the cluster-based labellers and are not ported."""
from pathlib import Path
from typing import Dict

import numpy
from PIL import ImageColor


class BaseDatasetSegmenter:

    def __init__(self, base_dir: Path, image_size: int, class_to_color_map: Dict):
        self.base_dir = base_dir
        self.image_size = image_size
        self.class_to_color_map = self.load_class_to_color_map(class_to_color_map)
        self.class_id_map = self.build_class_id_map(self.class_to_color_map)

    def load_class_to_color_map(self, class_to_color_map: dict) -> dict:
        return {class_name: ImageColor.getrgb(color) for class_name, color in class_to_color_map.items()}

    def build_class_id_map(self, class_to_color_map: dict) -> dict:
        return {class_name: class_id for class_id, class_name in enumerate(class_to_color_map)}

    def colour_table(self) -> numpy.ndarray:
        """uint8 [C, 3]: row = class id.  ``label_images_to_color_images`` of the reference equals ``table[label]``."""
        return numpy.array([c[:3] for c in self.class_to_color_map.values()], dtype=numpy.uint8).reshape(-1, 3)
