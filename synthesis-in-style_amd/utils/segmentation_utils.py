"""Ground-truth colour images -> class maps on the device (reference: utils/segmentation_utils.py:124-157).

The reference walks the class-to-colour map with one ``numpy.where`` over the whole image per class; here the image is
uploaded once and ``sis_color_to_class`` compares every pixel against the colour table in one pass.  The contour helpers of
the reference file are OpenCV code and have no counterpart here: the contour filter is ``sis_hip.remove_small_contours``,
``find_class_contours`` + ``cv2.boundingRect`` are ``sis_hip.page_regions`` (segmentation/evaluation/segmentation_visualization.py).
``BBox`` is the reference's (:21-64).
"""
from typing import Dict, NamedTuple, Tuple

import torch

import sis_hip


class BBox(NamedTuple):
    left: int
    top: int
    right: int
    bottom: int

    @classmethod
    def from_opencv_bounding_rect(cls, x, y, width, height):
        return cls(x, y, x + width, y + height)

    def top_left(self) -> Tuple:
        return self.left, self.top

    def bottom_right(self) -> Tuple:
        return self.right, self.bottom

    @property
    def width(self) -> int:
        return self.right - self.left

    @property
    def height(self) -> int:
        return self.bottom - self.top

    def as_points(self) -> Tuple:
        """top left, top right, bottom right, bottom left"""
        return self.top_left(), (self.right, self.top), self.bottom_right(), (self.left, self.bottom)

    def is_overlapping_with(self, other_box: "BBox") -> bool:
        return self.left < other_box.right and self.right > other_box.left and self.top < other_box.bottom \
            and self.bottom > other_box.top

    def get_mutual_bbox(self, other_box: "BBox") -> "BBox":
        return BBox(min(self.left, other_box.left), min(self.top, other_box.top), max(self.right, other_box.right),
                    max(self.bottom, other_box.bottom))


def get_class_id_map(background_class_name: str, class_to_color_map: dict) -> Dict[str, int]:
    """Class name -> id: the background class is 0, the other classes follow in the order of the map."""
    others = [name for name in class_to_color_map if name != background_class_name]
    if len(others) == len(class_to_color_map):
        raise KeyError(background_class_name)
    return {background_class_name: 0, **{name: i + 1 for i, name in enumerate(others)}}


def _rgb(color):
    if isinstance(color, str):
        from PIL import ImageColor
        color = ImageColor.getrgb(color)
    return tuple(int(v) for v in color)[:3]


def segmentation_image_to_class_image(segmentation_image, background_class_name: str, class_to_color_map: dict,
                                      device=None) -> torch.Tensor:
    """uint8 [H, W, 3] colour image (tensor or array) -> uint8 [H, W] class ids on the device.  Pixels whose colour is not in
    the map stay background; of two classes with one colour the later one in the map wins, as in the reference."""
    assert background_class_name in class_to_color_map.keys(), \
        f"The name of the background class ({background_class_name}) is not in the the class to color map "
    ids = get_class_id_map(background_class_name, class_to_color_map)
    names = [name for name in class_to_color_map if name != background_class_name]
    image = torch.as_tensor(segmentation_image)
    if device is not None:
        image = image.to(device)
    return sis_hip.color_to_class(image, [_rgb(class_to_color_map[n]) for n in names], [ids[n] for n in names],
                                  background_id=ids[background_class_name])
