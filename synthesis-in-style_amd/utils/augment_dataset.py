"""Training-time augmentation on the device (reference: utils/augment_dataset.py:33-59 ``augment_image``).

The reference builds two imgaug pipelines per sample -- geometric (one or two of elastic / ShearX / CropAndPad / translate, then
sometimes Rot90 or Rotate) and colour (sometimes a gamma contrast, sometimes invert) -- and runs them on the host, one PIL image
at a time.  Here the host only DRAWS a sample's parameters: the affine steps are composed into one matrix, the colour steps into
one 256-entry table, the elastic step into (alpha, sigma, seed word).  The pixels are touched once, on the device, by
``sis_hip.augment_warp`` (and ``sis_hip.elastic_field`` for the samples that drew the elastic step).

imgaug is not a dependency and the result is NOT pinned against it: the transformation is stated exactly in DESIGN.md §12 and
tested against a numpy / scipy restatement of that statement.  Deliberate differences from the reference: the affine steps are
resampled once instead of once per step (the reference rounds to uint8 after every step), the elastic step samples bilinearly
(imgaug's default there is cubic), and the class map is warped with nearest neighbours (the reference interpolates the colour
label image, and blended border colours become background).

Conventions: pixel (x, y) has its centre at (x, y); an image of width W covers [-0.5, W - 0.5]; the centre of rotation and
shear is ((W - 1) / 2, (H - 1) / 2); a resize from W to W' maps x to (x + 0.5) W' / W - 0.5.
"""
import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy
import torch

import sis_hip

ELASTIC_ALPHA = (5.0, 25.0)
ELASTIC_SIGMA = (5.0, 9.0)
SHEAR_DEGREES = 20.0
CROP_AND_PAD_PX = (-80, 80)
TRANSLATE_PERCENT = 0.15
P_ROTATION = 0.66
ROT90_K = (1, 3)
ROTATE_DEGREES = (-15.0, 15.0)
P_GAMMA = 0.8
GAMMA_DARKER = (1.5, 2.5)
GAMMA_LIGHTER = (0.1, 1.0)
P_INVERT = 0.10
GEOMETRIC_STEPS = ("elastic", "shear", "crop_and_pad", "translate")   # SomeOf keeps this order


def draw_augmentation(rng: numpy.random.Generator) -> Dict:
    """One sample's draws, in the reference's structure (augment_dataset.py:33-52); sizes enter only in ``compose_matrix``."""
    plan = {}
    count = int(rng.integers(1, 3))                                     # SomeOf((1, 2), ...)
    chosen = set(int(i) for i in rng.choice(4, size=count, replace=False))
    plan["steps"] = [name for i, name in enumerate(GEOMETRIC_STEPS) if i in chosen]
    if "elastic" in plan["steps"]:
        plan["elastic"] = {"alpha": float(rng.uniform(*ELASTIC_ALPHA)), "sigma": float(rng.uniform(*ELASTIC_SIGMA)),
                           "seed": int(rng.integers(0, 1 << 32, dtype=numpy.uint64))}
    if "crop_and_pad" in plan["steps"]:   # top, right, bottom, left; negative crops, positive pads
        plan["crop_and_pad"] = [int(v) for v in rng.integers(CROP_AND_PAD_PX[0], CROP_AND_PAD_PX[1] + 1, size=4)]
    if "translate" in plan["steps"]:
        plan["translate"] = [float(v) for v in rng.uniform(-TRANSLATE_PERCENT, TRANSLATE_PERCENT, size=2)]   # x, y
    if rng.random() < P_ROTATION:                                       # Sometimes(0.66, OneOf([Rot90, Rotate]))
        if rng.random() < 0.5:
            plan["rot90"] = int(ROT90_K[int(rng.integers(0, 2))])
        else:
            plan["rotate"] = float(rng.uniform(*ROTATE_DEGREES))
    if rng.random() < P_GAMMA:                                          # Sometimes(0.8, OneOf([darker, lighter]))
        plan["gamma"] = float(rng.uniform(*(GAMMA_DARKER if rng.random() < 0.5 else GAMMA_LIGHTER)))
    plan["invert"] = bool(rng.random() < P_INVERT)
    return plan


def _translation(tx, ty):
    return numpy.array([[1.0, 0.0, tx], [0.0, 1.0, ty], [0.0, 0.0, 1.0]])


def _resize(width, height, new_width, new_height):
    sx, sy = new_width / width, new_height / height
    return numpy.array([[sx, 0.0, 0.5 * sx - 0.5], [0.0, sy, 0.5 * sy - 0.5], [0.0, 0.0, 1.0]])


def _about_centre(linear, width, height):
    cx, cy = (width - 1) / 2.0, (height - 1) / 2.0
    m = numpy.eye(3)
    m[:2, :2] = linear
    return _translation(cx, cy) @ m @ _translation(-cx, -cy)


def shear_matrix(degrees, width, height):
    """x' = x + tan(degrees) (y - c_y)."""
    return _about_centre([[1.0, math.tan(math.radians(degrees))], [0.0, 1.0]], width, height)


def rotation_matrix(degrees, width, height):
    c, s = math.cos(math.radians(degrees)), math.sin(math.radians(degrees))
    return _about_centre([[c, -s], [s, c]], width, height)


def crop_and_pad_matrix(top, right, bottom, left, width, height):
    """Pad (positive) or crop (negative) every side by that many pixels, then resize back to width x height.  An axis whose
    crops would leave less than one pixel is left alone."""
    if width + left + right < 1:
        left = right = 0
    if height + top + bottom < 1:
        top = bottom = 0
    return _resize(width + left + right, height + top + bottom, width, height) @ _translation(left, top)


def translate_matrix(fraction_x, fraction_y, width, height):
    """Whole pixels: round(fraction * size)."""
    return _translation(float(numpy.rint(fraction_x * width)), float(numpy.rint(fraction_y * height)))


def rot90_matrix(k, width, height):
    """k clockwise quarter turns (``numpy.rot90(image, -k)``), then a resize back to width x height."""
    k = k % 4
    if k == 0:
        return numpy.eye(3)
    if k == 2:
        return numpy.array([[-1.0, 0.0, width - 1.0], [0.0, -1.0, height - 1.0], [0.0, 0.0, 1.0]])
    if k == 1:    # x' = H - 1 - y, y' = x
        turn = numpy.array([[0.0, -1.0, height - 1.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    else:         # x' = y, y' = W - 1 - x
        turn = numpy.array([[0.0, 1.0, 0.0], [-1.0, 0.0, width - 1.0], [0.0, 0.0, 1.0]])
    return _resize(height, width, width, height) @ turn


def _out_hw(out_size, height, width) -> Tuple[int, int]:
    if out_size is None:
        return height, width
    if isinstance(out_size, (int, numpy.integer)):
        return int(out_size), int(out_size)
    return int(out_size[0]), int(out_size[1])


def compose_matrix(plan: Optional[Dict], height: int, width: int, out_size=None) -> numpy.ndarray:
    """float64 3x3 matrix taking source pixel coordinates (of the elastically displaced image, when the plan has that step) to
    output pixel coordinates: shear, crop-and-pad, translate in that order, then rot90 / rotate, then the resize to
    ``out_size``.  ``plan`` None: only the resize."""
    m = numpy.eye(3)
    if plan is not None:
        for step in plan["steps"]:
            if step == "shear":
                m = shear_matrix(SHEAR_DEGREES, width, height) @ m
            elif step == "crop_and_pad":
                m = crop_and_pad_matrix(*plan["crop_and_pad"], width, height) @ m
            elif step == "translate":
                m = translate_matrix(*plan["translate"], width, height) @ m
        if "rot90" in plan:
            m = rot90_matrix(plan["rot90"], width, height) @ m
        elif "rotate" in plan:
            m = rotation_matrix(plan["rotate"], width, height) @ m
    out_h, out_w = _out_hw(out_size, height, width)
    return _resize(width, height, out_w, out_h) @ m


def inverse_map(matrix: numpy.ndarray) -> numpy.ndarray:
    """The kernel's ``minv``: the float64 inverse, cast to float32 [2, 3]."""
    return numpy.linalg.inv(matrix)[:2].astype(numpy.float32)


def gamma_lut(gamma: float) -> numpy.ndarray:
    v = numpy.arange(256, dtype=numpy.float64)
    return numpy.clip(numpy.rint(255.0 * (v / 255.0) ** gamma), 0, 255).astype(numpy.uint8)


def color_lut(plan: Optional[Dict]) -> numpy.ndarray:
    """uint8 [256]: gamma contrast 255 (v / 255)^gamma rounded, then invert."""
    lut = numpy.arange(256, dtype=numpy.uint8)
    if plan is not None:
        if "gamma" in plan:
            lut = gamma_lut(plan["gamma"])
        if plan.get("invert"):
            lut = (255 - lut).astype(numpy.uint8)
    return lut


def sample_augmentation(rng: numpy.random.Generator, height: int, width: int, out_size=None):
    """-> (minv float32 [2, 3], lut uint8 [256], elastic): ``elastic`` is None or (alpha, sigma, seed word)."""
    plan = draw_augmentation(rng)
    elastic = None
    if "elastic" in plan:
        e = plan["elastic"]
        elastic = (e["alpha"], min(float(numpy.float32(e["sigma"])), sis_hip.ELASTIC_MAX_SIGMA), e["seed"])
    return inverse_map(compose_matrix(plan, height, width, out_size)), color_lut(plan), elastic


def identity_parameters(height: int, width: int, out_size=None):
    """The parameters of an unaugmented slot: only the resize to ``out_size``."""
    return inverse_map(compose_matrix(None, height, width, out_size)), color_lut(None), None


def launch_parameters(parameters: Sequence, index: Sequence[int], device) -> Tuple[torch.Tensor, ...]:
    """B parameter sets + sample ids -> (index, field_slot, minv, lut) on the device through ONE pinned, non-blocking copy, and
    the host list of the elastic draws in slot order."""
    b = len(parameters)
    staged = torch.empty(b * (4 + 4 + 24 + 256), dtype=torch.uint8, pin_memory=True)
    host = staged.numpy()
    idx, slot = host[:4 * b].view(numpy.int32), host[4 * b:8 * b].view(numpy.int32)
    minv, lut = host[8 * b:32 * b].view(numpy.float32).reshape(b, 2, 3), host[32 * b:].reshape(b, 256)
    elastic: List = []
    for i, (m, table, e) in enumerate(parameters):
        idx[i], minv[i], lut[i] = int(index[i]), m, table
        slot[i] = -1 if e is None else len(elastic)
        if e is not None:
            elastic.append(e)
    dev = staged.to(device, non_blocking=True)
    return (dev[:4 * b].view(torch.int32), dev[4 * b:8 * b].view(torch.int32), dev[8 * b:32 * b].view(torch.float32).view(b, 2, 3),
            dev[32 * b:].view(b, 256), elastic)


def augment_batch(pixels: torch.Tensor, classes: torch.Tensor, index: Sequence[int], rng, out_size=None, augment=None,
                  background_id: int = 0, quantize: bool = True) -> Dict[str, torch.Tensor]:
    """A training batch from the resident dataset (pixels uint8 [N, H, W, 3], classes uint8 [N, H, W] on the device): slot b is
    sample ``index[b]``, augmented with parameters drawn from ``rng`` (a ``numpy.random.Generator``, or one per slot) unless
    ``augment[b]`` is False.  -> {"images": float32 [B, 3, S, S], "segmented": int64 [B, 1, S, S]}."""
    sis_hip.require_device(pixels, "pixels")
    height, width = int(pixels.shape[1]), int(pixels.shape[2])
    parameters = []
    for b in range(len(index)):
        if augment is not None and not augment[b]:
            parameters.append(identity_parameters(height, width, out_size))
        else:
            parameters.append(sample_augmentation(rng[b] if isinstance(rng, (list, tuple)) else rng, height, width, out_size))
    idx, slot, minv, lut, elastic = launch_parameters(parameters, index, pixels.device)
    field = None
    if elastic:
        field = sis_hip.elastic_field(height, width, [e[1] for e in elastic], [e[0] for e in elastic],
                                      seeds=[e[2] for e in elastic], device=pixels.device)
    return sis_hip.augment_warp(pixels, classes, idx, minv, lut, slot, field, background_id=background_id,
                                out_size=_out_hw(out_size, height, width), quantize=quantize)
