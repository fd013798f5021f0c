"""Host tables of the scan-patch kernels (csrc/scan_patches.h): everything Pillow decides in floating point
before a pixel is touched, restated in Python floats so that the kernels are left with integer arithmetic.

- ``thumbnail_size``: the size rule of ``Image.thumbnail`` (``preserve_aspect_ratio`` / ``round_aspect``);
- ``reducing_factors``: the ``reducing_gap = 2.0`` rule of ``Image.resize``, ``int(W / w / 2) or 1`` per axis;
- ``axis_table``: ``precompute_coeffs`` and ``normalize_coeffs_8bpc`` of Pillow's Resample.c for BICUBIC;
- ``thumbnail_plan``: the three composed, as ``sis_hip.scan_thumbnail`` runs them;
- ``patch_origins``: the windows of the reference's ``crop_patches`` (scripts/create_stylegan_train_dataset.py:18-34), each
  bound rounded as ``Image.crop`` rounds it (Python's ``round``: .5 goes to even);
- ``random_resize_size``: the size the reference's ``random_resize`` (:37-46) hands to ``thumbnail``;
- ``scale_bounding_box``: the reference's function of that name (:114-129), which carries the content box found on the
  ``ANALYSIS_SIZE`` thumbnail (``sis_hip.scan_content_box``) over to the page.

Sizes are (width, height) as Pillow writes them."""
import functools
import math
import struct
from typing import List, NamedTuple, Optional, Tuple

PRECISION_BITS = 22          # Pillow: 32 - 8 - 2
BICUBIC_SUPPORT = 2.0
ANALYSIS_SIZE = 1000         # the side of the thumbnail that the reference's remove_scanning_margin (:132-138) looks for the margin on


def c_float(value: float) -> float:
    """``value`` as it arrives in a C ``float`` argument (the resample box is float[4] in Pillow)."""
    return struct.unpack("f", struct.pack("f", value))[0]


def thumbnail_size(width: int, height: int, size) -> Optional[Tuple[int, int]]:
    """What ``Image.thumbnail((size, size))`` resizes a width x height image to; None where it leaves the image alone."""
    x = y = math.floor(size)
    if x >= width and y >= height:
        return None

    def round_aspect(number, key):
        return max(min(math.floor(number), math.ceil(number), key=key), 1)

    aspect = width / height
    if x / y >= aspect:
        x = round_aspect(y * aspect, key=lambda n: abs(aspect - n / y))
    else:
        y = round_aspect(x / aspect, key=lambda n: 0 if n == 0 else abs(aspect - x / n))
    return x, y


def reducing_factors(width: int, height: int, out_width: int, out_height: int, reducing_gap: float = 2.0) -> Tuple[int, int]:
    """(fx, fy) of the ``reduce`` that ``Image.resize`` runs before resampling the whole image to out_width x out_height."""
    return int(width / out_width / reducing_gap) or 1, int(height / out_height / reducing_gap) or 1


def bicubic(x: float) -> float:
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


class AxisTable(NamedTuple):
    ksize: int
    coef: List[List[int]]    # [out][ksize], zeros behind a row's taps
    first: List[int]         # [out] first source index
    count: List[int]         # [out] taps


@functools.lru_cache(maxsize=64)   # the pages of one scan run share a few sizes; a table is a few thousand Python-float filter values
def axis_table(in_size: int, in0: float, in1: float, out_size: int) -> AxisTable:
    """The taps of one axis: out_size outputs from the span [in0, in1) of in_size source pixels.  Cached: do not modify."""
    in0, in1 = c_float(in0), c_float(in1)
    scale = c_float(in1 - in0) / out_size
    filterscale = scale if scale >= 1.0 else 1.0
    support = BICUBIC_SUPPORT * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    inv = 1.0 / filterscale
    one = float(1 << PRECISION_BITS)
    coef, first, count = [], [], []
    for xx in range(out_size):
        center = in0 + (xx + 0.5) * scale
        xmin = int(center - support + 0.5)
        if xmin < 0:
            xmin = 0
        xmax = int(center + support + 0.5)
        if xmax > in_size:
            xmax = in_size
        xmax -= xmin
        weights, total = [], 0.0
        for x in range(xmax):
            w = bicubic((x + xmin - center + 0.5) * inv)
            weights.append(w)
            total += w
        row = [0] * ksize
        for x, w in enumerate(weights):
            if total != 0.0:
                w /= total
            row[x] = int(-0.5 + w * one) if w < 0 else int(0.5 + w * one)
        coef.append(row)
        first.append(xmin)
        count.append(xmax)
    return AxisTable(ksize, coef, first, count)


class ResamplePlan(NamedTuple):
    size: Tuple[int, int]                 # output (width, height)
    horizontal: Optional[AxisTable]       # None: Pillow skips the pass
    vertical: Optional[AxisTable]


def resample_plan(width: int, height: int, size: Tuple[int, int], box=None) -> ResamplePlan:
    """One call of Pillow's ImagingResample: width x height -> size, from ``box`` (floats; default the whole image)."""
    out_w, out_h = size
    box = (0.0, 0.0, float(width), float(height)) if box is None else tuple(c_float(v) for v in box)
    need_h = out_w != width or box[0] != 0 or box[2] != out_w
    need_v = out_h != height or box[1] != 0 or box[3] != out_h
    return ResamplePlan((out_w, out_h), axis_table(width, box[0], box[2], out_w) if need_h else None,
                        axis_table(height, box[1], box[3], out_h) if need_v else None)


def resize_plans(width: int, height: int, size: Tuple[int, int], box=None) -> List[ResamplePlan]:
    """``Image.resize(size, BICUBIC, box, reducing_gap=None)`` as calls of ImagingResample: one, or for an image more than a
    hundred times taller than wide that loses rows, two -- the vertical pass first, then the horizontal one."""
    out_w, out_h = size
    box = (0.0, 0.0, float(width), float(height)) if box is None else tuple(box)
    if height > width * 100 and out_h < height:
        return [resample_plan(width, height, (width, out_h), (0, box[1], width, box[3])),
                resample_plan(width, out_h, (out_w, out_h), (box[0], 0, box[2], out_h))]
    return [resample_plan(width, height, (out_w, out_h), box)]


class ThumbnailPlan(NamedTuple):
    size: Tuple[int, int]                 # final (width, height)
    factors: Tuple[int, int]              # (fx, fy) of the reduce, (1, 1): none
    reduced: Tuple[int, int]              # size after the reduce
    resamples: List[ResamplePlan]


def thumbnail_plan(width: int, height: int, size) -> Optional[ThumbnailPlan]:
    """``Image.thumbnail((size, size))`` of a fully decoded image (BICUBIC, reducing_gap 2.0, no draft); None: unchanged."""
    final = thumbnail_size(width, height, size)
    if final is None or final == (width, height):
        return None
    fx, fy = reducing_factors(width, height, final[0], final[1])
    box, reduced = None, (width, height)
    if fx > 1 or fy > 1:
        reduced = (-(-width // fx), -(-height // fy))
        box = (0.0, 0.0, width / fx, height / fy)
    return ThumbnailPlan(final, (fx, fy), reduced, resize_plans(reduced[0], reduced[1], final, box))


def random_resize_size(width: int, height: int, downsample_factor: int, min_size: int = 1000) -> float:
    """The (float) side that the reference's random_resize hands to ``thumbnail`` for a drawn factor 1..4."""
    return max(height / downsample_factor, width / downsample_factor, min_size)


def window_starts(side: int, image_size: int) -> List[float]:
    """Float starts of the windows that cover ``side`` pixels: ceil(side / image_size) of them, the surplus spread evenly."""
    windows = math.ceil(side / image_size)
    overlap = (windows * image_size - side) / windows
    return [index * (image_size - overlap) for index in range(windows)]


def patch_origins(width: int, height: int, image_size: int) -> List[Tuple[int, int]]:
    """Integer (x, y) origins of crop_patches' windows, rows first as the reference lists them; both bounds of a window are
    rounded as ``Image.crop`` rounds them and must stay ``image_size`` apart."""
    def rounded(starts):
        out = []
        for start in starts:
            low, high = int(round(start)), int(round(start + image_size))
            if high - low != image_size:
                raise ValueError(f"crop bounds {start} and {start + image_size} round to {high - low} pixels")
            out.append(low)
        return out

    columns = rounded(window_starts(width, image_size))
    return [(x, y) for y in rounded(window_starts(height, image_size)) for x in columns]


def scale_bounding_box(box, box_extent, new_extent) -> List[int]:
    """``box`` = [x0, y0, x1, y1] found on an image of ``box_extent`` = (width, height), carried to ``new_extent``: every bound
    times the axis' float factor, truncated by ``int`` -- written as the reference writes it."""
    box_width, box_height = box_extent
    new_width, new_height = new_extent
    width_factor = new_width / box_width
    height_factor = new_height / box_height
    new_box = [box[0] * width_factor, box[1] * height_factor, box[2] * width_factor, box[3] * height_factor]
    return list(map(int, new_box))
