"""The scanner-margin statement of DESIGN.md §20, restated with numpy and scipy.ndimage on the host: the yardstick of
tests/test_scan_margin_cpu.py and tests/test_scan_margin_gpu.py.  Written from §20, not from csrc/scan_margin.h: whole-array
shifts instead of tiles, ``scipy.ndimage.label`` / ``find_objects`` instead of union-find, ``binary_dilation`` /
``binary_erosion`` for the closing, and the reference's own sorted list (a stable Python sort) for the cut.

Like §20 itself this follows OpenCV's documented behaviour (blur with BORDER_REFLECT_101, Canny with aperture 3 and the L1
norm, dilate / erode with the cross, one contour per outer border and per hole border, boundingRect); OpenCV is not
installed here and nothing was compared with it."""
from typing import List, NamedTuple

import numpy as np
from scipy import ndimage

EIGHT = np.ones((3, 3), dtype=bool)
CROSS = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], dtype=bool)


def blur(a):
    """Step 1: the 3x3 box sum over the mirrored image (the edge pixel not repeated), (s + 4) // 9."""
    p = np.pad(a.astype(np.int64), ((1, 1), (1, 1), (0, 0)), mode="reflect")
    h, w = a.shape[:2]
    s = sum(p[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3))
    return (s + 4) // 9


def gradients(b):
    """Step 2: Sobel dx, dy per channel on the replicated image, then the channel with the largest |dx| + |dy| (first on a tie)."""
    p = np.pad(b, ((1, 1), (1, 1), (0, 0)), mode="edge")
    h, w = b.shape[:2]

    def at(dy, dx):
        return p[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]

    gx = (at(-1, 1) + 2 * at(0, 1) + at(1, 1)) - (at(-1, -1) + 2 * at(0, -1) + at(1, -1))
    gy = (at(1, -1) + 2 * at(1, 0) + at(1, 1)) - (at(-1, -1) + 2 * at(-1, 0) + at(-1, 1))
    mag = np.abs(gx) + np.abs(gy)
    best = np.argmax(mag, axis=2)[..., None]   # the first maximum
    return (np.take_along_axis(gx, best, 2)[..., 0], np.take_along_axis(gy, best, 2)[..., 0], np.take_along_axis(mag, best, 2)[..., 0])


def local_maxima(dx, dy, m):
    """Step 3."""
    h, w = m.shape
    p = np.pad(m, 1)   # zeros outside

    def at(oy, ox):
        return p[1 + oy:1 + oy + h, 1 + ox:1 + ox + w]

    x = np.abs(dx).astype(np.int64)
    y = np.abs(dy).astype(np.int64) << 15
    t22 = x * 13573
    t67 = t22 + (x << 16)
    horizontal = y < t22
    vertical = ~horizontal & (y > t67)
    diagonal = ~horizontal & ~vertical
    falling = (dx ^ dy) < 0   # s = -1
    first = np.where(falling, at(-1, 1), at(-1, -1))   # m(y - 1, x - s)
    second = np.where(falling, at(1, -1), at(1, 1))    # m(y + 1, x + s)
    return ((horizontal & (m > at(0, -1)) & (m >= at(0, 1))) | (vertical & (m > at(-1, 0)) & (m >= at(1, 0))) |
            (diagonal & (m > first) & (m > second)))


def hysteresis(maxima, m, low, high):
    """Step 4."""
    candidates = maxima & (m > low)
    labels, count = ndimage.label(candidates, structure=EIGHT)
    has_strong = np.zeros(count + 1, dtype=bool)
    has_strong[np.unique(labels[candidates & (m > high)])] = True
    has_strong[0] = False
    return has_strong[labels]


def closing(edges):
    """Step 5: a pixel outside the image is off for the dilation and on for the erosion."""
    d = ndimage.binary_dilation(edges, structure=CROSS, border_value=0)
    return ndimage.binary_erosion(d, structure=CROSS, border_value=1)


class Contour(NamedTuple):
    kind: int   # 0 outer, 1 hole
    root: int
    x0: int
    y0: int
    w: int
    h: int

    @property
    def area(self):
        return self.w * self.h


def contours(e) -> List[Contour]:
    """Step 6, in its order."""
    h, w = e.shape
    out = []
    for kind, (labels, count) in enumerate((ndimage.label(e, structure=EIGHT), ndimage.label(~e, structure=CROSS))):
        if count == 0:
            continue
        flat = labels.ravel()
        roots = np.full(count + 1, h * w, dtype=np.int64)
        np.minimum.at(roots, flat, np.arange(h * w))
        framed = set(np.unique(np.concatenate([labels[0], labels[-1], labels[:, 0], labels[:, -1]]))) if kind == 1 else set()
        found = []
        for lab, box in enumerate(ndimage.find_objects(labels), start=1):
            if lab in framed:
                continue
            ys, xs = box
            grow = kind
            found.append(Contour(kind, int(roots[lab]), xs.start - grow, ys.start - grow, xs.stop - xs.start + 2 * grow,
                                 ys.stop - ys.start + 2 * grow))
        out += sorted(found, key=lambda c: c.root)
    return out


class Result(NamedTuple):
    box: List[int]
    info: List[int]
    edges: np.ndarray       # uint8 [h, w], 0 / 255
    contours: np.ndarray    # int32 [count, 6]


def decide(found: List[Contour], h: int, w: int):
    """Step 7 on the reference's own list: -> (box, kept, decision, T, largest)."""
    largest = max((c.area for c in found), default=0)
    if len(found) <= 1:
        return [0, 0, w, h], 0, 1, 0, largest
    if float(h * w) * 0.6 > float(largest):
        return [0, 0, w, h], 0, 2, 0, largest
    ordered = sorted(found, key=lambda c: c.area, reverse=True)   # stable: ties stay in step 6's order
    differences = [abs(a.area - b.area) for a, b in zip(ordered, ordered[1:])]
    cut = differences.index(max(differences))
    kept = ordered[:cut + 1]
    box = [min(c.x0 for c in kept), min(c.y0 for c in kept), max(c.x0 + c.w for c in kept), max(c.y0 + c.h for c in kept)]
    return box, len(kept), 0, kept[-1].area, largest


def content_box(a, low=20, high=150) -> Result:
    """Steps 1 to 7 of an analysis image uint8 [h, w, 3]."""
    a = np.asarray(a)
    assert a.dtype == np.uint8 and a.ndim == 3 and a.shape[2] == 3 and min(a.shape[:2]) >= 3
    h, w = a.shape[:2]
    dx, dy, m = gradients(blur(a))
    e = closing(hysteresis(local_maxima(dx, dy, m), m, low, high))
    found = contours(e)
    box, kept, decision, threshold, largest = decide(found, h, w)
    info = [len(found), sum(1 for c in found if c.kind == 0), largest, kept, decision, threshold, int(e.sum()), 0]
    table = np.array([list(c) for c in found], dtype=np.int32).reshape(-1, 6)
    return Result(box, info, (e * 255).astype(np.uint8), table)


def scale_bounding_box(box, box_extent, new_extent):
    """Step 8, as the reference writes it."""
    width_factor = new_extent[0] / box_extent[0]
    height_factor = new_extent[1] / box_extent[1]
    return [int(box[0] * width_factor), int(box[1] * height_factor), int(box[2] * width_factor), int(box[3] * height_factor)]


def remove_margin(page, analysis_size=1000):
    """The reference's remove_scanning_margin on a uint8 [H, W, 3] array with Pillow's own thumbnail: (cropped, box, crop)."""
    from PIL import Image
    image = Image.fromarray(page)
    analysis = image.copy()
    analysis.thumbnail((analysis_size, analysis_size))
    box = content_box(np.asarray(analysis)).box
    crop = scale_bounding_box(box, analysis.size, image.size)
    return np.asarray(image.crop(crop)), box, crop
