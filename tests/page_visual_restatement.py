"""Test infrastructure: the page visualisation of DESIGN.md §17, stated a second time and independently of the kernels --
regions, tables and label maps from page_eval_restatement's ``closed_mask`` / ``regions`` / ``twice_area_blocks`` on
rectangular planes, the colouring and the gradient table with numpy, the overlay, outlines by the pixel rule and crops by
slicing.  The product imports none of this (and neither scipy nor cv2)."""
import numpy as np
from scipy import ndimage

import page_eval_restatement as E

GREEN, RED = (0, 255, 0), (255, 0, 0)
STEPS = 100


# ---- regions ---------------------------------------------------------------------------------------------------------------------
def plane_regions(plane: np.ndarray, min_contour_area: int = 10):
    """(rows int32 [n, 8], labels int32 [H, W]): rows = root, x0, y0, w, h, twice_area, kept, 0 in ascending root order; labels
    hold root + 1 on the region's pixels and 0 elsewhere."""
    height, width = plane.shape
    labelled, count = E.regions(E.closed_mask(np.asarray(plane, dtype=np.float32)))
    rows, out = [], np.zeros((height, width), dtype=np.int32)
    for lab, box in enumerate(ndimage.find_objects(labelled), start=1):
        member = labelled[box] == lab
        ys, xs = np.nonzero(member)
        root = int(((ys + box[0].start) * width + xs + box[1].start).min())
        twice_area = E.twice_area_blocks(member)
        rows.append([root, box[1].start, box[0].start, box[1].stop - box[1].start, box[0].stop - box[0].start, twice_area,
                     int(twice_area >= 2 * int(min_contour_area)), 0])
        out[box][member] = root + 1
    rows.sort()
    assert len(rows) == count
    return np.asarray(rows, dtype=np.int32).reshape(-1, 8), out


def page_regions(pred: np.ndarray, background_class_id: int = 0, filter_classes=(), min_contour_area: int = 10):
    """{"rows": [per class int32 [n, 8]], "region_count", "kept_count": int32 [classes], "labels": int32 [classes, H, W]};
    skipped planes have no rows and a zero label plane."""
    classes = pred.shape[0]
    rows, labels = [], np.zeros(pred.shape, dtype=np.int32)
    for k in range(classes):
        if k == background_class_id or k in tuple(filter_classes):
            rows.append(np.zeros((0, 8), dtype=np.int32))
            continue
        table, labels[k] = plane_regions(pred[k], min_contour_area)
        rows.append(table)
    return {"rows": rows, "region_count": np.asarray([len(r) for r in rows], dtype=np.int32),
            "kept_count": np.asarray([int(r[:, 6].sum()) for r in rows], dtype=np.int32), "labels": labels}


def kept_boxes(rows):
    """Inclusive boxes (x0, y0, x0 + w, y0 + h) of the kept rows of every class, class after class."""
    return [(int(r[1]), int(r[2]), int(r[1] + r[3]), int(r[2] + r[4])) for table in rows for r in table if r[6]]


# ---- colouring -----------------------------------------------------------------------------------------------------------------------
def gradient_table(colours) -> np.ndarray:
    """uint8 [classes, 100, 3]: entry t of a class is int(255 + (t / 99) * (c - 255)) per channel in Python floats."""
    table = np.zeros((len(colours), STEPS, 3), dtype=np.uint8)
    for k, colour in enumerate(colours):
        for t in range(STEPS):
            for j in range(3):
                table[k, t, j] = 255 if t == 0 else int(255 + (t / (STEPS - 1)) * (int(colour[j]) - 255))
    return table


def colour_image(pred: np.ndarray, colours, background_class_id: int = 0, confidence: bool = False) -> np.ndarray:
    """uint8 [H, W, 3].  Plain: the colour of the first maximal class.  Confidence: where the float32 sum of the non-background
    planes (class order) is > 0, gradient entry int(100 * max) - 1 of the first maximal class (-1 is the last entry); the
    background colour elsewhere."""
    pred = np.asarray(pred, dtype=np.float32)
    palette = np.asarray(colours, dtype=np.uint8)
    which = pred.argmax(axis=0)   # the first maximum
    if not confidence:
        return palette[which]
    others = np.zeros(pred.shape[1:], dtype=np.float32)
    for k in range(pred.shape[0]):
        if k != background_class_id:
            others = (others + pred[k]).astype(np.float32)
    idx = np.floor(100.0 * pred.max(axis=0).astype(np.float64)).astype(np.int64) - 1   # the maximum is >= 0 where it counts
    idx[(idx < 0) | (idx >= STEPS)] = STEPS - 1
    image = gradient_table(colours)[which, idx]
    image[~(others > 0)] = palette[background_class_id]
    return image


def page_rgb(page: np.ndarray) -> np.ndarray:
    page = np.asarray(page, dtype=np.uint8)
    if page.ndim == 2:
        page = page[:, :, None]
    return np.repeat(page, 3, axis=2) if page.shape[2] == 1 else page.copy()


def overlay(segmented: np.ndarray, page: np.ndarray, background_colour) -> np.ndarray:
    out = page_rgb(page)
    coloured = (segmented != np.asarray(background_colour, dtype=np.uint8)).any(axis=2)
    out[coloured] = segmented[coloured]
    return out


# ---- outlines --------------------------------------------------------------------------------------------------------------------------
def outline(image: np.ndarray, box, colour, stroke: int) -> None:
    """Paints, in place, every pixel of [x0, x1] x [y0, y1] within the image for which one of x - x0, x1 - x, y - y0, y1 - y is
    below ``stroke``."""
    height, width = image.shape[:2]
    x0, y0, x1, y1 = (int(v) for v in box)
    ys, xs = np.mgrid[0:height, 0:width]
    inside = (xs >= x0) & (xs <= x1) & (ys >= y0) & (ys <= y1)
    near = (xs - x0 < stroke) | (x1 - xs < stroke) | (ys - y0 < stroke) | (y1 - ys < stroke)
    image[inside & near] = colour


def draw_boxes(base: np.ndarray, region_boxes, patch_boxes=()) -> np.ndarray:
    out = base.copy()
    for box in region_boxes:
        outline(out, box, GREEN, 3)
    for box in patch_boxes:
        outline(out, box, RED, 1)
    return out


def render(pred, page, colours, background_class_id=0, confidence=False, rows=None, patch_boxes=()):
    """The four pictures of sis_page_render as a dict."""
    segmented = colour_image(pred, colours, background_class_id, confidence)
    boxes = kept_boxes(rows) if rows is not None else []
    return {"segmented": segmented, "overlay": overlay(segmented, page, colours[background_class_id]),
            "boxes_on_page": draw_boxes(page_rgb(page), boxes, patch_boxes),
            "boxes_on_segmented": draw_boxes(segmented, boxes, patch_boxes)}


# ---- crops -----------------------------------------------------------------------------------------------------------------------------
def crop(page: np.ndarray, plane: int, row, labels: np.ndarray, mode: str) -> np.ndarray:
    root, x0, y0, w, h = (int(v) for v in row[:5])
    out = page_rgb(np.asarray(page)[y0:y0 + h, x0:x0 + w])
    if mode == "contour":
        out[labels[plane, y0:y0 + h, x0:x0 + w] != root + 1] = 255
    return out


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------
NOISE_CASES = [(1, (3, 33, 70), 0.15), (2, (3, 96, 160), 0.15), (3, (3, 257, 64), 0.15), (4, (2, 40, 1100), 0.15),
               (5, (4, 130, 130), 0.08)]


def noise_page(seed: int, shape, density: float) -> np.ndarray:
    return E.threshold(E.smooth_noise_planes(np.random.RandomState(seed), shape, density), 0.7)


def noise_scan(seed: int, height: int, width: int, channels: int) -> np.ndarray:
    return np.random.RandomState(1000 + seed).randint(0, 256, (height, width, channels)).astype(np.uint8)


def hand_made_page() -> np.ndarray:
    """float32 [2, 45, 70]: plane 1 holds, off the 32 x 32 tile grid, the ring with an island, the edge shape (in the plane's
    corner), a single pixel, a one-pixel line (area 0), a 2 x 11 bar (twice_area exactly 20, thinner than the stroke) and a
    region that spans four tiles.  The shapes lie more than the closing's reach apart."""
    masks = E.hand_made_masks()
    plane = np.zeros((45, 70), dtype=bool)
    plane[0:12, 0:12] |= masks["edge"]
    plane[25:41, 20:36] |= masks["ring_with_island"]     # rows 27..38, columns 22..33: across the tile borders at 32
    plane[5, 40] = True                                   # single pixel
    plane[8, 22:31] = True                                # one-pixel line
    plane[14:16, 18:29] = True                            # 2 x 11 bar
    plane[18:20, 48:67] = True                            # the last shape: rows 18..41, columns 48..66, over x = 64 and y = 32
    plane[18:42, 58:60] = True
    plane[40:42, 48:67] = True
    pred = np.zeros((2, 45, 70), dtype=np.float32)
    pred[1][plane] = 0.9
    pred[0] = 1.0 - pred[1]
    return pred
