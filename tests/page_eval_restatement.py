"""Test infrastructure: the page-evaluation definitions of DESIGN.md §10, stated a second time and independently of the
kernels -- the contour filter with numpy and scipy.ndimage (morphology, hole filling, labelling) plus a plain-Python border
trace with the shoelace formula for the area, voting assembly and the confusion matrix with torch / numpy loops, the metrics
with numpy float64.  The product imports none of this (and neither scipy nor cv2)."""
import numpy as np
import torch
from scipy import ndimage

BOX5 = np.ones((5, 5), dtype=bool)
EIGHT = np.ones((3, 3), dtype=bool)


# ---- contour filter --------------------------------------------------------------------------------------------------------
def threshold(pred: np.ndarray, min_confidence: float) -> np.ndarray:
    pred = np.asarray(pred, dtype=np.float32)
    return np.where(pred < np.float32(min_confidence), np.float32(0), pred)


def closed_mask(q: np.ndarray) -> np.ndarray:
    """(q * 255) >= 1 in float32, then 5x5 closing: dilation ignores what lies outside the plane (0), erosion too (1)."""
    m0 = (q.astype(np.float32) * np.float32(255.0)) >= np.float32(1.0)
    dilated = ndimage.binary_dilation(m0, structure=BOX5, border_value=0)
    return ndimage.binary_erosion(dilated, structure=BOX5, border_value=1)


def regions(mask: np.ndarray):
    """(labels, count): 8-connected components of the mask with everything filled that the 4-connected background cannot
    reach from outside the plane."""
    filled = ndimage.binary_fill_holes(mask)   # default structure: 4-connected background, seeded outside the plane
    return ndimage.label(filled, structure=EIGHT)


def twice_area_blocks(region: np.ndarray) -> int:
    """2 * area by the 2x2-block rule: a block with 4 region pixels counts 1, with 3 counts 1/2 (plane padded with zeros)."""
    r = np.pad(region.astype(np.int64), 1)
    count = r[:-1, :-1] + r[:-1, 1:] + r[1:, :-1] + r[1:, 1:]
    return int(2 * (count == 4).sum() + (count == 3).sum())


_RING = [(0, -1), (-1, -1), (-1, 0), (-1, 1), (0, 1), (1, 1), (1, 0), (1, -1)]   # clockwise from west (y grows downwards)


def trace_outer_border(region: np.ndarray):
    """Pixel centres (x, y) of the outer border of ONE 8-connected region, in order, by Moore neighbour tracing from its first
    pixel in raster order; a pixel is listed every time the border passes through it (thin strokes twice)."""
    r = np.pad(region.astype(bool), 1)
    ys, xs = np.nonzero(r)
    start = (int(ys[0]), int(xs[0]))

    def step(cur, back):
        for k in range(1, 9):
            d = (back + k) % 8
            nxt = (cur[0] + _RING[d][0], cur[1] + _RING[d][1])
            if r[nxt]:
                prev = (cur[0] + _RING[(d - 1) % 8][0], cur[1] + _RING[(d - 1) % 8][1])   # last background pixel looked at
                return nxt, _RING.index((prev[0] - nxt[0], prev[1] - nxt[1]))
        return None, back

    first, back = step(start, 0)
    if first is None:
        return [(start[1] - 1, start[0] - 1)]
    points, cur = [start], first
    for _ in range(8 * r.size + 8):
        nxt, new_back = step(cur, back)
        if cur == start and nxt == first:
            break
        points.append(cur)
        cur, back = nxt, new_back
    else:
        raise RuntimeError("border trace did not close")
    return [(x - 1, y - 1) for y, x in points]


def twice_area_shoelace(region: np.ndarray) -> int:
    pts = trace_outer_border(region)
    total = 0
    for (x0, y0), (x1, y1) in zip(pts, pts[1:] + pts[:1]):
        total += x0 * y1 - x1 * y0
    return abs(total)


def keep_mask(q_plane: np.ndarray, min_contour_area: int) -> np.ndarray:
    labels, count = regions(closed_mask(q_plane))
    if count == 0:
        return np.ones(q_plane.shape, dtype=np.float32)
    lab = np.pad(labels, 1)
    member = (lab > 0).astype(np.int64)
    inside = member[:-1, :-1] + member[:-1, 1:] + member[1:, :-1] + member[1:, 1:]
    which = np.maximum(np.maximum(lab[:-1, :-1], lab[:-1, 1:]), np.maximum(lab[1:, :-1], lab[1:, 1:]))
    twice_area = (2 * np.bincount(which[inside == 4], minlength=count + 1)
                  + np.bincount(which[inside == 3], minlength=count + 1))
    small = twice_area < 2 * int(min_contour_area)
    small[0] = False
    return np.where(small[labels], np.float32(0), np.float32(1))


def remove_small_contours(pred, min_confidence: float, min_contour_area: int, background_class_id: int) -> torch.Tensor:
    q = threshold(torch.as_tensor(pred).cpu().numpy(), min_confidence)
    out = q.copy()
    for b in range(q.shape[0]):
        for c in range(q.shape[1]):
            if c != background_class_id:
                out[b, c] = q[b, c] * keep_mask(q[b, c], min_contour_area)
    return torch.from_numpy(out)


# ---- voting assembly, confusion matrix, class map ------------------------------------------------------------------------------
def assemble_vote(predictions: torch.Tensor, boxes, width: int, height: int) -> torch.Tensor:
    """Sum of the patches' confidences in the order of ``boxes``, divided by the sum over the classes; 0 where that is 0."""
    summed = torch.zeros((predictions.shape[1], height, width), dtype=torch.float32)
    for patch, (left, top, right, bottom) in zip(predictions, boxes):
        right, bottom = min(right, width), min(bottom, height)
        summed[:, top:bottom, left:right] += patch[:, :bottom - top, :right - left]
    total = summed.sum(dim=0, keepdim=True)
    return torch.where(total == 0, torch.zeros_like(summed), summed / total)


def first_max_labels(confidences: torch.Tensor) -> torch.Tensor:
    return torch.max(confidences, dim=0)[1]


def confusion_matrix(labels, ground_truth, num_classes: int) -> np.ndarray:
    labels, ground_truth = np.asarray(labels), np.asarray(ground_truth)
    matrix = np.zeros((num_classes, num_classes), dtype=np.int64)
    for i in range(num_classes):
        for j in range(num_classes):
            matrix[i, j] = np.logical_and(ground_truth == i, labels == j).sum()
    return matrix


def class_id_map(background: str, class_to_color_map: dict) -> dict:
    ids, nxt = {background: 0}, 1
    for name in class_to_color_map:
        if name != background:
            ids[name] = nxt
            nxt += 1
    return ids


def color_to_class(image: np.ndarray, background: str, class_to_color_map: dict) -> np.ndarray:
    ids = class_id_map(background, class_to_color_map)
    out = np.zeros(image.shape[:2], dtype=np.uint8)
    for name, color in class_to_color_map.items():
        if name != background:
            out[(image == np.asarray(color, dtype=image.dtype)).all(axis=2)] = ids[name]
    return out


# ---- metrics ---------------------------------------------------------------------------------------------------------------
def _score(matrix: np.ndarray, k: int, metric: str) -> float:
    tp, predicted, actual = int(matrix[k, k]), int(matrix[:, k].sum()), int(matrix[k, :].sum())
    num, den = {"dice": (2 * tp, predicted + actual), "iou": (tp, predicted + actual - tp), "precision": (tp, predicted),
                "recall": (tp, actual)}[metric]
    return 1.0 if den == 0 else float(np.float64(num) / np.float64(den))


def calculate_metric(matrix, class_names, metric: str) -> dict:
    matrix = np.asarray(matrix, dtype=np.int64)
    total = int(matrix.sum())
    scores = {"weighted_avg": {"score": 0.0}, "weighted_text_avg": {"score": 0.0}}
    text_weight = 0.0
    for k, name in enumerate(class_names):
        weight = float(np.float64(int(matrix[k].sum())) / np.float64(total))
        score = _score(matrix, k, metric)
        scores[name] = {"score": score, "weight": weight}
        scores["weighted_avg"]["score"] += score * weight
        if "text" in name:
            text_weight += weight
    for name in class_names:
        if "text" in name:
            if text_weight > 0:
                scores["weighted_text_avg"]["score"] += scores[name]["score"] * scores[name]["weight"] / text_weight
            else:
                scores["weighted_text_avg"]["score"] = 1.0
    return scores


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def hand_made_masks():
    """name -> boolean mask: the shapes whose area the two formulas must agree on."""
    single = np.zeros((9, 9), dtype=bool)
    single[4, 4] = True
    line = np.zeros((9, 12), dtype=bool)
    line[3, 2:10] = True
    diagonal = np.zeros((10, 10), dtype=bool)
    for i in range(1, 8):
        diagonal[i, i] = True
    ring = np.zeros((16, 16), dtype=bool)
    ring[2:14, 2:14] = True
    ring[4:12, 4:12] = False
    ring[7:9, 7:9] = True   # island in the hole
    edge = np.zeros((12, 12), dtype=bool)
    edge[0:5, 0:7] = True
    edge[5:9, 0:2] = True
    return {"single": single, "line": line, "diagonal": diagonal, "ring_with_island": ring, "edge": edge}


def smooth_noise_planes(rng: np.random.RandomState, shape, density: float, sigma: float = 3.0) -> np.ndarray:
    """float32 confidences in [0, 1]: smoothed noise pushed so that about ``density`` of every plane exceeds 0.7, a second
    band sits between 1/255 and 0.7, and the rest is split between exact zeros and values below 1/255."""
    noise = ndimage.gaussian_filter(rng.rand(*shape), sigma=(0,) * (len(shape) - 2) + (sigma, sigma), mode="wrap")
    lo, hi = np.quantile(noise, 1.0 - 2.0 * density), np.quantile(noise, 1.0 - density)
    out = np.zeros(shape, dtype=np.float32)
    strong, weak = noise >= hi, (noise >= lo) & (noise < hi)
    out[strong] = (0.7 + 0.3 * rng.rand(int(strong.sum()))).astype(np.float32)
    out[weak] = (0.01 + 0.68 * rng.rand(int(weak.sum()))).astype(np.float32)
    faint = (~strong) & (~weak) & (rng.rand(*shape) < 0.3)
    out[faint] = (rng.rand(int(faint.sum())) / 300.0).astype(np.float32)
    speck = rng.rand(*shape) < 0.002   # isolated specks: single-pixel and thin regions
    out[speck] = 0.9
    return out
