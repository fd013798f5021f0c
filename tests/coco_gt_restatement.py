"""Test infrastructure: the ground-truth contract of DESIGN.md §16 stated a second time, with numpy and scipy and plain loops,
independently of the kernels and of segmentation/evaluation/coco_gt.py: colour-compare masks, the filled regions of
page_eval_restatement.regions in ascending root order, the collinearity rule, COCO's uncompressed run lengths from a
Fortran-order flatten, and the published rleToString / rleFrString codec.  The product imports none of this."""
import numpy as np

import page_eval_restatement as E


# ---- regions and runs ------------------------------------------------------------------------------------------------------
def class_mask(label: np.ndarray, colour) -> np.ndarray:
    """label uint8 [p][p][3] -> bool [p][p]: equal to ``colour`` on all three bytes."""
    return np.all(label == np.asarray(colour, dtype=np.uint8)[None, None, :], axis=2)


def is_degenerate(region: np.ndarray) -> bool:
    """All pixels on one line of the eight-neighbour grid."""
    ys, xs = np.nonzero(region)
    return bool(xs.max() == xs.min() or ys.max() == ys.min() or (xs - ys).max() == (xs - ys).min()
                or (xs + ys).max() == (xs + ys).min())


def turning_points(region: np.ndarray) -> int:
    """Points a CHAIN_APPROX_SIMPLE trace keeps: border pixels (cyclic) at which the direction of travel changes."""
    pts = E.trace_outer_border(region)
    if len(pts) < 2:
        return len(pts)
    n, kept = len(pts), 0
    for i in range(n):
        a, b, c = pts[i - 1], pts[i], pts[(i + 1) % n]
        if (b[0] - a[0], b[1] - a[1]) != (c[0] - b[0], c[1] - b[1]):
            kept += 1
    return kept


def rle_counts(region: np.ndarray):
    """COCO's uncompressed RLE of a boolean plane: column-major, the first count is the number of leading zeros."""
    flat = region.astype(bool).flatten(order="F")
    on = np.nonzero(flat)[0]
    first, last = int(on[0]), int(on[-1])
    counts, value, run = [first], True, 0          # the leading zeros; the loop walks from the first one to the last one
    for v in flat[first:last + 1].tolist():
        if v != value:
            counts.append(run)
            value, run = v, 0
        run += 1
    counts.append(run)                              # the run of ones that ends at the last one
    if last + 1 < flat.size:
        counts.append(flat.size - 1 - last)         # trailing zeros, if there are any
    return counts


def plane_table(mask: np.ndarray):
    """(rows, runs) of one plane: rows [R][8] = root, x0, y0, w, h, area, run_offset, run_count in ascending root order,
    runs the concatenated counts of the kept regions."""
    p = mask.shape[0]
    assert mask.shape == (p, p)
    labels, count = E.regions(mask)
    found = []
    for lab in range(1, count + 1):
        region = labels == lab
        ys, xs = np.nonzero(region)
        found.append((int((ys * p + xs).min()), region, xs, ys))
    found.sort(key=lambda t: t[0])
    rows, runs = [], []
    for root, region, xs, ys in found:
        counts = [] if is_degenerate(region) else rle_counts(region)
        rows.append([root, int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1),
                     int(region.sum()), len(runs), len(counts)])
        runs.extend(counts)
    return np.asarray(rows, dtype=np.int32).reshape(-1, 8), np.asarray(runs, dtype=np.int32)


def label_regions(label: np.ndarray, colours):
    """label uint8 [B][p][p][3], colours [K][3] -> {"has" uint8 [B][K], "region_count", "run_total" int32 [B][K],
    "tables": [[rows]], "runs": [[counts]]}: the whole contract, without capacities."""
    b, k = label.shape[0], len(colours)
    out = {"has": np.zeros((b, k), np.uint8), "region_count": np.zeros((b, k), np.int32), "run_total": np.zeros((b, k), np.int32),
           "tables": [], "runs": []}
    for i in range(b):
        tables, runs = [], []
        for j, colour in enumerate(colours):
            rows, counts = plane_table(class_mask(label[i], colour))
            out["has"][i, j] = int(bool((rows[:, 7] > 0).any())) if len(rows) else 0
            out["region_count"][i, j], out["run_total"][i, j] = len(rows), len(counts)
            tables.append(rows)
            runs.append(counts)
        out["tables"].append(tables)
        out["runs"].append(runs)
    return out


def provider(label: np.ndarray, colours, runs=True):
    """The region-provider interface of segmentation/evaluation/coco_gt.py on the host: (has, tables, runs) with tables[b][k] the
    rows and runs[b][k] the counts of plane (b, k)."""
    r = label_regions(np.asarray(label), colours)
    return r["has"], r["tables"], (r["runs"] if runs else None)


def assert_equal_to_device(result, label: np.ndarray, colours, runs=True, want=None):
    """A sis_hip.LabelRegions (any capacities) against the restatement: totals are the true ones, stored prefixes are right."""
    want = label_regions(label, colours) if want is None else want
    has, region_count, run_total = result.has.cpu().numpy(), result.region_count.cpu().numpy(), result.run_total.cpu().numpy()
    assert np.array_equal(has, want["has"]), (has, want["has"])
    assert np.array_equal(region_count, want["region_count"]), (region_count, want["region_count"])
    assert np.array_equal(run_total, want["run_total"]), (run_total, want["run_total"])
    regions = None if result.regions is None else result.regions.cpu().numpy()
    counts = None if result.runs is None else result.runs.cpu().numpy()
    assert (counts is not None) == bool(runs)
    for b in range(label.shape[0]):
        for k in range(len(colours)):
            rows, seq = want["tables"][b][k], want["runs"][b][k]
            if regions is not None:
                n = min(len(rows), regions.shape[2])
                assert np.array_equal(regions[b, k, :n], rows[:n]), (b, k, regions[b, k, :n], rows[:n])
            if counts is not None:
                n = min(len(seq), counts.shape[2])
                assert np.array_equal(counts[b, k, :n], seq[:n]), (b, k)
    return want


# ---- the string codec (COCO's published rleToString / rleFrString) ------------------------------------------------------------
def rle_to_string(counts) -> str:
    out = []
    for i, x in enumerate(int(c) for c in counts):
        if i > 2:
            x -= int(counts[i - 2])
        more = True
        while more:
            c = x & 0x1F
            x >>= 5   # Python's shift of a negative int is arithmetic
            more = (x != -1) if (c & 0x10) else (x != 0)
            if more:
                c |= 0x20
            out.append(chr(c + 48))
    return "".join(out)


def rle_from_string(s: str):
    counts, at = [], 0
    while at < len(s):
        x, k, more = 0, 0, True
        while more:
            c = ord(s[at]) - 48
            x |= (c & 0x1F) << (5 * k)
            more = bool(c & 0x20)
            at += 1
            k += 1
            if not more and (c & 0x10):
                x |= -1 << (5 * k)
        if len(counts) > 2:
            x += counts[-2]
        counts.append(x)
    return counts


STRING_VECTORS = [([5, 2, 2, 2, 8, 1], "52206O"), ([0, 16], "0`0"), ([16], "`0"), ([5, 3, 2, 3, 3], "53201"),
                  ([0, 1, 65534, 1], "01noo10"), ([70000, 40, 1000000, 3, 5, 700], "`[T2X1Pb`n0kNU^_QOie0")]


# ---- hand-made planes ----------------------------------------------------------------------------------------------------------
def hand_made_planes():
    """name -> (mask bool [p][p], expected rows, expected runs), written out by hand."""
    out = {}
    m = np.zeros((5, 5), bool)
    m[1, 1] = m[2, 1] = m[2, 2] = True                     # an L of three pixels: columns 1 (rows 1, 2) and 2 (row 2)
    out["l_shape"] = (m, [[6, 1, 1, 2, 2, 3, 0, 5]], [6, 2, 4, 1, 12])
    m = np.zeros((7, 7), bool)
    for i in range(3):
        m[i, i] = True                                      # a diagonal stroke ...
    m[6, 4] = m[5, 5] = m[4, 6] = True                      # ... and an anti-diagonal one, not touching it: no runs
    out["strokes"] = (m, [[0, 0, 0, 3, 3, 3, 0, 0], [34, 4, 4, 3, 3, 3, 0, 0]], [])
    m = np.zeros((9, 9), bool)
    m[1:8, 1:8] = True
    m[2:7, 2:7] = False
    m[4, 4] = True                                          # a ring with an island in its hole: one region, filled
    out["ring_with_island"] = (m, [[10, 1, 1, 7, 7, 49, 0, 15]], [10] + [7, 2] * 6 + [7, 10])
    m = np.zeros((4, 4), bool)
    m[0:2, 0:2] = True                                      # holds pixel (0, 0)
    out["first_pixel"] = (m, [[0, 0, 0, 2, 2, 4, 0, 5]], [0, 2, 2, 2, 10])
    m = np.zeros((4, 4), bool)
    m[2:4, 2:4] = True                                      # holds the last pixel: the last count is a run of ones
    out["last_pixel"] = (m, [[10, 2, 2, 2, 2, 4, 0, 4]], [10, 2, 2, 2])
    m = np.ones((3, 3), bool)
    out["full_plane"] = (m, [[0, 0, 0, 3, 3, 9, 0, 2]], [0, 9])
    m = np.zeros((4, 4), bool)
    m[2:4, 1] = True
    m[0:2, 2] = True                                        # the bottom of column 1 and the top of column 2: one run of four
    out["across_columns"] = (m, [[2, 1, 0, 2, 4, 4, 0, 3]], [6, 4, 6])
    return out


def embed(mask: np.ndarray, p: int, y: int, x: int) -> np.ndarray:
    out = np.zeros((p, p), bool)
    out[y:y + mask.shape[0], x:x + mask.shape[1]] = mask
    return out


def isolated_lattice(p: int) -> np.ndarray:
    """The most regions a plane can hold: single pixels on a 2-pixel lattice."""
    m = np.zeros((p, p), bool)
    m[0::2, 0::2] = True
    return m


def l_lattice(p: int) -> np.ndarray:
    """L-shapes of three pixels on a lattice of period 3 in x and y, shifted so that no two touch: many kept regions."""
    m = np.zeros((p, p), bool)
    for y in range(0, p - 1, 3):
        for x in range(0, p - 1, 3):
            m[y, x] = m[y + 1, x] = m[y + 1, x + 1] = True
    return m


def serpentine(p: int) -> np.ndarray:
    """A one-pixel line that runs through the whole plane: rows 0, 2, 4, ... joined alternately at the right and the left."""
    m = np.zeros((p, p), bool)
    for i, y in enumerate(range(0, p, 2)):
        m[y, :] = True
        if y + 1 < p and y + 2 < p:
            m[y + 1, p - 1 if i % 2 == 0 else 0] = True
    return m


def planes_to_label(masks, colours, other=(9, 9, 9)) -> np.ndarray:
    """masks bool [B][K][p][p] (disjoint per image) -> label uint8 [B][p][p][3]; pixels of no class are black, and a sprinkle
    of a colour that is in no class is added where nothing else is."""
    masks = np.asarray(masks)
    b, k, p, _ = masks.shape
    label = np.zeros((b, p, p, 3), np.uint8)
    taken = np.zeros((b, p, p), bool)
    for j in range(k):
        here = masks[:, j] & ~taken
        label[here] = np.asarray(colours[j], np.uint8)
        taken |= here
    rng = np.random.RandomState(p)
    stray = (rng.rand(b, p, p) < 0.05) & ~taken
    label[stray] = np.asarray(other, np.uint8)
    return label
