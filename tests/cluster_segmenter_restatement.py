"""Test infrastructure: the cluster-based labeller of DESIGN.md §11 stated twice, independently of the kernels.

1. ``segment`` and its steps: the definition, with numpy and scipy.ndimage (cross dilation, hole filling, labelling).
2. ``merge_pairwise``: the reference's merging procedure on pixel sets -- all pairs in order, the first overlapping pair is
   replaced by the hole-filled union, again until no pair overlaps.  It exists to measure how often the definition's group
   merging (difference (a) of §11) gives another result, and on which images.

The product imports none of this (and neither scipy nor cv2)."""
from itertools import combinations

import numpy as np
from scipy import ndimage

from page_eval_restatement import regions, twice_area_blocks

CROSS = ndimage.generate_binary_structure(2, 1)
FINE_GRAINED_CLASS = 'printed_text'


# ---- 1. the definition --------------------------------------------------------------------------------------------------------
def enlarge(low: np.ndarray, size: int) -> np.ndarray:
    """Nearest enlargement of [..., r, r] to [..., size, size]: out[y][x] = low[(y*r)//size][(x*r)//size]."""
    r = low.shape[-1]
    if r > size:
        raise ValueError(f"resolution {r} above the image size {size}")
    idx = (np.arange(size) * r) // size
    return low[..., idx[:, None], idx[None, :]]


def class_masks(cluster_maps: dict, label_map: dict, classes, size: int) -> dict:
    """Step 1: {key: {class: bool [size, size]}} of one image; a class the key's label map does not name is empty."""
    out = {}
    for key, cluster_map in cluster_maps.items():
        big = enlarge(np.asarray(cluster_map), size)
        out[key] = {c: np.isin(big, list(label_map[key].get(c, []))) for c in classes}
    return out


def merge_keys(masks: dict, keys_to_merge: dict, classes) -> dict:
    """Step 2, in dict order."""
    for dest, sources in keys_to_merge.items():
        masks[dest] = {c: np.logical_or.reduce([masks[s][c] for s in sources]) for c in classes}
    return masks


def plane_regions(mask: np.ndarray):
    """Step 3: list of boolean region masks of one plane."""
    dilated = ndimage.binary_dilation(mask, structure=CROSS, border_value=0)
    labels, count = regions(dilated)
    return [labels == k for k in range(1, count + 1)]


def enclosed_gaps(union: np.ndarray):
    """(labels, count) of the 4-connected components of the complement that do not reach the outside of the plane."""
    holes = ndimage.binary_fill_holes(union) & ~union
    return ndimage.label(holes, structure=CROSS)


def merge(regions_per_key, keep_only_overlapping: bool):
    """Step 4: list of (mask, member count), plus the number of gaps that border two or more groups."""
    if any(len(r) == 0 for r in regions_per_key):
        return [], 0
    if len(regions_per_key) == 1:
        return [(r, 1) for r in regions_per_key[0]], 0
    flat = [r for regs in regions_per_key for r in regs]
    parent = list(range(len(flat)))

    def find(a):
        while parent[a] != a:
            a = parent[a]
        return a

    for a, b in combinations(range(len(flat)), 2):
        if (flat[a] & flat[b]).any():
            parent[max(find(a), find(b))] = min(find(a), find(b))
    roots = sorted({find(a) for a in range(len(flat))})
    group_of = np.zeros(flat[0].shape, dtype=np.int64)   # 1 + position in roots, 0 outside the union
    masks, members = [], []
    for position, root in enumerate(roots):
        mine = [flat[a] for a in range(len(flat)) if find(a) == root]
        masks.append(np.logical_or.reduce(mine))
        members.append(len(mine))
        group_of[masks[-1]] = position + 1
    union = group_of > 0
    gaps, count = enclosed_gaps(union)
    shared = 0
    for k in range(1, count + 1):
        gap = gaps == k
        touching = ndimage.binary_dilation(gap, structure=CROSS, border_value=0) & union
        neighbours = np.unique(group_of[touching])
        if len(neighbours) == 1:
            masks[neighbours[0] - 1] = masks[neighbours[0] - 1] | gap
        else:
            shared += 1
    groups = [(m, n) for m, n in zip(masks, members) if n >= 2 or not keep_only_overlapping]
    return groups, shared


def is_small(mask: np.ndarray, min_class_contour_area: int) -> bool:
    return twice_area_blocks(mask) < 2 * int(min_class_contour_area)   # step 5


def segment_image(cluster_maps: dict, spec: dict):
    """One image: cluster_maps {key: int [r, r]} -> (class_map uint8 [S, S], drop flag)."""
    size, names = spec['image_size'], list(spec['class_to_color_map'])
    classes = [n for n in names if n != 'background']
    masks = merge_keys(class_masks(cluster_maps, spec['label_map'], classes, size), spec.get('keys_to_merge', {}), classes)
    fine_keys, det_keys = spec['keys_for_finegrained_segmentation'], spec['keys_for_class_determination']
    text_union = {}
    for c in classes:   # step 6
        groups, _ = merge([plane_regions(masks[k][c]) for k in det_keys], spec['only_keep_overlapping'])
        kept = [m for m, _ in groups if not is_small(m, spec['min_class_contour_area'])]
        text_union[c] = np.logical_or.reduce(kept) if kept else np.zeros((size, size), dtype=bool)
    fine, _ = merge([plane_regions(masks[k][FINE_GRAINED_CLASS]) for k in fine_keys], True)   # step 7
    assigned = []
    for f, _ in fine:   # step 8
        scores = [int((f & text_union[c]).sum()) for c in classes]
        best = int(np.argmax(scores))   # first maximal
        if scores[best] > 0 and not is_small(f, spec['min_class_contour_area']):
            assigned.append((f, classes[best]))
    extent = int(size * 0.95)   # step 9
    drop = False
    for c in classes:
        boxes = []
        for f, name in assigned:
            if name == c:
                ys, xs = np.nonzero(f)
                boxes.append((ys.max() - ys.min() + 1, xs.max() - xs.min() + 1))
        if any(h > extent for h, _ in boxes) and any(w > extent for _, w in boxes):
            drop = True
    class_map = np.full((size, size), names.index('background'), dtype=np.uint8)   # step 10
    paint = masks[fine_keys[-1]][FINE_GRAINED_CLASS]
    for f, name in assigned:
        class_map[f & paint] = names.index(name)
    return class_map, drop


def segment(cluster_maps: dict, spec: dict):
    """Batch: cluster_maps {key: int [B, r, r]} -> (class_map uint8 [B,S,S], colour uint8 [B,S,S,3], drop uint8 [B]).
    spec: image_size, class_to_color_map {name: (r, g, b)}, label_map {key: {class: [cluster ids]}},
    keys_for_class_determination, keys_for_finegrained_segmentation, keys_to_merge, only_keep_overlapping,
    min_class_contour_area."""
    batch = len(next(iter(cluster_maps.values())))
    results = [segment_image({k: np.asarray(v[b]) for k, v in cluster_maps.items()}, spec) for b in range(batch)]
    class_map = np.stack([r[0] for r in results])
    table = np.array([tuple(c)[:3] for c in spec['class_to_color_map'].values()], dtype=np.uint8)
    return class_map, table[class_map], np.array([r[1] for r in results], dtype=np.uint8)


# ---- 2. the reference's procedure on pixel sets ------------------------------------------------------------------------------------
def merge_pairwise(regions_per_key, keep_only_overlapping: bool):
    """List of (mask, member count).  Contours are filled pixel sets; overlap is a shared pixel (the reference's bounding-box
    shortcut, difference (b), is left out on purpose: this function isolates difference (a))."""
    if any(len(r) == 0 for r in regions_per_key):
        return []
    if len(regions_per_key) == 1:
        return [(r, 1) for r in regions_per_key[0]]
    pool = {(i,): r for i, r in enumerate(r for regs in regions_per_key for r in regs)}
    merged = True
    while merged:
        merged = False
        for a, b in combinations(list(pool), 2):
            if (pool[a] & pool[b]).any():
                both = ndimage.binary_fill_holes(pool[a] | pool[b])   # the filled external contour of the union
                del pool[a], pool[b]
                pool[a + b] = both
                merged = True
                break
    return [(m, len(ids)) for ids, m in pool.items() if len(ids) > 1 or not keep_only_overlapping]


def same_groups(a, b) -> bool:
    def canon(groups):
        return sorted((m.tobytes(), n) for m, n in groups)
    return canon(a) == canon(b)


# ---- inputs --------------------------------------------------------------------------------------------------------------------
def smooth_mask(rng: np.random.RandomState, r: int, coverage: float, specks: float = 0.004) -> np.ndarray:
    """bool [r, r]: smoothed noise cut so that about ``coverage`` of the plane is set, plus isolated specks."""
    noise = ndimage.gaussian_filter(rng.rand(r, r), sigma=max(r / 16.0, 1.0), mode='wrap')
    return (noise >= np.quantile(noise, 1.0 - coverage)) | (rng.rand(r, r) < specks)


def smooth_cluster_maps(rng: np.random.RandomState, batch: int, r: int, clusters: int, coverage: float = 0.06) -> np.ndarray:
    """int64 [batch, r, r]: cluster 0 everywhere, then for every other cluster the blobs where a smoothed noise field of its
    own is in its top ``coverage`` share (a later cluster overwrites an earlier one), and specks of any cluster on top.  With
    cluster 0 as background the classes stay below the coverage at which dilated regions span the whole image."""
    sigma = max(r / 24.0, 0.7)
    out = np.zeros((batch, r, r), dtype=np.int64)
    for cluster in range(1, clusters):
        field = ndimage.gaussian_filter(rng.rand(batch, r, r), sigma=(0, sigma, sigma), mode='wrap')
        out[field >= np.quantile(field, 1.0 - coverage)] = cluster
    speck = rng.rand(batch, r, r) < 0.004
    out[speck] = rng.randint(0, clusters, size=int(speck.sum()))
    return out


def random_class_table(rng: np.random.RandomState, keys, clusters: int) -> dict:
    """{key: {cluster id: class name}}: cluster 0 is background, cluster 1 printed_text, the others are drawn."""
    names = list(COLOURS)
    return {k: {0: names[0], 1: names[1], **{i: names[rng.randint(0, 3)] for i in range(2, clusters)}} for k in keys}


# ---- hand-made cases: three clusters per key (0 background, 1 printed_text, 2 handwritten_text), r = S = 64 --------------------
COLOURS = {"background": (0, 0, 0), "printed_text": (0, 0, 255), "handwritten_text": (255, 0, 0)}
KEYS = ("8", "9", "12", "13")
SIZE = 64


def make_spec(size=SIZE, clusters_to_class=None, keys=KEYS, **changes) -> dict:
    """clusters_to_class: {key: {cluster id: class name}}, the layout of merged_classes_K.json."""
    if clusters_to_class is None:
        clusters_to_class = {k: {0: "background", 1: "printed_text", 2: "handwritten_text"} for k in keys}
    label_map = {}
    for key, names in clusters_to_class.items():
        label_map[key] = {}
        for cluster_id, name in names.items():
            label_map[key].setdefault(name, []).append(int(cluster_id))
    spec = {"image_size": size, "class_to_color_map": dict(COLOURS), "label_map": label_map,
            "clusters_to_class": {k: {str(i): n for i, n in v.items()} for k, v in clusters_to_class.items()},
            "keys_for_class_determination": ["8", "9"], "keys_for_finegrained_segmentation": ["12", "13"], "keys_to_merge": {},
            "only_keep_overlapping": False, "min_class_contour_area": 4}
    spec.update(changes)
    return spec


def cluster_map(printed=None, handwritten=None, size=SIZE) -> np.ndarray:
    out = np.zeros((1, size, size), dtype=np.int64)
    if printed is not None:
        out[0][printed] = 1
    if handwritten is not None:
        out[0][handwritten] = 2
    return out


def box(y0, y1, x0, x1, size=SIZE) -> np.ndarray:
    """Rows y0..y1 and columns x0..x1, both inclusive."""
    m = np.zeros((size, size), dtype=bool)
    m[y0:y1 + 1, x0:x1 + 1] = True
    return m


def shapes() -> dict:
    """The pieces of the merge cases.  A dilated piece is one pixel larger on every side, so pieces drawn two pixels apart
    touch after the dilation without sharing a pixel, and pieces drawn one pixel apart or closer share pixels."""
    ring = box(10, 40, 10, 40) & ~box(14, 36, 14, 36)
    blob = box(22, 28, 22, 28)
    c_shape = (box(10, 40, 10, 13) | box(10, 13, 10, 40) | box(37, 40, 10, 40))          # open to the right
    touching_bar = box(10, 40, 43, 46)                                                     # two pixels right of the C's arms
    left_half = box(10, 40, 10, 13) | box(10, 13, 10, 30) | box(37, 40, 10, 30)
    right_half = box(10, 40, 43, 46) | box(10, 13, 30, 46) | box(37, 40, 30, 46)           # shares column 30 with left_half
    inside = box(22, 28, 24, 30)                                                           # well inside the enclosed area
    in_hole = box(16, 18, 16, 18)                                                          # in the ring's hole, away from the blob
    return {"ring": ring, "blob": blob, "c_shape": c_shape, "touching_bar": touching_bar, "left_half": left_half,
            "right_half": right_half, "inside": inside, "in_hole": in_hole}


def hand_made_cases() -> dict:
    """name -> (cluster maps {key: int64 [1, 64, 64]}, spec).  What each must give is asserted in tests/test_cluster_segmenter_cpu.py."""
    s = shapes()
    everything, nothing = box(0, SIZE - 1, 0, SIZE - 1), np.zeros((SIZE, SIZE), dtype=bool)
    fine_inside = cluster_map(printed=s["inside"])
    cases = {}
    # text regions of the two layers; a fine region strictly inside the enclosed area is painted only when that area is filled
    cases["ring_and_blob"] = ({"8": cluster_map(printed=s["ring"]), "9": cluster_map(printed=s["blob"]),
                               "12": cluster_map(printed=s["in_hole"]), "13": cluster_map(printed=s["in_hole"])},
                              make_spec(only_keep_overlapping=True))
    cases["c_closed_by_touching_piece"] = ({"8": cluster_map(printed=s["c_shape"]), "9": cluster_map(printed=s["touching_bar"]),
                                           "12": fine_inside, "13": fine_inside}, make_spec())
    cases["halves_enclosing_a_gap"] = ({"8": cluster_map(printed=s["left_half"]), "9": cluster_map(printed=s["right_half"]),
                                       "12": fine_inside, "13": fine_inside}, make_spec(only_keep_overlapping=True))
    cases["one_key_empty"] = ({"8": cluster_map(printed=everything), "9": cluster_map(printed=nothing),
                              "12": fine_inside, "13": fine_inside}, make_spec())
    cases["single_key_flag_set"] = ({"8": cluster_map(printed=everything), "9": cluster_map(printed=nothing),
                                    "12": fine_inside, "13": cluster_map(printed=nothing)},
                                   make_spec(keys_for_class_determination=["8"], keys_for_finegrained_segmentation=["12"],
                                             only_keep_overlapping=True))
    # the dilated bar shares ten columns with each of the two dilated text blocks
    text = cluster_map(printed=box(10, 40, 10, 19), handwritten=box(10, 40, 24, 33))
    bar = cluster_map(printed=box(20, 23, 12, 31))
    cases["score_tie"] = ({"8": text, "9": text, "12": bar, "13": bar}, make_spec())
    swapped = make_spec()
    swapped["class_to_color_map"] = {"background": (0, 0, 0), "handwritten_text": (255, 0, 0), "printed_text": (0, 0, 255)}
    cases["score_tie_other_order"] = ({"8": text, "9": text, "12": bar, "13": bar}, swapped)
    # a tall and a wide region that do not meet: 62 rows and 61 columns after the dilation, above int(64 * 0.95) = 60
    tall, wide = box(0, 60, 63, 63), box(63, 63, 0, 59)
    bars = cluster_map(printed=tall | wide)
    all_printed = cluster_map(printed=everything)
    cases["drop_same_class"] = ({"8": all_printed, "9": all_printed, "12": bars, "13": bars}, make_spec())
    split = cluster_map(printed=box(0, 55, 50, 63), handwritten=box(60, 63, 0, 45))
    cases["no_drop_different_classes"] = ({"8": split, "9": split, "12": bars, "13": bars}, make_spec())
    # a region through both tile borders of a 64 x 64 plane that also touches the plane's edge
    plus = box(0, 50, 30, 34) | box(30, 34, 5, 63)
    cases["across_tiles_and_edge"] = ({"8": all_printed, "9": all_printed, "12": cluster_map(printed=plus),
                                      "13": cluster_map(printed=plus | box(55, 58, 2, 8))}, make_spec())
    return cases


def area_threshold_case():
    """(cluster maps, spec without min_class_contour_area, 2*area of the only fine region)."""
    piece = box(20, 25, 20, 28)
    fine = cluster_map(printed=piece)
    whole = cluster_map(printed=box(0, SIZE - 1, 0, SIZE - 1))
    dilated = ndimage.binary_dilation(piece, structure=CROSS)
    return {"8": whole, "9": whole, "12": fine, "13": fine}, make_spec(), twice_area_blocks(dilated)


def write_segmenter_files(base_dir, spec: dict, num_clusters: int, channels: dict = None, rng=None) -> None:
    """catalogs/{K}.json with one .npy of unit centres per catalogued key, and merged_classes_{K}.json."""
    import json
    import os
    rng = rng or np.random.RandomState(0)
    os.makedirs(os.path.join(base_dir, "catalogs", str(num_clusters)), exist_ok=True)
    files = {}
    for key in spec["clusters_to_class"]:
        centres = rng.randn(num_clusters, (channels or {}).get(key, 4)).astype(np.float32)
        centres /= np.linalg.norm(centres, axis=1, keepdims=True)
        files[key] = os.path.join(str(num_clusters), f"centres_{key}.npy")
        np.save(os.path.join(base_dir, "catalogs", files[key]), centres)
    with open(os.path.join(base_dir, "catalogs", f"{num_clusters}.json"), "w") as f:
        json.dump({"catalogs": files}, f)
    with open(os.path.join(base_dir, f"merged_classes_{num_clusters}.json"), "w") as f:
        json.dump(spec["clusters_to_class"], f)


def segmenter_arguments(base_dir, spec: dict, num_clusters: int) -> dict:
    return dict(base_dir=base_dir, image_size=spec["image_size"],
                class_to_color_map={n: "#%02x%02x%02x" % tuple(c) for n, c in spec["class_to_color_map"].items()},
                keys_to_merge=spec["keys_to_merge"], only_keep_overlapping=spec["only_keep_overlapping"],
                keys_for_class_determination=spec["keys_for_class_determination"],
                keys_for_finegrained_segmentation=spec["keys_for_finegrained_segmentation"], num_clusters=num_clusters,
                min_class_contour_area=spec["min_class_contour_area"])
