"""Deterministic analysis images for the scanner-margin tests, with the results that the constructions were
made for.  Everything is generated from a seed; nothing is read from a file.  Sizes are (width, height) as Pillow writes them,
arrays uint8 [height, width, 3]."""
import numpy as np

PAPER, BED, BLOB = 225, 25, 60

# (width, height), paper rectangle (x0, y0, x1, y1), the box the tool must find: the paper grown by one pixel
SCANS = [((200, 150), (20, 15, 180, 140), [19, 14, 181, 141]),
         ((97, 131), (5, 6, 92, 120), [4, 5, 93, 121]),
         ((640, 900), (40, 30, 600, 880), [39, 29, 601, 881])]
SCAN_SEEDS = (0, 1, 2)
TOOL_SCAN = ((1000, 707), (60, 40, 950, 670), [59, 39, 951, 671])   # the tool's real analysis size for a landscape A4 page


def scan(size, paper, seed, blobs=40, noise=3):
    """Paper of value 225 on a scanner bed of 25, ``blobs`` dark rectangles of 2..6 pixels a side well inside the paper (ink),
    and uniform noise of +-``noise`` on every byte."""
    w, h = size
    rng = np.random.RandomState(seed)
    a = np.full((h, w), BED, dtype=np.int64)
    x0, y0, x1, y1 = paper
    a[y0:y1, x0:x1] = PAPER
    for _ in range(blobs):
        bw, bh = rng.randint(2, 7, size=2)
        bx = rng.randint(x0 + 4, max(x0 + 5, x1 - 4 - bw))
        by = rng.randint(y0 + 4, max(y0 + 5, y1 - 4 - bh))
        a[by:by + bh, bx:bx + bw] = BLOB
    a = a[..., None] + rng.randint(-noise, noise + 1, size=(h, w, 3))
    return np.clip(a, 0, 255).astype(np.uint8)


def grey(plane):
    return np.repeat(np.asarray(plane, dtype=np.uint8)[..., None], 3, axis=2)


def small_paper():
    return scan((200, 150), (60, 50, 140, 100), 0)


def no_margin():
    return scan((200, 150), (0, 0, 200, 150), 0)


def uniform():
    return grey(np.full((50, 60), 128))


def one_contour():
    plane = np.full((40, 50), 20)
    plane[20, 25] = 255
    return grey(plane)


def nested():
    plane = np.full((120, 120), 20)
    plane[10:110, 10:110] = 230
    plane[30:90, 30:90] = 20
    plane[50:70, 50:70] = 230
    return grey(plane)


def two_squares(side=6, width=140, height=64, xs=(20, 100)):
    """Two equal bright squares: four contours (two outers, two holes) with ONE area."""
    plane = np.full((height, width), 20)
    top = (height - side) // 2
    for x in xs:
        plane[top:top + side, x:x + side] = 230
    return grey(plane)


# The all-equal rule needs decision 0, i.e. ONE area of at least 0.6 of the image, which two disjoint boxes cannot have: the
# squares are grown until they touch.  What is left is one rectangle, whose outer contour and whose hole have the same box (the
# hole's, grown by one pixel, IS the outer's): two contours of one area, the first of which is kept.
TWO_SQUARES_GROWN = dict(side=40, width=100, height=48, xs=(10, 50))


def chain(ramp=True, transpose=False):
    """160 x 40: upper half 100, lower half 110 + max(0, 60 - 5 x): a step that is strong at the left end only and weak (above
    `low`, below `high`) along the rest, across five 32-pixel tiles.  Without the ramp the step is weak everywhere."""
    plane = np.full((40, 160), 100)
    lower = 110 + np.maximum(0, 60 - 5 * np.arange(160)) if ramp else np.full(160, 110)
    plane[20:] = lower[None, :]
    return grey(plane.T if transpose else plane)


def diagonal_chain(ramp=True):
    """100 x 100: 100 above the main diagonal, 112 (+ the ramp) on and below it."""
    y, x = np.mgrid[0:100, 0:100]
    lower = 112 + (np.maximum(0, 60 - 5 * x) if ramp else 0)
    return grey(np.where(y >= x, lower, 100))


def channel_step(all_channels):
    """A vertical step 30 -> 200 at x = 20 of a 40 x 30 image: in all three channels, or in channel 2 only."""
    a = np.full((30, 40, 3), 30, dtype=np.uint8)
    if all_channels:
        a[:, 20:] = 200
    else:
        a[:, 20:, 2] = 200
    return a


RANDOM_SIZES = [(3, 3), (33, 31), (64, 64), (120, 100)]


def random_bytes(size, seed=7):
    w, h = size
    return np.random.RandomState(seed).randint(0, 256, size=(h, w, 3)).astype(np.uint8)


def all_cases():
    """(name, image) of every case of the GPU tests."""
    out = []
    for size, paper, _ in SCANS:
        out += [(f"scan_{size[0]}x{size[1]}_s{seed}", scan(size, paper, seed)) for seed in SCAN_SEEDS]
    out += [("small_paper", small_paper()), ("no_margin", no_margin()), ("uniform", uniform()), ("one_contour", one_contour()),
            ("nested", nested()), ("two_squares", two_squares()), ("two_squares_grown", two_squares(**TWO_SQUARES_GROWN)),
            ("chain", chain()), ("chain_flat", chain(ramp=False)), ("chain_transposed", chain(transpose=True)),
            ("chain_diagonal", diagonal_chain()), ("chain_diagonal_flat", diagonal_chain(ramp=False)),
            ("channel_all", channel_step(True)), ("channel_2", channel_step(False))]
    out += [(f"random_{w}x{h}", random_bytes((w, h))) for w, h in RANDOM_SIZES]
    out.append(("scan_1000x707", scan(TOOL_SCAN[0], TOOL_SCAN[1], 0)))
    return out


# pages for the tool: (name, width, height); the first and the last are shrunk to the 1000-pixel analysis image, the second is not
TOOL_PAGES = [("a/wide.png", 1400, 1000), ("a/b/small.png", 640, 880), ("tall.png", 900, 1300)]


def margin_page(width, height, seed):
    """A text-like page (tests/scan_patches_pages.py) on a scanner bed: the paper leaves 5 % of each side free."""
    import scan_patches_pages as P
    rng = np.random.RandomState(seed)
    a = np.clip(BED + rng.randint(-3, 4, size=(height, width, 3)), 0, 255).astype(np.uint8)
    x0, y0 = width // 20, height // 20
    a[y0:height - y0, x0:width - x0] = P.synthetic_page(width - 2 * x0, height - 2 * y0, seed)
    return a


def write_tool_pages(root):
    from PIL import Image
    for seed, (name, width, height) in enumerate(TOOL_PAGES):
        path = root / name
        path.parent.mkdir(parents=True, exist_ok=True)
        Image.fromarray(margin_page(width, height, seed)).save(path)
    return root
