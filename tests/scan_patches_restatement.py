"""Numpy restatement of Pillow's 8-bit RGB ``reduce``, BICUBIC ``resize``, ``thumbnail`` and ``crop``, the
yardstick of the scan-patch kernels.  It shares no code with utils/scan_patches.py or csrc/scan_patches.h;
tests/test_scan_patches_cpu.py holds it against Pillow itself, byte for byte.

Shapes are given as Pillow gives them, (width, height); arrays are uint8 [H, W, 3]."""
import math

import numpy as np

PRECISION_BITS = 22

# (W, H) -> (w, h): Image.resize(size, BICUBIC, reducing_gap=None)
RESIZE_CASES = [((37, 29), (9, 7)), ((64, 48), (64, 12)), ((100, 70), (33, 70)), ((131, 97), (40, 31)), ((50, 41), (49, 40)),
                ((257, 123), (65, 31)), ((90, 60), (23, 15)), ((33, 47), (30, 11))]
# (W, H), s: Image.thumbnail((s, s))
THUMBNAIL_CASES = [((403, 297), 100), ((1000, 640), 120), ((517, 333), 64), ((300, 900), 100), ((256, 256), 31), ((801, 603), 50),
                   ((130, 97), 120), ((999, 1), 100), ((640, 480), 80)]
# (W, H), size: crop_patches -- origins 150.5 -> 150 and 151.5 -> 152, zero fill, an exact multiple
CROP_CASES = [((301, 260), 256), ((303, 257), 256), ((1000, 200), 256), ((512, 256), 256)]


def page(width, height, kind, seed=0):
    """A test page: ``random`` bytes, or ``binary`` 0 / 255 (which drives the negative lobes into the clip)."""
    rng = np.random.default_rng(1000 * seed + 7 * width + height)
    if kind == "random":
        return rng.integers(0, 256, (height, width, 3), dtype=np.uint8)
    return (rng.integers(0, 2, (height, width, 3), dtype=np.uint8) * 255).astype(np.uint8)


def _bicubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def axis_tables(in_size, in0, in1, out_size):
    """coef int64 [out, ksize], first [out], count [out] of one axis; in0, in1 as C floats."""
    in0, in1 = np.float32(in0), np.float32(in1)
    scale = float(np.float32(in1 - in0)) / out_size
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    coef = np.zeros((out_size, ksize), dtype=np.int64)
    first = np.zeros(out_size, dtype=np.int64)
    count = np.zeros(out_size, dtype=np.int64)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = float(in0) + (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        weights = [_bicubic((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        total = 0.0
        for w in weights:
            total += w
        for x, w in enumerate(weights):
            if total != 0.0:
                w = w / total
            coef[xx, x] = int(w * (1 << PRECISION_BITS) - 0.5) if w < 0 else int(w * (1 << PRECISION_BITS) + 0.5)
        first[xx], count[xx] = xmin, xmax
    return coef, first, count


def _pass(rows, tables):
    """``rows`` uint8 [n, L, 3] filtered along axis 1."""
    coef, first, count = tables
    out = np.empty((rows.shape[0], len(first), 3), dtype=np.uint8)
    src = rows.astype(np.int64)
    for xx in range(len(first)):
        f, c = int(first[xx]), int(count[xx])
        acc = (1 << (PRECISION_BITS - 1)) + np.tensordot(src[:, f:f + c, :], coef[xx, :c], axes=([1], [0]))
        out[:, xx, :] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return out


def resample(a, size, box=None):
    """Image.resize(size, BICUBIC, box=box, reducing_gap=None) of an RGB image."""
    h, w = a.shape[:2]
    ow, oh = size
    box = (0.0, 0.0, float(w), float(h)) if box is None else tuple(float(np.float32(v)) for v in box)
    need_h = ow != w or box[0] != 0 or box[2] != ow
    need_v = oh != h or box[1] != 0 or box[3] != oh
    if h > w * 100 and oh < h:   # Pillow's order for very tall images: the vertical pass first, as a call of its own
        if need_v:
            a = np.ascontiguousarray(_pass(a.transpose(1, 0, 2), axis_tables(h, box[1], box[3], oh)).transpose(1, 0, 2))
        need_h = ow != w or box[0] != 0 or box[2] != ow
        return _pass(a, axis_tables(w, box[0], box[2], ow)) if need_h else a.copy()
    if need_h:
        a = _pass(a, axis_tables(w, box[0], box[2], ow))
    if need_v:
        a = np.ascontiguousarray(_pass(a.transpose(1, 0, 2), axis_tables(h, box[1], box[3], oh)).transpose(1, 0, 2))
    return a.copy() if not (need_h or need_v) else a


def reduce_multiplier(n):
    return int(np.float32(4294967296.0) / np.float32(256 * n))


def reduce(a, fx, fy):
    """Image.reduce((fx, fy)) of an RGB image: ragged last rows and columns are averaged over the pixels that exist."""
    h, w = a.shape[:2]
    oh, ow = -(-h // fy), -(-w // fx)
    out = np.empty((oh, ow, 3), dtype=np.uint8)
    for oy in range(oh):
        rows = a[oy * fy:(oy + 1) * fy].astype(np.uint64)
        for ox in range(ow):
            block = rows[:, ox * fx:(ox + 1) * fx]
            n = block.shape[0] * block.shape[1]
            s = block.reshape(n, 3).sum(axis=0) + np.uint64(n // 2)
            out[oy, ox] = ((s * np.uint64(reduce_multiplier(n))) & np.uint64(0xFFFFFFFF)) >> np.uint64(24)
    return out


def thumbnail_size(width, height, size):
    """The size Image.thumbnail((size, size)) gives an image, or None where it leaves the image alone."""
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


def thumbnail(a, size):
    """Image.thumbnail((size, size)) of a fully decoded RGB image: BICUBIC, reducing_gap 2.0, no draft."""
    h, w = a.shape[:2]
    final = thumbnail_size(w, h, size)
    if final is None or final == (w, h):
        return a.copy()
    fx = int(w / final[0] / 2.0) or 1
    fy = int(h / final[1] / 2.0) or 1
    box = None
    if fx > 1 or fy > 1:
        a = reduce(a, fx, fy)
        box = (0.0, 0.0, w / fx, h / fy)
    return resample(a, final, box)


def crop_origins(width, height, size):
    """Integer (x, y) origins of the reference's crop_patches windows, rounded as Image.crop rounds its box."""
    nx, ny = math.ceil(width / size), math.ceil(height / size)
    ox, oy = (nx * size - width) / nx, (ny * size - height) / ny
    out = []
    for yi in range(ny):
        sy = yi * (size - oy)
        for xi in range(nx):
            sx = xi * (size - ox)
            x0, y0, x1, y1 = (int(round(v)) for v in (sx, sy, sx + size, sy + size))
            assert x1 - x0 == size and y1 - y0 == size
            out.append((x0, y0))
    return out


def crop(a, origins, size):
    """[n, size, size, 3]: the windows, black where they leave the image."""
    h, w = a.shape[:2]
    out = np.zeros((len(origins), size, size, 3), dtype=np.uint8)
    for i, (x0, y0) in enumerate(origins):
        xa, xb, ya, yb = max(x0, 0), min(x0 + size, w), max(y0, 0), min(y0 + size, h)
        if xa < xb and ya < yb:
            out[i, ya - y0:yb - y0, xa - x0:xb - x0] = a[ya:yb, xa:xb]
    return out
