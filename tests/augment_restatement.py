"""numpy restatement of the augmentation of DESIGN.md §12, in float64 with an explicit four-tap bilinear; scipy only for the
Gaussian.  It is a restatement of the project's own statement, not of imgaug."""
import numpy as np


def elastic_noise(seed, height, width):
    """[2, H, W] float32: the counter hash of (seed word, component, y * W + x) in uint32 arithmetic."""
    pixel = np.arange(height * width, dtype=np.uint32)
    out = np.empty((2, height * width), dtype=np.float32)
    with np.errstate(over="ignore"):
        for c in range(2):
            key = np.uint32(seed & 0xFFFFFFFF) ^ np.uint32((c * 0x85EBCA77) & 0xFFFFFFFF)
            h = pixel * np.uint32(0x9E3779B1) + key
            h ^= h >> np.uint32(16)
            h *= np.uint32(0x85EBCA6B)
            h ^= h >> np.uint32(13)
            h *= np.uint32(0xC2B2AE35)
            h ^= h >> np.uint32(16)
            out[c] = (h >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -23) - np.float32(1.0)
    return out.reshape(2, height, width)


def elastic_field(noise, sigma, alpha):
    """alpha * gaussian_filter(noise plane) in float64, mirror boundary, truncated at 4 sigma; noise [2, H, W]."""
    from scipy.ndimage import gaussian_filter
    return np.stack([alpha * gaussian_filter(plane.astype(np.float64), sigma, mode="mirror", truncate=4.0) for plane in noise])


def _bilinear_clamped(plane, qx, qy):
    h, w = plane.shape
    qx, qy = np.clip(qx, 0.0, w - 1.0), np.clip(qy, 0.0, h - 1.0)
    x0, y0 = np.floor(qx).astype(np.int64), np.floor(qy).astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    fx, fy = qx - x0, qy - y0
    top = plane[y0, x0] * (1 - fx) + plane[y0, x1] * fx
    bottom = plane[y1, x0] * (1 - fx) + plane[y1, x1] * fx
    return top * (1 - fy) + bottom * fy


def source_coordinates(minv, out_h, out_w, field=None):
    """float64 (s_x, s_y) [out_h, out_w] for the float32 ``minv`` [2, 3] and an optional field [2, H, W]."""
    m = np.asarray(minv, dtype=np.float64)
    y, x = np.mgrid[0:out_h, 0:out_w].astype(np.float64)
    qx = m[0, 0] * x + m[0, 1] * y + m[0, 2]
    qy = m[1, 0] * x + m[1, 1] * y + m[1, 2]
    if field is None:
        return qx, qy
    field = np.asarray(field, dtype=np.float64)
    return qx + _bilinear_clamped(field[0], qx, qy), qy + _bilinear_clamped(field[1], qx, qy)


def warp(pixels, classes, minv, lut, out_h, out_w, field=None, background_id=0):
    """pixels uint8 [H, W, 3], classes uint8 [H, W] -> (values float64 [3, out_h, out_w] in 0..255 units, before any rounding,
    labels int64 [out_h, out_w], (s_x, s_y))."""
    h, w = classes.shape
    sx, sy = source_coordinates(minv, out_h, out_w, field)
    coloured = np.asarray(lut)[pixels].astype(np.float64)
    x0, y0 = np.floor(sx), np.floor(sy)
    fx, fy = sx - x0, sy - y0
    values = np.zeros((3, out_h, out_w))
    for j in (0, 1):
        for i in (0, 1):
            xi, yi = (x0 + i), (y0 + j)
            inside = (xi >= 0) & (xi < w) & (yi >= 0) & (yi < h)
            weight = (fx if i else 1 - fx) * (fy if j else 1 - fy)
            xc, yc = np.clip(xi, 0, w - 1).astype(np.int64), np.clip(yi, 0, h - 1).astype(np.int64)
            values += np.where(inside, weight, 0.0)[None] * coloured[yc, xc].transpose(2, 0, 1)
    nx, ny = np.floor(sx + 0.5), np.floor(sy + 0.5)
    inside = (nx >= 0) & (nx < w) & (ny >= 0) & (ny < h)
    labels = np.where(inside, classes[np.clip(ny, 0, h - 1).astype(np.int64), np.clip(nx, 0, w - 1).astype(np.int64)],
                      background_id).astype(np.int64)
    return values, labels, (sx, sy)


def encode(values):
    """0..255 units -> the loaders' float32 range, with ToTensor's and Normalize's true divisions in float32."""
    v = np.asarray(values, dtype=np.float32)
    return (v / np.float32(255.0) - np.float32(0.5)) / np.float32(0.5)


def decode(images):
    """The inverse of ``encode`` to 0..255 units in float64 (exact up to float32 rounding of the encoding)."""
    return (np.asarray(images, dtype=np.float64) * 0.5 + 0.5) * 255.0


def near_rounding_boundary(sx, sy, eps):
    """True where floor(s + 0.5) could flip under an error of ``eps`` in either axis."""
    def near(s):
        frac = (s + 0.5) - np.floor(s + 0.5)
        return (frac < eps) | (frac > 1 - eps)
    return near(sx) | near(sy)
