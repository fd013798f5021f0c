"""The validation pass (``sis_seg_eval``) restated in numpy float64 on the CPU.  Shares no code with the binding or
the kernel: the float32 source-index rule of bilinear interpolation (align_corners=True) is derived here again, everything after
it is float64.

Per output pixel: v[c] = the stored logit (logits at the size of the labels) or ly0 (lx0 a + lx1 b) + ly1 (lx0 c + lx1 d) over the
2x2 neighbourhood with the float32 lambdas; prediction = the first maximal class; label l in [0, C): matrix[l][pred] += 1,
counted += 1, ce += -log softmax(v)[l]; any other label: ignored += 1; always I_c += p_c [l == c], P_c += p_c^2, T_c += [l == c].

``reference`` also returns what the tests' rule for the counts needs and the kernel knows nothing of: ``undecided``, the pixels
whose two largest values are closer than 12 * 2^-24 * max_c sum |w x| (twice the rounding bound of the four products and three
sums of the float32 interpolation): the device may take either of the two classes there.  The bound on ``sums`` is the same on
both routes and carries no allowance for the float32 rounding of the interpolated values.
"""
import collections

import numpy as np

U = 2.0 ** -24

Reference = collections.namedtuple("Reference", "counts sums undecided second values")


def lerp_tables(n_in, n_out):
    """float32: scale = (in - 1) / (out - 1) (0 for out = 1), src = scale * dst rounded to float32, i0 = (int) src clamped to
    in - 1, i1 = i0 + (i0 < in - 1), l1 = src - i0, l0 = 1 - l1."""
    one = np.float32(1)
    scale = np.float32(n_in - 1) / np.float32(n_out - 1) if n_out > 1 else np.float32(0)
    src = (scale * np.arange(n_out).astype(np.float32)).astype(np.float32)
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = np.where(i0 < n_in - 1, i0 + 1, i0)
    l1 = (src - i0.astype(np.float32)).astype(np.float32)
    l0 = (one - l1).astype(np.float32)
    return i0, i1, l0, l1


def pixel_values(logits, size):
    """logits [B, C, h, w] -> (v float64 [B, C, H, W], magnitude float64 [B, H, W] = max_c sum |w x|; 0 at full size)."""
    x = np.asarray(logits, dtype=np.float64)
    B, C, h, w = x.shape
    H, W = size
    if (h, w) == (H, W):
        return x, np.zeros((B, H, W))
    y0, y1, ly0, ly1 = lerp_tables(h, H)
    x0, x1, lx0, lx1 = lerp_tables(w, W)
    Y0, Y1, X0, X1 = y0[:, None], y1[:, None], x0[None, :], x1[None, :]
    a0, a1 = ly0.astype(np.float64)[:, None], ly1.astype(np.float64)[:, None]
    b0, b1 = lx0.astype(np.float64)[None, :], lx1.astype(np.float64)[None, :]
    p00, p01, p10, p11 = x[:, :, Y0, X0], x[:, :, Y0, X1], x[:, :, Y1, X0], x[:, :, Y1, X1]
    v = a0 * (b0 * p00 + b1 * p01) + a1 * (b0 * p10 + b1 * p11)
    mag = np.abs(a0 * b0 * p00) + np.abs(a0 * b1 * p01) + np.abs(a1 * b0 * p10) + np.abs(a1 * b1 * p11)
    return v, mag.max(axis=1)


def reference(logits, labels, size=None):
    """logits float [B, C, h, w] (the values the device is given: bf16-representable for a bf16 case), labels int [B, H, W]."""
    labels = np.asarray(labels, dtype=np.int64)
    B, H, W = labels.shape
    size = (H, W) if size is None else tuple(size)
    assert size == (H, W)
    v, mag = pixel_values(logits, size)
    C = v.shape[1]
    pred = np.argmax(v, axis=1)                                   # the first maximal class
    top = np.take_along_axis(v, pred[:, None], axis=1)[:, 0]
    masked = v.copy()
    np.put_along_axis(masked, pred[:, None], -np.inf, axis=1)
    second = np.argmax(masked, axis=1)
    gap = top - np.take_along_axis(v, second[:, None], axis=1)[:, 0]
    undecided = gap < 12 * U * mag
    valid = (labels >= 0) & (labels < C)
    counts = np.zeros(C * C + 2, dtype=np.int64)
    counts[:C * C] = np.bincount((labels[valid] * C + pred[valid]).ravel(), minlength=C * C)
    counts[C * C] = int(valid.sum())
    counts[C * C + 1] = int((~valid).sum())
    e = np.exp(v - top[:, None])
    others = e.copy()
    np.put_along_axis(others, pred[:, None], 0.0, axis=1)
    r = others.sum(axis=1)
    p = e / (1.0 + r)[:, None]
    safe = np.where(valid, labels, 0)
    v_l = np.take_along_axis(v, safe[:, None], axis=1)[:, 0]
    ce = np.log1p(r) + (top - v_l)
    sums = np.zeros(1 + 3 * C)
    sums[0] = ce[valid].sum()
    for c in range(C):
        hit = labels == c
        sums[1 + 3 * c] = p[:, c][hit].sum()
        sums[2 + 3 * c] = (p[:, c] ** 2).sum()
        sums[3 + 3 * c] = hit.sum()
    return Reference(counts, sums, undecided, second, v)


def check_counts(got, ref, labels, exact=False):
    """``got`` int64 [C*C + 2] from the device against ``ref``: equal, except that an undecided pixel may sit in the cell of its
    second class instead.  ``exact``: no pixel is excused (interpolated values that are exact in float32, or full size)."""
    got = np.asarray(got, dtype=np.int64)
    C = ref.values.shape[1]
    labels = np.asarray(labels, dtype=np.int64)
    assert got[C * C] == ref.counts[C * C] and got[C * C + 1] == ref.counts[C * C + 1], (got[C * C:], ref.counts[C * C:])
    und = ref.undecided & (labels >= 0) & (labels < C)
    if exact or not und.any():
        assert np.array_equal(got, ref.counts), (got[:C * C].reshape(C, C), ref.counts[:C * C].reshape(C, C))
        return 0
    pred = np.argmax(ref.values, axis=1)
    decided = ref.counts[:C * C] - np.bincount((labels[und] * C + pred[und]).ravel(), minlength=C * C)
    room = np.bincount((labels[und] * C + pred[und]).ravel(), minlength=C * C) + \
        np.bincount((labels[und] * C + ref.second[und]).ravel(), minlength=C * C)
    extra = got[:C * C] - decided
    assert (extra >= 0).all() and (extra <= room).all() and extra.sum() == und.sum(), (extra.reshape(C, C), room.reshape(C, C))
    return int(und.sum())


def sums_bound(ref, n_thread):
    """|device - reference| <= (n_thread + 8) * 2^-24 * sum |term| per entry (every term is non-negative: the sum of the absolute
    terms is the entry itself), on both routes."""
    return (n_thread + 8) * U * np.abs(ref.sums)


# ---- the cases ---------------------------------------------------------------------------------------------------------------

CLASS_COUNTS = list(range(2, 17))
FULL_SHAPES = [(1, 1, 1), (3, 5, 7), (2, 4, 4), (3, 1, 13), (2, 17, 9)]
EXACT_SCALES = [((3, 3), (5, 5)), ((5, 5), (9, 9)), ((2, 2), (5, 5)), ((9, 9), (33, 33)), ((3, 5), (9, 9))]
GENERAL_SCALES = [((5, 6), (13, 11)), ((4, 4), (31, 29)), ((7, 5), (23, 37)), ((32, 32), (256, 256))]
ODD_LABELS = (-1, 255, -100)   # and `classes` itself


def tie_logits(rng, shape):
    """Small integers (exact in bf16 and in every float32 interpolation at a power-of-two scale): ties are frequent."""
    return rng.integers(-2, 3, size=shape).astype(np.float32)


def labels_with_ignored(rng, shape, classes, share=0.2):
    lab = rng.integers(0, classes, size=shape).astype(np.int64)
    odd = np.array(ODD_LABELS + (classes,), dtype=np.int64)
    mask = rng.random(shape) < share
    lab[mask] = odd[rng.integers(0, len(odd), size=int(mask.sum()))]
    return lab


def to_bf16_values(x):
    """float32 values rounded to the nearest bfloat16 (ties to even), still float32."""
    bits = np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    bits = (bits + 0x7FFF + ((bits >> 16) & 1)) & 0xFFFF0000
    return bits.astype(np.uint32).view(np.float32)
