"""The arithmetic of the six kernels of csrc/upsample_ops.hip restated in numpy float32, on the CPU, in each kernel's association,
so that the bound constants of upsample_cases.py can be measured without a device and named mistakes (``fault=``) can be shown
to break those bounds (test_upsample_cases_cpu.py).

  forward, all three kernels   horizontal, then vertical:  ly0 (lx0 x[i0, j0] + lx1 x[i0, j1]) + ly1 (lx0 x[i1, j0] + lx1 x[i1, j1]).
      generic, tiled           indices and lambdas of the rule (``loss_cases.lerp_tables`` = sis_lerp_index).
      direct                   STATIC indices: output 2j reads (j - 1, j), output 2j + 1 reads (j, j + 1); the lambda is
                               fma(s, o, -i0), the unrounded product (float64 product of two floats, one rounding); column -1
                               is the lane's own first value under weight 0, column w is clamped to w - 1.
  backward, generic            per cell: over the output rows of its window in order  acc += wy racc,  racc the sum over the
                               output columns of its window in order of  wx g;  weight = (i0 == cell) l0 + (i1 == cell) l1.
            direct             the same order on the static window 2j - 1 .. 2j + 2:  hsum = ((w0 c0 + w1 c1) + w2 c2) + w3 c3,
                               acc += wy hsum.
            tiled              rows before columns: tmp[ox] = sum over the window rows 2i - 3 .. 2i + 2 in order of wy g, then
                               the sum over the window columns 2j - 3 .. 2j + 2 in order of wx tmp.
  strided entry                the dense result of the same kernels written to / read from the leading channels of a wide tensor.

Every operation is an ``np.float32`` operation; the compiler's contraction of a multiply-add inside these sums is NOT restated.

Faults:
  scale_in_over_out        scale = in / out instead of (in - 1) / (out - 1)
  i1_not_clamped           i1 = i0 + 1 at the last row / column too: the read goes to what lies behind the row / plane in memory.
                           NOT observable by a value test (test_upsample_cases_cpu.py says why and asserts that it is not)
  clamped_edge_l0_only     backward: where i1 == i0 the cell gets l0 only
  window_short_lo / _hi    backward: the window of candidates one short at its first / last end
  wave_edge_from_shuffle   direct kernels: at a wave boundary the neighbour is what the shuffle returns there (the lane's own
                           value: a shuffle from outside the wave hands back the caller's) instead of the value from memory
  strided_dense_offset     strided entry: image n of the wide tensor addressed with the dense stride
  first_column_weight      direct forward: column -1 (any finite value) under weight 1/2 instead of 0
  lerp_lambda_fused        the rule's lambda from the unrounded product: caught by the exact-zero footprint assertion
"""
import numpy as np

from loss_cases import lerp_tables
from upsample_cases import DIR_B, DIR_F, GEN_B, GEN_F, TIL_B, TIL_F, WAVE_COLS, round_to

f32 = np.float32


def _tables(n_in, n_out, fault):
    if fault == "scale_in_over_out":    # the rule at (in + 1, out + 1) has the scale in / out; its first n_out outputs
        i0, i1, l0, l1, s = lerp_tables(n_in + 1, n_out + 1)
        i0, i1, l0, l1 = i0[:n_out], np.minimum(i1[:n_out], n_in - 1), l0[:n_out], l1[:n_out]
    else:
        i0, i1, l0, l1, s = lerp_tables(n_in, n_out, fused=(fault == "lerp_lambda_fused"))
    if fault == "i1_not_clamped":
        i1 = i0 + 1
    return i0, i1, l0, l1, s


def _static_tables(n_in, n_out, fault):
    """The direct forward's: static indices, lambda = fma(s, o, -i0) with i0 the UNCLAMPED static index."""
    assert n_out == 2 * n_in
    s = lerp_tables(n_in, n_out)[4]
    o = np.arange(n_out)
    j = o // 2
    s0 = np.where(o % 2 == 0, j - 1, j)
    l1 = (np.float64(s) * o.astype(np.float64) - s0).astype(f32)
    l0 = (f32(1) - l1).astype(f32)
    i0 = np.maximum(s0, 0)                                   # column -1: the lane's own first value (weight 0)
    i1 = s0 + 1 if fault == "i1_not_clamped" else np.minimum(s0 + 1, n_in - 1)
    return i0, i1, l0, l1, s


def _behind(x):
    """x [B, C, h, w] -> [B, C, h + 1, w + 1]: index (i, w) and (h, j) read what lies there in memory (the next row, the next
    plane; ones behind the tensor)."""
    B, C, h, w = x.shape
    flat = np.concatenate([x.reshape(-1), np.ones(w + 1, dtype=f32)])
    base = (np.arange(B * C) * h * w).reshape(B, C, 1, 1)
    return flat[base + np.arange(h + 1).reshape(1, 1, -1, 1) * w + np.arange(w + 1).reshape(1, 1, 1, -1)]


def forward(x, size, kernel, dtype="f32", fault=None):
    """x float32 [B, C, h, w] (values of ``dtype``) -> [B, C, oh, ow] float32 holding values of ``dtype``."""
    x = np.ascontiguousarray(x, dtype=f32)
    B, C, h, w = x.shape
    oh, ow = size
    if kernel == DIR_F:
        ty, tx = _static_tables(h, oh, fault), _static_tables(w, ow, fault)
    else:
        assert kernel in (GEN_F, TIL_F)
        ty, tx = _tables(h, oh, fault), _tables(w, ow, fault)
    y0, y1, ly0, ly1, _ = ty
    x0, x1, lx0, lx1, _ = tx
    x0, x1, lx0 = x0.copy(), x1.copy(), lx0.copy()
    if kernel == DIR_F and fault == "wave_edge_from_shuffle":
        for j in range(WAVE_COLS, w, WAVE_COLS):
            x0[2 * j] = j + 3               # lane g (g % 64 == 0) takes its own a[3] for column 4g - 1
            x1[2 * j - 1] = j - 4           # lane g - 1 takes its own a[0] for column 4g
    if kernel == DIR_F and fault == "first_column_weight":
        lx0[0] = f32(0.5)
    xp = _behind(x)
    Y0, Y1, X0, X1 = y0[:, None], y1[:, None], x0[None, :], x1[None, :]
    a0, a1, b0, b1 = ly0[:, None], ly1[:, None], lx0[None, :], lx1[None, :]
    y = a0 * (b0 * xp[:, :, Y0, X0] + b1 * xp[:, :, Y0, X1]) + a1 * (b0 * xp[:, :, Y1, X0] + b1 * xp[:, :, Y1, X1])
    assert y.dtype == f32
    return round_to(y, dtype)


def _weights(n_in, n_out, fault):
    """[out, in] float32: 0 + (i0 == cell) l0 + (i1 == cell) l1, as the kernels add them."""
    i0, i1, l0, l1, s = _tables(n_in, n_out, None if fault == "i1_not_clamped" else fault)
    W = np.zeros((n_out, n_in), dtype=f32)
    o = np.arange(n_out)
    W[o, i0] = l0
    second = np.zeros((n_out, n_in), dtype=f32)
    keep = (i1 != i0) if fault == "clamped_edge_l0_only" else np.ones(n_out, dtype=bool)
    second[o[keep], i1[keep]] = l1[keep]
    return (W + second).astype(f32), s


def _window(n_in, n_out, s, kernel, fault):
    """[out, in] bool: the candidates each cell looks at."""
    cell = np.arange(n_in)
    if kernel == GEN_B:
        if s > 0:
            inv = f32(1) / s
            lo = np.floor((cell - 1).astype(f32) * inv).astype(np.int64)
            hi = np.ceil((cell + 1).astype(f32) * inv).astype(np.int64)
        else:
            lo, hi = np.zeros(n_in, dtype=np.int64), np.full(n_in, n_out - 1)
        lo, hi = np.maximum(lo, 0), np.minimum(hi, n_out - 1)
    else:
        lo, hi = 2 * cell - (1 if kernel == DIR_B else 3), 2 * cell + 2
    if fault == "window_short_lo":
        lo = lo + 1
    if fault == "window_short_hi":
        hi = hi - 1
    o = np.arange(n_out)[:, None]
    return (o >= lo[None, :]) & (o <= hi[None, :])


def backward(gy, in_hw, kernel, dtype="f32", fault=None):
    """gy float32 [B, C, oh, ow] (values of ``dtype``) -> gx [B, C, h, w] float32 holding values of ``dtype``."""
    g = np.ascontiguousarray(gy, dtype=f32)
    B, C, oh, ow = g.shape
    h, w = in_hw
    assert kernel in (GEN_B, TIL_B, DIR_B)
    Wy, sy = _weights(h, oh, fault)
    Wx, sx = _weights(w, ow, fault)
    Wy = np.where(_window(h, oh, sy, kernel, fault), Wy, f32(0))
    Wx = np.where(_window(w, ow, sx, kernel, fault), Wx, f32(0))
    src_col = {}                    # (ox, cell) -> the column actually read
    if kernel == DIR_B and fault == "wave_edge_from_shuffle":
        for j in range(WAVE_COLS, w, WAVE_COLS):
            src_col[(2 * j - 1, j)] = 2 * j + 7        # lane g (g % 64 == 0): its own v[7] for output column 8g - 1
            src_col[(2 * j, j - 1)] = 2 * j - 8        # lane g - 1: its own v[0] for output column 8g
    if kernel == TIL_B:             # rows before columns
        tmp = np.zeros((B, C, h, ow), dtype=f32)
        for oy in range(oh):
            rows = np.nonzero(Wy[oy])[0]
            tmp[:, :, rows, :] = tmp[:, :, rows, :] + Wy[oy, rows][None, None, :, None] * g[:, :, oy, None, :]
        acc = np.zeros((B, C, h, w), dtype=f32)
        for ox in range(ow):
            cols = np.nonzero(Wx[ox])[0]
            acc[:, :, :, cols] = acc[:, :, :, cols] + Wx[ox, cols][None, None, None, :] * tmp[:, :, :, ox, None]
    else:                           # per output row the sum over its columns, then the rows
        racc = np.zeros((B, C, oh, w), dtype=f32)
        for ox in range(ow):
            cols = np.nonzero(Wx[ox])[0]
            read = np.array([src_col.get((ox, int(c)), ox) for c in cols], dtype=np.int64)
            racc[:, :, :, cols] = racc[:, :, :, cols] + Wx[ox, cols][None, None, None, :] * g[:, :, :, read]
        acc = np.zeros((B, C, h, w), dtype=f32)
        for oy in range(oh):
            rows = np.nonzero(Wy[oy])[0]
            acc[:, :, rows, :] = acc[:, :, rows, :] + Wy[oy, rows][None, None, :, None] * racc[:, :, oy, None, :]
    assert acc.dtype == f32
    return round_to(acc, dtype)


def into_wide(wide, x, kernel, dtype="f32", fault=None):
    """``upsample2x_into``: the x2 result of x [B, C, h, w] in the leading C channels of ``wide`` [B, C + S, 2h, 2w] (a copy is
    returned)."""
    B, C, h, w = x.shape
    y = forward(x, (2 * h, 2 * w), kernel, dtype, None if fault == "strided_dense_offset" else fault)
    out = np.array(wide, dtype=f32)
    flat = out.reshape(-1)
    image, plane = out[0].size, 4 * h * w
    for n in range(B):
        at = n * (C * plane if fault == "strided_dense_offset" else image)
        flat[at:at + C * plane] = y[n].reshape(-1)
    return out


def grad_from_wide(gwide, channels, kernel, dtype="f32", fault=None):
    """``upsample2x_grad_from``: the gradient from the leading ``channels`` channels of ``gwide`` [B, C + S, 2h, 2w]."""
    gwide = np.ascontiguousarray(gwide, dtype=f32)
    B, _, oh, ow = gwide.shape
    flat = gwide.reshape(-1)
    image, plane = gwide[0].size, oh * ow
    g = np.stack([flat[(at := n * (channels * plane if fault == "strided_dense_offset" else image)):at + channels * plane]
                  .reshape(channels, oh, ow) for n in range(B)])
    return backward(g, (oh // 2, ow // 2), kernel, dtype, None if fault == "strided_dense_offset" else fault)
