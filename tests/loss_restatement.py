"""The arithmetic of the three loss-kernel families restated in numpy float32, on the CPU: the per-pixel expression order and
the reduction tree of each kernel, so that the bound constants of loss_cases.py can be measured without a device, and so that
named mistakes (``fault=``) can be shown to break those bounds (test_loss_cases_cpu.py).

  ce_dice      (csrc/loss_ops.hip)  thread (4 pixels of a quad, quads q, q + grid, ...) -> 64-lane xor butterfly -> 4 waves
               (r0 + r1) + (r2 + r3) -> one row per workgroup -> 32 ranges of ceil(blocks / 32) rows, each in order -> the 32 range
               sums in order -> the scalar finish.
  upsample_ce  (csrc/seg_ops.hip)   per-block sums (thread: pixels blk 256 + t + k grid 256; butterfly; 4 waves), finish: lane i adds
               partial[i], partial[i + 64], ..., butterfly.  Backward: 16 lanes per low-resolution cell, lane s takes the footprint
               rows y_lo + s, y_lo + s + 16, ..., every x of the window in order, then a 16-lane butterfly.
  wce          (csrc/doc_ufcn.hip)  256 fixed pixel ranges of ceil(P / 256), thread t takes lo + t, lo + t + 256, ... (the
               weighted term by a fused multiply-add), block sum, then one thread adds the 256 partials in order.

Every operation is an ``np.float32`` operation.  The exponential and the logarithm are ``np.exp2`` / ``np.exp`` / ``np.log`` on
float32: the device's ``__expf`` (2^(x log2 e) on the hardware's exponential), ``expf`` and ``logf`` are NOT restated bit for bit,
and neither is the compiler's contraction of multiply-adds.  The E_log / E_exp parts of the bounds therefore carry the device
routines' documented error, not this module's.

Faults (each restatement takes ``fault=None`` or one of its names):
  ce_dice      no_max_subtract, valid_counts_all_pixels, dice_row_for_out_of_range_label (clamps the label instead of giving a
               zero row), smooth_missing_in_b, drop_last_quad, finish_drops_last_range (a range that is not full is skipped),
               stride_loop_single_pass
  upsample_ce  no_max_subtract, footprint_one_short (the backward's window ends at y_hi - 1), lerp_lambda_fused (the lambda as
               fma(scale, dst, -i0): from the unrounded product, next to an i0 from the rounded one, which is what a compiler
               makes of src - i0 when it may contract it with the product)
  wce          no_max_subtract, weight_sum_counts_ignored, weight_missing_in_grad
"""
import numpy as np

f32 = np.float32
LOG2E = f32(1.4426950408889634)   # 0x1.715476p+0
SMOOTH = f32(1e-5)


def _butterfly(v, lanes=64):
    """v [..., lanes, k]: the xor butterfly o = lanes / 2 ... 1 of ``v += shfl_xor(v, o)``; lane 0's result [..., k]."""
    idx = np.arange(lanes)
    o = lanes // 2
    while o > 0:
        v = v + v[..., idx ^ o, :]
        o >>= 1
    return v[..., 0, :]


def _block_sum4(v):
    """v [blocks, 256, k] -> [blocks, k]: butterfly per wave, then (r0 + r1) + (r2 + r3)."""
    r = _butterfly(v.reshape(v.shape[0], 4, 64, v.shape[-1]))
    return (r[:, 0] + r[:, 1]) + (r[:, 2] + r[:, 3])


def _softmax32(z, fast_exp, fault):
    """z float32 [B, C, n] -> m, s [B, n], e (unnormalised) [B, C, n]; the sum over the classes in class order."""
    m = z.max(axis=1) if fault != "no_max_subtract" else np.zeros((z.shape[0], z.shape[2]), dtype=f32)
    d = z - m[:, None, :]
    e = np.exp2(LOG2E * d) if fast_exp else np.exp(d)
    s = np.zeros_like(m)
    for c in range(z.shape[1]):
        s = s + e[:, c, :]
    return m, s, e.astype(f32)


# ------------------------------------------------------------------------------------------------------------ ce_dice

def ce_dice(z, labels, g=1.0, out_bf16=False, fault=None):
    """z float32 [B, C, n] (bf16 logits: already rounded), labels [B, n] -> dict loss, ce, dice, inv_valid, a, b, grad."""
    with np.errstate(all="ignore"):
        return _ce_dice(np.ascontiguousarray(z, dtype=f32), labels, f32(g), out_bf16, fault)


def _ce_dice(z, labels, g, out_bf16, fault):
    B, C, n = z.shape
    NV = 2 + 3 * C
    m, s, e = _softmax32(z, True, fault)
    inv = f32(1) / s
    p = e * inv[:, None, :]
    valid = (labels >= 0) & (labels < C)
    cls = np.arange(C)[None, :, None]
    hit = labels[:, None, :] == cls
    dice_hit = (np.clip(labels, 0, C - 1)[:, None, :] == cls) if fault == "dice_row_for_out_of_range_label" else hit
    zl = np.where(hit, z, f32(0)).sum(axis=1, dtype=f32)     # (one non-zero term)
    nll = np.where(valid, (m + np.log(s)) - zl, f32(0)).astype(f32)
    vals = np.zeros((B, n, NV), dtype=f32)
    vals[:, :, 0] = nll
    vals[:, :, 1] = 1 if fault == "valid_counts_all_pixels" else valid
    vals[:, :, 2::3] = np.where(dice_hit, p, f32(0)).transpose(0, 2, 1)
    vals[:, :, 3::3] = (p * p).transpose(0, 2, 1)
    vals[:, :, 4::3] = dice_hit.transpose(0, 2, 1)
    # the forward's sums: quad q = flat pixel // 4 (n % 4 == 0), thread (q // 256 % blocks, q % 256), pass q // (blocks 256)
    quads = B * n // 4
    blocks = min((quads + 255) // 256, 512)
    passes = -(-quads // (blocks * 256))
    arr = np.zeros((passes * blocks * 256, 4, NV), dtype=f32)
    arr[:quads] = vals.reshape(quads, 4, NV)
    if fault == "drop_last_quad":
        arr[quads - 1] = 0
    arr = arr.reshape(passes, blocks, 256, 4, NV)
    acc = np.zeros((blocks, 256, NV), dtype=f32)
    for k in range(1 if fault == "stride_loop_single_pass" else passes):
        for q in range(4):
            acc = acc + arr[k, :, :, q, :]
    partial = _block_sum4(acc)
    # finish: 32 ranges of ``per`` rows, each in order, then the ranges in order
    per = -(-blocks // 32)
    tot = np.zeros(NV, dtype=f32)
    for r in range(32):
        k0, k1 = r * per, min(blocks, r * per + per)
        if fault == "finish_drops_last_range" and k1 - k0 < per:
            k1 = k0
        sr = np.zeros(NV, dtype=f32)
        for k in range(k0, k1):
            sr = sr + partial[k]
        tot = tot + sr
    inv_valid = f32(1) / tot[1] if tot[1] > 0 else f32(0)
    ce = tot[0] * inv_valid
    I, D = tot[2::3], tot[3::3] + tot[4::3]
    fC = f32(C)
    dice = f32(0)
    for c in range(C):
        dice = dice + (f32(1) - (f32(2) * I[c] + SMOOTH) / (D[c] + SMOOTH))
    dice = dice / fC
    a = f32(-2) / (fC * (D + SMOOTH))
    num = f32(2) * I if fault == "smooth_missing_in_b" else f32(2) * I + SMOOTH
    b = f32(2) * num / (fC * (D + SMOOTH) * (D + SMOOTH))
    loss = f32(0.5) * ce + f32(0.5) * dice
    # backward: element-wise
    wce, wd = f32(0.5) * g * inv_valid, f32(0.5) * g
    G = np.where(hit, a[None, :, None], f32(0)) + b[None, :, None] * p
    dot = np.zeros_like(m)
    for c in range(C):
        dot = dot + G[:, c, :] * p[:, c, :]
    cepart = np.where(valid[:, None, :], wce * (p - np.where(hit, f32(1), f32(0))), f32(0))
    grad = (cepart + wd * p * (G - dot[:, None, :])).astype(f32)
    if out_bf16:
        from loss_cases import round_bf16
        grad = round_bf16(grad)
    return dict(loss=loss, ce=ce, dice=dice, inv_valid=inv_valid, a=a, b=b, grad=grad)


# ------------------------------------------------------------------------------------------------------------ upsample_ce

def _lerp32(n_in, n_out, fused=False):
    from loss_cases import lerp_tables
    return lerp_tables(n_in, n_out, fused)


def _interp32(x, ty, tx):
    """x float32 [B, C, h, w] -> [B, C, H, W]: l0y (l0x x00 + l1x x01) + l1y (l0x x10 + l1x x11), float32."""
    y0, y1, ly0, ly1, _ = ty
    x0, x1, lx0, lx1, _ = tx
    Y0, Y1, X0, X1 = y0[:, None], y1[:, None], x0[None, :], x1[None, :]
    a0, a1 = ly0[:, None], ly1[:, None]
    b0, b1 = lx0[None, :], lx1[None, :]
    return a0 * (b0 * x[:, :, Y0, X0] + b1 * x[:, :, Y0, X1]) + a1 * (b0 * x[:, :, Y1, X0] + b1 * x[:, :, Y1, X1])


def upsample_ce(x, labels, size, ignore, gloss, fault=None):
    """x float32 [B, C, h, w], labels [B, H, W] -> dict loss [B], grad [B, C, h, w]."""
    with np.errstate(all="ignore"):
        return _upsample_ce(np.ascontiguousarray(x, dtype=f32), labels, size, ignore, np.asarray(gloss, dtype=f32), fault)


def _upsample_ce(x, labels, size, ignore, gloss, fault):
    B, C, h, w = x.shape
    H, W = size
    npix = H * W
    ty, tx = _lerp32(h, H, fault == "lerp_lambda_fused"), _lerp32(w, W, fault == "lerp_lambda_fused")
    v = _interp32(x, ty, tx).astype(f32).reshape(B, C, npix)
    lab = labels.reshape(B, npix)
    valid = lab != ignore
    m, s, e = _softmax32(v, False, fault)
    hit = (lab[:, None, :] == np.arange(C)[None, :, None]) & valid[:, None, :]
    zl = np.where(hit, v, f32(0)).sum(axis=1, dtype=f32)
    nll = np.where(valid, (m + np.log(s)) - zl, f32(0)).astype(f32)
    # forward sums
    bps = min(-(-npix // 1024), 256)
    passes = -(-npix // (bps * 256))
    arr = np.zeros((B, passes * bps * 256), dtype=f32)
    arr[:, :npix] = nll
    arr = arr.reshape(B, passes, bps, 256)
    acc = np.zeros((B, bps, 256), dtype=f32)
    for k in range(passes):
        acc = acc + arr[:, k]
    partial = _block_sum4(acc.reshape(B * bps, 256, 1)).reshape(B, bps)
    rows = -(-bps // 64)
    pp = np.zeros((B, rows * 64), dtype=f32)
    pp[:, :bps] = partial
    pp = pp.reshape(B, rows, 64)
    lane = np.zeros((B, 64), dtype=f32)
    for k in range(rows):
        lane = lane + pp[:, k]
    loss = _butterfly(lane[:, :, None])[:, 0] * (f32(1) / (f32(H) * f32(W)))
    # backward: per cell, 16 lanes over the rows of the window
    inv = f32(1) / s
    gv = np.where(valid[:, None, :], e * inv[:, None, :] - np.where(hit, f32(1), f32(0)), f32(0)).astype(f32).reshape(B, C, H, W)
    y0, y1, ly0, ly1, sy = ty
    x0, x1, lx0, lx1, sx = tx

    def window(i, scale, n_out):
        if not scale > 0:
            return 0, n_out - 1
        inv_s = f32(1) / scale
        lo = int(np.floor(f32(i - 1) * inv_s)) - 1
        hi = int(np.ceil(f32(i + 1) * inv_s)) + 1
        return max(lo, 0), min(hi, n_out - 1)

    wy_all = np.where(y0[:, None] == np.arange(h)[None, :], ly0[:, None], f32(0)) + np.where(y1[:, None] == np.arange(h)[None, :], ly1[:, None], f32(0))
    wx_all = np.where(x0[:, None] == np.arange(w)[None, :], lx0[:, None], f32(0)) + np.where(x1[:, None] == np.arange(w)[None, :], lx1[:, None], f32(0))
    wy_all, wx_all = wy_all.astype(f32), wx_all.astype(f32)     # [H, h], [W, w]: 0 + l0 (+ l1 where i1 = i0), as the kernel adds them
    grad = np.zeros((B, C, h, w), dtype=f32)
    gscale = gloss / f32(npix)
    for i in range(h):
        ylo, yhi = window(i, sy, H)
        if fault == "footprint_one_short":
            yhi -= 1
        for j in range(w):
            xlo, xhi = window(j, sx, W)
            lanes = np.zeros((B, C, 16), dtype=f32)
            for y in range(ylo, yhi + 1):
                wy = wy_all[y, i]
                if wy == 0:
                    continue
                sub = (y - ylo) % 16
                for xx in range(xlo, xhi + 1):
                    wx = wx_all[xx, j]
                    if wx == 0:
                        continue
                    lanes[:, :, sub] = lanes[:, :, sub] + (wy * wx) * gv[:, :, y, xx]
            grad[:, :, i, j] = _butterfly(lanes.transpose(0, 2, 1), 16) * gscale[:, None]
    return dict(loss=loss, grad=grad)


# ------------------------------------------------------------------------------------------------------------ wce

def wce(z, labels, weight, g=1.0, fault=None):
    """z float32 [B, K, n], labels [B, n], weight float32 [K] or None -> dict loss, grad."""
    with np.errstate(all="ignore"):
        return _wce(np.ascontiguousarray(z, dtype=f32), labels, None if weight is None else np.asarray(weight, dtype=f32), f32(g), fault)


def _wce(z, labels, weight, g, fault):
    B, C, n = z.shape
    P = B * n
    valid = (labels >= 0) & (labels < C)
    lab = np.where(valid, labels, 0)
    m, s, e = _softmax32(z, False, fault)
    hit = (labels[:, None, :] == np.arange(C)[None, :, None])
    zl = np.where(hit, z, f32(0)).sum(axis=1, dtype=f32)
    nll = ((np.log(s) + m) - zl).astype(f32)
    wy = (np.ones(C, dtype=f32) if weight is None else weight)[lab]
    wsum_term = np.where(valid, wy, f32(1) if fault == "weight_sum_counts_ignored" else f32(0)).astype(f32)
    wy = np.where(valid, wy, f32(0)).astype(f32)
    per = -(-P // 256)
    passes = -(-per // 256)

    def ranges(a):   # flat pixel -> [256 blocks, passes, 256 threads], zeros beyond each range
        out = np.zeros((256, passes * 256), dtype=f32)
        flat = np.zeros(256 * per, dtype=f32)
        flat[:P] = a.reshape(P)
        out[:, :per] = flat.reshape(256, per)
        return out.reshape(256, passes, 256)

    tw, tn, ts = ranges(wy), ranges(np.where(valid, nll, f32(0))), ranges(wsum_term)
    sl, sw = np.zeros((256, 256), dtype=f32), np.zeros((256, 256), dtype=f32)
    for k in range(passes):
        sl = (tw[:, k].astype(np.float64) * tn[:, k].astype(np.float64) + sl.astype(np.float64)).astype(f32)   # fused multiply-add
        sw = sw + ts[:, k]
    psl, psw = _block_sum4(sl[:, :, None])[:, 0], _block_sum4(sw[:, :, None])[:, 0]
    tl, tws = f32(0), f32(0)
    for i in range(256):
        tl, tws = tl + psl[i], tws + psw[i]
    loss = tl / tws
    gw = (g / tws) * (np.ones_like(wy) if fault == "weight_missing_in_grad" else wy)
    inv = f32(1) / s
    grad = np.where(valid[:, None, :], gw[:, None, :] * (e * inv[:, None, :] - np.where(hit, f32(1), f32(0))), f32(0)).astype(f32)
    return dict(loss=loss, grad=grad)
