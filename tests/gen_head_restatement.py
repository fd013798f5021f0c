"""The kernels of csrc/gen_small_ops.hip restated in numpy float32, in each kernel's own association: what their fp32 arithmetic
gives when every product and every sum is rounded once (the device may contract a product into the following sum; the factor 4
between the figures measured here and the K of gen_head_cases.py is the room for that).  No GPU, numpy only.

  one-wave kernels (pixel_norm, equal_linear, equal_linear_full<NJ>, demod): lane l sums its elements l, l + 64, l + 128, ...
      in ascending order from 0, then the 64 lanes meet in the butterfly of ``sis_wave_sum`` (csrc/sis_device.h): xor 32, 16, .. 1.
  head_gemm<MODE>: one fp32 chain per output, k ascending (the 32x32x2 matrix-core steps taken as two chained terms each).
  to_rgb<VEC>: wave w of four sums the channels w, w + 4, ... in ascending order; the partials are added in wave order to wave
      0's, then the bias, then the skip sum (taps in ``skip_up2``'s order, summed from 0).
  rgb_finish: the blocks in ascending order from 0, then the bias, then the skip sum.
"""
import numpy as np

F = np.float32
EPS = F(1e-8)
_XOR = [np.arange(64) ^ o for o in (32, 16, 8, 4, 2, 1)]


def f32(a):
    return np.ascontiguousarray(np.asarray(a), dtype=F)


def wave_sum(v):
    """[..., 64] -> [...]: the xor butterfly of sis_wave_sum (every lane ends with the same value)."""
    for idx in _XOR:
        v = v + v[..., idx]
    return v[..., 0]


def _lanes(a):
    """[..., n] -> [..., J, 64], zero padded (a lane past n adds nothing)."""
    n = a.shape[-1]
    j = (n + 63) // 64
    out = np.zeros(a.shape[:-1] + (j * 64,), dtype=F)
    out[..., :n] = a
    return out.reshape(a.shape[:-1] + (j, 64))


def _rsqrt(v):
    return F(1) / np.sqrt(v)


def _leaky(v):
    return np.where(v > 0, v, v * F(0.2)) * F(1.4142135623730951)


def pixel_norm(x):
    x = f32(x)
    xl = _lanes(x)
    ss = np.zeros(x.shape[:1] + (64,), dtype=F)
    for j in range(xl.shape[1]):
        ss = ss + xl[:, j] * xl[:, j]
    r = _rsqrt(wave_sum(ss) / F(x.shape[1]) + EPS)
    return x * r[:, None]


def _epilogue(acc, bias, scale, lr_mul, act, times_lr=True):
    v = acc * F(scale)
    if bias is not None:
        b = f32(bias) * F(lr_mul) if times_lr else f32(bias)
        v = v + b[None, :]
    return _leaky(v) if act else v


def equal_linear(x, w, bias, scale, lr_mul, act, times_lr=True):
    """equal_linear_kernel and equal_linear_full_kernel<NJ>: the same order (j ascending per lane, then the butterfly)."""
    xl, wl = _lanes(f32(x)), _lanes(f32(w))
    acc = np.zeros((xl.shape[0], wl.shape[0], 64), dtype=F)
    for j in range(xl.shape[1]):
        acc = acc + xl[:, None, j] * wl[None, :, j]
    return _epilogue(wave_sum(acc), bias, scale, lr_mul, act, times_lr)


def _chain(a, w):
    acc = np.zeros((a.shape[0], w.shape[0]), dtype=F)
    for k in range(a.shape[1]):
        acc = acc + a[:, k, None] * w[None, :, k]
    return acc


def head_gemm_linear(x, w, bias, scale, lr_mul, act, times_lr=True):
    """MODE 0 (EqualLinear wider than 1024) and, with lr_mul = 1 and no activation, MODE 1 (a layer's style vector)."""
    return _epilogue(_chain(f32(x), f32(w)), bias, scale, lr_mul, act, times_lr)


def head_gemm_demod(s, wsq, scale, demodulate=True):
    """MODE 2: (s * scale)^2 chained against wsq, then scale * rsqrt(acc + 1e-8f); ``scale`` itself without demodulation."""
    s, wsq = f32(s), f32(wsq)
    if not demodulate:
        return np.full((s.shape[0], wsq.shape[0]), F(scale), dtype=F)
    t = s * F(scale)
    return F(scale) * _rsqrt(_chain(t * t, wsq) + EPS)


def demod(s, wsq, scale, demodulate=True):
    """demod_kernel (sis_modconv_demod): one wave per (b, co)."""
    s, wsq = f32(s), f32(wsq)
    if not demodulate:
        return np.full((s.shape[0], wsq.shape[0]), F(scale), dtype=F)
    sv = _lanes(s * F(scale))
    wl = _lanes(wsq)
    acc = np.zeros((s.shape[0], wsq.shape[0], 64), dtype=F)
    for j in range(sv.shape[1]):
        acc = acc + (sv[:, None, j] * sv[:, None, j]) * wl[None, :, j]
    return F(scale) * _rsqrt(wave_sum(acc) + EPS)


def prepack_wsq(weight):
    """prepack_kernel's wsq [cout, cin]: the taps of weight [1, cout, cin, k, k] squared and summed in order from 0."""
    w = f32(weight)[0].reshape(weight.shape[1], weight.shape[2], -1)
    ss = np.zeros(w.shape[:2], dtype=F)
    for t in range(w.shape[2]):
        ss = ss + w[:, :, t] * w[:, :, t]
    return ss


def truncate(w, mean, psi):
    w, m = f32(w), f32(mean).reshape(-1)
    return m + F(psi) * (w - m)


def skip_sum(skip, taps, h, w, pad0, swap_sh_sw=False):
    """The upsampled skip image [B, C, h * w] by the polyphase walk of ``skip_up2`` / ``skip_taps`` (the same taps in the same
    order on both routes).  ``swap_sh_sw`` simulates a defect: the skip image's height and width exchanged."""
    skip, taps = f32(skip), f32(taps)
    b, c, sh, sw = skip.shape
    flat = skip.reshape(b, c, sh * sw)
    if swap_sh_sw:
        sh, sw = sw, sh
    kh, kw = taps.shape
    pix = np.arange(h * w)
    y, x = pix // w, pix % w
    mid_x, mid_y = x + 1 - pad0, y + 1 - pad0
    ix0, iy0 = mid_x // 2, mid_y // 2                       # (floor: what the kernel's two-branch division gives)
    kx0, ky0 = (ix0 + 1) * 2 - mid_x - 1, (iy0 + 1) * 2 - mid_y - 1
    u = np.zeros((b, c, h * w), dtype=F)
    for ty in range((kh + 1) // 2):
        for tx in range((kw + 1) // 2):
            iy, ix, fy, fx = iy0 + ty, ix0 + tx, ky0 + 2 * ty, kx0 + 2 * tx
            ok = (iy >= 0) & (iy < sh) & (ix >= 0) & (ix < sw) & (fy < kh) & (fx < kw)
            src = np.clip(iy, 0, sh - 1) * sw + np.clip(ix, 0, sw - 1)
            tap = taps[kh - 1 - np.minimum(fy, kh - 1), kw - 1 - np.minimum(fx, kw - 1)]
            u = np.where(ok[None, None, :], u + flat[:, :, src] * tap[None, None, :], u)
    return u


def to_rgb(x, w, s, bias, scale, skip=None, taps=None, pad0=0, swap_sh_sw=False):
    """x [B, cin, h, w], w [cout, cin], s [B, cin], bias [cout] or None -> [B, cout, h, w]."""
    x, w, s = f32(x), f32(w), f32(s)
    b, cin, h, wd = x.shape
    xf = x.reshape(b, cin, h * wd)
    weff = (F(scale) * w)[None, :, :] * s[:, None, :]
    total = None
    for wave in range(4):
        acc = np.zeros((b, w.shape[0], h * wd), dtype=F)
        for ci in range(wave, cin, 4):
            acc = acc + weff[:, :, ci, None] * xf[:, None, ci, :]
        total = acc if total is None else total + acc
    a = total + (f32(bias).reshape(1, -1, 1) if bias is not None else F(0))
    if skip is not None:
        a = a + skip_sum(skip, taps, h, wd, pad0, swap_sh_sw)
    return a.reshape(b, w.shape[0], h, wd)


def rgb_finish(part, bias, skip=None, taps=None, pad0=0):
    part = f32(part)
    blocks, b, c, h, wd = part.shape
    a = np.zeros((b, c, h * wd), dtype=F)
    for cb in range(blocks):
        a = a + part[cb].reshape(b, c, h * wd)
    a = a + (f32(bias).reshape(1, -1, 1) if bias is not None else F(0))
    if skip is not None:
        a = a + skip_sum(skip, taps, h, wd, pad0)
    return a.reshape(b, c, h, wd)
