"""Emulation and bounds of the bf16 modulated convolution (csrc/modconv_bf16.h), shared by tests/test_modconv_bf16_*.py.

The contract: y = dscale * sum bf16(W) * bf16(fl32(s * x)), both conversions round-to-nearest-even, fp32 accumulation.  The
emulation rounds the operands exactly that way (``exact_operands.rne_bf16``, pinned against torch's CPU cast by the CPU test),
forms the products and the sum in float64 (products of two bf16 values are exact there, and the sum's error is ~1e-16 of the
sum of magnitudes: nothing beside the bound) and applies the fp32 ``dscale`` in float64.

The element-wise bound on |kernel - emulation| is the standard accumulation bound of a sum of K = 9 cin exact products added in
fp32 in any order, |err| <= (K - 1) u sum|terms| to first order with u = 2^-24, written with K + 4 terms for the four further
fp32 roundings behind the sum (dscale, noise, bias, one activation constant) and doubled because the internal adds of the
matrix instruction are not documented to round to nearest:

    bound = 2 (9 cin + 4) 2^-24 dscale conv(|x_mod|, |W_b|)

With the fused tail the result is lrelu_0.2(y + nw noise + bias) sqrt(2): that map has slope sqrt(2) for a positive argument and
0.2 sqrt(2) for a negative one, so the bound on y carries over times sqrt(2), or times 0.2 sqrt(2) where the reference's
argument is negative by more than the bound (the kernel's is then negative too); the tail's own four roundings act on values
of magnitude at most |y| + |nw noise| + |bias| and add 4 * 2^-24 * sqrt(2) * (|y| + |nw noise| + |bias|).

Only torch is used here; nothing of the kernels, the package or the oracle is imported."""
import math

import torch
import torch.nn.functional as F

import exact_operands as E

U = 2.0 ** -24
SQRT2_F32 = float(torch.tensor(2.0 ** 0.5, dtype=torch.float32))
SLOPE_F32 = float(torch.tensor(0.2, dtype=torch.float32))


def rne(x32):
    """fp32 -> the fp32 value of its round-to-nearest-even bf16 image, written out on the bits."""
    return E.rne_bf16(x32.detach().cpu().float()).float()


def truncate(x32):
    return E.truncate_bf16(x32.detach().cpu().float()).float()


def conv64(x, w):
    """3x3 "same" convolution in float64 as one matrix product per sample (any device): x [B,Cin,H,W], w [Cout,Cin,3,3]."""
    b, cin, h, wd = x.shape
    cols = F.unfold(x.double(), 3, padding=1)                       # [B, Cin * 9, H * W]
    return (w.double().reshape(w.shape[0], cin * 9) @ cols).reshape(b, w.shape[0], h, wd)


def modulated(x, s):
    """fl32(s * x): the style product as the kernel forms it, one fp32 multiplication."""
    return x.float() * s.float().view(s.shape[0], s.shape[1], 1, 1)


def emulate(x, w, s, dscale, x_op=None, w_op=None):
    """(y, bound) in float64.  ``x_op`` / ``w_op``: the operands after rounding (default: the contract's)."""
    xm = rne(modulated(x, s)) if x_op is None else x_op
    wb = rne(w) if w_op is None else w_op
    dev = x.device
    xm, wb = xm.to(dev), wb.to(dev)
    d = dscale.double().to(dev).view(dscale.shape[0], dscale.shape[1], 1, 1)
    y = d * conv64(xm, wb)
    bound = 2.0 * (9 * x.shape[1] + 4) * U * d.abs() * conv64(xm.abs(), wb.abs())
    return y, bound


def tail64(y, noise, nw, bias):
    """The fused tail in float64 with the kernel's fp32 constants: lrelu_0.2(y + nw noise + bias) sqrt(2)."""
    v = y + float(nw) * noise.double().to(y.device) + bias.double().to(y.device).view(1, -1, 1, 1)
    return torch.maximum(v, v * SLOPE_F32) * SQRT2_F32


def tail_bound(y, bound, noise, nw, bias):
    nz, bs = float(nw) * noise.double().to(y.device), bias.double().to(y.device).view(1, -1, 1, 1)
    mag = y.abs() + nz.abs() + bs.abs()
    own = 4.0 * U * SQRT2_F32 * mag
    negative = (y + nz + bs) + bound + own <= 0      # the kernel's pre-activation is then negative as well: slope 0.2 sqrt(2)
    return torch.where(negative, SLOPE_F32 * SQRT2_F32, SQRT2_F32) * bound + own


def over_bound_share(got, y, bound):
    """Share of the elements with |got - y| > bound (a NaN counts as over)."""
    err = (got.double().to(y.device) - y).abs()
    return float((~(err <= bound)).double().mean()), float((err / bound.clamp_min(1e-300)).max())


def operands(b, cin, cout, h, w, seed=None):
    """randn operands of one layer: x, W [cout,cin,3,3], s [b,cin] around 1, a positive fp32 dscale of the layer's magnitude,
    noise [1,1,h,w], noise weight, bias."""
    gen = torch.Generator().manual_seed(b * 1000 + cin + cout + h if seed is None else seed)
    mk = lambda *sh: torch.randn(*sh, generator=gen)
    x, wt = mk(b, cin, h, w), mk(cout, cin, 3, 3)
    s = 1 + 0.3 * mk(b, cin)
    dscale = (0.5 + torch.rand(b, cout, generator=gen)) / math.sqrt(9 * cin)
    return dict(x=x, w=wt, s=s, dscale=dscale, noise=mk(1, 1, h, w), nw=0.3 * mk(1), bias=0.2 * mk(cout))


DEFECTS = ("x truncated", "W truncated", "x unrounded", "W unrounded", "x rounded before the style product")


def defective(name, L):
    """(x_op, w_op) of one of the five defects the rounding test has to see."""
    x, w, s = L["x"], L["w"], L["s"]
    xm = modulated(x, s)
    if name == "x truncated":
        return truncate(xm), rne(w)
    if name == "W truncated":
        return rne(xm), truncate(w)
    if name == "x unrounded":
        return xm, rne(w)
    if name == "W unrounded":
        return rne(xm), w.float()
    if name == "x rounded before the style product":
        return rne(modulated(rne(x), s)), rne(w)   # (the operand is a bf16 value either way: rounded twice)
    raise KeyError(name)
