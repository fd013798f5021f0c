"""Cases, float64 references and bounds for the generator head kernels of csrc/gen_small_ops.hip: ``sis_pixel_norm``,
``sis_equal_linear`` (four routes), ``sis_modulation_batch``, ``sis_demod_batch``, ``sis_truncate``, ``sis_modconv_prepack``,
``sis_modconv_demod``, ``sis_to_rgb`` (two routes) and ``sis_rgb_finish``.  Shared by test_gen_head_cases_cpu.py (on the fp32
restatement of gen_head_restatement.py), test_gen_head_gpu.py and test_gen_head_guard_bands_gpu.py (on the kernels).
torch on the CPU and numpy only; nothing of the package or the oracle is imported.

Every EqualLinear and ToRGB case names the kernel it MUST run (the GPU test asserts it through ``sis_last_kernel()``): a planner
change that moves a shape fails there instead of leaving a kernel untested.

Exact tier: no tolerance.  Operands are integers in [-r, r] (``exact_operands.integers`` in float32), every free scalar (scale,
lr_mul, psi, the demodulation scale bits) a power of two: every product and partial sum is an fp32 value in ANY association,
the fp32 matrix-core chain included, so the output must be ``exact_f32(ref)`` bit for bit.  The precondition is asserted from the
operands (``check_operands``) and from the reference (``check_reference``).  The two roundings of the activation (v * 0.2f, then
* 1.4142135f) follow an exact pre-activation and are restated in numpy float32 (``activate32``).

Bound tier, per element:   |got - ref64| <= K u32 A + B,   u32 = 2^-24
  A   the reference's expression with the absolute value of every operand:  |scale| sum|x||w| + |bias lr_mul| (times sqrt 2
      when activated);  |scale| sum|w||s||x| + |bias| + sum|skip||taps|;  |m| + |psi| (|w| + |m|);  sum over the blocks of |part|
      + |bias| + sum|skip||taps|.  pixel_norm and the demodulation scales: |ref64| (sums of non-negative terms: a relative error).
  B   the device's rsqrtf, taken as 2 ulp = 4 u32 |ref64| by the convention loss_cases.py uses for logf (the one number here
      that is a convention, not a measurement: the restatement's routine is numpy's, not the device's).  Zero elsewhere.
  K   4 x the largest figure of the numpy fp32 restatement (gen_head_restatement.py: the kernel's association) over every bound
      case of the kernel -- measured on the CPU (``python tests/test_gen_head_cases_cpu.py`` prints the table), NOT on the device:
        equal_linear_full_kernel<8>   K =  2.63   (0.655: el-9x512x513-randn)
        equal_linear_full_kernel<4>   K =  2.19   (0.546: el-9x256x513-randn)
        equal_linear_kernel           K =  7.21   (1.802: el-6x1x8-randn)
        head_gemm_kernel<0>           K = 15.11   (3.775: el-33x1088x257-randn)
        head_gemm_kernel<1>           K = 15.29   (3.821: mod-33x128-randn)
        head_gemm_kernel<2>           K = 33.77   (8.441: dem-33x192-randn)
        demod_kernel                  K = 14.99   (3.746: dem-32x192-randn)
        to_rgb_kernel<1>              K = 10.28   (2.570: rgb-1x9x3x17x19-noskip-randn)
        to_rgb_kernel<4>              K =  7.38   (1.845: rgb-2x33x2x18x18-kblur-randn)
        rgb_finish_kernel             K = 11.18   (2.794: fin-8x1x3x32x32-k4-randn)
        pixel_norm_kernel             K = 11.52   (2.879: pn-7x512-randn)
        truncate_kernel               K =  6.92   (1.728: tr-1x1x513-psi0.7-randn)
      (rounded up to two decimals.  The restatement's figures are taken with B = 0: its own 1 / sqrt counts into K, and the
      device's rsqrtf gets B on top.  u32 is the unit roundoff, half an ulp: a figure of 3 is an error of 1.5 ulp of A.)
  No element and no case is left out; besides the whole result the figure is taken on the last row and last column of every
  4 x 4 (one-wave kernels) or 32 x 128 (head_gemm) tile and on the last live pixel group, each held to K on its own.
"""
import functools
import struct
import zlib

import numpy as np
import torch

import exact_operands as X
from loss_cases import U32, need

EL8, EL4, ELG, HG0 = "equal_linear_full_kernel<8>", "equal_linear_full_kernel<4>", "equal_linear_kernel", "head_gemm_kernel<0>"
HG1, HG2, DEM, PN, TR = "head_gemm_kernel<1>", "head_gemm_kernel<2>", "demod_kernel", "pixel_norm_kernel", "truncate_kernel"
RGB4, RGB1, FIN = "to_rgb_kernel<4>", "to_rgb_kernel<1>", "rgb_finish_kernel"
K = {EL8: 2.63, EL4: 2.19, ELG: 7.21, HG0: 15.11, HG1: 15.29, HG2: 33.77, DEM: 14.99, RGB1: 10.28, RGB4: 7.38, FIN: 11.18, PN: 11.52,
     TR: 6.92}
TILE = {EL8: (4, 4), EL4: (4, 4), ELG: (4, 4), HG0: (32, 128), HG1: (32, 128), HG2: (32, 128), DEM: (4, 4)}
HEAD_TILE = 128            # sis_head_gemm_tile()
SQRT2_F32 = np.float32(1.4142135623730951)
SLOPE_F32 = np.float32(0.2)
B_RSQRT = 4 * U32          # 2 ulp of the device's rsqrtf, relative to |ref64|


def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def _randn(gen, *shape):
    return torch.randn(*shape, generator=gen)


# ------------------------------------------------------------------------------------------------------------ EqualLinear

COMBOS = [(bias, act, lr) for bias in (True, False) for act in (False, True) for lr in (1.0, 0.5)]
EL_SCALE = 2.0 ** -4       # exact tier


def _el_route(k):
    return EL8 if k == 512 else EL4 if k == 256 else ELG if k <= 1024 else HG0


def _el_shapes():
    """(batch, in, out, strided): ``strided`` None, or (latent index, misaligned base) of x = latent[:, i] in a [B, 3, D] tensor."""
    out = []
    for k in (512, 256):                                     # every residue of batch and out modulo 4, the row clamp past the batch
        out += [(b, k, o, None) for b, o in ((1, 4), (3, 6), (5, 7), (9, 513))]
    for k in (1, 63, 64, 65, 100, 1000, 1024):               # the general kernel: below / at / above a wave, the register row's end
        out += [(b, k, o, None) for b in (3, 6) for o in (5, 8)]
    out += [(b, 1088, o, None) for b in (32, 33) for o in (128, 130, 257)]   # 17 whole chunks: interior and edge tiles in one launch
    out += [(3, k, 5, None) for k in (1025, 1032, 1091)]     # chunk tails; rows that are 16-byte aligned (1032) and rows that are not
    for d, b, o in ((512, 5, 7), (100, 5, 7), (1088, 33, 130)):
        out += [(b, d, o, (i, False)) for i in (0, 2)]
    out += [(33, 1088, 130, (i, True)) for i in (0, 2)]      # the base one float into a buffer: no interior loads, the same bits
    return out


class ELShape:
    def __init__(self, batch, k, out, strided):
        self.batch, self.k, self.out, self.strided = batch, k, out, strided
        self.route = _el_route(k)
        self.id = f"el-{batch}x{k}x{out}" + ("" if strided is None else f"-lat{strided[0]}" + ("-misaligned" if strided[1] else ""))

    def __repr__(self):
        return self.id


EL_SHAPES = [ELShape(*s) for s in _el_shapes()]
EL_SHAPE = {s.id: s for s in EL_SHAPES}
EL_BOUND_COMBO = {s.id: COMBOS[i % len(COMBOS)] for i, s in enumerate(EL_SHAPES)}     # the bound tier's one combination per shape
N_LATENT = 3


@functools.lru_cache(maxsize=None)
def el_operands(shape_id, tier):
    """-> dict(x [B, k] (the rows the layer reads), latent ([B, 3, D] or None), w, bias, scale, r).  Left unchanged by every user."""
    s = EL_SHAPE[shape_id]
    gen = _gen(shape_id.replace("-misaligned", "") + tier)       # the misaligned twin has the aligned case's operands
    rows = (s.batch, N_LATENT, s.k) if s.strided else (s.batch, s.k)
    if tier == "exact":
        r = X.radius(s.k)
        X.check_operands(s.k, r, r, extra=2)
        xs, w, bias = (X.integers(sh, r, gen, dtype=torch.float32) for sh in (rows, (s.out, s.k), (s.out,)))
        scale = EL_SCALE
    else:
        r = None
        xs, w, bias = _randn(gen, *rows), _randn(gen, s.out, s.k), _randn(gen, s.out)
        scale = 1.0 / s.k ** 0.5
    latent = xs if s.strided else None
    x = xs[:, s.strided[0]] if s.strided else xs
    return dict(x=x, latent=latent, w=w, bias=bias, scale=scale, r=r)


def activate64(v):
    return torch.where(v > 0, v, 0.2 * v) * 2.0 ** 0.5


def el_ref(x, w, bias, scale, lr_mul, act):
    """-> (ref64 [B, out], pre-activation, A)."""
    x, w = x.double(), w.double()
    pre = scale * (x @ w.t())
    A = abs(scale) * (x.abs() @ w.abs().t())
    if bias is not None:
        pre = pre + bias.double() * lr_mul
        A = A + (bias.double() * lr_mul).abs()
    return (activate64(pre), pre, A * 2.0 ** 0.5) if act else (pre, pre, A)


def activate32(pre32):
    """The activation's two fp32 roundings on an exact pre-activation: (v > 0 ? v : v * 0.2f) * 1.4142135f."""
    v = pre32.numpy()
    assert v.dtype == np.float32
    return torch.from_numpy((np.where(v > 0, v, v * SLOPE_F32) * SQRT2_F32).astype(np.float32))


def el_expected(pre, act, unit=EL_SCALE * 0.5):
    """What the exact tier's output must be, bit for bit."""
    e = X.exact_f32(pre, unit)
    return activate32(e) if act else e


def tile_regions(shape, tile):
    """name -> boolean mask of a [rows, cols] result: everything, the last row and the last column of every tile."""
    rows, cols = shape
    r, c = np.arange(rows)[:, None], np.arange(cols)[None, :]
    full = np.ones((rows, cols), dtype=bool)
    return dict(all=full, tile_last_row=full & ((r % tile[0] == tile[0] - 1) | (r == rows - 1)),
                tile_last_col=full & ((c % tile[1] == tile[1] - 1) | (c == cols - 1)))


def figures(got, ref, A, B=0.0, regions=None):
    """name -> the K this result needs on that region (``loss_cases.need``: inf for a non-finite error)."""
    ref, A = np.asarray(ref, dtype=np.float64), np.asarray(A, dtype=np.float64)
    err = np.asarray(got, dtype=np.float64).reshape(ref.shape) - ref
    Bb = np.broadcast_to(np.asarray(B, dtype=np.float64), ref.shape)
    if regions is None:
        regions = dict(all=np.ones(ref.shape, dtype=bool))
    return {name: need(err[..., m], U32 * A[..., m], Bb[..., m]) for name, m in regions.items() if m.any()}


# ------------------------------------------------------------------------------------------------------------ modulation / demodulation

MOD_SCALE = 2.0 ** -3
DEM_SCALE = 2.0 ** -5
# (cin, cout, latent index, demodulation row: None = ToRGB (no row), else the row's ``demodulate``)
LAYERS = [(24, 136, 2, 1), (128, 128, 0, 1), (136, 3, 3, None), (260, 40, 1, 1), (40, 72, 4, 0), (192, 130, 2, 1)]
MOD_N_LATENT = 5
MOD_CASES = [(b, dim) for dim in (128, 192) for b in (3, 32, 33)]     # two and three chunks of K; below, at and past one row tile


def f32_bits(v):
    return struct.unpack("<i", struct.pack("<f", v))[0]


@functools.lru_cache(maxsize=None)
def mod_operands(batch, dim, tier):
    """-> dict(latent [B, 5, dim], layers: per layer dict(mw [cin, dim], mb [cin], weight [1, cout, cin, 3, 3], s_in [B, cin]))
    ``s_in`` is what the demodulation launches are fed: integers in the exact tier, so their sum is exact."""
    gen = _gen(f"mod-{batch}x{dim}-{tier}")
    layers = []
    if tier == "exact":
        r = X.radius(dim)
        X.check_operands(dim, r, r, extra=2)
        latent = X.integers((batch, MOD_N_LATENT, dim), r, gen, dtype=torch.float32)
    else:
        latent = _randn(gen, batch, MOD_N_LATENT, dim)
    for cin, cout, _, _ in LAYERS:
        if tier == "exact":
            mw, mb = X.integers((cin, dim), r, gen, dtype=torch.float32), X.integers((cin,), r, gen, dtype=torch.float32)
            weight, s_in = X.integers((1, cout, cin, 3, 3), 3, gen, dtype=torch.float32), X.integers((batch, cin), 3, gen, dtype=torch.float32)
            X.check_operands(cin, 3 * 3, 9 * 3 * 3)       # sum over cin of s^2 (sum of 9 w^2), in units of scale^2
        else:
            mw, mb = _randn(gen, cin, dim), 1 + 0.1 * _randn(gen, cin)
            weight, s_in = _randn(gen, 1, cout, cin, 3, 3), 1 + 0.5 * _randn(gen, batch, cin)
        layers.append(dict(mw=mw, mb=mb, weight=weight, s_in=s_in))
    return dict(latent=latent, layers=layers)


def mod_scale(dim, tier):
    return MOD_SCALE if tier == "exact" else 1.0 / dim ** 0.5


def dem_scale(cin, tier):
    return DEM_SCALE if tier == "exact" else 1.0 / (cin * 9) ** 0.5


def wsq_ref(weight):
    return weight[0].double().pow(2).sum((2, 3))


def demod_ref(s, wsq, scale):
    """scale * rsqrt(scale^2 sum s^2 wsq + 1e-8) in float64, the 1e-8 being the float32 constant of the operator (as in
    ``pn_ref``; it differs from the double 1e-8 by 6e-17, which counts only where the sum vanishes)."""
    return scale * torch.rsqrt(scale * scale * (s.double().pow(2) @ wsq.double().t()) + float(np.float32(1e-8)))


def layout(batch):
    """Offsets of the flat style / demodulation buffers and the block starts: per layer (s_off, d_off or None, mod block, dem block),
    then the totals (s floats, d floats, modulation blocks, demodulation blocks)."""
    rows, s_off, d_off, mb, db = [], 0, 0, 0, 0
    for cin, cout, _, dem in LAYERS:
        rows.append((s_off, d_off if dem is not None else None, mb, db))
        s_off += batch * cin
        mb += (cin + HEAD_TILE - 1) // HEAD_TILE
        if dem is not None:
            d_off += batch * cout
            db += (cout + HEAD_TILE - 1) // HEAD_TILE
    return rows, (s_off, d_off, mb, db)


def tables(batch, ptrs, tier):
    """The two int64 tables as Generator._modulate_all lays them out, from device addresses ``ptrs`` = per layer (mw, mb, wsq)."""
    rows, _ = layout(batch)
    mod, dem = [], []
    for (cin, cout, lat, d), (s_off, d_off, mb, db), (p_mw, p_mb, p_wsq) in zip(LAYERS, rows, ptrs):
        mod.append([p_mw, p_mb, s_off, lat, cin, mb, 0, 0])
        if d is not None:
            dem.append([p_wsq, f32_bits(dem_scale(cin, tier)), s_off, d_off, cout, db, cin, d])
    return torch.tensor(mod, dtype=torch.int64), torch.tensor(dem, dtype=torch.int64)


# ------------------------------------------------------------------------------------------------------------ ToRGB / rgb_finish

RGB_SCALE = 2.0 ** -3
RGB_R = 7                  # cin r^3 = 128 * 343 < 2^16
TAP_KINDS = (2, 3, 4, 6, "blur")


def upsample_pad(k, factor=2):
    """``Upsample``'s padding: p = k - factor -> ((p + 1) // 2 + factor - 1, p // 2)."""
    p = k - factor
    return ((p + 1) // 2 + factor - 1, p // 2)


@functools.lru_cache(maxsize=None)
def taps_of(kind, tier):
    """k x k taps: the project's own [1,3,3,1] (x) [1,3,3,1] / 64 * 4 ("blur"), else random ones that are neither symmetric under a
    flip or a transposition nor separable -- integers in the exact tier."""
    if kind == "blur":
        k1 = torch.tensor([1.0, 3.0, 3.0, 1.0])
        return (k1[None, :] * k1[:, None] / 64 * 4).contiguous()
    gen = _gen(f"taps-{kind}-{tier}")
    while True:
        t = X.integers((kind, kind), 4, gen, dtype=torch.float32) if tier == "exact" else _randn(gen, kind, kind)
        ok = not (torch.equal(t, t.flip(0)) or torch.equal(t, t.flip(1)) or torch.equal(t, t.t()) or torch.equal(t, t.flip(0, 1)))
        if ok and int(torch.linalg.matrix_rank(t.double())) > 1 and bool((t != 0).all()):
            return t


def upfirdn_up2_ref(skip, taps, pad):
    """up = 2 ``upfirdn2d`` in float64, written out: zero-stuff, pad, correlate with the flipped kernel.  skip [B, C, sh, sw]."""
    skip, taps = skip.double(), taps.double()
    b, c, sh, sw = skip.shape
    kh, kw = taps.shape
    z = torch.zeros(b, c, 2 * sh, 2 * sw, dtype=torch.float64)
    z[:, :, ::2, ::2] = skip
    p = torch.zeros(b, c, 2 * sh + pad[0] + pad[1], 2 * sw + pad[0] + pad[1], dtype=torch.float64)
    p[:, :, pad[0]:pad[0] + 2 * sh, pad[0]:pad[0] + 2 * sw] = z
    f = taps.flip(0, 1)
    oh, ow = p.shape[2] - kh + 1, p.shape[3] - kw + 1
    out = torch.zeros(b, c, oh, ow, dtype=torch.float64)
    for fy in range(kh):
        for fx in range(kw):
            out += f[fy, fx] * p[:, :, fy:fy + oh, fx:fx + ow]
    return out


def _skip_terms(skip, taps):
    """-> (the upsampled skip image, the same with |skip| and |taps|)."""
    pad = upsample_pad(taps.shape[0])
    return upfirdn_up2_ref(skip, taps, pad), upfirdn_up2_ref(skip.abs(), taps.abs(), pad)


# (b, cin, cout, h, w, misaligned x), the route
RGB_SHAPES = [
    ((2, 5, 3, 2, 2, False), RGB1),          # four pixels
    ((1, 37, 1, 6, 10, False), RGB1),        # one colour, a non-square map below one group
    ((2, 16, 4, 4, 4, False), RGB1),         # four colours
    ((1, 9, 3, 17, 19, False), RGB1),        # an odd map (no skip): several groups, the last one partial
    ((1, 32, 3, 16, 16, True), RGB1),        # x one float into a buffer: the misaligned fallback
    ((2, 32, 3, 16, 16, False), RGB4),       # exactly one group
    ((1, 100, 3, 10, 26, False), RGB4),      # w % 4 = 2: a float4 straddles rows; the second group is partial
    ((2, 33, 2, 18, 18, False), RGB4),       # the channel-trip clamp (33 = 32 + 1)
    ((1, 128, 3, 32, 8, False), RGB4),
    ((1, 128, 3, 8, 32, False), RGB4),
]


class RGBCase:
    def __init__(self, dims, route, kind):
        self.b, self.cin, self.cout, self.h, self.w, self.misaligned = dims
        self.route, self.kind = route, kind
        self.shape_id = f"rgb-{self.b}x{self.cin}x{self.cout}x{self.h}x{self.w}" + ("-misaligned" if self.misaligned else "")
        self.id = self.shape_id + ("-noskip" if kind is None else f"-k{kind}")
        self.vec = 4 if route == RGB4 else 1

    def __repr__(self):
        return self.id


RGB_CASES = [RGBCase(d, r, kind) for d, r in RGB_SHAPES for kind in (None,) + TAP_KINDS
             if kind is None or (d[3] % 2 == 0 and d[4] % 2 == 0)]
RGB_CASE = {c.id: c for c in RGB_CASES}


@functools.lru_cache(maxsize=None)
def rgb_operands(shape_id, tier):
    """-> dict(x, w [1, cout, cin, 1, 1], s [B, cin], bias [1, cout, 1, 1], skip [B, cout, h/2, w/2] or None, scale)."""
    c = next(c for c in RGB_CASES if c.shape_id == shape_id)
    gen = _gen(shape_id + tier)
    shapes = ((c.b, c.cin, c.h, c.w), (1, c.cout, c.cin, 1, 1), (c.b, c.cin), (1, c.cout, 1, 1), (c.b, c.cout, c.h // 2, c.w // 2))
    if tier == "exact":
        X.check_operands(c.cin, RGB_R * RGB_R, RGB_R, extra=2)
        x, w, s, bias, skip = (X.integers(sh, RGB_R, gen, dtype=torch.float32) for sh in shapes)
        scale = RGB_SCALE
    else:
        x, w, s, bias, skip = (_randn(gen, *sh) for sh in shapes)
        scale = 1.0 / c.cin ** 0.5
    if c.h % 2 or c.w % 2:
        skip = None
    return dict(x=x, w=w, s=s, bias=bias, skip=skip, scale=scale)


def rgb_ref(op, taps):
    """-> (ref64 [B, cout, h, w], A).  ``taps`` None: no skip."""
    x, w, s = op["x"].double(), op["w"].double()[0, :, :, 0, 0], op["s"].double()
    ref = op["scale"] * torch.einsum("ci,bi,bihw->bchw", w, s, x) + op["bias"].double()
    A = abs(op["scale"]) * torch.einsum("ci,bi,bihw->bchw", w.abs(), s.abs(), x.abs()) + op["bias"].double().abs()
    if taps is not None:
        u, ua = _skip_terms(op["skip"], taps)
        ref, A = ref + u, A + ua
    return ref, A


def pixel_regions(hw, vec_pixels):
    """name -> mask over the h * w pixels: everything and the last live pixel group (``vec_pixels`` pixels per group)."""
    p = np.arange(hw)
    return dict(all=np.ones(hw, dtype=bool), last_group=p >= ((hw - 1) // vec_pixels) * vec_pixels)


def rgb_unit(kind):
    """The unit every exact-tier ToRGB value is a multiple of: the scale, over 16 with the blur's sixteenths."""
    return RGB_SCALE / 16 if kind == "blur" else RGB_SCALE


FIN_SHAPES = [(1, 2, 3, 2, 2), (2, 1, 1, 16, 16), (3, 2, 4, 8, 40), (8, 1, 3, 32, 32),
              (3, 1, 3, 36, 36)]         # 1296 pixels: the second group of 1024 is partial
FIN_KINDS = (None, 4, 6)


@functools.lru_cache(maxsize=None)
def fin_operands(dims, tier):
    """-> dict(part [blocks, B, cout, h, w], bias [1, cout, 1, 1], skip [B, cout, h/2, w/2])."""
    blocks, b, cout, h, w = dims
    gen = _gen(f"fin-{dims}-{tier}")
    shapes = ((blocks, b, cout, h, w), (1, cout, 1, 1), (b, cout, h // 2, w // 2))
    if tier == "exact":
        part, bias, skip = (X.integers(sh, 15, gen, dtype=torch.float32) for sh in shapes)
    else:
        part, bias, skip = (_randn(gen, *sh) for sh in shapes)
    return dict(part=part, bias=bias, skip=skip)


def fin_id(dims, kind):
    return "fin-" + "x".join(str(d) for d in dims) + ("-noskip" if kind is None else f"-k{kind}")


def fin_ref(op, taps):
    ref = op["part"].double().sum(0) + op["bias"].double()
    A = op["part"].double().abs().sum(0) + op["bias"].double().abs()
    if taps is not None:
        u, ua = _skip_terms(op["skip"], taps)
        ref, A = ref + u, A + ua
    return ref, A


# ------------------------------------------------------------------------------------------------------------ pixel_norm, truncate, prepack

PN_SHAPES = [(1, 1), (3, 40), (5, 64), (4, 65), (7, 512), (2, 1000)]
PN_FAMILIES = ("randn", "offset", "zero_row", "tiny")


@functools.lru_cache(maxsize=None)
def pn_input(shape, family):
    gen = _gen(f"pn-{shape}-{family}")
    x = _randn(gen, *shape)
    if family == "offset":          # |x| ~ 1e3
        x = x + 1e3
    if family == "zero_row":        # the result of an all-zero row is exactly 0
        x[shape[0] // 2] = 0.0
    if family == "tiny":            # the 1e-8 dominates the mean square
        x = 1e-6 * (1 + 0.5 * torch.rand(*shape, generator=gen))
    return x


def pn_ref(x):
    """model.py's PixelNorm in float64, with the device's float32(1e-8)."""
    x = x.double()
    return x * torch.rsqrt(x.pow(2).mean(dim=1, keepdim=True) + float(np.float32(1e-8)))


def pn_id(shape, family):
    return f"pn-{shape[0]}x{shape[1]}-{family}"


TR_SHAPES = [(3, 5, 40), (1, 1, 513)]
TR_PSI = (0.0, 0.7, 1.0)
TR_PSI_EXACT = 0.5


@functools.lru_cache(maxsize=None)
def tr_operands(shape, tier):
    """-> (w [..., dim], mean [1, dim]); the exact tier's are even integers, so the halving is exact."""
    gen = _gen(f"tr-{shape}-{tier}")
    if tier == "exact":
        return 2 * X.integers(shape, 15, gen, dtype=torch.float32), 2 * X.integers((1, shape[-1]), 15, gen, dtype=torch.float32)
    return _randn(gen, *shape), _randn(gen, 1, shape[-1])


def tr_ref(w, mean, psi):
    w, m = w.double(), mean.double()
    return m + psi * (w - m), m.abs() + abs(psi) * (w.abs() + m.abs())


def tr_id(shape, psi):
    return "tr-" + "x".join(str(d) for d in shape) + f"-psi{psi}"


PREPACK_SHAPES = [(3, 5, 1), (130, 7, 3), (64, 64, 3)]


@functools.lru_cache(maxsize=None)
def prepack_weight(dims):
    cout, cin, k = dims
    X.check_operands(k * k, 15, 15)
    return X.integers((1, cout, cin, k, k), 15, _gen(f"prepack-{dims}"), dtype=torch.float32)


def prepack_ref(weight):
    """-> (wpk [cin, k * k, cout]: the permutation, wsq [cout, cin]: the exact sum)."""
    _, cout, cin, k, _ = weight.shape
    return weight[0].permute(1, 2, 3, 0).reshape(cin, k * k, cout).contiguous(), X.exact_f32(wsq_ref(weight))


# ------------------------------------------------------------------------------------------------------------ checks
# One function per operation: the result of a case (the restatement's on the CPU, the kernel's on the device) against its
# reference.  -> Result: the figures of a bound-tier case per region, and the failures (a bitwise mismatch of the exact tier,
# localised by ``exact_operands.mismatch_report``; a region whose figure exceeds K; a non-finite value).

class Result:
    def __init__(self, kernel, case_id, figs=None, bad=None):
        self.kernel, self.id, self.figs, self.bad = kernel, case_id, figs or {}, [b for b in (bad or []) if b]
        for name, v in self.figs.items():
            if not v <= K[kernel]:
                self.bad.append(f"{case_id}: {name} needs K = {v:.4g} (K of {kernel} = {K[kernel]})")

    @property
    def worst(self):
        return max(self.figs.values(), default=0.0)


class Report:
    """Collects the results of a test and fails once, with every failure."""

    def __init__(self):
        self.results = []

    def add(self, result):
        self.results.append(result)
        return result

    def finish(self):
        print("; ".join(f"{r.id} " + " ".join(f"{k} {v:.3g}" for k, v in r.figs.items()) for r in self.results if r.figs))
        bad = [b for r in self.results for b in r.bad]
        assert not bad, "\n".join(bad)


def _t(a):
    return a.detach().cpu() if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))


def el_id(shape_id, tier, combo):
    if tier == "randn":
        return f"{shape_id}-randn"
    return f"{shape_id}-" + ("bias" if combo[0] else "nobias") + ("-act" if combo[1] else "") + f"-lr{combo[2]}"


def el_check(shape_id, tier, combo, got, x=None):
    """``x``: other rows than the case's (a simulated defect's)."""
    s, op = EL_SHAPE[shape_id], el_operands(shape_id, tier)
    has_bias, act, lr_mul = combo
    scale = el_scale(shape_id, tier, combo)
    ref, pre, A = el_ref(op["x"] if x is None else x, op["w"], op["bias"] if has_bias else None, scale, lr_mul, act)
    cid = el_id(shape_id, tier, combo)
    if tier == "exact":
        return Result(s.route, cid, bad=[X.mismatch_report(_t(got), el_expected(pre, act), cid, TILE[s.route])])
    return Result(s.route, cid, figures(_t(got).numpy(), ref.numpy(), A.numpy(), regions=tile_regions(tuple(ref.shape), TILE[s.route])))


def el_scale(shape_id, tier, combo):
    """model.py's scale = lr_mul / sqrt(in) in the bound tier; the exact tier's power of two as it is."""
    return el_operands(shape_id, tier)["scale"] * (combo[2] if tier == "randn" else 1.0)


def mod_check(batch, dim, tier, li, got):
    """Layer ``li``'s style vectors [B, cin] of ``modulation_batch``."""
    op, (cin, cout, lat, _) = mod_operands(batch, dim, tier), LAYERS[li]
    L = op["layers"][li]
    ref, pre, A = el_ref(op["latent"][:, lat], L["mw"], L["mb"], mod_scale(dim, tier), 1.0, False)
    cid = f"mod-{batch}x{dim}-{tier}"
    if tier == "exact":
        return Result(HG1, cid, bad=[X.mismatch_report(_t(got), X.exact_f32(pre, MOD_SCALE), f"{cid} layer {li}", TILE[HG1])])
    return Result(HG1, cid, figures(_t(got).numpy(), ref.numpy(), A.numpy(), regions=tile_regions(tuple(ref.shape), TILE[HG1])))


def dem_check(batch, dim, tier, li, kernel, got, wsq, device_rsqrt=True):
    """Layer ``li``'s demodulation scales [B, cout] from ``s_in`` and the fp32 ``wsq`` the kernel was handed.  A row without
    demodulation must hold the scale itself, bit for bit."""
    op, (cin, cout, _, dem) = mod_operands(batch, dim, tier), LAYERS[li]
    scale = dem_scale(cin, tier)
    cid = f"dem-{batch}x{dim}-{tier}"
    if not dem:
        want = torch.full((batch, cout), float(np.float32(scale)), dtype=torch.float32)
        return Result(kernel, cid, bad=[X.mismatch_report(_t(got), want, f"{cid} layer {li} (no demodulation)", TILE[kernel])])
    ref = demod_ref(op["layers"][li]["s_in"], _t(wsq), float(np.float32(scale))).numpy()
    return Result(kernel, cid, figures(_t(got).numpy(), ref, np.abs(ref), B_RSQRT * np.abs(ref) * device_rsqrt, tile_regions(ref.shape, TILE[kernel])))


def rgb_check(case, tier, got, taps=None):
    """``taps``: the taps the reference uses (default: the case's own)."""
    op = rgb_operands(case.shape_id, tier)
    if taps is None and case.kind is not None:
        taps = taps_of(case.kind, tier)
    ref, A = rgb_ref(op, taps if case.kind is not None else None)
    cid = f"{case.id}-{tier}"
    hw = case.h * case.w
    if tier == "exact":
        return Result(case.route, cid, bad=[X.mismatch_report(_t(got), X.exact_f32(ref, rgb_unit(case.kind)), cid)])
    regions = {k: m.reshape(case.h, case.w) for k, m in pixel_regions(hw, 64 * case.vec).items()}
    return Result(case.route, cid, figures(_t(got).numpy(), ref.numpy(), A.numpy(), regions=regions))


def fin_check(dims, kind, tier, got):
    op = fin_operands(dims, tier)
    ref, A = fin_ref(op, None if kind is None else taps_of(kind, tier))
    cid = f"{fin_id(dims, kind)}-{tier}"
    if tier == "exact":
        return Result(FIN, cid, bad=[X.mismatch_report(_t(got), X.exact_f32(ref), cid)])
    regions = {k: m.reshape(dims[3], dims[4]) for k, m in pixel_regions(dims[3] * dims[4], 1024).items()}
    return Result(FIN, cid, figures(_t(got).numpy(), ref.numpy(), A.numpy(), regions=regions))


def pn_check(shape, family, got, device_rsqrt=True):
    x = pn_input(shape, family)
    ref = pn_ref(x).numpy()
    cid, got = pn_id(shape, family), _t(got)
    bad = []
    if family == "zero_row" and not bool((got[shape[0] // 2] == 0).all()):
        bad.append(f"{cid}: the all-zero row does not come back exactly 0")
    return Result(PN, cid, figures(got.numpy(), ref, np.abs(ref), B_RSQRT * np.abs(ref) * device_rsqrt, tile_regions(ref.shape, (4, 64))), bad)


def tr_check(shape, psi, tier, got):
    w, mean = tr_operands(shape, tier)
    ref, A = tr_ref(w, mean, psi)
    cid = f"{tr_id(shape, psi)}-{tier}"
    if tier == "exact":
        return Result(TR, cid, bad=[X.mismatch_report(_t(got), X.exact_f32(ref), cid)])
    return Result(TR, cid, figures(_t(got).numpy(), ref.numpy(), A.numpy()))
