"""Exactly summable operands for the bf16 matrix-core kernels (csrc/gemm_bf16.hip, gemm256_bf16.hip, conv_bf16.hip,
conv_bf16_wgrad.hip, stem_conv.hip, column_sum.hip): tests without a tolerance.

bf16 holds every integer of magnitude <= 256, the matrix cores multiply bf16 operands exactly and add in fp32.  With integer
operands in [-r_a, r_a] and [-r_b, r_b] (optionally times one common power of two) and K * r_a * r_b < 2^24, every partial sum
of a contraction of length K is an integer below 2^24 and therefore exact in fp32 -- in ANY association, split-K slab order or
tile plan.  So an fp32 result must be bitwise the exact result and a bf16 result bitwise its round-to-nearest-even image; one
differing element is a defect, no rounding can excuse it.  References are computed in float64 on the CPU (53 bits: exact too).

The fp32 matrix-core convolutions (modconv_wino.hip through sis_conv3x3, conv_wgrad_wino.hip, conv1x1_f32.hip,
conv1x1_wgrad_f32.hip) follow the same rule with fp32 operands; the Winograd radii and the wide operand pairs are at the end.

Only torch on the CPU is used here; nothing of the kernels, the package or the oracle is imported."""
import torch
import torch.nn.functional as F

EXACT_F32 = 2 ** 24      # integers of magnitude below this are fp32 values, and so are their sums while they stay below it


def radius(k, cap=15):
    """Largest r <= cap with k * r * r < 2^23: a contraction of length k over operands in [-r, r] stays below 2^23, which
    leaves a factor of 2 for a bias or residual term."""
    r = cap
    while r > 1 and k * r * r >= 2 ** 23:
        r -= 1
    assert k * r * r < 2 ** 23, (k, r)
    return r


def integers(shape, r, gen, shift=0, dtype=torch.bfloat16):
    """Uniform integers in [-r, r] times 2^-shift, in ``dtype``; the cast must lose nothing."""
    exact = torch.randint(-r, r + 1, tuple(shape), generator=gen).double() * 2.0 ** -shift
    out = exact.to(dtype)
    assert torch.equal(out.double(), exact), f"integers in [-{r}, {r}] * 2^-{shift} are not all {dtype} values"
    return out


def check_operands(k, r_a, r_b, extra=1):
    """The precondition on the operands: every partial sum of the contraction (times ``extra``, a later exact factor) is an
    integer multiple of the common unit below 2^24."""
    assert k * r_a * r_b * extra < EXACT_F32, (k, r_a, r_b, extra)


def check_reference(ref, unit=1.0):
    """The precondition on the float64 reference itself: integers (multiples of ``unit``) below 2^24, hence fp32 values."""
    assert ref.dtype == torch.float64
    scaled = ref / unit
    assert torch.equal(scaled, scaled.round()), "the reference is not a multiple of its unit"
    assert float(scaled.abs().max()) < EXACT_F32, float(scaled.abs().max())
    assert torch.equal(ref.float().double(), ref)
    return ref


def exact_f32(ref, unit=1.0):
    """What an fp32 output must be, bit for bit."""
    return check_reference(ref, unit).float()


def expected_bf16(ref, unit=1.0):
    """What a bf16 output must be, bit for bit: the RNE image of the exact result (torch's CPU cast; test_exact_operands_cpu.py
    checks that cast against ``rne_bf16`` below)."""
    return check_reference(ref, unit).float().bfloat16()


def _bits(x32):
    assert x32.dtype == torch.float32
    return x32.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF


def _from_upper_bits(upper):
    word = (upper & 0xFFFF) << 16
    word = torch.where(word >= 2 ** 31, word - 2 ** 32, word)
    return word.to(torch.int32).view(torch.float32).bfloat16()    # (the low 16 bits are zero: this cast is exact)


def rne_bf16(x32):
    """fp32 -> bf16 by round-to-nearest-even, written out on the bits (finite values): add 0x7FFF plus the bit that will become
    the last one, then drop the low 16 bits."""
    u = _bits(x32)
    return _from_upper_bits((u + 0x7FFF + ((u >> 16) & 1)) >> 16)


def truncate_bf16(x32):
    """fp32 -> bf16 toward zero (a defect: simulated by the CPU test)."""
    return _from_upper_bits(_bits(x32) >> 16)


def half_away_bf16(x32):
    """fp32 -> bf16, ties away from zero (a defect: simulated by the CPU test)."""
    return _from_upper_bits((_bits(x32) + 0x8000) >> 16)


def tie_share(ref):
    """Fraction of the reference values that lie exactly half way between two bf16 values."""
    return float(((_bits(check_reference(ref.double()).float()) & 0xFFFF) == 0x8000).double().mean())


def inexact_share(ref):
    """Fraction of the reference values that are no bf16 values, i.e. that the output conversion has to round."""
    return float(((_bits(check_reference(ref.double()).float()) & 0xFFFF) != 0).double().mean())


MIN_INEXACT_SHARE, MIN_TIE_SHARE = 0.25, 0.05


def check_rounding_is_exercised(ref, what):
    """Condition on every bf16-output case, from the reference alone: the rounding path is exercised, ties included."""
    inexact, tie = inexact_share(ref), tie_share(ref)
    assert inexact >= MIN_INEXACT_SHARE and tie >= MIN_TIE_SHARE, f"{what}: inexact share {inexact:.3f}, tie share {tie:.3f}"
    return inexact, tie


def old_rule_accepts(got, ref, tol=1e-2):
    """The bound of test_gemm_bf16_gpu.py / test_conv_bf16_gpu.py: max|err| <= tol * max|ref|."""
    return float((got.double() - ref.double()).abs().max()) <= tol * float(ref.double().abs().max())


def mismatch_report(got, want, what, tile=None):
    """None when ``got`` equals ``want``; else a text that localises the mismatch: count, first 8 indices with both values,
    bounding box of the mismatching indices and, with ``tile`` = (rows, cols) of the last two axes (or one int for the last
    axis), that box modulo the tile -- an edge or tile bug shows there without another run.  The comparison is ``torch.equal``:
    value for value, a zero of either sign being one value."""
    got = got.detach().cpu()
    if got.dtype != want.dtype or got.shape != want.shape:
        return f"{what}: got {got.dtype} {tuple(got.shape)}, want {want.dtype} {tuple(want.shape)}"
    if torch.equal(got, want):
        return None
    bad = (got != want) | (got.isnan() != want.isnan())
    idx = bad.nonzero()
    lines = [f"{what}: {idx.shape[0]} of {want.numel()} elements differ"]
    for i in idx[:8]:
        at = tuple(int(v) for v in i)
        lines.append(f"  at {at}: got {float(got[at])!r}, want {float(want[at])!r}")
    lo, hi = idx.min(0).values.tolist(), idx.max(0).values.tolist()
    lines.append("  bounding box: " + " x ".join(f"[{a}, {b}]" for a, b in zip(lo, hi)) + f" of shape {tuple(want.shape)}")
    if tile is not None:
        tiles = (tile,) if isinstance(tile, int) else tuple(tile)
        mod = idx[:, idx.shape[1] - len(tiles):] % torch.tensor(tiles)
        lines.append(f"  modulo the tile {tiles}: " + " x ".join(f"[{a}, {b}]" for a, b in
                                                                 zip(mod.min(0).values.tolist(), mod.max(0).values.tolist())))
    return "\n".join(lines)


def assert_bitwise(got, want, what, tile=None):
    report = mismatch_report(got, want, what, tile)
    assert report is None, report


# ---- references: float64 on the CPU


def gemm_ref(a, b, layout):
    """layout "NT": a [m,k] b [n,k];  "NN": a [m,k] b [k,n];  "TN": a [k,m] b [k,n]  ->  [m,n] float64."""
    a, b = a.double(), b.double()
    return {"NT": lambda: a @ b.t(), "NN": lambda: a @ b, "TN": lambda: a.t() @ b}[layout]()


def conv_ref(x, w, bias=None, stride=1, dilation=1):
    """F.conv2d with padding dilation * (k // 2) in float64."""
    return F.conv2d(x.double(), w.double(), None if bias is None else bias.double(), stride=stride,
                    padding=dilation * (w.shape[2] // 2), dilation=dilation)


def conv_grads_ref(x, w, gy, stride=1, dilation=1):
    """(dL/dx, dL/dw) of ``conv_ref`` by autograd in float64."""
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    F.conv2d(xr, wr, stride=stride, padding=dilation * (w.shape[2] // 2), dilation=dilation).backward(gy.double())
    return xr.grad, wr.grad


def pointwise_wgrad_ref(x, gy):
    """dW [Cout, Cin] of a 1x1 convolution: the contraction over images and pixels, float64."""
    return torch.einsum("bop,bip->oi", gy.double().flatten(2), x.double().flatten(2))


# ---- fp32 matrix-core convolutions (csrc/modconv_wino.hip through sis_conv3x3, conv_wgrad_wino.hip, conv1x1_f32.hip,
# conv1x1_wgrad_f32.hip): v_mfma_f32_32x32x2_f32 is a true fp32 fma, so the rule above holds with fp32 operands too -- and the
# Winograd F(2x2,3x3) transforms keep it: G has only 1/2 entries, B^T and A^T only add, so with integer operands every
# intermediate is a multiple of 1/4 and exact while it stays below 2^24 quarter units.  The pointwise kernels use ``radius`` /
# ``check_operands`` with k = cin, cout or batch * pixels.


def _largest_radius(factor, cap):
    r = cap
    while r > 1 and factor * r * r >= EXACT_F32:
        r -= 1
    assert factor * r * r < EXACT_F32, (factor, r)
    return r


def winograd_radius(cin, cap=15):
    """Largest r <= cap with 324 * cin * r * r < 2^24, for image and filter integers in [-r, r] of a Winograd F(2x2,3x3) forward
    (or, with cin = the layer's cout, data gradient).  U = G g G^T: a row of G sums to at most 3/2 in magnitude, so |U| <= 9r/4,
    a multiple of 1/4.  V = B^T d B: a row of B^T has two entries +-1, so |V| <= 4r, an integer.  M = sum over cin of U * V:
    |M| <= 9 * cin * r^2, i.e. 36 * cin * r^2 quarter units.  The output transform A^T M A adds up to 3 x 3 = 9 values of M:
    every partial sum stays below 9 * 36 * cin * r^2 = 324 * cin * r^2 quarter units.  Below 2^24 all of them are fp32 values, in
    any channel order or K split."""
    return _largest_radius(324 * cin, cap)


def check_winograd_operands(cin, r_x, r_w):
    assert 324 * cin * r_x * r_w < EXACT_F32, (cin, r_x, r_w)


def winograd_wgrad_radius(tiles, cap=15):
    """Largest r <= cap with 576 * tiles * r * r < 2^24, for image and gradient integers in [-r, r] of the Winograd-domain weight
    gradient over ``tiles`` = batch * H/2 * W/2 tiles of the launch (a dilated layer: of its space-to-batch shape).
    E = A dY A^T adds up to 4 pixels: |E| <= 4r; V = B^T d B: |V| <= 4r; both integers.  S = sum over tiles of E * V:
    |S| <= 16 * tiles * r^2, an integer, in any tile order or slice plan.  dW = G^T S G adds up to 9 values of S with factors
    1, 1/2, 1/4: every partial sum stays below 9 * 4 * 16 * tiles * r^2 = 576 * tiles * r^2 quarter units."""
    return _largest_radius(576 * tiles, cap)


def check_winograd_wgrad_operands(tiles, r_x, r_g):
    assert 576 * tiles * r_x * r_g < EXACT_F32, (tiles, r_x, r_g)


# Wide operands.  Integers up to 15 (or 28) fit an 8-bit significand: they cannot see an operand path that drops mantissa bits
# (a reduced-precision MFMA, a 16-bit staging format).  A wide pair is a dense operand of integers of up to ``dense_bits`` bits
# (of either parity: B^T d B adds four of them, and four odd numbers would always give an even V, one bit short) and a sparse
# one with a single odd entry of up to ``sparse_bits`` bits per contraction, so that every contraction is ONE product (no sum
# grows) while the matrix-core operands need 12 significant bits:
#   plain   (10, 8): dense |x| <= 1023: V = B^T d B <= 4 * 1023 needs 12 bits; sparse |v| <= 255: U = v * {1, 1/2, 1/4}
#   mirrored (6, 12): dense |x| <= 63: V <= 252 (8 bits); sparse |v| <= 4095: U = v / 4 needs 12 bits
# The bound: a filter with one tap g[a][b] = v has U[i][j] = G[i][a] G[j][b] v, and the column sums of |G| are 2, 1, 2, so the
# 3 x 3 values of M that the output transform adds have magnitudes that sum to at most 4 * |v| * max|V| = 16 * |v| * max|x|:
# in quarter units 64 * |v| * |x| < 2^24 (plain: 16 695 360; mirrored: 16 511 040); the single-channel |M| < 2^20 is one
# 8 x 12-bit (12 x 8-bit) product.  The weight gradients are the same with dY in the sparse role (E = A dY A^T of a tile with one
# nonzero pixel is +-v or 0, and dW = G^T S G weighs S like the filter transform does): one nonzero pixel per (sample, channel)
# and ONE sample, so that S is a single product.
WIDE_PLAIN, WIDE_MIRRORED = (10, 8), (6, 12)


def check_wide_operands(dense_max, sparse_max, winograd=True):
    """The precondition on a wide pair (see above); pointwise: the one product per output is below 2^24."""
    if winograd:
        assert 4 * dense_max < 2 ** 12 and 4 * dense_max * sparse_max < 2 ** 20, (dense_max, sparse_max)
        assert 64 * dense_max * sparse_max < EXACT_F32, (dense_max, sparse_max)
    else:
        assert dense_max * sparse_max < EXACT_F32, (dense_max, sparse_max)


def odd_integers(shape, bits, gen):
    """Odd integers of magnitude below 2^bits, both signs, float32; at least a quarter of them need all ``bits`` bits."""
    mag = 2 * torch.randint(0, 2 ** (bits - 1), tuple(shape), generator=gen) + 1
    sign = 2 * torch.randint(0, 2, tuple(shape), generator=gen) - 1
    exact = (mag * sign).double()
    out = exact.float()
    assert torch.equal(out.double(), exact) and float(out.abs().max()) < 2 ** bits
    return out


def wide_pair(shape_x, shape_w, gen, mirrored=False, winograd=True):
    """(x, w): a dense image of integers and a filter bank with exactly one nonzero tap, in one input channel, per output
    channel (square banks: the input channels are a permutation of the output channels, so the adjoint bank is as sparse and the
    data gradient is one product per pixel too).  ``mirrored``: 12-bit taps against a 6-bit image."""
    dense_bits, sparse_bits = WIDE_MIRRORED if mirrored else WIDE_PLAIN
    check_wide_operands(2 ** dense_bits - 1, 2 ** sparse_bits - 1, winograd)
    cout, cin, kh, kw = shape_w
    x = integers(shape_x, 2 ** dense_bits - 1, gen, dtype=torch.float32)
    v = odd_integers((cout,), sparse_bits, gen)
    chan = torch.randperm(cin, generator=gen) if cout == cin else torch.randint(0, cin, (cout,), generator=gen)
    tap = torch.arange(cout) % (kh * kw)    # every tap is somebody's
    w = torch.zeros(cout, cin, kh * kw)
    w[torch.arange(cout), chan, tap] = v
    return x, w.view(cout, cin, kh, kw)


def wide_wgrad_pair(shape_x, cout, gen, mirrored=False, winograd=True):
    """(x, gy) for the weight gradients: a dense image of ONE sample and a gradient with one nonzero pixel per channel."""
    dense_bits, sparse_bits = WIDE_MIRRORED if mirrored else WIDE_PLAIN
    check_wide_operands(2 ** dense_bits - 1, 2 ** sparse_bits - 1, winograd)
    batch, _, h, w = shape_x
    assert batch == 1, "a second sample would add a second product to every contraction"
    x = integers(shape_x, 2 ** dense_bits - 1, gen, dtype=torch.float32)
    gy = torch.zeros(1, cout, h * w)
    gy[0, torch.arange(cout), torch.randint(0, h * w, (cout,), generator=gen)] = odd_integers((cout,), sparse_bits, gen)
    return x, gy.view(1, cout, h, w)


def truncate_significand(x32, bits):
    """fp32 values cut to a ``bits``-bit significand (toward zero): what an operand path that drops mantissa bits would feed the
    matrix cores (a defect: simulated by the CPU test)."""
    keep = 0xFFFFFFFF ^ ((1 << (24 - bits)) - 1)
    word = _bits(x32) & keep
    word = torch.where(word >= 2 ** 31, word - 2 ** 32, word)
    return word.to(torch.int32).view(torch.float32).view(x32.shape)
