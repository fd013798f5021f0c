"""Exactly summable operands for the bf16 matrix-core kernels (csrc/gemm_bf16.hip, gemm256_bf16.hip, conv_bf16.hip,
conv_bf16_wgrad.hip, stem_conv.hip, column_sum.hip): tests without a tolerance.

bf16 holds every integer of magnitude <= 256, the matrix cores multiply bf16 operands exactly and add in fp32.  With integer
operands in [-r_a, r_a] and [-r_b, r_b] (optionally times one common power of two) and K * r_a * r_b < 2^24, every partial sum
of a contraction of length K is an integer below 2^24 and therefore exact in fp32 -- in ANY association, split-K slab order or
tile plan.  So an fp32 result must be bitwise the exact result and a bf16 result bitwise its round-to-nearest-even image; one
differing element is a defect, no rounding can excuse it.  References are computed in float64 on the CPU (53 bits: exact too).

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


def conv_ref(x, w, bias=None, stride=1):
    """F.conv2d with padding k // 2 in float64."""
    return F.conv2d(x.double(), w.double(), None if bias is None else bias.double(), stride=stride, padding=w.shape[2] // 2)


def conv_grads_ref(x, w, gy, stride=1):
    """(dL/dx, dL/dw) of ``conv_ref`` by autograd in float64."""
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    F.conv2d(xr, wr, stride=stride, padding=w.shape[2] // 2).backward(gy.double())
    return xr.grad, wr.grad


def pointwise_wgrad_ref(x, gy):
    """dW [Cout, Cin] of a 1x1 convolution: the contraction over images and pixels, float64."""
    return torch.einsum("bop,bip->oi", gy.double().flatten(2), x.double().flatten(2))
