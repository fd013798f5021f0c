"""Inputs, float64 references and element-wise error bounds shared by the bilinear-upsampling tests (``test_upsample_cases_cpu.py``
on the fp32 restatement of ``upsample_restatement.py``, ``test_upsample_cases_gpu.py`` on the kernels of csrc/upsample_ops.hip).
No GPU, numpy only (torch is used on the CPU to round to bfloat16 / float16).

Six kernels, three dtypes each, picked by ``launch_up`` from shape, alignment and stride.  SHAPES names, for every shape, the
kernel each direction MUST run (the GPU test asserts it through ``sis_last_kernel()``): a change of the planner that moves a shape
to another kernel fails there instead of leaving a kernel untested.

Reference.  ``ref = My x Mx^T`` (forward) and ``My^T gy Mx`` (backward) in float64, My / Mx from ``loss_cases.lerp_matrix``: the
source indices and lambdas are the FLOAT32 rule of ``sis_lerp_index`` (csrc/sis_device.h; it is the operator's definition and
PyTorch's own float32 rule), everything after them is float64.  Against this reference the only error left is the kernel's
own fp32 arithmetic.  16-bit inputs are generated as bf16 / f16 values: the cast is exact.

Bound, per element:   |got - ref| <= K u32 A + B,   u32 = 2^-24
  A   the same product taken with |M| and |x| (or |gy|): what every fp32 product and sum of the expression scales with.
  B   16-bit outputs: u_out |ref| + tiny (the rounding of the stored result; u_out = 2^-8 bf16, 2^-11 f16; tiny = 2^-25 for f16,
      the half spacing of its subnormals, 1e-37 for bf16).  f32: 0.
      bilinear_up2_fwd_direct_kernel alone gets a coordinate term in B: it forms its lambdas around STATIC indices as
      fma(s, 2j, -(j - 1)), from the unrounded product -- these products are NOT kept from contracting (the route's results stay
      bitwise what they were) -- so each lambda is within ulp32(src) of the rule's:  ulp32(src_x) |x[i1] - x[i0]| per axis, taken
      through the other axis' |M| (x axis) resp. on the horizontally interpolated rows (y axis).  No other route has one: they
      take their lambdas from ``sis_lerp_index``, whose product is rounded before it is used.
  ``figure = max(0, |error| - B) / (u32 A)``, so ``figure <= K`` IS the bound.  No case and no element is left out; besides the
  whole map the figure is taken on the first / last row and column, on the columns next to a wave boundary (direct kernels, rows
  wider than a wave) and on the rows / columns next to a tile boundary (tiled kernels), each held to K on its own (``regions``).

K = 4 x the largest figure of the fp32 restatement (upsample_restatement.py: the kernel's association in numpy float32) over
every case of CASES and STRIDED, per kernel -- measured on the CPU (``python tests/test_upsample_cases_cpu.py`` prints the
table), NOT on the device:
  bilinear_up_fwd_kernel            K =  9.64   (2.409: y, gen_2_26_32-f32-const)
  bilinear_up2_fwd_tiled_kernel     K = 11.61   (2.903: y, tiled_9x68-f32-noise)
  bilinear_up2_fwd_direct_kernel    K = 12.80   (3.200: y, direct_6x32-f32-ramp_i)
  bilinear_up_bwd_kernel            K = 14.10   (3.525: gx, gen_2_26_32-f32-offset)
  bilinear_up2_bwd_tiled_kernel     K = 12.41   (3.102: gx, tiled_9x68-f32-ramp_i)
  bilinear_up2_bwd_direct_kernel    K = 12.16   (3.039: gx, direct_3x16-f32-offset)
(u32 is the unit roundoff, half an ulp: a figure of 3 is an error of 1.5 ulp of A.  The forward has 6 products and 3 sums per
output, the backward up to 9 x 7 weighted terms per cell; 16-bit outputs leave figures of 0 almost everywhere: B covers them.)

Exact checks (no K): a constant field comes back within 2 ulp of the output type; with a one-hot x (forward) or gy (backward)
every element outside the footprint the rule names is exactly 0.0 -- impulses at the first and last cell, next to a wave edge,
next to tile edges, and at the outputs where ``lerp_tables(fused=True)`` differs from the rule (3 -> 7 at output 3, 3 -> 11 at
output 5; 2 -> 26 / 32 at the last output, where l1 turns negative but both weights share a cell).  Identities, in float64 on the returned tensors:  <up(x), gy> = <x, up^T(gy)> within
the two bounds summed, and sum gx = sum gy within the bound of gx plus the float64 deviation of the lambda pairs from 1.
"""
import functools
import zlib

import numpy as np

from loss_cases import U32, U_BF16, lerp_matrix, lerp_tables, need

U_F16 = 2.0 ** -11
U_OUT = {"f32": 0.0, "bf16": U_BF16, "f16": U_F16}
TINY_OUT = {"f32": 0.0, "bf16": 1e-37, "f16": 2.0 ** -25}
ULP_OUT = {"f32": 2.0 ** -23, "bf16": 2.0 ** -7, "f16": 2.0 ** -10}    # spacing of the type at [1, 2)
DTYPES = ("f32", "bf16", "f16")
CONST = 1.375          # a bf16 value in [1, 2): one ulp of the output type is ULP_OUT

GEN_F, TIL_F, DIR_F = "bilinear_up_fwd_kernel", "bilinear_up2_fwd_tiled_kernel", "bilinear_up2_fwd_direct_kernel"
GEN_B, TIL_B, DIR_B = "bilinear_up_bwd_kernel", "bilinear_up2_bwd_tiled_kernel", "bilinear_up2_bwd_direct_kernel"
K = {GEN_F: 9.64, TIL_F: 11.61, DIR_F: 12.80, GEN_B: 14.10, TIL_B: 12.41, DIR_B: 12.16}

# the constants of csrc/upsample_ops.hip the regions and the LDS checks depend on
UF_OR, UF_OC, UF_SR, UF_SC = 16, 512, 16 // 2 + 2, 512 // 2 + 2     # tiled forward: output tile, source rows / columns in LDS
UB_TY, UB_TX = 8, 64                                                # tiled backward: grad_x tile
WAVE_COLS = 256                                                     # direct kernels: 64 lanes x 4 source columns

# id: (shape [B, C, h, w], (oh, ow), forward kernel, backward kernel)
SHAPES = {
    # ---- direct (x2, w / 4 divides 64 or is a multiple of it)
    "direct_3x16": ((2, 3, 3, 16), (6, 32), DIR_F, DIR_B),      # 4 lanes per row: 16 rows per wave, waves span planes; h odd: RP = 1;
                                                                # 72 lanes: a ragged (only) workgroup
    "direct_2x4": ((1, 1, 2, 4), (4, 8), DIR_F, DIR_B),         # one lane per row, two lanes in all; h even: RP = 2, ONE lane
    "direct_6x32": ((1, 3, 6, 32), (12, 64), DIR_F, DIR_B),     # h even with several row pairs; 8 lanes per row, 144 / 72 lanes
    "direct_5x256": ((1, 2, 5, 256), (10, 512), DIR_F, DIR_B),  # exactly one wave per row; 640 lanes: the third workgroup ragged
    "direct_2x512": ((1, 1, 2, 512), (4, 1024), DIR_F, DIR_B),  # two waves per row: the wl == 0 / wl == 63 neighbour loads
    "direct_4x1024": ((1, 2, 4, 1024), (8, 2048), DIR_F, DIR_B),  # four waves per row, a row per workgroup
    # ---- tiled forward (x2, the direct kernel declines: w % 4 != 0); their backward is the generic kernel (ow % 8 != 0)
    "tiled_9x258": ((1, 2, 9, 258), (18, 516), TIL_F, GEN_B),   # two row tiles, a 4-wide second column tile
    "tiled_3x259": ((1, 2, 3, 259), (6, 518), TIL_F, GEN_B),    # odd w: row starts alternate 16-byte alignment, scalar stores
    "tiled_2x2": ((1, 2, 2, 2), (4, 4), TIL_F, GEN_B),          # the smallest plane
    "tiled_7x9": ((1, 2, 7, 9), (14, 18), TIL_F, GEN_B),        # x2 with odd w in the backward: the 6-candidate branch
    # ---- tiled backward (x2, w % 4 == 0 but w / 4 neither divides 64 nor is a multiple of it, ow % 8 == 0)
    "tiled_9x68": ((2, 2, 9, 68), (18, 136), TIL_F, TIL_B),     # two ragged tiles per axis
    "tiled_5x12": ((1, 3, 5, 12), (10, 24), TIL_F, TIL_B),
    "tiled_1x12": ((1, 2, 1, 12), (2, 24), GEN_F, TIL_B),       # h = 1: the forward is the generic kernel's, the backward tiled
    # ---- generic
    "gen_12_27": ((1, 2, 5, 12), (11, 27), GEN_F, GEN_B),       # 12 -> 27, 5 -> 11; ow % 4 != 0
    "gen_x4_x3": ((1, 2, 5, 6), (20, 18), GEN_F, GEN_B),        # x4 and x3: the backward's general loop (7 / 9 candidates)
    "gen_same": ((1, 2, 6, 6), (6, 6), GEN_F, GEN_B),           # out equal to in: scale 1, every lambda 0
    "gen_h1_x2": ((1, 2, 1, 5), (2, 10), GEN_F, GEN_B),         # x2 with h = 1
    "gen_in1_h": ((1, 2, 1, 4), (3, 9), GEN_F, GEN_B),          # in = 1 on the y axis (scale 0)
    "gen_in1_w": ((1, 2, 4, 1), (9, 3), GEN_F, GEN_B),          # in = 1 on the x axis
    "gen_out1_h": ((1, 2, 3, 5), (1, 9), GEN_F, GEN_B),         # out = 1 on the y axis (scale 0 with in > 1: the sy > 0 branches)
    "gen_out1_w": ((1, 2, 5, 3), (7, 1), GEN_F, GEN_B),         # out = 1 on the x axis
    "gen_down": ((1, 2, 9, 10), (4, 7), GEN_F, GEN_B),          # down-sampling: scale > 1, cells nobody reads
    "gen_3_7_11": ((1, 2, 3, 3), (7, 11), GEN_F, GEN_B),        # 3 -> 7 and 3 -> 11: where a fused lambda leaks
    "gen_138_274": ((1, 1, 2, 138), (3, 274), GEN_F, GEN_B),    # the last source coordinate rounds to 137 + 1.5e-5: i1 is clamped under a
                                                                # NON-zero l1 (at every other shape here it is exactly 0 there)
    "gen_2_26_32": ((1, 1, 2, 2), (26, 32), GEN_F, GEN_B),      # in = 2: a fused lambda is negative at the last output
}

# the strided entry (upsample2x_into / upsample2x_grad_from): id: (shape of x, extra channels S, forward, backward kernel)
STRIDED = {
    "strided_direct": ((2, 3, 4, 16), 2, DIR_F, DIR_B),
    "strided_tiled": ((2, 2, 5, 12), 3, TIL_F, TIL_B),
}

DATA = ("noise", "offset", "const", "ramp_i", "ramp_j")


def round_to(a, dtype):
    """float32 array rounded to ``dtype`` ('f32', 'bf16', 'f16'), as float32."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    if dtype == "f32":
        return a
    import torch
    return torch.from_numpy(a).to(torch.bfloat16 if dtype == "bf16" else torch.float16).float().numpy()


class Case:
    def __init__(self, shape_id, dtype, data, strided=False):
        self.shape_id, self.dtype, self.data, self.strided = shape_id, dtype, data, strided
        if strided:
            self.shape, self.extra, self.fwd, self.bwd = STRIDED[shape_id]
            self.size = (2 * self.shape[2], 2 * self.shape[3])
        else:
            self.shape, self.size, self.fwd, self.bwd = SHAPES[shape_id]
            self.extra = 0
        self.id = f"{shape_id}-{dtype}-{data}"

    def __repr__(self):
        return self.id


# ------------------------------------------------------------------------------------------------------------ impulses

def leak_outputs(n_in, n_out):
    """Outputs where the lambda of an unrounded product (``lerp_tables(fused=True)``) names another footprint than the rule:
    a weight that is exactly 0 becomes non-zero, or l1 turns negative."""
    _, _, l0, l1, _ = lerp_tables(n_in, n_out)
    _, _, f0, f1, _ = lerp_tables(n_in, n_out, fused=True)
    return [int(o) for o in np.nonzero(((l1 == 0) != (f1 == 0)) | ((l0 == 0) != (f0 == 0)) | (f1 < 0))[0]]


def _edges(n, step):
    """Both neighbours of every multiple of ``step`` inside 0..n-1."""
    out = []
    for k in range(step, n, step):
        out += [k - 1, k]
    return out


def _axis_points(n_in, n_out, fwd, bwd, axis):
    """(input positions for a one-hot x, output positions for a one-hot gy) on one axis."""
    i0, i1, _, _, _ = lerp_tables(n_in, n_out)
    leaks = leak_outputs(n_in, n_out)
    ins = [0, n_in - 1] + [int(i1[o]) for o in leaks] + [int(i0[o]) for o in leaks]
    outs = [0, n_out - 1] + leaks
    if axis == "x":
        if fwd == DIR_F:
            ins += _edges(n_in, WAVE_COLS)
        if bwd == DIR_B:
            outs += _edges(n_out, 2 * WAVE_COLS)
        if fwd == TIL_F:
            ins += _edges(n_in, UF_OC // 2)
        if bwd == TIL_B:
            outs += _edges(n_out, 2 * UB_TX)
    else:
        if fwd == TIL_F:
            ins += _edges(n_in, UF_OR // 2)
        if bwd == TIL_B:
            outs += _edges(n_out, 2 * UB_TY)
    uniq = lambda v, n: sorted({p for p in v if 0 <= p < n})
    return uniq(ins, n_in), uniq(outs, n_out)


def impulses(shape_id):
    """-> (cells (i, j) for a one-hot x, outputs (Y, X) for a one-hot gy): the points of the two axes paired up (the longer list
    sets the count, the shorter one cycles), so every listed row and every listed column carries an impulse."""
    (_, _, h, w), (oh, ow), fwd, bwd = SHAPES[shape_id]
    yi, yo = _axis_points(h, oh, fwd, bwd, "y")
    xi, xo = _axis_points(w, ow, fwd, bwd, "x")
    pair = lambda a, b: [(a[k % len(a)], b[k % len(b)]) for k in range(max(len(a), len(b)))]
    return pair(yi, xi), pair(yo, xo)


def _cases():
    out = []
    for sid in SHAPES:
        nx, ng = map(len, impulses(sid))
        for dt in DTYPES:
            out += [Case(sid, dt, d) for d in DATA]
            out += [Case(sid, dt, f"hot{k}") for k in range(max(nx, ng))]
    return out


CASES = _cases()
STRIDED_CASES = [Case(sid, dt, d, strided=True) for sid in STRIDED for dt in DTYPES for d in ("noise", "offset")]
CASE = {c.id: c for c in CASES + STRIDED_CASES}


# ------------------------------------------------------------------------------------------------------------ inputs, references, bounds

def _field(kind, rng, shape):
    n = rng.standard_normal(shape)
    if kind == "noise":
        return n
    if kind == "offset":        # shows up an error in the weight sum: 1e3 (l0 + l1 - 1) is not hidden by the noise
        return n + 1e3
    if kind == "const":
        return np.full(shape, CONST)
    if kind == "ramp_i":
        return np.broadcast_to(np.arange(shape[2], dtype=np.float64)[:, None], shape)
    if kind == "ramp_j":
        return np.broadcast_to(np.arange(shape[3], dtype=np.float64)[None, :], shape)
    raise KeyError(kind)


def _ulp32(v):
    return np.spacing(np.abs(np.asarray(v, dtype=np.float32))).astype(np.float64)


def _build(case):
    rng = np.random.default_rng(zlib.crc32(case.id.encode()))
    B, C, h, w = case.shape
    oh, ow = case.size
    hot_x = hot_g = None
    if case.data.startswith("hot"):
        k = int(case.data[3:])
        cells, outs = impulses(case.shape_id)
        hot_x, hot_g = cells[k % len(cells)], outs[k % len(outs)]
        x = np.zeros((B, C, h, w))
        x[:, :, hot_x[0], hot_x[1]] = 1.0
        gy = np.zeros((B, C, oh, ow))
        gy[:, :, hot_g[0], hot_g[1]] = 1.0
    else:
        x, gy = _field(case.data, rng, (B, C, h, w)), _field(case.data, rng, (B, C, oh, ow))
        if case.data == "offset" and case.dtype == "f16" and 1e3 * (oh / h) * (ow / w) > 3e4:
            gy = gy - 900.0     # a cell of 2 -> 26 x 2 -> 32 sums 208 weights: at 1e3 its gradient is no float16; the offset is 1e2 there
    x, gy = round_to(x, case.dtype), round_to(gy, case.dtype)          # float32 arrays holding values of the case's type
    My, Mx = lerp_matrix(h, oh), lerp_matrix(w, ow)
    x64, g64 = x.astype(np.float64), gy.astype(np.float64)
    fwd = lambda a, P=My, Q=Mx: np.einsum("Yi,bcij,Xj->bcYX", P, a, Q)
    bwd = lambda a, P=My, Q=Mx: np.einsum("Yi,bcYX,Xj->bcij", P, a, Q)
    y, gx = fwd(x64), bwd(g64)
    A_y, A_gx = U32 * fwd(np.abs(x64), np.abs(My), np.abs(Mx)), U32 * bwd(np.abs(g64), np.abs(My), np.abs(Mx))
    u, tiny = U_OUT[case.dtype], TINY_OUT[case.dtype]
    B_y, B_gx = u * np.abs(y) + tiny, u * np.abs(gx) + tiny
    (y0, y1, _, _, sy), (x0, x1, _, _, sx) = lerp_tables(h, oh), lerp_tables(w, ow)
    if case.fwd == DIR_F:   # the coordinate term of the static-index lambdas (module docstring)
        ux = _ulp32(sx * np.arange(ow, dtype=np.float32))
        uy = _ulp32(sy * np.arange(oh, dtype=np.float32))
        Ex = np.einsum("Yi,bciX->bcYX", np.abs(My), np.abs(x64[:, :, :, x1] - x64[:, :, :, x0])) * ux[None, None, None, :]
        hrows = np.einsum("bcij,Xj->bciX", x64, Mx)
        Ey = np.abs(hrows[:, :, y1, :] - hrows[:, :, y0, :]) * uy[None, None, :, None]
        B_y = B_y + Ex + Ey
    return dict(x=x, gy=gy, My=My, Mx=Mx, y=y, gx=gx, A_y=A_y, B_y=B_y, A_gx=A_gx, B_gx=B_gx, hot_x=hot_x, hot_g=hot_g,
                src_y=(sy * np.arange(oh, dtype=np.float32)), src_x=(sx * np.arange(ow, dtype=np.float32)))


@functools.lru_cache(maxsize=4)
def _build_cached(case_id):
    return _build(CASE[case_id])


def build(case):
    """Inputs (float32 arrays holding values of the case's type), float64 references and bounds at K = 1.  Left unchanged by
    every user; the last few are kept."""
    return _build_cached(case.id)


# ------------------------------------------------------------------------------------------------------------ figures

def regions(case, which):
    """name -> boolean mask [rows, cols] of the map ``which`` ('y': the forward's output, 'gx': the backward's)."""
    rows, cols = case.size if which == "y" else case.shape[2:]
    kern = case.fwd if which == "y" else case.bwd
    r, c = np.arange(rows)[:, None], np.arange(cols)[None, :]
    full = np.ones((rows, cols), dtype=bool)
    out = dict(all=full, first_row=full & (r == 0), last_row=full & (r == rows - 1), first_col=full & (c == 0),
               last_col=full & (c == cols - 1))
    if kern in (DIR_F, DIR_B):      # a lane's neighbour across a wave boundary: outputs 8g / 8g + 7, cells 4g / 4g + 3 at g % 64 = 0 / 63
        step = 2 * WAVE_COLS if which == "y" else WAVE_COLS
        out["wave_cols"] = full & np.isin(c, _edges(cols, step))
    if kern == TIL_F:
        out["tile_rows"] = full & np.isin(r, _edges(rows, UF_OR))
        out["tile_cols"] = full & np.isin(c, _edges(cols, UF_OC))
    if kern == TIL_B:
        out["tile_rows"] = full & np.isin(r, _edges(rows, UB_TY))
        out["tile_cols"] = full & np.isin(c, _edges(cols, UB_TX))
    return {k: m for k, m in out.items() if m.any()}


def figures(case, inp, y=None, gx=None):
    """'y/region' / 'gx/region' -> the K this result needs on that region (``loss_cases.need``: inf for a non-finite error)."""
    out = {}
    for which, got in (("y", y), ("gx", gx)):
        if got is None:
            continue
        ref, A, Bb = inp[which], inp["A_" + which], inp["B_" + which]
        err = np.asarray(got, dtype=np.float64).reshape(ref.shape) - ref
        for name, m in regions(case, which).items():
            out[f"{which}/{name}"] = need(err[:, :, m], A[:, :, m], Bb[:, :, m])
    return out


def kernel_of(case, key):
    return case.fwd if key.startswith("y") else case.bwd


def exact_checks(case, inp, y=None, gx=None):
    """-> list of failures of the checks that carry no K: footprints of the one-hot cases (exactly 0.0 outside), the constant
    field within 2 ulp of the output type, the ramps on the float32 source coordinate (see ``ramp_slack``)."""
    bad = []
    My, Mx = inp["My"], inp["Mx"]
    if inp["hot_x"] is not None and y is not None:
        i, j = inp["hot_x"]
        outside = np.outer(My[:, i], Mx[:, j]) == 0
        leak = np.abs(np.asarray(y, dtype=np.float64))[:, :, outside]
        if leak.size and leak.max() != 0:
            Y, X = np.argwhere(outside)[int(np.argmax(leak.max(axis=(0, 1))))]
            bad.append(f"{case.id}: one-hot x at {(i, j)}: output {(int(Y), int(X))} outside the footprint holds {leak.max():.3g}")
    if inp["hot_g"] is not None and gx is not None:
        Y, X = inp["hot_g"]
        outside = np.outer(My[Y, :], Mx[X, :]) == 0
        leak = np.abs(np.asarray(gx, dtype=np.float64))[:, :, outside]
        if leak.size and leak.max() != 0:
            i, j = np.argwhere(outside)[int(np.argmax(leak.max(axis=(0, 1))))]
            bad.append(f"{case.id}: one-hot gy at {(Y, X)}: cell {(int(i), int(j))} outside the footprint holds {leak.max():.3g}")
    if case.data == "const" and y is not None:
        ulps = np.abs(np.asarray(y, dtype=np.float64) - CONST).max() / ULP_OUT[case.dtype]
        if not ulps <= 2:
            bad.append(f"{case.id}: the constant field comes back {ulps:.3g} ulp off")
    if case.data in ("ramp_i", "ramp_j") and y is not None:
        src = inp["src_y"][:, None] if case.data == "ramp_i" else inp["src_x"][None, :]
        if _ramp_exact(case, inp["x"].astype(np.float64)):
            off = np.abs(np.asarray(y, dtype=np.float64) - src.astype(np.float64)[None, None])
            lim = K[case.fwd] * inp["A_y"] + inp["B_y"] + ramp_slack(src)[None, None]
            if not (off <= lim).all():
                at = np.unravel_index(int(np.argmax(off - lim)), off.shape)
                bad.append(f"{case.id}: ramp: output {at[2:]} is {off[at]:.3g} off its source coordinate (allowed {lim[at]:.3g})")
    return bad


def _ramp_exact(case, ramp):
    """The ramp survived the rounding to the case's type (bf16 holds the integers up to 256, f16 up to 2048)."""
    idx = np.arange(ramp.shape[2])[:, None] if case.data == "ramp_i" else np.arange(ramp.shape[3])[None, :]
    return bool((ramp == idx[None, None]).all())


def ramp_slack(src):
    """The float64 reference of a ramp is l0 i0 + l1 i1 with l0 = fl(1 - l1): it differs from the float32 source coordinate
    by at most u32 i0 (the rounding of l0), 2 u32 src with room."""
    return 2 * U32 * np.abs(src.astype(np.float64))


def identity_checks(case, inp, y, gx):
    """-> list of failures: <up(x), gy> = <x, up^T(gy)> within the two bounds summed; sum gx = sum gy within the bound of gx plus
    the deviation of the float32 lambda pairs from 1 (float64 row sums of My, Mx), per plane."""
    bad = []
    y, gx = np.asarray(y, dtype=np.float64), np.asarray(gx, dtype=np.float64)
    x, gy = inp["x"].astype(np.float64), inp["gy"].astype(np.float64)
    by, bg = K[case.fwd] * inp["A_y"] + inp["B_y"], K[case.bwd] * inp["A_gx"] + inp["B_gx"]
    lhs, rhs = (y * gy).sum(), (x * gx).sum()
    tol = (np.abs(gy) * by).sum() + (np.abs(x) * bg).sum()
    tol += 8 * 2.0 ** -53 * ((np.abs(y * gy)).sum() + np.abs(x * gx).sum())          # the float64 sums of this check itself
    if not abs(lhs - rhs) <= tol:
        bad.append(f"{case.id}: <up x, gy> - <x, up^T gy> = {lhs - rhs:.3g}, allowed {tol:.3g}")
    rs = np.outer(inp["My"].sum(axis=1), inp["Mx"].sum(axis=1))                    # weight each gy element hands out in all
    want = (gy * rs[None, None]).sum(axis=(2, 3))
    tol2 = bg.sum(axis=(2, 3)) + 8 * 2.0 ** -53 * np.abs(gy).sum(axis=(2, 3)) * max(1, rs.max())
    dev = np.abs(gx.sum(axis=(2, 3)) - want)
    if not (dev <= tol2).all():
        bad.append(f"{case.id}: sum gx - sum gy = {dev.max():.3g}, allowed {tol2.flat[int(np.argmax(dev))]:.3g}")
    return bad
