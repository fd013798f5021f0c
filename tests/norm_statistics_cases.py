"""Inputs, float64 references and error bounds shared by the norm-statistics tests (``test_norm_statistics_cpu.py`` on the fp32
restatement of ``norm_restatement.py``, ``test_norm_statistics_gpu.py`` on the kernels).  No GPU, numpy only (torch is used on
the CPU to round to bfloat16).

Every normalisation here is stated on ONE canonical layout ``X[R, U, L]``: R statistic rows (a GroupNorm (sample, group), a
batch-norm channel, a LayerNorm / weight row), each made of U units of L elements (the channels of a group, the samples of a
channel; U = 1 for rows) -- ``to_canon`` / ``from_canon`` are pure reshapes of the operator's own layout, ``canon_param``
broadcasts gamma / beta, ``param_grad`` reduces per-element terms to d(gamma) / d(beta).

Bounds (u = 2^-24, K per kernel form, measured on the restatement -- see the constants below):
  output   |y - y64|       <= K u |gamma| (|mean| rstd + |xhat| + 1) + u_out |y64|
  mean     |m - m64|       <= K u (|mean| + 1 / rstd)
  rstd     |r - r64| / r64 <= K u (1 + |mean| rstd)
  dx       |dx - dx64|     <= K u G (|mean| rstd + |xhat| + 1) + u_out |dx64|,   G = rstd * max_row |gamma g'|
  dgamma   |dg - dg64|     <= K u sum |g'| (|mean| rstd + |xhat| + 1)      (the terms g' xhat, each with xhat's own error)
  dbeta    |db - db64|     <= K u sum |g'|
The (|mean| rstd) part is what fp32 storage of the mean forces on xhat = (x - mean) rstd; in d(gamma) that error is common to
the whole row, which is why its terms carry it (u sum |g' xhat| alone would be below the error of ANY fp32 kernel at
|mean| / std = 4096)."""
import numpy as np

U32 = 2.0 ** -24
U_BF16 = 2.0 ** -8

# K = 4 x the largest ratio error / (bound at K = 1) of the fp32 restatement over every family and shape of
# test_norm_statistics_cpu.py (``python tests/test_norm_statistics_cpu.py`` prints the table).  Measured on the CPU restatement,
# NOT on the device.
K_GN = 14.43       # measured 3.608 (y, const_0p1, 132 x 132 planes)  GroupNorm: sliced two-pass + Chan merge, x a + b apply
K_GN_GROUP = 11.21 # measured 2.802 (y, offset_p256 in bf16)          GroupNorm single-pass group kernels
K_BN_MODE = 22.43  # measured 5.607 (y, offset_m4096, 70 samples)     batch-norm mode of group_norm.hip: a merge step per sample
K_BN3 = 13.61      # measured 3.402 (y, offset_m4096)                 bn_ops three-launch form (16 384-element slices)
K_BN1 = 12.72      # measured 3.181 (y, const_0p1 + residual)         bn_ops fused / wide forms (the channel as one slice)
K_LN = 9.90        # measured 2.475 (dgamma, const_0p1)               LayerNorm, (x - mean) rstd g + b
K_WS = 7.56        # measured 1.890 (y, offset_m4096)                 weight standardisation
# No form needs K > 32: the x a + b apply loses nothing beyond what fp32 storage of the mean forces.
RELU_MARGIN = 8.0  # every pre-activation of a ReLU case is at least this many output bounds away from zero ...
K_RELU = 32.0      # ... at THIS K (no form's K may exceed it), so that the inputs do not depend on the measured constants


def round_bf16(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).bfloat16().float().numpy()


# ------------------------------------------------------------------------------------------------------------ layouts

def to_canon(op, x, groups=None):
    """op layout -> [R, U, L].  'gn': x [B, C, HW]; 'bn' (batch-norm mode of group_norm.hip): rows = channels, units = samples;
    'bnops' (bn_ops.hip): a channel's B * HW values as ONE unit (its slices run across samples); 'rows': x [rows, n]."""
    if op == "gn":
        b, c, hw = x.shape
        return x.reshape(b * groups, c // groups, hw)
    if op == "bn":
        return np.ascontiguousarray(x.transpose(1, 0, 2))
    if op == "bnops":
        b, c, hw = x.shape
        return np.ascontiguousarray(x.transpose(1, 0, 2)).reshape(c, 1, b * hw)
    return x.reshape(x.shape[0], 1, -1)


def canon_shape(op, shape, groups=None):
    b, c = shape[0], shape[1]
    hw = int(np.prod(shape[2:]))
    if op == "gn":
        return (b * groups, c // groups, hw)
    if op == "bn":
        return (c, b, hw)
    if op == "bnops":
        return (c, 1, b * hw)
    return (b, 1, int(np.prod(shape[1:])))


def from_canon(op, X, shape, groups=None):
    b, c = shape[0], shape[1]
    hw = int(np.prod(shape[2:]))
    if op == "gn":
        return X.reshape(b, c, hw).reshape(shape)
    if op == "bn":
        return np.ascontiguousarray(X.transpose(1, 0, 2)).reshape(shape)
    if op == "bnops":
        return np.ascontiguousarray(X.reshape(c, b, hw).transpose(1, 0, 2)).reshape(shape)
    return X.reshape(shape)


def canon_param(op, p, shape, groups=None):
    """gamma / beta [C] (LayerNorm: [n]) broadcastable against the canonical layout."""
    b, c = shape[0], shape[1]
    if op == "gn":
        return np.tile(p, b).reshape(b * groups, c // groups, 1)
    if op in ("bn", "bnops"):
        return p.reshape(c, 1, 1)
    return p.reshape(1, 1, -1)


def param_grad(op, T, shape, groups=None):
    """per-element terms [R, U, L] -> their sum per parameter (in T's dtype: float64 for references and bounds)."""
    b, c = shape[0], shape[1]
    if op == "gn":
        return T.reshape(b, c, -1).sum(axis=(0, 2))
    if op in ("bn", "bnops"):
        return T.sum(axis=(1, 2))
    return T.sum(axis=(0, 1))


# ------------------------------------------------------------------------------------------------------------ input families

FAMILIES = ("control", "offset_p256", "offset_m4096", "between", "halves", "const_64", "const_0p1", "const_plane", "scale_hi",
            "scale_lo")


def family(name, cshape, dtype="f32", seed=0):
    """-> (X float32 [R, U, L] exact in ``dtype`` ('f32' / 'bf16'), free bool [R, U, L]: the elements a ReLU case may re-draw).

    control       mean 0, std 1
    offset_p256   256 + z                 (bf16: 64 + 0.5 k, k in {-2..1} -- the type's grid at 64, |mean| / std = 114)
    offset_m4096  -4096 + z               (bf16: -4096 + 32 k, the same on the grid at 4096)
    between       unit (r, u) has its own mean, spread evenly over [-50, 50], std 0.1: Chan's cross term carries the variance
    halves        first half of every unit at -50, second half at +50, std 0.1: the same across the slices of one plane
    const_64      all elements 64.0 (exact: variance 0, rstd = 1 / sqrt(eps))
    const_0p1     all elements fl(0.1) (the mean is not a short sum of exact terms)
    const_plane   unit 0 of every row constant 3.0 inside an otherwise random row (U = 1: row 0 constant)
    scale_hi      std 2^12
    scale_lo      std 2^-12: variance far below eps"""
    R, U, L = cshape
    rng = np.random.default_rng(1000 * seed + FAMILIES.index(name))
    z = rng.standard_normal(cshape)
    free = np.ones(cshape, dtype=bool)
    if name == "control":
        X = z
    elif name in ("offset_p256", "offset_m4096"):
        m = 256.0 if name == "offset_p256" else -4096.0
        if dtype == "bf16":
            m = 64.0 if name == "offset_p256" else -4096.0
            X = m + (abs(m) / 128.0) * rng.integers(-2, 2, size=cshape)
        else:
            X = m + z
    elif name == "between":
        means = np.linspace(-50.0, 50.0, R * U).reshape(R, U, 1) if R * U > 1 else np.full((1, 1, 1), 50.0)
        X = means + 0.1 * z
    elif name == "halves":
        X = np.where(np.arange(L) < L // 2, -50.0, 50.0) + 0.1 * z
    elif name in ("const_64", "const_0p1"):
        X = np.full(cshape, 64.0 if name == "const_64" else 0.1)
        free[:] = False
    elif name == "const_plane":
        X = z.copy()
        if U > 1:
            X[:, 0, :] = 3.0
            free[:, 0, :] = False
        else:
            X[0] = 3.0
            free[0] = False
    elif name == "scale_hi":
        X = z * 2.0 ** 12
    elif name == "scale_lo":
        X = z * 2.0 ** -12
    else:
        raise KeyError(name)
    X = X.astype(np.float32)
    if dtype == "bf16":
        X = round_bf16(X)
    return X, free


def params(n, seed, unit=False):
    rng = np.random.default_rng(77 + seed)
    if unit:
        return np.ones(n, dtype=np.float32), np.zeros(n, dtype=np.float32)
    return (1 + 0.2 * rng.standard_normal(n)).astype(np.float32), (0.3 * rng.standard_normal(n)).astype(np.float32)


def gradient(cshape, seed, dtype="f32"):
    g = np.random.default_rng(991 + seed).standard_normal(cshape).astype(np.float32)
    return round_bf16(g) if dtype == "bf16" else g


# ------------------------------------------------------------------------------------------------------------ float64 reference

def reference(X, gamma, beta, eps, relu=False, res=None, g=None):
    """Plain formulas in float64 on the canonical layout (gamma / beta broadcastable).  -> dict: mean, var (biased), rstd [R],
    n, xhat, pre (pre-activation, residual included), y, and with ``g``: gp (gated gradient), dx, tg / tb (the terms of
    d(gamma) / d(beta))."""
    X = X.astype(np.float64)
    gamma, beta = np.asarray(gamma, dtype=np.float64), np.asarray(beta, dtype=np.float64)
    n = X.shape[1] * X.shape[2]
    mean = X.mean(axis=(1, 2))
    var = ((X - mean[:, None, None]) ** 2).mean(axis=(1, 2))
    rstd = 1.0 / np.sqrt(var + eps)
    xhat = (X - mean[:, None, None]) * rstd[:, None, None]
    pre = xhat * gamma + beta
    if res is not None:
        pre = pre + res.astype(np.float64)
    y = np.maximum(pre, 0.0) if relu else pre
    out = dict(mean=mean, var=var, rstd=rstd, n=n, xhat=xhat, pre=pre, y=y, gamma=np.broadcast_to(gamma, X.shape))
    if g is not None:
        gp = g.astype(np.float64) * (pre > 0.0) if relu else g.astype(np.float64)
        gg = gp * gamma
        m1 = gg.mean(axis=(1, 2))[:, None, None]
        m2 = (gg * xhat).mean(axis=(1, 2))[:, None, None]
        out.update(gp=gp, dx=rstd[:, None, None] * (gg - m1 - xhat * m2), tg=gp * xhat, tb=gp)
    return out


def running_reference(ref, rm0, rv0, momentum):
    """running_mean / running_var (unbiased) after one training step, float64."""
    n = ref["n"]
    unb = ref["var"] * (n / (n - 1.0)) if n > 1 else ref["var"]
    return (1 - momentum) * rm0.astype(np.float64) + momentum * ref["mean"], (1 - momentum) * rv0.astype(np.float64) + momentum * unb


# ------------------------------------------------------------------------------------------------------------ bounds (at K = 1)

def _cond(ref):
    return (np.abs(ref["mean"]) * ref["rstd"])[:, None, None] + np.abs(ref["xhat"]) + 1.0


def bound_y(ref, K, u_out=U32):
    return K * U32 * np.abs(ref["gamma"]) * _cond(ref) + u_out * np.abs(ref["y"])


def bound_mean(ref, K):
    return K * U32 * (np.abs(ref["mean"]) + 1.0 / ref["rstd"])


def bound_rstd_rel(ref, K):
    return K * U32 * (1.0 + np.abs(ref["mean"]) * ref["rstd"])


def bound_dx(ref, K, u_out=U32):
    G = ref["rstd"] * np.abs(ref["gamma"] * ref["gp"]).max(axis=(1, 2))
    return K * U32 * G[:, None, None] * _cond(ref) + u_out * np.abs(ref["dx"])


def bound_dgamma_terms(ref):
    return np.abs(ref["gp"]) * _cond(ref)


def bound_dbeta_terms(ref):
    return np.abs(ref["gp"])


def bound_running(ref, rm64, rv64, momentum, K):
    """The K part of the running statistics' bounds (the update's own rounding, 2 u |value|, is added by ``ratios``).
    running_mean: the mean's bound scaled by the momentum; running_var: var = 1 / rstd^2 - eps, so twice rstd's relative bound
    on the (unbiased) variance, scaled by the momentum."""
    n = ref["n"]
    unb = ref["var"] * (n / (n - 1.0)) if n > 1 else ref["var"]
    return momentum * bound_mean(ref, K), momentum * 2 * bound_rstd_rel(ref, K) * unb


# ------------------------------------------------------------------------------------------------------------ ReLU cases

def build_relu_case(op, shape, groups, name, dtype, seed, eps, residual=False, K=K_RELU):
    """Inputs of a ReLU case whose every pre-activation (residual included) is at least RELU_MARGIN output bounds away from zero,
    so that no kernel within the bound can flip a gate: offending elements are re-drawn (x where the family leaves it free, else
    the residual), and where a whole constant plane offends, its channel's beta is moved away from zero.  No element is excluded.
    -> (X, gamma, beta, res or None), parameters in the operator's layout ([C])."""
    cshape = canon_shape(op, shape, groups)
    X, free = family(name, cshape, dtype, seed)
    gamma, beta = params(shape[1], seed)
    rng = np.random.default_rng(5 + seed)
    res = rng.standard_normal(cshape).astype(np.float32) if residual else None
    for it in range(200):
        gc, bc = canon_param(op, gamma, shape, groups), canon_param(op, beta, shape, groups)
        ref = reference(X, gc, bc, eps, True, res)
        bad = np.abs(ref["pre"]) < RELU_MARGIN * bound_y(ref, K)
        if not bad.any():
            return X, gamma, beta, res
        if residual:
            res[bad] = (rng.standard_normal(int(bad.sum())) * 2).astype(np.float32)
            continue
        redraw = bad & free
        if redraw.any():
            X2, _ = family(name, cshape, dtype, seed + 100 + it)
            X = np.where(redraw, X2, X)
        stuck = bad & ~free if it < 10 else bad   # (after ten rounds of re-drawing: move beta for whatever still offends)
        if stuck.any():
            ch = param_grad(op, stuck.astype(np.float64), shape, groups) > 0
            beta = np.where(ch, beta + np.where(beta >= 0, 0.5, -0.5), beta).astype(np.float32)
    raise AssertionError(f"no ReLU case with a margin for {op} {shape} {name}")


def relu_margin_ok(op, shape, groups, X, gamma, beta, res, eps, K=K_RELU):
    ref = reference(X, canon_param(op, gamma, shape, groups), canon_param(op, beta, shape, groups), eps, True, res)
    return bool((np.abs(ref["pre"]) >= RELU_MARGIN * bound_y(ref, K)).all())


# ------------------------------------------------------------------------------------------------------------ kernel forms

class Case:
    """One shape of one kernel form.  ``slicing``: 'gn' (planes cut by gn_slice_len), 'bn3' (the channel cut every 16 384
    values), None (one partial per row).  ``fwd`` / ``bwd``: the forms of norm_restatement."""

    def __init__(self, id, kname, op, shape, groups=None, eps=1e-6, slicing=None, fwd="ab", bwd="coef", bn_mode=False,
                 dtypes=("f32",), relu=(False,), residual=False):
        self.id, self.kname, self.op, self.shape, self.groups, self.eps = id, kname, op, shape, groups, eps
        self.slicing, self.fwd, self.bwd, self.bn_mode, self.dtypes, self.relu, self.residual = slicing, fwd, bwd, bn_mode, dtypes, relu, residual

    @property
    def K(self):
        return globals()[self.kname]

    @property
    def running(self):
        return self.op in ("bn", "bnops")


_GN = dict(op="gn", slicing="gn", dtypes=("f32", "bf16"), relu=(False, True))
_GG = dict(op="gn", slicing=None, dtypes=("bf16",), relu=(False, True))   # single-pass group kernels: 16-bit x, hw % 512 == 0
_BN = dict(kname="K_BN_MODE", op="bn", slicing="gn", eps=1e-5, bn_mode=True, relu=(False, True))
_BO = dict(op="bnops", eps=1e-5, bwd="factored", relu=(False, True), residual=True)
CASES = [
    Case("gn_vector", "K_GN", shape=(2, 4, 8, 8), groups=2, residual=True, **_GN),
    Case("gn_flat", "K_GN", shape=(2, 4, 5, 5), groups=2, **_GN),             # hw % 4 != 0, total % 4 == 0
    Case("gn_scalar", "K_GN", shape=(1, 3, 5, 5), groups=1, **_GN),           # total % 4 != 0
    Case("gn_two_slices", "K_GN", shape=(1, 4, 132, 132), groups=2, **_GN),   # 17 424 -> 2 x 8 712
    Case("gn_two_slices_odd", "K_GN", shape=(1, 2, 131, 127), groups=1, **_GN),   # 16 637 -> 8 320 + 8 317
    Case("gn_group_nit1_cpg1", "K_GN_GROUP", shape=(2, 2, 16, 32), groups=2, **_GG),    # 64 vectors, one wave, one-channel groups
    Case("gn_group_nit1", "K_GN_GROUP", shape=(2, 4, 16, 32), groups=2, residual=True, **_GG),
    Case("gn_group_nit2", "K_GN_GROUP", shape=(2, 36, 16, 32), groups=2, **_GG),        # 1 152 vectors: the first count above 1 024
    Case("gn_group_nit4", "K_GN_GROUP", shape=(1, 72, 16, 32), groups=2, **_GG),        # 2 304 vectors: the first count above 2 048
    Case("bn_mode", shape=(3, 4, 8, 8), **_BN),
    Case("bn_mode_70_samples", shape=(70, 2, 8, 8), **_BN),           # more samples than merging lanes
    Case("bn_mode_sliced", shape=(2, 2, 132, 132), **_BN),
    Case("bnops_fused", "K_BN1", shape=(2, 4, 16, 16), **_BO),
    Case("bnops_wide", "K_BN1", shape=(5, 2, 64, 64), **_BO),                 # 20 480 values per channel
    Case("bnops_three_launch", "K_BN3", shape=(17, 2, 64, 64), slicing="bn3", **_BO),   # 69 632 values: 4 slices + one of 4 096
    Case("ln_256", "K_LN", op="rows", shape=(5, 256), fwd="centered", bwd="ln"),
    Case("ln_768", "K_LN", op="rows", shape=(5, 768), fwd="centered", bwd="ln"),
    Case("ln_1024", "K_LN", op="rows", shape=(5, 1024), fwd="centered", bwd="ln"),
    Case("ws_5x27", "K_WS", op="rows", shape=(5, 3, 3, 3), eps=1e-5, fwd="ws", bwd="factored"),
    Case("ws_8x64", "K_WS", op="rows", shape=(8, 64, 1, 1), eps=1e-5, fwd="ws", bwd="factored"),
    Case("ws_4x784", "K_WS", op="rows", shape=(4, 16, 7, 7), eps=1e-5, fwd="ws", bwd="factored"),
]
CASE = {c.id: c for c in CASES}
MOMENTUM = 0.1


def build_inputs(case, name, dtype="f32", relu=False, residual=False, seed=0):
    """Everything one run needs, canonical layout: X, g, res, radd (LayerNorm's residual gradient), gamma / beta in the
    operator's layout and broadcast (gc / bc), running statistics' starting values, and the float64 reference."""
    op, shape, groups = case.op, case.shape, case.groups
    cshape = canon_shape(op, shape, groups)
    if case.fwd == "ws":
        gamma, beta = params(1, seed, unit=True)
    elif relu:
        X, gamma, beta, res = build_relu_case(op, shape, groups, name, dtype, seed, case.eps, residual)
    else:
        gamma, beta = params(shape[1], seed)
    if not relu:
        X, _ = family(name, cshape, dtype, seed)
        res = np.random.default_rng(5 + seed).standard_normal(cshape).astype(np.float32) if residual else None
    gc, bc = canon_param(op, gamma, shape, groups), canon_param(op, beta, shape, groups)
    g = gradient(cshape, seed, dtype)
    rng = np.random.default_rng(31 + seed)
    inp = dict(X=X, g=g, res=res, gamma=gamma, beta=beta, gc=gc, bc=bc, relu=relu, dtype=dtype,
               radd=rng.standard_normal(cshape).astype(np.float32) if case.bwd == "ln" else None,
               ref=reference(X, gc, bc, case.eps, relu, res, g))
    if case.running:
        inp["rm0"] = (0.5 + 0.1 * rng.standard_normal(cshape[0])).astype(np.float32)
        inp["rv0"] = (2.0 + 0.1 * rng.standard_normal(cshape[0])).astype(np.float32)
        inp["rm64"], inp["rv64"] = running_reference(inp["ref"], inp["rm0"], inp["rv0"], MOMENTUM)
    return inp


def ratios(case, inp, out, u_y=U32, u_dx=U32, finite=True):
    """The K each result of ``out`` would need: every bound above is K A + B (B: the part without K, e.g. u_out |y64|), and the
    figure is max(0, |error| - B) / A, so ``figure <= K`` IS the bound.  ``out``: canonical layout, keys y, y_lp (the bf16 copy),
    mean, rstd, dx, dx_fused (LayerNorm with the residual gradient added), dgamma, dbeta, rm, rv.  Every result must be finite.
    -> dict name -> largest figure."""
    ref, op, shape, groups = inp["ref"], case.op, case.shape, case.groups
    f = {k: np.asarray(v, dtype=np.float64) for k, v in out.items() if v is not None}
    for k, v in f.items():
        assert not finite or np.isfinite(v).all(), f"{case.id}: {k} is not finite"

    def need(err, A, B):
        excess = np.maximum(np.where(np.isfinite(err), np.abs(err), np.inf) - B, 0.0)
        A = np.broadcast_to(A, excess.shape)
        return float(np.max(np.where(excess == 0, 0.0, excess / np.where(A > 0, A, 1e-300))))

    ay, adx = bound_y(ref, 1.0, 0.0), bound_dx(ref, 1.0, 0.0)
    want = {"y": (ref["y"], ay, u_y * np.abs(ref["y"])),
            "y_lp": (ref["y"], ay, U_BF16 * np.abs(ref["y"])),
            "mean": (ref["mean"], bound_mean(ref, 1.0), 0.0),
            "rstd": (ref["rstd"], bound_rstd_rel(ref, 1.0) * ref["rstd"], 0.0),
            "dx": (ref["dx"], adx, u_dx * np.abs(ref["dx"]))}
    if "dx_fused" in f:
        dxr = ref["dx"] + inp["radd"].astype(np.float64)
        want["dx_fused"] = (dxr, adx, u_dx * np.abs(dxr))
    if "dgamma" in f:
        want["dgamma"] = (param_grad(op, ref["tg"], shape, groups), U32 * param_grad(op, bound_dgamma_terms(ref), shape, groups), 0.0)
        want["dbeta"] = (param_grad(op, ref["tb"], shape, groups), U32 * param_grad(op, bound_dbeta_terms(ref), shape, groups), 0.0)
    if "rm" in f:
        brm, brv = bound_running(ref, inp["rm64"], inp["rv64"], MOMENTUM, 1.0)
        want["rm"] = (inp["rm64"], brm, 2 * U32 * np.abs(inp["rm64"]))
        want["rv"] = (inp["rv64"], brv, 2 * U32 * np.abs(inp["rv64"]))
    return {k: need(f[k] - w, A, B) for k, (w, A, B) in want.items() if k in f}


