"""Inputs, float64 references and error bounds shared by the loss-kernel tests (``test_loss_cases_cpu.py`` on the fp32
restatement of ``loss_restatement.py``, ``test_loss_cases_gpu.py`` on the kernels).  No GPU, numpy only (torch is used on the
CPU to round to bfloat16).

Three kernel families, every one a per-pixel softmax cross entropy with its own reduction:
  ce_dice      csrc/loss_ops.hip   0.5 CE + 0.5 Dice on z[B, C, HW], f32 / bf16 logits, C = 2..8
  upsample_ce  csrc/seg_ops.hip    bilinear upsample (align_corners) + log-softmax + NLL(ignore) + per-sample mean, C <= 32
  wce          csrc/doc_ufcn.hip   class-weighted CE, K <= 32

Labels.  ce_dice and wce define labels outside [0, C): no cross-entropy term, no weight, an all-zero one-hot row for the Dice
sums.  upsample_ce knows ONE ignore index and indexes a register array with every other label: its cases carry labels in
[0, C) and the ignore index 255 only -- any other value would be provoking a fault, not testing, and no case here has one.

Bounds.  u = 2^-24.  Every bound has the form  K A + B:  A is what fp32 evaluation of the kernel's expressions forces (at K = 1),
K one constant per family and quantity, and B the part that does not scale with K: the documented error of the device's
exponential and logarithm (the restatement's numpy routines are not the device's, so this part is NOT measured on the
restatement) and the rounding of the stored result.  ``figure = max(0, |error| - B) / A``, so ``figure <= K`` IS the bound.
Per pixel, with m = max_k z_k, d_k = z_k - m, s = sum_k exp(d_k), p_k = exp(d_k) / s, w = sum_k p_k |d_k|:
  nll   |nll - nll64| <= K u (|m| + log C + |z_l| + C + w)  +  E_log + E_exp
        (m + log s) - z_l is evaluated in fp32: the rounding of m + log s and of the subtraction scale with |m|, |z_l| and
        log s <= log C; s carries a relative u per addition (C - 1 of them, in class order: with the leading class first every
        later term is rounded on the grid of 1, which is why C and not 1 stands here: 'late' at 32 classes is
        the case) and the relative error of its terms (u (1 + |d_k|) each, weighted by p_k: the subtraction z_k - m and the
        product with log2(e) before the hardware's 2^x).
        E_log = 4 u log s: the device's log is documented at 1 ulp (the accurate logf of the device library; with this
        toolchain ``__logf`` IS ``__builtin_logf`` unless fast-math is on, and it is not), taken as 2 ulp.  It is relative
        to log s, so it vanishes where the loss does: what remains near s = 1 is the u of s itself, which is in the K part.
        E_exp = 4 u (s - 1) / s: the 2^x instruction / expf at 1 ulp (taken as 2) on every term of s but the leading one,
        exp(0) = 1, which both return exactly.  Like E_log it vanishes where the loss does: a log routine with an ABSOLUTE
        error of 2^-22 is a quarter of a 'late' loss of 1e-6 and has nowhere to hide.
  p     |p_k - p64_k| <= K u p64_k (C + |d_k| + w)  +  p64_k (4 u [d_k != 0] + E_exp) + TINY
        (TINY = 1e-37: results below the normal range; a gradient carries one TINY of its own for a stored result there)
  upsample_ce adds the fp32 bilinear sum of four corners: 4 u X_k on the interpolated logit of class k, X_k the largest of its
        four corner magnitudes at the pixel.  In nll it enters through m (X_m: the maximal class), through z_l (X_l) and through
        s weighted by p_k:  4 u (X_m + X_l + sum_k p_k X_k)  -- NOT the largest corner of any class: in 'late' the unlabelled
        classes sit at -16 with p_k ~ 1e-7 and must not buy the labelled class at 0 a bound larger than the loss.  In p_k:
        4 u p_k (X_k + 2 X_m + sum_j p_j X_j)  (d_k = z_k - m, and s through its own d_j).  The source indices and lambdas are
        NOT part of the error: see ``upsample_ce64``.
Sums (the CE mean, the Dice sums I_c = sum p t, P_c = sum p^2, the weighted sums of wce, a footprint of the upsample backward) get
the sum of the per-pixel bounds plus u n sum |term|, n the number of additions on the longest chain of the kernel's summation
order (``chain_*``).  The Dice value and the backward's constants get the propagated error of I, P (T is an exact count):
  dice_c = 1 - N / Dn, N = 2 I + s, Dn = P + T + s:   2 e_I / Dn + N e_P / Dn^2 + 4 u (1 + N / Dn)
  a_c = -2 / (C Dn):          |a_c| (e_P / Dn + 4 u)
  b_c = 2 N / (C Dn^2):       |b_c| (2 e_I / N + 2 e_P / Dn + 6 u)
so a class that is neither labelled nor predicted (Dn ~ 1e-5, b_c ~ 2e5 / C) is held to a RELATIVE bound on b_c of a few u.
The gradient bound is the first-order propagation of the bounds of p, a, b through
  dz_k = g [ 0.5 (p_k - t_k) / n_valid + 0.5 p_k (G_k - sum_c G_c p_c) ],  G_c = a_c t_c + b_c p_c   (``_grad_terms``)
plus u_out |dz64| for the stored result (2^-8 for bf16).  Near-zero losses (sat_right, late) are held to these ABSOLUTE bounds;
no bound here is relative to the loss value.
"""
import functools

import numpy as np

U32 = 2.0 ** -24
U_BF16 = 2.0 ** -8
SMOOTH = 1e-5
TINY = 1e-37
IGNORE = 255          # upsample_ce's ignore index
IGNORED_SAMPLE = 2    # ... and the sample that all_ignored blanks: NOT the one whose d(loss) is 0 (GLOSS)

# K = 4 x the largest figure of the fp32 restatement over every case of CASES (``python tests/test_loss_cases_cpu.py`` prints
# the table).  Measured on the CPU restatement against the float64 references, NOT on the device.
K_CD_CE = 0.72     # measured 0.179 (ce, shape a, C = 2, f32, late / ignored10)
K_CD_DICE = 0.68   # measured 0.170 (dice, shape a, C = 3, f32, randn3 / all_ignored); also holds the combined loss
K_CD_STATS = 3.47  # measured 0.869 (inv_valid, shape d, C = 2, bf16, randn3 / ignored10); also holds a_c, b_c
K_CD_GRAD = 4.81   # measured 1.203 (grad, shape a, C = 4, f32, wide / uniform)
K_UP_LOSS = 0.94   # measured 0.236 (loss, (3,3)->(19,27), C = 32, late / all_ignored)
K_UP_GRAD = 1.96   # measured 0.490 (grad, (6,6)->(6,6), C = 2, late / all_ignored)
K_WCE_LOSS = 1.29  # measured 0.323 (loss, P = 1, K = 2, late / uniform, random weights)
K_WCE_GRAD = 2.86  # measured 0.716 (grad, P = 2049, K = 5, late / uniform, no weights)
# A constant below 1 says that the restatement stays that far inside the worst case A assumes (every rounding at its limit and
# in the same direction); the device's own exponential and logarithm are not in these figures but in the B parts.

# which constant holds which result of ``ratios``
K_OF = {"ce_dice": dict(ce="K_CD_CE", dice="K_CD_DICE", loss="K_CD_DICE", a="K_CD_STATS", b="K_CD_STATS", inv_valid="K_CD_STATS",
                        grad="K_CD_GRAD"),
        "upsample_ce": dict(loss="K_UP_LOSS", grad="K_UP_GRAD"),
        "wce": dict(loss="K_WCE_LOSS", grad="K_WCE_GRAD")}


def K(family, key):
    return globals()[K_OF[family][key]]


def round_bf16(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).bfloat16().float().numpy()


# ------------------------------------------------------------------------------------------------------------ inputs

LOGITS = ("randn3", "offset_p60", "offset_m60", "sat_right", "sat_wrong", "late", "ties", "wide")
LABELS = ("uniform", "absent", "absent_unpredicted", "ignored10", "all_ignored")
LABEL_DEPENDENT = ("sat_right", "sat_wrong", "late")


def make_labels(name, rng, family, B, C, n):
    """labels int64 [B, n].
    uniform             every class
    absent              class C - 1 never labelled (C = 1: the same as uniform)
    absent_unpredicted  the same labels; ``make_logits`` puts class C - 1 another 40 below the lowest other class everywhere
    ignored10           10 % replaced: -100 and C in turn (ce_dice, wce), 255 (upsample_ce); at least 80 % stay valid and at least
                        one is replaced.  Sizes below 10 labels are exempt from the 80 %: exactly one of 2..9 labels is replaced,
                        a single label is not
    all_ignored         ce_dice, wce: every label of the batch out of range; upsample_ce: sample IGNORED_SAMPLE entirely 255"""
    hi = C - 1 if (name in ("absent", "absent_unpredicted") and C > 1) else C
    lab = rng.integers(0, hi, size=(B, n)).astype(np.int64)
    out_of_range = np.where(np.arange(B * n).reshape(B, n) % 2 == 0, -100, C) if family != "upsample_ce" else np.full((B, n), IGNORE)
    if name == "ignored10":
        if B * n >= 10:
            lab = np.where(rng.random((B, n)) < 0.1, out_of_range, lab)
            if not (lab == out_of_range).any():
                lab[0, 0] = out_of_range[0, 0]
        elif B * n >= 2:
            lab[-1, -1] = out_of_range[-1, -1]      # fewer than 10 labels: exactly one replaced (75 % valid of 4) ...
        # ... and a single label stays valid: the case is then the uniform one (all labels out of range is all_ignored's)
    elif name == "all_ignored":
        if family == "upsample_ce":
            lab[min(IGNORED_SAMPLE, B - 1)] = IGNORE
        else:
            lab = out_of_range.astype(np.int64)
    return lab.astype(np.int64)


def make_logits(name, rng, shape, labels):
    """float32 [B, C, n]; ``labels`` [B, n] gives the 'labelled class' of the label-dependent families (an out-of-range label
    counts as its value modulo C there).
    randn3      3 randn: the baseline of the earlier tests
    offset_p60  randn + 60 on every class of a pixel  (float64: the same softmax; fp32: needs the max-subtraction to be right)
    offset_m60  randn - 60
    sat_right   the labelled class leads the best other class by 25..35: NLL ~ 1e-11..1e-15, loss ~ 0
    sat_wrong   the labelled class trails the worst other class by 25..35: NLL ~ 30, gradient on the label ~ -1
    late        labelled class at 0, the others at -(12..16) - log(C - 1): NLL in [1e-7, 1e-5], log evaluated next to 1; the
                labelled logit and the maximum are 0, so nothing but s, log and the sums decides the answer
    ties        all classes equal at a pixel: p = 1 / C exactly
    wide        uniform in [-100, 100]: exp(z - m) underflows to denormals and to 0"""
    B, C, n = shape
    z = rng.standard_normal(shape)
    lab = np.mod(labels, C)[:, None, :]
    hit = lab == np.arange(C)[None, :, None]
    if name == "randn3":
        z = 3.0 * z
    elif name == "offset_p60":
        z = z + 60.0
    elif name == "offset_m60":
        z = z - 60.0
    elif name in ("sat_right", "sat_wrong"):
        z = rng.uniform(-1.0, 1.0, size=shape)
        gap = rng.uniform(25.0, 35.0, size=(B, 1, n))
        if name == "sat_right":
            z = np.where(hit, np.where(hit, -np.inf, z).max(axis=1, keepdims=True) + gap if C > 1 else z, z)
        else:
            z = np.where(hit, np.where(hit, np.inf, z).min(axis=1, keepdims=True) - gap if C > 1 else z, z)
    elif name == "late":
        z = np.where(hit, 0.0, -(rng.uniform(12.0, 16.0, size=shape) + np.log(max(C - 1, 1))))
    elif name == "ties":
        z = np.broadcast_to(z[:, :1, :], shape).copy()
    elif name == "wide":
        z = rng.uniform(-100.0, 100.0, size=shape)
    else:
        raise KeyError(name)
    return np.ascontiguousarray(z, dtype=np.float32)


def push_down_last_class(z):
    """absent_unpredicted: class C - 1 another 40 below the lowest other class of every pixel."""
    z = z.copy()
    if z.shape[1] > 1:
        z[:, -1, :] = z[:, :-1, :].min(axis=1) - 40.0
    return z


# ------------------------------------------------------------------------------------------------------------ per-pixel pieces

def softmax64(z):
    """z float64 [B, C, n] -> m, s, logs [B, n], d, p [B, C, n], w = sum_k p_k |d_k| [B, n]."""
    m = z.max(axis=1)
    d = z - m[:, None, :]
    e = np.exp(d)
    s = e.sum(axis=1)
    p = e / s[:, None, :]
    return dict(m=m, d=d, s=s, logs=np.log(s), p=p, w=(p * np.abs(d)).sum(axis=1))


def pixel_bounds(sp, zl, C, X=None, t=None):
    """(A_nll, B_nll) [B, n], (A_p, B_p) [B, C, n] at K = 1 (module docstring); X [B, C, n], t [B, C, n]: upsample_ce's corner
    magnitudes per class and its one-hot labels."""
    p = sp["p"]
    e_s = 4 * U32 * (sp["s"] - 1.0) / sp["s"]      # the exponential's error on s, relative: the leading term exp(0) = 1 is exact
    A_nll = U32 * (np.abs(sp["m"]) + np.log(C) + np.abs(zl) + C + sp["w"])
    B_nll = 4 * U32 * sp["logs"] + e_s
    A_p = U32 * p * (C + np.abs(sp["d"]) + sp["w"][:, None, :])
    B_p = p * (4 * U32 * (sp["d"] != 0) + e_s[:, None, :]) + TINY
    if X is not None:
        Xm = np.where(sp["d"] > -1e-4, X, 0.0).max(axis=1)  # the maximal class (any class within 1e-4 of it may be fp32's)
        Xl = (X * t).sum(axis=1)                            # the labelled class
        Xp = (X * p).sum(axis=1)                            # the others, through s
        A_nll = A_nll + 4 * U32 * (Xm + Xl + Xp)
        A_p = A_p + 4 * U32 * p * (X + (2 * Xm + Xp)[:, None, :])
    return A_nll, B_nll, A_p, B_p


def need(err, A, B):
    """The K this error needs: max(0, |err| - B) / A, inf where a non-finite error or an error with A = 0 exceeds B."""
    err = np.asarray(err, dtype=np.float64)
    excess = np.maximum(np.where(np.isfinite(err), np.abs(err), np.inf) - B, 0.0)
    A = np.broadcast_to(np.asarray(A, dtype=np.float64), excess.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.max(np.where(excess == 0, 0.0, excess / np.where(A > 0, A, 1e-300)), initial=0.0))


# ------------------------------------------------------------------------------------------------------------ ce_dice

def chain_ce_dice(B, hw):
    """Additions on the longest chain of ce_dice_fwd / finish: 4 per quad and pass of a thread, 6 butterfly steps, 2 over the
    waves, ceil(blocks / 32) rows of a finish range, 32 ranges."""
    quads = B * (hw // 4)
    blocks = min((quads + 255) // 256, 512)
    passes = -(-quads // (blocks * 256))
    return 4 * passes + 6 + 2 + -(-blocks // 32) + 32


def ce_dice_ref(z, labels):
    """Float64 reference of csrc/loss_ops.hip with everything the bounds need.  z [B, C, n], labels [B, n]."""
    z = np.asarray(z, dtype=np.float64)
    B, C, n = z.shape
    sp = softmax64(z)
    p = sp["p"]
    valid = (labels >= 0) & (labels < C)
    t = (labels[:, None, :] == np.arange(C)[None, :, None]).astype(np.float64)   # out of range: a zero row
    zl = (z * t).sum(axis=1)
    nll = np.where(valid, (sp["m"] + sp["logs"]) - zl, 0.0)
    nv = int(valid.sum())
    inv = 1.0 / nv if nv else 0.0
    ce = nll.sum() * inv
    I, P, T = (p * t).sum(axis=(0, 2)), (p * p).sum(axis=(0, 2)), t.sum(axis=(0, 2))
    N, Dn = 2 * I + SMOOTH, P + T + SMOOTH
    dice_c = 1.0 - N / Dn
    dice = dice_c.mean()
    a, b = -2.0 / (C * Dn), 2.0 * N / (C * Dn * Dn)
    G = a[None, :, None] * t + b[None, :, None] * p
    dot = (G * p).sum(axis=1, keepdims=True)
    dz = 0.5 * (p - t) * valid[:, None, :] * inv + 0.5 * p * (G - dot)
    return dict(sp=sp, p=p, t=t, zl=zl, valid=valid, nll=nll, nv=nv, inv_valid=inv, ce=ce, dice=dice, dice_c=dice_c, loss=0.5 * ce + 0.5 * dice,
                I=I, P=P, T=T, N=N, Dn=Dn, a=a, b=b, G=G, dot=dot, dz=dz, C=C, B=B, n=n)


def ce_dice64(z, labels):
    """-> (loss, ce, dice, dz) in float64, the semantics of the header of csrc/loss_ops.hip: CE is the mean over the labels in
    [0, C) (0 when there are none), Dice per class 1 - (2 I + s) / (P + T + s), s = 1e-5, sums over the whole batch, mean over
    the classes; labels outside the range give a zero one-hot row; dz the analytic gradient of loss = 0.5 ce + 0.5 dice."""
    r = ce_dice_ref(z, labels)
    return r["loss"], r["ce"], r["dice"], r["dz"]


def _grad_terms(r, ep, ea, eb, uu):
    """First-order propagation of the bounds ep [B, C, n] of p, ea / eb [C] of a / b through the gradient at g = 1."""
    p, t, G, dot, C = r["p"], r["t"], r["G"], r["dot"], r["C"]
    ea, eb, bb = ea[None, :, None], eb[None, :, None], np.abs(r["b"])[None, :, None]
    dG = t * ea + bb * ep + p * eb + uu * 2 * np.abs(G)
    ddot = (np.abs(G) * ep + p * dG).sum(axis=1, keepdims=True) + uu * (C + 1) * np.abs(G * p).sum(axis=1, keepdims=True)
    dd = ep * np.abs(G - dot) + p * (dG + ddot) + uu * 3 * p * (np.abs(G) + np.abs(dot))
    dce = r["valid"][:, None, :] * r["inv_valid"] * (ep + uu * 3 * np.abs(p - t))
    return 0.5 * (dce + dd) + uu * 2 * np.abs(r["dz"])


def ce_dice_bounds(r, g=1.0, u_out=U32):
    """name -> (reference, A, B)."""
    C, chain = r["C"], chain_ce_dice(r["B"], r["n"])
    A_nll, B_nll, A_p, B_p = pixel_bounds(r["sp"], r["zl"], C)
    v, inv, t, p = r["valid"], r["inv_valid"], r["t"], r["p"]
    A_ce = (A_nll * v).sum() * inv + U32 * chain * np.abs(r["nll"]).sum() * inv + 2 * U32 * abs(r["ce"])
    B_ce = (B_nll * v).sum() * inv
    A_I = (t * A_p).sum(axis=(0, 2)) + U32 * chain * r["I"]
    B_I = (t * B_p).sum(axis=(0, 2))
    A_P = (2 * p * A_p).sum(axis=(0, 2)) + U32 * (chain + 1) * r["P"]
    B_P = (2 * p * B_p).sum(axis=(0, 2))
    N, Dn = r["N"], r["Dn"]
    A_dc = 2 * A_I / Dn + N * A_P / Dn ** 2 + 4 * U32 * (1 + N / Dn)
    B_dc = 2 * B_I / Dn + N * B_P / Dn ** 2
    A_dice = A_dc.mean() + U32 * C * np.abs(r["dice_c"]).mean()
    B_dice = B_dc.mean()
    A_a, B_a = np.abs(r["a"]) * (A_P / Dn + 4 * U32), np.abs(r["a"]) * B_P / Dn
    A_b, B_b = np.abs(r["b"]) * (2 * A_I / N + 2 * A_P / Dn + 6 * U32), np.abs(r["b"]) * (2 * B_I / N + 2 * B_P / Dn)
    A_g = abs(g) * _grad_terms(r, A_p, A_a, A_b, U32)
    B_g = abs(g) * _grad_terms(r, B_p, B_a, B_b, 0.0) + u_out * np.abs(g * r["dz"]) + TINY
    return dict(ce=(r["ce"], A_ce, B_ce), dice=(r["dice"], A_dice, B_dice),
                loss=(r["loss"], 0.5 * A_ce + 0.5 * A_dice + 2 * U32 * abs(r["loss"]), 0.5 * B_ce + 0.5 * B_dice),
                inv_valid=(r["inv_valid"], U32 * r["inv_valid"], 0.0), a=(r["a"], A_a, B_a), b=(r["b"], A_b, B_b),
                grad=(g * r["dz"], A_g, B_g))


# ------------------------------------------------------------------------------------------------------------ upsample_ce

def lerp_tables(n_in, n_out, fused=False):
    """The float32 source-index rule of ``lerp_index`` (csrc/seg_ops.hip) = PyTorch's align_corners=True rule:
    scale = (in - 1) / (out - 1) in float32 (0 when out = 1), src = scale * dst in float32, i0 = (int) src clamped to in - 1,
    i1 = i0 + (i0 < in - 1), l1 = src - i0, l0 = 1 - l1, both float32.  -> i0, i1 (int), l0, l1 (float32), scale (float32).
    ``fused`` (loss_restatement's fault lerp_lambda_fused): l1 = fma(scale, dst, -i0), the lambda of the UNROUNDED product next
    to the i0 of the rounded one."""
    f = np.float32
    scale = f(n_in - 1) / f(n_out - 1) if n_out > 1 else f(0)
    src = (scale * np.arange(n_out, dtype=np.float32)).astype(np.float32)
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    l1 = (src - i0.astype(np.float32)).astype(np.float32)
    if fused:
        l1 = (np.float64(scale) * np.arange(n_out, dtype=np.float64) - i0).astype(np.float32)
    l0 = (f(1) - l1).astype(np.float32)
    return i0, i1, l0, l1, scale


def lerp_matrix(n_in, n_out):
    """[out, in] float64 matrix holding the float32 lambdas (both land on the same entry where i1 = i0)."""
    i0, i1, l0, l1, _ = lerp_tables(n_in, n_out)
    M = np.zeros((n_out, n_in))
    np.add.at(M, (np.arange(n_out), i0), l0.astype(np.float64))
    np.add.at(M, (np.arange(n_out), i1), l1.astype(np.float64))
    return M


def upsample_ce_ref(x, labels, size, ignore, gloss):
    x = np.asarray(x, dtype=np.float64)
    B, C, h, w = x.shape
    H, W = size
    My, Mx = lerp_matrix(h, H), lerp_matrix(w, W)
    v = np.einsum("Yi,bcij,Xj->bcYX", My, x, Mx).reshape(B, C, H * W)
    ax = np.abs(x)
    (y0, y1, _, _, _), (x0, x1, _, _, _) = lerp_tables(h, H), lerp_tables(w, W)
    X = np.maximum(np.maximum(ax[:, :, y0[:, None], x0[None, :]], ax[:, :, y0[:, None], x1[None, :]]),        # per class: [B, C, H W]
                   np.maximum(ax[:, :, y1[:, None], x0[None, :]], ax[:, :, y1[:, None], x1[None, :]])).reshape(B, C, H * W)
    lab = labels.reshape(B, H * W)
    valid = lab != ignore
    sp = softmax64(v)
    t = ((lab[:, None, :] == np.arange(C)[None, :, None]) & valid[:, None, :]).astype(np.float64)
    zl = (v * t).sum(axis=1)
    nll = np.where(valid, (sp["m"] + sp["logs"]) - zl, 0.0)
    npix = H * W
    loss = nll.sum(axis=1) / npix
    gl = np.asarray(gloss, dtype=np.float64)
    gv = (sp["p"] - t) * valid[:, None, :]
    dx = np.einsum("Yi,bcYX,Xj->bcij", My, gv.reshape(B, C, H, W), Mx) * (gl / npix)[:, None, None, None]
    return dict(sp=sp, v=v, X=X, t=t, zl=zl, valid=valid, nll=nll, loss=loss, dx=dx, gv=gv, My=My, Mx=Mx, gl=gl, C=C, B=B, h=h, w=w, H=H, W=W)


def upsample_ce64(x, labels, size, ignore, gloss):
    """-> (loss [B], dx [B, C, h, w]) in float64: bilinear upsampling of x [B, C, h, w] to ``size`` (align_corners=True),
    log-softmax, NLL with one ignore index, the mean over ALL H W pixels of a sample (ignored ones count as 0, as
    nll_loss(reduction='none').mean does), and the gradient for d(loss[b]) = gloss[b].
    The source indices and lambdas are computed in FLOAT32 exactly as ``lerp_index`` and PyTorch's align_corners=True rule do
    (``lerp_tables``); everything after them is float64.  That float32 index step is part of the operator's definition, not an
    error of the kernel: PyTorch's own float32 kernel takes the same step, and a float64 index would move every lambda by ~u."""
    r = upsample_ce_ref(x, labels, size, ignore, gloss)
    return r["loss"], r["dx"]


def chain_upsample_fwd(H, W):
    npix = H * W
    bps = min(-(-npix // 1024), 256)
    return -(-npix // (bps * 256)) + 6 + 2 + -(-bps // 64) + 6


def upsample_ce_bounds(r):
    C, npix = r["C"], r["H"] * r["W"]
    A_nll, B_nll, A_p, B_p = pixel_bounds(r["sp"], r["zl"], C, r["X"], r["t"])
    v = r["valid"]
    chain = chain_upsample_fwd(r["H"], r["W"])
    A_loss = ((A_nll * v).sum(axis=1) + U32 * chain * np.abs(r["nll"]).sum(axis=1)) / npix + 2 * U32 * np.abs(r["loss"])
    B_loss = (B_nll * v).sum(axis=1) / npix
    B_, H, W, My, Mx = r["B"], r["H"], r["W"], r["My"], r["Mx"]
    sc = (np.abs(r["gl"]) / npix)[:, None, None, None]

    def scatter(q):   # per-pixel [B, C, npix] -> per-cell [B, C, h, w] through the footprint weights
        return np.einsum("Yi,bcYX,Xj->bcij", My, q.reshape(B_, -1, H, W), Mx)

    count = np.einsum("Yi,Xj->ij", (My > 0).astype(np.float64), (Mx > 0).astype(np.float64))   # pixels of a footprint
    vv = v[:, None, :]
    absgv = np.abs(r["gv"])
    A_dx = sc * (scatter(A_p * vv + 3 * U32 * absgv) + U32 * (count + 4)[None, None] * scatter(absgv)) + 3 * U32 * np.abs(r["dx"])
    B_dx = sc * scatter(B_p * vv) + TINY
    return dict(loss=(r["loss"], A_loss, B_loss), grad=(r["dx"], A_dx, B_dx))


# ------------------------------------------------------------------------------------------------------------ wce

def chain_wce(P):
    per = -(-P // 256)
    return -(-per // 256) + 6 + 2 + 256


def wce_ref(z, labels, weight, g=1.0):
    z = np.asarray(z, dtype=np.float64)
    B, C, n = z.shape
    wt = np.ones(C) if weight is None else np.asarray(weight, dtype=np.float64)
    valid = (labels >= 0) & (labels < C)
    t = (labels[:, None, :] == np.arange(C)[None, :, None]).astype(np.float64)
    wy = (t * wt[None, :, None]).sum(axis=1)      # 0 for out-of-range labels
    sp = softmax64(z)
    zl = (z * t).sum(axis=1)
    nll = np.where(valid, (sp["m"] + sp["logs"]) - zl, 0.0)
    Wsum = wy.sum()
    with np.errstate(divide="ignore", invalid="ignore"):
        loss = (wy * nll).sum() / Wsum
        dz = g * wy[:, None, :] * (sp["p"] - t) / Wsum if Wsum > 0 else np.zeros_like(z)
    return dict(sp=sp, t=t, wy=wy, zl=zl, valid=valid, nll=nll, Wsum=Wsum, loss=loss, dz=dz, C=C, B=B, n=n, g=g)


def wce64(z, labels, weight, g=1.0):
    """-> (loss, dz) in float64: sum w_y nll / sum w_y over the labels in [0, K) (weight None: all ones); out-of-range labels
    carry no weight and get a zero gradient.  With no weight at all the loss is 0 / 0 (nan) and dz is zero."""
    r = wce_ref(z, labels, weight, g)
    return r["loss"], r["dz"]


def wce_bounds(r):
    C, Wsum, wy, g = r["C"], r["Wsum"], r["wy"], r["g"]
    if Wsum == 0:   # no weight at all: the loss is 0 / 0 and not asserted, the gradient is exactly zero
        return dict(grad=(r["dz"], 0.0, 0.0))
    chain = chain_wce(r["B"] * r["n"])
    A_nll, B_nll, A_p, B_p = pixel_bounds(r["sp"], r["zl"], C)
    A_N = (wy * A_nll).sum() + U32 * chain * (wy * np.abs(r["nll"])).sum()
    A_W = U32 * chain * Wsum
    A_loss = A_N / Wsum + abs(r["loss"]) * A_W / Wsum + 2 * U32 * abs(r["loss"])
    B_loss = (wy * B_nll).sum() / Wsum
    k = abs(g) * wy[:, None, :] / Wsum
    A_g = k * (A_p + 3 * U32 * np.abs(r["sp"]["p"] - r["t"])) + np.abs(r["dz"]) * (A_W / Wsum + 3 * U32)
    B_g = k * B_p + TINY
    return dict(loss=(r["loss"], A_loss, B_loss), grad=(r["dz"], A_g, B_g))


# ------------------------------------------------------------------------------------------------------------ cases

class Case:
    """One input of one family.  ``geom``: ce_dice (B, hw); upsample_ce ((h, w), (H, W)); wce (B, HW).  ``weight``: wce only,
    None / 'random' / 'zero_class' (class 0 at weight 0, and class 0 is labelled)."""

    def __init__(self, family, shape_id, C, geom, logits, labels, dtype="f32", weight=None):
        self.family, self.shape_id, self.C, self.geom, self.logits, self.labels, self.dtype, self.weight = \
            family, shape_id, C, geom, logits, labels, dtype, weight
        self.id = f"{family}-{shape_id}-C{C}-{dtype}-{logits}-{labels}" + (f"-w_{weight}" if family == "wce" else "")

    def __repr__(self):
        return self.id


# every logits family on plain and on 10 %-ignored labels, every label family on the baseline logits
COMBOS = [(lg, lb) for lg in LOGITS for lb in ("uniform", "ignored10")] + [("randn3", lb) for lb in ("absent", "absent_unpredicted", "all_ignored")]
BIG_COMBOS = [("randn3", "ignored10"), ("late", "uniform")]

CE_DICE_SHAPES = {
    "a": (1, 4),               # one quad, one thread
    "b": (3, 400),             # 300 quads: a ragged second workgroup
    "c": (5, 4 * 3277),        # 16 385 quads -> 65 workgroups: finish ranges of 3 rows, the last used range short, the rest empty
    "d": (11, 4 * 11939),      # 131 329 quads > 512 x 256, no multiple of 256: the grid-stride loop with a ragged second pass
}
GLOSS = (1.5, 0.0, -2.0)       # upsample_ce, B = 3
UPSAMPLE_GEOMS = {
    "row": ((1, 5), (1, 40)),          # h = 1: the y axis degenerate (scale 0)
    "col": ((5, 1), (33, 1)),          # w = 1
    "up": ((7, 9), (40, 33)),          # plain upsampling, different scales per axis
    "down": ((9, 7), (4, 3)),          # H < h: scale > 1, the other branch of the footprint arithmetic; cells nobody reads
    "identity": ((6, 6), (6, 6)),      # scale 1: every lambda 0
    "nine_cells": ((3, 3), (19, 27)),  # h w = 9: 7 idle lane groups shadow the last cell
    "two_groups": ((17, 16), (33, 31)),  # 272 cells = 17 workgroups of 16 cells; 1 023 pixels
}
UPSAMPLE_C = (1, 2, 21, 32)
WCE_GEOMS = {
    "one": (1, 1),             # P = 1
    "p255": (1, 255),          # P < 256: one pixel per block, the last block empty
    "p258": (2, 129),          # per = 2: the second image starts in the middle of a block's range
    "p2049": (3, 683),         # per = 9, the last block short (2 049 = 227 x 9 + 6), blocks 228..255 empty
}
WCE_K = (1, 2, 5, 32)
WCE_WEIGHTS = (None, "random", "zero_class")


def _cases():
    out = []
    for C in range(2, 9):
        for dtype in ("f32", "bf16"):
            for sid in ("a", "b"):
                out += [Case("ce_dice", sid, C, CE_DICE_SHAPES[sid], lg, lb, dtype) for lg, lb in COMBOS]
            if C in (2, 8):
                out += [Case("ce_dice", "c", C, CE_DICE_SHAPES["c"], lg, lb, dtype) for lg, lb in BIG_COMBOS]
                out += [Case("ce_dice", "d", C, CE_DICE_SHAPES["d"], *BIG_COMBOS[0], dtype)]
    for gid, geom in UPSAMPLE_GEOMS.items():
        for C in UPSAMPLE_C:
            combos = COMBOS if (gid == "up" and C in (2, 21)) else [("randn3", "ignored10"), ("late", "all_ignored"), ("wide", "uniform")]
            out += [Case("upsample_ce", gid, C, geom, lg, lb) for lg, lb in combos if lb not in ("absent", "absent_unpredicted")]
    for gid, geom in WCE_GEOMS.items():
        for C in WCE_K:
            for wt in WCE_WEIGHTS:
                if wt == "zero_class" and (C == 1 or gid == "one"):
                    continue   # the only class / the only pixel at weight 0: no weight at all, 0 / 0 (see test_loss_cases_gpu.py)
                combos = COMBOS if (gid == "p2049" and C == 5 and wt == "random") else [("randn3", "ignored10"), ("late", "uniform"), ("wide", "uniform")]
                out += [Case("wce", gid, C, geom, lg, lb, weight=wt) for lg, lb in combos if lb != "absent_unpredicted"]
    return out


CASES = _cases()
CASE = {c.id: c for c in CASES}


def _seed(case):
    import zlib
    return zlib.crc32(case.id.encode())


def _build(case):
    rng = np.random.default_rng(_seed(case))
    fam, C = case.family, case.C
    if fam == "upsample_ce":
        (h, w), (H, W) = case.geom
        B = len(GLOSS)
        labels = make_labels("uniform" if case.labels == "all_ignored" else case.labels, rng, fam, B, C, H * W)
        low = None
        if case.logits in LABEL_DEPENDENT:
            # bilinear blends of cells with different leading classes are not 'late' or 'saturated': every sample gets ONE class
            # (ignored pixels are laid over it afterwards)
            one = (np.arange(B) % C)[:, None]
            labels = np.where(labels == IGNORE, IGNORE, one)
            low = np.broadcast_to(one, (B, h * w))
        if case.labels == "all_ignored":
            labels = labels.copy()
            labels[IGNORED_SAMPLE] = IGNORE
        x = make_logits(case.logits, rng, (B, C, h * w), low if low is not None else rng.integers(0, C, size=(B, h * w))).reshape(B, C, h, w)
        labels = np.ascontiguousarray(labels.reshape(B, H, W), dtype=np.int64)
        gl = np.asarray(GLOSS, dtype=np.float32)
        return dict(x=x, labels=labels, size=(H, W), gloss=gl, ref=upsample_ce_ref(x, labels, (H, W), IGNORE, gl))
    B, n = case.geom
    labels = make_labels(case.labels, rng, fam, B, C, n)
    weight = None
    if case.weight is not None:
        weight = rng.uniform(0.25, 4.0, size=C).astype(np.float32)
        if case.weight == "zero_class":
            weight[0] = 0.0
            labels[0, 0] = 0     # ... and class 0 IS labelled
    z = make_logits(case.logits, rng, (B, C, n), labels)
    if case.labels == "absent_unpredicted":
        z = push_down_last_class(z)
    if case.dtype == "bf16":
        z = round_bf16(z)
    if fam == "ce_dice":
        return dict(z=z, labels=labels, ref=ce_dice_ref(z, labels))
    g = -0.75
    return dict(z=z, labels=labels, weight=weight, g=g, ref=wce_ref(z, labels, weight, g))


@functools.lru_cache(maxsize=2)
def _build_cached(case_id):
    return _build(CASE[case_id])


def build(case):
    """The inputs and the float64 reference of a case (the last few are kept: the large ones are computed once per module)."""
    return _build_cached(case.id)


def ratios(case, inp, out):
    """name -> the K each result of ``out`` needs (``need``).  out: ce_dice: loss, ce, dice, inv_valid, a, b, and grad as a dict
    {g: gradient for d(loss) = g} (the bounds are computed once, at g = 1, and scale with |g|; the figure is the largest);
    upsample_ce / wce: loss, grad.  Keys that are absent are skipped."""
    r = inp["ref"]
    if case.family == "ce_dice":
        want = ce_dice_bounds(r, 1.0, U_BF16 if case.dtype == "bf16" else U32)
    elif case.family == "upsample_ce":
        want = upsample_ce_bounds(r)
    else:
        want = wce_bounds(r)
    res = {}
    for k, (ref, A, B) in want.items():
        if k not in out or out[k] is None:
            continue
        if isinstance(out[k], dict):
            res[k] = max(need(np.asarray(v, dtype=np.float64).reshape(np.shape(ref)) - g * ref, abs(g) * A, abs(g) * B + TINY)
                         for g, v in out[k].items())
        else:
            res[k] = need(np.asarray(out[k], dtype=np.float64).reshape(np.shape(ref)) - ref, A, B)
    return res
