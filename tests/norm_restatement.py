"""fp32 numpy restatement of the normalisation kernels (csrc/group_norm.hip, bn_ops.hip, layer_norm.hip, weight_std.hip) in the
kernels' own order of operations, on the canonical layout of ``norm_statistics_cases`` (X [R, U, L]: rows, units, elements):

  statistics  per (unit, slice) the two-pass (count, mean, M2) in fp32; Chan's merge of the partials in (unit, slice) order --
              (channel, slice) for GroupNorm, (sample, slice) for the batch-norm mode; ``sl`` = the slice length inside a unit
              (``gn_slice_len``), None = the whole row as one partial (single-pass group / fused / wide / row kernels);
  apply       'ab'        y = x a + b,  a = rstd gamma,  b = beta - mean a            (gn_apply_kernel, bn_chan_finish_wave, bn_ops)
              'centered'  y = (x - mean) rstd gamma + beta                           (ln_fwd_kernel)
              'ws'        y = (x - mean) / sqrt(var + eps), invstd = 1 / sqrt(..)     (weight_std_fwd_kernel)
  backward    'coef'      dx = k1 g' - k2 - k3 xhat  (gn_bwd_row; ``bn_mode``: k2 = k1 s1 / n as bn_bwd_chan_wave)
              'factored'  dx = k (g' - m1 - xhat m2)                                   (bn_ops, weight_std)
              'ln'        dx = rstd (g gamma - m1 - xhat m2) (+ residual gradient)     (ln_bwd_kernel)

What is NOT restated: the order of the sums INSIDE one partial (a workgroup's tree; numpy's pairwise fp32 sum stands in) and the
contraction of x a + b into one fused multiply-add.  Both stay inside the bounds' K.

``defect`` swaps in one deliberately wrong step (the defect-separation test): 'one_pass', 'no_cross', 'cross_nb_nt',
'unweighted_mean', 'eps_outside', 'biased_running', 'count_sl'."""
import numpy as np

f32 = np.float32

GN_SLICE = 16384
BN_SLICE = 16384


def gn_slices(hw):
    return (hw + GN_SLICE - 1) // GN_SLICE


def gn_slice_len(hw):
    s = gn_slices(hw)
    return (((hw + s - 1) // s) + 3) & ~3


def _segments(U, L, sl):
    if sl is None:
        return [(None, 0, U * L)]
    return [(u, lo, min(L, lo + sl)) for u in range(U) for lo in range(0, L, sl)]


def _seg(X, u, lo, hi):
    return X.reshape(X.shape[0], -1)[:, lo:hi] if u is None else X[:, u, lo:hi]


def statistics(X, eps, sl=None, defect=None):
    """-> (mean, rstd, m2, n) float32 [R] (n: the merged count)."""
    R, U, L = X.shape
    parts = []
    for u, lo, hi in _segments(U, L, sl):
        seg = _seg(X, u, lo, hi)
        cnt = f32(sl if (defect == "count_sl" and sl is not None) else hi - lo)
        s = seg.sum(axis=1, dtype=f32)
        mean = s / cnt
        if defect == "one_pass":
            m2 = (seg * seg).sum(axis=1, dtype=f32) - cnt * mean * mean
        else:
            d = seg - mean[:, None]
            m2 = (d * d).sum(axis=1, dtype=f32)
        parts.append((cnt, mean, m2))
    n, mean, m2 = f32(0), np.zeros(R, f32), np.zeros(R, f32)
    for nb, mb, m2b in parts:
        nt = f32(n + nb)
        delta = mb - mean
        mean = mean + delta * f32(nb / nt)
        if defect == "no_cross":
            m2 = m2 + m2b
        elif defect == "cross_nb_nt":
            m2 = m2 + (m2b + delta * delta * f32(nb / nt))
        else:
            m2 = m2 + (m2b + delta * delta * f32(f32(n * nb) / nt))
        n = nt
    if defect == "unweighted_mean":
        mean = np.stack([p[1] for p in parts]).sum(axis=0, dtype=f32) / f32(len(parts))
    var = m2 / n
    rstd = f32(1) / (np.sqrt(var) + f32(eps)) if defect == "eps_outside" else f32(1) / np.sqrt(var + f32(eps))
    return mean.astype(f32), rstd.astype(f32), m2.astype(f32), n


def running_update(mean, m2, n, rm0, rv0, momentum, defect=None):
    mom = f32(momentum)
    unb = m2 / n if (defect == "biased_running" or n <= 1) else m2 / f32(n - f32(1))
    return (f32(1) - mom) * rm0 + mom * mean, (f32(1) - mom) * rv0 + mom * unb


def forward(X, gamma, beta, eps, sl=None, form="ab", relu=False, res=None, defect=None):
    """-> dict mean, rstd, m2, n, y (fp32, before any rounding to a 16-bit output)."""
    X = X.astype(f32)
    mean, rstd, m2, n = statistics(X, eps, sl, defect)
    mc, rc = mean[:, None, None], rstd[:, None, None]
    if form == "ab":
        a = rc * gamma
        b = beta - mc * a
        y = X * a + b
    elif form == "centered":
        y = (X - mc) * rc * gamma + beta
    else:  # 'ws'
        sd = np.sqrt(m2 / n + f32(eps))
        rstd = (f32(1) / sd).astype(f32)
        y = (X - mc) / sd[:, None, None]
    if res is not None:
        y = y + res
    if relu:
        y = np.maximum(y, f32(0))
    assert y.dtype == f32
    return dict(mean=mean, rstd=rstd, m2=m2, n=n, y=y)


def backward(X, g, mean, rstd, gamma, beta, sl=None, form="coef", relu=False, y=None, bn_mode=False, radd=None):
    """``y``: the saved output whose sign is the ReLU gate (None: the gate is recomputed as xhat gamma + beta > 0, GroupNorm
    without a residual).  -> dict dx, sg / sgx [R, U] (per-unit sums of g' and g' xhat), s1 / s2 [R]."""
    X, g = X.astype(f32), g.astype(f32)
    R, U, L = X.shape
    mc, rc = mean[:, None, None], rstd[:, None, None]
    xh = (X - mc) * rc
    gp = g
    if relu:
        gp = np.where((xh * gamma + beta > 0) if y is None else (y > 0), g, f32(0)).astype(f32)
    n = f32(U) * f32(L)
    if form == "ln":
        gv = gp * gamma
        m1 = gv.sum(axis=(1, 2), dtype=f32) / n
        m2 = (gv * xh).sum(axis=(1, 2), dtype=f32) / n
        dx = rc * (gv - m1[:, None, None] - xh * m2[:, None, None])
        if radd is not None:
            dx = dx + radd
        dgamma, dbeta = np.zeros(L, f32), np.zeros(L, f32)
        for r in range(R):   # column sums in row order
            dgamma = dgamma + gp[r, 0] * xh[r, 0]
            dbeta = dbeta + gp[r, 0]
        return dict(dx=dx.astype(f32), dgamma=dgamma, dbeta=dbeta)
    # per (unit, slice) sums, slices added in order (the single-pass group kernel keeps per-channel sums too)
    if sl is None and form == "coef":
        sl = L
    if sl is None:
        sg = gp.reshape(R, -1).sum(axis=1, dtype=f32)[:, None]
        sgx = (gp * xh).reshape(R, -1).sum(axis=1, dtype=f32)[:, None]
    else:
        sg, sgx = np.zeros((R, U), f32), np.zeros((R, U), f32)
        for u, lo, hi in _segments(U, L, sl):
            sg[:, u] += gp[:, u, lo:hi].sum(axis=1, dtype=f32)
            sgx[:, u] += (gp[:, u, lo:hi] * xh[:, u, lo:hi]).sum(axis=1, dtype=f32)
    gu = np.broadcast_to(gamma, X.shape)[:, :, 0] if sg.shape[1] == U else np.broadcast_to(gamma, X.shape)[:, :1, 0]
    s1, s2 = np.zeros(R, f32), np.zeros(R, f32)
    weighted = form == "coef" and not bn_mode
    for u in range(sg.shape[1]):   # units in order
        s1 = s1 + (gu[:, u] * sg[:, u] if weighted else sg[:, u])
        s2 = s2 + (gu[:, u] * sgx[:, u] if weighted else sgx[:, u])
    if form == "coef":
        k1 = rc * gamma
        if bn_mode:
            k2 = (k1 * s1[:, None, None]) / n
            k3 = (k1 * s2[:, None, None]) / n
        else:
            k2, k3 = (rstd * s1 / n)[:, None, None], (rstd * s2 / n)[:, None, None]
        dx = k1 * gp - k2 - k3 * xh
    else:  # 'factored'
        inv_n = f32(1) / n
        m1, m2 = (s1 * inv_n)[:, None, None], (s2 * inv_n)[:, None, None]
        dx = (gamma * rc) * (gp - m1 - xh * m2)
    assert dx.dtype == f32
    return dict(dx=dx, sg=sg, sgx=sgx, s1=s1, s2=s2)


def gn_param_grads(bwd, batch, channels):
    """d(gamma) / d(beta) of GroupNorm: the plane sums added over the batch in sample order (gn_param_reduce)."""
    sg, sgx = bwd["sg"].reshape(batch, channels), bwd["sgx"].reshape(batch, channels)
    dg, db = np.zeros(channels, f32), np.zeros(channels, f32)
    for b in range(batch):
        dg, db = dg + sgx[b], db + sg[b]
    return dg, db
