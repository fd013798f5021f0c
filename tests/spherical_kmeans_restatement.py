"""Plain numpy restatement of the spherical mini-batch k-means contract of DESIGN.md §9, in float64 or float32.

Test-only: the yardstick for csrc/spherical_kmeans.hip and segmentation/gan_local_edit/spherical_kmeans.py, never imported by
product code and importing none of it.  It draws its random numbers itself, straight from the three ``RandomState`` streams, so
it also checks the product's ``FitPlan`` (a fit only agrees when the plan produces the same numbers).
"""
import numpy as np


def normalize(x):
    n = np.sqrt((x * x).sum(1, keepdims=True))
    n[n == 0] = 1
    return x / n


def sqdist(x, c):
    """[n, k] squared Euclidean distances."""
    return np.maximum((x * x).sum(1)[:, None] - 2 * x @ c.T + (c * c).sum(1)[None], 0)


def kmeans_plus_plus(x, k, rs):
    n = len(x)
    trials = 2 + int(np.log(k))
    cen = [x[rs.randint(n)]]
    d = sqdist(x, cen[0][None])[:, 0]
    pot = d.sum()
    for _ in range(1, k):
        cand = np.searchsorted(np.cumsum(d.astype(np.float64)), rs.random_sample(trials) * float(pot))
        cand = np.clip(cand, None, n - 1)
        dc = np.minimum(d[None], sqdist(x[cand], x).astype(d.dtype))
        pots = dc.sum(1)
        b = int(np.argmin(pots))
        cen.append(x[cand[b]])
        d, pot = dc[b], pots[b]
    return np.stack(cen)


def step(xb, cen, cnt, reassign, picks, ratio):
    """One mini-batch step, in place on cen / cnt.  Returns (inertia, labels)."""
    d = sqdist(xb, cen)
    lab = d.argmin(1)
    inertia = d[np.arange(len(xb)), lab].sum()
    if reassign and ratio > 0:
        to = cnt < ratio * cnt.max()
        if to.sum() > .5 * len(xb):
            to[np.argsort(cnt, kind="stable")[int(.5 * len(xb)):]] = False
        nr = int(to.sum())
        if nr:
            cen[to] = xb[picks[:nr]]
        cnt[to] = cnt[~to].min()
    for j in range(len(cen)):
        m = lab == j
        w = m.sum()
        if w > 0:
            cen[j] = (cen[j] * cnt[j] + xb[m].sum(0)) / (cnt[j] + w)
            cnt[j] += w
    return inertia, lab


def is_reassignment_iteration(t, cnt):
    return (t + 1) % (10 + int(cnt.min())) == 0


def fit(x, k, seed=0, batch=100, max_iter=100, n_init=3, max_no_imp=10, ratio=.01, dtype=np.float64):
    """x: [N, C] rows (partial_flat order).  Returns (centres, labels, inertia, n_iter, counts)."""
    x = normalize(x.astype(dtype))
    n = len(x)
    rs, rb, rp = np.random.RandomState(seed), np.random.RandomState(seed + 1), np.random.RandomState(seed + 2)
    isz = min(3 * batch, n)
    xv = x[rs.randint(0, n, isz)]
    best = None
    for _ in range(n_init):
        ii = rs.randint(0, n, isz)
        cen = normalize(kmeans_plus_plus(x[ii], k, rs))
        cnt = np.zeros(k, dtype)
        step(xv, cen, cnt, False, None, ratio)
        cen = normalize(cen)
        ine = sqdist(xv, cen).min(1).sum()
        if best is None or ine < best[0]:
            best = (ine, cen.copy(), cnt.copy())
    _, cen, cnt = best
    n_iter = max_iter * int(np.ceil(n / batch))
    alpha = min(batch * 2 / (n + 1), 1.0)
    ewa = ewa_min = None
    noimp = 0
    for t in range(n_iter):
        idx = rb.randint(0, n, batch)
        picks = rp.permutation(batch)[:k]
        cen = normalize(cen)
        bi = step(x[idx], cen, cnt, is_reassignment_iteration(t, cnt), picks, ratio)[0] / batch
        cen = normalize(cen)
        ewa = bi if ewa is None else ewa * (1 - alpha) + bi * alpha
        if ewa_min is None or ewa < ewa_min:
            ewa_min, noimp = ewa, 0
        else:
            noimp += 1
        if noimp >= max_no_imp:
            break
    d = sqdist(x, cen)
    return cen, d.argmin(1), d.min(1).sum(), t + 1, cnt


def planted(n, c, k, noise, seed):
    """Planted directions with log-normal row scales: (x float32 [n, c], planted labels)."""
    r = np.random.RandomState(seed)
    dirs = normalize(r.randn(k, c))
    lab = r.randint(0, k, n)
    scale = np.exp(r.randn(n, 1) * 0.5)
    return ((dirs[lab] + noise * r.randn(n, c) / np.sqrt(c)) * scale).astype(np.float32), lab, dirs


PLANTED_CASES = [(4096, 64, 5, 0.3), (8192, 128, 8, 0.5), (8192, 128, 8, 1.0), (16384, 128, 12, 0.5), (4096, 24, 3, 0.3)]
PLANTED_SEEDS = (0, 1, 2)


def agreement(a, b, k):
    """Fraction of rows on which labelings a and b agree after the best one-to-one relabelling."""
    from scipy.optimize import linear_sum_assignment
    cm = np.zeros((k, k), int)
    np.add.at(cm, (a, b), 1)
    r, c = linear_sum_assignment(-cm)
    return cm[r, c].sum() / len(a)


def to_nchw(x, b):
    """[N, C] rows -> [B, C, H, W] with N = B * H * W (H = W), the layout the device fit reads."""
    n, c = x.shape
    hw = n // b
    h = int(round(hw ** 0.5))
    assert b * h * h == n, (n, b)
    return np.ascontiguousarray(x.reshape(b, h, h, c).transpose(0, 3, 1, 2))
