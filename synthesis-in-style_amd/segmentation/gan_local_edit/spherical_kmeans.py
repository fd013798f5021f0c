"""Mini-batch spherical k-means on generator activations that stay on the MI355X.

Same module path, class name and constructor as the reference (segmentation/gan_local_edit/spherical_kmeans.py:159-312, which
subclasses scikit-learn 0.24's MiniBatchKMeans through private modules that no longer exist).  The observable algorithm is the
same -- mini-batch k-means on unit-normalised rows, centres re-normalised around every step, k-means++ initialisation with
``n_init`` tries judged on a validation set, the reassignment rule, the EWA no-improvement stop -- but this is a new
implementation: the data never leaves the device and no scikit-learn is imported.

Randomness is a *fit plan* (``FitPlan``) that depends on ``(N, k, batch_size, n_init, init_size, seed)`` only, never on the
data: validation rows, per-try init rows and the k-means++ draws from ``RandomState(seed)``, the mini-batch row stream from
``RandomState(seed + 1)``, and per iteration a permutation of the mini-batch positions from ``RandomState(seed + 2)`` whose
first entries replace starved centres when that iteration reassigns.  The device therefore runs ``chunk`` iterations per
launch (csrc/spherical_kmeans.hip: skm_loop_kernel) and the host reads the stop flags once per chunk.

Host / device split: k-means++ and the one validation step of each init try run in numpy (float64) on the at most
``(1 + n_init) * init_size`` rows the device gathered and normalised; everything that touches all N pixels (the label pass) or
sits in the iteration loop is a HIP kernel.  All fits over the same activation (the CLI's range of cluster counts) share the
mini-batch stream, so one gather and one loop launch per chunk advance all of them.
"""
import collections
import math
import time

import numpy as np
import torch

import sis_hip

TRANSFERS = collections.Counter()   # "d2h" / "h2d" copies issued by the fits since the last clear (tests, tools)


def _to_host(t):
    TRANSFERS["d2h"] += 1
    return t.cpu().numpy()


def _to_device(a, device):
    TRANSFERS["h2d"] += 1
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


class FitPlan:
    """Every random number of a fit, as plain integer / float arrays."""

    def __init__(self, n, batch_size=100, n_init=3, seed=0, init_size=None):
        if n < 1 or n >= 2 ** 31:
            raise ValueError(f"{n} rows (1 .. 2^31 - 1 are supported)")
        self.n, self.batch_size, self.n_init, self.seed = int(n), int(batch_size), int(n_init), int(seed)
        self.init_size = min(3 * self.batch_size if init_size is None else int(init_size), self.n)
        self._cursor = None

    def init(self, k):
        """{"validation": int32 [init_size], "tries": [{"rows": int32 [init_size], "first": int, "u": float64 [k-1, trials]}]}:
        the validation rows, and per try the init rows, the first k-means++ centre (a position among the init rows) and the
        uniform draws of its k - 1 rounds of ``2 + int(log k)`` candidates."""
        rs = np.random.RandomState(self.seed)
        trials = 2 + int(math.log(k))
        validation = rs.randint(0, self.n, self.init_size).astype(np.int32)
        tries = []
        for _ in range(self.n_init):
            rows = rs.randint(0, self.n, self.init_size).astype(np.int32)
            first = int(rs.randint(self.init_size))
            u = np.stack([rs.random_sample(trials) for _ in range(k - 1)]) if k > 1 else np.zeros((0, trials))
            tries.append({"rows": rows, "first": first, "u": u})
        return {"validation": validation, "tries": tries}

    def batches(self, t0, count):
        """Iterations t0 .. t0 + count - 1: (int32 [count, batch_size] rows of the mini-batches, int32 [count, 32] distinct
        mini-batch positions).  One draw per iteration from each stream, so the values do not depend on how the iterations are
        cut into chunks."""
        if self._cursor is None or t0 < self._cursor:
            self._rb, self._rp = np.random.RandomState(self.seed + 1), np.random.RandomState(self.seed + 2)
            self._cursor = 0
        idx = np.empty((count, self.batch_size), np.int32)
        picks = np.zeros((count, 32), np.int32)
        m = min(32, self.batch_size)
        for s in range(self._cursor - t0, count):   # (negative: iterations to skip over)
            row = self._rb.randint(0, self.n, self.batch_size)
            perm = self._rp.permutation(self.batch_size)
            if s >= 0:
                idx[s] = row
                picks[s, :m] = perm[:m]
        self._cursor = t0 + count
        return idx, picks


def _mark(timings, key, since):
    """tools/bench_semantic_clusters.py: with a dict, wait for the device and add the seconds since ``since`` under ``key``."""
    if timings is None:
        return since
    torch.cuda.synchronize()
    now = time.perf_counter()
    timings[key] = timings.get(key, 0.0) + now - since
    return now


def _unit(x):
    n = np.sqrt((x * x).sum(1, keepdims=True))
    n[n == 0] = 1
    return x / n


def _sqdist(x, c):
    return np.maximum((x * x).sum(1)[:, None] - 2 * x @ c.T + (c * c).sum(1)[None], 0)


def _kmeans_plus_plus(x, k, first, u):
    """Greedy k-means++ over the rows x with the plan's draws (host, float64)."""
    n = len(x)
    centres = [x[first]]
    d = _sqdist(x, centres[0][None])[:, 0]
    pot = d.sum()
    for r in range(k - 1):
        cand = np.clip(np.searchsorted(np.cumsum(d), u[r] * pot), None, n - 1)
        dc = np.minimum(d[None], _sqdist(x[cand], x))
        pots = dc.sum(1)
        best = int(np.argmin(pots))
        centres.append(x[cand[best]])
        d, pot = dc[best], pots[best]
    return np.stack(centres)


def _init_try(xv, xi, k, first, u):
    """One init try: k-means++ on xi, one step on the validation rows from zero counts, inertia on the validation rows."""
    cen = _unit(_kmeans_plus_plus(xi, k, first, u))
    lab = _sqdist(xv, cen).argmin(1)
    cnt = np.zeros(k)
    for j in range(k):
        m = lab == j
        w = int(m.sum())
        if w:
            cen[j] = xv[m].sum(0) / w
            cnt[j] = w
    cen = _unit(cen)
    return _sqdist(xv, cen).min(1).sum(), cen, cnt


class MiniBatchSphericalKMeans:
    """``fit(X)`` takes the activation ``[B, C, H, W]`` as the generator returns it (float32, on the device); row
    ``n = (b H + h) W + w`` of the reference's ``partial_flat(X)`` is one sample of ``C`` features.  Sets ``cluster_centers_``
    (numpy float32 ``[k, C]``, unit rows), ``labels_`` (device int64 ``[N]``), ``inertia_``, ``n_iter_`` and ``counts_`` (the
    mini-batch member counts of the centres); ``label_counts_`` holds the pixels per centre of the final label pass.

    Envelope (anything else raises): ``n_clusters <= 32``, ``C <= 512`` and a multiple of 8, ``batch_size <= 256``,
    ``N < 2^31``.  ``tol > 0`` and sample weights are not implemented.  ``chunk``: iterations per loop-kernel launch."""

    def __init__(self, n_clusters=8, random_state=0, batch_size=100, max_iter=100, n_init=3, init_size=None, max_no_improvement=10,
                 reassignment_ratio=0.01, tol=0.0, compute_labels=True, chunk=64):
        if tol > 0:
            raise NotImplementedError("tol > 0 (the centre-movement stop rule) is not implemented")
        if random_state is None or not isinstance(random_state, (int, np.integer)):
            raise ValueError("random_state must be an integer seed (the fit plan is a function of it)")
        if max_no_improvement is None or max_no_improvement < 1:
            raise NotImplementedError("max_no_improvement must be a positive integer")
        self.n_clusters, self.random_state, self.batch_size, self.max_iter = int(n_clusters), int(random_state), int(batch_size), int(max_iter)
        self.n_init, self.init_size, self.max_no_improvement = int(n_init), init_size, int(max_no_improvement)
        self.reassignment_ratio, self.tol, self.compute_labels, self.chunk = float(reassignment_ratio), tol, compute_labels, int(chunk)
        self.cluster_centers_ = self.labels_ = self.inertia_ = self.n_iter_ = self.counts_ = self.label_counts_ = None

    def fit(self, X, y=None, sample_weight=None):
        if sample_weight is not None:
            raise NotImplementedError("sample weights are not implemented")
        fitted = self.fit_many(X, [self.n_clusters], random_state=self.random_state, batch_size=self.batch_size,
                               max_iter=self.max_iter, n_init=self.n_init, init_size=self.init_size,
                               max_no_improvement=self.max_no_improvement, reassignment_ratio=self.reassignment_ratio, tol=self.tol,
                               compute_labels=self.compute_labels, chunk=self.chunk)[0]
        self.__dict__.update(fitted.__dict__)
        return self

    @classmethod
    def fit_many(cls, X, n_clusters_list, timings=None, **params):
        """Fit one model per entry of ``n_clusters_list`` on the same activation: one loop launch per chunk advances all of
        them (they share the mini-batch stream).  Returns the fitted estimators in order; each equals a separate ``fit``.
        ``timings``: a dict that receives the seconds of the three phases (adds device synchronisations)."""
        models = [cls(n_clusters=k, **params) for k in n_clusters_list]
        if not models:
            return models
        p = models[0]
        if not torch.is_tensor(X) or X.dim() != 4:
            raise ValueError("MiniBatchSphericalKMeans.fit takes the activation as [B, C, H, W]; a flattened [N, C] matrix "
                             "(ptutils.partial_flat) would be a transposed copy of it -- pass the 4-D tensor")
        sis_hip.require_device(X, "X")
        if X.dtype != torch.float32:
            raise RuntimeError(f"X must be float32, got {X.dtype}")
        X = X.contiguous()
        b, ch, h, w = X.shape
        n = b * h * w
        ks = [m.n_clusters for m in models]
        if min(ks) < 1 or max(ks) > sis_hip.SKM_KMAX:
            raise RuntimeError(f"n_clusters {ks}: 1 .. {sis_hip.SKM_KMAX} are supported")
        if p.batch_size < 1 or p.batch_size > sis_hip.SKM_BMAX:
            raise RuntimeError(f"batch_size {p.batch_size}: 1 .. {sis_hip.SKM_BMAX} are supported")
        plan = FitPlan(n, p.batch_size, p.n_init, p.random_state, p.init_size)
        dev = X.device
        since = _mark({} if timings is not None else None, "start", 0.0)

        # ---- initialisation: every planned row of every fit in one gather, k-means++ and the validation step on the host
        inits = [plan.init(k) for k in ks]
        lists = [np.concatenate([ini["validation"]] + [t["rows"] for t in ini["tries"]]) for ini in inits]
        rows = _to_host(sis_hip.skm_gather(X, _to_device(np.concatenate(lists), dev))).astype(np.float64)
        centres = np.zeros((len(ks), sis_hip.SKM_KMAX, ch), np.float32)
        state = sis_hip.skm_new_state(ks, "cpu").numpy()
        isz, off = plan.init_size, 0
        for f, (k, ini) in enumerate(zip(ks, inits)):
            xv, best = rows[off:off + isz], None
            for i, t in enumerate(ini["tries"]):
                xi = rows[off + (1 + i) * isz:off + (2 + i) * isz]
                got = _init_try(xv, xi, k, t["first"], t["u"])
                if best is None or got[0] < best[0]:
                    best = got
            centres[f, :k] = best[1]
            state[f, 8:8 + k] = best[2]
            off += (1 + p.n_init) * isz
        centres_d, state_d = _to_device(centres, dev), _to_device(state, dev)
        last_labels = torch.zeros((len(ks), sis_hip.SKM_BMAX), dtype=torch.int32, device=dev)
        since = _mark(timings, "plan_init_s", since)

        # ---- the loop: per chunk one upload of the plan, one gather, one launch, one read of the flags
        max_iterations = p.max_iter * int(math.ceil(n / p.batch_size))
        alpha = min(2.0 * p.batch_size / (n + 1), 1.0)
        t = 0
        idx, picks = plan.batches(0, min(p.chunk, max_iterations))
        while t < max_iterations:
            count = len(idx)
            buf = _to_device(np.concatenate([idx.ravel(), picks.ravel()]), dev)
            batch_rows = sis_hip.skm_gather(X, buf[:idx.size])
            sis_hip.skm_loop(state_d, centres_d, last_labels, batch_rows, buf[idx.size:], p.batch_size, count, alpha,
                             p.max_no_improvement, p.reassignment_ratio, max_iterations)
            t += count
            if t < max_iterations:   # the next chunk's plan is drawn while the device runs this one
                idx, picks = plan.batches(t, min(p.chunk, max_iterations - t))
            if _to_host(state_d[:, 4]).all():
                break

        since = _mark(timings, "loop_s", since)
        # ---- labels and inertia of all pixels against the final unit centres
        results = []
        for f, (k, m) in enumerate(zip(ks, models)):
            if p.compute_labels:
                m.labels_, res = sis_hip.skm_label(X, centres_d[f, :k])
                results.append(res)
        state, centres = _to_host(state_d), _to_host(centres_d)
        results = _to_host(torch.stack(results)) if results else None
        _mark(timings, "label_pass_s", since)
        for f, (k, m) in enumerate(zip(ks, models)):
            m.cluster_centers_ = centres[f, :k].copy()
            m.counts_ = state[f, 8:8 + k].copy()
            m.n_iter_ = int(state[f, 2])
            m.last_batch_labels_ = last_labels[f, :p.batch_size]
            if results is not None:
                m.inertia_ = float(results[f, 0])
                m.label_counts_ = results[f, 1:1 + k].astype(np.int64)
        return models
