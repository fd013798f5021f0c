"""Spherical k-means fit, the parts that need no device:
* the numpy restatement (tests/spherical_kmeans_restatement.py) recovers planted partitions, and so does scikit-learn's public
  MiniBatchKMeans on the normalised rows where it is installed: the restatement is pinned to an independent implementation;
* the fit plan does not depend on how iterations are cut into chunks, and is the random stream the restatement draws;
* header / ctypes table agree on the new symbols; the product imports neither the oracle nor scikit-learn;
* a FactorCatalog without centres and without a fit still raises.
"""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spherical_kmeans_restatement as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "synthesis-in-style_amd")
CASES = [(case, seed) for case in R.PLANTED_CASES for seed in R.PLANTED_SEEDS]


@pytest.mark.parametrize("case,seed", CASES)
def test_restatement_recovers_the_planted_partition(case, seed):
    n, c, k, noise = case
    x, lab, dirs = R.planted(n, c, k, noise, seed)
    s = np.sort(R.normalize(x.astype(np.float64)) @ dirs.T, 1)
    assert np.array_equal((R.normalize(x.astype(np.float64)) @ dirs.T).argmax(1), lab)
    assert (s[:, -1] - s[:, -2]).min() >= 0.27   # the planted partition is well separated at every row
    cen, labels, inertia, n_iter, counts = R.fit(x, k, dtype=np.float64)
    assert R.agreement(labels, lab, k) == 1.0
    assert np.allclose(np.linalg.norm(cen, axis=1), 1.0, atol=1e-12)
    assert counts.sum() >= n_iter * 100   # (the validation step's members plus 100 per iteration)


@pytest.mark.parametrize("case,seed", CASES)
def test_scikit_learn_recovers_the_same_partition(case, seed):
    cluster = pytest.importorskip("sklearn.cluster")
    n, c, k, noise = case
    x, lab, _ = R.planted(n, c, k, noise, seed)
    km = cluster.MiniBatchKMeans(n_clusters=k, random_state=0, batch_size=100, max_iter=100, n_init=3, max_no_improvement=10,
                                 reassignment_ratio=0.01, tol=0.0).fit(R.normalize(x.astype(np.float64)))
    assert R.agreement(km.labels_, lab, k) == 1.0


def test_restatement_float32_and_float64_agree():
    n, c, k, noise = R.PLANTED_CASES[0]
    x, _, _ = R.planted(n, c, k, noise, 0)
    c64, l64, i64, n64, w64 = R.fit(x, k, dtype=np.float64)
    c32, l32, i32, n32, w32 = R.fit(x, k, dtype=np.float32)
    assert n64 == n32 and np.array_equal(l64, l32) and np.array_equal(w64, w32)
    assert np.abs(c64 - c32).max() < 2e-6 and abs(i64 - i32) / i64 < 2e-6


def test_fit_plan_does_not_depend_on_the_chunk_length():
    from segmentation.gan_local_edit.spherical_kmeans import FitPlan
    n, batch, total = 5000, 100, 300
    got = {}
    for chunk in (1, 7, 256):
        plan = FitPlan(n, batch, n_init=3, seed=4)
        idx, picks = [], []
        for t0 in range(0, total, chunk):
            a, b = plan.batches(t0, min(chunk, total - t0))
            idx.append(a)
            picks.append(b)
        got[chunk] = (np.concatenate(idx), np.concatenate(picks))
    for chunk in (7, 256):
        assert np.array_equal(got[1][0], got[chunk][0]) and np.array_equal(got[1][1], got[chunk][1])
    idx, picks = got[1]
    assert idx.dtype == np.int32 and idx.shape == (total, batch) and idx.min() >= 0 and idx.max() < n
    assert picks.shape == (total, 32) and picks.min() >= 0 and picks.max() < batch
    assert all(len(set(row)) == 32 for row in picks.tolist())   # distinct mini-batch positions
    # a plan asked again for an earlier chunk replays it
    plan = FitPlan(n, batch, n_init=3, seed=4)
    plan.batches(0, 50)
    again = plan.batches(20, 10)
    assert np.array_equal(again[0], idx[20:30]) and np.array_equal(again[1], picks[20:30])
    # and it is the stream the restatement draws
    rb, rp = np.random.RandomState(5), np.random.RandomState(6)
    for t in range(5):
        assert np.array_equal(rb.randint(0, n, batch), idx[t])
        assert np.array_equal(rp.permutation(batch)[:32], picks[t])


def test_fit_plan_small_batch_and_init():
    from segmentation.gan_local_edit.spherical_kmeans import FitPlan
    plan = FitPlan(50, batch_size=20, n_init=2, seed=1)
    assert plan.init_size == 50
    idx, picks = plan.batches(0, 3)
    assert idx.max() < 50 and picks.max() < 20
    assert all(len(set(row[:20])) == 20 for row in picks.tolist())   # 20 positions: all of them, each once
    ini = plan.init(5)
    assert ini["validation"].shape == (50,) and len(ini["tries"]) == 2
    for t in ini["tries"]:
        assert t["rows"].min() >= 0 and t["rows"].max() < 50 and 0 <= t["first"] < 50
        assert t["u"].shape == (4, 2 + int(np.log(5))) and (t["u"] >= 0).all() and (t["u"] < 1).all()
    rs = np.random.RandomState(1)   # the restatement's order of draws
    assert np.array_equal(rs.randint(0, 50, 50), ini["validation"])
    assert np.array_equal(rs.randint(0, 50, 50), ini["tries"][0]["rows"])
    assert rs.randint(50) == ini["tries"][0]["first"]


def test_host_initialisation_matches_the_restatement():
    """k-means++ and the validation step of the product (host, float64) against the restatement's, same draws."""
    from segmentation.gan_local_edit import spherical_kmeans as P
    x, _, _ = R.planted(4096, 64, 5, 0.3, 0)
    xn = R.normalize(x.astype(np.float64))
    plan = P.FitPlan(len(x), 100, 3, 0)
    ini = plan.init(5)
    rs = np.random.RandomState(0)
    xv = xn[rs.randint(0, len(x), 300)]
    for t in ini["tries"]:
        ii = rs.randint(0, len(x), 300)
        cen = R.normalize(R.kmeans_plus_plus(xn[ii], 5, rs))
        cnt = np.zeros(5)
        R.step(xv, cen, cnt, False, None, 0.01)
        cen = R.normalize(cen)
        inertia, got_cen, got_cnt = P._init_try(xn[ini["validation"]], xn[t["rows"]], 5, t["first"], t["u"])
        assert np.array_equal(got_cnt, cnt) and np.abs(got_cen - cen).max() < 1e-12
        assert abs(inertia - R.sqdist(xv, cen).min(1).sum()) < 1e-9


def _declared_symbols():
    text = open(os.path.join(ROOT, "include", "sis_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(sis_[a-z0-9_]+)\s*\(", text))


def test_header_and_ctypes_table_agree_on_the_new_symbols():
    import sis_hip
    new = {"sis_skm_state_doubles", "sis_skm_gather", "sis_skm_loop", "sis_skm_label_workspace_doubles", "sis_skm_label"}
    assert new <= _declared_symbols() and new <= set(sis_hip.exported_symbols())
    L = sis_hip.lib()
    assert L.sis_skm_state_doubles() == 40
    assert L.sis_skm_label_workspace_doubles(1) == 33 and L.sis_skm_label_workspace_doubles(10 ** 9) == 1024 * 33
    header = open(os.path.join(ROOT, "include", "sis_hip.h")).read()
    for name, (argtypes, _) in sis_hip._SIGNATURES.items():
        if name in new:
            decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, re.sub(r"/\*.*?\*/", "", header, flags=re.S)).group(1)
            n_args = 0 if decl.strip() == "void" else decl.count(",") + 1
            assert n_args == len(argtypes), name


def test_unsupported_shapes_fail_with_a_message():
    import sis_hip
    L = sis_hip.lib()
    assert L.sis_skm_label(None, None, None, None, None, 1, 520, 16, 3, None) != 0 and b"channels" in L.sis_last_error()
    assert L.sis_skm_label(None, None, None, None, None, 1, 20, 16, 3, None) != 0 and b"channels" in L.sis_last_error()
    assert L.sis_skm_label(None, None, None, None, None, 1, 64, 16, 33, None) != 0 and b"centres" in L.sis_last_error()
    assert L.sis_skm_label(None, None, None, None, None, 1 << 15, 64, 1 << 16, 3, None) != 0 and b"pixels" in L.sis_last_error()
    assert L.sis_skm_loop(None, None, None, None, None, 1, 64, 257, 1, 0.1, 10, 0.01, 100, None) != 0 and b"batch_size" in L.sis_last_error()
    assert L.sis_skm_gather(None, None, None, 4, 1, 1024, 16, None) != 0 and b"channels" in L.sis_last_error()


def test_product_imports_neither_the_oracle_nor_scikit_learn():
    for base, _, files in os.walk(SRC):
        for name in files:
            if name.endswith(".py"):
                text = open(os.path.join(base, name)).read()
                assert not re.search(r"^\s*(from|import)\s+(oracle|sklearn)\b", text, flags=re.M), os.path.join(base, name)
                assert "spherical_kmeans_restatement" not in text, os.path.join(base, name)


def test_estimator_arguments():
    import torch
    from segmentation.gan_local_edit.spherical_kmeans import MiniBatchSphericalKMeans
    with pytest.raises(NotImplementedError):
        MiniBatchSphericalKMeans(3, tol=1e-3)
    km = MiniBatchSphericalKMeans(3)
    assert (km.batch_size, km.max_iter, km.n_init, km.max_no_improvement, km.reassignment_ratio) == (100, 100, 3, 10, 0.01)
    with pytest.raises(NotImplementedError):
        km.fit(torch.zeros(1, 8, 4, 4), sample_weight=torch.ones(16))
    with pytest.raises(ValueError, match=r"\[B, C, H, W\]"):
        km.fit(torch.zeros(16, 8))
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        km.fit(torch.zeros(1, 8, 4, 4))   # no CPU path


def test_catalog_without_centres_and_without_a_fit_still_raises():
    import torch
    from segmentation.gan_local_edit.factor_catalog import FactorCatalog
    for cat in (FactorCatalog(5), FactorCatalog(5, random_state=1, compute_labels=True), FactorCatalog()):
        with pytest.raises(RuntimeError, match="no cluster centres"):
            cat.predict(torch.zeros(1, 8, 4, 4))
    with pytest.raises(RuntimeError, match="nothing to fit"):
        FactorCatalog(cluster_centers=np.zeros((3, 8), np.float32)).fit_predict(torch.zeros(1, 8, 4, 4))
    assert FactorCatalog(3, cluster_centers=np.zeros((3, 8), np.float32)).cluster_centers.shape == (3, 8)


def test_ptutils_round_trip():
    import torch
    from segmentation.gan_local_edit import ptutils
    x = torch.arange(2 * 3 * 4 * 4, dtype=torch.float32).reshape(2, 3, 4, 4)
    flat = ptutils.partial_flat(x)
    assert flat.shape == (32, 3) and torch.equal(flat[(1 * 4 + 2) * 4 + 3], x[1, :, 2, 3])
    assert torch.equal(ptutils.partial_unflat(flat, N=2, H=4), x)
    store = ptutils.MultiResolutionStore(x, 'nearest')
    assert store.get() is x and store.get(8).shape == (2, 3, 8, 8) and 8 in store and len(store) == 2
    assert torch.equal(store.get(8)[:, :, ::2, ::2], x)
