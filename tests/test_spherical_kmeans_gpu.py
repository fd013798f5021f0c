"""Spherical k-means fit on the device (csrc/spherical_kmeans.hip, segmentation/gan_local_edit/spherical_kmeans.py) against the
float64 numpy restatement (tests/spherical_kmeans_restatement.py).

Bounds.  Discrete results (labels, counts, n_iter) must equal the float64 restatement's.  Centres and inertia: 8 x the difference
between the restatement's own float32 run and its float64 run, computed here per case from the restatement alone (a different
float32 summation order should cost no more than a few times what float32 itself costs); each test prints the device's
difference next to the bound before it asserts.
"""
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spherical_kmeans_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu


def _bound(v32, v64, relative=False):
    d = np.abs(np.asarray(v32, np.float64) - np.asarray(v64, np.float64)).max()
    return 8.0 * (d / abs(float(v64)) if relative else d)


# ------------------------------------------------------------------------------------------------------------ one step
def _exact_unit_centres(k, c, rs):
    """Centres whose entries are +-0.25 on 16 coordinates: unit norm exactly, in float32 and float64 alike."""
    cen = np.zeros((k, c))
    for j in range(k):
        cen[j, rs.choice(c, 16, replace=False)] = 0.25 * rs.choice([-1.0, 1.0], 16)
    return cen


def _one_step_cases():
    cases = {}
    rs = np.random.RandomState(3)
    x, _, dirs = R.planted(100, 64, 5, 0.3, 11)
    rows = R.normalize(x.astype(np.float64)).astype(np.float32)
    cen = R.normalize(dirs + 0.05 * rs.randn(5, 64))
    picks = rs.permutation(100)[:32]
    cases["plain"] = (rows, cen, np.array([30., 25., 40., 20., 35.]), 0, picks, False)
    # counts put into the state make iteration 9 a reassignment ((9 + 1) % (10 + 0) == 0): centres 1 and 3 are starved
    cases["reassignment"] = (rows, cen, np.array([500., 0., 450., 3., 480.]), 9, picks, True)
    cases["same_counts_other_iteration"] = (rows, cen, np.array([500., 0., 450., 3., 480.]), 10, picks, False)
    away = cen.copy()
    away[2] = -R.normalize(rows.astype(np.float64).sum(0)[None])[0]   # points away from every row: nobody's nearest centre
    cases["centre_without_members"] = (rows, away, np.array([30., 25., 40., 20., 35.]), 3, picks, False)
    x, _, dirs = R.planted(256, 512, 32, 0.5, 12)   # the envelope's corner: 256 rows, 512 channels, 32 centres
    cases["largest"] = (R.normalize(x.astype(np.float64)).astype(np.float32), R.normalize(dirs + 0.05 * rs.randn(32, 512)),
                        np.arange(32, dtype=np.float64) * 7 + 20, 5, rs.permutation(256)[:32], False)
    x, _, dirs = R.planted(50, 24, 3, 0.3, 13)
    cases["small"] = (R.normalize(x.astype(np.float64)).astype(np.float32), R.normalize(dirs + 0.05 * rs.randn(3, 24)),
                      np.array([0., 12., 2000.]), 19, rs.permutation(50)[:32], True)
    # a zero row (distance 1 to every unit centre: label 0) and an exact tie between two equal centres (the lower index wins)
    ec = _exact_unit_centres(4, 64, rs)
    ec[2] = ec[1]
    zrows = rows.copy()
    zrows[:40] = R.normalize(ec[1][None] + 0.3 * rs.randn(40, 64) / 8).astype(np.float32)
    zrows[7] = 0
    cases["zero_row_and_tie"] = (zrows, ec, np.array([10., 20., 30., 40.]), 1, picks, False)
    return cases


ONE_STEP = _one_step_cases()


@pytest.mark.parametrize("name", sorted(ONE_STEP))
def test_one_step_equals_the_restatement(device, name):
    import sis_hip
    rows, cen0, counts, t, picks, expect_reassign = ONE_STEP[name]
    batch, c = rows.shape
    k = len(cen0)
    ref = {}
    for dt in (np.float64, np.float32):
        cen, cnt = R.normalize(cen0.astype(dt)), counts.astype(dt)
        reassign = R.is_reassignment_iteration(t, cnt)
        assert reassign == expect_reassign
        inertia, lab = R.step(rows.astype(dt), cen, cnt, reassign, picks[:k], 0.01)
        ref[dt] = (R.normalize(cen), cnt, float(inertia), lab)
    if name == "zero_row_and_tie":
        assert ref[np.float64][3][7] == 0 and not (ref[np.float64][3] == 2).any() and (ref[np.float64][3] == 1).sum() >= 40
    if name == "centre_without_members":
        assert not (ref[np.float64][3] == 2).any()
    state = sis_hip.skm_new_state([k], "cpu")
    state[0, 2] = t
    state[0, 8:8 + k] = torch.from_numpy(counts)
    state = state.to(device)
    centres = torch.zeros(1, 32, c)
    centres[0, :k] = torch.from_numpy(cen0.astype(np.float32))
    centres = centres.to(device)
    last = torch.full((1, 256), -1, dtype=torch.int32, device=device)
    pk = torch.zeros(1, 32, dtype=torch.int32)
    pk[0, :len(picks)] = torch.from_numpy(picks.astype(np.int32))
    sis_hip.skm_loop(state, centres, last, torch.from_numpy(rows).to(device), pk.to(device), batch, 1, 0.05, 10, 0.01, 10 ** 6)
    torch.cuda.synchronize()
    st = state.cpu().numpy()[0]
    cen64, cnt64, ine64, lab64 = ref[np.float64]
    cen32, _, ine32, _ = ref[np.float32]
    got_cen = centres.cpu().numpy()[0, :k].astype(np.float64)
    d_cen, b_cen = np.abs(got_cen - cen64).max(), _bound(cen32, cen64)
    d_ine, b_ine = abs(st[5] - ine64) / ine64, _bound(ine32, ine64, relative=True)
    print(f"{name}: centres {d_cen:.2e} (bound {b_cen:.2e}), inertia rel {d_ine:.2e} (bound {b_ine:.2e})")
    assert np.array_equal(last.cpu().numpy()[0, :batch], lab64)
    assert (last.cpu().numpy()[0, batch:] == -1).all()
    assert np.array_equal(st[8:8 + k], cnt64) and st[2] == t + 1 and st[4] == 0
    assert d_cen <= b_cen and d_ine <= b_ine


# ------------------------------------------------------------------------------------------------ gather and label pass
# (B, C, H, W, k, unit centres); every entry was checked on the CPU: numpy's float32 argmax differs from the float64 one on no row
PASS_CASES = [(1, 24, 4, 4, 2, True), (3, 64, 8, 8, 3, True), (5, 128, 16, 16, 12, True), (1, 256, 32, 32, 24, True),
              (3, 512, 16, 16, 32, True), (1, 128, 256, 256, 12, True), (5, 512, 4, 4, 3, True), (1, 64, 64, 64, 32, True),
              (3, 24, 5, 5, 3, True), (3, 128, 32, 32, 12, False)]


def _pass_case(b, c, h, w, k, unit, seed=5):
    n = b * h * w
    x, lab, dirs = R.planted(n, c, k, 0.5, seed)
    rs = np.random.RandomState(seed + 100)
    cen = R.normalize(dirs + 0.05 * rs.randn(k, c))
    if not unit:
        cen = cen * np.exp(0.2 * rs.randn(k, 1))
    if n >= 1024:
        x[n // 3] = 0   # one zero pixel
    xn = np.ascontiguousarray(x.reshape(b, h, w, c).transpose(0, 3, 1, 2))
    return x, xn, cen.astype(np.float32)


@pytest.mark.parametrize("b,c,h,w,k,unit", PASS_CASES)
def test_gather_normalises_the_listed_rows(device, b, c, h, w, k, unit):
    import sis_hip
    x, xn, _ = _pass_case(b, c, h, w, k, unit)
    n = len(x)
    idx = np.random.RandomState(1).randint(0, n, 777).astype(np.int32)
    idx[:3] = (0, n - 1, n // 3)
    got = sis_hip.skm_gather(torch.from_numpy(xn).to(device), torch.from_numpy(idx).to(device)).cpu().numpy()
    want = R.normalize(x.astype(np.float64))[idx]
    err = np.abs(got - want).max()
    print(f"gather {b}x{c}x{h}x{w}: max abs err {err:.2e} (bound {2 * 2.0 ** -23:.2e})")
    assert got.shape == (777, c) and ((got[2] == 0).all() or n < 1024)
    assert err <= 2 * 2.0 ** -23


@pytest.mark.parametrize("b,c,h,w,k,unit", PASS_CASES)
def test_label_pass_equals_the_float64_argmax(device, b, c, h, w, k, unit):
    import sis_hip
    x, xn, cen = _pass_case(b, c, h, w, k, unit)
    n = len(x)
    ref = {}
    for dt in (np.float64, np.float32):
        d = R.sqdist(R.normalize(x.astype(dt)), cen.astype(dt))
        ref[dt] = (d.argmin(1), float(d.min(1).sum(dtype=np.float64)))
    c64 = cen.astype(np.float64)
    score = R.normalize(x.astype(np.float64)) @ c64.T - 0.5 * (c64 * c64).sum(1)[None]
    top = np.sort(score, 1)
    gap = top[:, -1] - top[:, -2]
    lab64 = score.argmax(1)
    sure = gap > 1e-5   # (the zero pixel scores -|c|^2/2 at every centre: a tie for unit centres, up to their rounding)
    left_out = int((~sure).sum())
    assert left_out <= int(0.005 * n), left_out
    assert np.array_equal(ref[np.float32][0][sure], lab64[sure])   # the CPU check of the case list
    labels, result = sis_hip.skm_label(torch.from_numpy(xn).to(device), torch.from_numpy(cen).to(device))
    labels, result = labels.cpu().numpy(), result.cpu().numpy()
    wrong = int((labels[sure] != lab64[sure]).sum())
    counts64 = np.bincount(lab64, minlength=k)
    d_cnt = int(np.abs(result[1:1 + k] - counts64).max())
    ine64 = ref[np.float64][1]
    d_ine, b_ine = abs(result[0] - ine64) / ine64, _bound(ref[np.float32][1], ine64, relative=True)
    print(f"label pass {b}x{c}x{h}x{w} k={k}: {wrong} wrong of {int(sure.sum())} sure rows, {left_out} left out, counts differ by "
          f"{d_cnt}, inertia rel {d_ine:.2e} (bound {b_ine:.2e})")
    assert labels.shape == (n,) and labels.min() >= 0 and labels.max() < k
    assert wrong == 0
    assert np.array_equal(result[1:1 + k], np.bincount(labels, minlength=k)) and (result[1 + k:] == 0).all()
    assert d_cnt <= left_out
    assert d_ine <= b_ine


# ------------------------------------------------------------------------------------------------------------ whole fit
FIT_CASES = [(case, seed) for case in R.PLANTED_CASES for seed in R.PLANTED_SEEDS]


def _planted_tensor(case, seed, device, b=None):
    n, c, k, noise = case
    x, lab, _ = R.planted(n, c, k, noise, seed)
    b = b or {4096: 4, 8192: 2, 16384: 4}[n]
    return x, lab, torch.from_numpy(R.to_nchw(x, b)).to(device)


@pytest.mark.parametrize("case,seed", FIT_CASES)
def test_whole_fit_equals_the_restatement(device, case, seed):
    """Measured on an MI355X (all 15 cases): see DESIGN.md §9 for the table of device differences next to the bounds."""
    from segmentation.gan_local_edit.spherical_kmeans import MiniBatchSphericalKMeans
    n, c, k, noise = case
    x, planted_labels, xd = _planted_tensor(case, seed, device)
    c64, l64, i64, n64, w64 = R.fit(x, k, dtype=np.float64)
    c32, l32, i32, n32, w32 = R.fit(x, k, dtype=np.float32)
    km = MiniBatchSphericalKMeans(k).fit(xd)
    labels = km.labels_.cpu().numpy()
    d_cen, b_cen = np.abs(km.cluster_centers_.astype(np.float64) - c64).max(), _bound(c32, c64)
    d_ine, b_ine = abs(km.inertia_ - i64) / i64, _bound(i32, i64, relative=True)
    print(f"fit {case} seed {seed}: n_iter {km.n_iter_} (restatement {n64}, float32 {n32}), centres {d_cen:.2e} (bound {b_cen:.2e}), "
          f"inertia rel {d_ine:.2e} (bound {b_ine:.2e}), labels differing {(labels != l64).sum()}")
    assert km.n_iter_ == n64
    assert np.array_equal(labels, l64)
    assert np.array_equal(km.counts_, w64)
    assert np.array_equal(km.label_counts_, np.bincount(l64, minlength=k))
    assert R.agreement(labels, planted_labels, k) == 1.0
    assert km.cluster_centers_.dtype == np.float32 and km.cluster_centers_.shape == (k, c)
    assert d_cen <= b_cen and d_ine <= b_ine


def _bytes_of(km):
    return (km.cluster_centers_.tobytes(), km.labels_.cpu().numpy().tobytes(), km.counts_.tobytes(), km.n_iter_, km.inertia_,
            km.label_counts_.tobytes())


def test_chunking_batching_and_reruns_give_the_same_bytes(device):
    from segmentation.gan_local_edit.spherical_kmeans import MiniBatchSphericalKMeans
    case = R.PLANTED_CASES[1]
    _, _, xd = _planted_tensor(case, 0, device)
    base = _bytes_of(MiniBatchSphericalKMeans(8, chunk=16).fit(xd))
    assert base[3] > 20   # (several chunks of 16)
    for chunk in (1, 256):
        assert _bytes_of(MiniBatchSphericalKMeans(8, chunk=chunk).fit(xd)) == base, chunk
    assert _bytes_of(MiniBatchSphericalKMeans(8, chunk=16).fit(xd)) == base   # a second run
    many = MiniBatchSphericalKMeans.fit_many(xd, [3, 5, 8])
    assert [m.n_clusters for m in many] == [3, 5, 8]
    assert _bytes_of(many[2]) == _bytes_of(MiniBatchSphericalKMeans(8).fit(xd)) == base
    for m in many[:2]:
        assert _bytes_of(m) == _bytes_of(MiniBatchSphericalKMeans(m.n_clusters).fit(xd))
    assert len({m.n_iter_ for m in many}) > 1   # (the batched fits did stop at different iterations)


def test_no_host_round_trip_per_iteration(device):
    """Launches and copies of one fit, counted by sis_hip's launch accounting and the module's transfer counter.  Per chunk of T
    iterations the fit issues one upload (rows and picks of the plan), one gather launch, one loop launch and one read of the
    done flags; around the loop a constant number: init gather + its read, the uploads of centres and state, the label pass and
    the three final reads.  So: loop launches <= ceil(I / T), device-to-host copies <= ceil(I / T) + 4, all launches
    <= 2 ceil(I / T) + 2 -- nothing grows with I but through ceil(I / T)."""
    import sis_hip
    from segmentation.gan_local_edit import spherical_kmeans as P
    _, _, xd = _planted_tensor(R.PLANTED_CASES[1], 0, device)
    for chunk in (16, 64):
        records = []
        P.TRANSFERS.clear()
        sis_hip.set_profiler(records)
        try:
            km = P.MiniBatchSphericalKMeans(8, chunk=chunk).fit(xd)
        finally:
            sis_hip.set_profiler(None)
        chunks = math.ceil(km.n_iter_ / chunk)
        names = [r[0] for r in records]
        print(f"chunk {chunk}: {km.n_iter_} iterations, launches {len(names)}, transfers {dict(P.TRANSFERS)}")
        assert names.count("skm_loop_kernel") == chunks
        assert names.count("skm_gather_kernel") == chunks + 1 and names.count("skm_label_kernel") == 1
        assert len(names) <= 2 * chunks + 2
        assert P.TRANSFERS["d2h"] <= chunks + 4 and P.TRANSFERS["h2d"] <= chunks + 3


# ------------------------------------------------------------------------------------------------ generator activations
@pytest.fixture(scope="module")
def generator_activations(device):
    from networks.stylegan2.model import Generator
    from oracle import stylegan2_ref as O
    g = Generator(64, 512, 8, channel_multiplier=2)
    g.load_state_dict(O.seeded_state_dict(64, 512, 8, 2, seed=21), strict=True)
    g = g.to(device).eval()
    z, noise = O.seeded_inputs(64, 4, 512, seed=22)
    with torch.no_grad():
        _, acts = g([z.to(device)], noise=[n.to(device) for n in noise], return_intermediate_activations=True)
    torch.cuda.synchronize()
    acts = {key: a.contiguous() for key, a in acts.items() if a.shape[-1] >= 16}
    assert sorted(acts) == [4, 5, 6, 7, 8, 9] and all(a.shape[1] == 512 for a in acts.values())
    return acts


@pytest.mark.parametrize("k", [3, 8])
@pytest.mark.parametrize("layer", [4, 5, 6, 7, 8, 9])
def test_fit_predict_on_generator_activations(device, generator_activations, layer, k):
    from segmentation.gan_local_edit.factor_catalog import FactorCatalog
    act = generator_activations[layer]
    b, c, h, w = act.shape
    x = act.permute(0, 2, 3, 1).reshape(-1, c).cpu().numpy()
    c64, l64, i64, n64, w64 = R.fit(x, k, dtype=np.float64)
    c32, l32, i32, n32, w32 = R.fit(x, k, dtype=np.float32)
    cat = FactorCatalog(k, compute_labels=True)
    heat = cat.fit_predict(act, raw=True).get()
    km = cat._factorization
    labels = km.labels_.cpu().numpy()
    s = np.sort(R.normalize(x.astype(np.float64)) @ c64.T, 1)
    sure = (s[:, -1] - s[:, -2]) >= 1e-4
    left_out = int((~sure).sum())
    wrong = int((labels[sure] != l64[sure]).sum())
    d_cen, b_cen = np.abs(km.cluster_centers_.astype(np.float64) - c64).max(), _bound(c32, c64)
    d_ine, b_ine = abs(km.inertia_ - i64) / i64, _bound(i32, i64, relative=True)
    print(f"layer {layer} {tuple(act.shape)} k={k}: n_iter {km.n_iter_} (restatement {n64}, float32 {n32}), {wrong} wrong labels, "
          f"{left_out} of {len(x)} rows left out, centres {d_cen:.2e} (bound {b_cen:.2e}), inertia rel {d_ine:.2e} (bound {b_ine:.2e})")
    assert km.n_iter_ == n64
    assert left_out <= 0.005 * len(x)
    assert wrong == 0
    assert d_cen <= b_cen and d_ine <= b_ine
    assert heat.shape == (b, k, h, w) and torch.equal(heat.sum(1), torch.ones_like(heat[:, 0]))
    assert torch.equal(heat.argmax(1).reshape(-1), km.labels_)
    assert torch.equal(cat.cluster_centers.cpu(), torch.from_numpy(km.cluster_centers_))
    assert cat.predict(act).shape == (b, h, w)   # (works after the fit; its rule differs from labels_, see factor_catalog.py)


# ------------------------------------------------------------------------------------------------------------ end to end
def test_cli_end_to_end(device, tmp_path):
    import argparse
    import create_dataset_for_segmentation as D
    import create_semantic_segmentation as S
    from segmentation.gan_local_edit.factor_catalog import FactorCatalog
    torch.manual_seed(0)
    args = S.build_parser().parse_args(["--destination", str(tmp_path / "out"), "-n", "8", "-b", "4", "-c", "3", "5", "-s", "8",
                                        "--image-size", "64"])
    dest, found = S.main(args)
    layers = sorted(found[3])
    assert layers == [4, 5, 6, 7, 8, 9] and sorted(found) == [3, 4]
    for k in (3, 4):
        meta = json.load(open(dest / "catalogs" / f"{k}.json"))
        assert sorted(meta) == ["catalogs", "counts", "id_to_size_map", "inertia", "n_iter"]
        assert meta["id_to_size_map"]["4"] == "16x16" and meta["id_to_size_map"]["9"] == "64x64"
        arrays = np.load(dest / "cluster_arrays" / f"{k}.npz")
        assert sorted(arrays.files, key=int) == [str(layer) for layer in layers] + ["10"]
        assert arrays["10"].shape == (8, 3, 64, 64) and arrays["10"].dtype == np.uint8
        pal = S.palette(k).numpy()
        for layer in layers:
            m = found[k][layer]
            centres = np.load(meta["catalogs"][str(layer)])
            assert np.array_equal(centres, m.cluster_centers_) and centres.shape == (k, 512)
            assert sum(meta["counts"][str(layer)]) == m.labels_.numel() and meta["n_iter"][str(layer)] == m.n_iter_
            size = int(meta["id_to_size_map"][str(layer)].split("x")[0])
            want = pal[m.labels_.cpu().numpy().reshape(8, size, size)].transpose(0, 3, 1, 2)
            assert np.array_equal(arrays[str(layer)], want)
        from PIL import Image
        png = Image.open(dest / "cluster_images" / f"{k}.png")
        assert png.size == (8 * 64, 7 * 64)
    with pytest.raises(NotImplementedError):
        S.main(S.build_parser().parse_args(["-i", "some/dir"]))
    # the json's "catalogs" entry is what the dataset CLI's config takes: its label maps are FactorCatalog.predict's
    meta = json.load(open(dest / "catalogs" / "3.json"))
    config = {"image_size": 64, "catalogs": {"9": meta["catalogs"]["9"]}, "seed": 1}
    seen = {}
    original = D.label_and_encode

    def spy(image, acts, catalogs, dataset_gan=None):
        out = original(image, acts, catalogs, dataset_gan)
        if out[2] is not None:
            out[2].synchronize()
        seen["labels"], seen["act"] = out[1][9].clone(), acts[9].clone()
        return out

    D.label_and_encode = spy
    try:
        torch.manual_seed(0)
        D.build_dataset(argparse.Namespace(checkpoint=None, num_images=4, batch_size=4, truncate=False, save_to=None), config)
    finally:
        D.label_and_encode = original
    cat = FactorCatalog(cluster_centers=np.load(meta["catalogs"]["9"]))
    assert torch.equal(seen["labels"], cat.predict(seen["act"]))
