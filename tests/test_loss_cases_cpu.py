"""The fp32 restatement of the loss kernels (loss_restatement.py) against the float64 references and bounds of loss_cases.py:
(1) the float64 references agree with torch's float64 autograd where torch defines the operation; (2) on every case the
restatement stays within the bounds -- this is where the K of each family and quantity is measured
(``python tests/test_loss_cases_cpu.py`` prints the figures; K = 4 x the largest); (3) each named mistake of the restatement
exceeds a bound by at least 10 x on the case named in FAULTS, i.e. the GPU tests, which hold the kernels to the same bounds,
would notice it; (4) the inputs are what their names say; (5) in the late-training regime a loss of 0 and a loss of twice the
reference are both outside the bound, i.e. the bound is smaller than the loss it guards.

No fault models a missing edge guard in ``lerp_index`` (the clamp of i0 to in - 1, i1 = i0 + (i0 < in - 1)): it is unobservable
by a value test.  The clamp of i0 never acts: src = fl(fl((in - 1) / (out - 1)) dst) <= (in - 1) (1 + 2 u) < in, so
(int) src <= in - 1 already.  Without the guard on i1, the one pixel whose src rounds to in - 1 or an ulp above would read index
``in`` with weight l1 <= ulp(in - 1) ~ 1e-6: a read past the row, but no value any bound could see (and nothing a numpy
restatement can index).  ``lerp_lambda_fused`` models the lambda taken from an unrounded product: src - i0 contracted into
fma(scale, dst, -i0) is a negative 1e-7 where the rounded product is an integer, and gives cell i1 a share it does not have."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import loss_cases as L
import loss_restatement as R


CE_DICE_G = (1.0, -0.25)    # d(loss) of the ce_dice backward; the other two families carry theirs in the inputs


def restate(case, inp, fault=None):
    if case.family == "ce_dice":
        runs = {g: R.ce_dice(inp["z"], inp["labels"], g, case.dtype == "bf16", fault) for g in CE_DICE_G}
        return dict(runs[1.0], grad={g: r["grad"] for g, r in runs.items()})
    if case.family == "upsample_ce":
        return R.upsample_ce(inp["x"], inp["labels"], inp["size"], L.IGNORE, inp["gloss"], fault)
    return R.wce(inp["z"], inp["labels"], inp["weight"], inp["g"], fault)


# ------------------------------------------------------------------------------------------------------------ references vs torch

@pytest.mark.parametrize("labels_kind", ["in_range", "with_ignore"])
@pytest.mark.parametrize("C", [2, 5])
def test_ce_dice64_is_the_updaters_objective(C, labels_kind):
    """ce_dice64 == 0.5 F.cross_entropy(ignore_index=-100) + 0.5 DiceLoss(softmax=True) (networks/trans_u_net/utils.py, re-expressed
    in float64: the module builds its one-hot rows in float32), value and torch.autograd gradient."""
    rng = np.random.default_rng(C)
    B, n = 2, 24
    z = rng.standard_normal((B, C, n)) * 3
    labels = rng.integers(0, C, size=(B, n))
    if labels_kind == "with_ignore":
        labels[rng.random((B, n)) < 0.2] = -100
    zt = torch.from_numpy(z).requires_grad_(True)
    lt = torch.from_numpy(labels)
    ce = F.cross_entropy(zt, lt, ignore_index=-100)
    p = torch.softmax(zt, dim=1)
    t = (lt.unsqueeze(1) == torch.arange(C).view(1, -1, 1)).double()
    dice = (1 - (2 * (p * t).sum((0, 2)) + 1e-5) / ((p * p).sum((0, 2)) + (t * t).sum((0, 2)) + 1e-5)).sum() / C
    loss = 0.5 * ce + 0.5 * dice
    loss.backward()
    got = L.ce_dice64(z, labels)
    for u, v in zip(got[:3], (loss, ce, dice)):
        assert abs(u - v.item()) <= 1e-14 * (1 + abs(v.item()))
    assert np.abs(got[3] - zt.grad.numpy()).max() <= 1e-15


def test_ce_dice64_without_a_valid_label():
    z = np.random.default_rng(0).standard_normal((1, 3, 8))
    loss, ce, dice, dz = L.ce_dice64(z, np.full((1, 8), -100))
    assert ce == 0.0 and np.isfinite(loss) and np.isfinite(dz).all() and loss == 0.5 * dice


@pytest.mark.parametrize("geom", list(L.UPSAMPLE_GEOMS), ids=list(L.UPSAMPLE_GEOMS))
def test_upsample_ce64_against_torch(geom):
    """upsample_ce64 == F.interpolate(float64, align_corners=True) + log_softmax + nll_loss(ignore) + mean, to 2e-6 relative: torch's
    float64 kernel computes the source index in float64, the operator here (and torch's float32 kernel) in float32, which moves
    every lambda by up to ~(in - 1) 2^-24."""
    (h, w), (H, W) = L.UPSAMPLE_GEOMS[geom]
    rng = np.random.default_rng(h + W)
    B, C = 3, 4
    x = rng.standard_normal((B, C, h, w)) * 2
    labels = rng.integers(0, C, size=(B, H, W))
    labels[rng.random((B, H, W)) < 0.1] = L.IGNORE
    gl = np.asarray(L.GLOSS)
    xt = torch.from_numpy(x).requires_grad_(True)
    pred = F.interpolate(xt, size=(H, W), mode="bilinear", align_corners=True)
    ref = F.nll_loss(F.log_softmax(pred, dim=1), torch.from_numpy(labels), ignore_index=L.IGNORE, reduction="none").mean(dim=2).mean(dim=1)
    (gref,) = torch.autograd.grad(ref, xt, torch.from_numpy(gl))
    loss, dx = L.upsample_ce64(x, labels, (H, W), L.IGNORE, gl)
    assert np.abs(loss - ref.detach().numpy()).max() <= 2e-6 * np.abs(ref.detach().numpy()).max()
    assert np.abs(dx - gref.numpy()).max() <= 2e-6 * np.abs(gref.numpy()).max()


@pytest.mark.parametrize("weighted", [False, True])
def test_wce64_against_torch(weighted):
    rng = np.random.default_rng(3)
    B, C, n = 2, 5, 40
    z = rng.standard_normal((B, C, n)) * 3
    labels = rng.integers(0, C, size=(B, n))
    labels[rng.random((B, n)) < 0.2] = -100
    wt = rng.uniform(0.0, 3.0, size=C) if weighted else None
    zt = torch.from_numpy(z).requires_grad_(True)
    ref = F.cross_entropy(zt, torch.from_numpy(labels), weight=None if wt is None else torch.from_numpy(wt), ignore_index=-100)
    ref.backward()
    loss, dz = L.wce64(z, labels, wt)
    assert abs(loss - ref.item()) <= 1e-14 * abs(ref.item())
    assert np.abs(dz - zt.grad.numpy()).max() <= 1e-16


# ------------------------------------------------------------------------------------------------------------ the restatement within the bounds

def groups():
    out = {}
    for c in L.CASES:
        out.setdefault((c.family, c.shape_id, c.C, c.dtype), []).append(c)
    return out


GROUPS = groups()


def figures(cases):
    worst = {}
    for case in cases:
        inp = L.build(case)
        for k, v in L.ratios(case, inp, restate(case, inp)).items():
            if v > worst.get(k, (-1.0,))[0]:
                worst[k] = (v, case.id)
    return worst


@pytest.mark.parametrize("key", list(GROUPS), ids=["-".join(map(str, k)) for k in GROUPS])
def test_restatement_within_bounds(key):
    """Every case: each result within its bound at its K, and at least a factor 2 inside it (K is 4 x the largest figure: a
    restatement that drifts towards K is reported before the bound fails)."""
    worst = figures(GROUPS[key])
    print(key, {k: (round(v[0], 3), v[1]) for k, v in worst.items()})
    for k, (v, cid) in worst.items():
        assert v <= L.K(key[0], k) / 2, f"{cid}: {k} needs K = {v:.3g}, its K is {L.K(key[0], k)}"


# (fault, the case that shows it, the result that shows it)
FAULTS = [
    ("no_max_subtract", "ce_dice-b-C3-f32-wide-uniform", "ce"),                       # exp(100) overflows: inf / inf
    ("no_max_subtract", "upsample_ce-up-C2-f32-wide-uniform", "loss"),
    ("no_max_subtract", "wce-p2049-C5-f32-wide-uniform-w_random", "loss"),
    ("valid_counts_all_pixels", "ce_dice-b-C3-f32-randn3-ignored10", "ce"),          # the mean divides by 1 200, not by ~1 080
    ("dice_row_for_out_of_range_label", "ce_dice-b-C3-f32-randn3-ignored10", "dice"),  # -100 counted as class 0, C as class C - 1
    ("smooth_missing_in_b", "ce_dice-b-C3-f32-randn3-absent", "b"),                  # I_c = 0: b_c is all smooth term
    ("drop_last_quad", "ce_dice-a-C2-f32-randn3-uniform", "ce"),                     # the only quad
    ("finish_drops_last_range", "ce_dice-c-C2-f32-randn3-ignored10", "ce"),          # rows 63, 64 of 65
    ("stride_loop_single_pass", "ce_dice-d-C2-f32-randn3-ignored10", "ce"),          # quads 131 072 .. 131 328
    ("footprint_one_short", "upsample_ce-up-C2-f32-randn3-uniform", "grad"),         # the last pixel row feeds the last cell row
    ("lerp_lambda_fused", "upsample_ce-up-C21-f32-wide-uniform", "grad"),            # a cell next to the footprint gets 2e-11, not 1e-26
    ("weight_sum_counts_ignored", "wce-p2049-C5-f32-randn3-ignored10-w_random", "loss"),
    ("weight_missing_in_grad", "wce-p2049-C5-f32-randn3-uniform-w_random", "grad"),
]


@pytest.mark.parametrize("fault,case_id,key", FAULTS, ids=[f"{f}-{c.split('-')[0]}" for f, c, _ in FAULTS])
def test_faults_are_caught(fault, case_id, key):
    case = L.CASE[case_id]
    inp = L.build(case)
    k = L.K(case.family, key)
    good = L.ratios(case, inp, restate(case, inp))[key]
    bad = L.ratios(case, inp, restate(case, inp, fault))[key]     # (a NaN counts as caught: figure inf)
    print(f"{fault}: {key} on {case_id}: {bad / k:.3g} x the bound (sound restatement: {good / k:.3g} x)")
    assert good <= k
    assert bad >= 10 * k, f"{fault} is only {bad / k:.3g} x the bound of {key} on {case_id}"


def _labels_of(case):
    return int(np.prod(case.geom)) if case.family != "upsample_ce" else len(L.GLOSS) * int(np.prod(case.geom[1]))


LATE = [c for c in L.CASES if c.logits == "late" and 1 < c.C <= 8 and _labels_of(c) > 1]


@pytest.mark.parametrize("case", LATE, ids=[c.id for c in LATE])
def test_late_bound_is_smaller_than_the_loss(case):
    """Late training: a cross entropy of 0 and one of twice the reference are both outside the bound, in every family, at every
    class count up to 8 and every size but a single pixel.  The two exemptions are fp32's, not the bound's: s = 1 + delta
    lies on a grid of 1.2e-7, so ONE pixel at NLL 1e-7 cannot be told from 0 by any fp32 kernel; and at 21 and 32 classes the
    kernels' sum over the classes in class order adds terms of 1e-6 / C < 6e-8 to 1 one by one and loses them, an error of up to
    u C that reaches the loss itself (only a sum that starts with the small terms would do better)."""
    inp = L.build(case)
    key = "ce" if case.family == "ce_dice" else "loss"
    ref = np.asarray(inp["ref"][key])
    assert (ref > 0).any()
    for wrong in (0.0 * ref, 2.0 * ref):
        fig = L.ratios(case, inp, {key: wrong})[key]
        assert fig > L.K(case.family, key), f"{case.id}: {key} := {wrong} needs only K = {fig:.3g}"


# ------------------------------------------------------------------------------------------------------------ the inputs are what they say

def _nll_and_valid(case, inp):
    r = inp["ref"]
    ok = r["valid"] if case.family != "wce" else r["wy"] > 0
    return r["nll"], ok


@pytest.mark.parametrize("key", list(GROUPS), ids=["-".join(map(str, k)) for k in GROUPS])
def test_inputs_are_what_they_say(key):
    for case in GROUPS[key]:
        inp = L.build(case)
        r = inp["ref"]
        nll, ok = _nll_and_valid(case, inp)
        lab = inp["labels"]
        C = case.C
        in_range = (lab >= 0) & (lab < C)
        if case.family == "upsample_ce":
            assert (in_range | (lab == L.IGNORE)).all(), "upsample_ce takes labels in [0, C) and the ignore index only"
        if case.labels == "ignored10":     # (loss_cases.make_labels: below 10 labels exactly one is replaced, a single label is not)
            if lab.size >= 10:
                assert 0.8 <= in_range.mean() < 1.0, case.id
            else:
                assert (~in_range).sum() == (1 if lab.size >= 2 else 0), case.id
        if case.labels in ("absent", "absent_unpredicted") and C > 1:
            assert not (lab == C - 1).any() and r["t"][:, C - 1].sum() == 0, case.id     # T_c = 0
        if case.labels == "absent_unpredicted":
            assert r["P"][C - 1] < 1e-30 and r["Dn"][C - 1] < 1.001e-5, case.id
        if case.labels == "all_ignored":
            assert not in_range[L.IGNORED_SAMPLE if case.family == "upsample_ce" else slice(None)].any(), case.id
        if case.logits == "late" and C > 1 and ok.any():
            assert 1e-7 <= nll[ok].min() and nll[ok].max() <= 1e-5, (case.id, nll[ok].min(), nll[ok].max())
        if case.logits == "sat_right" and C > 1 and ok.any():
            gap = 25.0 - (0.25 if case.dtype == "bf16" else 1e-3)    # (bf16: two roundings on the grid of 1 / 8 at 16..32)
            assert nll[ok].max() <= (C - 1) * np.exp(-gap), case.id              # (C - 1 classes, each at least 25 below)
        if case.logits == "sat_wrong" and C > 1 and ok.any():
            assert nll[ok].min() > 24, case.id
        if case.logits == "ties":
            assert np.ptp(r["sp"]["p"]) == 0
        if case.weight == "zero_class":
            assert inp["weight"][0] == 0 and (lab == 0).any()
        for k in ("loss", "ce", "dice", "dz", "dx", "a", "b"):
            if k in r and not (case.family == "wce" and r["Wsum"] == 0 and k == "loss"):
                assert np.isfinite(r[k]).all(), (case.id, k)


def test_ce_dice_cases_cover_every_instantiation():
    pairs = {(c.C, c.dtype) for c in L.CASES if c.family == "ce_dice"}
    assert pairs == {(C, d) for C in range(2, 9) for d in ("f32", "bf16")}
    for C, d in pairs:
        assert {"a", "b"} <= {c.shape_id for c in L.CASES if c.family == "ce_dice" and (c.C, c.dtype) == (C, d)}


if __name__ == "__main__":   # the K table
    by_k = {}
    for key, cases in GROUPS.items():
        worst = figures(cases)
        print("-".join(map(str, key)).ljust(34) + "  ".join(f"{k} {v[0]:.3f}" for k, v in worst.items()))
        for k, (v, cid) in worst.items():
            name = L.K_OF[key[0]][k]
            if v > by_k.get(name, (-1.0,))[0]:
                by_k[name] = (v, k, cid)
    for name, (v, k, cid) in sorted(by_k.items()):
        print(f"{name}: largest figure {v:.3f} ({k}, {cid}) -> K = {4 * v:.2f}; in the module: {getattr(L, name)}")
