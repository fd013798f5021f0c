"""The fp32 restatement of the norm kernels (norm_restatement.py) against the float64 references and bounds of
norm_statistics_cases.py: (1) on every family and shape it stays within the bounds -- this is where the K of each kernel form
is measured (``python tests/test_norm_statistics_cpu.py`` prints the figures; K = 4 x the largest); (2) each deliberately
defective restatement exceeds a bound by at least 10 x on the family named in the parametrisation, i.e. the GPU tests, which
apply the same bounds to the kernels, would notice that defect; (3) the ReLU cases keep every pre-activation a margin away from
zero, with no element excluded."""
import numpy as np
import pytest

import norm_restatement as R
import norm_statistics_cases as N


def slice_len(case):
    L = N.canon_shape(case.op, case.shape, case.groups)[2]
    return {"gn": R.gn_slice_len(L), "bn3": R.BN_SLICE, None: None}[case.slicing]


def restate(case, inp, defect=None):
    """One forward + backward of the restatement, results in the canonical layout under the keys of ``N.ratios``."""
    sl, X, gc, bc, relu = slice_len(case), inp["X"], inp["gc"], inp["bc"], inp["relu"]
    fw = R.forward(X, gc, bc, case.eps, sl, case.fwd, relu, inp["res"], defect)
    out = dict(y=fw["y"], mean=fw["mean"], rstd=fw["rstd"])
    if inp["dtype"] == "bf16":
        out["y_lp"] = N.round_bf16(fw["y"])
    if case.running:
        out["rm"], out["rv"] = R.running_update(fw["mean"], fw["m2"], fw["n"], inp["rm0"], inp["rv0"], N.MOMENTUM, defect)
    saved = None if (case.op in ("gn", "bn") and inp["res"] is None) else fw["y"]   # GroupNorm recomputes its gate, bn_ops reads y
    bw = R.backward(X, inp["g"], fw["mean"], fw["rstd"], gc, bc, sl, case.bwd, relu, saved, case.bn_mode)
    out["dx"] = bw["dx"]
    if case.bwd == "ln":
        out["dgamma"], out["dbeta"] = bw["dgamma"], bw["dbeta"]
        out["dx_fused"] = R.backward(X, inp["g"], fw["mean"], fw["rstd"], gc, bc, sl, "ln", radd=inp["radd"])["dx"]
    elif case.op == "gn":
        out["dgamma"], out["dbeta"] = R.gn_param_grads(bw, case.shape[0], case.shape[1])
    elif case.running:
        out["dgamma"], out["dbeta"] = bw["s2"], bw["s1"]
    return out


def variants(case):
    for dtype in case.dtypes:
        for relu in case.relu:
            yield dtype, relu, False
            if case.residual and (relu or case.op == "bnops"):   # (GroupNorm's residual form always has the ReLU)
                yield dtype, relu, True


def figures(case):
    worst = {}
    for dtype, relu, residual in variants(case):
        for fam in N.FAMILIES:
            inp = N.build_inputs(case, fam, dtype, relu, residual)
            for k, v in N.ratios(case, inp, restate(case, inp)).items():
                if v > worst.get(k, (0.0,))[0]:
                    worst[k] = (v, fam, dtype, relu, residual)
    return worst


@pytest.mark.parametrize("case", N.CASES, ids=lambda c: c.id)
def test_restatement_within_bounds(case):
    """Every family, dtype, ReLU / residual variant: each result within its bound at the form's K, and at least a factor 2 inside
    it (K is 4 x the measured figure: a restatement that drifts towards K is reported before the bound fails)."""
    worst = figures(case)
    print(case.id, {k: (round(v[0], 3),) + v[1:] for k, v in worst.items()})
    for k, v in worst.items():
        assert v[0] <= case.K / 2, f"{case.id}: {k} needs K = {v[0]:.3g} on {v[1:]}, the form's K is {case.K}"


@pytest.mark.parametrize("case", [c for c in N.CASES if True in c.relu], ids=lambda c: c.id)
def test_relu_cases_keep_their_margin(case):
    """No gate can flip within the bound: every pre-activation of every ReLU case, residual included, is at least RELU_MARGIN
    output bounds from zero -- over ALL elements (the share of excluded elements is 0), and the families keep their character
    (the constant inputs are still constant)."""
    assert case.K <= N.K_RELU
    for dtype, relu, residual in variants(case):
        if not relu:
            continue
        for fam in N.FAMILIES:
            inp = N.build_inputs(case, fam, dtype, True, residual)
            gamma, beta = inp["gamma"], inp["beta"]
            assert N.relu_margin_ok(case.op, case.shape, case.groups, inp["X"], gamma, beta, inp["res"], case.eps), (case.id, fam)
            if fam in ("const_64", "const_0p1"):
                assert np.ptp(inp["X"]) == 0
            if fam.startswith("offset"):
                ref = inp["ref"]
                assert (np.abs(ref["mean"]) * ref["rstd"] > 100).all(), (case.id, fam)


# (defect, case, family, the result that shows it, measured error / bound at the form's K -- at least 10 is asserted)
DEFECTS = [
    ("one_pass", "gn_vector", "offset_m4096", "rstd", 1.0e3),          # E[x^2] - E[x]^2 at |mean| / std = 4096: negative, rstd NaN
    ("no_cross", "gn_vector", "between", "rstd", 2.91e7),              # the variance IS the cross term
    ("cross_nb_nt", "gn_vector", "between", "rstd", 2.13e6),           # delta^2 nb / nt instead of delta^2 n nb / nt
    ("unweighted_mean", "bnops_three_launch", "halves", "mean", 1.85e5),  # four slices of 16 384 and one of 4 096
    ("eps_outside", "gn_vector", "scale_lo", "rstd", 3.88e6),          # 1 / (sqrt(var) + eps): var << eps shows where eps sits
    ("biased_running", "bn_mode", "control", "rv", 1.92e3),            # m2 / n into running_var at n = 192
    ("count_sl", "gn_two_slices_odd", "offset_m4096", "mean", 210.0),  # the last slice holds 8 317 elements, not sl = 8 320
]


@pytest.mark.parametrize("defect,case_id,fam,key,measured", DEFECTS, ids=[d[0] for d in DEFECTS])
def test_defective_restatements_are_caught(defect, case_id, fam, key, measured):
    case = N.CASE[case_id]
    inp = N.build_inputs(case, fam, "f32")
    good = N.ratios(case, inp, restate(case, inp))[key]
    with np.errstate(invalid="ignore"):
        bad = N.ratios(case, inp, restate(case, inp, defect), finite=False)[key]   # (a NaN counts as caught: figure inf)
    print(f"{defect}: {key} on {case_id} / {fam}: {bad / case.K:.3g} x the bound (sound restatement: {good / case.K:.3g} x)")
    assert good <= case.K
    assert bad >= 10 * case.K, f"{defect} is only {bad / case.K:.3g} x the bound of {key} on {case_id} / {fam}"
    assert bad / case.K >= measured / 3, "the recorded factor is stale"


if __name__ == "__main__":   # the K table
    by_form = {}
    for case in N.CASES:
        worst = figures(case)
        top = max(worst.items(), key=lambda kv: kv[1][0])
        print(f"{case.id:22s} {case.kname:11s} " + "  ".join(f"{k} {v[0]:.2f}" for k, v in worst.items()))
        if top[1][0] > by_form.get(case.kname, (0.0,))[0]:
            by_form[case.kname] = (top[1][0], case.id, top[0]) + top[1][1:]
    for k, v in by_form.items():
        print(f"{k}: largest figure {v[0]:.3f} ({v[1:]}) -> K = {4 * v[0]:.2f}; in the module: {getattr(N, k)}")
