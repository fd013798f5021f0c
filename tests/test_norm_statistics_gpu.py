"""The normalisation kernels (csrc/group_norm.hip, bn_ops.hip, layer_norm.hip, weight_std.hip) through the public ``sis_hip``
wrappers against the float64 references of norm_statistics_cases.py, on the input families where statistics go wrong unnoticed --
offset (|mean| / std up to 4096), a different mean per plane / per slice / per row, constant inputs, variance far below eps --
with the element-wise bounds whose K was measured on the CPU restatement (test_norm_statistics_cpu.py, which also shows that a
one-pass variance, a wrong Chan cross term, a mis-counted short slice, a misplaced eps or a biased running variance break these
bounds by 10 x and more).  Shapes: the smallest that reach each kernel form (norm_statistics_cases.CASES)."""
import numpy as np
import pytest
import torch

import norm_statistics_cases as N

pytestmark = pytest.mark.gpu


def _t(a, device, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device).to(dtype)


def _op(case, A, device, dtype=torch.float32):
    return _t(N.from_canon(case.op, A, case.shape, case.groups), device, dtype)


def _canon(case, t):
    a = t.detach().double().cpu().numpy()
    if case.op != "rows":
        a = a.reshape(case.shape[0], case.shape[1], -1)
    return N.to_canon(case.op, a, case.groups)


def _vec(t):
    return t.detach().double().cpu().numpy()


class Report:
    """Collects the figure (the K a result would need) of every family and fails once, with all of them."""

    def __init__(self, case):
        self.case, self.lines, self.bad = case, [], []

    def add(self, tag, inp, out, **kw):
        for k, v in N.ratios(self.case, inp, out, **kw).items():
            self.lines.append(f"{tag} {k} {v:.3g}")
            if not v <= self.case.K:
                self.bad.append(f"{tag}: {k} needs K = {v:.3g}")

    def finish(self):
        print(f"{self.case.id} (K = {self.case.K}): " + "; ".join(self.lines))
        assert not self.bad, f"{self.case.id}, K = {self.case.K}: " + "; ".join(self.bad)


# ------------------------------------------------------------------------------------------------------------ GroupNorm

def _group_norm(case, inp, device, dtype):
    import sis_hip
    td = torch.bfloat16 if dtype == "bf16" else torch.float32
    groups, eps, relu = case.groups, case.eps, inp["relu"]
    x = _op(case, inp["X"], device, td)
    gamma, beta = _t(inp["gamma"], device), _t(inp["beta"], device)
    out = {}
    if inp["res"] is not None:   # the residual form: fp32 output, the gate as one bit per element, 16-bit copy of a 16-bit input
        res, gy = _op(case, inp["res"], device), _op(case, inp["g"], device)
        if dtype == "bf16":
            y, mean, rstd, y_lp, gate = sis_hip.group_norm_fwd(x, gamma, beta, groups, eps, relu, residual=res, low_precision_copy=True,
                                                               want_gate=True)
            assert torch.equal(y_lp, y.to(td))
            out["y_lp"] = _canon(case, y_lp)
        else:
            y, mean, rstd, gate = sis_hip.group_norm_fwd(x, gamma, beta, groups, eps, relu, residual=res, want_gate=True)
        dx, dg, db, dres = sis_hip.group_norm_bwd(gy, x, mean, rstd, gamma, beta, groups, relu, want_residual_grad=True, gate=gate)
        via_y = sis_hip.group_norm_bwd(gy, x, mean, rstd, gamma, beta, groups, relu, y_mask=y, want_residual_grad=True)
        for u, v in zip((dx, dg, db, dres), via_y):
            assert torch.equal(u, v)   # the gate bits and the saved output are the same gate
        assert np.array_equal(_canon(case, dres), inp["ref"]["gp"])   # the residual's gradient IS the gated gradient
    else:
        gy = _op(case, inp["g"], device, td)
        y, mean, rstd = sis_hip.group_norm_fwd(x, gamma, beta, groups, eps, relu, out_dtype=torch.float32)
        if dtype == "bf16":
            y_lp, m2, r2 = sis_hip.group_norm_fwd(x, gamma, beta, groups, eps, relu)
            assert y_lp.dtype == td and torch.equal(m2, mean) and torch.equal(r2, rstd)
            out["y_lp"] = _canon(case, y_lp)
        dx, dg, db = sis_hip.group_norm_bwd(gy, x, mean, rstd, gamma, beta, groups, relu)
    assert dx.dtype == td
    out.update(y=_canon(case, y), mean=_vec(mean), rstd=_vec(rstd), dx=_canon(case, dx), dgamma=_vec(dg), dbeta=_vec(db))
    return out


_GN_RUNS = [(c, d, r, f) for c in N.CASES if c.op == "gn" for d in c.dtypes for r in c.relu
            for f in ((True, False) if c.slicing == "gn" else (True,))]


@pytest.mark.parametrize("case,dtype,relu,fused", _GN_RUNS, ids=[f"{c.id}-{d}-{'relu' if r else 'plain'}-{'fused' if f else 'own_launch'}"
                                                                  for c, d, r, f in _GN_RUNS])
def test_group_norm_statistics(device, monkeypatch, case, dtype, relu, fused):
    """GroupNorm forward and backward on every family: unsliced vector / flat / scalar apply forms, planes of two slices (even,
    and 131 x 127 with a short last slice), the merge inside the statistics launch and as its own launch, the residual + gate +
    16-bit-copy form, and (bf16, hw % 512 == 0) the single-pass group kernels at each of their three iteration counts."""
    import sis_hip
    monkeypatch.setattr(sis_hip, "_GN_FUSED_FINISH", fused)
    rep = Report(case)
    u16 = N.U_BF16 if dtype == "bf16" else N.U32
    for fam in N.FAMILIES:
        for residual in ((False, True) if (relu and case.residual) else (False,)):
            inp = N.build_inputs(case, fam, dtype, relu, residual)
            rep.add(f"{fam}{'+res' if residual else ''}", inp, _group_norm(case, inp, device, dtype), u_dx=u16)
    assert sis_hip.group_counters_are_zero()
    rep.finish()


# ------------------------------------------------------------------------------------------------------------ batch-norm mode

_BN_RUNS = [(c, r, f) for c in N.CASES if c.op == "bn" for r in c.relu for f in (True, False)]


@pytest.mark.parametrize("case,relu,fused", _BN_RUNS, ids=[f"{c.id}-{'relu' if r else 'plain'}-{'fused' if f else 'own_launch'}" for c, r, f in _BN_RUNS])
def test_batch_norm_mode_statistics(device, monkeypatch, case, relu, fused):
    """Batch-norm mode of csrc/group_norm.hip: (sample, slice) merge by the completing wave and by its own launch, more samples
    than merging lanes, sliced planes; running statistics from non-trivial starting values."""
    import sis_hip
    monkeypatch.setattr(sis_hip, "_GN_FUSED_FINISH", fused)
    rep = Report(case)
    for fam in N.FAMILIES:
        inp = N.build_inputs(case, fam, "f32", relu)
        x, gy = _op(case, inp["X"], device), _op(case, inp["g"], device)
        gamma, beta = _t(inp["gamma"], device), _t(inp["beta"], device)
        rm, rv = _t(inp["rm0"], device), _t(inp["rv0"], device)
        y, mean, rstd = sis_hip.batch_norm_train_fwd(x, gamma, beta, rm, rv, case.eps, N.MOMENTUM, relu)
        dx, dg, db = sis_hip.batch_norm_train_bwd(gy, x, mean, rstd, gamma, beta, relu)
        rep.add(fam, inp, dict(y=_canon(case, y), mean=_vec(mean), rstd=_vec(rstd), rm=_vec(rm), rv=_vec(rv), dx=_canon(case, dx),
                               dgamma=_vec(dg), dbeta=_vec(db)))
    assert sis_hip.group_counters_are_zero()
    rep.finish()


# ------------------------------------------------------------------------------------------------------------ bn_ops.hip

_BO_RUNS = [(c, r, s) for c in N.CASES if c.op == "bnops" for r, s in ((False, False), (True, False), (True, True), (False, True))]
_BO_KERNELS = {   # what the library reports having launched (forward, backward)
    "bnops_fused": ({"bn_fused_fwd_kernel"}, {"bn_wide_bwd_kernel", "bn_fused_bwd_kernel"}),
    "bnops_wide": ({"bn_wide_fwd_kernel"}, {"bn_wide_bwd_kernel"}),
    "bnops_three_launch": (None, {"bn_bwd_reduce_kernel+bn_bwd_apply_kernel"}),
}


@pytest.mark.parametrize("case,relu,residual", _BO_RUNS, ids=[f"{c.id}-{'relu' if r else 'plain'}{'-res' if s else ''}" for c, r, s in _BO_RUNS])
def test_bn_ops_statistics(device, case, relu, residual):
    """EMANet / DocUFCN batch norm, each form directly against float64: fused (a channel in one 256-thread workgroup), wide
    (16 385 ... 65 536 values per channel), three-launch (slices of 16 384, here a short last one); with and without residual,
    ReLU, and the one-bit gate mask (which must give bitwise what the saved output gives)."""
    import sis_hip
    rep = Report(case)
    fwd_names, bwd_names = _BO_KERNELS[case.id]
    for fam in N.FAMILIES:
        inp = N.build_inputs(case, fam, "f32", relu, residual)
        x, gy = _op(case, inp["X"], device), _op(case, inp["g"], device)
        res = _op(case, inp["res"], device) if residual else None
        gamma, beta = _t(inp["gamma"], device), _t(inp["beta"], device)
        rm, rv = _t(inp["rm0"], device), _t(inp["rv0"], device)
        assert sis_hip.bn_supported(x) and sis_hip.bn_fused_supported(x) == (fwd_names is not None)
        records = []
        sis_hip.set_profiler(records)
        try:
            if fwd_names:
                y, mean, invstd, mask = sis_hip.bn_fused_fwd(x, res, gamma, beta, rm, rv, case.eps, N.MOMENTUM, relu, want_mask=True)
            else:
                mean, invstd = sis_hip.bn_stats(x, rm, rv, case.eps, N.MOMENTUM)
                y, mask = sis_hip.bn_act_fwd(x, res, mean, invstd, gamma, beta, relu, want_mask=True)
            n_fwd = len(records)
            dx, dres, dg, db = sis_hip.bn_act_bwd(gy, y, x, mean, invstd, gamma, relu, residual)
        finally:
            sis_hip.set_profiler(None)
        if fwd_names:
            assert {r[0] for r in records[:n_fwd]} == {next(iter(fwd_names))}
        assert {r[0] for r in records[n_fwd:]} <= bwd_names and len(records) > n_fwd
        if relu:
            via_mask = sis_hip.bn_act_bwd(gy, None, x, mean, invstd, gamma, relu, residual, mask=mask)
            for u, v in zip((dx, dres, dg, db), via_mask):
                assert (u is None and v is None) or torch.equal(u, v)
        if residual:
            assert np.array_equal(_canon(case, dres), inp["ref"]["gp"])
        rep.add(fam, inp, dict(y=_canon(case, y), mean=_vec(mean), rstd=_vec(invstd), rm=_vec(rm), rv=_vec(rv), dx=_canon(case, dx),
                               dgamma=_vec(dg), dbeta=_vec(db)))
    rep.finish()


# ------------------------------------------------------------------------------------------------------------ LayerNorm

@pytest.mark.parametrize("case", [c for c in N.CASES if c.bwd == "ln"], ids=lambda c: c.id)
def test_layer_norm_statistics(device, case):
    """LayerNorm rows of 256 / 768 / 1024 (one, three and four vectors per lane), five rows = two workgroups, every row with its
    own offset in the 'between' family: forward with fp32 and bf16 output, backward alone and with the residual gradient fused."""
    import sis_hip
    rep = Report(case)
    for fam in N.FAMILIES:
        inp = N.build_inputs(case, fam)
        x, gy, radd = _op(case, inp["X"], device), _op(case, inp["g"], device), _op(case, inp["radd"], device)
        gamma, beta = _t(inp["gamma"], device), _t(inp["beta"], device)
        assert sis_hip.layer_norm_supported(x, case.shape[1])
        y, mean, rstd = sis_hip.layer_norm_fwd(x, gamma, beta, case.eps)
        y_lp, m2, r2 = sis_hip.layer_norm_fwd(x, gamma, beta, case.eps, out_dtype=torch.bfloat16)
        assert y_lp.dtype == torch.bfloat16 and torch.equal(m2, mean) and torch.equal(r2, rstd)
        dx, dg, db = sis_hip.layer_norm_bwd(gy, x, mean, rstd, gamma)
        dxf, dgf, dbf, cast = sis_hip.layer_norm_bwd_fused(gy, x, mean, rstd, gamma, residual_grad=radd)
        assert cast is None and torch.equal(dg, dgf) and torch.equal(db, dbf)
        rep.add(fam, inp, dict(y=_canon(case, y), y_lp=_canon(case, y_lp), mean=_vec(mean), rstd=_vec(rstd), dx=_canon(case, dx),
                               dx_fused=_canon(case, dxf), dgamma=_vec(dg), dbeta=_vec(db)))
    rep.finish()


# ------------------------------------------------------------------------------------------------------------ weight standardisation

@pytest.mark.parametrize("case", [c for c in N.CASES if c.fwd == "ws"], ids=lambda c: c.id)
def test_weight_std_statistics(device, case):
    """Weight standardisation, rows of 27 / 64 / 784 weights (less than, a fraction of, and more than one 256-thread sweep), both
    directions, fp32 and bf16 output; a constant row standardises to exactly zero."""
    import sis_hip
    rep = Report(case)
    for fam in N.FAMILIES:
        inp = N.build_inputs(case, fam)
        w, gy = _op(case, inp["X"], device), _op(case, inp["g"], device)
        w_hat, invstd = sis_hip.weight_std_fwd(w, case.eps)
        w_lp, i2 = sis_hip.weight_std_fwd(w, case.eps, out_dtype=torch.bfloat16)
        assert w_lp.dtype == torch.bfloat16 and torch.equal(i2, invstd)
        dw = sis_hip.weight_std_bwd(gy, w, invstd, case.eps)
        if fam == "const_64":
            assert not w_hat.any() and not w_lp.any()
        if fam == "const_plane":
            assert not w_hat[0].any() and w_hat[1:].any()
        out = dict(y=_canon(case, w_hat), y_lp=_canon(case, w_lp), rstd=_vec(invstd), dx=_canon(case, dw))
        rep.add(fam, inp, out)
    rep.finish()
