"""The three loss-kernel families (csrc/loss_ops.hip, seg_ops.hip, doc_ufcn.hip) through the public ``sis_hip`` wrappers against
the float64 references of loss_cases.py, on the inputs where a loss goes wrong unnoticed -- a per-pixel offset of +-60, saturated
pixels (right and wrong), the late-training regime (NLL ~ 1e-6), exact ties, logits 200 apart, labels outside [0, C), classes that
are absent or absent and unpredicted, a batch / a sample without one valid label -- at the smallest shapes that reach each
path (loss_cases.CASES), with the element-wise bounds whose K was measured on the CPU restatement (test_loss_cases_cpu.py, which
also shows that a missing max-subtraction, a wrong valid count, a clamped out-of-range label, a Dice constant without its smooth
term, a dropped quad / finish range / second pass, a short footprint and two weight mistakes break these bounds by 10 x and more)."""
import numpy as np
import pytest
import torch

import loss_cases as L

pytestmark = pytest.mark.gpu

CE_DICE_G = (1.0, -0.25)


def _np(t):
    return t.detach().double().cpu().numpy()


def groups(family):
    out = {}
    for c in L.CASES:
        if c.family == family:
            out.setdefault((c.shape_id, c.C, c.dtype), []).append(c)
    return out


class Report:
    """Collects the figure (the K a result would need) of every case and fails once, with all of them."""

    def __init__(self, family):
        self.family, self.lines, self.bad = family, [], []

    def add(self, case, inp, out):
        for k, v in L.ratios(case, inp, out).items():
            self.lines.append(f"{case.logits}/{case.labels}{'/' + str(case.weight) if case.family == 'wce' else ''} {k} {v:.3g}")
            if not v <= L.K(self.family, k):
                self.bad.append(f"{case.id}: {k} needs K = {v:.3g} (K = {L.K(self.family, k)})")

    def finish(self):
        print("; ".join(self.lines))
        assert not self.bad, "; ".join(self.bad)


# ------------------------------------------------------------------------------------------------------------ ce_dice

def _ce_dice_inputs(case, inp, device):
    z = torch.from_numpy(inp["z"]).to(device)
    if case.dtype == "bf16":
        z = z.to(torch.bfloat16)       # (exact: the case's logits are bf16 values)
    return z, torch.from_numpy(inp["labels"]).to(device)


def _ce_dice_run(case, inp, device):
    import sis_hip as S
    z, lab = _ce_dice_inputs(case, inp, device)
    assert S.ce_dice_supported(z, lab)
    out, stats = S.ce_dice_fwd(z, lab)
    out2, stats2 = S.ce_dice_fwd(z, lab)
    assert torch.equal(out, out2) and torch.equal(stats, stats2), "the forward is bitwise repeatable"
    grads = {}
    for g in CE_DICE_G:
        gt = torch.tensor(g, device=device)
        gr = S.ce_dice_bwd(gt, z, lab, stats)
        assert gr.dtype == z.dtype and gr.shape == z.shape
        assert torch.equal(gr, S.ce_dice_bwd(gt, z, lab, stats)), "the backward is bitwise repeatable"
        grads[g] = _np(gr)
    o, s = _np(out), _np(stats)
    return dict(loss=o[0], ce=o[1], dice=o[2], inv_valid=s[0], a=s[1::2], b=s[2::2], grad=grads)


CE_DICE_GROUPS = groups("ce_dice")


@pytest.mark.parametrize("key", list(CE_DICE_GROUPS), ids=["-".join(map(str, k)) for k in CE_DICE_GROUPS])
def test_ce_dice_cases(device, key):
    """Every class count 2..8 in f32 and bf16, both directions: (a) one quad, (b) a ragged second workgroup, and at C = 2, 8
    (c) 65 workgroups -> a short and ten empty finish ranges, (d) the grid-stride loop with a ragged second pass.  The three loss
    values, 1 / n_valid, a_c, b_c and the gradient at d(loss) = 1 and -0.25; a batch without a valid label has ce == 0 exactly,
    everything finite, and the Dice-only gradient (the reference's, by the same bound)."""
    rep = Report("ce_dice")
    for case in CE_DICE_GROUPS[key]:
        inp = L.build(case)
        out = _ce_dice_run(case, inp, device)
        for k, v in out.items():
            for a in (v.values() if isinstance(v, dict) else (v,)):
                assert np.isfinite(a).all(), f"{case.id}: {k} is not finite"
        if case.labels == "all_ignored":
            assert out["ce"] == 0.0 and out["inv_valid"] == 0.0, case.id
        rep.add(case, inp, out)
    rep.finish()


def test_ce_dice_cases_launch_all_28_instantiations():
    """7 class counts x 2 dtypes, and test_ce_dice_cases runs the forward and the backward kernel of each."""
    pairs = {(C, d) for (_, C, d) in CE_DICE_GROUPS}
    assert len(pairs) == 14 and pairs == {(C, d) for C in range(2, 9) for d in ("f32", "bf16")}
    for C, d in pairs:
        assert {"a", "b"} <= {s for (s, c2, d2) in CE_DICE_GROUPS if (c2, d2) == (C, d)}
    assert {s for (s, C, d) in CE_DICE_GROUPS if C in (2, 8)} == {"a", "b", "c", "d"}


def test_ce_dice_late_through_the_updater_function(device):
    """The autograd function the TransUNet updater calls, on a late-training batch (loss ~ 1e-6): value and gradient end to end."""
    from updater.segmentation_updater import _CeDiceFn
    case = L.CASE["ce_dice-b-C3-f32-late-uniform"]
    inp = L.build(case)
    z, lab = _ce_dice_inputs(case, inp, device)
    z.requires_grad_(True)
    loss, parts = _CeDiceFn.apply(z, lab)
    loss.backward()
    o = _np(parts)
    assert loss.item() == o[0] and 0 < o[1] < 1e-5
    rep = Report("ce_dice")
    rep.add(case, inp, dict(loss=o[0], ce=o[1], dice=o[2], grad={1.0: _np(z.grad)}))
    rep.finish()


# ------------------------------------------------------------------------------------------------------------ upsample_ce

UPSAMPLE_GROUPS = groups("upsample_ce")


@pytest.mark.parametrize("key", list(UPSAMPLE_GROUPS), ids=["-".join(map(str, k)) for k in UPSAMPLE_GROUPS])
def test_upsample_ce_cases(device, key):
    """C = 1, 2, 21, 32 on: each axis degenerate alone, upsampling, downsampling (the other footprint branch), identity, 9 cells
    (idle lane groups shadow the last cell), 272 cells (17 workgroups).  Per-sample loss and dx; the sample without a valid
    label has loss 0 and a zero gradient, the sample with d(loss) = 0 a gradient that is exactly zero; bitwise repeatable."""
    import sis_hip as S
    rep = Report("upsample_ce")
    for case in UPSAMPLE_GROUPS[key]:
        inp = L.build(case)
        x, lab, gl = torch.from_numpy(inp["x"]).to(device), torch.from_numpy(inp["labels"]).to(device), torch.from_numpy(inp["gloss"]).to(device)
        loss = S.upsample_ce_fwd(x, lab, inp["size"], L.IGNORE)
        gx = S.upsample_ce_bwd(gl, x, lab, inp["size"], L.IGNORE)
        assert torch.equal(loss, S.upsample_ce_fwd(x, lab, inp["size"], L.IGNORE))
        assert torch.equal(gx, S.upsample_ce_bwd(gl, x, lab, inp["size"], L.IGNORE))
        assert torch.isfinite(loss).all() and torch.isfinite(gx).all(), case.id
        zero = L.GLOSS.index(0.0)
        assert not gx[zero].any(), f"{case.id}: d(loss) = 0 must give a zero gradient"
        if case.labels == "all_ignored":
            assert loss[L.IGNORED_SAMPLE].item() == 0.0 and not gx[L.IGNORED_SAMPLE].any(), case.id
            assert case.C == 1 or gx[0].any()
        rep.add(case, inp, dict(loss=_np(loss), grad=_np(gx)))
    rep.finish()


def test_upsample_ce_late_through_the_network_tail(device):
    """The autograd function EMANet's tail calls, on a late-training batch: per-sample loss and gradient end to end."""
    from networks.ema_net.network import _UpsampleCrossEntropy
    case = L.CASE["upsample_ce-up-C2-f32-late-uniform"]
    inp = L.build(case)
    x = torch.from_numpy(inp["x"]).to(device).requires_grad_(True)
    loss = _UpsampleCrossEntropy.apply(x, torch.from_numpy(inp["labels"]).to(device), inp["size"], L.IGNORE)
    loss.backward(torch.from_numpy(inp["gloss"]).to(device))
    assert (loss > 0).all() and (loss < 1e-5).all()
    rep = Report("upsample_ce")
    rep.add(case, inp, dict(loss=_np(loss), grad=_np(x.grad)))
    rep.finish()


# ------------------------------------------------------------------------------------------------------------ wce

WCE_GROUPS = groups("wce")


def _wce_inputs(inp, device):
    z = torch.from_numpy(inp["z"]).to(device).unsqueeze(2)       # [B, K, 1, HW]
    lab = torch.from_numpy(inp["labels"]).to(device).unsqueeze(1)
    wt = None if inp["weight"] is None else torch.from_numpy(inp["weight"]).to(device)
    return z, lab, wt


@pytest.mark.parametrize("key", list(WCE_GROUPS), ids=["-".join(map(str, k)) for k in WCE_GROUPS])
def test_weighted_ce_cases(device, key):
    """K = 1, 2, 5, 32 at P = 1, 255 (< 256: one pixel per range, an empty range), 258 (the second image starts inside a range) and
    2 049 (ranges of 9, a short one, 28 empty); weight None, random, and one labelled class at weight 0.  Loss and gradient; pixels
    of the zero-weight class and pixels with an out-of-range label have a gradient that is exactly zero.

    With EVERY label out of range (all_ignored) the gradient must be exactly zero; the loss is 0 / 0 there: the kernel returns
    NaN (0.f / 0.f in wce_finish_kernel), and so does F.cross_entropy (mean reduction over no element).  No value is asserted for it."""
    import sis_hip as S
    rep = Report("wce")
    for case in WCE_GROUPS[key]:
        inp = L.build(case)
        z, lab, wt = _wce_inputs(inp, device)
        loss, stats = S.weighted_ce_fwd(z, lab, wt)
        gz = S.weighted_ce_bwd(torch.tensor(inp["g"], device=device), z, lab, wt, stats)
        labels = inp["labels"]
        dead = (labels < 0) | (labels >= case.C)
        if case.weight == "zero_class":
            dead = dead | (labels == 0)
        g = _np(gz)[:, :, 0, :]
        assert np.isfinite(g).all(), case.id
        assert not g.transpose(0, 2, 1)[dead].any(), f"{case.id}: pixels without weight must have a zero gradient"
        assert case.labels != "all_ignored" or dead.all()
        if inp["ref"]["Wsum"] == 0:     # all_ignored
            assert not g.any()
            print(f"{case.id}: loss with no weight at all = {loss.item()}")
            rep.add(case, inp, dict(grad=g))
        else:
            assert torch.isfinite(loss).all(), case.id
            rep.add(case, inp, dict(loss=_np(loss)[0], grad=g))
    rep.finish()


def test_weighted_ce_late_through_the_updater_function(device):
    """``weighted_cross_entropy`` as DocUFCN's updater calls it, on a late-training batch: loss and gradient end to end."""
    from updater.segmentation_updater import weighted_cross_entropy
    case = L.CASE["wce-p2049-C5-f32-late-uniform-w_random"]
    inp = L.build(case)
    z, lab, wt = _wce_inputs(inp, device)
    z.requires_grad_(True)
    loss = weighted_cross_entropy(z, lab, wt)
    assert 0 < loss.item() < 1e-5
    loss.backward(torch.tensor(inp["g"], device=device))
    rep = Report("wce")
    rep.add(case, inp, dict(loss=loss.item(), grad=_np(z.grad)[:, :, 0, :]))
    rep.finish()
