"""The six bilinear-upsampling kernels (csrc/upsample_ops.hip) through the public wrappers -- ``sis_hip.upsample_bilinear``,
``upsample2x_into``, ``upsample2x_grad_from``, ``HipUpsamplingBilinear2d`` -- against the float64 references of upsample_cases.py:
the float32 index rule with float64 arithmetic after it, so the only error left is the kernel's own fp32 arithmetic, held per
element to K u32 A + B with the K measured on the CPU restatement (test_upsample_cases_cpu.py, which also shows that a wrong
scale, an unclamped or half-weighted edge, a short window, a neighbour from the wrong side of a wave boundary, a dense plane
offset in the strided entry and a weighted column -1 break these bounds by 10 x and more).

Every shape names the kernel each direction must run (upsample_cases.SHAPES) and the test asserts it through
``sis_last_kernel()`` BEFORE it compares a value: every kernel is reached in-process by shape alone, in f32, bf16 and f16.
Per case: unit noise, noise on an offset of 1e3, a constant (within 2 ulp of the output type), ramps along both axes (the output
is the float32 source coordinate), one-hot x and gy (exactly 0.0 outside the footprint the rule names); the figure on the whole
map and on every edge, wave-boundary and tile-boundary region; <up x, gy> = <x, up^T gy> and sum gx = sum gy; bitwise repeatable.

The process-wide switch of the direct kernels (the tiled-kernel A/B run of test_switches_gpu.py) is none of this file's business;
with it set the route assertions here fail, as they should."""
import numpy as np
import pytest
import torch

import upsample_cases as U

pytestmark = pytest.mark.gpu

TORCH = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


def _np(t):
    return t.detach().double().cpu().numpy()


def _dev(a, case, device):
    return torch.from_numpy(a).to(device).to(TORCH[case.dtype])      # (exact: the case's values are values of its type)


def _last_kernel():
    import sis_hip
    return sis_hip.lib().sis_last_kernel().decode()


class Report:
    """Collects the figure (the K a result would need) of every case and region and fails once, with all of them."""

    def __init__(self):
        self.lines, self.bad = [], []

    def add(self, case, inp, y, gx):
        fig = U.figures(case, inp, y, gx)
        worst = {}
        for k, v in fig.items():
            kern = U.kernel_of(case, k)
            if not v <= U.K[kern]:
                self.bad.append(f"{case.id}: {k} needs K = {v:.3g} (K of {kern} = {U.K[kern]})")
            which = k.split("/")[0]
            if v >= worst.get(which, (-1.0,))[0]:
                worst[which] = (v, k)
        self.lines.append(f"{case.data} " + " ".join(f"{k} {v:.3g}" for _, (v, k) in sorted(worst.items())))
        self.bad += U.exact_checks(case, inp, y, gx)
        if not case.data.startswith("hot"):
            self.bad += U.identity_checks(case, inp, y, gx)

    def finish(self):
        print("; ".join(self.lines))
        assert not self.bad, "; ".join(self.bad)


GROUPS = {}
for _c in U.CASES:
    GROUPS.setdefault((_c.shape_id, _c.dtype), []).append(_c)


@pytest.mark.parametrize("key", list(GROUPS), ids=["-".join(k) for k in GROUPS])
def test_upsample_cases(device, key):
    """Every shape of upsample_cases.SHAPES in one dtype, both directions, every data family: the kernel that ran, then every
    element against its bound (whole map and regions), the exact checks, the identities; finite; bitwise repeatable."""
    import sis_hip as S
    rep = Report()
    for case in GROUPS[key]:
        inp = U.build(case)
        x, gy = _dev(inp["x"], case, device), _dev(inp["gy"], case, device)
        y = S.upsample_bilinear(x, *case.size)
        assert _last_kernel() == case.fwd, f"{case.id}: the forward ran {_last_kernel()}, not {case.fwd}"
        gx = S.upsample_bilinear(x, *case.size, grad_output=gy)
        assert _last_kernel() == case.bwd, f"{case.id}: the backward ran {_last_kernel()}, not {case.bwd}"
        assert y.dtype == x.dtype and tuple(y.shape) == case.shape[:2] + case.size and gx.dtype == x.dtype and gx.shape == x.shape
        assert torch.equal(y, S.upsample_bilinear(x, *case.size)), f"{case.id}: the forward is bitwise repeatable"
        assert torch.equal(gx, S.upsample_bilinear(x, *case.size, grad_output=gy)), f"{case.id}: the backward is bitwise repeatable"
        assert torch.isfinite(y).all() and torch.isfinite(gx).all(), case.id
        rep.add(case, inp, _np(y), _np(gx))
    rep.finish()


def test_down_sampling_is_accepted(device):
    """9 x 10 -> 4 x 7 goes through the wrapper (no exception) on the generic kernels: the case gen_down above holds its values."""
    import sis_hip as S
    case = U.CASE["gen_down-f32-noise"]
    inp = U.build(case)
    y = S.upsample_bilinear(_dev(inp["x"], case, device), *case.size)
    assert tuple(y.shape) == (1, 2, 4, 7) and _last_kernel() == U.GEN_F


STRIDED_GROUPS = {}
for _c in U.STRIDED_CASES:
    STRIDED_GROUPS.setdefault((_c.shape_id, _c.dtype), []).append(_c)


@pytest.mark.parametrize("key", list(STRIDED_GROUPS), ids=["-".join(k) for k in STRIDED_GROUPS])
def test_strided_entry(device, key):
    """``upsample2x_into`` / ``upsample2x_grad_from`` on a direct and a tiled shape with extra channels: the leading channels held
    to the float64 reference itself (not to the dense call), the extra channels bitwise untouched, the kernel asserted."""
    import sis_hip as S
    rep = Report()
    for case in STRIDED_GROUPS[key]:
        inp = U.build(case)
        B, C, h, w = case.shape
        rng = np.random.default_rng(11)
        fill = U.round_to(rng.standard_normal((B, C + case.extra, 2 * h, 2 * w)) + 7.0, case.dtype)
        wide = _dev(fill, case, device)
        before = wide.clone()
        x = _dev(inp["x"], case, device)
        S.upsample2x_into(wide, x)
        assert _last_kernel() == case.fwd, f"{case.id}: the forward ran {_last_kernel()}, not {case.fwd}"
        assert torch.equal(wide[:, C:], before[:, C:]), f"{case.id}: the extra channels were written"
        again = before.clone()
        S.upsample2x_into(again, x)
        assert torch.equal(again, wide)
        gwide = before.clone()
        gwide[:, :C] = _dev(inp["gy"], case, device)
        gkeep = gwide.clone()
        gx = S.upsample2x_grad_from(gwide, C)
        assert _last_kernel() == case.bwd, f"{case.id}: the backward ran {_last_kernel()}, not {case.bwd}"
        assert torch.equal(gwide, gkeep) and torch.equal(gx, S.upsample2x_grad_from(gwide, C))
        rep.add(case, inp, _np(wide[:, :C]), _np(gx))
    rep.finish()


@pytest.mark.parametrize("dtype", U.DTYPES)
def test_module_autograd(device, dtype):
    """``HipUpsamplingBilinear2d(scale_factor=2)`` under autograd on the direct shape 6 x 32: the same bounds end to end.  (Only
    the forward's kernel is asserted: the library keeps the name per thread, and autograd runs the backward on a thread of its
    own; test_upsample_cases holds the backward's route at this shape.)"""
    from networks.hip_upsample import HipUpsamplingBilinear2d
    case = U.CASE[f"direct_6x32-{dtype}-noise"]
    inp = U.build(case)
    x = _dev(inp["x"], case, device).requires_grad_(True)
    y = HipUpsamplingBilinear2d(scale_factor=2)(x)
    assert _last_kernel() == case.fwd
    y.backward(_dev(inp["gy"], case, device))
    assert x.grad.dtype == x.dtype and x.grad.shape == x.shape
    rep = Report()
    rep.add(case, inp, _np(y), _np(x.grad))
    rep.finish()
