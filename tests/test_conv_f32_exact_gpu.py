"""GPU, bit for bit: the fp32 convolution family -- Winograd F(2x2,3x3) forward and data gradient (csrc/modconv_wino.hip through
``sis_conv3x3``), its weight gradient (csrc/conv_wgrad_wino.hip), the pointwise forward / data gradient / ``dgrad_add``
(csrc/conv1x1_f32.hip), the pointwise weight gradient (csrc/conv1x1_wgrad_f32.hip), the queued launches and the wrappers of
networks/hip_conv.py -- on exactly summable operands (tests/exact_operands.py).  v_mfma_f32_32x32x2_f32 is a true fp32 fma and
the F(2x2,3x3) transforms only add and halve, so with bounded integers every result IS float64 ``F.conv2d`` / its autograd on
the CPU, in any split-K plan, slab order or tile plan: no tolerance anywhere; a mismatch is reported with its bounding box
modulo the tile.  The wide cases carry 12-bit matrix-core operands, which an operand path that drops mantissa bits would spoil.

Cases, claimed routes and references: tests/conv_f32_exact_cases.py (CPU only; tests/test_conv_f32_exact_cpu.py checks the
claims, the operand rules and the sensitivity of the cases).  Here every observable route fact -- the kernel name the library
records, the eligibility entries, the workspace size of the pointwise weight gradient -- is held against the restated plans
(tests/conv_f32_plan.py)."""
import contextlib
import itertools

import pytest
import torch

import conv_f32_exact_cases as C
import conv_f32_plan as P
import exact_operands as E

pytestmark = pytest.mark.gpu

WGRAD_KERNEL, PWG_KERNEL = "conv_wgrad_wino_kernel", "conv1x1_wgrad_f32_kernel"


@contextlib.contextmanager
def _recorded():
    """The kernel names the library reports for the launches inside, and no fallback to the ROCm libraries among them."""
    import sis_hip
    records, names = [], []
    sis_hip.library_calls(reset=True)
    sis_hip.set_profiler(records)
    try:
        yield names
    finally:
        sis_hip.set_profiler(None)
    names.extend(r[0] for r in records)
    calls = sis_hip.library_calls(reset=True)
    assert calls["fallback"] == {}, calls


def _conv3x3_both_ways(device, c, shape, what):
    """Forward on the prepacked image, data gradient on the adjoint image with the channel counts transposed."""
    import sis_hip as S
    batch, cin, cout, h, w = shape
    assert S.WORKSPACE_BYTES == P.WORKSPACE_BYTES
    wd = c["w"].to(device)
    for x, image, ref, dims, name in ((c["x"], S.conv3x3_prepack(wd), c["y"], (batch, cin, cout, h, w), "forward"),
                                      (c["gy"], S.conv3x3_prepack(wd, adjoint=True), c["dx"], (batch, cout, cin, h, w), "data gradient")):
        route = P.wino_forward_route(*dims)
        assert bool(S.lib().sis_conv3x3_eligible(*dims)) and route is not None
        with _recorded() as names:
            got = S.conv3x3(x.to(device), image)
        assert names == [route["kernel"]], (name, names, route)
        E.assert_bitwise(got, E.exact_f32(ref), f"{what} {name} {shape}", route["tile"])


@pytest.mark.parametrize("batch,cin,cout,h,w", list(C.FORWARD_CASES))
def test_winograd_forward_and_data_gradient_exact(device, batch, cin, cout, h, w):
    shape = (batch, cin, cout, h, w)
    _conv3x3_both_ways(device, C.forward_case(*shape), shape, "Winograd")


@pytest.mark.parametrize("mirrored", [False, True])
def test_winograd_forward_wide_operands_exact(device, mirrored):
    _conv3x3_both_ways(device, C.wide_forward_case(mirrored), C.WIDE_FORWARD_SHAPE, f"Winograd wide (mirrored={mirrored})")


def test_eligibility_entries_agree_with_the_restated_plans(device):
    """``sis_conv3x3_eligible``, ``sis_conv3x3_wgrad_eligible`` (with workspaces around the slab size), ``sis_conv1x1_f32_supported``,
    ``sis_conv1x1_wgrad_f32_supported`` and the workspace size / (4 cout cin) = slice count of the pointwise weight gradient, on a
    grid of shapes on both sides of every rule (host code only: nothing is launched)."""
    import sis_hip as S
    L = S.lib()
    for b, ci, co, h, w in itertools.product((1, 4, 9, 300), (8, 12, 32, 64), (4, 6, 64, 72), (1, 2, 6, 16, 20, 64, 256), (2, 4, 8, 12, 128, 512)):
        assert bool(L.sis_conv3x3_eligible(b, ci, co, h, w)) == P.wino_forward_eligible(b, ci, co, h, w), (b, ci, co, h, w)
    for b, ci, co, h, w in itertools.product((1, 3, 8), (64, 96, 128), (64, 128), (2, 3, 6, 8, 16), (2, 8, 10, 26, 28)):
        slab = 64 * ci * co
        for ws in (P.WORKSPACE_BYTES, slab, slab - 1, 3 * slab):
            assert bool(L.sis_conv3x3_wgrad_eligible(b, ci, co, h, w, ws)) == (P.wino_wgrad_plan(b, ci, co, h, w, ws) is not None), (b, ci, co, h, w, ws)
    for ci, co, hw in itertools.product((16, 32, 64, 96), (30, 32, 64, 160), (4, 6, 80, 132)):
        assert bool(L.sis_conv1x1_f32_supported(ci, co, hw)) == P.pointwise_supported(ci, co, hw), (ci, co, hw)
    for b, ci, co, hw in itertools.product((1, 3, 5, 16), (32, 64, 128, 256), (64, 128, 256, 512), (32, 64, 128)):
        assert bool(L.sis_conv1x1_wgrad_f32_supported(b, ci, co, hw)) == P.pwg_supported(b, ci, co, hw), (b, ci, co, hw)
        assert int(L.sis_conv1x1_wgrad_f32_workspace(b, ci, co, hw)) == P.pwg_workspace(b, ci, co, hw), (b, ci, co, hw)
    for (b, ci, co, h, w) in C.POINTWISE_WGRAD_CASES:
        plan = P.pwg_plan(b, ci, co, h * w)
        assert int(L.sis_conv1x1_wgrad_f32_workspace(b, ci, co, h * w)) // (4 * co * ci) == (plan["ksplit"] if plan["ksplit"] > 1 else 0)


def _wgrad3(device, c, shape, what):
    import sis_hip as S
    assert S.conv3x3_wgrad_supported(*shape) and P.wino_wgrad_plan(*shape) is not None
    with _recorded() as names:
        got = S.conv3x3_wgrad(c["x"].to(device), c["gy"].to(device))
    assert names == [WGRAD_KERNEL], names
    E.assert_bitwise(got, E.exact_f32(c["dw"]), f"{what} {shape}")


@pytest.mark.parametrize("batch,cin,cout,h,w", list(C.WGRAD_CASES))
def test_winograd_weight_gradient_exact(device, batch, cin, cout, h, w):
    """Every plan of ``wgrad_plan``: 1, 2 and 3 chunks in all, slices that end in 1, 2, 3 chunks, odd and even slices, with and
    without the reduce kernel, tile rows and samples of 1, 3, 5, 7 tiles, 2-pixel-wide and 2-pixel-high images."""
    _wgrad3(device, C.wgrad_case(batch, cin, cout, h, w), (batch, cin, cout, h, w), "Winograd weight gradient")


@pytest.mark.parametrize("mirrored", [False, True])
def test_winograd_weight_gradient_wide_operands_exact(device, mirrored):
    _wgrad3(device, C.wide_wgrad_case(mirrored), C.WIDE_WGRAD_SHAPE, f"Winograd weight gradient wide (mirrored={mirrored})")


@pytest.mark.parametrize("kind,jobs,shape", list(C.BATCHED_CASES))
def test_queued_weight_gradients_exact(device, kind, jobs, shape):
    """Layers of one shape through ``_defer_conv_wgrad`` + ``flush_deferred``: every layer against float64 (not against the
    single-layer kernel), whatever slices the joint plan cuts."""
    import sis_hip as S
    batch, cin, cout, h, w = shape
    c = C.batched_case(kind, jobs, shape)
    k = 3 if kind == "f3" else 1
    dims = shape if kind == "f3" else (batch, cin, cout, h * w)
    xs, gys = [x.to(device) for x, _ in c["layers"]], [gy.to(device) for _, gy in c["layers"]]
    dws = [torch.full((cout, cin, k, k), float("nan"), device=device) for _ in range(jobs)]
    assert S.deferred_pending() == 0
    for x, gy, dw in zip(xs, gys, dws):
        S._defer_conv_wgrad(kind, x, gy, dw, dims)
    assert S.deferred_pending() == jobs
    with _recorded() as names:
        S.flush_deferred()
    assert S.deferred_pending() == 0
    assert names == [WGRAD_KERNEL if kind == "f3" else PWG_KERNEL], names      # (one binding call per shape; it cuts the launches)
    for j in range(jobs):
        E.assert_bitwise(dws[j], E.exact_f32(c["dw"][j]), f"queued {kind} weight gradient {shape}, layer {j} of {jobs}")


def _pointwise_both_ways(device, c, shape, what):
    import sis_hip as S
    batch, cin, cout, h, w = shape
    xd, wd, gd = c["x"].to(device), c["w"].to(device), c["gy"].to(device)
    bd = None if c.get("bias") is None else c["bias"].to(device)
    assert S.conv1x1_f32_supported(xd, wd) and S.conv1x1_f32_supported(gd, wd)
    fwd, dgrad = P.pointwise_plan(batch, cin, cout, h * w), P.pointwise_plan(batch, cin, cout, h * w, True)
    with _recorded() as names:
        y = S.conv1x1_f32(xd, wd, bd)
        dx = S.conv1x1_f32(gd, wd, data_gradient=True)
    assert names == [fwd["kernel"], dgrad["kernel"]], (names, fwd, dgrad)
    E.assert_bitwise(y.flatten(2), E.exact_f32(c["y"]).flatten(2), f"{what} forward {shape}", fwd["npix"])
    E.assert_bitwise(dx.flatten(2), E.exact_f32(c["dx"]).flatten(2), f"{what} data gradient {shape}", dgrad["npix"])
    return gd, wd, dgrad


@pytest.mark.parametrize("batch,cin,cout,h,w,bias", list(C.POINTWISE_CASES))
def test_pointwise_forward_and_data_gradient_exact(device, batch, cin, cout, h, w, bias):
    import sis_hip as S
    shape = (batch, cin, cout, h, w)
    c = C.pointwise_case(batch, cin, cout, h, w, bias)
    gd, wd, dgrad = _pointwise_both_ways(device, c, shape, "pointwise")
    if (batch, cin, cout, h, w, bias) in C.DGRAD_ADD_CASES:
        with _recorded() as names:
            got = S.conv1x1_f32_dgrad_add(gd, wd, c["skip"].to(device))
        assert names == [dgrad["kernel"]], names
        E.assert_bitwise(got.flatten(2), E.exact_f32(c["dx_add"]).flatten(2), f"pointwise dgrad_add {shape}", dgrad["npix"])


@pytest.mark.parametrize("mirrored", [False, True])
def test_pointwise_wide_operands_exact(device, mirrored):
    _pointwise_both_ways(device, C.wide_pointwise_case(mirrored), C.WIDE_POINTWISE_SHAPE, f"pointwise wide (mirrored={mirrored})")


def _wgrad1(device, c, shape, what):
    import sis_hip as S
    xd, gd = c["x"].to(device), c["gy"].to(device)
    assert S.conv1x1_wgrad_f32_supported(gd, xd)
    with _recorded() as names:
        got = S.conv1x1_wgrad_f32(gd, xd)
    assert names == [PWG_KERNEL], names
    E.assert_bitwise(got, E.exact_f32(c["dw"]), f"{what} {shape}")


@pytest.mark.parametrize("batch,cin,cout,h,w", list(C.POINTWISE_WGRAD_CASES))
def test_pointwise_weight_gradient_exact(device, batch, cin, cout, h, w):
    _wgrad1(device, C.pointwise_wgrad_case(batch, cin, cout, h, w), (batch, cin, cout, h, w), "pointwise weight gradient")


@pytest.mark.parametrize("mirrored", [False, True])
def test_pointwise_weight_gradient_wide_operands_exact(device, mirrored):
    _wgrad1(device, C.wide_pointwise_wgrad_case(mirrored), C.WIDE_POINTWISE_WGRAD_SHAPE, f"pointwise weight gradient wide (mirrored={mirrored})")


# ---- through networks.hip_conv

def _layer_exact(device, c, run, what, must_run, unit=1.0):
    """forward, dx and dw of ``run(x, w)`` bitwise; ``must_run``: kernel names that have to be among the recorded launches."""
    xd = c["x"].to(device).requires_grad_(True)
    wd = c["w"].to(device).requires_grad_(True)
    with _recorded() as names:
        y = run(xd, wd)
        y.backward(c["gy"].to(device))
    for kernel in must_run:
        assert any(n.startswith(kernel) for n in names), (kernel, names)
    E.assert_bitwise(y, E.exact_f32(c["y"], unit), what + " y", (16, 16))
    E.assert_bitwise(xd.grad, E.exact_f32(c["dx"], unit), what + " dx", (16, 16))
    E.assert_bitwise(wd.grad, E.exact_f32(c["dw"], unit), what + " dw")


@pytest.mark.parametrize("shape,dilation", C.DILATED_CASES)
def test_dilated_conv3x3_exact(device, shape, dilation):
    """Dilation by space-to-batch: d * d ordinary convolutions of the stride-d sub-images, in all three directions."""
    import sis_hip as S
    from networks.hip_conv import conv3x3
    c = C.dilated_case(shape, dilation)
    assert S.conv3x3_supported(c["x"].to(device), c["w"].to(device), dilation)
    _layer_exact(device, c, lambda x, w: conv3x3(x, w, dilation), f"conv3x3 {shape} dilation {dilation}", ["modconv_wino", WGRAD_KERNEL])


def _module_exact(device, conv, c, what, must_run):
    with torch.no_grad():
        conv.weight.copy_(c["w"].to(device))
    conv.weight.grad = None
    xd = c["x"].to(device).requires_grad_(True)
    with _recorded() as names:
        y = conv(xd)
        y.backward(c["gy"].to(device))
    for kernel in must_run:
        assert any(n.startswith(kernel) for n in names), (kernel, names)
    E.assert_bitwise(y, E.exact_f32(c["y"]), what + " y", (16, 16))
    E.assert_bitwise(xd.grad, E.exact_f32(c["dx"]), what + " dx", (16, 16))
    E.assert_bitwise(conv.weight.grad, E.exact_f32(c["dw"]), what + " dw")


def test_half_image_dilation_layer_exact(device):
    """Gather kernel + the pointwise kernels in all three directions, nothing on the ROCm libraries."""
    from networks.hip_conv import HipConv2d
    batch, cin, cout, h, w = C.HALF_DILATION_CASE
    conv = HipConv2d(cin, cout, 3, 1, h // 2, h // 2, bias=False).to(device)
    assert conv._half_image_dilation(torch.zeros(batch, cin, h, w, device=device))
    _module_exact(device, conv, C.half_dilation_case(), "half-image dilation", ["conv1x1_f32_kernel", PWG_KERNEL])


@pytest.mark.parametrize("shape,k", C.STRIDE2_CASES)
def test_stride_2_layers_exact(device, shape, k):
    """Stride 2 by sampling: the dense 3x3 layer at the even pixels, the 1x1 layer on the sampled input."""
    from networks.hip_conv import HipConv2d
    conv = HipConv2d(shape[1], shape[2], k, 2, k // 2, bias=False).to(device)
    must = ["modconv_wino", WGRAD_KERNEL] if k == 3 else ["conv1x1_f32_kernel", PWG_KERNEL]
    _module_exact(device, conv, C.stride2_case(shape, k), f"HipConv2d k={k} stride 2 {shape}", must)


def test_down_conv3x3_exact(device):
    """Blur + stride-2 convolution as one convolution over the pixel phases: results are multiples of 2^-9."""
    from networks.hip_conv import down_conv3x3, down_conv3x3_supported
    c = C.down_case()
    fir = c["fir"].to(device)
    assert down_conv3x3_supported(c["x"].to(device), c["w"].to(device), fir)
    _layer_exact(device, c, lambda x, w: down_conv3x3(x, w, fir, c["scale"]), f"down_conv3x3 {C.DOWN_CASE}", ["modconv_wino", WGRAD_KERNEL], c["unit"])


def test_second_order_terms_exact(device):
    """``_Conv3x3Backward`` differentiated once more: d gy = conv(ggx, W) + conv(x, ggW), d x = dgrad(gy, ggW), d W = wgrad(ggx, gy)."""
    from networks.hip_conv import _Conv3x3Backward
    c = C.second_order_case()
    gy, x, w = (c[k].to(device).requires_grad_(True) for k in ("gy", "x", "w"))
    with _recorded() as names:
        dx, dw = _Conv3x3Backward.apply(gy, x, w, 1, True, True, None, None, False)
        d_gy, d_x, d_w = torch.autograd.grad((dx, dw), (gy, x, w), (c["ggx"].to(device), c["ggw"].to(device)))
    assert names.count(WGRAD_KERNEL) == 2 and sum(n.startswith("modconv_wino") for n in names) == 4, names
    what = f"second order {C.SECOND_ORDER_CASE} "
    E.assert_bitwise(dx, E.exact_f32(c["dx"]), what + "dx", (4, 8))
    E.assert_bitwise(dw, E.exact_f32(c["dw"]), what + "dw")
    E.assert_bitwise(d_gy, E.exact_f32(c["d_gy"]), what + "d gy", (4, 8))
    E.assert_bitwise(d_x, E.exact_f32(c["d_x"]), what + "d x", (4, 8))
    E.assert_bitwise(d_w, E.exact_f32(c["d_w"]), what + "d W")
