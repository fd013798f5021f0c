"""GPU, bit for bit: the bf16 convolutions (csrc/conv_bf16.hip), their weight gradients (csrc/conv_bf16_wgrad.hip, 3x3 and 1x1,
single and batched) and the 7x7 stem (csrc/stem_conv.hip) on exactly summable operands (tests/exact_operands.py): integer
images, filters and gradients keep every fp32 partial sum exact, so an fp32 result IS float64 ``F.conv2d`` / its autograd on
the CPU and a bf16 result IS the round-to-nearest-even image of it -- no tolerance.

The shapes are the smallest that reach each path of ``conv_plan``: M tile 32 / 64 / 128 (by cout), tile width 32 / 64 (by
wo <= 32), channel chunk 16 or 64 (flat 1x1), the ragged output-channel tile, the unaligned staging path, stride 2.

The case builders run on the CPU only; tests/test_exact_operands_cpu.py imports them for the rounding-path conditions."""
import functools

import pytest
import torch

import exact_operands as E

pytestmark = pytest.mark.gpu

BIAS_R = 64

FORWARD_CASES = [
    # batch, cin, cout, h, w, k, stride, bias
    (1, 16, 3, 24, 40, 3, 1, True),       # M tile 32, ragged channel tile (3 of 32), tile 64 wide, bias
    (1, 32, 48, 20, 28, 3, 1, False),     # M tile 64 (ragged: 48), tile 32 wide
    (1, 16, 136, 33, 31, 3, 1, False),    # M tile 128, second tile ragged (8 of 128), odd plane: unaligned staging
    (1, 48, 64, 9, 70, 3, 1, False),      # M tile 64 whole, tile 64 wide, ragged in x, width % 4 != 0
    (2, 64, 72, 20, 28, 1, 1, False),     # flat 1x1 (chunk 64), M tile 128 ragged, two images
    (1, 64, 64, 15, 17, 1, 1, True),      # flat 1x1, 255 pixels: unaligned, bias
    (1, 32, 80, 31, 31, 3, 2, False),     # stride 2, M tile 128 ragged, odd map
    (1, 16, 64, 63, 63, 1, 2, False),     # 1x1 stride 2 (chunk 16), M tile 64
    (1, 32, 64, 63, 63, 1, 2, False),     # the same path with two chunks: see SHORT_CONTRACTIONS
]
# A contraction over 16 products of integers in [-15, 15] leaves only 23 % of the outputs in need of rounding (ties: 18 %), below the
# 25 % every bf16-output case must show.  The case still runs -- its result must be exact like any other -- but the rounding-path
# conditions are met by its neighbour with 32 input channels, which reaches the same kernel instance.
SHORT_CONTRACTIONS = [(1, 16, 64, 63, 63, 1, 2, False)]
# adjoint pack, stride 1: the stride-1 shapes above whose cout meets the adjoint's chunk rule (% 16 for 3x3, % 64 for 1x1), plus one
DGRAD_CASES = [(1, 32, 48, 20, 28, 3), (1, 48, 64, 9, 70, 3), (1, 64, 64, 15, 17, 1), (1, 128, 128, 24, 40, 3)]
WGRAD_CASES = [(1, 16, 16, 8, 256), (1, 16, 3, 8, 512), (1, 48, 16, 12, 136), (2, 16, 16, 48, 80), (2, 96, 160, 24, 40), (1, 64, 64, 31, 33),
               (2, 64, 64, 64, 64)]       # (the last: many pixels, r = radius(2 * 64 * 64))
WGRAD_1X1_CASES = [(2, 72, 40, 20, 28), (2, 512, 128, 9, 7), (1, 64, 64, 31, 33), (3, 128, 64, 16, 16)]
BATCHED_CASES = [(3, 3, 2, 128, 128, 16, 16), (3, 17, 1, 64, 64, 16, 16), (1, 18, 2, 72, 40, 20, 28)]   # kind, jobs, batch, cin, cout, h, w
STEM_CASES = [(1, 37, 129), (2, 50, 70), (1, 64, 64)]


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 104729 * int(v) for i, v in enumerate(key)) + 29)


@functools.lru_cache(maxsize=None)
def forward_case(batch, cin, cout, h, w, k, stride, bias):
    gen, r = _gen(batch, cin, cout, h, w, k, stride), E.radius(cin * k * k)
    E.check_operands(cin * k * k, r, r, 2)
    x = E.integers((batch, cin, h, w), r, gen)
    wt = E.integers((cout, cin, k, k), r, gen, dtype=torch.float32)
    b = E.integers((cout,), BIAS_R, gen, dtype=torch.float32) if bias else None
    return dict(x=x, w=wt, bias=b, y=E.conv_ref(x, wt, b, stride))


@functools.lru_cache(maxsize=None)
def dgrad_case(batch, cin, cout, h, w, k):
    gen, r = _gen(batch, cin, cout, h, w, k, 7), E.radius(cout * k * k)
    E.check_operands(cout * k * k, r, r)
    wt, gy = E.integers((cout, cin, k, k), r, gen), E.integers((batch, cout, h, w), r, gen)
    dx, _ = E.conv_grads_ref(torch.zeros(batch, cin, h, w), wt, gy)
    return dict(w=wt, gy=gy, dx=dx)


def _wgrad_operands(batch, cin, cout, h, w, gen):
    r = E.radius(batch * h * w)
    E.check_operands(batch * h * w, r, r)
    return E.integers((batch, cin, h, w), r, gen), E.integers((batch, cout, h, w), r, gen)


@functools.lru_cache(maxsize=None)
def wgrad_case(batch, cin, cout, h, w):
    x, gy = _wgrad_operands(batch, cin, cout, h, w, _gen(batch, cin, cout, h, w, 3))
    _, dw = E.conv_grads_ref(x, torch.zeros(cout, cin, 3, 3), gy)
    return dict(x=x, gy=gy, dw=dw)


@functools.lru_cache(maxsize=None)
def wgrad_1x1_case(batch, cin, cout, h, w):
    x, gy = _wgrad_operands(batch, cin, cout, h, w, _gen(batch, cin, cout, h, w, 1))
    return dict(x=x, gy=gy, dw=E.pointwise_wgrad_ref(x, gy).view(cout, cin, 1, 1))


@functools.lru_cache(maxsize=None)
def batched_case(kind, jobs, batch, cin, cout, h, w):
    gen = _gen(kind, jobs, batch, cin, cout, h, w)
    layers = [_wgrad_operands(batch, cin, cout, h, w, gen) for _ in range(jobs)]
    if kind == 3:
        dws = [E.conv_grads_ref(x, torch.zeros(cout, cin, 3, 3), gy)[1] for x, gy in layers]
    else:
        dws = [E.pointwise_wgrad_ref(x, gy).view(cout, cin, 1, 1) for x, gy in layers]
    return dict(layers=layers, dw=dws)


@functools.lru_cache(maxsize=None)
def stem_case(batch, h, w):
    gen, r = _gen(batch, h, w), 15
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    E.check_operands(147, r, r)
    x, wt = E.integers((batch, 3, h, w), r, gen), E.integers((64, 3, 7, 7), r, gen)
    rg = E.radius(batch * ho * wo)
    E.check_operands(batch * ho * wo, r, rg)
    gy = E.integers((batch, 64, ho, wo), rg, gen)
    xr, wr = x.double(), wt.double().requires_grad_(True)
    y = torch.nn.functional.conv2d(xr, wr, stride=2, padding=3)
    y.backward(gy.double())
    return dict(x=x, w=wt, gy=gy, y=y.detach(), dw=wr.grad)


def bf16_output_references():
    """(label, float64 reference) of every bf16-output case of this file, for the rounding-path conditions."""
    for case in FORWARD_CASES:
        if case in SHORT_CONTRACTIONS:
            continue
        yield f"conv forward {case}", forward_case(*case)["y"]
    for case in DGRAD_CASES:
        yield f"conv data gradient {case}", dgrad_case(*case)["dx"]
    for case in WGRAD_CASES:
        yield f"conv 3x3 weight gradient {case}", wgrad_case(*case)["dw"]
    for case in WGRAD_1X1_CASES:
        yield f"conv 1x1 weight gradient {case}", wgrad_1x1_case(*case)["dw"]
    for case in BATCHED_CASES:
        yield f"batched weight gradients {case}", torch.stack(batched_case(*case)["dw"])
    for case in STEM_CASES:
        yield f"stem forward {case}", stem_case(*case)["y"]
        yield f"stem weight gradient {case}", stem_case(*case)["dw"]


@pytest.mark.parametrize("batch,cin,cout,h,w,k,stride,bias", FORWARD_CASES)
def test_conv_forward_exact(device, batch, cin, cout, h, w, k, stride, bias):
    """The output is the RNE image of the exact convolution; fp32 master weights and bf16 weights pack to one image, and so
    does the two-image launch of the stride-1 layers that have an adjoint plan."""
    import sis_hip as S
    assert S.conv_bf16_supported(cin, cout, h, w, k, stride)
    c = forward_case(batch, cin, cout, h, w, k, stride, bias)
    xd, wd = c["x"].to(device), c["w"].to(device)
    bd = c["bias"].to(device) if bias else None
    packed = S.conv_bf16_pack(wd, h, w, stride)
    assert torch.equal(packed, S.conv_bf16_pack(wd.bfloat16(), h, w, stride)), "fp32 and bf16 weights pack differently"
    images = [packed]
    if stride == 1 and S.conv_bf16_supported(cout, cin, h, w, k, 1):
        both, adjoint = S.conv_bf16_pack_both(wd, h, w)
        assert torch.equal(both, packed) and torch.equal(adjoint, S.conv_bf16_pack(wd, h, w, 1, adjoint=True))
        images.append(both)
    for image in images:
        E.assert_bitwise(S.conv_bf16(xd, image, cout, k, stride, bd), E.expected_bf16(c["y"]), f"conv forward {(batch, cin, cout, h, w, k, stride)}", (8, 32))


@pytest.mark.parametrize("batch,cin,cout,h,w,k", DGRAD_CASES)
def test_conv_data_gradient_exact(device, batch, cin, cout, h, w, k):
    """dL/dx = the forward kernel on adjoint-packed weights, contracting over cout * k * k."""
    import sis_hip as S
    assert S.conv_bf16_supported(cout, cin, h, w, k, 1)
    c = dgrad_case(batch, cin, cout, h, w, k)
    packed = S.conv_bf16_pack(c["w"].to(device), h, w, 1, adjoint=True)
    E.assert_bitwise(S.conv_bf16(c["gy"].to(device), packed, cin, k, 1), E.expected_bf16(c["dx"]), f"conv data gradient {(batch, cin, cout, h, w, k)}",
                     (8, 32))


@pytest.mark.parametrize("batch,cin,cout,h,w", WGRAD_CASES)
def test_conv_wgrad_exact(device, batch, cin, cout, h, w):
    """dL/dw of the 3x3 layers over all pixels: exact in fp32 whatever the strip / row-block plan, its RNE image in bf16."""
    import sis_hip as S
    assert S.conv_bf16_wgrad_supported(batch, cin, cout, h, w)
    c = wgrad_case(batch, cin, cout, h, w)
    xd, gd = c["x"].to(device), c["gy"].to(device)
    what = f"conv 3x3 weight gradient {(batch, cin, cout, h, w)}"
    E.assert_bitwise(S.conv_bf16_wgrad(xd, gd, torch.float32), E.exact_f32(c["dw"]), what + " fp32")
    E.assert_bitwise(S.conv_bf16_wgrad(xd, gd, torch.bfloat16), E.expected_bf16(c["dw"]), what + " bf16")


@pytest.mark.parametrize("batch,cin,cout,h,w", WGRAD_1X1_CASES)
def test_conv1x1_wgrad_exact(device, batch, cin, cout, h, w):
    import sis_hip as S
    assert S.conv1x1_bf16_wgrad_supported(batch, cin, cout, h * w)
    c = wgrad_1x1_case(batch, cin, cout, h, w)
    xd, gd = c["x"].to(device), c["gy"].to(device)
    what = f"conv 1x1 weight gradient {(batch, cin, cout, h, w)}"
    E.assert_bitwise(S.conv1x1_bf16_wgrad(xd, gd, torch.float32), E.exact_f32(c["dw"]), what + " fp32")
    E.assert_bitwise(S.conv1x1_bf16_wgrad(xd, gd, torch.bfloat16), E.expected_bf16(c["dw"]), what + " bf16")


@pytest.mark.parametrize("kind,jobs,batch,cin,cout,h,w", BATCHED_CASES)
def test_batched_wgrads_exact(device, kind, jobs, batch, cin, cout, h, w):
    """Layers of one shape through ``_defer_conv_wgrad`` + ``flush_deferred`` (one tile launch and one reduction launch per 16):
    every job is exact, so every job is bitwise its single-layer result although the joint plan cuts the layers differently."""
    import sis_hip as S
    c = batched_case(kind, jobs, batch, cin, cout, h, w)
    xs, gys = [x.to(device) for x, _ in c["layers"]], [gy.to(device) for _, gy in c["layers"]]
    single = S.conv_bf16_wgrad if kind == 3 else S.conv1x1_bf16_wgrad
    dims = (batch, cin, cout, h, w) if kind == 3 else (batch, cin, cout, h * w)
    for dtype in (torch.float32, torch.bfloat16):
        dws = [torch.empty(cout, cin, kind, kind, dtype=dtype, device=device) for _ in range(jobs)]
        for x, gy, dw in zip(xs, gys, dws):
            S._defer_conv_wgrad(kind, x, gy, dw, dims)
        assert S.deferred_pending() == jobs
        S.flush_deferred()
        assert S.deferred_pending() == 0
        for j in range(jobs):
            want = E.exact_f32(c["dw"][j]) if dtype == torch.float32 else E.expected_bf16(c["dw"][j])
            E.assert_bitwise(dws[j], want, f"batched {kind}x{kind} weight gradient, job {j} of {jobs}, {dtype}")
            assert torch.equal(dws[j], single(xs[j], gys[j], dtype))


@pytest.mark.parametrize("image_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("batch,h,w", STEM_CASES)
def test_stem_conv_exact(device, batch, h, w, image_dtype):
    """The 7x7 stride-2 stem on integer pixels (float32 images are converted while they are staged: exact) and filters in
    [-15, 15]: the forward output is the RNE image of the exact result, dW exact in fp32 and its RNE image in bf16."""
    import sis_hip as S
    c = stem_case(batch, h, w)
    xd, wd, gd = c["x"].to(device).to(image_dtype), c["w"].to(device), c["gy"].to(device)
    assert S.stem_conv_supported(xd, wd, 2, 3)
    what = f"stem {(batch, h, w)} {image_dtype}"
    E.assert_bitwise(S.stem_conv_fwd(xd, wd), E.expected_bf16(c["y"]), what + " forward", (1, 32))
    E.assert_bitwise(S.stem_conv_wgrad(xd, gd, torch.float32), E.exact_f32(c["dw"]), what + " dW fp32")
    E.assert_bitwise(S.stem_conv_wgrad(xd, gd, torch.bfloat16), E.expected_bf16(c["dw"]), what + " dW bf16")
