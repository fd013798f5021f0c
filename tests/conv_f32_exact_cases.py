"""Case tables and CPU-only builders of tests/test_conv_f32_exact_gpu.py: the fp32 convolution family (Winograd F(2x2,3x3)
forward / data gradient / weight gradient, pointwise forward / data gradient / dgrad_add / weight gradient, the queued
launches and the wrappers of networks/hip_conv.py) on exactly summable operands (tests/exact_operands.py), with float64
references.  Every case carries the route it claims; tests/test_conv_f32_exact_cpu.py holds the claims to the restated launch
plans (tests/conv_f32_plan.py) and asserts that every reachable route value is claimed.

The shapes are the smallest that reach each route.  Nothing of the package is imported here."""
import functools

import torch
import torch.nn.functional as F

import exact_operands as E

W2, W1 = "modconv_wino2_kernel", "modconv_wino_kernel"

# ---- Winograd forward and data gradient: (batch, cin, cout, h, w) -> claimed route of the forward launch.  The data gradient
# runs the adjoint image on the transposed channel counts; its route is whatever the plan gives for (batch, cout, cin, h, w).
FORWARD_CASES = {
    (4, 8, 8, 2, 8): dict(kernel=W2, xi=1, split="none", tpw=1),                      # xt = 256: pipelined kernel, XI = 1; Cin < 32: no split
    (1, 32, 8, 16, 16): dict(kernel=W2, xi=2, split="even", ksplit=2),                # xt = 432: XI = 2, even K slices
    (9, 40, 72, 4, 8): dict(kernel=W1, split="uneven", ksplit=2, short_batch_tile=True, partial_co=True, co_blocks=2),   # xt = 768; 24 + 16 channels
    (5, 8, 8, 2, 4): dict(kernel=W1, split="none"),                                   # xt < 256
    (2, 64, 64, 20, 12): dict(kernel=W2, xi=2, partial_rows=True, partial_cols=True, tile=(16, 16)),
    (1, 16, 64, 2, 128): dict(kernel=W1, tile=(2, 16), partial_co=False),             # one tile row, eight tile columns
    (8, 32, 128, 16, 16): dict(kernel=W2, co_blocks=2, xcd_group=1),
    (2, 16, 16, 8, 16): dict(kernel=W2, xi=2, tile=(8, 16)),                          # xt = 480: two samples per tile on the pipelined kernel
    (2048, 16, 16, 10, 12): dict(kernel=W2, tpw=2, partial_rows=True, partial_cols=True),   # 2048 tiles: the tile-to-tile pipeline (31 MB in all)
    (4096, 16, 16, 10, 12): dict(kernel=W2, tpw=4),
}
WIDE_FORWARD_SHAPE = (1, 64, 64, 8, 8)

# ---- Winograd weight gradient: (batch, cin, cout, h, w) -> claimed route
WGRAD_CASES = {
    (1, 64, 64, 4, 8): dict(chunks=1, slices=[1]),
    (1, 64, 64, 8, 8): dict(chunks=2, slices=[2]),
    (3, 64, 64, 4, 8): dict(chunks=3, slices=[3]),
    (8, 64, 64, 2, 2): dict(w2=True, h2=True, chunks=1),                              # every neighbour of the one tile is masked (dW is still dense:
                                                                                      # the off-centre taps pair the four pixels with each other)
    (8, 64, 64, 6, 2): dict(tiles_per_sample=3, tiles_per_row=1, w2=True),
    (8, 64, 64, 2, 10): dict(tiles_per_row=5, tiles_per_sample=5, h2=True),
    (4, 64, 64, 4, 14): dict(tiles_per_row=7, slices=[7], chunk_crosses_samples=True),
    (3, 64, 64, 8, 28): dict(slices=[5, 5, 5, 5, 1], reduce=True, last_slice=1),
    (1, 64, 64, 16, 26): dict(slices=[5, 5, 3], reduce=False, last_slice=3),
    (1, 64, 64, 16, 44): dict(slices=[5, 5, 5, 5, 2], reduce=True, last_slice=2),
    (1, 64, 64, 16, 32): dict(slices=[4, 4, 4, 4], reduce=False),                      # even slices: the chunk loop ends on its second half
    (2, 128, 64, 8, 8): dict(ci_blocks=2, co_blocks=1),
    (2, 64, 128, 8, 8): dict(ci_blocks=1, co_blocks=2),
}
WIDE_WGRAD_SHAPE = (1, 64, 64, 8, 8)

# ---- queued launches: (kind, jobs, (batch, cin, cout, h, w)) -> the slice lists of the launches the queue is flushed in
BATCHED_CASES = {
    ("f3", 3, (1, 64, 64, 8, 8)): [[2]],
    ("f3", 18, (3, 64, 64, 8, 28)): [[5, 5, 5, 5, 1], [5, 5, 5, 5, 1]],                # more layers than one launch takes
    ("f3", 18, (3, 128, 128, 8, 28)): [[6, 6, 6, 3], [5, 5, 5, 5, 1]],                 # 16 layers share the chip: other slices, no reduce kernel
    ("f1", 3, (5, 64, 128, 8, 8)): [[3, 2]],
    ("f1", 18, (16, 256, 256, 8, 8)): [[3, 3, 3, 3, 3, 1], [2] * 8],                   # (a single layer: eight slices of two chunks)
}

# ---- pointwise forward, data gradient and dgrad_add: (batch, cin, cout, h, w, bias) -> (forward route, data-gradient route)
PW = "conv1x1_f32_kernel<%d,%d,16>"
POINTWISE_CASES = {
    (256, 32, 128, 2, 2, True): (dict(kernel=PW % (128, 256), live_pixels_last=4, checked=False), dict(kernel=PW % (64, 256))),
    (128, 32, 128, 2, 128, False): (dict(kernel=PW % (128, 128), checked=False, partial_pixels=False), dict(kernel=PW % (64, 128))),
    (256, 32, 64, 2, 2, False): (dict(kernel=PW % (64, 256)), dict(kernel=PW % (64, 256), checked=True)),
    (1, 32, 64, 8, 10, True): (dict(kernel=PW % (64, 128), partial_pixels=True, live_pixels_last=80), dict(kernel=PW % (64, 128))),
    (1, 64, 160, 8, 10, False): (dict(kernel=PW % (64, 128), checked=True), dict(kernel=PW % (64, 128), checked=False)),
    (3, 32, 96, 2, 66, False): (dict(kernel=PW % (64, 128), px_tiles=2, live_pixels_last=4, checked=True), dict(kernel=PW % (64, 128), px_tiles=2)),
    (128, 32, 160, 2, 2, False): (dict(kernel=PW % (128, 256), checked=True), dict(kernel=PW % (64, 128))),   # checked 128-channel tile
    # the 128-channel tiles of the data gradient (its output channels are cin)
    (256, 128, 32, 2, 2, False): (dict(kernel=PW % (64, 256)), dict(kernel=PW % (128, 256), checked=False)),
    (128, 128, 32, 2, 128, False): (dict(kernel=PW % (64, 128)), dict(kernel=PW % (128, 128), checked=False)),
    (128, 160, 32, 2, 2, False): (dict(kernel=PW % (64, 128)), dict(kernel=PW % (128, 256), checked=True)),
    (256, 64, 32, 2, 2, False): (dict(kernel=PW % (64, 256), checked=True), dict(kernel=PW % (64, 256), checked=False)),
}
DGRAD_ADD_CASES = [(1, 32, 64, 8, 10, True), (256, 128, 32, 2, 2, False)]
SKIP_R = 64
WIDE_POINTWISE_SHAPE = (2, 64, 64, 8, 10)

# ---- pointwise weight gradient: (batch, cin, cout, h, w) -> claimed plan
POINTWISE_WGRAD_CASES = {
    (1, 64, 128, 8, 8): dict(tile_id=0, slices=[1]),                                   # one chunk, no workspace
    (1, 128, 64, 8, 8): dict(tile_id=1),
    (1, 32, 256, 8, 8): dict(tile_id=2),
    (1, 256, 512, 8, 8): dict(tile_id=3, tiles=8),
    (5, 64, 128, 8, 8): dict(tile_id=0, slices=[3, 2]),
    (3, 64, 128, 8, 16): dict(tile_id=0, slices=[2, 2, 2]),
}
WIDE_POINTWISE_WGRAD_SHAPE = (1, 64, 128, 8, 8)

# ---- through networks.hip_conv
DILATED_CASES = [((1, 64, 64, 8, 16), 2), ((1, 64, 64, 8, 32), 4)]
HALF_DILATION_CASE = (1, 64, 64, 32, 32)
STRIDE2_CASES = [((2, 64, 64, 6, 8), 3), ((2, 64, 128, 16, 16), 1)]
DOWN_CASE = (2, 16, 64, 8, 16)
DOWN_FIR_SHIFT, DOWN_SCALE_SHIFT = 6, 3      # fir = outer([1,3,3,1]) / 2^6, scale = 2^-3: every result is a multiple of 2^-9
SECOND_ORDER_CASE = (1, 64, 64, 4, 8)


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 104729 * int(v) for i, v in enumerate(key)) + 31)


def _ints(shape, r, gen):
    return E.integers(shape, r, gen, dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def forward_case(batch, cin, cout, h, w):
    """x, w, gy and the float64 y = conv(x, w), dx = dgrad(gy, w)."""
    gen = _gen(batch, cin, cout, h, w, 1)
    rx, rg = E.winograd_radius(cin), E.winograd_radius(cout)
    rw = min(rx, rg)
    E.check_winograd_operands(cin, rx, rw)
    E.check_winograd_operands(cout, rg, rw)
    x, wt, gy = _ints((batch, cin, h, w), rx, gen), _ints((cout, cin, 3, 3), rw, gen), _ints((batch, cout, h, w), rg, gen)
    y = E.conv_ref(x, wt)
    dx = F.conv_transpose2d(gy.double(), wt.double(), padding=1)     # the adjoint of conv_ref in its first argument
    return dict(x=x, w=wt, gy=gy, y=y, dx=dx, r=(rx, rw, rg))


@functools.lru_cache(maxsize=None)
def wide_forward_case(mirrored):
    batch, cin, cout, h, w = WIDE_FORWARD_SHAPE
    gen = _gen(batch, cin, cout, h, w, 2 + int(mirrored))
    x, wt = E.wide_pair((batch, cin, h, w), (cout, cin, 3, 3), gen, mirrored)
    gy, _ = E.wide_pair((batch, cout, h, w), (cout, cin, 3, 3), gen, mirrored)
    return dict(x=x, w=wt, gy=gy, y=E.conv_ref(x, wt), dx=F.conv_transpose2d(gy.double(), wt.double(), padding=1))


def wgrad_tiles(batch, h, w):
    return batch * (h // 2) * (w // 2)


@functools.lru_cache(maxsize=None)
def wgrad_case(batch, cin, cout, h, w):
    gen, r = _gen(batch, cin, cout, h, w, 5), E.winograd_wgrad_radius(wgrad_tiles(batch, h, w))
    E.check_winograd_wgrad_operands(wgrad_tiles(batch, h, w), r, r)
    x, gy = _ints((batch, cin, h, w), r, gen), _ints((batch, cout, h, w), r, gen)
    return dict(x=x, gy=gy, dw=E.conv_grads_ref(x, torch.zeros(cout, cin, 3, 3), gy)[1], r=r)


@functools.lru_cache(maxsize=None)
def wide_wgrad_case(mirrored):
    batch, cin, cout, h, w = WIDE_WGRAD_SHAPE
    x, gy = E.wide_wgrad_pair((batch, cin, h, w), cout, _gen(batch, cin, cout, h, w, 6 + int(mirrored)), mirrored)
    return dict(x=x, gy=gy, dw=E.conv_grads_ref(x, torch.zeros(cout, cin, 3, 3), gy)[1])


@functools.lru_cache(maxsize=None)
def batched_case(kind, jobs, shape):
    batch, cin, cout, h, w = shape
    gen = _gen(jobs, *shape, 8 + len(kind) + int(kind[1]))
    layers, dws = [], []
    for _ in range(jobs):
        if kind == "f3":
            r = E.winograd_wgrad_radius(wgrad_tiles(batch, h, w))
            E.check_winograd_wgrad_operands(wgrad_tiles(batch, h, w), r, r)
        else:
            r = E.radius(batch * h * w)
            E.check_operands(batch * h * w, r, r)
        x, gy = _ints((batch, cin, h, w), r, gen), _ints((batch, cout, h, w), r, gen)
        layers.append((x, gy))
        dws.append(E.conv_grads_ref(x, torch.zeros(cout, cin, 3, 3), gy)[1] if kind == "f3"
                   else E.pointwise_wgrad_ref(x, gy).view(cout, cin, 1, 1))
    return dict(layers=layers, dw=dws)


@functools.lru_cache(maxsize=None)
def pointwise_case(batch, cin, cout, h, w, bias):
    """y = W x (+ bias), dx = W^T gy, and dx + skip for ``conv1x1_f32_dgrad_add``."""
    gen = _gen(batch, cin, cout, h, w, 11)
    rx, rg = E.radius(cin), E.radius(cout)
    rw = min(rx, rg)
    E.check_operands(cin, rx, rw, 2)       # (the factor 2: bias / skip term, both at most SKIP_R << 2^23)
    E.check_operands(cout, rg, rw, 2)
    x, wt, gy = _ints((batch, cin, h, w), rx, gen), _ints((cout, cin, 1, 1), rw, gen), _ints((batch, cout, h, w), rg, gen)
    b = _ints((cout,), SKIP_R, gen) if bias else None
    skip = _ints((batch, cin, h, w), SKIP_R, gen)
    dx = torch.einsum("oi,bohw->bihw", wt.double()[:, :, 0, 0], gy.double())
    return dict(x=x, w=wt, gy=gy, bias=b, skip=skip, y=E.conv_ref(x, wt, b), dx=dx, dx_add=dx + skip.double())


@functools.lru_cache(maxsize=None)
def wide_pointwise_case(mirrored):
    batch, cin, cout, h, w = WIDE_POINTWISE_SHAPE
    gen = _gen(batch, cin, cout, h, w, 12 + int(mirrored))
    x, wt = E.wide_pair((batch, cin, h, w), (cout, cin, 1, 1), gen, mirrored, winograd=False)
    gy, _ = E.wide_pair((batch, cout, h, w), (cout, cin, 1, 1), gen, mirrored, winograd=False)
    return dict(x=x, w=wt, gy=gy, y=E.conv_ref(x, wt), dx=torch.einsum("oi,bohw->bihw", wt.double()[:, :, 0, 0], gy.double()))


@functools.lru_cache(maxsize=None)
def pointwise_wgrad_case(batch, cin, cout, h, w):
    gen, r = _gen(batch, cin, cout, h, w, 14), E.radius(batch * h * w)
    E.check_operands(batch * h * w, r, r)
    x, gy = _ints((batch, cin, h, w), r, gen), _ints((batch, cout, h, w), r, gen)
    return dict(x=x, gy=gy, dw=E.pointwise_wgrad_ref(x, gy).view(cout, cin, 1, 1))


@functools.lru_cache(maxsize=None)
def wide_pointwise_wgrad_case(mirrored):
    batch, cin, cout, h, w = WIDE_POINTWISE_WGRAD_SHAPE
    x, gy = E.wide_wgrad_pair((batch, cin, h, w), cout, _gen(batch, cin, cout, h, w, 15 + int(mirrored)), mirrored, winograd=False)
    return dict(x=x, gy=gy, dw=E.pointwise_wgrad_ref(x, gy).view(cout, cin, 1, 1))


def _layer_case(shape, k, stride, dilation, key):
    """x, w, gy and float64 (y, dx, dw) of one convolution layer with padding dilation * (k // 2)."""
    batch, cin, cout, h, w = shape
    gen = _gen(*shape, k, stride, dilation, key)
    d = dilation
    if k == 3:
        tiles = wgrad_tiles(batch * d * d, h // d, w // d)       # the launch works on the space-to-batch shape
        r = min(E.winograd_radius(max(cin, cout)), E.winograd_wgrad_radius(tiles))
        E.check_winograd_operands(max(cin, cout), r, r)
        E.check_winograd_wgrad_operands(tiles, r, r)
    else:
        r = E.radius(max(cin, cout, batch * h * w))
        E.check_operands(max(cin, cout, batch * h * w), r, r)
    x, wt = _ints((batch, cin, h, w), r, gen), _ints((cout, cin, k, k), r, gen)
    y = E.conv_ref(x, wt, None, stride, dilation)
    gy = _ints(tuple(y.shape), r, gen)
    dx, dw = E.conv_grads_ref(x, wt, gy, stride, dilation)
    return dict(x=x, w=wt, gy=gy, y=y, dx=dx, dw=dw)


@functools.lru_cache(maxsize=None)
def dilated_case(shape, dilation):
    return _layer_case(shape, 3, 1, dilation, 17)


@functools.lru_cache(maxsize=None)
def stride2_case(shape, k):
    return _layer_case(shape, k, 2, 1, 18)


@functools.lru_cache(maxsize=None)
def half_dilation_case():
    """Dilation = half the image side: the layer contracts 4 taps x cin channels per output (a pointwise product over
    4 * cin channels in all three directions); its dW taps add up to 4 blocks of the pointwise weight gradient."""
    batch, cin, cout, h, w = HALF_DILATION_CASE
    gen, d = _gen(*HALF_DILATION_CASE, 19), h // 2
    r = E.radius(4 * max(cin, cout, batch * d * d))
    E.check_operands(4 * max(cin, cout, batch * d * d), r, r)
    x, wt, gy = _ints((batch, cin, h, w), r, gen), _ints((cout, cin, 3, 3), r, gen), _ints((batch, cout, h, w), r, gen)
    dx, dw = E.conv_grads_ref(x, wt, gy, 1, d)
    return dict(x=x, w=wt, gy=gy, y=E.conv_ref(x, wt, None, 1, d), dx=dx, dw=dw)


def down_fir():
    k = torch.tensor([1.0, 3.0, 3.0, 1.0])
    return torch.outer(k, k) * 2.0 ** -DOWN_FIR_SHIFT


def down_ref(x, wt, fir, scale):
    """Blur(pad 2, fir) then 3x3 stride-2 convolution with scale * weight, float64 (the FIR is symmetric: no flip)."""
    c = x.shape[1]
    blurred = F.conv2d(F.pad(x, (2, 2, 2, 2)), fir.double()[None, None].expand(c, 1, 4, 4), groups=c)
    return F.conv2d(blurred, wt * scale, stride=2)


@functools.lru_cache(maxsize=None)
def down_case():
    """The composed weight of the polyphase form is the 6 x 6 kernel w (*) fir cut into 4 phases x 3 x 3 taps: in units of
    2^-9 its entries are at most 49 r_w (a 3 x 3 window of outer([1,3,3,1]) sums to at most 7 * 7).  The Winograd rules then hold
    for 4 * cin channels with that filter radius; the builder takes the radius of the composed integers themselves."""
    batch, cin, cout, h, w = DOWN_CASE
    gen, r = _gen(*DOWN_CASE, 20), 4
    fir, scale = down_fir(), 2.0 ** -DOWN_SCALE_SHIFT
    x, wt = _ints((batch, cin, h, w), r, gen), _ints((cout, cin, 3, 3), r, gen)
    gy = _ints((batch, cout, h // 2, w // 2), r, gen)
    composed = F.conv_transpose2d(wt.double().view(cout * cin, 1, 3, 3), (fir.double() * 2.0 ** DOWN_FIR_SHIFT)[None, None])
    r_composed = int(composed.abs().max())
    assert r_composed <= 49 * r
    E.check_winograd_operands(4 * cin, r, r_composed)
    E.check_winograd_operands(cout, r, r_composed)
    E.check_winograd_wgrad_operands(wgrad_tiles(batch, h // 2, w // 2), r, r)
    xr, wr = x.double().requires_grad_(True), wt.double().requires_grad_(True)
    y = down_ref(xr, wr, fir, scale)
    y.backward(gy.double())
    return dict(x=x, w=wt, gy=gy, fir=fir, scale=scale, y=y.detach(), dx=xr.grad, dw=wr.grad, unit=2.0 ** -(DOWN_FIR_SHIFT + DOWN_SCALE_SHIFT))


@functools.lru_cache(maxsize=None)
def second_order_case():
    """(gy, x, W) -> (dx, dW) differentiated once more with cotangents (ggx, ggW):
    d gy = conv(ggx, W) + conv(x, ggW)  (two convolutions: the radius leaves the factor 2),  d x = dgrad(gy, ggW),
    d W = wgrad(ggx, gy)."""
    batch, cin, cout, h, w = SECOND_ORDER_CASE
    gen, r = _gen(*SECOND_ORDER_CASE, 21), 15
    assert 2 * 324 * max(cin, cout) * r * r < E.EXACT_F32
    E.check_winograd_wgrad_operands(wgrad_tiles(batch, h, w), r, r)
    x, wt, gy = _ints((batch, cin, h, w), r, gen), _ints((cout, cin, 3, 3), r, gen), _ints((batch, cout, h, w), r, gen)
    ggx, ggw = _ints((batch, cin, h, w), r, gen), _ints((cout, cin, 3, 3), r, gen)
    xr, wr, gr = (t.double().requires_grad_(True) for t in (x, wt, gy))
    dx, dw = torch.autograd.grad(F.conv2d(xr, wr, padding=1), (xr, wr), gr, create_graph=True)
    d_gy, d_x, d_w = torch.autograd.grad((dx, dw), (gr, xr, wr), (ggx.double(), ggw.double()))
    return dict(x=x, w=wt, gy=gy, ggx=ggx, ggw=ggw, dx=dx.detach(), dw=dw.detach(), d_gy=d_gy, d_x=d_x, d_w=d_w)


def references():
    """(label, float64 reference, kind) of every case, for the conditions the CPU test puts on the references alone.  kind:
    "map" (an image: last two axes are rows and columns), "dw3" (a 3x3 weight gradient), "dw1", "wide" (sparse by construction)."""
    for s in FORWARD_CASES:
        if s[0] > 64:      # (the tile-pipeline cases: a hundred copies of the same conditions)
            continue
        c = forward_case(*s)
        yield f"forward {s}", c["y"], "map"
        yield f"data gradient {s}", c["dx"], "map"
    for m in (False, True):
        yield f"wide forward mirrored={m}", wide_forward_case(m)["y"], "wide"
        yield f"wide data gradient mirrored={m}", wide_forward_case(m)["dx"], "wide"
        yield f"wide weight gradient mirrored={m}", wide_wgrad_case(m)["dw"], "wide"
        yield f"wide pointwise mirrored={m}", wide_pointwise_case(m)["y"], "wide"
        yield f"wide pointwise weight gradient mirrored={m}", wide_pointwise_wgrad_case(m)["dw"], "wide"
    for s in WGRAD_CASES:
        yield f"weight gradient {s}", wgrad_case(*s)["dw"], "dw3"
    for (kind, jobs, shape) in BATCHED_CASES:
        for j, dw in enumerate(batched_case(kind, jobs, shape)["dw"][:3]):
            yield f"queued {kind} {shape} layer {j}", dw, "dw3" if kind == "f3" else "dw1"
    for s in POINTWISE_CASES:
        c = pointwise_case(*s)
        yield f"pointwise {s}", c["y"], "map"
        yield f"pointwise data gradient {s}", c["dx"], "map"
    for s in POINTWISE_WGRAD_CASES:
        yield f"pointwise weight gradient {s}", pointwise_wgrad_case(*s)["dw"], "dw1"
    layer_cases = [(f"dilated {s} d={d}", dilated_case(s, d)) for s, d in DILATED_CASES]
    layer_cases += [(f"stride 2 {s} k={k}", stride2_case(s, k)) for s, k in STRIDE2_CASES]
    layer_cases += [("half-image dilation", half_dilation_case())]
    for label, c in layer_cases:
        yield label + " y", c["y"], "map"
        sampled = label.endswith("k=1")      # a 1x1 stride-2 layer reads the even pixels only: the gradient of the others is zero
        assert not sampled or not (c["dx"][:, :, 1::2] != 0).any() and not (c["dx"][:, :, :, 1::2] != 0).any()
        yield label + " dx", c["dx"][:, :, ::2, ::2] if sampled else c["dx"], "map"
        yield label + " dw", c["dw"], "dw3" if c["dw"].shape[2] == 3 else "dw1"
    c = second_order_case()
    for name in ("d_gy", "d_x"):
        yield "second order " + name, c[name], "map"
    yield "second order d_w", c["d_w"], "dw3"
