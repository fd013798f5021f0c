"""GPU guard-band tests: every direct ``sis_hip`` wrapper between ``0xFF`` bands (tests/guard_bands.py).

Every case does the same five things: build inputs on the CPU from a seeded generator, place each with ``banded``, call the wrapper
inside ``guarded`` (its results, scratch and split-K workspace are then banded and born ``0xFF``), run ``check()`` -- no band
byte changed, no input changed, no allocation escaped -- and compare every returned tensor with the reference and the tolerance
the op's own parity test states (named in each case's docstring).  A load from a band or from a never-written part of a result
or workspace is a NaN (or -1 / 255): where it can reach a stored value the parity comparison fails, because ``_rel`` / ``_abs``
treat a non-finite difference as infinite.

``CASES`` is exported: tests/test_guard_bands_cpu.py fails when a ``csrc/*.hip`` file has no case here.
"""
import collections
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import guard_bands as G

G.HELPER_FRAMES.update({("test_guard_bands_gpu.py", "put"), ("test_guard_bands_gpu.py", "run")})

Case = collections.namedtuple("Case", "name files fn args")
CASES = []


def case(name, files, *arg_sets):
    """Registers ``fn(t, *args)`` once per entry of ``arg_sets`` (or once without arguments)."""
    def deco(fn):
        for args in (arg_sets or [()]):
            tag = name + ("[" + "-".join(str(a) for a in args) + "]" if args else "")
            CASES.append(Case(tag.replace(" ", ""), tuple(files), fn, tuple(args)))
        return fn
    return deco


class T:
    """What a case works with: ``put`` places an input, ``run`` calls a wrapper between the bands and checks them."""

    def __init__(self, device, monkeypatch):
        self.dev, self.mp = device, monkeypatch

    def put(self, t, inplace=False):
        return None if t is None else G.banded(t, self.dev, inplace)

    def run(self, fn, *args, workspace_bytes=None, **kwargs):
        with G.guarded(self.mp, self.dev, workspace_bytes=workspace_bytes):
            out = fn(*args, **kwargs)
        torch.cuda.synchronize()
        G.check()
        return out


def _finite_max(d):
    m = d.abs().max().item() if d.numel() else 0.0
    return m if m == m else float("inf")   # NaN -> inf: a non-finite result never passes a bound


def _abs(got, ref):
    assert tuple(got.shape) == tuple(ref.shape), (tuple(got.shape), tuple(ref.shape))
    return _finite_max(got.detach().double().cpu() - ref.detach().double().cpu())


def _rel(got, ref):
    return _abs(got, ref) / max(ref.detach().double().abs().max().item(), 1e-30)


def _allclose(got, ref, rtol, atol):
    """np.testing.assert_allclose as the parity tests call it (a NaN against a finite reference value is a mismatch)."""
    assert tuple(got.shape) == tuple(ref.shape), (tuple(got.shape), tuple(ref.shape))
    np.testing.assert_allclose(got.detach().float().cpu().numpy(), ref.detach().float().cpu().numpy(), rtol=rtol, atol=atol)


def _close(got, ref, tol):
    """|err| <= tol * max|ref|, element-wise (the bf16 kernels' tests)."""
    assert _abs(got.float(), ref) <= tol * ref.abs().max().item(), (_abs(got.float(), ref), ref.abs().max().item())


def _mk(gen, *shape):
    return torch.randn(*shape, generator=gen)


# =================================================================================================== generator, fp32
# references and bounds: tests/test_generator_gpu.py (2e-5 of max|ref| per layer, 1e-5 for equal_linear and to_rgb)

def _modconv_operands(t, gen, b, cin, cout, sdim):
    import sis_hip
    from oracle import stylegan2_ref as R
    style = _mk(gen, b, sdim)
    weight, mod_w, mod_b = _mk(gen, 1, cout, cin, 3, 3), _mk(gen, cin, sdim), 1 + 0.1 * _mk(gen, cin)
    wpk, wsq = t.run(sis_hip.modconv_prepack, t.put(weight))
    assert torch.equal(wpk.cpu(), weight[0].permute(1, 2, 3, 0).reshape(cin, 9, cout))
    s = t.run(sis_hip.equal_linear, t.put(style), t.put(mod_w), t.put(mod_b), 1 / sdim ** 0.5, 1.0, False)
    assert _rel(s, R.equal_linear(style, mod_w, mod_b)) < 1e-5
    ds = t.run(sis_hip.modconv_demod, s, wsq, 1 / (cin * 9) ** 0.5, True)
    return style, weight, mod_w, mod_b, wpk, s, ds


@case("modconv2d", ["modconv_entries.hip", "modconv_mfma.hip", "modconv_mfma2.hip", "modconv_wino.hip", "gen_small_ops.hip"],
      *[(b, cin, cout, h, w, fuse, wino) for (b, cin, cout, h, w) in [(3, 24, 136, 16, 16), (5, 64, 128, 4, 4)]
        for fuse in (False, True) for wino in (False, True)], (2, 6, 6, 5, 6, False, False), (2, 6, 6, 5, 6, True, False))
def _modconv2d(t, b, cin, cout, h, w, fuse, wino):
    """test_modconv3x3_vs_oracle: direct MFMA and Winograd F(2x2,3x3) kernels, plain and with noise + bias + activation.
    (2, 6, 6, 5, 6): channels and width that are no multiple of 4, which the pipelined kernel declines: the register-staged
    kernel of csrc/modconv_mfma.hip, same reference and bound."""
    import sis_hip
    from oracle import ops_ref
    from oracle import stylegan2_ref as R
    gen = torch.Generator().manual_seed(b * 1000 + cin + cout + h)
    x = _mk(gen, b, cin, h, w)
    style, weight, mod_w, mod_b, wpk, s, ds = _modconv_operands(t, gen, b, cin, cout, 48)
    noise, nw, bias = _mk(gen, 1, 1, h, w), 0.3 * _mk(gen, 1), 0.2 * _mk(gen, cout)
    with torch.no_grad():
        ref = R.modulated_conv2d(x, style, weight, mod_w, mod_b, demodulate=True)
        if fuse:
            ref = ops_ref.fused_leaky_relu(ref + nw * noise, bias)
    u = t.run(sis_hip.modconv_prepack_wino, t.put(weight)) if wino else None
    y = t.run(sis_hip.modconv2d, t.put(x), wpk, s, ds, 3, t.put(noise) if fuse else None, t.put(nw) if fuse else None,
              t.put(bias) if fuse else None, fuse_act=fuse, wino_u=u)
    if cin % 4:
        assert sis_hip.lib().sis_last_kernel().decode().startswith("modconv_mfma_kernel<0, 3>")
    assert _rel(y, ref) < 2e-5, _rel(y, ref)


def _up_reference(x, style, weight, mod_w, mod_b, noise, nw, bias):
    from oracle import ops_ref
    from oracle import stylegan2_ref as R
    b, cin, h, w = x.shape
    cout = weight.shape[1]
    taps = ops_ref.make_kernel([1, 3, 3, 1]) * 4
    with torch.no_grad():
        s_ref = R.equal_linear(style, mod_w, mod_b).view(b, 1, cin, 1, 1)
        wt = (1 / (cin * 9) ** 0.5) * weight * s_ref
        wt = wt * torch.rsqrt(wt.pow(2).sum([2, 3, 4]) + 1e-8).view(b, cout, 1, 1, 1)
        t_ref = F.conv_transpose2d(x.reshape(1, b * cin, h, w), wt.transpose(1, 2).reshape(b * cin, cout, 3, 3), stride=2,
                                   groups=b).view(b, cout, 2 * h + 1, 2 * w + 1)
        ref = R.modulated_conv2d(x, style, weight, mod_w, mod_b, True, True, taps)
        ref_act = ops_ref.fused_leaky_relu(ref + nw * noise, bias)
    return taps, t_ref, ref, ref_act


@case("modconv2d_up", ["modconv_entries.hip", "modconv_mfma.hip", "modconv_mfma2.hip", "upfirdn2d.hip"], (3, 24, 72, 8, 8, False), (3, 24, 72, 8, 8, True),
      (2, 6, 12, 5, 6, False), (2, 6, 12, 5, 6, True))
def _modconv2d_up(t, b, cin, cout, h, w, padded):
    """test_modconv_up_vs_oracle: the 4-phase transposed convolution, then blur_noise_act reading the buffer it wrote (with
    ``padded``: the 2W+4 row stride, whose pad columns were born 0xFF).  (2, 6, 12, 5, 6): six input channels, which the
    pipelined kernel declines: the register-staged kernel of csrc/modconv_mfma.hip, same reference and bound."""
    import sis_hip
    gen = torch.Generator().manual_seed(b * 77 + cin + cout + h)
    x = _mk(gen, b, cin, h, w)
    style, weight, mod_w, mod_b, wpk, s, ds = _modconv_operands(t, gen, b, cin, cout, 32)
    noise, nw, bias = _mk(gen, b, 1, 2 * h, 2 * w), 0.3 * _mk(gen, 1), 0.2 * _mk(gen, cout)
    taps, t_ref, ref, ref_act = _up_reference(x, style, weight, mod_w, mod_b, noise, nw, bias)
    up = t.run(sis_hip.modconv2d_up, t.put(x), wpk, s, ds, padded_rows=padded)
    if cin % 8:
        assert sis_hip.lib().sis_last_kernel().decode().startswith("modconv_mfma_kernel<1, 3>")
    in_w = 2 * w + 1 if padded else None
    if padded:
        assert tuple(up.shape) == (b, cout, 2 * h + 1, 2 * w + 4)
    assert _rel(up[..., :2 * w + 1], t_ref) < 2e-5, _rel(up[..., :2 * w + 1], t_ref)
    y = t.run(sis_hip.blur_noise_act, up, t.put(taps), (1, 1), in_w=in_w)
    assert _rel(y, ref) < 2e-5
    ya = t.run(sis_hip.blur_noise_act, up, t.put(taps), (1, 1), t.put(noise), t.put(nw), t.put(bias), fuse_act=True, in_w=in_w)
    assert _rel(ya, ref_act) < 2e-5


@case("modconv2d_up_fir", ["modconv_upfir.hip", "upfirdn2d.hip"], (2, 24, 64, 34, 40), (3, 40, 128, 32, 32))
def _modconv2d_up_fir(t, b, cin, cout, h, w):
    """test_modconv_up_fir_vs_oracle: the fast-FIR kernel (edge blocks, a non-square map) into padded rows, then the blur."""
    import sis_hip
    gen = torch.Generator().manual_seed(b * 131 + cin + cout + h + w)
    x = _mk(gen, b, cin, h, w)
    style, weight, mod_w, mod_b, wpk, s, ds = _modconv_operands(t, gen, b, cin, cout, 32)
    noise, nw, bias = _mk(gen, b, 1, 2 * h, 2 * w), 0.3 * _mk(gen, 1), 0.2 * _mk(gen, cout)
    taps, t_ref, ref, ref_act = _up_reference(x, style, weight, mod_w, mod_b, noise, nw, bias)
    fir_u = t.run(sis_hip.modconv_prepack_up_fir, t.put(weight))
    assert tuple(fir_u.shape) == (cin, 8, cout, 2)
    assert sis_hip.lib().sis_modconv_up_fir_supported(b, cin, cout, h, w, 2 * w + 4)
    records = []
    sis_hip.set_profiler(records)
    try:
        tp = t.run(sis_hip.modconv2d_up, t.put(x), wpk, s, ds, padded_rows=True, fir_u=fir_u)
    finally:
        sis_hip.set_profiler(None)
    assert [r[0] for r in records] == ["modconv_upfir_kernel"]
    assert _rel(tp[..., :2 * w + 1], t_ref) < 2e-5, _rel(tp[..., :2 * w + 1], t_ref)
    yp = t.run(sis_hip.blur_noise_act, tp, t.put(taps), (1, 1), t.put(noise), t.put(nw), t.put(bias), fuse_act=True, in_w=2 * w + 1)
    assert _rel(yp, ref_act) < 2e-5


@case("to_rgb", ["gen_small_ops.hip"], (1, 16, 6), (2, 32, 4))
def _to_rgb(t, b, cin, h):
    """test_to_rgb_vs_oracle, without and with skip + taps."""
    import sis_hip
    from oracle import ops_ref
    from oracle import stylegan2_ref as R
    gen = torch.Generator().manual_seed(cin + h)
    sd = {"p.conv.weight": _mk(gen, 1, 3, cin, 1, 1), "p.conv.modulation.weight": _mk(gen, cin, 32),
          "p.conv.modulation.bias": 1 + 0.1 * _mk(gen, cin), "p.bias": 0.1 * _mk(gen, 1, 3, 1, 1),
          "p.upsample.kernel": ops_ref.make_kernel([1, 3, 3, 1]) * 4}
    x, style, skip = _mk(gen, b, cin, h, h), _mk(gen, b, 32), _mk(gen, b, 3, h // 2, h // 2)
    with torch.no_grad():
        s = t.run(sis_hip.equal_linear, t.put(style), t.put(sd["p.conv.modulation.weight"]), t.put(sd["p.conv.modulation.bias"]),
                  1 / 32 ** 0.5, 1.0, False)
        xd, wd, bd = t.put(x), t.put(sd["p.conv.weight"]), t.put(sd["p.bias"])
        y0 = t.run(sis_hip.to_rgb, xd, wd, s, bd, 1 / cin ** 0.5)
        assert _rel(y0, R.to_rgb(sd, "p", x, style)) < 1e-5
        y1 = t.run(sis_hip.to_rgb, xd, wd, s, bd, 1 / cin ** 0.5, t.put(skip), t.put(sd["p.upsample.kernel"]), (2, 1))
        assert _rel(y1, R.to_rgb(sd, "p", x, style, skip)) < 1e-5


@case("upfirdn2d", ["upfirdn2d.hip"], ("float32", 2e-5), ("float16", 2e-2))
def _upfirdn2d(t, dtype, tol):
    """test_upfirdn2d_vs_oracle, its odd-sized cases."""
    import sis_hip
    from oracle import ops_ref
    dtype = getattr(torch, dtype)
    gen = torch.Generator().manual_seed(3)
    for (major, ih, iw, minor, kh, kw, up, down, p0, p1) in [(6, 9, 9, 1, 4, 4, 1, 1, 1, 1), (2, 6, 5, 1, 2, 2, 2, 1, 1, 0),
                                                             (2, 7, 5, 1, 3, 3, 1, 1, 1, 1), (2, 7, 5, 3, 4, 3, 1, 1, 2, -1),
                                                             (2, 5, 6, 2, 5, 5, 3, 2, 2, 3), (1, 33, 65, 1, 4, 4, 1, 1, 0, 0)]:
        x = torch.randn(major, ih, iw, minor, generator=gen, dtype=torch.float64)
        k = torch.randn(kh, kw, generator=gen, dtype=torch.float64)
        xq, kq = x.to(dtype), k.to(dtype)
        ref = ops_ref.upfirdn2d_nhwc(xq.double(), kq.double(), up, up, down, down, p0, p1, p0, p1)
        y = t.run(sis_hip.upfirdn2d, t.put(xq), t.put(kq), up, up, down, down, p0, p1, p0, p1)
        assert y.dtype == dtype
        assert _abs(y, ref) <= tol * max(1.0, ref.abs().max().item()), (dtype, (major, ih, iw, minor, kh, kw, up, down, p0, p1))


@case("fused_bias_act", ["fused_bias_act.hip"], ((1, 5, 3),), ((2, 16, 7, 9),))
def _fused_bias_act(t, shape):
    """test_fused_leaky_relu_vs_oracle in fp32 (1e-6), through the C binding the public wrapper calls."""
    import sis_hip
    from oracle import ops_ref
    gen = torch.Generator().manual_seed(11)
    x = torch.randn(*shape, generator=gen, dtype=torch.float64).float()
    b = torch.randn(shape[1], generator=gen, dtype=torch.float64).float()
    ref = ops_ref.fused_leaky_relu(x.double(), b.double())
    xd = t.put(x)
    y = t.run(sis_hip.fused_bias_act, xd, t.put(b), xd.new_empty(0), 3, 0, 0.2, 2 ** 0.5)
    assert _abs(y, ref) <= 1e-6 * max(1.0, ref.abs().max().item())


# =================================================================================================== plain fp32 convolutions
# references and bounds: tests/test_hip_conv_gpu.py, tests/test_conv1x1_f32_gpu.py

@case("conv3x3", ["modconv_entries.hip", "modconv_wino.hip"], (5, 8, 8, 2, 4, 1), (9, 40, 72, 4, 8, 1), (1, 16, 64, 2, 128, 1), (1, 8, 16, 16, 24, 2))
def _conv3x3(t, batch, cin, cout, h, w, dil):
    """test_forward_and_data_gradient (2e-5 of the range), the kernel called directly: forward image and adjoint image."""
    import sis_hip
    import networks.hip_conv as hc
    g = torch.Generator().manual_seed(batch * 1000 + cin)
    x = torch.randn(batch, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, 3, 3, generator=g) * (cin * 9) ** -0.5
    gy = torch.randn(batch, cout, h, w, generator=g)
    assert sis_hip.conv3x3_supported(x.to(t.dev), wt.to(t.dev), dil)
    xr = x.double().requires_grad_(True)
    ref = F.conv2d(xr, wt.double(), padding=dil, dilation=dil)
    ref.backward(gy.double())
    wd = t.put(wt)
    u = t.run(sis_hip.conv3x3_prepack, wd)
    ua = t.run(sis_hip.conv3x3_prepack, wd, adjoint=True)
    u2, ua2 = t.run(sis_hip.conv3x3_prepack_both, wd)
    assert torch.equal(u, u2) and torch.equal(ua, ua2)
    y = hc._batch_to_space(t.run(sis_hip.conv3x3, t.put(hc._space_to_batch(x, dil)), u), dil)
    gx = hc._batch_to_space(t.run(sis_hip.conv3x3, t.put(hc._space_to_batch(gy, dil)), ua), dil)
    assert _rel(y, ref.detach().float()) < 2e-5
    assert _rel(gx, xr.grad.float()) < 2e-5


@case("conv3x3_wgrad", ["conv_wgrad_wino.hip"], (4, 128, 64, 6, 20), (64, 64, 64, 4, 4))
def _conv3x3_wgrad(t, batch, cin, cout, h, w):
    """test_weight_gradient_kernel (2e-4): split-K slabs in the 0xFF-born per-device workspace."""
    import sis_hip
    g = torch.Generator().manual_seed(cin + cout)
    x = torch.randn(batch, cin, h, w, generator=g)
    gy = torch.randn(batch, cout, h, w, generator=g)
    assert sis_hip.conv3x3_wgrad_supported(batch, cin, cout, h, w, min_work=0)
    got = t.run(sis_hip.conv3x3_wgrad, t.put(x), t.put(gy))
    wt = torch.zeros(cout, cin, 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv2d(x.double(), wt, padding=1).backward(gy.double())
    assert _rel(got, wt.grad.float()) < 2e-4


@case("conv1x1_f32", ["conv1x1_f32.hip"], (2, 64, 64, 20, 12, True), (1, 128, 160, 8, 10, False))
def _conv1x1_f32(t, batch, cin, cout, h, w, bias):
    """test_conv1x1_f32_forward_and_data_gradient (1e-5), and conv1x1_f32_dgrad_add = data gradient + skip (one more addition)."""
    import sis_hip
    gen = torch.Generator().manual_seed(cin + cout)
    x = torch.randn(batch, cin, h, w, generator=gen)
    wt = torch.randn(cout, cin, 1, 1, generator=gen) / cin ** 0.5
    b = torch.randn(cout, generator=gen) if bias else None
    gy = torch.randn(batch, cout, h, w, generator=gen)
    skip = torch.randn(batch, cin, h, w, generator=gen)
    xd, wd, gyd = t.put(x), t.put(wt), t.put(gy)
    assert sis_hip.conv1x1_f32_supported(xd, wd)
    xr = x.double().requires_grad_(True)
    ref = F.conv2d(xr, wt.double(), b.double() if bias else None)
    ref.backward(gy.double())
    y = t.run(sis_hip.conv1x1_f32, xd, wd, t.put(b))
    assert _abs(y, ref) <= 1e-5 * ref.abs().max().item()
    gx = t.run(sis_hip.conv1x1_f32, gyd, wd, data_gradient=True)
    assert _abs(gx, xr.grad) <= 1e-5 * xr.grad.abs().max().item()
    want = xr.grad + skip.double()
    gs = t.run(sis_hip.conv1x1_f32_dgrad_add, gyd, wd, t.put(skip))
    assert _abs(gs, want) <= 1e-5 * want.abs().max().item()


def _wgrad1x1_ref(gy, x):
    return torch.einsum("bop,bip->oi", gy.double().flatten(2), x.double().flatten(2)).view(gy.shape[1], x.shape[1], 1, 1)


@case("conv1x1_wgrad_f32", ["conv1x1_wgrad_f32.hip"], (1, 64, 128, 8, 8, False), (5, 192, 384, 8, 16, False),
      (1, 64, 128, 8, 8, True), (5, 192, 384, 8, 16, True))
def _conv1x1_wgrad_f32(t, batch, cin, cout, h, w, small_ws):
    """test_weight_gradient_kernel of test_conv1x1_f32_gpu.py (2e-5).  The single-layer wrapper brings a scratch of exactly the
    planned slabs, so the band begins where the last slab ends; ``small_ws`` repeats the case with ``WORKSPACE_BYTES`` at twice
    one dW slab (the batched form below is the one that plans its K slices by it)."""
    import sis_hip
    g = torch.Generator().manual_seed(batch * 7 + cin + cout)
    x = torch.randn(batch, cin, h, w, generator=g)
    gy = torch.randn(batch, cout, h, w, generator=g)
    xd, gyd = t.put(x), t.put(gy)
    assert sis_hip.conv1x1_wgrad_f32_supported(gyd, xd)
    dw = t.run(sis_hip.conv1x1_wgrad_f32, gyd, xd, workspace_bytes=2 * cout * cin * 4 if small_ws else None)
    assert _rel(dw, _wgrad1x1_ref(gy, x)) < 2e-5


@case("conv1x1_wgrad_f32_multi", ["conv1x1_wgrad_f32.hip"], (False,), (True,))
def _conv1x1_wgrad_f32_multi(t, small_ws):
    """test_batched_fp32_weight_gradients_of_one_shape, ("f1", 17, 1, 64, 256, 16, 16): 17 layers through ``_defer_conv_wgrad`` and
    ``flush_deferred``.  That test allows 1e-4 of the largest entry against the single-layer kernel, which is itself within 2e-5
    of the fp64 product; here each dW is held to the fp64 product at 1e-4.  ``small_ws``: a per-device workspace of twice one dW
    slab -- the 16-layer launch then gets no slab at all (every layer straight into its dW), the 17th layer two slices instead of
    the planned number, with the end of the workspace right behind them."""
    import sis_hip
    jobs, batch, cin, cout, h, w = 17, 1, 64, 256, 16, 16
    gen = torch.Generator().manual_seed(2 * 100 + jobs * 10 + cin)
    xs = [torch.randn(batch, cin, h, w, generator=gen) for _ in range(jobs)]
    gys = [torch.randn(batch, cout, h, w, generator=gen) for _ in range(jobs)]
    xd, gyd = [t.put(x) for x in xs], [t.put(gy) for gy in gys]
    assert sis_hip.conv1x1_wgrad_f32_supported(gyd[0], xd[0])

    def batch_of_layers():
        dws = [sis_hip.torch.empty((cout, cin, 1, 1), dtype=torch.float32, device=t.dev) for _ in range(jobs)]
        for x, gy, dw in zip(xd, gyd, dws):
            sis_hip._defer_conv_wgrad("f1", x, gy, dw, (batch, cin, cout, h * w))
        sis_hip.flush_deferred()
        assert sis_hip.deferred_pending() == 0
        return dws

    dws = t.run(batch_of_layers, workspace_bytes=2 * cout * cin * 4 if small_ws else None)
    for j in range(jobs):
        assert _rel(dws[j], _wgrad1x1_ref(gys[j], xs[j])) <= 1e-4, j


@case("half_dilation_taps", ["dilation_taps.hip"], (24, 16))
def _half_dilation_taps(t, cout, cin):
    """Each of the 16 quadrant pairs sees one tap: the matrix is a gather of the weight (exact), its backward the matching sum of
    at most four entries (1e-5, the bound of test_half_image_dilation_is_the_dilated_convolution)."""
    import sis_hip
    gen = torch.Generator().manual_seed(16)
    wt = torch.randn(cout, cin, 3, 3, generator=gen)
    taps = t.run(sis_hip.half_dilation_taps, t.put(wt))
    assert tuple(taps.shape) == (4 * cout, 4 * cin)
    flat = wt.reshape(-1)
    tc = taps.cpu()
    # every entry of the matrix is one weight entry or zero; recover the (linear) map by pushing an index image through it
    idx = t.run(sis_hip.half_dilation_taps, t.put(torch.arange(1, wt.numel() + 1, dtype=torch.float32).view_as(wt))).cpu().long()
    want = torch.where(idx > 0, flat[(idx - 1).clamp(min=0)], torch.zeros(()))
    assert torch.equal(tc, want)
    g = torch.randn(4 * cout, 4 * cin, generator=gen)
    dw = t.run(sis_hip.half_dilation_taps_bwd, t.put(g), cout, cin)
    ref = torch.zeros(wt.numel(), dtype=torch.float64).index_add_(0, (idx - 1).clamp(min=0).reshape(-1),
                                                                   (g.double() * (idx > 0)).reshape(-1)).view_as(wt)
    assert _abs(dw, ref) <= 1e-5 * ref.abs().max().item()


# =================================================================================================== bf16 encoder kernels
# references and bounds: tests/test_conv_bf16_gpu.py (bf16 results 1e-2, fp32 weight gradients 2e-3 of max|ref|),
# tests/test_gemm_bf16_gpu.py (BF16_TOL 1e-2, F32_TOL 2e-4), tests/test_attention_gpu.py (2e-2; log-sum-exp 1e-3)

BF16_TOL, F32_TOL = 1e-2, 2e-4


@case("conv_bf16", ["conv_bf16.hip"], (1, 16, 3, 64, 64, 3, True), (1, 256, 128, 24, 40, 3, False), (2, 64, 256, 20, 28, 1, False))
def _conv_bf16(t, batch, cin, cout, h, w, k, bias):
    """test_conv_bf16_forward: three output channels + bias, ragged tiles in both directions, the pointwise ragged tail tile."""
    import sis_hip
    assert sis_hip.conv_bf16_supported(cin, cout, h, w, k, 1)
    gen = torch.Generator().manual_seed(cin + cout + h)
    x = torch.randn(batch, cin, h, w, generator=gen).bfloat16()
    wt = torch.randn(cout, cin, k, k, generator=gen) / (cin * k * k) ** 0.5
    b = torch.randn(cout, generator=gen) if bias else None
    ref = F.conv2d(x.float(), wt.bfloat16().float(), b, padding=k // 2)
    xd, bd = t.put(x), t.put(b)
    for weight in (wt, wt.bfloat16()):
        packed = t.run(sis_hip.conv_bf16_pack, t.put(weight), h, w, 1)
        y = t.run(sis_hip.conv_bf16, xd, packed, cout, k, 1, bd)
        assert y.dtype == torch.bfloat16
        _close(y, ref, 1e-2)


@case("conv_bf16_dgrad", ["conv_bf16.hip"], (1, 128, 128, 24, 40, 3), (2, 256, 64, 16, 16, 1))
def _conv_bf16_dgrad(t, batch, cin, cout, h, w, k):
    """test_conv_bf16_data_gradient: the same kernel on adjoint-packed weights; both images also from ``conv_bf16_pack_both``."""
    import sis_hip
    gen = torch.Generator().manual_seed(cin * 3 + cout)
    wt = (torch.randn(cout, cin, k, k, generator=gen) / (cout * k * k) ** 0.5).bfloat16()
    gy = torch.randn(batch, cout, h, w, generator=gen).bfloat16()
    x = torch.zeros(batch, cin, h, w, requires_grad=True)
    F.conv2d(x, wt.float(), padding=k // 2).backward(gy.float())
    assert sis_hip.conv_bf16_supported(cout, cin, h, w, k, 1)
    wd = t.put(wt)
    adj = t.run(sis_hip.conv_bf16_pack, wd, h, w, 1, adjoint=True)
    gx = t.run(sis_hip.conv_bf16, t.put(gy), adj, cin, k, 1)
    _close(gx, x.grad, 1e-2)
    if sis_hip.conv_bf16_supported(cin, cout, h, w, k, 1):
        packed, adj2 = t.run(sis_hip.conv_bf16_pack_both, wd, h, w)
        assert torch.equal(adj2, adj) and torch.equal(packed, t.run(sis_hip.conv_bf16_pack, wd, h, w, 1))


@case("conv_bf16_wgrad", ["conv_bf16_wgrad.hip"], (1, 48, 16, 12, 136), (2, 96, 160, 24, 40))
def _conv_bf16_wgrad(t, batch, cin, cout, h, w):
    """test_conv_bf16_weight_gradient: fp32 result 2e-3, bf16 result 1e-2."""
    import sis_hip
    gen = torch.Generator().manual_seed(cin + 7 * cout + h)
    x = torch.randn(batch, cin, h, w, generator=gen).bfloat16()
    gy = torch.randn(batch, cout, h, w, generator=gen).bfloat16()
    wt = torch.zeros(cout, cin, 3, 3, requires_grad=True)
    F.conv2d(x.float(), wt, padding=1).backward(gy.float())
    assert sis_hip.conv_bf16_wgrad_supported(batch, cin, cout, h, w)
    xd, gyd = t.put(x), t.put(gy)
    for dtype, tol in ((torch.float32, 2e-3), (torch.bfloat16, 1e-2)):
        dw = t.run(sis_hip.conv_bf16_wgrad, xd, gyd, dtype)
        assert dw.dtype == dtype
        _close(dw, wt.grad, tol)


@case("conv1x1_bf16_wgrad", ["conv_bf16_wgrad.hip"], (2, 72, 40, 20, 28), (2, 512, 128, 9, 7))
def _conv1x1_bf16_wgrad(t, batch, cin, cout, h, w):
    """test_conv1x1_bf16_weight_gradient: channel counts that are no tile multiples, planes shorter than a stage."""
    import sis_hip
    gen = torch.Generator().manual_seed(cin + 3 * cout + h)
    x = torch.randn(batch, cin, h, w, generator=gen).bfloat16()
    gy = torch.randn(batch, cout, h, w, generator=gen).bfloat16()
    ref = torch.einsum("bop,bip->oi", gy.double().flatten(2), x.double().flatten(2)).float().view(cout, cin, 1, 1)
    assert sis_hip.conv1x1_bf16_wgrad_supported(batch, cin, cout, h * w)
    xd, gyd = t.put(x), t.put(gy)
    for dtype, tol in ((torch.float32, 2e-3), (torch.bfloat16, 1e-2)):
        dw = t.run(sis_hip.conv1x1_bf16_wgrad, xd, gyd, dtype)
        assert dw.dtype == dtype
        _close(dw, ref, tol)


@case("stem_conv", ["stem_conv.hip"], (1, 37, 129, "float32"), (1, 37, 129, "bfloat16"))
def _stem_conv(t, batch, h, w, image_dtype):
    """test_stem_conv_7x7_stride_2_on_the_image at its odd size: forward 1e-2, dW 2e-3 (fp32) / 1e-2 (bf16)."""
    import sis_hip
    gen = torch.Generator().manual_seed(h * 3 + w)
    x = torch.randn(batch, 3, h, w, generator=gen).to(getattr(torch, image_dtype))
    wt = (torch.randn(64, 3, 7, 7, generator=gen) / 147 ** 0.5).bfloat16()
    xd, wd = t.put(x), t.put(wt)
    assert sis_hip.stem_conv_supported(xd, wd, 2, 3)
    wr = wt.float().requires_grad_(True)
    ref = F.conv2d(x.bfloat16().float(), wr, stride=2, padding=3)
    y = t.run(sis_hip.stem_conv_fwd, xd, wd)
    assert y.dtype == torch.bfloat16
    _close(y, ref.detach(), 1e-2)
    gy = torch.randn(*ref.shape, generator=gen).bfloat16()
    ref.backward(gy.float())
    gyd = t.put(gy)
    for dtype, tol in ((torch.float32, 2e-3), (torch.bfloat16, 1e-2)):
        dw = t.run(sis_hip.stem_conv_wgrad, xd, gyd, dtype)
        assert dw.dtype == dtype
        _close(dw, wr.grad, tol)


def _rand16(shape, gen, scale=1.0):
    return (torch.randn(*shape, generator=gen) * scale).bfloat16()


def _gelu(x):
    return 0.5 * x * (1 + torch.erf(x / math.sqrt(2)))


def _gelu_grad(x):
    return 0.5 * (1 + torch.erf(x / math.sqrt(2))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)


@case("gemm_bf16_nt", ["gemm_bf16.hip", "gemm256_bf16.hip"], (130, 132, 192, 0), (130, 132, 192, 4), (300, 100, 192, 9), (64, 96, 256, 10))
def _gemm_nt(t, m, n, k, tile):
    """test_gemm_nt_epilogues / test_gemm256_nt_epilogues at their ragged shapes (M, N and K tails): no epilogue, bias, bias + GELU
    (two outputs), bias + residual (fp32) and, on the 128-wide tiles, the fp32 output; the 256-row tiles also GELU-backward."""
    import sis_hip as S
    gen = torch.Generator().manual_seed(m * 7 + n * 3 + k + tile)
    x, w = _rand16((m, k), gen), _rand16((n, k), gen, k ** -0.5)
    bias, resid, pre_in = torch.randn(n, generator=gen), torch.randn(m, n, generator=gen), _rand16((m, n), gen)
    xd, wd, bd, rd = t.put(x), t.put(w), t.put(bias), t.put(resid)
    y = x.float() @ w.float().t()
    _close(t.run(S.gemm_bf16, xd, wd, S.GEMM_NT, S.EPI_NONE, tile=tile), y, BF16_TOL)
    _close(t.run(S.gemm_bf16, xd, wd, S.GEMM_NT, S.EPI_BIAS, bias=bd, tile=tile), y + bias, BF16_TOL)
    out, dact = t.run(S.gemm_bf16, xd, wd, S.GEMM_NT, S.EPI_BIAS_GELU_DROP, bias=bd, tile=tile)
    _close(out, _gelu(y + bias), BF16_TOL)
    _close(dact, _gelu_grad(y + bias), BF16_TOL)
    res = t.run(S.gemm_bf16, xd, wd, S.GEMM_NT, S.EPI_BIAS_DROP_RESID, bias=bd, resid=rd, tile=tile)
    assert res.dtype == torch.float32
    _close(res, resid + y + bias, F32_TOL * 4)
    if tile < S.TILE_256X96:
        _close(t.run(S.gemm_bf16, xd, wd, S.GEMM_NT, S.EPI_F32, tile=tile), y, F32_TOL)
    else:
        _close(t.run(S.gemm_bf16, xd, wd, S.GEMM_NT, S.EPI_GELU_BWD, pre=t.put(pre_in), tile=tile), y * pre_in.float(), BF16_TOL)


@case("gemm_bf16_nn", ["gemm_bf16.hip"], (200, 136, 64, 0), (200, 136, 64, 5))
def _gemm_nn(t, m, n, k, tile):
    """test_gemm_nn_data_gradient: plain and with the GELU-backward epilogue."""
    import sis_hip as S
    gen = torch.Generator().manual_seed(m + n + k + tile)
    g, w, pre = _rand16((m, k), gen), _rand16((k, n), gen, k ** -0.5), _rand16((m, n), gen)
    gd, wd = t.put(g), t.put(w)
    y = g.float() @ w.float()
    _close(t.run(S.gemm_bf16, gd, wd, S.GEMM_NN, S.EPI_NONE, tile=tile), y, BF16_TOL)
    _close(t.run(S.gemm_bf16, gd, wd, S.GEMM_NN, S.EPI_GELU_BWD, pre=t.put(pre), tile=tile), y * pre.float(), BF16_TOL)


@case("gemm_bf16_tn", ["gemm_bf16.hip", "column_sum.hip"], (136, 264, 200, 2, 0), (768, 768, 320, 4, 0), (264, 72, 1000, 2, 4))
def _gemm_tn(t, m, n, k, splits, tile):
    """test_gemm_tn_weight_gradient (split-K slabs in the 0xFF-born workspace; 320 tokens: 5 K steps for 4 slices) and
    test_gemm_weight_and_bias_gradient_in_one_pair_of_launches: dW bitwise the plain run, db the column sums."""
    import sis_hip as S
    gen = torch.Generator().manual_seed(m + n + k + splits + tile)
    g, x = _rand16((k, m), gen), _rand16((k, n), gen)
    ref = g.float().t() @ x.float()
    gd, xd = t.put(g), t.put(x)
    got = t.run(S.gemm_bf16, gd, xd, S.GEMM_TN, S.EPI_F32, splits=splits, tile=tile)
    assert got.dtype == torch.float32
    _close(got, ref, F32_TOL)
    dw, db = t.run(S.gemm_bf16_wgrad_bias, gd, xd, splits, tile)
    assert torch.equal(dw, got)
    assert torch.equal(db, t.run(S.column_sum, gd))
    _close(db, g.float().sum(0), F32_TOL)


@case("gemm_bf16_wgrad_bias_multi", ["gemm_bf16.hip"], (3, 136, 264, 200))
def _gemm_wgrad_multi(t, jobs, m, n, k):
    """Several Linear layers of one shape from one launch: every problem contracts all its tokens per tile, so each dW / db is
    held to the fp32 product of its own operands at F32_TOL, as the single-layer form is."""
    import sis_hip as S
    gen = torch.Generator().manual_seed(jobs + m + n + k)
    gs, xs = [_rand16((k, m), gen) for _ in range(jobs)], [_rand16((k, n), gen) for _ in range(jobs)]
    gd, xd = [t.put(g) for g in gs], [t.put(x) for x in xs]

    def launch():
        out = [(S.torch.empty((m, n), dtype=torch.float32, device=t.dev), S.torch.empty(m, dtype=torch.float32, device=t.dev)) for _ in range(jobs)]
        S.gemm_bf16_wgrad_bias_multi([(g, x, dw, db) for g, x, (dw, db) in zip(gd, xd, out)])
        return out

    for (dw, db), g, x in zip(t.run(launch), gs, xs):
        _close(dw, g.float().t() @ x.float(), F32_TOL)
        _close(db, g.float().sum(0), F32_TOL)


@case("gemm_bf16_batched", ["gemm_bf16.hip"], (4, 64, 72, 256))
def _gemm_batched(t, batch, cin, cout, hw):
    """test_gemm_batched_as_pointwise_convolution at its smallest shape: forward, data gradient, weight gradient summed over the
    images (slabs in the workspace)."""
    import sis_hip as S
    gen = torch.Generator().manual_seed(batch + cin + cout)
    x = torch.randn(batch, cin, hw, generator=gen).bfloat16()
    w = (torch.randn(cout, cin, generator=gen) * cin ** -0.5).bfloat16()
    gy = torch.randn(batch, cout, hw, generator=gen).bfloat16()
    xr = x.float().view(batch, cin, hw, 1).requires_grad_(True)
    wr = w.float().view(cout, cin, 1, 1).requires_grad_(True)
    yr = F.conv2d(xr, wr)
    yr.backward(gy.float().view(batch, cout, hw, 1))
    xd, wd, gd = t.put(x), t.put(w), t.put(gy)
    _close(t.run(S.gemm_bf16_batched, wd, xd, S.GEMM_NN), yr.detach().view(batch, cout, hw), BF16_TOL)
    _close(t.run(S.gemm_bf16_batched, wd, gd, S.GEMM_TN), xr.grad.view(batch, cin, hw), BF16_TOL)
    dw = t.run(S.gemm_bf16_batched, gd, xd, S.GEMM_NT, S.EPI_F32, sum_over_batches=True)
    assert dw.dtype == torch.float32
    _close(dw, wr.grad.view(cout, cin), F32_TOL)


@case("attention", ["attention_bf16.hip"], (1, 70, 1), (2, 196, 2))
def _attention(t, b, n, heads):
    """test_attention_forward_backward: token counts that are no multiple of the tile; the descriptor's bound ends where the band
    begins."""
    import sis_hip as S
    from test_attention_gpu import _reference
    gen = torch.Generator().manual_seed(b * 1000 + n + heads)
    qkv = torch.randn(b, n, 3 * heads * 64, generator=gen).bfloat16()
    d_ctx = torch.randn(b, n, heads * 64, generator=gen).bfloat16()
    ref_ctx, ref_lse, ref_grad = _reference(qkv, heads, d_ctx)
    qd = t.put(qkv)
    ctx, lse = t.run(S.attention_fwd, qd, heads)
    assert ctx.dtype == torch.bfloat16
    _close(ctx, ref_ctx, 2e-2)
    assert _abs(lse, ref_lse) <= 1e-3 * max(1.0, ref_lse.abs().max().item())
    d_qkv = t.run(S.attention_bwd, t.put(d_ctx), qd, ctx, lse, heads)
    assert d_qkv.dtype == torch.bfloat16
    hd = heads * 64
    for sl in (slice(0, hd), slice(hd, 2 * hd), slice(2 * hd, 3 * hd)):
        _close(d_qkv[..., sl], ref_grad[..., sl], 2e-2)


@case("dropout_bwd_cast", ["vit_elementwise.hip"], (37, 100))
def _dropout_bwd_cast(t, m, n):
    """test_gemm_dropout_stream's backward: bf16(g * factor); p = 0 keeps everything (exactly bf16(g)), with p = 0.1 every
    survivor is g * 65536 / (65536 - round(p * 65536)) within bf16 rounding and the dropped fraction is p (+- 5e-3 there at 786 432
    elements; here 3 700 elements: +- 4 sigma = 2e-2)."""
    import sis_hip as S
    gen = torch.Generator().manual_seed(11)
    g = torch.randn(m, n, generator=gen)
    gd, seed = t.put(g), t.put(torch.tensor([12345], dtype=torch.int64), inplace=True)   # (dropout_advance steps the word)
    assert torch.equal(t.run(S.dropout_bwd_cast, gd, seed, 3, 0.0).cpu(), g.bfloat16())
    p = 0.1
    gb = t.run(S.dropout_bwd_cast, gd, seed, 3, p).cpu()
    scale = 65536 / (65536 - int(p * 65536 + 0.5))
    assert torch.isfinite(gb.float()).all()
    mask = gb != 0
    assert abs((1 - mask.float().mean().item()) - p) < 2e-2
    _close(gb[mask], g[mask] * scale, BF16_TOL)
    t.run(S.dropout_advance, seed)
    assert seed.item() != 12345


@case("swap_last2", ["vit_elementwise.hip"], ((3, 70, 33), "bfloat16"), ((3, 70, 33), "float32"))
def _swap_last2(t, shape, dtype):
    """test_swap_last2_is_the_contiguous_transpose (bitwise), the kernel without its autograd shell."""
    import sis_hip
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(sum(shape))).to(getattr(torch, dtype))
    y = t.run(sis_hip._swap_last2, t.put(x))
    assert y.is_contiguous() and torch.equal(y.cpu(), x.transpose(-1, -2).contiguous())


# =================================================================================================== normalisation
# references and bounds: tests/test_upsample_gpu.py (np.testing.assert_allclose with the rtol / atol stated there)

def _gn_inputs(shape, seed, scale=2.0, shift=0.5):
    g = torch.Generator().manual_seed(seed)
    c = shape[1]
    x = torch.randn(*shape, generator=g) * scale + shift
    gamma, beta = 1 + 0.2 * torch.randn(c, generator=g), 0.3 * torch.randn(c, generator=g)
    gy = torch.randn(*shape, generator=g)
    return g, x, gamma, beta, gy


@case("group_norm", ["group_norm.hip"], ((3, 256, 7, 9), 32, False), ((2, 96, 5, 5), 96, True))
def _group_norm(t, shape, groups, relu):
    """test_group_norm_relu: fp32 both directions, bf16 tensors in and out."""
    import sis_hip
    _, x, gamma, beta, gy = _gn_inputs(shape, shape[1])
    xr = x.double().requires_grad_(True)
    gr, br = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    ref = F.group_norm(xr, groups, gr, br, 1e-6)
    ref = F.relu(ref) if relu else ref
    ref.backward(gy.double())
    xd, gd, bd, gyd = t.put(x), t.put(gamma), t.put(beta), t.put(gy)
    y, mean, rstd = t.run(sis_hip.group_norm_fwd, xd, gd, bd, groups, 1e-6, relu)
    _allclose(y, ref, 1e-4, 1e-5)
    dx, dg, db = t.run(sis_hip.group_norm_bwd, gyd, xd, mean, rstd, gd, bd, groups, relu)
    _allclose(dx, xr.grad, 1e-3, 1e-4)
    _allclose(dg, gr.grad, 1e-3, 1e-3)
    _allclose(db, br.grad, 1e-3, 1e-3)
    xb = x.bfloat16()
    xbd = t.put(xb)
    yb, mb, rb = t.run(sis_hip.group_norm_fwd, xbd, gd, bd, groups, 1e-6, relu)
    assert yb.dtype == torch.bfloat16
    xq = xb.double().requires_grad_(True)
    rq = F.group_norm(xq, groups, gamma.double(), beta.double(), 1e-6)
    rq = F.relu(rq) if relu else rq
    _allclose(yb, rq, 1e-2, 1e-2)
    rq.backward(gy.bfloat16().double())
    dxb, dgb, dbb = t.run(sis_hip.group_norm_bwd, t.put(gy.bfloat16()), xbd, mb, rb, gd, bd, groups, relu)
    assert dxb.dtype == torch.bfloat16
    _allclose(dxb, xq.grad, 2e-2, 1e-2 * float(xq.grad.abs().max()))


@case("group_norm_residual", ["group_norm.hip"], ((2, 32, 64, 64), 32, True), ((2, 64, 9, 7), 32, False))
def _group_norm_residual(t, shape, groups, single_pass):
    """test_group_norm_single_pass_groups (one-workgroup groups: hw % 512 == 0; parameter gradients to 1e-3 of their largest
    entry) and test_group_norm_residual_relu (odd planes; 1e-3 absolute): y = relu(group_norm(x) + residual) with the
    low-precision copy and the gate bits, then the backward through the saved output and through the bits."""
    import sis_hip
    g, x, gamma, beta, gy = _gn_inputs(shape, shape[1] + shape[2])
    x = x.bfloat16()
    res, g_lp = torch.randn(*shape, generator=g), torch.randn(*shape, generator=g).bfloat16()
    xr, rr = x.double().requires_grad_(True), res.double().requires_grad_(True)
    gr, br = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    ref = F.relu(F.group_norm(xr, groups, gr, br, 1e-6) + rr)
    ref.backward(gy.double() + g_lp.double())
    xd, gd, bd, rd, gyd, gld = t.put(x), t.put(gamma), t.put(beta), t.put(res), t.put(gy), t.put(g_lp)
    y, mean, rstd, y_lp, gate = t.run(sis_hip.group_norm_fwd, xd, gd, bd, groups, 1e-6, True, residual=rd, low_precision_copy=True, want_gate=True)
    assert y.dtype == torch.float32 and torch.equal(y_lp, y.to(x.dtype))
    _allclose(y, ref, 1e-4, 1e-4)
    bits = ((gate.cpu().numpy()[:, None] >> np.arange(8)) & 1).reshape(-1)[:y.numel()]
    assert np.array_equal(bits.astype(bool), (y > 0).cpu().numpy().reshape(-1))
    for kw in ({"y_mask": y}, {"gate": gate}):
        dx, dg, db, dres = t.run(sis_hip.group_norm_bwd, gyd, xd, mean, rstd, gd, bd, groups, True, want_residual_grad=True, grad_y_lp=gld, **kw)
        _allclose(dres, rr.grad, 1e-5, 1e-6)
        _allclose(dx, xr.grad, 2e-2, 1e-2 * float(xr.grad.abs().max()))
        _allclose(dg, gr.grad, 1e-3, 1e-3 * (float(gr.grad.abs().max()) if single_pass else 1.0))
        _allclose(db, br.grad, 1e-3, 1e-3 * (float(br.grad.abs().max()) if single_pass else 1.0))


@case("batch_norm_train", ["group_norm.hip"], ((2, 64, 33, 31), False))
def _batch_norm_train(t, shape, relu):
    """test_batch_norm_train_relu, incl. the running statistics (banded operands updated in place)."""
    import sis_hip
    g = torch.Generator().manual_seed(shape[1] + shape[2])
    c = shape[1]
    x = torch.randn(*shape, generator=g) * 1.5 - 0.3
    gamma, beta = 1 + 0.2 * torch.randn(c, generator=g), 0.3 * torch.randn(c, generator=g)
    gy = torch.randn(*shape, generator=g)
    rm_ref, rv_ref = torch.zeros(c, dtype=torch.float64), torch.ones(c, dtype=torch.float64)
    xr = x.double().requires_grad_(True)
    gr, br = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    ref = F.batch_norm(xr, rm_ref, rv_ref, gr, br, True, 0.1, 1e-5)
    ref = F.relu(ref) if relu else ref
    ref.backward(gy.double())
    xd, gd, bd = t.put(x), t.put(gamma), t.put(beta)
    rm, rv = t.put(torch.zeros(c), inplace=True), t.put(torch.ones(c), inplace=True)
    y, mean, rstd = t.run(sis_hip.batch_norm_train_fwd, xd, gd, bd, rm, rv, 1e-5, 0.1, relu)
    _allclose(y, ref, 1e-4, 1e-5)
    _allclose(rm, rm_ref, 1e-5, 1e-6)
    _allclose(rv, rv_ref, 1e-5, 1e-6)
    dx, dg, db = t.run(sis_hip.batch_norm_train_bwd, t.put(gy), xd, mean, rstd, gd, bd, relu)
    _allclose(dx, xr.grad, 1e-3, 1e-4)
    _allclose(dg, gr.grad, 1e-3, 1e-3)
    _allclose(db, br.grad, 1e-3, 1e-3)
    yb, _, _ = t.run(sis_hip.batch_norm_train_fwd, t.put(x.bfloat16()), gd, bd, None, None, 1e-5, 0.1, relu)
    assert yb.dtype == torch.bfloat16
    _allclose(yb, ref, 3e-2, 3e-2)


@case("layer_norm", ["layer_norm.hip"], (37, 768), (5, 1024))
def _layer_norm(t, rows, n):
    """test_layer_norm: both directions, fp32 and the bf16 forms; ``layer_norm_bwd_fused`` = the same gradients plus the residual
    stream's gradient (one more fp32 addition), and its bf16 cast at p = 0."""
    import sis_hip
    g = torch.Generator().manual_seed(n + rows)
    x = torch.randn(rows, n, generator=g) * 2 + 0.5
    gamma, beta = 1 + 0.2 * torch.randn(n, generator=g), 0.3 * torch.randn(n, generator=g)
    gy = torch.randn(rows, n, generator=g)
    rg = torch.randn(rows, n, generator=g)
    xr = x.double().requires_grad_(True)
    gr, br = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    F.layer_norm(xr, (n,), gr, br, 1e-6).backward(gy.double())
    ref = F.layer_norm(x.double(), (n,), gamma.double(), beta.double(), 1e-6)
    xd, gd, bd, gyd = t.put(x), t.put(gamma), t.put(beta), t.put(gy)
    assert sis_hip.layer_norm_supported(xd, n)
    y, mean, rstd = t.run(sis_hip.layer_norm_fwd, xd, gd, bd, 1e-6)
    _allclose(y, ref, 1e-4, 1e-5)
    dx, dg, db = t.run(sis_hip.layer_norm_bwd, gyd, xd, mean, rstd, gd)
    _allclose(dx, xr.grad, 1e-3, 1e-4)
    _allclose(dg, gr.grad, 1e-3, 1e-3)
    _allclose(db, br.grad, 1e-3, 1e-3)
    yb, _, _ = t.run(sis_hip.layer_norm_fwd, xd, gd, bd, 1e-6, torch.bfloat16)
    assert yb.dtype == torch.bfloat16
    _allclose(yb, ref, 1e-2, 1e-2)
    dxb, _, _ = t.run(sis_hip.layer_norm_bwd, t.put(gy.bfloat16()), xd, mean, rstd, gd)
    assert dxb.dtype == torch.float32
    _allclose(dxb, xr.grad, 5e-2, 2e-2 * float(xr.grad.abs().max()))
    seed = t.put(torch.tensor([777], dtype=torch.int64))
    fx, fg, fb, cast = t.run(sis_hip.layer_norm_bwd_fused, gyd, xd, mean, rstd, gd, residual_grad=t.put(rg), cast_seed=seed, cast_site=2, cast_p=0.0)
    _allclose(fx, xr.grad + rg.double(), 1e-3, 1e-4)
    _allclose(fg, gr.grad, 1e-3, 1e-3)
    _allclose(fb, br.grad, 1e-3, 1e-3)
    assert cast.dtype == torch.bfloat16 and torch.equal(cast, fx.bfloat16())
    px, pg, pb, none = t.run(sis_hip.layer_norm_bwd_fused, gyd, xd, mean, rstd, gd)
    assert none is None and torch.equal(px, dx) and torch.equal(pg, dg) and torch.equal(pb, db)


@case("column_sum", ["column_sum.hip"], (77, 3072, "bfloat16"), (513, 260, "float32"))
def _column_sum(t, rows, n, dt):
    """test_column_sum."""
    import sis_hip
    x = torch.randn(rows, n, generator=torch.Generator().manual_seed(rows + n)).to(getattr(torch, dt))
    got = t.run(sis_hip.column_sum, t.put(x))
    assert got.dtype == torch.float32
    _allclose(got, x.double().sum(0), 1e-5, 1e-4 * rows ** 0.5)


@case("weight_std", ["weight_std.hip"], ((5, 3, 3, 3),), ((64, 3, 7, 7),))
def _weight_std(t, shape):
    """test_weight_standardisation, both directions, fp32 and bf16."""
    import sis_hip
    g = torch.Generator().manual_seed(shape[0])
    w = torch.randn(*shape, generator=g) * 0.3 + 0.1
    gy = torch.randn(*shape, generator=g)
    wd, gyd = t.put(w), t.put(gy)
    w_hat, invstd = t.run(sis_hip.weight_std_fwd, wd, 1e-5)
    wr = w.double().requires_grad_(True)
    var, mean = torch.var_mean(wr, dim=[1, 2, 3], keepdim=True, unbiased=False)
    ref = (wr - mean) / torch.sqrt(var + 1e-5)
    ref.backward(gy.double())
    _allclose(w_hat, ref, 1e-5, 1e-5)
    dw = t.run(sis_hip.weight_std_bwd, gyd, wd, invstd, 1e-5)
    _allclose(dw, wr.grad, 1e-4, 1e-4 * float(wr.grad.abs().max()))
    w16, _ = t.run(sis_hip.weight_std_fwd, wd, 1e-5, torch.bfloat16)
    _allclose(w16, ref, 1e-2, 1e-2)
    dw16 = t.run(sis_hip.weight_std_bwd, t.put(gy.bfloat16()), wd, invstd, 1e-5)
    _allclose(dw16, wr.grad, 5e-2, 2e-2 * float(wr.grad.abs().max()))


@case("upsample_bilinear", ["upsample_ops.hip"], ((1, 5, 7, 9), (14, 18)))
def _upsample_bilinear(t, shape, size):
    """test_forward_backward_f32; then an x2 map written into / read from the leading channels of a wider tensor
    (test_upsample_cat_fused at (3, 5, 3, 12, 20): bitwise the dense kernels), whose other channels must stay as they were."""
    import sis_hip
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(*shape, generator=g)
    gy = torch.randn(shape[0], shape[1], *size, generator=g)
    xd, gyd = t.put(x), t.put(gy)
    y = t.run(sis_hip.upsample_bilinear, xd, *size)
    xr = x.double().requires_grad_(True)
    ref = F.interpolate(xr, size=size, mode="bilinear", align_corners=True)
    ref.backward(gy.double())
    _allclose(y, ref, 1e-5, 4e-5)
    gx = t.run(sis_hip.upsample_bilinear, xd, *size, grad_output=gyd)
    _allclose(gx, xr.grad, 1e-5, 1e-4)
    b, c, extra, h, w = 3, 5, 3, 12, 20
    x2, wide, gw = torch.randn(b, c, h, w, generator=g), torch.randn(b, c + extra, 2 * h, 2 * w, generator=g), torch.randn(b, c + extra, 2 * h, 2 * w, generator=g)
    x2d, wd, gwd = t.put(x2), t.put(wide, inplace=True), t.put(gw)
    t.run(sis_hip.upsample2x_into, wd, x2d)
    assert torch.equal(wd[:, :c], t.run(sis_hip.upsample_bilinear, x2d, 2 * h, 2 * w)) and torch.equal(wd[:, c:].cpu(), wide[:, c:])
    dense = t.run(sis_hip.upsample_bilinear, x2d, 2 * h, 2 * w, grad_output=t.put(gw[:, :c].contiguous()))
    assert torch.equal(t.run(sis_hip.upsample2x_grad_from, gwd, c), dense)


@case("equal_linear_pixel_norm", ["gen_small_ops.hip"], (3,))
def _head_ops(t, b):
    """The mapping network's pieces at batch 3: pixel_norm and equal_linear with the activation (1e-5 of max|ref|, the bound
    test_modconv3x3_vs_oracle puts on equal_linear), and truncate (an fp32 lerp: the same bound)."""
    import sis_hip
    from oracle import stylegan2_ref as R
    gen = torch.Generator().manual_seed(b)
    z, w, bias = _mk(gen, b, 40), _mk(gen, 56, 40), 0.1 * _mk(gen, 56)
    zn = t.run(sis_hip.pixel_norm, t.put(z))
    assert _rel(zn, R.pixel_norm(z)) < 1e-5
    y = t.run(sis_hip.equal_linear, zn, t.put(w), t.put(bias), 0.01 / 40 ** 0.5, 0.01, True)
    assert _rel(y, R.equal_linear(R.pixel_norm(z), w, bias, lr_mul=0.01, activation=True)) < 1e-5
    lat, mean = _mk(gen, b, 5, 40), _mk(gen, 1, 40)
    tr = t.run(sis_hip.truncate, t.put(lat), t.put(mean), 0.7)
    assert _rel(tr, mean + 0.7 * (lat - mean)) < 1e-5


@case("modulation_demod_batch", ["gen_small_ops.hip"], (3,))
def _modulation_batch(t, b):
    """Every layer's style vector and demodulation scale from two launches (Generator._modulate_all), on tables that point at
    banded weights: channel counts that are no multiple of the head tile.  s to 1e-5 (equal_linear's bound), the scales to the
    generator kernels' per-layer 2e-5."""
    import struct
    import sis_hip
    from oracle import stylegan2_ref as R
    gen = torch.Generator().manual_seed(17 + b)
    dim, n_latent, tile = 48, 4, sis_hip.head_gemm_tile()
    layers = [(24, 136, 0, True), (136, 3, 1, False), (136, 40, 2, True), (40, 72, 3, True)]   # (cin, cout, latent index, styled conv)
    latent = _mk(gen, b, n_latent, dim)
    mod_rows, dem_rows, refs, s_off, d_off, mblocks, dblocks = [], [], [], 0, 0, 0, 0
    for cin, cout, lat, styled in layers:
        mw, mb, weight = _mk(gen, cin, dim), 1 + 0.1 * _mk(gen, cin), _mk(gen, 1, cout, cin, 3, 3)
        mwd, mbd = t.put(mw), t.put(mb)
        s_ref = R.equal_linear(latent[:, lat], mw, mb).double()
        mod_rows.append([mwd.data_ptr(), mbd.data_ptr(), s_off, lat, cin, mblocks, 0, 0])
        mblocks += (cin + tile - 1) // tile
        d_ref = None
        if styled:
            scale = 1 / (cin * 9) ** 0.5
            _, wsq = t.run(sis_hip.modconv_prepack, t.put(weight))
            bits = struct.unpack("<i", struct.pack("<f", scale))[0]
            dem_rows.append([wsq.data_ptr(), bits, s_off, d_off, cout, dblocks, cin, 1])
            dblocks += (cout + tile - 1) // tile
            wsq_ref = weight[0].double().pow(2).sum((2, 3))
            d_ref = scale * torch.rsqrt((scale * scale) * (s_ref.pow(2) @ wsq_ref.t()) + 1e-8)
        refs.append((s_off, cin, s_ref, d_off if styled else None, cout, d_ref, wsq if styled else None))
        s_off += b * cin
        d_off += b * cout if styled else 0
    mod, dem, ld = t.put(torch.tensor(mod_rows, dtype=torch.int64)), t.put(torch.tensor(dem_rows, dtype=torch.int64)), t.put(latent)

    def launch():
        s_flat = sis_hip.torch.empty(s_off, dtype=torch.float32, device=t.dev)
        d_flat = sis_hip.torch.empty(d_off, dtype=torch.float32, device=t.dev)
        sis_hip.modulation_batch(s_flat, ld, mod, len(mod_rows), mblocks, 1 / dim ** 0.5)
        sis_hip.demod_batch(d_flat, s_flat, dem, len(dem_rows), dblocks, b)
        return s_flat, d_flat

    s_flat, d_flat = t.run(launch)
    for so, cin, s_ref, do, cout, d_ref, wsq in refs:
        s = s_flat[so:so + b * cin].view(b, cin)
        assert _rel(s, s_ref) < 1e-5
        if d_ref is not None:
            d = d_flat[do:do + b * cout].view(b, cout)
            assert _rel(d, d_ref) < 2e-5
            assert _rel(t.run(sis_hip.modconv_demod, s.contiguous(), wsq, 1 / (cin * 9) ** 0.5, True), d_ref) < 2e-5


# =================================================================================================== losses, pooling, EM attention
# references and bounds: tests/test_loss_ops_gpu.py, tests/test_seg_ops_gpu.py, tests/test_pool_gpu.py, tests/test_emau_gpu.py

@case("ce_dice", ["loss_ops.hip"], (1, 2, 32, 36, "float32"), (3, 8, 40, 40, "bfloat16"))
def _ce_dice(t, b, c, h, w, dtype):
    """test_ce_dice_forward_backward: 2e-5 relative on the three loss values, 1e-5 (fp32) / 2^-8 (bf16) of max|grad|."""
    import sis_hip as S
    from test_loss_ops_gpu import _reference
    dtype = getattr(torch, dtype)
    gen = torch.Generator().manual_seed(b + c + h)
    logits = (torch.randn(b, c, h, w, generator=gen) * 3).to(dtype)
    labels = torch.randint(0, c, (b, h, w), generator=gen)
    loss, ce, dice, grad = _reference(logits, labels, c)
    zd, ld = t.put(logits), t.put(labels)
    assert S.ce_dice_supported(zd, ld)
    out, stats = t.run(S.ce_dice_fwd, zd, ld)
    for got, want in zip(out.cpu().tolist(), (loss.item(), ce.item(), dice.item())):
        assert abs(got - want) <= 2e-5 * abs(want), (got, want)
    g = t.run(S.ce_dice_bwd, t.put(torch.tensor(1.0)), zd, ld, stats)
    assert g.dtype == dtype
    _close(g, grad, 1e-5 if dtype == torch.float32 else 2 ** -8)


@case("upsample_ce", ["seg_ops.hip"], (3, 5, 7, 9, 40, 33), (2, 2, 1, 1, 8, 8))
def _upsample_ce(t, b, c, h, w, H, W):
    """test_upsample_ce_forward_backward at its odd shape and at the one-pixel map."""
    import sis_hip
    from test_seg_ops_gpu import _ref_loss
    gen = torch.Generator().manual_seed(b + c + h + H)
    logits = torch.randn(b, c, h, w, generator=gen) * 2
    labels = torch.randint(0, c, (b, H, W), generator=gen)
    labels[torch.rand(b, H, W, generator=gen) < 0.1] = 255
    gl = torch.randn(b, generator=gen)
    x64 = logits.double().requires_grad_(True)
    ref = _ref_loss(x64, labels, (H, W), 255)
    (gref,) = torch.autograd.grad(ref, x64, gl.double())
    xd, ld = t.put(logits), t.put(labels)
    loss = t.run(sis_hip.upsample_ce_fwd, xd, ld, (H, W), 255)
    assert torch.allclose(loss.cpu().double(), ref.detach(), rtol=2e-5, atol=1e-6)
    gx = t.run(sis_hip.upsample_ce_bwd, t.put(gl), xd, ld, (H, W), 255)
    assert _abs(gx, gref) <= 2e-5 * gref.abs().max().item() + 1e-9


@case("ema_update", ["seg_ops.hip"], (6, 40, 64))
def _ema_update(t, n, c, k):
    """test_ema_update (in place on a banded operand)."""
    import sis_hip
    gen = torch.Generator().manual_seed(9)
    mu, mub = torch.randn(1, c, k, generator=gen), torch.randn(n, c, k, generator=gen)
    ref = mu.clone()
    ref *= 0.9
    ref += mub.mean(dim=0, keepdim=True) * (1 - 0.9)
    d = t.put(mu, inplace=True)
    t.run(sis_hip.ema_update, d, t.put(mub), 0.9)
    assert torch.allclose(d.cpu(), ref, rtol=1e-6, atol=1e-7) and bool(torch.isfinite(d).all())


@case("bn_ops", ["bn_ops.hip"], (3, 20, 10, 6, True, True, False), (3, 5, 12, 20, True, False, False), (4, 37, 16, 16, True, True, True),
      (4, 37, 16, 16, False, False, True))
def _bn_ops(t, b, c, h, w, relu, use_res, fused):
    """test_fused_batch_norm_act (planes of 60 and 240 values: no multiple of a wave) through the kernels the module calls: bn_stats +
    bn_act_fwd + bn_act_bwd with the sign mask, or (``fused``, a channel fits one workgroup) bn_fused_fwd and the single-pass
    backward.  Output 1e-4 / 1e-5, running statistics 1e-4 / 1e-7 and 1e-5, every gradient 2e-4 of its largest entry."""
    import sis_hip
    gen = torch.Generator().manual_seed(b + c + h)
    x, res, gy = (torch.randn(b, c, h, w, generator=gen) * s + o for s, o in ((2, 0.5), (1, 0), (1, 0)))
    gamma, beta = 1 + 0.1 * torch.randn(c, generator=gen), 0.1 * torch.randn(c, generator=gen)
    xr, rr = x.double().requires_grad_(True), res.double().requires_grad_(True)
    gr, br = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    rm, rv = torch.zeros(c, dtype=torch.float64), torch.ones(c, dtype=torch.float64)
    ref = F.batch_norm(xr, rm, rv, gr, br, True, 3e-4, 1e-5)
    ref = ref + rr if use_res else ref
    ref = F.relu(ref) if relu else ref
    grads_ref = torch.autograd.grad(ref, [xr, gr, br] + ([rr] if use_res else []), gy.double())
    xd, rd, gd, bd = t.put(x), t.put(res) if use_res else None, t.put(gamma), t.put(beta)
    rmd, rvd = t.put(torch.zeros(c), inplace=True), t.put(torch.ones(c), inplace=True)
    assert sis_hip.bn_supported(xd) and sis_hip.bn_fused_supported(xd) == fused
    if fused:
        y, mean, invstd, mask = t.run(sis_hip.bn_fused_fwd, xd, rd, gd, bd, rmd, rvd, 1e-5, 3e-4, relu, want_mask=relu)
    else:
        mean, invstd = t.run(sis_hip.bn_stats, xd, rmd, rvd, 1e-5, 3e-4)
        out = t.run(sis_hip.bn_act_fwd, xd, rd, mean, invstd, gd, bd, relu, want_mask=relu)
        y, mask = out if relu else (out, None)
    assert torch.allclose(y.cpu().double(), ref.detach(), rtol=1e-4, atol=1e-5)
    assert torch.allclose(rmd.cpu().double(), rm, rtol=1e-4, atol=1e-7)
    assert torch.allclose(rvd.cpu().double(), rv, rtol=1e-5)
    gyd = t.put(gy)
    for gate in ({"mask": mask}, {}) if mask is not None else ({},):
        dx, dres, dg, db = t.run(sis_hip.bn_act_bwd, gyd, None if gate else y, xd, mean, invstd, gd, relu, use_res, **gate)
        for got, want in zip([dx, dg, db] + ([dres] if use_res else []), grads_ref):
            assert _abs(got, want) <= 2e-4 * (want.abs().max().item() + 1e-12)


@case("max_pool2d", ["pool_ops.hip"], ((3, 4, 17, 23), (3, 2, 1), "float32"), ((1, 2, 7, 9), (3, 2, 0), "bfloat16"), ((1, 3, 3, 3), (3, 1, 1), "float32"))
def _max_pool2d(t, shape, geom, dtype):
    """test_max_pool_equals_aten: bit-equal in both directions, ties and a NaN included."""
    import sis_hip
    k, s, p = geom
    dtype = getattr(torch, dtype)
    g = torch.Generator().manual_seed(sum(shape) + k * 10 + s)
    x = torch.relu(torch.randn(*shape, generator=g)).mul(4).round().div(4)
    x[0, 0, 0, 0] = float("nan")
    x = x.to(dtype)
    ref_in = x.clone().requires_grad_(True)
    ref = F.max_pool2d(ref_in, k, s, p)
    got, arg = t.run(sis_hip.max_pool2d, t.put(x), k, s, p)
    assert got.shape == ref.shape
    assert torch.equal(torch.nan_to_num(got.cpu(), nan=-7.0), torch.nan_to_num(ref.detach(), nan=-7.0))
    gy = torch.randn(ref.shape, generator=g).to(dtype)
    ref.backward(gy)
    dx = t.run(sis_hip.max_pool2d_backward, t.put(gy), arg, shape[2], shape[3], k, s, p)
    assert torch.equal(dx.cpu(), ref_in.grad)


@case("emau_forward", ["emau.hip"], (3, 128, 16, 8, 1), (1, 64, 16, 16, 2))
def _emau(t, b, c, h, w, stages):
    """test_emau_kernels_vs_float64_composition: bases to 1e-5 per (unit) column, reconstruction to 2e-5 of max|ref|."""
    import sis_hip
    from test_emau_gpu import _reference
    gen = torch.Generator().manual_seed(b * 1000 + c + h)
    x = torch.randn(b, c, h, w, generator=gen) * 0.5 + torch.randn(b, c, 1, 1, generator=gen) * 0.3
    mu0 = torch.randn(1, c, 64, generator=gen)
    mu0 = mu0 / (1e-6 + mu0.norm(dim=1, keepdim=True))
    xd, md = t.put(x), t.put(mu0)
    assert sis_hip.emau_supported(xd, md)
    y, mu = t.run(sis_hip.emau_forward, xd, md, stages)
    y_ref, mu_ref = _reference(x, mu0, stages)
    assert bool(torch.isfinite(mu).all())
    assert (mu.cpu().double() - mu_ref).norm(dim=1).max().item() < 1e-5
    assert _abs(y.view(b, c, -1), y_ref) / y_ref.abs().max().item() < 2e-5


# =================================================================================================== DocUFCN
# references and bounds: tests/doc_ufcn_checks.py (per plane / per channel figures), tests/test_doc_ufcn_gpu.py (Frobenius 1e-5)

SENTINEL = -77.25


def _figures(title, figs):
    bad = [str(f) for f in figs if not f.ok]
    assert not bad, (title, bad)


def _frob(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    r = ((a - b).norm() / b.norm().clamp_min(1e-30)).item()
    return r if r == r else float("inf")


@case("dconv3x3", ["doc_ufcn.hip"], (3, 16, 8, 9, 1), (2, 64, 64, 10, 2))
def _dconv3x3(t, batch, cin, cout, size, d):
    """test_dconv3x3_matches_conv2d / test_dconv3x3_wgrad_slice_plans at maps whose pixel count is no multiple of the 16-pixel stage:
    forward, data gradient on the adjoint weights, weight gradient (3x3 and one tap), bias gradient; per plane (doc_ufcn_checks)
    and in the Frobenius norm."""
    import sis_hip
    import doc_ufcn_checks as K
    g = torch.Generator().manual_seed(batch * size + cin)
    x = torch.randn(batch, cin, size, size, generator=g)
    w = torch.randn(cout, cin, 3, 3, generator=g) / (3 * cin ** 0.5)
    b = torch.randn(cout, generator=g)
    gy = torch.randn(batch, cout, size, size, generator=g)
    xr, wr, br = (v.double().requires_grad_() for v in (x, w, b))
    ref = F.conv2d(xr, wr, br, padding=d, dilation=d)
    ref.backward(gy.double())
    xd, wd, bd, gyd = t.put(x), t.put(w), t.put(b), t.put(gy)
    y = t.run(sis_hip.dconv3x3, xd, wd, bd, d)
    assert _frob(y, ref) < 1e-5
    _figures("y", K.check_dconv3x3(xd, wd, bd, d, y))
    wa = t.run(sis_hip.dconv3x3_adjoint, wd)
    _figures("adjoint", K.check_dconv3x3_adjoint(wd, wa))
    dx = t.run(sis_hip.dconv3x3, gyd, wa, None, d)
    assert _frob(dx, xr.grad) < 1e-5
    dw = t.run(sis_hip.dconv3x3_wgrad, gyd, xd, d)
    assert _frob(dw, wr.grad) < 1e-5
    _figures("dw", K.check_dconv3x3_wgrad(gyd, xd, d, 9, dw))
    dw1 = t.run(sis_hip.dconv3x3_wgrad, gyd, xd, taps=1)
    _figures("dw one tap", K.check_dconv3x3_wgrad(gyd, xd, 1, 1, dw1))
    db = t.run(sis_hip.channel_sum, gyd)
    assert _frob(db, br.grad) < 1e-5
    _figures("db", K.check_channel_sum(gyd, db))
    m = torch.randn(cout, 4 * cin + 3, generator=g)
    md = t.put(m)
    _figures("transpose", K.check_transpose2d(md, t.run(sis_hip.transpose2d, md)))


@case("pixel_shuffle2", ["doc_ufcn.hip"], (3, 5, 3, 7))
def _pixel_shuffle2(t, b, c, h, w):
    """test_pixel_shuffle2_into_and_from_a_wider_buffer: a fresh result and both halves of a wider buffer (the other half stays)."""
    import sis_hip
    import doc_ufcn_checks as K
    g = torch.Generator().manual_seed(c + w)
    x, bias = torch.randn(b, 4 * c, h, w, generator=g), torch.randn(c, generator=g)
    wide = torch.randn(b, 2 * c, 2 * h, 2 * w, generator=g)
    xd, bd, wided = t.put(x), t.put(bias), t.put(wide)
    _figures("fresh", K.check_pixel_shuffle2(xd, bd, t.run(sis_hip.pixel_shuffle2, xd, bd)))
    for off in (0, c):
        for bs in (bd, None):
            out = t.put(torch.full((b, 2 * c, 2 * h, 2 * w), SENTINEL), inplace=True)
            assert t.run(sis_hip.pixel_shuffle2, xd, bs, out=out, channel_offset=off) is out
            _figures(f"shuffle offset={off}", K.check_pixel_shuffle2(xd, bs, out[:, off:off + c]))
            assert torch.equal(out[:, c - off:2 * c - off], torch.full_like(out[:, :c], SENTINEL))
        got = t.run(sis_hip.pixel_shuffle2_grad, wided, c, off)
        _figures(f"unshuffle offset={off}", K.check_pixel_shuffle2_grad(wided[:, off:off + c], got))


@case("max_pool2x2_slice", ["pool_ops.hip", "doc_ufcn.hip"], (3, 5, 12, 20), (3, 4, 6, 10))
def _max_pool2x2_slice(t, b, c, h, w):
    """test_max_pool2x2_slice: both halves of a [B, 2C, H, W] buffer; W = 20 the four-pixel backward kernel, W = 10 the one-pixel one."""
    import sis_hip
    import doc_ufcn_checks as K
    g = torch.Generator().manual_seed(b * 100 + w)
    buf = (torch.randperm(b * 2 * c * h * w, generator=g).float() - b * c * h * w).reshape(b, 2 * c, h, w)
    gy = torch.randn(b, c, h // 2, w // 2, generator=g)
    bufd, gyd = t.put(buf), t.put(gy)
    for off in (c, 0):
        out, arg = t.run(sis_hip.max_pool2x2_slice, bufd, off, c)
        src = bufd[:, off:off + c]
        _figures(f"pool offset={off}", K.check_max_pool2x2(src, out, arg))
        dx = t.run(sis_hip.max_pool2d_backward, gyd, arg, h, w, 2, 2, 0)
        _figures(f"pool backward offset={off}", K.check_max_pool2d_backward(src, gyd, dx))


@case("bn_drop", ["doc_ufcn.hip", "bn_ops.hip"], ((1, 3, 4, 12), 0.0), ((1, 3, 4, 12), 0.4), ((3, 4, 72, 80), 0.4))
def _bn_drop(t, shape, p):
    """test_bn_drop_fwd_into_a_wider_buffer / _eval_mode / test_bn_drop_bwd_from_a_wider_buffer: a partial last wave and mask-word
    group (36 float4s), and two backward slices of which the short last one crosses a sample boundary."""
    import sis_hip
    import doc_ufcn_checks as K
    from test_doc_ufcn_gpu import _keep_dev
    seed_word, site = 0x123456789ABCDEF, 0x0D0C0011
    b, c, h, w = shape
    g = torch.Generator().manual_seed(b * 1000 + c * 10 + h)
    z = torch.randn(b, c, h, w, generator=g) * 2 + 0.3
    gamma, beta = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.1
    wide, dy2 = torch.randn(b, 2 * c, h, w, generator=g), torch.randn(b, c, h, w, generator=g)
    zd, gd, bd, wided, dy2d = t.put(z), t.put(gamma), t.put(beta), t.put(wide), t.put(dy2)
    seed = t.put(torch.tensor([seed_word], dtype=torch.int64)) if p > 0 else None
    keep = _keep_dev(seed_word, site, z.shape, p) if p > 0 else None
    rm, rv = t.put(torch.zeros(c), inplace=True), t.put(torch.ones(c), inplace=True)
    mean, invstd = t.run(sis_hip.bn_stats, zd, rm, rv, 1e-5, 0.1)
    _figures("stats", K.check_bn_stats(zd, torch.zeros(c, device=t.dev), torch.ones(c, device=t.dev), 1e-5, 0.1, mean, invstd, rm, rv))
    y, mask = t.run(sis_hip.bn_drop_fwd, zd, mean, invstd, gd, bd, seed=seed, site=site, drop_p=p)
    _figures("contiguous", K.check_bn_drop_fwd(zd, mean, invstd, gd, bd, False, 1e-5, keep, p, y, mask))
    for off in (0, c):
        out = t.put(torch.full((b, 2 * c, h, w), SENTINEL), inplace=True)
        got, m2 = t.run(sis_hip.bn_drop_fwd, zd, mean, invstd, gd, bd, seed=seed, site=site, drop_p=p, out=out, channel_offset=off)
        assert got is out and torch.equal(out[:, off:off + c], y) and torch.equal(m2, mask)
        assert torch.equal(out[:, c - off:2 * c - off], torch.full_like(y, SENTINEL)), off
    if p == 0:
        ye, me = t.run(sis_hip.bn_drop_fwd, zd, mean, (invstd ** -2 - 1e-3).clamp_min(0.05), gd, bd, eval_mode=True, eps=1e-3, want_mask=False)
        assert me is None
        _figures("eval", K.check_bn_drop_fwd(zd, mean, (invstd ** -2 - 1e-3).clamp_min(0.05), gd, bd, True, 1e-3, None, 0.0, ye, None))
    for off in (0, c):
        part = wided[:, off:off + c].contiguous()
        for second in (None, dy2d):
            sliced = t.run(sis_hip.bn_drop_bwd, wided, zd, mean, invstd, gd, mask, p, channel_offset=off, dy2=second)
            grad = part if second is None else part + second
            _figures(f"bwd offset={off} dy2={second is not None}", K.check_bn_drop_bwd(grad, zd, gd, bd, keep, p, 1e-5, mask, *sliced))
    only = t.run(sis_hip.bn_drop_bwd, None, zd, mean, invstd, gd, mask, p, dy2=dy2d)
    _figures("bwd dy2 only", K.check_bn_drop_bwd(dy2d, zd, gd, bd, keep, p, 1e-5, mask, *only))


@case("weighted_ce", ["doc_ufcn.hip"], (2, 3, 5, 7, True), (1, 3, 4, 12, False))
def _weighted_ce(t, b, k, h, w, weighted):
    """The checks of doc_ufcn_checks.py (1e-5 of the loss / of each plane's largest gradient), with and without class weights."""
    import sis_hip
    import doc_ufcn_checks as K
    g = torch.Generator().manual_seed(b + k + w)
    logits = torch.randn(b, k, h, w, generator=g) * 2
    labels = torch.randint(0, k, (b, h, w), generator=g)
    wts = t.put(torch.tensor([1.0, 2.0, 0.5])) if weighted else None
    ld, lbl = t.put(logits), t.put(labels)
    loss, stats = t.run(sis_hip.weighted_ce_fwd, ld, lbl, wts)
    _figures("loss", K.check_weighted_ce_fwd(ld, lbl, wts, loss, stats))
    gl = t.put(torch.tensor([0.7]))
    grad = t.run(sis_hip.weighted_ce_bwd, gl, ld, lbl, wts, stats)
    _figures("dlogits", K.check_weighted_ce_bwd(gl, ld, lbl, wts, grad))


# =================================================================================================== dataset and page operators
# integer and byte results: equality, as their tests ask

@case("kmeans_assign", ["dataset_ops.hip"], (1, 20, 3, 3, 5), (2, 5, 7, 9, 16), (2, 64, 16, 24, 32))
def _kmeans_assign(t, b, c, h, w, k):
    """test_kmeans_assign_matches_reference_rule (near-duplicate centres), the label map bit for bit; the last shape takes the
    fast first pass, whose list of open pixels lives in a 0xFF-born workspace."""
    import sis_hip
    from oracle import kmeans_ref
    gen = torch.Generator().manual_seed(c + k)
    x, centres = torch.randn(b, c, h, w, generator=gen), torch.randn(k, c, generator=gen)
    centres[1::2] = centres[0:2 * (k // 2):2] * (1 + 1e-7 * torch.randn(k // 2, c, generator=gen))
    ref32, _ = kmeans_ref.predict(x, centres)
    got = t.run(sis_hip.kmeans_assign, t.put(x), t.put(centres))
    assert got.dtype == torch.int64 and torch.equal(got.cpu(), ref32)


@case("make_image_u8", ["dataset_ops.hip"], (3, 3, 32, 40), (1, 3, 5, 7))
def _make_image_u8(t, b, c, h, w):
    """test_make_image_u8: every byte."""
    import sis_hip
    from oracle import kmeans_ref
    x = torch.randn(b, c, h, w, generator=torch.Generator().manual_seed(2)) * 0.8
    x[0, 0, 0, 0], x[0, 1, 0, 0], x[0, 2, 0, 0] = -1.0, 1.0, 0.0
    got = t.run(sis_hip.make_image_u8, t.put(x))
    assert got.dtype == torch.uint8 and torch.equal(got.cpu(), kmeans_ref.make_image(x))


@case("skm_gather_label", ["spherical_kmeans.hip"], (1, 24, 4, 4, 2), (3, 24, 5, 5, 3))
def _skm(t, b, c, h, w, k):
    """test_gather_normalises_the_listed_rows (2 ulp of a unit row) and test_label_pass_equals_the_float64_argmax (labels of the rows
    whose top-2 gap exceeds 1e-5, counts equal to the labels' histogram, unused count slots zero)."""
    import sis_hip
    import spherical_kmeans_restatement as R
    from test_spherical_kmeans_gpu import _bound, _pass_case
    x, xn, cen = _pass_case(b, c, h, w, k, True)
    n = len(x)
    idx = np.random.RandomState(1).randint(0, n, 77).astype(np.int32)
    idx[:3] = (0, n - 1, n // 3)
    xd = t.put(torch.from_numpy(xn))
    got = t.run(sis_hip.skm_gather, xd, t.put(torch.from_numpy(idx))).cpu().numpy()
    assert np.isfinite(got).all() and np.abs(got - R.normalize(x.astype(np.float64))[idx]).max() <= 2 * 2.0 ** -23
    c64 = cen.astype(np.float64)
    score = R.normalize(x.astype(np.float64)) @ c64.T - 0.5 * (c64 * c64).sum(1)[None]
    top = np.sort(score, 1)
    sure, lab64 = (top[:, -1] - top[:, -2]) > 1e-5, score.argmax(1)
    labels, result = t.run(sis_hip.skm_label, xd, t.put(torch.from_numpy(cen)))
    labels, result = labels.cpu().numpy(), result.cpu().numpy()
    assert labels.shape == (n,) and labels.min() >= 0 and labels.max() < k
    assert int((labels[sure] != lab64[sure]).sum()) == 0
    assert np.array_equal(result[1:1 + k], np.bincount(labels, minlength=k)) and (result[1 + k:] == 0).all()
    ine = {dt: float(R.sqdist(R.normalize(x.astype(dt)), cen.astype(dt)).min(1).sum(dtype=np.float64)) for dt in (np.float64, np.float32)}
    assert abs(result[0] - ine[np.float64]) / ine[np.float64] <= _bound(ine[np.float32], ine[np.float64], relative=True)


@case("page_ops", ["page_ops.hip"], (97, 33, 64, 7, 4))
def _page_ops(t, w, h, p, o, c):
    """test_crop_patches_bit_exact, test_assemble_matches_reference_golden (max: bit-exact) and the voting assembly (1e-6 relative
    against the restatement; labels where the top-2 gap exceeds 1e-5), at a page that is no multiple of the patch."""
    import sis_hip
    import page_eval_restatement as PR
    from oracle import analysis_ref as A
    from segmentation.analysis_segmenter import AnalysisSegmenter
    rng = np.random.RandomState(5)
    page = rng.randint(0, 256, size=(h, w, c), dtype=np.uint8)
    xs, ys = AnalysisSegmenter(torch.nn.Identity(), p, t.dev, patch_overlap=o).patch_grid(w, h)
    boxes = A.calculate_bboxes_for_patches(w, h, p, o)
    got = t.run(sis_hip.crop_patches_u8, t.put(torch.from_numpy(page)), xs, ys, p)
    assert torch.equal(got.cpu(), A.crop_patches(page, boxes))
    preds = torch.from_numpy(rng.rand(len(boxes), 3, p, p).astype(np.float32))
    pd = t.put(preds)
    out, labels = t.run(sis_hip.assemble_max, pd, xs, ys, h, w, with_labels=True)
    want = A.assemble_predictions(preds, boxes, w, h)
    assert torch.equal(out.cpu(), want) and torch.equal(labels.cpu().long(), A.label_map(want))
    out, labels = t.run(sis_hip.assemble_vote, pd, xs, ys, h, w, with_labels=True)
    want = PR.assemble_vote(preds, boxes, w, h)
    np.testing.assert_allclose(out.cpu().numpy(), want.numpy(), rtol=1e-6, atol=0)
    top2 = torch.topk(want, 2, dim=0)[0]
    decided = (top2[0] - top2[1]) > 1e-5
    assert torch.equal(labels.cpu().long()[decided], PR.first_max_labels(want)[decided])


@case("confusion_color", ["page_ops.hip"], (5,))
def _confusion_color(t, classes):
    """test_confusion_matrix_is_exact at its odd page sizes (from confidences, from labels, accumulated) and
    test_ground_truth_color_image_to_class_map."""
    import sis_hip
    import page_eval_restatement as PR
    rng = np.random.RandomState(classes)
    total = t.put(torch.zeros((classes, classes), dtype=torch.int64), inplace=True)
    want_total = np.zeros((classes, classes), dtype=np.int64)
    for h, w in [(37, 53), (1, 4099)]:
        gt = rng.randint(0, classes, size=(h, w)).astype(np.uint8)
        conf = (rng.randint(0, 12, size=(classes, h, w)) / 11.0).astype(np.float32)
        labels = torch.argmax(torch.from_numpy(conf), dim=0)
        want = PR.confusion_matrix(labels.numpy(), gt, classes)
        gtd, cd = t.put(torch.from_numpy(gt)), t.put(torch.from_numpy(conf))
        np.testing.assert_array_equal(t.run(sis_hip.confusion_matrix, cd, gtd, classes).cpu().numpy(), want)
        np.testing.assert_array_equal(t.run(sis_hip.confusion_matrix, t.put(labels.to(torch.uint8)), gtd, classes).cpu().numpy(), want)
        assert t.run(sis_hip.confusion_matrix, cd, gtd, classes, out=total) is total
        want_total += want
    np.testing.assert_array_equal(total.cpu().numpy(), want_total)
    palette = np.asarray([[0, 0, 0], [255, 0, 0], [0, 0, 255], [255, 0, 1], [12, 200, 7], [0, 0, 254]], dtype=np.uint8)
    image = palette[np.random.RandomState(4).randint(0, len(palette), size=(123, 77))]
    colors = {"printed_text": [255, 0, 0], "background": [0, 0, 0], "handwritten_text": [0, 0, 255]}
    got = t.run(sis_hip.color_to_class, t.put(torch.from_numpy(image)), [colors["printed_text"], colors["handwritten_text"]], [1, 2], 0)
    want = np.zeros(image.shape[:2], dtype=np.uint8)
    want[(image == np.asarray(colors["printed_text"], dtype=np.uint8)).all(2)] = 1
    want[(image == np.asarray(colors["handwritten_text"], dtype=np.uint8)).all(2)] = 2
    np.testing.assert_array_equal(got.cpu().numpy(), want)


@case("remove_small_contours", ["contour_ops.hip"], (64, 3, 3, 0.45, 400, 0.7, 0), (64, 16, 4, 0.25, 55, 0.7, 2))
def _remove_small_contours(t, p, b, c, density, min_area, min_conf, background):
    """test_contour_filter_bit_exact_on_smooth_noise at its 64 x 64 cases."""
    import sis_hip
    import page_eval_restatement as PR
    from test_page_eval_gpu import _noise
    pred = _noise(p, b, c, density, seed=p + 7 * min_area + b)
    got = t.run(sis_hip.remove_small_contours, t.put(torch.from_numpy(pred)), min_conf, min_area, background)
    assert torch.equal(got.cpu(), PR.remove_small_contours(pred, min_conf, min_area, background))


@case("cluster_segment", ["cluster_segment.hip"], (False, 4), (True, 50))
def _cluster_segment(t, only_keep_overlapping, min_area):
    """test_random_maps: class map, colour image and drop flags byte for byte, the segmenter's class table banded too."""
    import pathlib
    import tempfile
    import sis_hip
    import cluster_segmenter_restatement as CR
    from test_cluster_segmenter_gpu import CLUSTERS, RESOLUTIONS, build
    from segmentation.black_white_handwritten_printed_text_segmenter import FINE_GRAINED_CLASS
    rng = np.random.RandomState(7)
    maps = {k: CR.smooth_cluster_maps(rng, 3, r, CLUSTERS) for k, r in RESOLUTIONS.items()}
    table = CR.random_class_table(rng, RESOLUTIONS, CLUSTERS)
    spec = CR.make_spec(clusters_to_class=table, only_keep_overlapping=only_keep_overlapping, min_class_contour_area=min_area)
    tmp = tempfile.TemporaryDirectory()
    seg = build(pathlib.Path(tmp.name), spec)
    md = [t.put(torch.from_numpy(np.ascontiguousarray(maps[k]))) for k in seg.base_keys]
    lut = t.put(seg._device_table(t.dev).cpu())
    classes = seg.non_background_classes()
    order = ["background"] + classes
    got = t.run(sis_hip.cluster_segment, md, lut, [seg.sources_of[k] for k in seg.keys_for_class_determination],
                [seg.sources_of[k] for k in seg.keys_for_finegrained_segmentation], classes.index(FINE_GRAINED_CLASS),
                [seg.class_id_map[n] for n in order], [seg.class_to_color_map[n][:3] for n in order], seg.image_size,
                seg.only_keep_overlapping, seg.min_class_contour_area)
    want = CR.segment(maps, spec)
    tmp.cleanup()
    for g_, w_ in zip(got, want):
        assert np.array_equal(g_.cpu().numpy(), w_)


@case("augment_warp", ["augment.hip"], ("s32",), ("same",))
def _augment_warp(t, size):
    """test_general_warp_unquantized (0.5 of 255 against the float64 restatement; labels away from rounding boundaries) with the
    elastic fields computed between the bands, and test_elastic_field_matches_gaussian_filter's bound on the field itself."""
    import sis_hip
    import augment_restatement as AR
    from test_augment_gpu import FIELDS, IDENTITY_LUT, _blocks
    from utils.augment_dataset import _resize, _translation, inverse_map, rotation_matrix, shear_matrix
    rng = np.random.default_rng(4583)
    h, w = 45, 83
    out_h, out_w = (h, w) if size == "same" else (32, 32)
    pixels = rng.integers(0, 256, (3, h, w, 3), dtype=np.uint8)
    classes = np.stack([_blocks(rng, h, w) for _ in range(3)])
    fields = t.run(sis_hip.elastic_field, h, w, [f[0] for f in FIELDS], [f[1] for f in FIELDS], seeds=[f[2] for f in FIELDS], device=t.dev)
    assert bool(torch.isfinite(fields).all())
    fields_host = fields.cpu().numpy()
    forward = rotation_matrix(7.5, w, h) @ _translation(3.3, -2.1) @ shear_matrix(20.0, w, h)
    minv = inverse_map(_resize(w, h, out_w, out_h) @ forward)
    slots = [-1, 0, 1]
    dev = lambda a, dtype: t.put(torch.as_tensor(np.ascontiguousarray(a), dtype=dtype))   # noqa: E731
    out = t.run(sis_hip.augment_warp, dev(pixels, torch.uint8), dev(classes, torch.uint8), dev([0, 1, 2], torch.int32),
                dev(np.stack([minv] * 3), torch.float32), dev(np.stack([IDENTITY_LUT] * 3), torch.uint8), dev(slots, torch.int32),
                fields, out_size=(out_h, out_w), quantize=False)
    images, segmented = out["images"].cpu().numpy(), out["segmented"][:, 0].cpu().numpy()
    for b, slot in enumerate(slots):
        values, labels, (sx, sy) = AR.warp(pixels[b], classes[b], minv, IDENTITY_LUT, out_h, out_w, None if slot < 0 else fields_host[slot])
        error = np.abs(AR.decode(images[b]) - values).max()
        assert error <= 0.5, (size, b, error)   # (a NaN compares false)
        unsure = AR.near_rounding_boundary(sx, sy, 1e-3)
        assert unsure.mean() <= 0.02 and np.array_equal(segmented[b][~unsure], labels[~unsure]), (size, b)


@case("pixel_ensemble_label", ["pixel_ensemble.hip"], (3, 3))
def _pixel_ensemble(t, members, classes):
    """test_logits_and_labels_match_fp64 at its smallest configuration (eight layers of 4^2 .. 32^2 to 64^2, no full-resolution layer):
    member logits within 1e-4 of max|logit| of the float64 oracle, labels where every member's top-2 gap exceeds twice that.  The
    activations, the projections, the results are banded; the ensemble's weights are the segmenter's own tensors."""
    import pathlib
    import tempfile
    from test_dataset_gan_gpu import NOFULL, _check_against, _fp64_logits, _segmenter
    size = 64
    with tempfile.TemporaryDirectory() as tmp:
        seg = _segmenter(pathlib.Path(tmp), NOFULL, size, members, classes)
        g = torch.Generator().manual_seed(11)
        acts = {k: t.put(torch.randn(2, c, r, r, generator=g)) for k, c, r in NOFULL}
        labels, rgb, logits = t.run(seg.label_activations, acts, want_logits=True)
    assert labels.dtype == torch.int64 and labels.shape == (2, size, size)
    assert bool(torch.isfinite(logits).all())
    _check_against(logits, labels, _fp64_logits(seg, acts, size))
    assert torch.equal(rgb, torch.from_numpy(seg.colour_table()).to(t.dev)[labels])


# =================================================================================================== the harness itself

@pytest.mark.gpu
def test_harness_sees_a_store_one_element_past_a_view(device):
    """torch ops only: an ``as_strided`` store one element past a banded view (inside the same raw buffer -- an ordinary
    in-allocation store) makes ``check()`` fail; the untouched twin passes."""
    G.reset()
    clean = G.banded(torch.arange(24, dtype=torch.float32).view(2, 3, 4), device)
    clean.mul_(1.0)
    torch.cuda.synchronize()
    G.check()
    G.reset()
    v = G.banded(torch.arange(24, dtype=torch.float32).view(2, 3, 4), device)
    v.as_strided((1,), (1,), v.storage_offset() + v.numel()).fill_(1.0)
    torch.cuda.synchronize()
    with pytest.raises(AssertionError, match="band after"):
        G.check()
    G.reset()


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_guarded(device, monkeypatch, case):
    G.reset()
    try:
        case.fn(T(device, monkeypatch), *case.args)
    finally:
        G.reset()
