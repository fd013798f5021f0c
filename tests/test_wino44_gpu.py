"""modconv_wino44_kernel (csrc/modconv_wino44.h, Winograd F(4x4,3x3)) against a float64 direct convolution.

The kernel computes out[b, co] = tail(dscale[b, co] * sum_ci conv3x3(w[co, ci], s[b, ci] * x[b, ci])); the tests hand it s and dscale
directly.  Tile classes: one-sample tiles of 512 pixels, 8 x 64 (maps wider than 32) or 16 x 32, as 32 tiles of 4 x 4; a chunk is
4 input channels, chunks run in pairs.  Every case is asserted at 2e-5 * max|ref|, the project's per-layer bound.  Measured on
MI355X: 2.7e-6 .. 4.1e-6 on the 8- to 24-channel shapes, 7.1e-6 / 9.8e-6 / 1.2e-5 .. 1.8e-5 at Cin = 128 / 256 / 512
(profiles/wino44_layers.txt)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

NAME = "modconv_wino44_kernel"
BOUND = 2e-5


def _rel(a, b):
    return (a.double().cpu() - b.double()).abs().max().item() / max(b.abs().max().item(), 1e-30)


def _reference(x, w, s, ds, noise=None, nw=None, bias=None, fuse=False):
    y = F.conv2d(x.double() * s.double()[:, :, None, None], w[0].double(), padding=1) * ds.double()[:, :, None, None]
    if not fuse:
        return y
    if noise is not None:
        y = y + nw.double() * noise.double()
    if bias is not None:
        y = y + bias.double()[None, :, None, None]
    return torch.where(y > 0, y, 0.2 * y) * 2 ** 0.5


@functools.lru_cache(maxsize=None)
def _layer(b, cin, cout, h, w):
    """Operands and float64 results (plain, fused tail) of one layer; computed once, shared, never modified."""
    gen = torch.Generator().manual_seed(b * 1000 + cin + cout + h + 7 * w)
    mk = lambda *s: torch.randn(*s, generator=gen)
    L = dict(x=mk(b, cin, h, w), w=mk(1, cout, cin, 3, 3), s=1 + 0.3 * mk(b, cin), ds=(0.5 + torch.rand(b, cout, generator=gen)) / (3 * cin ** 0.5),
             noise=mk(1, 1, h, w), nw=0.3 * mk(1), bias=0.2 * mk(cout))
    L["ref"] = _reference(L["x"], L["w"], L["s"], L["ds"])
    L["ref_act"] = _reference(L["x"], L["w"], L["s"], L["ds"], L["noise"], L["nw"], L["bias"], fuse=True)
    return L


def _run(device, x, w, s, ds, noise=None, nw=None, bias=None, fuse=False, tpw=0, rgb=None, u44=None):
    import sis_hip
    d = lambda t: None if t is None else t.to(device)
    with torch.no_grad():
        wpk, _ = sis_hip.modconv_prepack(d(w))
        if u44 is None:
            u44 = sis_hip.modconv_prepack_wino44(d(w))
        y = sis_hip.modconv2d(d(x), wpk, d(s).contiguous(), d(ds).contiguous(), 3, d(noise), d(nw), d(bias), fuse_act=fuse, wino44_u=u44,
                              wino44_tiles_per_wg=tpw, rgb=rgb)
    torch.cuda.synchronize()
    assert sis_hip.lib().sis_last_kernel().decode() == NAME
    return y


def _run_layer(device, L, fuse, lo=0, hi=None, **kw):
    tail = dict(noise=L["noise"], nw=L["nw"], bias=L["bias"]) if fuse else {}
    return _run(device, L["x"][lo:hi], L["w"], L["s"][lo:hi], L["ds"][lo:hi], fuse=fuse, **tail, **kw)


SHAPES = [(1, 8, 64, 16, 32),      # one tile, two chunks: the shortest pipeline
          (1, 24, 128, 16, 32),    # odd chunk-pair count, a second output-channel block
          (1, 8, 64, 8, 64),       # the other tile class: image borders on all four sides of one tile
          (3, 8, 64, 32, 32),      # two tiles per sample, three samples
          (3, 8, 64, 16, 128),     # 8 x 64 tiles, four per sample
          (1, 8, 64, 12, 64),      # rows that do not fill the last tile
          (1, 16, 64, 20, 96),     # partial tiles in H and in W
          (1, 512, 64, 16, 32)]    # one deep contraction: 128 chunks


@pytest.mark.parametrize("fuse", [False, True])
@pytest.mark.parametrize("b,cin,cout,h,w", SHAPES)
def test_kernel_vs_float64(device, b, cin, cout, h, w, fuse):
    import sis_hip
    L = _layer(b, cin, cout, h, w)
    assert sis_hip.modconv_wino44_eligible(cin, cout, h, w)
    err = _rel(_run_layer(device, L, fuse), L["ref_act"] if fuse else L["ref"])
    print(f"wino44 B{b} {cin}->{cout} {h}x{w} fuse={int(fuse)}: {err:.3e}")
    assert err < BOUND, err


# The generator's layers at their own (Cin, Cout) on a map of one tile row.  Measured on MI355X: profiles/wino44_layers.txt.
@pytest.mark.parametrize("cin,cout,h,w", [(512, 512, 16, 32), (512, 512, 8, 64), (256, 256, 8, 128), (128, 128, 8, 256)])
def test_generator_layers_on_one_tile_row(device, cin, cout, h, w):
    L = _layer(1, cin, cout, h, w)
    err = _rel(_run_layer(device, L, True), L["ref_act"])
    print(f"wino44 layer {cin}->{cout} on {h}x{w}: {err:.3e} of max|ref|")
    assert err < BOUND, err


def _probe_weight():
    return torch.randn(1, 64, 8, 3, 3, generator=torch.Generator().manual_seed(11))


def test_impulse_at_every_patch_position(device):
    """One non-zero input pixel per sample: the 36 patch positions of the corner tile (rows -1..4, columns -1..4; those outside
    the image have no pixel) and of an inner tile of a 16 x 32 map.  A wrong plane index shows in one sample."""
    w, h, wd = _probe_weight(), 16, 32
    spots = [(ty + r, tx + c) for ty, tx in ((0, 0), (4, 8), (12, 28)) for r in range(-1, 5) for c in range(-1, 5)]
    spots = [(y, x) for y, x in spots if 0 <= y < h and 0 <= x < wd]
    x = torch.zeros(len(spots), 8, h, wd)
    for b, (y, xx) in enumerate(spots):
        x[b, b % 8, y, xx] = 1.0 + b / 64
    s, ds = torch.ones(len(spots), 8), torch.ones(len(spots), 64)
    got, ref = _run(device, x, w, s, ds).double().cpu(), _reference(x, w, s, ds)
    for b, spot in enumerate(spots):
        assert (got[b] - ref[b]).abs().max().item() < BOUND * ref[b].abs().max().item(), spot


def test_impulse_at_every_weight_tap(device):
    L = _layer(1, 8, 64, 16, 32)
    for tap in range(9):
        w = torch.zeros(1, 64, 8, 3, 3)
        w[0, :, :, tap // 3, tap % 3] = _probe_weight()[0, :, :, tap // 3, tap % 3]
        err = _rel(_run(device, L["x"], w, L["s"], L["ds"]), _reference(L["x"], w, L["s"], L["ds"]))
        assert err < BOUND, (tap, err)


def test_impulse_at_every_channel_of_a_chunk_pair(device):
    """Sample b holds input channel b only: a wrong lane group (channel of the MFMA step) or chunk parity shows in one sample."""
    L, w = _layer(1, 8, 64, 16, 32), _probe_weight()
    x = torch.zeros(8, 8, 16, 32)
    for b in range(8):
        x[b, b] = L["x"][0, b]
    s, ds = L["s"].expand(8, -1), L["ds"].expand(8, -1)
    got, ref = _run(device, x, w, s, ds).double().cpu(), _reference(x, w, s, ds)
    for b in range(8):
        assert (got[b] - ref[b]).abs().max().item() < BOUND * ref[b].abs().max().item(), b


@pytest.mark.parametrize("term", ["demodulation", "noise", "bias"])
def test_epilogue_terms_one_by_one(device, term):
    """Each term of the tail alone, behind the leaky ReLU (about half of the pre-activations are negative: the slope shows)."""
    L = _layer(3, 8, 64, 32, 32)
    ones = torch.ones_like(L["ds"]) / 8
    kw = dict(ds=L["ds"] if term == "demodulation" else ones, noise=L["noise"] if term == "noise" else None,
              nw=L["nw"] if term == "noise" else None, bias=L["bias"] if term == "bias" else None)
    ref = _reference(L["x"], L["w"], L["s"], fuse=True, **kw)
    assert (ref < 0).float().mean().item() > 0.3
    err = _rel(_run(device, L["x"], L["w"], L["s"], fuse=True, **kw), ref)
    assert err < BOUND, err


def test_batch_and_walk_independence(device):
    """A sample alone against the same sample inside B = 3, and 1, 2, 3 and 6 tiles per workgroup on the 6 tiles: the same bits."""
    L = _layer(3, 8, 64, 32, 32)
    ys = [_run_layer(device, L, True, tpw=n) for n in (1, 2, 3, 6)]
    assert _rel(ys[0], L["ref_act"]) < BOUND
    for y in ys[1:]:
        assert torch.equal(y, ys[0])
    for k in range(3):
        assert torch.equal(_run_layer(device, L, True, lo=k, hi=k + 1)[0], ys[0][k])


@pytest.mark.parametrize("b,cin,cout,h,w,tpw", [(2, 8, 64, 16, 32, 2), (3, 16, 128, 32, 32, 3), (2, 24, 128, 8, 64, 1), (1, 8, 192, 12, 64, 1)])
def test_rgb_instantiation(device, b, cin, cout, h, w, tpw):
    """modconv_wino44_kernel<true>: the same activation bits, channel-block sums within the bound of their float64 values, and a
    finished image that matches to_rgb_kernel on that activation."""
    import sis_hip
    L = _layer(b, cin, cout, h, w)
    gen = torch.Generator().manual_seed(cout + h)
    rgb_w, rgb_s, rgb_b = torch.randn(3, cout, generator=gen), 1 + 0.3 * torch.randn(b, cout, generator=gen), 0.1 * torch.randn(1, 3, 1, 1, generator=gen)
    skip, taps = torch.randn(b, 3, h // 2, w // 2, generator=gen), torch.tensor([1., 3., 3., 1.])
    taps = (taps[:, None] * taps[None, :]) / 16
    scale = 1 / cout ** 0.5
    d = lambda t: t.to(device)
    plain = _run_layer(device, L, True, tpw=tpw)
    part = torch.full(sis_hip.rgb_part_shape(b, cout, h, w), float("nan"), device=device)
    act = _run_layer(device, L, True, tpw=tpw, rgb=(d(rgb_w), d(rgb_s), scale, part))
    assert torch.equal(act, plain)
    assert bool(torch.isfinite(part).all())   # born NaN: every element written
    wr = scale * rgb_w.double()[None] * rgb_s.double()[:, None]                                # [B, 3, Cout]
    sums = torch.einsum("bkco,bkohw->kbchw", wr.view(b, 3, cout // 64, 64).transpose(1, 2), act.double().cpu().view(b, cout // 64, 64, h, w))
    assert (part.double().cpu() - sums).abs().max().item() < BOUND * sums.abs().max().item()
    image = sis_hip.rgb_finish(part, d(rgb_b), d(skip), d(taps), (2, 1))
    image_ref = sis_hip.to_rgb(act, d(rgb_w).view(1, 3, cout, 1, 1), d(rgb_s), d(rgb_b), scale, d(skip), d(taps), (2, 1))
    torch.cuda.synchronize()
    assert _rel(image, image_ref.cpu()) < BOUND
    # a sample alone: the same sums, bit for bit
    k = b - 1
    part_k = torch.full(sis_hip.rgb_part_shape(1, cout, h, w), float("nan"), device=device)
    _run_layer(device, L, True, lo=k, hi=k + 1, rgb=(d(rgb_w), d(rgb_s[k:k + 1]).contiguous(), scale, part_k))
    assert torch.equal(part_k[:, 0], part[:, k])


DECLINED = [(12, 64, 16, 32),   # Cin % 8
            (8, 32, 16, 32),    # Cout % 64
            (8, 64, 18, 32),    # H % 4
            (8, 64, 64, 16)]    # W <= 16


@pytest.mark.parametrize("cin,cout,h,w", DECLINED)
def test_declined_shapes_are_refused_with_an_error(device, cin, cout, h, w):
    import sis_hip
    assert not sis_hip.modconv_wino44_eligible(cin, cout, h, w)
    x, wt = torch.zeros(1, cin, h, w, device=device), torch.zeros(1, cout, cin, 3, 3, device=device)
    s, ds, out = torch.ones(1, cin, device=device), torch.ones(1, cout, device=device), torch.full((1, cout, h, w), 7.0, device=device)
    u44 = sis_hip.modconv_prepack_wino44(wt)
    p = lambda t: t.data_ptr()
    rc = sis_hip.lib().sis_modconv2d_wino44(p(out), p(x), p(u44), p(s), p(ds), None, 0, None, None, 1, cin, cout, h, w, 0, 0, None)
    torch.cuda.synchronize()
    assert rc != 0 and "not eligible" in sis_hip.lib().sis_last_error().decode()
    assert bool((out == 7.0).all())   # nothing was launched
    with pytest.raises(RuntimeError):
        wpk, _ = sis_hip.modconv_prepack(wt)
        sis_hip.modconv2d(x, wpk, s, ds, 3, wino44_u=u44)


def test_prepack(device):
    """u[ci][row][co][k] against (G g G^T) in float64: 1e-6 relative."""
    import sis_hip
    import wino44_restatement as W
    cout, cin = 72, 24
    w = torch.randn(1, cout, cin, 3, 3, generator=torch.Generator().manual_seed(5))
    u = sis_hip.modconv_prepack_wino44(w.to(device)).cpu().numpy().astype(np.float64)
    assert u.shape == (cin, 9, cout, 4)
    ref = W.weight_planes(w[0].numpy().astype(np.float64))
    assert np.abs(W.unshuffle_u(u) - ref).max() <= 1e-6 * np.abs(ref).max()


def test_profiler_record(device):
    import sis_hip
    L = _layer(1, 8, 64, 16, 32)
    rec = []
    sis_hip.set_profiler(rec)
    try:
        _run_layer(device, L, True)
    finally:
        sis_hip.set_profiler(None)
    convs = [r for r in rec if r[0] == NAME]
    assert len(convs) == 1 and convs[0][1] == 0.5625 * 2.0 * 1 * 64 * 8 * 9 * 16 * 32   # direct form x 9/16 (see the record site)
