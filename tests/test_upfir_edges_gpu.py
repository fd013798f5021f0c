"""The fast-FIR up-convolution (csrc/modconv_upfir.hip) computes its result in two passes: the 25-product kernel on the
2 x 2 position blocks of the H x W interior (T rows 0 .. 2H - 1, columns 0 .. 2W - 1) and an edge pass with the five products
that are not multiplications by padding for T row 2H, T column 2W and the corner.  Shapes as the generator runs them (many
channel chunks, grids of whole rounds), non-square maps, an odd number of block rows and tiles that cross from one sample
into the next; row 2H, column 2W and the corner are each held to the tolerance on their own, measured against their own
max|ref|, so that a wrong edge cannot hide inside a maximum taken over the interior.

Tolerance: the per-layer bound of every generator kernel (tests/test_generator_gpu.py), |err| <= 2e-5 * max|ref|."""
import pytest
import torch

from oracle import ops_ref
from oracle import stylegan2_ref as R

pytestmark = pytest.mark.gpu

TOL = 2e-5


def _rel(a, b):
    return (a.double().cpu() - b.double()).abs().max().item() / max(b.abs().max().item(), 1e-30)


def _mk(gen, *shape):
    return torch.randn(*shape, generator=gen)


# (3, 16, 64, 18, 20): 90 interior blocks per sample, 32-block tiles 2, 5 and 8 hold blocks of two samples (64-block tiles: 1 and 2)
# (2, 24, 64, 34, 40): 17 block rows of 20, tile 10 crosses; (5, 8, 64, 32, 36): 288 blocks per sample
@pytest.mark.parametrize("b,cin,cout,h,w", [(8, 64, 64, 64, 64), (8, 64, 128, 128, 128), (32, 16, 512, 32, 32), (32, 16, 512, 16, 16),
                                             (2, 24, 64, 34, 40), (3, 16, 64, 18, 20), (5, 8, 64, 32, 36), (2, 16, 128, 64, 16)])
def test_modconv_up_fir_interior_and_edges(device, b, cin, cout, h, w):
    import sis_hip
    gen = torch.Generator().manual_seed(b * 257 + cin + cout + 3 * h + w)
    x, style = _mk(gen, b, cin, h, w), _mk(gen, b, 32)
    weight, mod_w, mod_b = _mk(gen, 1, cout, cin, 3, 3), _mk(gen, cin, 32), 1 + 0.1 * _mk(gen, cin)
    noise, nw, bias = _mk(gen, b, 1, 2 * h, 2 * w), 0.3 * _mk(gen, 1), 0.2 * _mk(gen, cout)
    taps = ops_ref.make_kernel([1, 3, 3, 1]) * 4
    with torch.no_grad():
        s_ref = R.equal_linear(style, mod_w, mod_b).view(b, 1, cin, 1, 1)
        wt = (1 / (cin * 9) ** 0.5) * weight * s_ref
        wt = wt * torch.rsqrt(wt.pow(2).sum([2, 3, 4]) + 1e-8).view(b, cout, 1, 1, 1)
        t_ref = torch.nn.functional.conv_transpose2d(x.reshape(1, b * cin, h, w),
                                                     wt.transpose(1, 2).reshape(b * cin, cout, 3, 3), stride=2,
                                                     groups=b).view(b, cout, 2 * h + 1, 2 * w + 1)
        ref_act = ops_ref.fused_leaky_relu(R.modulated_conv2d(x, style, weight, mod_w, mod_b, True, True, taps) + nw * noise, bias)
        d = lambda t: t.to(device)
        wpk, wsq = sis_hip.modconv_prepack(d(weight))
        fir_u = sis_hip.modconv_prepack_up_fir(d(weight))
        s = sis_hip.equal_linear(d(style), d(mod_w), d(mod_b), 1 / 32 ** 0.5, 1.0, False)
        ds = sis_hip.modconv_demod(s, wsq, 1 / (cin * 9) ** 0.5, True)
        assert sis_hip.lib().sis_modconv_up_fir_supported(b, cin, cout, h, w, 2 * w + 4)
        records = []
        sis_hip.set_profiler(records)
        try:
            tp = sis_hip.modconv2d_up(d(x), wpk, s, ds, padded_rows=True, fir_u=fir_u)
        finally:
            sis_hip.set_profiler(None)
        assert [r[0] for r in records] == ["modconv_upfir_kernel"]          # both passes: one call, one record
        assert tuple(tp.shape) == (b, cout, 2 * h + 1, 2 * w + 4)
        t = tp[..., :2 * w + 1].cpu()
        regions = {"whole map": (t, t_ref),
                   "interior": (t[:, :, :2 * h, :2 * w], t_ref[:, :, :2 * h, :2 * w]),
                   "row 2H": (t[:, :, 2 * h, :], t_ref[:, :, 2 * h, :]),
                   "column 2W": (t[:, :, :, 2 * w], t_ref[:, :, :, 2 * w]),
                   "corner": (t[:, :, 2 * h, 2 * w], t_ref[:, :, 2 * h, 2 * w])}
        errs = {name: _rel(got, want) for name, (got, want) in regions.items()}
        print(f"up_fir {b} x ({cin} -> {cout}) on {h} x {w}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
        for name, e in errs.items():
            assert e < TOL, (name, e)
        assert torch.isfinite(tp).all()                                     # pad columns 2W+1 .. 2W+3: written, finite
        again = sis_hip.modconv2d_up(d(x), wpk, s, ds, padded_rows=True, fir_u=fir_u)
        assert torch.equal(again[..., :2 * w + 1], tp[..., :2 * w + 1])
        yp = sis_hip.blur_noise_act(tp, d(taps), (1, 1), d(noise), d(nw), d(bias), fuse_act=True, in_w=2 * w + 1)
        e = _rel(yp, ref_act)
        print(f"  through blur + noise + bias + activation: {e:.2e}")
        assert e < TOL, e


def test_modconv_up_fir_edges_equal_the_four_phase_kernel_where_inputs_are_exact(device):
    """Small-integer inputs, unit style factors: every product and partial sum is an exact fp32 integer, so the interior pass,
    the edge pass and the 4-phase gather kernel must agree to the bit before demodulation scales them alike -- row 2H, column 2W
    and the corner included."""
    import sis_hip
    b, cin, cout, h, w = 3, 16, 64, 18, 20
    gen = torch.Generator().manual_seed(5)
    x = torch.randint(-4, 5, (b, cin, h, w), generator=gen).float()
    weight = torch.randint(-3, 4, (1, cout, cin, 3, 3), generator=gen).float()
    s = torch.ones(b, cin)
    ds = torch.full((b, cout), 0.25)
    with torch.no_grad():
        t_ref = 0.25 * torch.nn.functional.conv_transpose2d(x, weight[0].transpose(0, 1).contiguous(), stride=2)
        d = lambda t: t.to(device)
        wpk, _ = sis_hip.modconv_prepack(d(weight))
        fir_u = sis_hip.modconv_prepack_up_fir(d(weight))
        tp = sis_hip.modconv2d_up(d(x), wpk, d(s), d(ds), padded_rows=True, fir_u=fir_u)
        t4 = sis_hip.modconv2d_up(d(x), wpk, d(s), d(ds), padded_rows=True)
    assert torch.equal(tp[..., :2 * w + 1].cpu(), t_ref)
    assert torch.equal(tp[..., :2 * w + 1], t4[..., :2 * w + 1])
    assert torch.isfinite(tp).all()
