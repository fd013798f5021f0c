"""modconv_wino24_kernel<true> (csrc/modconv_wino24.h): the F(2x4,3x3) convolution that also leaves the following ToRGB's channel
sum in blocks of 64 channels, and rgb_finish_kernel (csrc/gen_small_ops.hip), which adds the blocks, the bias and the skip image.

Per shape, with and without skip, with and without noise:
(a) the activation is bit-equal to the convolution without the flag;
(b) the image agrees with the fp64 ToRGB of the oracle on that activation within 2e-5 * max|ref| (the project's per-layer bound);
(c) two calls give the same bits;
(d) a sample of the batch equals the same sample run alone, bit for bit;
(e) small-integer operands with unit style give the exact image.  (e) runs without the fused tail: the activation's gain
    sqrt(2) has no exact product, and without the tail the kernel applies no noise, so (e) has no noise axis.  Weights are
    multiples of 24 with one non-zero tap column per filter: every transformed plane (sixths and twenty-fourths) is then a single
    product that rounds to its exact half-integer, whether or not the compiler contracts the transform's sums into FMAs (with two
    non-zero columns a contracted sum that cancels would show the product's rounding).  The test checks the planes first."""
import functools

import numpy as np
import pytest
import torch

from oracle import ops_ref
from oracle import stylegan2_ref as R

pytestmark = pytest.mark.gpu

NAME = "modconv_wino24_kernel"   # both instantiations report this name; the filled partial-sum buffer tells them apart
# B, Cin, Cout, H, W, tiles per workgroup (the launcher's test override; it must divide the B * tiles-per-sample tiles)
SHAPES = [(2, 8, 64, 16, 32, 2),     # smallest eligible map, one channel block, two chunks; one workgroup walks both samples
          (3, 16, 128, 32, 32, 3),   # two channel blocks, 16 x 32 tile class
          (2, 24, 128, 8, 64, 1),    # 8 x 64 tile class, six chunks
          (2, 8, 192, 32, 64, 4)]    # three blocks, four tiles per sample: the walk crosses tile and sample boundaries
SDIM = 48


def _rel(a, b):
    return (a.double().cpu() - b.double()).abs().max().item() / max(b.abs().max().item(), 1e-30)


@functools.lru_cache(maxsize=None)
def _case(b, cin, cout, h, w):
    """Operands of one convolution + ToRGB pair; computed once, shared, never modified."""
    gen = torch.Generator().manual_seed(b * 1000 + cin + cout + h)
    mk = lambda *s: torch.randn(*s, generator=gen)
    return dict(x=mk(b, cin, h, w), style=mk(b, SDIM), weight=mk(1, cout, cin, 3, 3), mod_w=mk(cin, SDIM), mod_b=1 + 0.1 * mk(cin),
                noise=mk(1, 1, h, w), nw=0.3 * mk(1), bias=0.2 * mk(cout), skip=mk(b, 3, h // 2, w // 2), rgb_style=mk(b, SDIM),
                sd={"p.conv.weight": mk(1, 3, cout, 1, 1), "p.conv.modulation.weight": mk(cout, SDIM),
                    "p.conv.modulation.bias": 1 + 0.1 * mk(cout), "p.bias": 0.1 * mk(1, 3, 1, 1),
                    "p.upsample.kernel": ops_ref.make_kernel([1, 3, 3, 1]) * 4})


def _fused(device, conv, rgb_w, rgb_s, rgb_scale, rgb_bias, skip, taps, tpw):
    """conv: the positional and keyword operands of sis_hip.modconv2d.  Returns (activation, image, kernel name)."""
    import sis_hip
    args, kw = conv
    b, _, h, w = args[0].shape
    cout = args[1].shape[2]
    part = torch.full(sis_hip.rgb_part_shape(b, cout, h, w), float("nan"), device=device)
    act = sis_hip.modconv2d(*args, **kw, rgb=(rgb_w, rgb_s, rgb_scale, part), wino24_tiles_per_wg=tpw)
    name = sis_hip.lib().sis_last_kernel().decode()
    image = sis_hip.rgb_finish(part, rgb_bias, skip, taps if skip is not None else None, (2, 1))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(part).all())   # born NaN: the flagged instantiation wrote every element
    return act, image, name


@pytest.mark.parametrize("with_noise", [False, True])
@pytest.mark.parametrize("with_skip", [False, True])
@pytest.mark.parametrize("b,cin,cout,h,w,tpw", SHAPES)
def test_activation_image_repeat_and_batch(device, b, cin, cout, h, w, tpw, with_skip, with_noise):
    import sis_hip
    C = _case(b, cin, cout, h, w)
    sd = C["sd"]
    d = lambda t: t.to(device)
    assert sis_hip.modconv_wino24_eligible(cin, cout, h, w)
    with torch.no_grad():
        wpk, wsq = sis_hip.modconv_prepack(d(C["weight"]))
        u24 = sis_hip.modconv_prepack_wino24(d(C["weight"]))
        s = sis_hip.equal_linear(d(C["style"]), d(C["mod_w"]), d(C["mod_b"]), 1 / SDIM ** 0.5, 1.0, False)
        ds = sis_hip.modconv_demod(s, wsq, 1 / (cin * 9) ** 0.5, True)
        rgb_s = sis_hip.equal_linear(d(C["rgb_style"]), d(sd["p.conv.modulation.weight"]), d(sd["p.conv.modulation.bias"]),
                                     1 / SDIM ** 0.5, 1.0, False)
        x, bias, rgb_w, rgb_b, taps = d(C["x"]), d(C["bias"]), d(sd["p.conv.weight"]), d(sd["p.bias"]), d(sd["p.upsample.kernel"])
        noise, nw = (d(C["noise"]), d(C["nw"])) if with_noise else (None, None)
        skip = d(C["skip"]) if with_skip else None
        scale = 1 / cout ** 0.5
        conv = lambda lo, hi: ((x[lo:hi].contiguous(), wpk, s[lo:hi].contiguous(), ds[lo:hi].contiguous(), 3, noise, nw, bias),
                               dict(fuse_act=True, wino24_u=u24))
        cargs, ckw = conv(0, b)
        plain = sis_hip.modconv2d(*cargs, **ckw)
        act, image, name = _fused(device, (cargs, ckw), rgb_w, rgb_s, scale, rgb_b, skip, taps, tpw)
        assert name == NAME
        # (a)
        assert torch.equal(act, plain)
        # (b)
        sd64 = {k: v.double() for k, v in sd.items()}
        ref = R.to_rgb(sd64, "p", act.double().cpu(), C["rgb_style"].double(), C["skip"].double() if with_skip else None)
        err = _rel(image, ref)
        print(f"wino24 rgb B{b} {cin}->{cout} {h}x{w} skip={int(with_skip)} noise={int(with_noise)}: {err:.3e}")
        assert bool(torch.isfinite(image).all()) and err < 2e-5, err
        # (c)
        act2, image2, _ = _fused(device, (cargs, ckw), rgb_w, rgb_s, scale, rgb_b, skip, taps, tpw)
        assert torch.equal(act2, act) and torch.equal(image2, image)
        # (d)
        k = b - 1
        _, image_k, name = _fused(device, conv(k, k + 1), rgb_w, rgb_s[k:k + 1].contiguous(), scale, rgb_b,
                                  None if skip is None else skip[k:k + 1].contiguous(), taps, 1)
        assert name == NAME and torch.equal(image_k[0], image[k])


@pytest.mark.parametrize("with_skip", [False, True])
@pytest.mark.parametrize("b,cin,cout,h,w,tpw", SHAPES)
def test_small_integers_give_the_exact_image(device, b, cin, cout, h, w, tpw, with_skip):
    """(e).  |activation| <= 9 * 24 * 2 * Cin <= 10368 and |image| <= 2 * 192 * 10368 + skip + bias < 2^24: every sum is an integer
    that fp32 holds, so the order of the channel sum cannot show."""
    import sis_hip
    from test_wino24_cpu import G2, G4
    gen = torch.Generator().manual_seed(7 * b + cin + cout + h)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=gen).float()
    x = ri(-2, 2, b, cin, h, w)
    column = torch.nn.functional.one_hot(torch.randint(0, 3, (1, cout, cin, 1), generator=gen), 3).float()
    weight = 24 * ri(-1, 1, 1, cout, cin, 3, 3) * column
    rgb_w, rgb_b, skip = ri(-2, 2, 1, 3, cout, 1, 1), ri(-3, 3, 1, 3, 1, 1), 16 * ri(-4, 4, b, 3, h // 2, w // 2)
    taps = ops_ref.make_kernel([1, 3, 3, 1]) * 4
    d = lambda t: t.to(device)
    with torch.no_grad():
        wpk, _ = sis_hip.modconv_prepack(d(weight))
        u24 = sis_hip.modconv_prepack_wino24(d(weight))
        # the transformed planes are exact (same un-shuffle as tests/test_wino24_guard_bands_gpu.py::test_prepack_wino24)
        u_ref = np.einsum("ia,ocab,jb->ocij", G2, weight[0].numpy().astype(np.float64), G4)
        assert np.abs(u_ref - np.round(2 * u_ref) / 2).max() < 1e-9
        u_ref = np.round(2 * u_ref) / 2
        u_got = u24.cpu().numpy().astype(np.float64)
        u_got = u_got.transpose(0, 1, 3, 2, 4).reshape(cin, 2, cout, 4, 3).transpose(2, 0, 3, 1, 4).reshape(cout, cin, 4, 6)
        assert np.array_equal(u_got, u_ref)
        ones = lambda n: torch.ones(b, n, device=device)
        conv = ((d(x), wpk, ones(cin), ones(cout), 3), dict(fuse_act=False, wino24_u=u24))
        act, image, name = _fused(device, conv, d(rgb_w), ones(cout), 1.0, d(rgb_b), d(skip) if with_skip else None, d(taps), tpw)
    assert name == NAME
    act_ref = torch.nn.functional.conv2d(x.double(), weight[0].double(), padding=1)
    assert torch.equal(act.double().cpu(), act_ref)
    ref = torch.einsum("co,bohw->bchw", rgb_w[0, :, :, 0, 0].double(), act_ref) + rgb_b.double()
    if with_skip:
        ref = ref + ops_ref.upfirdn2d(skip.double(), taps.double(), up=2, down=1, pad=(2, 1))
    assert ref.abs().max().item() < 2 ** 24
    assert torch.equal(image.double().cpu(), ref)
