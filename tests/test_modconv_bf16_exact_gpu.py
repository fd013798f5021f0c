"""modconv_bf16_kernel (csrc/modconv_bf16.h) bit for bit, on the exactly summable operands of tests/exact_operands.py.

x and W are integers in [-r, r] with 9 cin r^2 < 2^23, the style factor is 0.5 or 1 per (sample, channel) -- so s * x is a bf16
value and every partial sum an exact fp32 value in any order --, dscale is 0.25, 0.5 or 1.  Without the tail the result must
equal the float64 convolution; with it, integer noise and bias and noise_weight = 0.5 keep the pre-activation exact and the
result is within 2 units in the last place of the float64 tail evaluated with the fp32 constants (the tail rounds twice:
the product with 0.2 and the product with sqrt(2)).

Shapes: the smallest that reach every path of the launch plan -- both output-channel tiles (64; 128, whole and ragged at
Cout = 192), both pixel tiles (8 x 32 up to 32 wide, 4 x 64 beyond), a one-tile map, partial tiles in H only, in W only and in
both, one chunk, a half-empty last chunk (Cin = 24), two chunks, the deep contraction of the generator (Cin = 512), B = 1, 3, 5."""
import functools

import pytest
import torch

import exact_operands as E
import modconv_bf16_checks as M

pytestmark = pytest.mark.gpu

KERNEL = "modconv_bf16_kernel"

SHAPES = [(1, 16, 64, 8, 32),      # 64-channel tile, one 8 x 32 tile, one chunk
          (1, 16, 128, 8, 32),     # 128-channel tile, the same map
          (3, 32, 192, 4, 64),     # ragged channel tile (128 + 64), one 4 x 64 tile, two chunks, three samples
          (1, 16, 64, 12, 32),     # partial tile in H only
          (1, 24, 128, 8, 40),     # partial tile in W only, half-empty last chunk
          (5, 16, 64, 10, 72),     # partial tiles in H and in W, five samples
          (1, 512, 64, 32, 32)]    # the deep contraction: 32 chunks


@functools.lru_cache(maxsize=None)
def _case(b, cin, cout, h, w):
    """Operands and the two float64 references; computed once, shared, never modified."""
    r = E.radius(9 * cin)
    E.check_operands(9 * cin, r, r, 2)
    gen = torch.Generator().manual_seed(b * 1000 + cin + cout + h)
    x = E.integers((b, cin, h, w), r, gen, dtype=torch.float32)
    wt = E.integers((cout, cin, 3, 3), r, gen, dtype=torch.float32)
    s = torch.tensor([0.5, 1.0])[torch.randint(0, 2, (b, cin), generator=gen)]
    dscale = torch.tensor([0.25, 0.5, 1.0])[torch.randint(0, 3, (b, cout), generator=gen)]
    noise = E.integers((1, 1, h, w), 7, gen, dtype=torch.float32)
    bias = E.integers((cout,), 7, gen, dtype=torch.float32)
    xm = x * s.view(b, cin, 1, 1)
    assert torch.equal(M.rne(xm), xm) and torch.equal(M.rne(wt), wt)        # both operands are bf16 values
    ref = dscale.double().view(b, cout, 1, 1) * E.conv_ref(xm, wt)
    plain = E.exact_f32(ref, unit=0.125)
    pre = E.check_reference(ref + 0.5 * noise.double() + bias.double().view(1, -1, 1, 1), unit=0.125)
    return dict(x=x, w=wt, s=s, dscale=dscale, noise=noise, nw=torch.tensor([0.5]), bias=bias, plain=plain,
                fused=M.tail64(pre, torch.zeros(1, 1, 1, 1), 0.0, torch.zeros(cout)))


def _run(device, L, fuse):
    import sis_hip
    d = lambda t: t.to(device)
    cout, cin = L["w"].shape[:2]
    wpk = torch.empty((cin, 9, cout), device=device)     # only its shape is read on this route
    packed = sis_hip.modconv_prepack_bf16(d(L["w"]).unsqueeze(0))
    y = sis_hip.modconv2d(d(L["x"]), wpk, d(L["s"]), d(L["dscale"]), 3, d(L["noise"]) if fuse else None,
                          d(L["nw"]) if fuse else None, d(L["bias"]) if fuse else None, fuse_act=fuse, bf16_w=packed)
    torch.cuda.synchronize()
    assert sis_hip.lib().sis_last_kernel().decode() == KERNEL
    return y.cpu()


@pytest.mark.parametrize("b,cin,cout,h,w", SHAPES)
def test_plain_is_the_exact_result(device, b, cin, cout, h, w):
    import sis_hip
    assert sis_hip.modconv_bf16_eligible(cin, cout, h, w)
    L = _case(b, cin, cout, h, w)
    E.assert_bitwise(_run(device, L, False), L["plain"], f"modconv_bf16 B{b} {cin}->{cout} {h}x{w}", tile=(8, 32) if w <= 32 else (4, 64))


@pytest.mark.parametrize("b,cin,cout,h,w", SHAPES)
def test_fused_tail_within_two_ulp(device, b, cin, cout, h, w):
    L = _case(b, cin, cout, h, w)
    got, want = _run(device, L, True).double(), L["fused"]
    _, exponent = torch.frexp(want.float().abs())
    ulp = torch.ldexp(torch.ones_like(want), exponent.to(torch.int32) - 24)     # spacing of fp32 at |want| (want = m 2^e, m in [0.5, 1))
    err = (got - want).abs()
    assert bool(((err <= 2 * ulp) & ((want != 0) | (got == 0))).all()), \
        f"B{b} {cin}->{cout} {h}x{w}: {int((err > 2 * ulp).sum())} elements off by more than 2 ulp, worst {float((err / ulp).max()):.2f} ulp"
    # the positive branch rounds once
    pos = want > 0
    assert bool((err[pos] <= ulp[pos]).all())
