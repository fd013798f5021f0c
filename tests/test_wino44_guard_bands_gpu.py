"""Guard-band cases (tests/guard_bands.py) of the Winograd F(4x4,3x3) entries, in the manner of tests/test_wino24_guard_bands_gpu.py
and tests/test_wino24_rgb_guard_bands_gpu.py: input, weight image, result and partial-sum buffer between 0xFF bands, results born
NaN, on a one-tile, a multi-tile and a partial-tile shape.  Reference and bound as tests/test_wino24_gpu.py (2e-5 * max|ref|)."""
import numpy as np
import pytest
import torch

import guard_bands as G
from test_guard_bands_gpu import T, _mk, _modconv_operands, _rel

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _fresh_session():
    G.reset()
    yield
    G.reset()


@pytest.mark.parametrize("b,cin,cout,h,w", [(1, 8, 64, 16, 32),      # one tile
                                             (2, 16, 128, 32, 64),    # four tiles per sample, two channel blocks
                                             (1, 24, 64, 20, 72)])    # partial tiles in H and in W
def test_modconv2d_wino44_rgb_and_finish(device, monkeypatch, b, cin, cout, h, w):
    import sis_hip
    from oracle import ops_ref
    from oracle import stylegan2_ref as R
    t = T(device, monkeypatch)
    gen = torch.Generator().manual_seed(b * 1000 + cin + cout + h)
    x = _mk(gen, b, cin, h, w)
    style, weight, mod_w, mod_b, wpk, s, ds = _modconv_operands(t, gen, b, cin, cout, 48)
    noise, nw, bias = _mk(gen, 1, 1, h, w), 0.3 * _mk(gen, 1), 0.2 * _mk(gen, cout)
    sd = {"p.conv.weight": _mk(gen, 1, 3, cout, 1, 1), "p.conv.modulation.weight": _mk(gen, cout, 48),
          "p.conv.modulation.bias": 1 + 0.1 * _mk(gen, cout), "p.bias": 0.1 * _mk(gen, 1, 3, 1, 1),
          "p.upsample.kernel": ops_ref.make_kernel([1, 3, 3, 1]) * 4}
    rgb_style, skip = _mk(gen, b, 48), _mk(gen, b, 3, h // 2, w // 2)
    with torch.no_grad():
        ref = ops_ref.fused_leaky_relu(R.modulated_conv2d(x, style, weight, mod_w, mod_b, demodulate=True) + nw * noise, bias)
    u44 = t.run(sis_hip.modconv_prepack_wino44, t.put(weight))
    # the plain instantiation
    y0 = t.run(sis_hip.modconv2d, t.put(x), wpk, s, ds, 3, t.put(noise), t.put(nw), t.put(bias), fuse_act=True, wino44_u=u44)
    assert sis_hip.lib().sis_last_kernel().decode() == "modconv_wino44_kernel"
    assert _rel(y0, ref) < 2e-5, _rel(y0, ref)
    # the one that also leaves the channel sums
    rgb_s = t.run(sis_hip.equal_linear, t.put(rgb_style), t.put(sd["p.conv.modulation.weight"]), t.put(sd["p.conv.modulation.bias"]),
                  1 / 48 ** 0.5, 1.0, False)
    part = t.put(torch.full(sis_hip.rgb_part_shape(b, cout, h, w), float("nan")), inplace=True)
    y = t.run(sis_hip.modconv2d, t.put(x), wpk, s, ds, 3, t.put(noise), t.put(nw), t.put(bias), fuse_act=True, wino44_u=u44,
              rgb=(t.put(sd["p.conv.weight"]), rgb_s, 1 / cout ** 0.5, part))
    assert sis_hip.lib().sis_last_kernel().decode() == "modconv_wino44_kernel"
    assert torch.equal(y, y0)
    assert bool(torch.isfinite(part).all())
    sd64 = {k: v.double() for k, v in sd.items()}
    with torch.no_grad():
        ref1 = R.to_rgb(sd64, "p", y.double().cpu(), rgb_style.double(), skip.double())
    img1 = t.run(sis_hip.rgb_finish, part, t.put(sd["p.bias"]), t.put(skip), t.put(sd["p.upsample.kernel"]), (2, 1))
    assert _rel(img1, ref1) < 2e-5, _rel(img1, ref1)


def test_prepack_wino44(device, monkeypatch):
    import sis_hip
    import wino44_restatement as W
    t = T(device, monkeypatch)
    cout, cin = 72, 24
    w = _mk(torch.Generator().manual_seed(5), 1, cout, cin, 3, 3)
    u = t.run(sis_hip.modconv_prepack_wino44, t.put(w)).cpu().numpy().astype(np.float64)
    ref = W.weight_planes(w[0].numpy().astype(np.float64))
    err = np.abs(W.unshuffle_u(u) - ref).max()
    assert err == err and err <= 1e-6 * np.abs(ref).max()
