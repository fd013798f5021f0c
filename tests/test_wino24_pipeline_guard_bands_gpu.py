"""Guard-band cases (tests/guard_bands.py) of modconv_wino24_kernel with workgroups that walk several tiles: per-sample noise,
operands and result between 0xFF bands, results born NaN.  Reference and bound as tests/test_wino24_gpu.py."""
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


@pytest.mark.parametrize("b,cin,cout,h,w,tpw", [(2, 16, 64, 8, 64, 2),       # full tiles, the next tile is the next sample
                                                 (1, 24, 128, 44, 72, 4)])    # partial tiles in H and in W
def test_modconv2d_wino24_walk(device, monkeypatch, b, cin, cout, h, w, tpw):
    import sis_hip
    from oracle import ops_ref
    from oracle import stylegan2_ref as R
    t = T(device, monkeypatch)
    gen = torch.Generator().manual_seed(b * 1000 + cin + cout + h + tpw)
    x = _mk(gen, b, cin, h, w)
    style, weight, mod_w, mod_b, wpk, s, ds = _modconv_operands(t, gen, b, cin, cout, 48)
    noise, nw, bias = _mk(gen, b, 1, h, w), 0.3 * _mk(gen, 1), 0.2 * _mk(gen, cout)
    with torch.no_grad():
        ref = ops_ref.fused_leaky_relu(R.modulated_conv2d(x, style, weight, mod_w, mod_b, demodulate=True) + nw * noise, bias)
    u24 = t.run(sis_hip.modconv_prepack_wino24, t.put(weight))
    y = t.run(sis_hip.modconv2d, t.put(x), wpk, s, ds, 3, t.put(noise), t.put(nw), t.put(bias), fuse_act=True, wino24_u=u24,
              wino24_tiles_per_wg=tpw)
    assert sis_hip.lib().sis_last_kernel().decode() == "modconv_wino24_kernel"
    assert torch.isfinite(y).all()
    assert _rel(y, ref) < 2e-5, _rel(y, ref)
