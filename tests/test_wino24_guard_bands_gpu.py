"""Guard-band cases (tests/guard_bands.py) of the Winograd F(2x4,3x3) entries: operands, result and workspace between 0xFF
bands, results born NaN.  Reference and bound as tests/test_wino24_gpu.py (2e-5 * max|ref|; prepack 1e-6)."""
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


@pytest.mark.parametrize("b,cin,cout,h,w", [(2, 16, 64, 8, 64),      # full tiles only
                                             (1, 24, 128, 44, 72)])   # partial tiles in H and in W
def test_modconv2d_wino24(device, monkeypatch, b, cin, cout, h, w):
    import sis_hip
    from oracle import ops_ref
    from oracle import stylegan2_ref as R
    t = T(device, monkeypatch)
    gen = torch.Generator().manual_seed(b * 1000 + cin + cout + h)
    x = _mk(gen, b, cin, h, w)
    style, weight, mod_w, mod_b, wpk, s, ds = _modconv_operands(t, gen, b, cin, cout, 48)
    noise, nw, bias = _mk(gen, 1, 1, h, w), 0.3 * _mk(gen, 1), 0.2 * _mk(gen, cout)
    with torch.no_grad():
        ref = ops_ref.fused_leaky_relu(R.modulated_conv2d(x, style, weight, mod_w, mod_b, demodulate=True) + nw * noise, bias)
    u24 = t.run(sis_hip.modconv_prepack_wino24, t.put(weight))
    y = t.run(sis_hip.modconv2d, t.put(x), wpk, s, ds, 3, t.put(noise), t.put(nw), t.put(bias), fuse_act=True, wino24_u=u24)
    assert sis_hip.lib().sis_last_kernel().decode() == "modconv_wino24_kernel"
    assert _rel(y, ref) < 2e-5, _rel(y, ref)


def test_prepack_wino24(device, monkeypatch):
    import sis_hip
    from test_wino24_cpu import G2, G4
    t = T(device, monkeypatch)
    cout, cin = 72, 24
    w = _mk(torch.Generator().manual_seed(5), 1, cout, cin, 3, 3)
    u = t.run(sis_hip.modconv_prepack_wino24, t.put(w)).cpu().numpy().astype(np.float64)
    ref = np.einsum("ia,ocab,jb->ocij", G2, w[0].numpy().astype(np.float64), G4)
    got = u.transpose(0, 1, 3, 2, 4).reshape(cin, 2, cout, 4, 3).transpose(2, 0, 3, 1, 4).reshape(cout, cin, 4, 6)
    err = np.abs(got - ref).max()
    assert err == err and err <= 1e-6 * np.abs(ref).max()
