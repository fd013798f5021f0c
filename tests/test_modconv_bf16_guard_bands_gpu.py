"""Guard-band cases (tests/guard_bands.py) of the bf16 modulated convolution (csrc/modconv_bf16.h): operands, weight image and
result between 0xFF bands, the result born NaN.  No store outside ``out`` (the bands stay 0xFF), and no load from outside
reaches a result (a NaN from a band would break the element-wise bound of tests/modconv_bf16_checks.py)."""
import pytest
import torch

import guard_bands as G
import modconv_bf16_checks as M
from test_guard_bands_gpu import T

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _fresh_session():
    G.reset()
    yield
    G.reset()


@pytest.mark.parametrize("b,cin,cout,h,w", [(2, 16, 64, 8, 64),      # whole tiles only (two 4 x 64 tiles per sample)
                                             (1, 24, 192, 44, 72)])   # partial tiles in H and W, ragged channel tile, half-empty chunk
@pytest.mark.parametrize("fuse", [False, True])
def test_modconv2d_bf16(device, monkeypatch, b, cin, cout, h, w, fuse):
    import sis_hip
    t = T(device, monkeypatch)
    L = M.operands(b, cin, cout, h, w)
    y_ref, bound = M.emulate(L["x"], L["w"], L["s"], L["dscale"])
    if fuse:
        y_ref, bound = M.tail64(y_ref, L["noise"], L["nw"], L["bias"]), M.tail_bound(y_ref, bound, L["noise"], L["nw"], L["bias"])
    packed = t.run(sis_hip.modconv_prepack_bf16, t.put(L["w"].unsqueeze(0)))
    assert packed.dtype == torch.bfloat16 and bool(torch.isfinite(packed.float()).all())      # written in full
    wpk = torch.empty((cin, 9, cout), device=device)       # only its shape is read on this route
    y = t.run(sis_hip.modconv2d, t.put(L["x"]), wpk, t.put(L["s"]), t.put(L["dscale"]), 3, t.put(L["noise"]) if fuse else None,
              t.put(L["nw"]) if fuse else None, t.put(L["bias"]) if fuse else None, fuse_act=fuse, bf16_w=packed)
    assert sis_hip.lib().sis_last_kernel().decode() == "modconv_bf16_kernel"
    share, worst = M.over_bound_share(y.cpu(), y_ref, bound)
    assert share == 0.0, (share, worst)
