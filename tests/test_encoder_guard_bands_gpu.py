"""Guard-band cases (tests/guard_bands.py) of the projection encoders' kernels at their remainder shapes: operands, results
and workspaces between 0xFF bands, results born NaN.  References and bound as tests/test_encoder_gpu.py (2e-5 * max|ref|)."""
import pytest
import torch

import encoder_checks as C
import guard_bands as G
from test_guard_bands_gpu import T, _mk, _rel

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _fresh_session():
    G.reset()
    yield
    G.reset()


def _fold(gen, c):
    return 0.5 + torch.rand(c, generator=gen), 0.3 * torch.randn(c, generator=gen)


@pytest.mark.parametrize("b,cin,cout,h,w", [(1, 16, 24, 12, 20),    # partial channel tile, partial pixel tile
                                             (3, 40, 72, 36, 36)])   # several chunks and tiles, the last ones partial
@pytest.mark.parametrize("shortcut", [True, False])
def test_conv3x3_s2(device, monkeypatch, b, cin, cout, h, w, shortcut):
    import sis_hip
    t = T(device, monkeypatch)
    gen = torch.Generator().manual_seed(b * 1000 + cin + cout + h)
    x, w1, wd = _mk(gen, b, cin, h, w), _mk(gen, cout, cin, 3, 3) / (3 * cin ** 0.5), _mk(gen, cout, cin, 1, 1) / cin ** 0.5
    f1, fd = _fold(gen, cout), _fold(gen, cout)
    ref_main, ref_short = C.ref_conv3x3_s2(x, w1, *f1, wd, *fd)
    packed = t.run(sis_hip.enc_conv3x3_s2_pack, t.put(w1), t.put(wd) if shortcut else None)
    extra = (t.put(fd[0]), t.put(fd[1])) if shortcut else ()
    y, ys = t.run(sis_hip.enc_conv3x3_s2, t.put(x), packed, cout, t.put(f1[0]), t.put(f1[1]), *extra)
    assert _rel(y, ref_main) < 2e-5, _rel(y, ref_main)
    if shortcut:
        assert _rel(ys, ref_short) < 2e-5, _rel(ys, ref_short)


@pytest.mark.parametrize("cin,h,w", [(1, 8, 12), (3, 17, 23)])   # fewer pixels than a workgroup; odd sizes, a partial workgroup
def test_stem(device, monkeypatch, cin, h, w):
    import sis_hip
    t = T(device, monkeypatch)
    b, cout = 2, 40
    gen = torch.Generator().manual_seed(cin + h)
    x, w1, wd, bd = _mk(gen, b, cin, h, w), _mk(gen, cout, cin, 3, 3) / 3, _mk(gen, cout, cin, 1, 1), _mk(gen, cout)
    f1, fd = _fold(gen, cout), _fold(gen, cout)
    ref_main, ref_short = C.ref_stem(x, w1, *f1, wd, bd, *fd)
    y, ys = t.run(sis_hip.enc_stem, t.put(x), t.put(w1), t.put(f1[0]), t.put(f1[1]), t.put(wd), t.put(bd), t.put(fd[0]), t.put(fd[1]))
    assert _rel(y, ref_main) < 2e-5 and _rel(ys, ref_short) < 2e-5


@pytest.mark.parametrize("b,ch,h,w", [(3, 8, 4, 4), (3, 40, 12, 20), (1, 6, 20, 20), (2, 72, 36, 36)])
def test_block_tail(device, monkeypatch, b, ch, h, w):
    import sis_hip
    t = T(device, monkeypatch)
    gen = torch.Generator().manual_seed(b + ch + h)
    c, res, (scale, shift) = _mk(gen, b, ch, h, w), _mk(gen, b, ch, h, w), _fold(gen, ch)
    nw, nb = _mk(gen, 1, ch, 1, 1), _mk(gen, 1)
    ref_y, ref_noise, ref_pool = C.ref_block_tail(c, res, scale, shift, nw, nb)
    y, nz, partial = t.run(sis_hip.enc_block_tail, t.put(c), t.put(res), t.put(scale), t.put(shift), t.put(nw), t.put(nb), want_pool=True)
    assert _rel(y, ref_y) < 2e-5 and _rel(nz, ref_noise) < 2e-5 and _rel(partial.sum(dim=2) / (h * w), ref_pool) < 2e-5


@pytest.mark.parametrize("sum_heads", [False, True])
def test_latent_heads(device, monkeypatch, sum_heads):
    import sis_hip
    t = T(device, monkeypatch)
    batch, latent, channels, hws = 3, 48, [8, 24, 40, 264], [12, 292, 572, 16]
    gen = torch.Generator().manual_seed(11)
    partials = [_mk(gen, batch, c, sis_hip.enc_block_tail_tiles(hw)) for c, hw in zip(channels, hws)]
    weights, biases = [_mk(gen, latent, c, 1, 1) / c ** 0.5 for c in channels], [_mk(gen, latent) for _ in channels]
    ref = C.ref_latent_heads([p.double().sum(dim=2) / hw for p, hw in zip(partials, hws)], weights, biases)
    rows = [(t.put(p), hw, t.put(w), t.put(bb), i) for i, (p, hw, w, bb) in enumerate(zip(partials, hws, weights, biases))]
    table = sis_hip.enc_heads_table(rows, device)
    table.table = t.put(table.table.cpu())
    out = t.run(sis_hip.enc_latent_heads, table, sum_heads=sum_heads)
    want = torch.stack(ref, dim=1).sum(dim=1) if sum_heads else torch.stack(ref, dim=1)
    assert _rel(out, want) < 2e-5, _rel(out, want)
