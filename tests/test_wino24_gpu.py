"""modconv_wino24_kernel (csrc/modconv_wino24.h, Winograd F(2x4,3x3)) against the oracle, its persistent path, its independence
of the batch, its prepack, and the routing of sis_hip.modconv2d / the generator to it.

Tile classes of the kernel: one-sample tiles of 512 pixels, 8 x 64 (maps wider than 32) or 16 x 32.  A tile never holds more
than one sample and never crosses into the next, so B = 3 / 5 below exercise the walk over samples only.  Per-layer bound:
2e-5 * max|ref|, the project's (tests/test_generator_gpu.py).  Measured on MI355X: 8e-7 .. 2.2e-6 (profiles/wino24_layers.txt)."""
import functools

import pytest
import torch

from oracle import ops_ref
from oracle import stylegan2_ref as R

pytestmark = pytest.mark.gpu

NEW, OLD = "modconv_wino24_kernel", "modconv_wino2_kernel"


def _rel(a, b):
    return (a.double().cpu() - b.double()).abs().max().item() / max(b.abs().max().item(), 1e-30)


@functools.lru_cache(maxsize=None)
def _layer(b, cin, cout, h, w):
    """Operands and oracle results (plain, fused tail) of one layer; computed once, shared, never modified."""
    gen = torch.Generator().manual_seed(b * 1000 + cin + cout + h)
    mk = lambda *s: torch.randn(*s, generator=gen)
    x, style = mk(b, cin, h, w), mk(b, 48)
    weight, mod_w, mod_b = mk(1, cout, cin, 3, 3), mk(cin, 48), 1 + 0.1 * mk(cin)
    noise, nw, bias = mk(1, 1, h, w), 0.3 * mk(1), 0.2 * mk(cout)
    with torch.no_grad():
        ref = R.modulated_conv2d(x, style, weight, mod_w, mod_b, demodulate=True)
        ref_act = ops_ref.fused_leaky_relu(ref + nw * noise, bias)
    return dict(x=x, style=style, weight=weight, mod_w=mod_w, mod_b=mod_b, noise=noise, nw=nw, bias=bias, ref=ref, ref_act=ref_act)


def _run(device, L, fuse, x=None, s=None, ds=None, **kw):
    """sis_hip.modconv2d on the layer's operands with both Winograd packs offered the way the generator offers one of them."""
    import sis_hip
    d = lambda t: t.to(device)
    cin = L["weight"].shape[2]
    with torch.no_grad():
        wpk, wsq = sis_hip.modconv_prepack(d(L["weight"]))
        if s is None:
            s = sis_hip.equal_linear(d(L["style"]), d(L["mod_w"]), d(L["mod_b"]), 1 / 48 ** 0.5, 1.0, False)
            ds = sis_hip.modconv_demod(s, wsq, 1 / (cin * 9) ** 0.5, True)
        y = sis_hip.modconv2d(d(L["x"]) if x is None else x, wpk, s, ds, 3, d(L["noise"]) if fuse else None,
                              d(L["nw"]) if fuse else None, d(L["bias"]) if fuse else None, fuse_act=fuse, **kw)
    torch.cuda.synchronize()
    return y, sis_hip.lib().sis_last_kernel().decode(), (s, ds)


SHAPES = [(2, 8, 64, 8, 64),      # two chunks, a map that is exactly one tile per sample
          (1, 24, 64, 16, 32),    # six chunks, one 16 x 32 tile
          (1, 40, 192, 24, 32),   # ten chunks, three output-channel blocks, partial tile in H only
          (1, 8, 64, 32, 48),     # partial tile in W only (8 x 64 tiles on a 48-wide map)
          (1, 16, 64, 44, 72),    # partial tiles in H and in W
          (3, 16, 128, 32, 32),   # two tiles per sample, three samples, two output-channel blocks
          (5, 8, 64, 8, 64),      # five samples
          (1, 512, 64, 32, 32)]   # one deep contraction: 128 chunks


@pytest.mark.parametrize("fuse", [False, True])
@pytest.mark.parametrize("b,cin,cout,h,w", SHAPES)
def test_kernel_vs_oracle(device, b, cin, cout, h, w, fuse):
    import sis_hip
    L = _layer(b, cin, cout, h, w)
    assert sis_hip.modconv_wino24_eligible(cin, cout, h, w)
    u24 = sis_hip.modconv_prepack_wino24(L["weight"].to(device))
    y, name, _ = _run(device, L, fuse, wino24_u=u24)
    err = _rel(y, L["ref_act"] if fuse else L["ref"])
    print(f"wino24 B{b} {cin}->{cout} {h}x{w} fuse={int(fuse)}: {err:.3e}")
    assert name == NEW
    assert err < 2e-5, err


DECLINED = [(2, 16, 64, 16, 16),   # a map of fewer than 512 pixels
            (2, 16, 32, 32, 32),   # Cout % 64
            (1, 8, 64, 64, 16)]    # no tile class for 16-wide maps


@pytest.mark.parametrize("b,cin,cout,h,w", DECLINED)
def test_declined_shapes_take_the_old_path(device, b, cin, cout, h, w):
    import sis_hip
    L = _layer(b, cin, cout, h, w)
    assert not sis_hip.modconv_wino24_eligible(cin, cout, h, w)
    u24 = sis_hip.modconv_prepack_wino24(L["weight"].to(device))
    u16 = sis_hip.modconv_prepack_wino(L["weight"].to(device))
    y, name, _ = _run(device, L, True, wino24_u=u24, wino_u=u16)
    y0, name0, _ = _run(device, L, True, wino_u=u16)
    assert name == name0 and "wino24" not in name and torch.equal(y, y0)
    assert _rel(y, L["ref_act"]) < 2e-5


def test_persistent_path(device):
    """1, 2 and 4 tiles per workgroup (the launcher's test-only override) on 32 tiles: the same bits."""
    import sis_hip
    L = _layer(4, 16, 64, 64, 64)
    u24 = sis_hip.modconv_prepack_wino24(L["weight"].to(device))
    ys = [_run(device, L, True, wino24_u=u24, wino24_tiles_per_wg=n)[0] for n in (1, 2, 4)]
    assert _rel(ys[0], L["ref_act"]) < 2e-5
    assert torch.equal(ys[0], ys[1]) and torch.equal(ys[0], ys[2])


def test_batch_independence(device):
    """Samples 2:4 of a B = 6 call against a B = 2 call on those samples: the same bits (one-sample tiles, one plan per map).
    The eligibility query has no batch argument, and calls of B = 1, 4, 32, 33 all run the new kernel."""
    import sis_hip
    L = _layer(6, 16, 64, 16, 32)
    u24 = sis_hip.modconv_prepack_wino24(L["weight"].to(device))
    y6, _, (s, ds) = _run(device, L, True, wino24_u=u24)
    y2, name, _ = _run(device, L, True, x=L["x"][2:4].to(device), s=s[2:4].contiguous(), ds=ds[2:4].contiguous(), wino24_u=u24)
    assert name == NEW and torch.equal(y6[2:4], y2)
    assert sis_hip.lib().sis_modconv_wino24_eligible.argtypes == [sis_hip._i] * 4
    for b in (1, 4, 32, 33):
        x = L["x"][:1].to(device).expand(b, -1, -1, -1).contiguous()
        yb, name, _ = _run(device, L, True, x=x, s=s[:1].expand(b, -1).contiguous(), ds=ds[:1].expand(b, -1).contiguous(), wino24_u=u24)
        assert name == NEW and torch.equal(yb[b - 1], y6[0])


def test_prepack(device):
    """u[ci][q][g][co][k] = (G2 g G4^T)[i][3 q + jj] with 3 i + jj = 4 g + k, against float64 on the CPU: 1e-6 relative."""
    import numpy as np
    import sis_hip
    from test_wino24_cpu import G2, G4
    cout, cin = 72, 24
    w = torch.randn(1, cout, cin, 3, 3, generator=torch.Generator().manual_seed(5))
    u = sis_hip.modconv_prepack_wino24(w.to(device)).cpu().numpy().astype(np.float64)
    assert u.shape == (cin, 2, 3, cout, 4)
    ref = np.einsum("ia,ocab,jb->ocij", G2, w[0].numpy().astype(np.float64), G4)          # [co][ci][4][6]
    planes = u.transpose(0, 1, 3, 2, 4).reshape(cin, 2, cout, 4, 3)                           # [ci][q][co][i][jj]
    got = planes.transpose(2, 0, 3, 1, 4).reshape(cout, cin, 4, 6)                            # [co][ci][i][3 q + jj]
    assert np.abs(got - ref).max() <= 1e-6 * np.abs(ref).max()


def test_profiler_record_names_the_kernel(device):
    import sis_hip
    L, Ld = _layer(2, 8, 64, 8, 64), _layer(2, 16, 64, 16, 16)
    rec = []
    sis_hip.set_profiler(rec)
    try:
        for layer in (L, Ld):
            u24 = sis_hip.modconv_prepack_wino24(layer["weight"].to(device))
            u16 = sis_hip.modconv_prepack_wino(layer["weight"].to(device))
            _run(device, layer, True, wino24_u=u24, wino_u=u16)
    finally:
        sis_hip.set_profiler(None)
    convs = [r for r in rec if "modconv_wino" in r[0] and "prepack" not in r[0]]
    assert [r[0] for r in convs] == [NEW, OLD]
    assert convs[0][1] == 0.75 * 2.0 * 2 * 64 * 8 * 9 * 8 * 64       # direct form x 3/4 (see the record site)


def test_generator_switch(device, monkeypatch):
    """Generator(64, 512, 8, 2) at B = 2: SIS_WINO24=0 (F(2x2,3x3) everywhere) and the default agree to 1e-5 * max."""
    import sis_hip
    from networks.stylegan2.model import Generator
    sd = R.seeded_state_dict(64, 512, 8, 2, seed=21)
    z, noise = R.seeded_inputs(64, 2, 512, seed=22)

    def forward():
        g = Generator(64, 512, 8, channel_multiplier=2)
        g.load_state_dict(sd, strict=True)
        g = g.to(device).eval()
        rec = []
        sis_hip.set_profiler(rec)
        try:
            with torch.no_grad():
                img, acts = g([z.to(device)], noise=[n.to(device) for n in noise], return_intermediate_activations=True)
            torch.cuda.synchronize()
        finally:
            sis_hip.set_profiler(None)
        return img, acts, {r[0] for r in rec}

    img, acts, names = forward()
    monkeypatch.setenv("SIS_WINO24", "0")
    img0, acts0, names0 = forward()
    assert NEW in names and NEW not in names0 and OLD in names0
    assert _rel(img, img0.cpu()) < 1e-5
    for k in acts0:
        assert _rel(acts[k], acts0[k].cpu()) < 1e-5, k
