"""Winograd F(4x4,3x3) as csrc/modconv_wino44.h uses it (tests/wino44_restatement.py): the matrices against a direct correlation, the
fp32 error of the kernel's sum order as a regression pin on them, and the route of every layer.  Host code only."""
import functools

import numpy as np
import pytest
import torch

import wino44_restatement as W

BOUND = 2e-5   # the project's per-layer bound, as a fraction of max|ref| (tests/test_generator_gpu.py)


def test_matrices_reproduce_a_direct_correlation():
    """A wrong interpolation point or sign shows as an error of order 1; float64 rounding stays under 1e-12."""
    rng = np.random.default_rng(3)
    d, g = rng.standard_normal((64, 6, 6)), rng.standard_normal((64, 3, 3))
    got = W.output_tile(W.weight_planes(g) * W.data_planes(d))
    ref = W.direct_tile(d, g)
    assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()


def test_plane_order_is_a_permutation():
    assert sorted(W.plane(i, jj) for i in range(6) for jj in range(3)) == list(range(18))
    u = np.arange(2 * 9 * 5 * 4, dtype=np.float64).reshape(2, 9, 5, 4)
    assert sorted(W.unshuffle_u(u).ravel()) == sorted(u.ravel())


@functools.lru_cache(maxsize=None)
def _emulated(seed, cin):
    """Leaky-ReLU-shaped inputs, style factors 1 +- 0.5, 64 tiles x 32 output channels; (fp32 emulation, float64 reference)."""
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((64, cin, 6, 6))
    d = np.where(d > 0, d, 0.2 * d) * np.sqrt(2)
    g = rng.standard_normal((32, cin, 3, 3))
    s = 1 + rng.uniform(-0.5, 0.5, cin)
    d32, g32, s32 = d.astype(np.float32), g.astype(np.float32), s.astype(np.float32)
    ref = np.zeros((64, 32, 4, 4))
    ds = d32.astype(np.float64) * s32.astype(np.float64)[None, :, None, None]
    for a in range(3):
        for b in range(3):
            ref += np.einsum("oc,tcrx->torx", g32[:, :, a, b].astype(np.float64), ds[:, :, a:a + 4, b:b + 4])
    return W.emulate_fp32(d32, g32, s32), W.emulate_fp32(d32, g32, s32, fma_chain=True), ref


@pytest.mark.parametrize("seed", [0, 1])
def test_fp32_emulation_stays_under_half_the_bound_at_512_channels(seed):
    """Accumulation in chunks of 4 (one accumulator rounding per chunk): 8.4e-6 / 8.5e-6 of max|ref|, under half the bound.  With one
    FMA per channel, the documented equivalent of the MFMA step, the same data give 1.22e-5 / 1.26e-5: inside the bound, not
    inside half of it -- which is what the device measures on the 512-channel layers (profiles/wino44_layers.txt) and why those
    stay on F(2x4,3x3)."""
    chunked, chain, ref = _emulated(seed, 512)
    err = np.abs(chunked.astype(np.float64) - ref).max() / np.abs(ref).max()
    err_chain = np.abs(chain.astype(np.float64) - ref).max() / np.abs(ref).max()
    print(f"F(4x4,3x3) fp32 emulation, Cin = 512, seed {seed}: chunks of 4 {err:.3e}, FMA chain {err_chain:.3e} of max|ref|")
    assert err < 0.5 * BOUND, err
    assert err_chain < BOUND, err_chain


# ---- routes

def _routes(size, monkeypatch, env):
    from networks.stylegan2.model import Generator
    for name in ("SIS_WINOGRAD", "SIS_WINO24", "SIS_WINO44", "SIS_GEN_PRECISION"):
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    g = Generator(size, 32, 1, channel_multiplier=2)
    layers = [g.conv1] + [g.convs[2 * r + 1] for r in range(g.log_size - 2)]
    return [(layer.conv.in_channel, layer.conv.out_channel, 4 << i, layer.conv.route(4 << i, 4 << i)) for i, layer in enumerate(layers)]


@pytest.mark.parametrize("size", [256, 64])
def test_route_names_wino44_exactly_on_the_ship_list(monkeypatch, size):
    import sis_hip
    from networks.stylegan2.model import ROUTES, WINO44_LAYERS
    assert "wino44" in ROUTES and ROUTES.index("wino44") < ROUTES.index("wino24")
    routes = _routes(size, monkeypatch, {})
    for cin, cout, res, route in routes:
        assert (route == "wino44") == ((cin, cout, res, res) in WINO44_LAYERS), (cin, cout, res, route)
    for cin, cout, h, w in WINO44_LAYERS:
        assert sis_hip.modconv_wino44_eligible(cin, cout, h, w)
    if size == 256:
        assert {r[:3] for r in routes if r[3] == "wino44"} == {l[:3] for l in WINO44_LAYERS}


@pytest.mark.parametrize("size", [256, 64])
def test_switch_restores_the_previous_routes(monkeypatch, size):
    """SIS_WINO44=0: the routes of a tree without the F(4x4,3x3) kernel -- F(2x4,3x3) from 32^2 up, F(2x2,3x3) below."""
    routes = _routes(size, monkeypatch, {"SIS_WINO44": "0"})
    assert [r[3] for r in routes] == ["wino" if r[2] < 32 else "wino24" for r in routes]
    assert [r[3] for r in _routes(size, monkeypatch, {"SIS_WINO24": "0"})] == ["wino"] * len(routes)
    assert [r[3] for r in _routes(size, monkeypatch, {"SIS_WINOGRAD": "0"})] == ["direct"] * len(routes)


def test_rgb_fusion_accepts_both_winograd_routes(monkeypatch):
    from networks.stylegan2.model import Generator
    for name in ("SIS_WINOGRAD", "SIS_WINO24", "SIS_WINO44", "SIS_GEN_PRECISION"):
        monkeypatch.delenv(name, raising=False)
    g = Generator(64, 32, 1, channel_multiplier=2)
    conv, rgb, skip = g.convs[-1], g.to_rgbs[-1], torch.zeros(1)
    assert g._rgb_fused(conv, rgb, 64, 64, skip, route="wino44") and g._rgb_fused(conv, rgb, 64, 64, skip, route="wino24")
    assert not g._rgb_fused(conv, rgb, 64, 64, skip, route="wino") and not g._rgb_fused(conv, rgb, 64, 64, None, route="wino44")


def test_eligibility_rule():
    import sis_hip
    ok = sis_hip.modconv_wino44_eligible
    assert ok(8, 64, 16, 32) and ok(8, 64, 8, 64) and ok(8, 64, 12, 64) and ok(128, 128, 256, 256)
    assert not ok(12, 64, 16, 32)    # Cin % 8
    assert not ok(8, 32, 16, 32)     # Cout % 64
    assert not ok(8, 64, 18, 32)     # H % 4
    assert not ok(8, 64, 16, 34)     # W % 4
    assert not ok(8, 64, 64, 16)     # W <= 16
    assert not ok(8, 64, 16, 16)     # fewer than 512 pixels
    assert {"sis_modconv2d_wino44", "sis_modconv2d_wino44_rgb", "sis_modconv_prepack_wino44",
            "sis_modconv_wino44_eligible"} <= set(sis_hip.exported_symbols())
    assert {"modconv_wino44_kernel", "wino44_prepack_kernel"} <= sis_hip.own_kernel_names()
