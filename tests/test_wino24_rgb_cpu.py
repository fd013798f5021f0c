"""Which resolutions of Generator.forward's fast path let the second convolution form the ToRGB channel sum
(Generator._rgb_fused): those where sis_modconv_wino24_eligible takes the convolution and a skip image exists; and which
route (ModulatedConv2d.route) every layer of a generator takes in every switch position.  Host code only: no kernel runs, and
where weights are packed the pack functions are stubs."""
import functools

import pytest
import torch


@functools.lru_cache(maxsize=None)
def _generator():
    from networks.stylegan2.model import Generator
    return Generator(64, 32, 1, channel_multiplier=2)   # 4^2 .. 64^2: 512 channels everywhere


def _resolutions(g):
    return [(4 << (r + 1), g.convs[2 * r + 1], g.to_rgbs[r]) for r in range(g.log_size - 2)]


def test_binding_declares_the_entries():
    import sis_hip
    assert {"sis_modconv2d_wino24_rgb", "sis_rgb_finish"} <= set(sis_hip.exported_symbols())
    assert sis_hip.rgb_part_shape(5, 192, 8, 64) == (3, 5, 3, 8, 64)


def test_fused_only_where_the_kernel_takes_the_convolution(monkeypatch):
    import sis_hip
    g = _generator()
    skip = torch.zeros(1)
    asked = []
    real = sis_hip.modconv_wino24_eligible
    monkeypatch.setattr(sis_hip, "modconv_wino24_eligible", lambda *a: asked.append(a) or real(*a))
    fused = {}
    for res, conv, rgb in _resolutions(g):
        c = conv.conv
        fused[res] = g._rgb_fused(conv, rgb, res, res, skip)
        assert fused[res] == bool(real(c.in_channel, c.out_channel, res, res)), res
    assert fused == {8: False, 16: False, 32: True, 64: True} and asked[-1] == (512, 512, 64, 64)
    # the kernel's own answer decides: a map it declines, and a kernel that declines everything
    conv, rgb = _resolutions(g)[-1][1:3]
    assert not real(512, 512, 16, 16) and not g._rgb_fused(conv, rgb, 16, 16, skip)
    monkeypatch.setattr(sis_hip, "modconv_wino24_eligible", lambda *a: False)
    assert not g._rgb_fused(conv, rgb, 64, 64, skip)
    monkeypatch.setattr(sis_hip, "modconv_wino24_eligible", real)
    # no skip image: the unfused launch (ToRGB without upsampling has no finish form)
    assert g._rgb_fused(conv, rgb, 64, 64, skip) and not g._rgb_fused(conv, rgb, 64, 64, None)


@pytest.mark.parametrize("switch", ["SIS_WINO24", "SIS_WINOGRAD"])
def test_not_fused_when_the_kernel_is_switched_off(monkeypatch, switch):
    from networks.stylegan2.model import Generator
    monkeypatch.setenv(switch, "0")
    g = Generator(64, 32, 1, channel_multiplier=2)
    conv, rgb = _resolutions(g)[-1][1:3]
    assert not g._rgb_fused(conv, rgb, 64, 64, torch.zeros(1))


# ---- one route per layer: Generator(64, 512, 8, 2), the stride-1 3x3 layers at their own maps (4^2 .. 64^2)

POSITIONS = {   # position: (environment, set_matrix_precision, routes)
    "default": ({}, None, ["wino", "wino", "wino", "wino24", "wino24"]),
    "SIS_WINO24=0": ({"SIS_WINO24": "0"}, None, ["wino"] * 5),
    "SIS_WINOGRAD=0": ({"SIS_WINOGRAD": "0"}, None, ["direct"] * 5),
    "bf16": ({}, "bf16", ["wino", "wino", "wino", "bf16", "bf16"]),
    "bf16, SIS_WINOGRAD=0": ({"SIS_WINOGRAD": "0"}, "bf16", ["direct", "direct", "direct", "bf16", "bf16"]),
}


@pytest.mark.parametrize("position", POSITIONS)
def test_route_of_every_layer(monkeypatch, position):
    import sis_hip
    from networks.stylegan2.model import ROUTES, Generator, ToRGB
    env, precision, want = POSITIONS[position]
    for name in ("SIS_WINOGRAD", "SIS_WINO24", "SIS_GEN_PRECISION"):
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    packed = []
    monkeypatch.setattr(sis_hip, "modconv_prepack", lambda w: (w, w))
    for pack in ("modconv_prepack_bf16", "modconv_prepack_wino24", "modconv_prepack_wino", "modconv_prepack_up_fir"):
        monkeypatch.setattr(sis_hip, pack, lambda w, pack=pack: packed.append(pack) or w)
    g = Generator(64, 512, 8, channel_multiplier=2)
    if precision is not None:
        g.set_matrix_precision(precision)
    assert ROUTES == ("bf16", "wino44", "wino24", "wino", "direct")
    res, skip, routes, images = 4, None, [], {}
    for layer, _ in g._layer_sequence():
        conv = layer.conv
        if conv.upsample:
            res *= 2
            assert conv.fir_weights() is not None
            images[layer] = {"up_fir"}
            continue
        route = conv.route(res, res)
        assert route in ROUTES and conv.bf16_takes(res, res) == (route == "bf16") and conv.wino24_takes(res, res) == (route == "wino24")
        conv.operand(route)
        images[layer] = {route} - {"direct"}
        if isinstance(layer, ToRGB):
            assert route == "direct", res
            assert g._rgb_fused(before, layer, res, res, skip) == (routes[-1] == "wino24" and skip is not None), res
            assert not g._rgb_fused(before, layer, res, res, None)
            skip = torch.zeros(1)
        else:
            routes.append(route)
            before = layer
    assert routes == want
    # one route + operand request per layer: one image per stride-1 layer (none for "direct"), the fast-FIR planes on the
    # up-convolutions (all of this generator's qualify), and none on a ToRGB
    assert {layer: set(layer.conv._images) for layer in images} == images
    assert len(packed) == sum(len(v) for v in images.values())
