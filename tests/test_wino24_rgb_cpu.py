"""Which resolutions of Generator.forward's fast path let the second convolution form the ToRGB channel sum
(Generator._rgb_fused): those where sis_modconv_wino24_eligible takes the convolution, and never the batch-part form of
SIS_RGB_TAIL_SPLIT > 1.  Host code only: no weights are packed and no kernel runs."""
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


@pytest.mark.parametrize("switch", ["SIS_WINO24", "SIS_WINOGRAD"])
def test_not_fused_when_the_kernel_is_switched_off(monkeypatch, switch):
    from networks.stylegan2.model import Generator
    monkeypatch.setenv(switch, "0")
    g = Generator(64, 32, 1, channel_multiplier=2)
    conv, rgb = _resolutions(g)[-1][1:3]
    assert not g._rgb_fused(conv, rgb, 64, 64, torch.zeros(1))


def test_batch_parts_keep_the_separate_to_rgb(monkeypatch):
    g = _generator()
    conv, rgb = _resolutions(g)[-1][1:3]
    x, skip = torch.zeros(8, 1, 1, 1), torch.zeros(1)
    assert g._tail_parts(x, rgb, skip) == 1 and g._rgb_fused(conv, rgb, 64, 64, skip, g._tail_parts(x, rgb, skip))
    monkeypatch.setenv("SIS_RGB_TAIL_SPLIT", "2")
    assert g._tail_parts(x, rgb, skip) == 2 and not g._rgb_fused(conv, rgb, 64, 64, skip, g._tail_parts(x, rgb, skip))
    # no skip image: the unfused launch (ToRGB without upsampling has no finish form)
    assert not g._rgb_fused(conv, rgb, 64, 64, None)
