"""The opt-in bf16 route of the generator's stride-1 3x3 layers (csrc/modconv_bf16.h), host side: the entries are declared,
bound and exported; the switch defaults to fp32; the tools parse the flag; and the bound of tests/test_modconv_bf16_gpu.py is
checked from the reference alone -- each of five operand-rounding defects puts more than half of the outputs over it while an
fp32-accumulated convolution of correctly rounded operands stays far under it.  No kernel runs."""
import ctypes
import functools
import os

import pytest
import torch
import torch.nn.functional as F

import exact_operands as E
import modconv_bf16_checks as M

ENTRIES = ("sis_modconv_bf16_eligible", "sis_modconv_bf16_packed_elems", "sis_modconv_prepack_bf16", "sis_modconv2d_bf16")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entries_are_declared_bound_and_exported():
    import sis_hip
    with open(os.path.join(ROOT, "include", "sis_hip.h")) as f:
        header = f.read()
    for name in ENTRIES:
        assert f" {name}(" in header, name
        assert name in sis_hip.exported_symbols(), name
        assert getattr(ctypes.CDLL(sis_hip.LIB_PATH), name) is not None
    assert sis_hip.lib().sis_modconv_bf16_eligible.argtypes == [sis_hip._i] * 4    # no batch argument
    assert sis_hip.lib().sis_modconv_bf16_packed_elems.restype is sis_hip._i64


def test_eligibility_is_by_layer_shape():
    import sis_hip
    ok = sis_hip.modconv_bf16_eligible
    # Generator(256) and Generator(64, 512, 8, 2)
    for cin, cout, hw in [(512, 512, 32), (512, 512, 64), (256, 256, 128), (128, 128, 256)]:
        assert ok(cin, cout, hw, hw), (cin, cout, hw)
    assert ok(8, 64, 8, 32) and ok(40, 192, 24, 40) and ok(24, 128, 44, 72)
    for cin, cout, h, w in [(12, 64, 32, 32), (16, 32, 32, 32), (16, 64, 32, 34), (16, 64, 16, 16), (16, 64, 4, 32), (2048, 64, 32, 32)]:
        assert not ok(cin, cout, h, w), (cin, cout, h, w)
    assert sis_hip.lib().sis_modconv_bf16_packed_elems(512, 512) == 512 * 512 * 9
    assert sis_hip.lib().sis_modconv_bf16_packed_elems(40, 192) == 256 * 48 * 9      # rows to the tile, channels to the chunk
    assert sis_hip.lib().sis_modconv_bf16_packed_elems(16, 64) == 64 * 16 * 9
    assert sis_hip.lib().sis_modconv_bf16_packed_elems(12, 64) == -1


def _conv(g, res):
    r = {8: 0, 16: 1, 32: 2, 64: 3}[res]
    return g.convs[2 * r + 1].conv


def test_switch_defaults_to_fp32(monkeypatch):
    from networks.stylegan2.model import Generator
    monkeypatch.delenv("SIS_GEN_PRECISION", raising=False)
    g = Generator(64, 32, 1, channel_multiplier=2)
    for res in (8, 16, 32, 64):
        c = _conv(g, res)
        assert c.matrix_precision is None and not c._read_switches().bf16 and not c.bf16_takes(res, res)
    assert _conv(g, 64).wino24_takes(64, 64)
    monkeypatch.setenv("SIS_GEN_PRECISION", "fp32")
    assert not _conv(g, 64).bf16_takes(64, 64) and _conv(g, 64).wino24_takes(64, 64)


def test_switch_on_by_environment_and_by_method(monkeypatch):
    from networks.stylegan2.model import Generator
    monkeypatch.setenv("SIS_GEN_PRECISION", "bf16")
    g = Generator(64, 32, 1, channel_multiplier=2)
    assert [_conv(g, res).bf16_takes(res, res) for res in (8, 16, 32, 64)] == [False, False, True, True]
    # where a layer runs bf16 the F(2x4,3x3) kernel does not take it, so its ToRGB is the separate pass
    assert not _conv(g, 64).wino24_takes(64, 64) and not g._rgb_fused(g.convs[7], g.to_rgbs[3], 64, 64, torch.zeros(1))
    # up-convolutions, ToRGB and the mapping network have no bf16 route
    assert not g.convs[6].conv._read_switches().bf16 and not g.to_rgbs[3].conv._read_switches().bf16
    assert g.set_matrix_precision("fp32") is g
    assert not _conv(g, 64).bf16_takes(64, 64) and _conv(g, 64).wino24_takes(64, 64)
    monkeypatch.delenv("SIS_GEN_PRECISION")
    g.set_matrix_precision("bf16")
    assert _conv(g, 32).bf16_takes(32, 32) and all(m._pack_key is None for m in g.modules() if hasattr(m, "_pack_key"))
    g.set_matrix_precision(None)
    assert not _conv(g, 32).bf16_takes(32, 32)
    with pytest.raises(ValueError):
        g.set_matrix_precision("fp16")
    monkeypatch.setenv("SIS_GEN_PRECISION", "half")
    with pytest.raises(ValueError):
        _conv(g, 32).bf16_takes(32, 32)


def test_cli_flag_parses():
    import create_dataset_for_segmentation as D
    import create_semantic_segmentation as S
    for mod in (D, S):
        assert mod.build_parser().parse_args([]).generator_precision == "fp32"
        assert mod.build_parser().parse_args(["--generator-precision", "bf16"]).generator_precision == "bf16"
        with pytest.raises(SystemExit):
            mod.build_parser().parse_args(["--generator-precision", "fp16"])


def test_cli_flag_sets_the_switch_and_names_the_mode(capsys):
    import argparse
    import create_dataset_for_segmentation as D
    from networks.stylegan2.model import Generator
    g = Generator(64, 32, 1, channel_multiplier=2)
    D.apply_generator_precision(g, argparse.Namespace(generator_precision="bf16"))
    assert _conv(g, 64).bf16_takes(64, 64) and "generator precision: bf16" in capsys.readouterr().out
    D.apply_generator_precision(g, argparse.Namespace(generator_precision="fp32"))
    assert not _conv(g, 64).bf16_takes(64, 64) and "generator precision: fp32" in capsys.readouterr().out
    D.apply_generator_precision(g, argparse.Namespace())            # callers without the flag
    assert capsys.readouterr().out == ""


def test_emulation_rounding_is_torchs_cpu_cast():
    gen = torch.Generator().manual_seed(3)
    x = torch.cat([torch.randn(1 << 16, generator=gen) * 10.0 ** torch.randint(-6, 7, (1 << 16,), generator=gen),
                   torch.tensor([0.0, -0.0, 1.0, 1.00390625, 1.01171875, -1.00390625, 3.0e38, 1e-30])])   # ties to even on both sides
    assert torch.equal(M.rne(x), x.bfloat16().float())
    assert not torch.equal(M.truncate(x), x.bfloat16().float())


# ---- the bound, from the reference alone (small K only: at K = 4608 the worst-case bound no longer separates the defects)

SMALL_K = [(2, 16, 64, 32, 32), (1, 40, 192, 24, 40)]


@functools.lru_cache(maxsize=None)
def _case(shape):
    L = M.operands(*shape)
    y, bound = M.emulate(L["x"], L["w"], L["s"], L["dscale"])
    return L, y, bound


@pytest.mark.parametrize("shape", SMALL_K)
def test_correct_form_is_far_under_the_bound(shape):
    """F.conv2d accumulating in fp32 on correctly rounded operands, fp32 dscale: at most 0.02 of the bound."""
    L, y, bound = _case(shape)
    got = F.conv2d(M.rne(M.modulated(L["x"], L["s"])), M.rne(L["w"]), padding=1) * L["dscale"].view(*L["dscale"].shape, 1, 1)
    share, worst = M.over_bound_share(got, y, bound)
    print(f"correct form {shape}: worst error / bound = {worst:.4f}")
    assert share == 0.0 and worst <= 0.02, (share, worst)
    # ... and through the fused tail
    ref = M.tail64(y, L["noise"], L["nw"], L["bias"])
    v = got + L["nw"] * L["noise"] + L["bias"].view(1, -1, 1, 1)
    got_t = torch.maximum(v, v * 0.2) * M.SQRT2_F32
    share, worst = M.over_bound_share(got_t, ref, M.tail_bound(y, bound, L["noise"], L["nw"], L["bias"]))
    assert share == 0.0 and worst <= 0.02, (share, worst)


@pytest.mark.parametrize("defect", M.DEFECTS)
@pytest.mark.parametrize("shape", SMALL_K)
def test_bound_sees_the_defect(shape, defect):
    L, y, bound = _case(shape)
    x_op, w_op = M.defective(defect, L)
    bad, _ = M.emulate(L["x"], L["w"], L["s"], L["dscale"], x_op=x_op, w_op=w_op)
    share, worst = M.over_bound_share(bad, y, bound)
    print(f"{defect} {shape}: {100 * share:.1f} % of the outputs over the bound, worst {worst:.1f} x")
    assert share > 0.5, share
    # the fused tail keeps them apart as well
    ref_t = M.tail64(y, L["noise"], L["nw"], L["bias"])
    share_t, _ = M.over_bound_share(M.tail64(bad, L["noise"], L["nw"], L["bias"]), ref_t, M.tail_bound(y, bound, L["noise"], L["nw"], L["bias"]))
    assert share_t > 0.5, share_t
