"""CPU checks of tests/exact_operands.py and of the case lists of the two bit-exact GPU files: the references do not depend on
the summation order, the rounding path of every bf16-output case is exercised (ties included), torch's CPU cast is the bit-level
round-to-nearest-even, and the bitwise comparison rejects defects that the older ``1e-2 * max|ref|`` rule lets through."""
import pytest
import torch
import torch.nn.functional as F

import exact_operands as E
import test_conv_bf16_exact_gpu as conv_cases
import test_gemm_bf16_exact_gpu as gemm_cases


def test_radius_and_integers():
    assert E.radius(8192) == 15 and E.radius(8 * 128 * 128) == 7 and E.radius(64) == 15 and E.radius(2 ** 21) == 1
    gen = torch.Generator().manual_seed(0)
    v = E.integers((4096,), 15, gen)
    assert v.dtype == torch.bfloat16 and float(v.min()) == -15 and float(v.max()) == 15
    assert torch.equal(v.double(), v.double().round())
    s = E.integers((4096,), 15, gen, shift=10)
    assert torch.equal(s.double() * 1024, (s.double() * 1024).round()) and float(s.abs().max()) == 15 / 1024
    assert E.integers((8,), 1024, gen, dtype=torch.float32).dtype == torch.float32
    with pytest.raises(AssertionError):
        E.integers((4096,), 1000, gen)                    # bf16 holds the integers up to 256 only
    with pytest.raises(AssertionError):
        E.check_operands(8192, 64, 64)
    with pytest.raises(AssertionError):
        E.check_reference(torch.tensor([2.0 ** 24], dtype=torch.float64))
    with pytest.raises(AssertionError):
        E.check_reference(torch.tensor([0.5], dtype=torch.float64))
    E.check_reference(torch.tensor([0.5], dtype=torch.float64), unit=2.0 ** -10)


@pytest.mark.parametrize("m,n,k", [(130, 132, 192), (392, 768, 768)])
def test_gemm_reference_does_not_depend_on_the_summation_order(m, n, k):
    """float64, float32 and int64 products of the same integer operands agree bitwise: three arithmetics, three blockings."""
    c = gemm_cases.nt_case(m, n, k)
    ref = E.check_reference(c["y"])
    f32 = c["x"].float() @ c["w"].float().t()
    i64 = c["x"].long() @ c["w"].long().t()
    assert torch.equal(ref.float(), f32) and torch.equal(ref, i64.double())
    halves = c["x"][:, k // 2:].float() @ c["w"][:, k // 2:].float().t() + c["x"][:, :k // 2].float() @ c["w"][:, :k // 2].float().t()
    assert torch.equal(halves, f32)                       # another association (two slabs, added in the other order)


def test_conv_reference_does_not_depend_on_the_summation_order():
    c = conv_cases.forward_case(1, 32, 48, 20, 28, 3, 1, False)
    ref = E.check_reference(c["y"])
    f32 = F.conv2d(c["x"].float(), c["w"].float(), padding=1)
    cols = F.unfold(c["x"].double(), 3, padding=1).long()                   # [1, cin * 9, h * w]
    i64 = (c["w"].long().view(48, -1) @ cols[0]).view(1, 48, 20, 28)
    assert torch.equal(ref.float(), f32) and torch.equal(ref, i64.double())


def test_cpu_cast_is_round_to_nearest_even():
    """``ref.float().bfloat16()`` is the expected output only if torch's CPU cast is RNE: checked on the bits, ties included."""
    gen = torch.Generator().manual_seed(1)
    ints = torch.randint(-2 ** 23, 2 ** 23, (4096,), generator=gen).float()
    up = torch.arange(128, 256).float()                                     # the bf16 values of one binade ...
    ties = torch.cat([(up + 0.5) * 2.0 ** e for e in range(1, 12)])         # ... and the points half way to the next, in 11 binades
    ties = torch.cat([ties, -ties])
    small = torch.randn(2048, generator=gen) * 3
    x = torch.cat([ints, ties, small, torch.tensor([0.0, 1.0, -1.0, 255.5, 256.5, 257.5, 3.0 * 2 ** 20])])
    assert E.tie_share(ties.double()) == 1.0 and E.inexact_share(ties.double()) == 1.0
    assert torch.equal(x.bfloat16(), E.rne_bf16(x))
    assert float(E.rne_bf16(torch.tensor([257.0]))) == 256.0 and float(E.rne_bf16(torch.tensor([259.0]))) == 260.0    # ties go to even
    assert float(E.truncate_bf16(torch.tensor([-259.5]))) == -258.0 and float(E.half_away_bf16(torch.tensor([257.0]))) == 258.0
    assert not torch.equal(x.bfloat16(), E.truncate_bf16(x)) and not torch.equal(x.bfloat16(), E.half_away_bf16(x))


@pytest.mark.parametrize("cases", [gemm_cases, conv_cases], ids=["gemm", "conv"])
def test_rounding_path_is_exercised_by_every_bf16_output_case(cases, capsys):
    """From the references alone: at least a quarter of the outputs need rounding and at least 5 % are exact ties."""
    shares = [(what, E.inexact_share(ref), E.tie_share(ref)) for what, ref in cases.bf16_output_references()]
    assert len(shares) >= 20
    with capsys.disabled():
        print()
        for what, inexact, tie in shares:
            print(f"[exact operands] {what}: inexact {inexact:.3f}, ties {tie:.3f}")
    short = [s for s in shares if s[1] < E.MIN_INEXACT_SHARE or s[2] < E.MIN_TIE_SHARE]
    assert not short, short


def test_fp32_output_references_are_exact():
    """The fp32-output cases: every reference is a sum of integers below 2^24 (``exact_f32`` asserts it while building)."""
    for m, n, k, _ in gemm_cases.TN_CASES + gemm_cases.WGRAD_BIAS_CASES:
        c = gemm_cases.tn_case(m, n, k)
        assert c["dw"].dtype == torch.float32 and c["db"].dtype == torch.float32
    for m, n, k in gemm_cases.NT_CASES + gemm_cases.G256_CASES:
        E.exact_f32(gemm_cases.nt_case(m, n, k)["y_resid"])
    for case in gemm_cases.BATCHED_CASES:
        E.exact_f32(gemm_cases.batched_case(*case)["dw"])
    h = gemm_cases.gelu_case()["h"]
    assert -6 < float(h.min()) < -3 and 3 < float(h.max()) < 6 and 0.9 < float(h.std()) < 1.3


DEFECTS_THE_OLD_RULE_ACCEPTS = ("truncation", "round half away", "bias after rounding", "one element off by 2 ulp")


@pytest.mark.parametrize("m,n,k", gemm_cases.NT_CASES)
def test_bitwise_comparison_rejects_simulated_defects(m, n, k, capsys):
    """Each defect is applied to the reference, not to a kernel.  The bitwise comparison must reject all of them; the older rule
    (max|err| <= 1e-2 max|ref|) accepts the rounding defects, the misplaced bias and the 2-ulp element: what the new tests add."""
    c = gemm_cases.nt_case(m, n, k)
    y, bias = c["y"], c["bias"].double()
    want = E.expected_bf16(y + bias)
    assert E.mismatch_report(want.clone(), want, "the reference itself") is None
    at = (m - 1, n - 3)                                                       # an element of the ragged tile's last row
    bits = want.view(torch.int16).clone()
    bits[at] += 2                                                             # two bf16 ulps away in magnitude
    zeroed = want.clone()
    col = int((want[m - 1] != 0).nonzero()[0])
    zeroed[m - 1, col] = 0
    defects = {
        "truncation": E.truncate_bf16((y + bias).float()),
        "round half away": E.half_away_bf16((y + bias).float()),
        "bias after rounding": (y.float().bfloat16().float() + bias.float()).bfloat16(),
        "last k element dropped": E.expected_bf16(y - c["x"][:, -1:].double() @ c["w"][:, -1:].double().t() + bias),
        "one element off by 2 ulp": bits.view(torch.bfloat16),
        "one element of the last row zeroed": zeroed,
    }
    accepted = {}
    for name, got in defects.items():
        report = E.mismatch_report(got, want, name, tile=(128, 128))
        assert report is not None and "bounding box" in report and "modulo the tile" in report, name
        with pytest.raises(AssertionError):
            E.assert_bitwise(got, want, name)
        accepted[name] = E.old_rule_accepts(got, y + bias)
    with capsys.disabled():
        print(f"\n[exact operands] {(m, n, k)}: the 1e-2 * max|ref| rule accepts " + ", ".join(f"{k_}: {v}" for k_, v in accepted.items()))
    for name in DEFECTS_THE_OLD_RULE_ACCEPTS:
        assert accepted[name], name


def test_mismatch_report_localises_an_edge():
    want = torch.zeros(300, 200)
    got = want.clone()
    got[256:, 130] = 1.0
    report = E.mismatch_report(got, want, "edge", tile=(128, 128))
    assert "44 of 60000 elements differ" in report and "[256, 299] x [130, 130]" in report and "[0, 43] x [2, 2]" in report
    assert "got torch.float32 (2, 2)" in E.mismatch_report(torch.zeros(2, 2), torch.zeros(2, 3), "shape")
    assert E.mismatch_report(torch.zeros(2, 2), torch.zeros(2, 2).bfloat16(), "dtype") is not None
    nan = torch.tensor([float("nan"), 1.0])
    assert E.mismatch_report(nan, torch.tensor([0.0, 1.0]), "nan") is not None
