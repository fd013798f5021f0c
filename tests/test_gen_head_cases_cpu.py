"""The cases of gen_head_cases.py on the CPU: every exact-tier case meets its precondition and the restatement of
gen_head_restatement.py reproduces it bit for bit; every bound-tier case's restatement stays within K / 4 (K is 4 x the largest
figure: ``python tests/test_gen_head_cases_cpu.py`` prints the table the constants of gen_head_cases.py are taken from); and the
checks reject simulated defects -- flipped or transposed taps, the skip image's height and width exchanged, a dropped last K
chunk, latent row 0 instead of row i, a bias that misses lr_mul, one element of a 33-row result taken from row 31 -- while the
inputs the suite had before (the symmetric blur, square maps, lr_mul = 1) give identical results with and without them."""
import numpy as np
import pytest
import torch

import exact_operands as X
import gen_head_cases as C
import gen_head_restatement as R


def _el_impl(shape_id, tier, combo, x=None, times_lr=True, drop_tail=False):
    s, op = C.EL_SHAPE[shape_id], C.el_operands(shape_id, tier)
    has_bias, act, lr_mul = combo
    x = op["x"] if x is None else x
    w = op["w"]
    if drop_tail:
        x, w = x[:, :s.k // 64 * 64], w[:, :s.k // 64 * 64]
    fn = R.head_gemm_linear if s.route == C.HG0 else R.equal_linear
    return fn(x.numpy(), w.numpy(), op["bias"].numpy() if has_bias else None, C.el_scale(shape_id, tier, combo), lr_mul, act, times_lr)


def _rgb_impl(case, tier, taps="own", swap=False):
    op = C.rgb_operands(case.shape_id, tier)
    if taps == "own":
        taps = None if case.kind is None else C.taps_of(case.kind, tier)
    if case.kind is None:
        return R.to_rgb(op["x"], op["w"][0, :, :, 0, 0], op["s"], op["bias"].reshape(-1), op["scale"])
    return R.to_rgb(op["x"], op["w"][0, :, :, 0, 0], op["s"], op["bias"].reshape(-1), op["scale"], op["skip"], taps,
                    C.upsample_pad(taps.shape[0])[0], swap)


def _fin_impl(dims, kind, tier):
    op = C.fin_operands(dims, tier)
    if kind is None:
        return R.rgb_finish(op["part"], op["bias"].reshape(-1))
    taps = C.taps_of(kind, tier)
    return R.rgb_finish(op["part"], op["bias"].reshape(-1), op["skip"], taps, C.upsample_pad(kind)[0])


def _mod_results(tier):
    for b, dim in C.MOD_CASES:
        op = C.mod_operands(b, dim, tier)
        for li, (cin, cout, lat, dem) in enumerate(C.LAYERS):
            L = op["layers"][li]
            s = R.head_gemm_linear(op["latent"][:, lat].numpy(), L["mw"].numpy(), L["mb"].numpy(), C.mod_scale(dim, tier), 1.0, False)
            yield C.mod_check(b, dim, tier, li, s)


def _dem_results(tier):
    for b, dim in C.MOD_CASES:
        op = C.mod_operands(b, dim, tier)
        for li, (cin, cout, lat, dem) in enumerate(C.LAYERS):
            if dem is None:
                continue
            L = op["layers"][li]
            wsq = R.prepack_wsq(L["weight"].numpy())
            scale = C.dem_scale(cin, tier)
            yield C.dem_check(b, dim, tier, li, C.HG2, R.head_gemm_demod(L["s_in"], wsq, scale, dem), wsq, device_rsqrt=False)
            yield C.dem_check(b, dim, tier, li, C.DEM, R.demod(L["s_in"], wsq, scale, dem), wsq, device_rsqrt=False)


def exact_results():
    for s in C.EL_SHAPES:
        for combo in C.COMBOS:
            yield C.el_check(s.id, "exact", combo, _el_impl(s.id, "exact", combo))
    yield from _mod_results("exact")
    for case in C.RGB_CASES:
        yield C.rgb_check(case, "exact", _rgb_impl(case, "exact"))
    for dims in C.FIN_SHAPES:
        for kind in C.FIN_KINDS:
            yield C.fin_check(dims, kind, "exact", _fin_impl(dims, kind, "exact"))
    for shape in C.TR_SHAPES:
        w, mean = C.tr_operands(shape, "exact")
        yield C.tr_check(shape, C.TR_PSI_EXACT, "exact", R.truncate(w, mean, C.TR_PSI_EXACT))


def bound_results():
    for s in C.EL_SHAPES:
        combo = C.EL_BOUND_COMBO[s.id]
        yield C.el_check(s.id, "randn", combo, _el_impl(s.id, "randn", combo))
    yield from _mod_results("randn")
    yield from _dem_results("exact")
    yield from _dem_results("randn")
    for case in C.RGB_CASES:
        yield C.rgb_check(case, "randn", _rgb_impl(case, "randn"))
    for dims in C.FIN_SHAPES:
        for kind in C.FIN_KINDS:
            yield C.fin_check(dims, kind, "randn", _fin_impl(dims, kind, "randn"))
    for shape in C.PN_SHAPES:
        for family in C.PN_FAMILIES:
            yield C.pn_check(shape, family, R.pixel_norm(C.pn_input(shape, family)), device_rsqrt=False)
    for shape in C.TR_SHAPES:
        w, mean = C.tr_operands(shape, "randn")
        for psi in C.TR_PSI:
            yield C.tr_check(shape, psi, "randn", R.truncate(w, mean, psi))


def k_table():
    """kernel -> (largest figure of the restatement, the case it came from)."""
    worst = {}
    for r in bound_results():
        if r.figs and r.worst >= worst.get(r.kernel, (-1.0, ""))[0]:
            worst[r.kernel] = (r.worst, r.id)
    return worst


@pytest.fixture(scope="module")
def table():
    return k_table()


def test_exact_tier_preconditions_and_restatement():
    """Every exact-tier case: the operands' and the reference's preconditions hold (asserted inside the builders and
    ``exact_f32``), and one fp32 association -- the restatement's -- gives the reference bit for bit."""
    n = 0
    bad = []
    for r in exact_results():
        n += 1
        bad += r.bad
    assert n > 500 and not bad, "\n".join(bad[:20])


def test_prepack_reference_is_exact():
    for dims in C.PREPACK_SHAPES:
        w = C.prepack_weight(dims)
        wpk, wsq = C.prepack_ref(w)
        assert torch.equal(torch.from_numpy(R.prepack_wsq(w.numpy())), wsq)
        cout, cin, k = dims
        assert wpk[cin - 1, k * k - 1, cout - 1] == w[0, cout - 1, cin - 1, k - 1, k - 1] and tuple(wpk.shape) == (cin, k * k, cout)


def test_restatement_within_a_quarter_of_k(table):
    """K = 4 x the largest figure per kernel (two decimals): the constants of gen_head_cases.py are this table's."""
    assert set(table) == set(C.K)
    for kernel, (fig, case_id) in table.items():
        assert fig <= C.K[kernel] / 4, (kernel, fig, case_id, C.K[kernel])
        assert C.K[kernel] <= 4 * fig + 0.01, (kernel, fig, C.K[kernel])


def test_every_route_has_a_case():
    assert {s.route for s in C.EL_SHAPES} == {C.EL8, C.EL4, C.ELG, C.HG0}
    assert {c.route for c in C.RGB_CASES} == {C.RGB4, C.RGB1}
    for c in C.RGB_CASES:       # the launcher's rule, restated: float4 needs h * w % 4 == 0, h * w >= 256 and aligned pointers
        vec4 = (c.h * c.w) % 4 == 0 and c.h * c.w >= 256 and not c.misaligned
        assert (c.route == C.RGB4) == vec4, c.id
    for kind in (2, 3, 4, 6):
        for tier in ("exact", "randn"):
            t = C.taps_of(kind, tier)
            assert not torch.equal(t, t.flip(0)) and not torch.equal(t, t.t()) and int(torch.linalg.matrix_rank(t.double())) > 1
    rows, (s_total, d_total, mb, db) = C.layout(33)
    assert mb == sum((cin + 127) // 128 for cin, _, _, _ in C.LAYERS) and [l[2] for l in C.LAYERS] != sorted(l[2] for l in C.LAYERS)


# ------------------------------------------------------------------------------------------------------------ simulated defects

def _rejected(result):
    return bool(result.bad)


# (the 2 x 2 map is left out: its one skip pixel meets four taps of a 6 x 6 kernel, and those can agree under a transposition)
SKIP_CASES = [c for c in C.RGB_CASES if c.kind not in (None, "blur") and min(c.h, c.w) >= 4]
NONSQUARE = [c for c in SKIP_CASES if c.h != c.w]
BLUR_SQUARE = [c for c in C.RGB_CASES if c.kind == "blur" and c.h == c.w]


@pytest.mark.parametrize("tier", ["exact", "randn"])
@pytest.mark.parametrize("defect", ["flip_vertical", "transpose"])
def test_wrong_taps_are_rejected(tier, defect):
    change = (lambda t: t.flip(0).contiguous()) if defect == "flip_vertical" else (lambda t: t.t().contiguous())
    for case in SKIP_CASES:
        assert not _rejected(C.rgb_check(case, tier, _rgb_impl(case, tier))), case.id
        assert _rejected(C.rgb_check(case, tier, _rgb_impl(case, tier, taps=change(C.taps_of(case.kind, tier))))), (case.id, defect)
    for case in BLUR_SQUARE:        # the inputs the suite had: the symmetric kernel hides both
        blur = C.taps_of("blur", tier)
        assert np.array_equal(_rgb_impl(case, tier), _rgb_impl(case, tier, taps=change(blur))), case.id
    assert SKIP_CASES and BLUR_SQUARE


@pytest.mark.parametrize("tier", ["exact", "randn"])
def test_swapped_skip_height_and_width_are_rejected(tier):
    assert len(NONSQUARE) >= 8
    for case in NONSQUARE:
        assert _rejected(C.rgb_check(case, tier, _rgb_impl(case, tier, swap=True))), case.id
    for case in [c for c in C.RGB_CASES if c.kind is not None and c.h == c.w]:      # a square map hides it
        assert np.array_equal(_rgb_impl(case, tier), _rgb_impl(case, tier, swap=True)), case.id


@pytest.mark.parametrize("tier", ["exact", "randn"])
def test_dropped_last_chunk_is_rejected(tier):
    tails = [s for s in C.EL_SHAPES if s.k % 64 and s.k > 64]
    assert {s.route for s in tails} == {C.ELG, C.HG0}
    for s in tails:
        combo = C.EL_BOUND_COMBO[s.id]
        assert _rejected(C.el_check(s.id, tier, combo, _el_impl(s.id, tier, combo, drop_tail=True))), s.id


@pytest.mark.parametrize("tier", ["exact", "randn"])
def test_latent_row_0_instead_of_i_is_rejected(tier):
    strided = [s for s in C.EL_SHAPES if s.strided and s.strided[0] != 0]
    assert {s.route for s in strided} == {C.EL8, C.ELG, C.HG0}
    for s in strided:
        combo = C.EL_BOUND_COMBO[s.id]
        row0 = C.el_operands(s.id, tier)["latent"][:, 0]
        assert _rejected(C.el_check(s.id, tier, combo, _el_impl(s.id, tier, combo, x=row0))), s.id
    for b, dim in C.MOD_CASES[:1]:      # the batched modulation reads latent[:, index] too
        op = C.mod_operands(b, dim, tier)
        for li, (cin, cout, lat, dem) in enumerate(C.LAYERS):
            L = op["layers"][li]
            s0 = R.head_gemm_linear(op["latent"][:, 0].numpy(), L["mw"].numpy(), L["mb"].numpy(), C.mod_scale(dim, tier), 1.0, False)
            assert _rejected(C.mod_check(b, dim, tier, li, s0)) == (lat != 0), li


@pytest.mark.parametrize("tier", ["exact", "randn"])
def test_bias_without_lr_mul_is_rejected(tier):
    n = 0
    for s in C.EL_SHAPES:
        for combo in (C.COMBOS if tier == "exact" else [C.EL_BOUND_COMBO[s.id]]):
            has_bias, act, lr_mul = combo
            if not has_bias:
                continue
            got = _el_impl(s.id, tier, combo, times_lr=False)
            if lr_mul == 1.0:       # the inputs the suite had: nothing to see
                assert np.array_equal(got, _el_impl(s.id, tier, combo)), s.id
            else:
                n += 1
                assert _rejected(C.el_check(s.id, tier, combo, got)), (s.id, combo)
    assert n >= 6


@pytest.mark.parametrize("tier", ["exact", "randn"])
def test_an_element_from_row_31_is_rejected(tier):
    rows33 = [s for s in C.EL_SHAPES if s.batch == 33]
    assert rows33
    for s in rows33:
        combo = C.EL_BOUND_COMBO[s.id]
        got = _el_impl(s.id, tier, combo).copy()
        col = s.out - 1
        assert got[32, col] != got[31, col]
        got[32, col] = got[31, col]
        res = C.el_check(s.id, tier, combo, got)
        assert _rejected(res), s.id
        if tier == "exact":
            assert "1 of" in res.bad[0] and f"(32, {col})" in res.bad[0]
        # the bound the suite had -- 1e-5 of the largest element -- is a property of the whole tensor, not of the element
    for b, dim in [c for c in C.MOD_CASES if c[0] == 33][:1]:
        op = C.mod_operands(b, dim, tier)
        L = op["layers"][0]
        s_ = R.head_gemm_linear(op["latent"][:, C.LAYERS[0][2]].numpy(), L["mw"].numpy(), L["mb"].numpy(), C.mod_scale(dim, tier), 1.0, False)
        s_[32, 5] = s_[31, 5]
        assert _rejected(C.mod_check(b, dim, tier, 0, s_))


def test_zero_row_and_no_demodulation_are_exact():
    x = C.pn_input((7, 512), "zero_row")
    got = R.pixel_norm(x)
    assert not C.pn_check((7, 512), "zero_row", got).bad
    got[3, 100] = 1e-30
    assert C.pn_check((7, 512), "zero_row", got).bad
    li = next(i for i, l in enumerate(C.LAYERS) if l[3] == 0)
    cin, cout = C.LAYERS[li][:2]
    for kernel, fn in ((C.HG2, R.head_gemm_demod), (C.DEM, R.demod)):
        L = C.mod_operands(3, 128, "randn")["layers"][li]
        wsq = R.prepack_wsq(L["weight"].numpy())
        assert not C.dem_check(3, 128, "randn", li, kernel, fn(L["s_in"], wsq, C.dem_scale(cin, "randn"), 0), wsq).bad
        assert C.dem_check(3, 128, "randn", li, kernel, fn(L["s_in"], wsq, C.dem_scale(cin, "randn"), 1), wsq).bad


if __name__ == "__main__":
    import math
    for kernel, (fig, case_id) in k_table().items():
        print(f"        {kernel:<29s} K = {math.ceil(400 * fig) / 100:5.2f}   ({fig:.3f}: {case_id})")
