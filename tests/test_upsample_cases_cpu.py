"""The fp32 restatement of the bilinear-upsampling kernels (upsample_restatement.py) against the float64 references and bounds of
upsample_cases.py, and the index facts the x2 kernels rest on:
(1) the float64 reference agrees with torch's float64 ``F.interpolate(align_corners=True)`` up to the float32 index step;
(2) on every case the restatement stays within the bounds -- this is where the K of each kernel is measured
    (``python tests/test_upsample_cases_cpu.py`` prints the figures; K = 4 x the largest) -- and passes the exact checks;
(3) each named mistake of the restatement exceeds a bound by at least 10 x on the case and region named in FAULTS, i.e. the GPU
    test, which holds the kernels to the same bounds, would notice it;
(4) exhaustively for every size 2..4096: the direct forward's static indices ARE the float32 rule's, every output with weight
    on cell j lies in 2j - 1 .. 2j + 2 (the direct backward's window) and so in 2j - 3 .. 2j + 2 (the tiled backward's), and the
    tiled forward's source tile fits its LDS array.

Where a fault cannot be made to fail by a value test, the tests below assert exactly that:
  i1_not_clamped        src = fl(fl((in - 1) / (out - 1)) (out - 1)) at the last output is exactly in - 1 at every shape here but 138 -> 274
                        (and at every x2 size up to 4096): l1 = 0 there, what lies behind the row is multiplied by 0 and the
                        generic and tiled forward return the same bits without the clamp.  It IS caught at 138 -> 274 (l1 = 1.5e-5
                        there) and on the direct forward, whose fused lambda at the last output is up to ulp(w - 1) / 2, not 0.
  clamped_edge_l0_only  likewise: the l1 it drops is 0 wherever the last source coordinate is exactly in - 1; caught at 138 -> 274.
  window_short_lo       on the tiled backward: its window 2j - 3 .. 2j + 2 has two candidates to spare at the first end (every
                        contributor lies in 2j - 1 .. 2j + 2), so one short is still complete.  Caught on the other two kernels.
  lerp_lambda_fused     moves values by 1e-8: inside the bound wherever the rule's weight is not exactly 0.  It is caught by the
                        exact-zero footprint assertion (test_fused_lambda_breaks_the_footprint).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import upsample_cases as U
import upsample_restatement as R
from loss_cases import lerp_tables


def restate(case, inp, fault=None):
    if case.strided:
        rng = np.random.default_rng(7)
        B, C, h, w = case.shape
        wide = U.round_to(rng.standard_normal((B, C + case.extra, 2 * h, 2 * w)), case.dtype)
        gwide = wide.copy()
        gwide[:, :C] = inp["gy"]
        y = R.into_wide(wide, inp["x"], case.fwd, case.dtype, fault)
        return dict(y=y[:, :C], gx=R.grad_from_wide(gwide, C, case.bwd, case.dtype, fault), wide=wide, y_wide=y)
    return dict(y=R.forward(inp["x"], case.size, case.fwd, case.dtype, fault),
                gx=R.backward(inp["gy"], case.shape[2:], case.bwd, case.dtype, fault))


# ------------------------------------------------------------------------------------------------------------ the reference

@pytest.mark.parametrize("sid", list(U.SHAPES))
def test_reference_against_torch(sid):
    """ref == F.interpolate(float64, align_corners=True) and its autograd to 4e-6 of the data's scale: torch's float64 kernel
    takes the source index in float64, the operator in float32, which moves every lambda by up to ~(in - 1) 2^-24."""
    case = U.CASE[f"{sid}-f32-noise"]
    inp = U.build(case)
    xt = torch.from_numpy(inp["x"]).double().requires_grad_(True)
    ref = F.interpolate(xt, size=case.size, mode="bilinear", align_corners=True)
    (gref,) = torch.autograd.grad(ref, xt, torch.from_numpy(inp["gy"]).double())
    n = max(case.shape[2:]) * 2.0 ** -24
    assert np.abs(inp["y"] - ref.detach().numpy()).max() <= 8 * n * np.abs(inp["x"]).max()
    assert np.abs(inp["gx"] - gref.numpy()).max() <= 8 * n * np.abs(gref.numpy()).max() + 1e-12


def test_ramps_are_the_source_coordinate():
    """A ramp's float64 reference IS the float32 source coordinate up to the rounding of l0 (``ramp_slack``), on both axes of every
    shape: holding a kernel to the reference on a ramp pins its coordinates."""
    for sid in U.SHAPES:
        for d in ("ramp_i", "ramp_j"):
            inp = U.build(U.CASE[f"{sid}-f32-{d}"])
            src = inp["src_y"][:, None] if d == "ramp_i" else inp["src_x"][None, :]
            assert (np.abs(inp["y"] - src.astype(np.float64)[None, None]) <= U.ramp_slack(src)[None, None]).all(), (sid, d)


# ------------------------------------------------------------------------------------------------------------ within the bounds

GROUPS = {}
for _c in U.CASES + U.STRIDED_CASES:
    GROUPS.setdefault((_c.shape_id, _c.dtype), []).append(_c)


def figures(cases):
    """kernel -> (largest figure, key, case id); and the failures of the exact checks and identities."""
    worst, bad = {}, []
    for case in cases:
        inp = U.build(case)
        out = restate(case, inp)
        for k, v in U.figures(case, inp, out["y"], out["gx"]).items():
            kern = U.kernel_of(case, k)
            if v > worst.get(kern, (-1.0,))[0]:
                worst[kern] = (v, k, case.id)
        bad += U.exact_checks(case, inp, out["y"], out["gx"])
        if not case.data.startswith("hot"):
            bad += U.identity_checks(case, inp, out["y"], out["gx"])
        if case.strided:
            C = case.shape[1]
            assert np.array_equal(out["y_wide"][:, C:], out["wide"][:, C:])
    return worst, bad


@pytest.mark.parametrize("key", list(GROUPS), ids=["-".join(k) for k in GROUPS])
def test_restatement_within_bounds(key):
    """Every case, every region: within the bound at its kernel's K and at least a factor 2 inside it (K is 4 x the largest
    figure); footprints exactly zero, the constant within 2 ulp, the ramps on their coordinate, both identities."""
    worst, bad = figures(GROUPS[key])
    print(key, {k: (round(v[0], 3), v[1], v[2]) for k, v in worst.items()})
    assert not bad, "; ".join(bad)
    for kern, (v, k, cid) in worst.items():
        assert v <= U.K[kern] / 2, f"{cid}: {k} needs K = {v:.3g}, the K of {kern} is {U.K[kern]}"


def test_cases_cover_every_kernel_in_every_dtype():
    for dt in U.DTYPES:
        assert {c.fwd for c in U.CASES if c.dtype == dt} == {U.GEN_F, U.TIL_F, U.DIR_F}
        assert {c.bwd for c in U.CASES if c.dtype == dt} == {U.GEN_B, U.TIL_B, U.DIR_B}
        assert {(c.fwd, c.bwd) for c in U.STRIDED_CASES if c.dtype == dt} == {(U.DIR_F, U.DIR_B), (U.TIL_F, U.TIL_B)}
    # the impulses the issue names are there
    cells, outs = U.impulses("direct_2x512")
    assert {j for _, j in cells} >= {0, 255, 256, 511} and {X for _, X in outs} >= {0, 511, 512, 1023}
    assert 3 in U.leak_outputs(3, 7) and 5 in U.leak_outputs(3, 11)   # (and the last output, whose two weights share a cell)
    assert 3 in {Y for Y, _ in U.impulses("gen_3_7_11")[1]} and 5 in {X for _, X in U.impulses("gen_3_7_11")[1]}
    assert all(U.leak_outputs(2, n)[-1:] == [n - 1] for n in (26, 32))


# ------------------------------------------------------------------------------------------------------------ faults

# (fault, the case that shows it, the figure that shows it)
FAULTS = [
    ("scale_in_over_out", "gen_12_27-f32-noise", "y/all"),
    ("scale_in_over_out", "gen_12_27-f32-noise", "gx/all"),
    ("scale_in_over_out", "direct_3x16-f32-ramp_j", "gx/last_col"),
    ("i1_not_clamped", "gen_138_274-f32-noise", "y/last_col"),
    ("i1_not_clamped", "direct_5x256-f32-noise", "y/last_col"),
    ("i1_not_clamped", "direct_3x16-f32-ramp_j", "y/last_row"),                # the ramp is 0 at column 0: A = 0, any leak is outside the bound
    ("clamped_edge_l0_only", "gen_138_274-f32-noise", "gx/last_col"),
    ("window_short_lo", "direct_3x16-f32-noise", "gx/all"),
    ("window_short_hi", "direct_3x16-f32-noise", "gx/all"),
    ("window_short_hi", "tiled_5x12-f32-noise", "gx/all"),
    ("window_short_lo", "gen_x4_x3-f32-noise", "gx/all"),
    ("window_short_hi", "gen_x4_x3-f32-noise", "gx/all"),
    ("wave_edge_from_shuffle", "direct_2x512-f32-noise", "y/wave_cols"),
    ("wave_edge_from_shuffle", "direct_2x512-f32-noise", "gx/wave_cols"),
    ("wave_edge_from_shuffle", "direct_4x1024-bf16-noise", "y/wave_cols"),
    ("strided_dense_offset", "strided_direct-f32-noise", "y/all"),
    ("strided_dense_offset", "strided_tiled-f32-noise", "gx/all"),
    ("first_column_weight", "direct_3x16-f32-noise", "y/first_col"),
]


@pytest.mark.parametrize("fault,case_id,key", FAULTS, ids=[f"{f}-{c}-{k.replace('/', '_')}" for f, c, k in FAULTS])
def test_faults_are_caught(fault, case_id, key):
    case = U.CASE[case_id]
    inp = U.build(case)
    k = U.K[U.kernel_of(case, key)]
    good = U.figures(case, inp, **{n: restate(case, inp)[n] for n in ("y", "gx")})[key]
    bad = U.figures(case, inp, **{n: restate(case, inp, fault)[n] for n in ("y", "gx")})[key]
    print(f"{fault}: {key} on {case_id}: {bad / k:.3g} x the bound (sound restatement: {good / k:.3g} x)")
    assert good <= k
    assert bad >= 10 * k, f"{fault} is only {bad / k:.3g} x the bound of {key} on {case_id}"


def test_faults_that_no_value_shows():
    """Module docstring: l1 is exactly 0 at the last output of every shape but 138 -> 274, so there the generic and tiled
    restatements return the same bits without the clamp of i1 and with l0 alone at the clamped edge; and the tiled backward
    returns the same bits with its window one short at the first end."""
    for sid, (shape, size, fwd, bwd) in U.SHAPES.items():
        case = U.CASE[f"{sid}-f32-noise"]
        inp = U.build(case)
        if bwd == U.TIL_B:
            assert np.array_equal(R.backward(inp["gy"], shape[2:], bwd), R.backward(inp["gy"], shape[2:], bwd, fault="window_short_lo"))
        if sid == "gen_138_274":
            continue
        for n_in, n_out in zip(shape[2:], size):
            i0, _, _, l1, _ = lerp_tables(n_in, n_out)
            assert (l1[i0 == n_in - 1] == 0).all(), (sid, n_in, n_out)
        if fwd != U.DIR_F:
            assert np.array_equal(R.forward(inp["x"], size, fwd), R.forward(inp["x"], size, fwd, fault="i1_not_clamped"))
        assert np.array_equal(R.backward(inp["gy"], shape[2:], bwd), R.backward(inp["gy"], shape[2:], bwd, fault="clamped_edge_l0_only"))


def test_fused_lambda_breaks_the_footprint():
    """lerp_lambda_fused leaves the footprint at 3 -> 7 (output 3) and 3 -> 11 (output 5), in both directions.  (At in = 2 its l1
    is negative at the last output, but i1 = i0 there: both weights land on one cell and no value shows it.)"""
    for n in (26, 30, 32):
        assert lerp_tables(2, n, fused=True)[3][-1] < 0 and lerp_tables(2, n)[3][-1] == 0
    for sid in ("gen_3_7_11",):
        hits = []
        for case in (c for c in U.CASES if c.shape_id == sid and c.dtype == "f32" and c.data.startswith("hot")):
            inp = U.build(case)
            hits += U.exact_checks(case, inp, R.forward(inp["x"], case.size, case.fwd, fault="lerp_lambda_fused"),
                                   R.backward(inp["gy"], case.shape[2:], case.bwd, fault="lerp_lambda_fused"))
        print(hits)
        assert any("one-hot x" in m for m in hits) and any("one-hot gy" in m for m in hits), sid


# ------------------------------------------------------------------------------------------------------------ exhaustive index facts

SIZES = np.arange(2, 4097)


def test_static_indices_are_the_rule():
    """For every w in 2..4096 at out = 2w: output 2j reads (j - 1, j) (j >= 1; output 0 reads cell 0 with l1 = 0) and output 2j + 1
    reads (j, j + 1), clamped to w - 1 at the last -- the float32 rule lands where the direct forward's static indices say."""
    for w in SIZES:
        i0, i1, _, l1, _ = lerp_tables(int(w), 2 * int(w))
        j = np.arange(w)
        assert i0[0] == 0 and l1[0] == 0
        assert np.array_equal(i0[2::2], j[1:] - 1) and np.array_equal(i1[2::2], j[1:]), w
        assert np.array_equal(i0[1::2], j) and np.array_equal(i1[1::2], np.minimum(j + 1, w - 1)), w


def test_backward_windows_hold_every_contributor():
    """For every w in 2..4096 at out = 2w: every output with a non-zero weight on cell j lies in 2j - 1 .. 2j + 2 (the direct
    backward's 4 candidates), hence in 2j - 3 .. 2j + 2 (the tiled backward's 6)."""
    for w in SIZES:
        i0, i1, l0, l1, _ = lerp_tables(int(w), 2 * int(w))
        o = np.arange(2 * w)
        for idx, lam in ((i0, l0), (i1, l1)):
            live = lam != 0
            assert (o[live] >= 2 * idx[live] - 1).all() and (o[live] <= 2 * idx[live] + 2).all(), w
            assert (o[live] >= 2 * idx[live] - 3).all(), w


def test_tiled_forward_source_tile_fits_lds():
    """For every h up to 4096 and every 16-row tile: r_hi - r_lo + 1 <= UF_SR; every w and every 512-column tile: <= UF_SC."""
    for n in SIZES:
        i0, i1, _, _, _ = lerp_tables(int(n), 2 * int(n))
        for tile, room in ((U.UF_OR, U.UF_SR), (U.UF_OC, U.UF_SC)):
            first = np.arange(0, 2 * n, tile)
            last = np.minimum(first + tile, 2 * n) - 1
            assert (i1[last] - i0[first] + 1).max() <= room, (n, tile)


if __name__ == "__main__":   # the K table
    by_kernel = {}
    for key, cases in GROUPS.items():
        worst, bad = figures(cases)
        print("-".join(key).ljust(28) + "  ".join(f"{k[9:-7]} {v[0]:.3f} ({v[1]})" for k, v in worst.items()) + ("  " + "; ".join(bad) if bad else ""))
        for kern, v in worst.items():
            if v[0] > by_kernel.get(kern, (-1.0,))[0]:
                by_kernel[kern] = v
    for kern, (v, k, cid) in by_kernel.items():
        print(f"{kern}: largest figure {v:.3f} ({k}, {cid}) -> K = {4 * v:.2f}; in the module: {U.K[kern]}")
