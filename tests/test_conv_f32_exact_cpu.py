"""CPU: what tests/test_conv_f32_exact_gpu.py rests on, checked without a GPU and without the package.

* the plans: the restatement (tests/conv_f32_plan.py) gives every case of tests/conv_f32_exact_cases.py the route it claims,
  and every route value that a grid of eligible shapes reaches is claimed by some case;
* the operand rules (tests/exact_operands.py): an fp32 emulation of Winograd F(2x2,3x3) forward and weight gradient -- fp32
  transforms, fp32 chained accumulation in channel / tile order and in the plan's slab order, the output / finish transforms step
  by step as the kernels write them -- gives the float64 reference bit for bit, also at the radius boundaries with all-r operands;
* conditions on every reference: exactly representable, dense, every tap / row / column populated;
* sensitivity: simulated defects in that pipeline change the result of a case that claims the route concerned."""
import itertools
import math

import pytest
import torch
import torch.nn.functional as F

import conv_f32_exact_cases as C
import conv_f32_plan as P
import exact_operands as E


# ---------------------------------------------------------------------------------------------------- the plans

def _claims_hold(route, claim, what):
    assert route is not None, f"{what}: not eligible"
    for key, value in claim.items():
        assert route[key] == value, f"{what}: {key} is {route[key]!r}, the case claims {value!r}"


def test_every_case_reaches_the_route_it_claims():
    for s, claim in C.FORWARD_CASES.items():
        _claims_hold(P.wino_forward_route(*s), claim, f"forward {s}")
        b, ci, co, h, w = s
        assert P.wino_forward_eligible(b, co, ci, h, w), f"data gradient of {s}"
    for s in (C.WIDE_FORWARD_SHAPE, C.SECOND_ORDER_CASE):
        assert P.wino_forward_eligible(*s)
    for s, claim in C.WGRAD_CASES.items():
        _claims_hold(P.wino_wgrad_route(*s), claim, f"weight gradient {s}")
    assert P.wino_wgrad_route(*C.WIDE_WGRAD_SHAPE) is not None
    for (kind, jobs, shape), slices in C.BATCHED_CASES.items():
        b, ci, co, h, w = shape
        launches = P.wino_wgrad_launches(jobs, *shape) if kind == "f3" else P.pwg_launches(jobs, b, ci, co, h * w)
        assert [p["slices"] for _, _, p in launches] == slices, (kind, jobs, shape, launches)
        assert sum(n for _, n, _ in launches) == jobs
    for s, (fwd, dgrad) in C.POINTWISE_CASES.items():
        b, ci, co, h, w, _ = s
        assert P.pointwise_supported(ci, co, h * w)
        _claims_hold(P.pointwise_plan(b, ci, co, h * w), fwd, f"pointwise {s}")
        _claims_hold(P.pointwise_plan(b, ci, co, h * w, True), dgrad, f"pointwise data gradient {s}")
    for s, claim in C.POINTWISE_WGRAD_CASES.items():
        b, ci, co, h, w = s
        _claims_hold(P.pwg_plan(b, ci, co, h * w), claim, f"pointwise weight gradient {s}")
    # the wrappers: the launches behind them are eligible, so nothing has a reason to fall back
    for (b, ci, co, h, w), d in C.DILATED_CASES:
        assert P.wino_forward_eligible(b * d * d, ci, co, h // d, w // d) and P.wino_forward_eligible(b * d * d, co, ci, h // d, w // d)
        assert P.wino_wgrad_plan(b * d * d, ci, co, h // d, w // d) is not None
    b, ci, co, h, w = C.HALF_DILATION_CASE
    assert P.pointwise_supported(4 * ci, 4 * co, h * w // 4) and P.pwg_supported(b, 4 * ci, 4 * co, h * w // 4)
    (b, ci, co, h, w), _ = C.STRIDE2_CASES[0]
    assert P.wino_forward_eligible(b, ci, co, h, w) and P.wino_wgrad_plan(b, ci, co, h, w) is not None
    (b, ci, co, h, w), _ = C.STRIDE2_CASES[1]
    assert P.pointwise_supported(ci, co, h * w // 4) and P.pwg_supported(b, ci, co, h * w // 4)
    b, ci, co, h, w = C.DOWN_CASE
    assert P.wino_forward_eligible(b, 4 * ci, co, h // 2, w // 2) and P.wino_forward_eligible(b, co, 4 * ci, h // 2, w // 2)
    assert P.wino_wgrad_plan(b, 4 * ci, co, h // 2, w // 2) is not None
    assert P.wino_wgrad_plan(*C.SECOND_ORDER_CASE) is not None


MAX_OPERAND_BYTES = 32 << 20      # what a test of a few seconds can upload and check


def _values(routes, keys):
    return {k: {tuple(r[k]) if isinstance(r[k], list) else r[k] for r in routes} for k in keys}


def test_every_reachable_route_value_is_claimed():
    # Winograd forward (both directions of every case count: the data gradient is the same launch on transposed channels)
    keys = ("kernel", "xi", "split", "tpw", "xcd_group", "partial_rows", "partial_cols", "short_batch_tile", "partial_co", "co_blocks")
    grid = []
    for b, ci, co, h, w in itertools.product((1, 2, 4, 5, 8, 9, 16, 64, 2048, 4096), (8, 16, 32, 40, 64, 256), (8, 64, 72, 128, 256),
                                             (2, 4, 8, 10, 16, 20, 32, 64), (4, 8, 12, 16, 32, 64, 128)):
        if 4 * b * max(ci, co) * h * w <= MAX_OPERAND_BYTES:
            r = P.wino_forward_route(b, ci, co, h, w)
            if r is not None:
                grid.append(r)
    assert len(grid) > 1000
    claimed = [P.wino_forward_route(*s) for s in C.FORWARD_CASES] + [P.wino_forward_route(s[0], s[2], s[1], s[3], s[4]) for s in C.FORWARD_CASES]
    reachable, have = _values(grid, keys), _values(claimed, keys)
    assert reachable["xi"] == {None, 1, 2} and reachable["tpw"] == {1, 2, 4}, reachable     # (the module docstring of conv_f32_plan says why)
    for k in keys:
        assert reachable[k] <= have[k], f"forward route {k}: reachable {reachable[k]}, claimed {have[k]}"
    # Winograd weight gradient
    keys = ("chunks", "last_slice", "reduce", "odd_divisors", "w2", "h2", "chunk_crosses_samples", "ci_blocks", "co_blocks")
    grid = [r for r in (P.wino_wgrad_route(*s) for s in itertools.product((1, 2, 3, 4, 8), (64, 128), (64, 128), (2, 4, 6, 8, 12, 16),
                                                                         (2, 4, 8, 10, 14, 20, 26, 28, 32, 44))) if r is not None]
    reachable, have = _values(grid, keys), _values([P.wino_wgrad_route(*s) for s in C.WGRAD_CASES], keys)
    for k in keys:
        assert reachable[k] <= have[k], f"weight-gradient route {k}: reachable {reachable[k]}, claimed {have[k]}"
    multi = [r for r in (P.wino_wgrad_route(*s) for s in C.WGRAD_CASES) if r["ksplit"] > 1]
    assert {r["last_slice"] for r in multi} >= {1, 2, 3, 4} and {r["slices"][0] % 2 for r in multi} == {0, 1}
    # pointwise forward / data gradient: every tile, whole and checked, in both directions
    keys = ("kernel", "checked_tile", "partial_pixels")
    grid, have = [], []
    for dg in (False, True):
        for b, ci, co, hw in itertools.product((1, 3, 128, 256), (32, 64, 96, 128, 160), (32, 64, 96, 128, 160), (4, 80, 132, 256)):
            r = P.pointwise_plan(b, ci, co, hw, dg)
            if r is not None and P.pointwise_supported(ci, co, hw):
                grid.append(dict(r, kernel=(dg, r["kernel"]), checked_tile=(dg, r["mt"], r["checked"])))
        for (b, ci, co, h, w, _) in C.POINTWISE_CASES:
            r = P.pointwise_plan(b, ci, co, h * w, dg)
            have.append(dict(r, kernel=(dg, r["kernel"]), checked_tile=(dg, r["mt"], r["checked"])))
    reachable, have = _values(grid, keys), _values(have, keys)
    assert len(reachable["kernel"]) == 8
    for k in keys:
        assert reachable[k] <= have[k], f"pointwise route {k}: reachable {reachable[k] - have[k]} not claimed"
    # pointwise weight gradient
    plans = [P.pwg_plan(b, ci, co, h * w) for (b, ci, co, h, w) in C.POINTWISE_WGRAD_CASES]
    assert {p["tile_id"] for p in plans} == {0, 1, 2, 3}
    assert {(p["ksplit"] > 1, len(set(p["slices"])) > 1) for p in plans} == {(False, False), (True, False), (True, True)}
    for (b, ci, co, h, w) in C.POINTWISE_WGRAD_CASES:
        assert (P.pwg_workspace(b, ci, co, h * w) == 0) == (P.pwg_plan(b, ci, co, h * w)["ksplit"] == 1)


def test_tile_index_split_is_exact_on_every_case():
    """The kernel's float-reciprocal split with its one correction step is divmod for every tile of every case -- also when the
    truncated quotient is replaced by one rounded up (the correction absorbs an error of one in either direction)."""
    for (b, ci, co, h, w) in list(C.WGRAD_CASES) + [(64, 64, 64, 6, 6), (1 << 12, 64, 64, 6, 14)]:
        tps, tpr = (h // 2) * (w // 2), w // 2
        for t in range(0, b * tps, 1 if b * tps < 4096 else 97):
            want = (t // tps, (t % tps) // tpr, t % tpr)
            assert P.tile_split(t, tps, tpr) == want
            assert P.tile_split(t, tps, tpr, quotient=lambda q: int(math.ceil(q))) == want


# ---------------------------------------------------------------------------------------------------- fp32 emulation

def _fma(acc, a, b):
    """acc + a * b as the fp32 matrix core computes it: the product exact, one rounding of the sum."""
    return (acc.double() + a.double() * b.double()).float()


def _patches(x, clamp=None):
    """[B,C,H,W] -> the 4x4 input patches of the 2x2 output tiles [B,C,TY,TX,4,4], zero beyond the image.  ``clamp`` (a defect):
    the masked neighbour on that side is read as the nearest in-image value instead."""
    xp = F.pad(x, (1, 1, 1, 1))
    if clamp == "left":
        xp[..., :, 0] = xp[..., :, 1]
    elif clamp == "right":
        xp[..., :, -1] = xp[..., :, -2]
    elif clamp == "top":
        xp[..., 0, :] = xp[..., 1, :]
    elif clamp == "bottom":
        xp[..., -1, :] = xp[..., -2, :]
    return xp.unfold(2, 4, 2).unfold(3, 4, 2)


def _bt_d_b(d):
    """V = B^T d B in the steps of the kernels (conv_wgrad_wino.hip:128-143): adds only."""
    r = torch.stack([d[..., 0, :] - d[..., 2, :], d[..., 1, :] + d[..., 2, :], d[..., 2, :] - d[..., 1, :], d[..., 1, :] - d[..., 3, :]], -2)
    return torch.stack([r[..., 0] - r[..., 2], r[..., 1] + r[..., 2], r[..., 2] - r[..., 1], r[..., 1] - r[..., 3]], -1)


def _g_g_gt(g):
    """U = G g G^T, G = [[1,0,0],[.5,.5,.5],[.5,-.5,.5],[0,0,1]]."""
    r = torch.stack([g[..., 0, :], 0.5 * ((g[..., 0, :] + g[..., 1, :]) + g[..., 2, :]), 0.5 * ((g[..., 0, :] - g[..., 1, :]) + g[..., 2, :]),
                     g[..., 2, :]], -2)
    return torch.stack([r[..., 0], 0.5 * ((r[..., 0] + r[..., 1]) + r[..., 2]), 0.5 * ((r[..., 0] - r[..., 1]) + r[..., 2]), r[..., 2]], -1)


def _at_m_a(m):
    """y = A^T M A step by step: (M0 + M1) + M2, (M1 - M2) - M3 on rows, then on columns."""
    r = torch.stack([(m[..., 0, :] + m[..., 1, :]) + m[..., 2, :], (m[..., 1, :] - m[..., 2, :]) - m[..., 3, :]], -2)
    return torch.stack([(r[..., 0] + r[..., 1]) + r[..., 2], (r[..., 1] - r[..., 2]) - r[..., 3]], -1)


def _a_dy_at(t):
    """E = A dY A^T of the 2x2 tiles [..., 2, 2] (conv_wgrad_wino.hip:117-126), A = [[1,0],[1,1],[1,-1],[0,-1]]."""
    a, b, c, d = t[..., 0, 0], t[..., 0, 1], t[..., 1, 0], t[..., 1, 1]
    rp, rq = [a, a + c, a - c, -c], [b, b + d, b - d, -d]
    return torch.stack([torch.stack([p, p + q, p - q, -q], -1) for p, q in zip(rp, rq)], -2)


def _gt_s_g(s):
    """dW = G^T S G as conv_wgrad_finish_kernel writes it (conv_wgrad_wino.hip:281-294)."""
    t = torch.stack([s[..., 0, :] + 0.5 * (s[..., 1, :] + s[..., 2, :]), 0.5 * (s[..., 1, :] - s[..., 2, :]),
                     0.5 * (s[..., 1, :] + s[..., 2, :]) + s[..., 3, :]], -2)
    return torch.stack([t[..., 0] + 0.5 * (t[..., 1] + t[..., 2]), 0.5 * (t[..., 1] - t[..., 2]), 0.5 * (t[..., 1] + t[..., 2]) + t[..., 3]], -1)


def emulate_forward(x, w, slabs=1, chained=True, operand=None, twice=False):
    """Winograd F(2x2,3x3) forward in fp32.  ``slabs``: K slices of the channel axis, summed in slice order (the split-K finish);
    ``chained`` = False: float64 sums per slab, rounded once (the quick form for the sensitivity checks).  Defects: ``operand``
    maps the matrix-core operands U and V (a truncation), ``twice`` adds the second slab twice."""
    u, v = _g_g_gt(w.float()), _bt_d_b(_patches(x.float()))            # [O,C,4,4], [B,C,TY,TX,4,4]
    if operand is not None:
        u, v = operand(u), operand(v)
    cin = x.shape[1]
    per = -(-cin // slabs)
    parts = []
    for c0 in range(0, cin, per):
        if chained:
            acc = torch.zeros(x.shape[0], w.shape[0], v.shape[2], v.shape[3], 4, 4)
            for c in range(c0, min(cin, c0 + per)):
                acc = _fma(acc, u[None, :, c, None, None], v[:, None, c])
        else:
            acc = torch.einsum("ocij,bcyxij->boyxij", u[:, c0:c0 + per].double(), v[:, c0:c0 + per].double()).float()
        parts.append(acc)
    if twice:
        parts.append(parts[1])
    m = parts[0]
    for p in parts[1:]:
        m = m + p
    y = _at_m_a(m)                                                      # [B,O,TY,TX,2,2]
    return y.permute(0, 1, 2, 4, 3, 5).reshape(x.shape[0], w.shape[0], x.shape[2], x.shape[3])


def emulate_wgrad(x, gy, slices=None, chained=True, operand=None, twice=False, drop_last_chunk=False, clamp=None, split=None):
    """The Winograd-domain weight gradient in fp32: S accumulated over the tiles in flat (sample, row, column) order, one slab
    per slice of the plan (``slices``: chunks per slice, 8 tiles per chunk), slabs added in slice order, then the finish
    transform.  Defects: ``operand`` (truncation of E and V), ``twice`` (the second slab added twice), ``drop_last_chunk`` (of the
    last slice), ``clamp`` (a masked neighbour read clamped), ``split`` (another tile-index split: tile t reads the patch and the
    dY tile that split names, zeros where it points outside)."""
    b, cin, h, w = x.shape
    cout, ty, tx = gy.shape[1], h // 2, w // 2
    v = _bt_d_b(_patches(x.float(), clamp)).permute(0, 2, 3, 1, 4, 5).reshape(b * ty * tx, cin, 4, 4)
    e = _a_dy_at(gy.float().unfold(2, 2, 2).unfold(3, 2, 2)).permute(0, 2, 3, 1, 4, 5).reshape(b * ty * tx, cout, 4, 4)
    if split is not None:
        idx, ok = [], []
        for t in range(b * ty * tx):
            bb, yy, xx = split(t, ty * tx, tx)
            inside = 0 <= bb < b and 0 <= yy < ty and 0 <= xx < tx
            idx.append((bb * ty + yy) * tx + xx if inside else 0)
            ok.append(inside)
        idx, ok = torch.tensor(idx), torch.tensor(ok)
        v, e = v[idx] * ok[:, None, None, None], e[idx] * ok[:, None, None, None]
    if operand is not None:
        e, v = operand(e), operand(v)
    tiles = b * ty * tx
    slices = slices or [tiles // P.GK]
    slabs, t0 = [], 0
    for n, chunks in enumerate(slices):
        t1 = t0 + chunks * P.GK
        hi = t1 - P.GK if drop_last_chunk and n == len(slices) - 1 else t1
        if chained:
            acc = torch.zeros(cout, cin, 4, 4)
            for t in range(t0, hi):
                acc = _fma(acc, e[t, :, None], v[t, None])
        else:
            acc = torch.einsum("toij,tcij->ocij", e[t0:hi].double(), v[t0:hi].double()).float()
        slabs.append(acc)
        t0 = t1
    if twice:
        slabs.append(slabs[1])
    s = torch.zeros_like(slabs[0])
    for slab in slabs:
        s = s + slab
    return _gt_s_g(s)


def _same(got, ref):
    return torch.equal(got.double(), ref)


def test_fp32_emulation_of_the_forward_is_the_float64_reference():
    shapes = sorted(C.FORWARD_CASES, key=lambda s: s[0] * s[1] * s[2] * s[3] * s[4])[:2] + [(1, 32, 8, 16, 16)]
    for s in shapes:
        c = C.forward_case(*s)
        assert _same(emulate_forward(c["x"], c["w"]), c["y"]), s
        assert _same(emulate_forward(c["x"], c["w"], slabs=2), c["y"]), s
        dx = emulate_forward(c["gy"], c["w"].flip(2, 3).transpose(0, 1))          # the adjoint filter bank
        assert _same(dx, c["dx"]), s
    for mirrored in (False, True):
        c = C.wide_forward_case(mirrored)
        assert _same(emulate_forward(c["x"], c["w"]), c["y"]) and _same(emulate_forward(c["x"], c["w"], slabs=4), c["y"])
        assert _same(emulate_forward(c["gy"], c["w"].flip(2, 3).transpose(0, 1)), c["dx"])


@pytest.mark.parametrize("cin,cap", [(64, 15), (64, 28), (230, 15), (512, 15), (2048, 15)])
def test_forward_radius_boundary_with_all_r_operands(cin, cap):
    """r = winograd_radius(cin): all-r operands (every bound of the derivation is met at the image centre) and random ones."""
    r = E.winograd_radius(cin, cap)
    assert 324 * cin * r * r < E.EXACT_F32 <= 324 * cin * (r + 1) * (r + 1) or r == cap
    gen = torch.Generator().manual_seed(cin)
    for x, w in ((torch.full((1, cin, 4, 4), float(r)), torch.full((2, cin, 3, 3), float(r))),
                 (E.integers((1, cin, 4, 4), r, gen, dtype=torch.float32), E.integers((2, cin, 3, 3), r, gen, dtype=torch.float32))):
        ref = E.check_reference(E.conv_ref(x, w))
        assert _same(emulate_forward(x, w), ref) and _same(emulate_forward(x, w, slabs=2), ref)


def test_fp32_emulation_of_the_weight_gradient_is_the_float64_reference():
    shapes = sorted(C.WGRAD_CASES, key=lambda s: s[0] * s[3] * s[4])[:2] + [(3, 64, 64, 8, 28)]
    for s in shapes:
        c, plan = C.wgrad_case(*s), P.wino_wgrad_plan(*s)
        assert _same(emulate_wgrad(c["x"], c["gy"]), c["dw"]), s
        assert _same(emulate_wgrad(c["x"], c["gy"], plan["slices"]), c["dw"]), s
        if plan["chunks_total"] >= 2:
            assert _same(emulate_wgrad(c["x"], c["gy"], [1, plan["chunks_total"] - 1]), c["dw"]), s
    for mirrored in (False, True):
        c = C.wide_wgrad_case(mirrored)
        assert _same(emulate_wgrad(c["x"], c["gy"]), c["dw"]) and _same(emulate_wgrad(c["x"], c["gy"], [1, 1]), c["dw"])


@pytest.mark.parametrize("tiles", [8, 168, 1024])
def test_weight_gradient_radius_boundary_with_all_r_operands(tiles):
    r = E.winograd_wgrad_radius(tiles, cap=60)
    assert 576 * tiles * r * r < E.EXACT_F32 <= 576 * tiles * (r + 1) * (r + 1)
    h, w = 4, tiles       # tiles = 1 * 2 * (w / 2)
    for x, gy in ((torch.full((1, 2, h, w), float(r)), torch.full((1, 2, h, w), float(r))),):
        ref = E.check_reference(E.conv_grads_ref(x, torch.zeros(2, 2, 3, 3), gy)[1])
        assert _same(emulate_wgrad(x, gy), ref) and _same(emulate_wgrad(x, gy, [tiles // 16, tiles // 8 - tiles // 16]), ref)


# ---------------------------------------------------------------------------------------------------- the references

def test_every_reference_is_exact_dense_and_populated():
    for label, ref, kind in C.references():
        E.check_reference(ref)
        nonzero = float((ref != 0).double().mean())
        assert nonzero >= (0.5 if kind == "wide" else 0.9), f"{label}: {nonzero:.3f} nonzero"
        if kind == "dw3":
            assert all(bool(ref[:, :, a, b].any()) for a in range(3) for b in range(3)), label
        elif kind == "map":
            assert bool((ref != 0).flatten(0, 1).any(0).all()), f"{label}: an output pixel position that is zero in every image and channel"
    c = C.down_case()
    for name in ("y", "dx", "dw"):
        E.check_reference(c[name], c["unit"])
        assert float((c[name] != 0).double().mean()) >= 0.9, name


# ---------------------------------------------------------------------------------------------------- sensitivity

def _wg(s, **defect):
    c, plan = C.wgrad_case(*s), P.wino_wgrad_plan(*s)
    got = emulate_wgrad(c["x"], c["gy"], plan["slices"], chained=False, **defect)
    return got, c["dw"]


def test_the_quick_pipeline_is_the_reference_on_every_case():
    """(chained = False: float64 sums per slab; what the sensitivity checks below apply their defects to)"""
    for s in C.WGRAD_CASES:
        got, ref = _wg(s)
        assert _same(got, ref), s
    for s in C.FORWARD_CASES:
        if s[0] <= 64:
            c = C.forward_case(*s)
            assert _same(emulate_forward(c["x"], c["w"], P.wino_forward_plan(*s)["ksplit"], chained=False), c["y"]), s


def test_a_dropped_last_chunk_of_a_slice_shows():
    for s in C.WGRAD_CASES:
        got, ref = _wg(s, drop_last_chunk=True)
        assert not _same(got, ref), s


@pytest.mark.parametrize("side", ["left", "right", "top", "bottom"])
def test_a_masked_neighbour_read_clamped_shows(side):
    for s in C.WGRAD_CASES:
        got, ref = _wg(s, clamp=side)
        assert not _same(got, ref), (s, side)


def test_a_slab_added_twice_shows():
    hit = 0
    for s in C.WGRAD_CASES:
        if P.wino_wgrad_plan(*s)["ksplit"] > 1:
            got, ref = _wg(s, twice=True)
            assert not _same(got, ref), s
            hit += 1
    assert hit >= 4
    for s in C.FORWARD_CASES:
        k = P.wino_forward_plan(*s)["ksplit"]
        if k > 1:
            c = C.forward_case(*s)
            assert not _same(emulate_forward(c["x"], c["w"], k, chained=False, twice=True), c["y"]), s
            hit += 1
    assert hit >= 7


def test_a_tile_split_without_its_correction_step_shows():
    """The quotient rounded up instead of truncated, and no correction: every case whose divisors are no powers of two (and
    every other case with more than one tile per sample) reads wrong tiles."""
    wrong = lambda t, tps, tpr: P.tile_split(t, tps, tpr, correct=False, quotient=lambda q: int(math.ceil(q)))
    hit = 0
    for s in C.WGRAD_CASES:
        route = P.wino_wgrad_route(*s)
        if any(route["odd_divisors"]):
            got, ref = _wg(s, split=wrong)
            assert not _same(got, ref), s
            hit += 1
            got, ref = _wg(s, split=P.tile_split)
            assert _same(got, ref), s
    assert hit >= 4


def test_operands_cut_to_11_bits_show_on_the_wide_cases_only():
    """Why the wide cases exist: small integers pass through an operand path that keeps 11 significant bits, 12-bit operands do
    not.  (Pointwise kernels multiply the raw operands: there the 12-bit taps of the mirrored pair are the wide ones.)"""
    cut = lambda t: E.truncate_significand(t, 11)
    for s in [s for s in C.FORWARD_CASES if s[0] <= 64]:
        c = C.forward_case(*s)
        assert _same(emulate_forward(c["x"], c["w"], chained=False, operand=cut), c["y"]), s
    for s in C.WGRAD_CASES:
        got, ref = _wg(s, operand=cut)
        assert _same(got, ref), s
    for mirrored in (False, True):
        c = C.wide_forward_case(mirrored)
        assert not _same(emulate_forward(c["x"], c["w"], chained=False, operand=cut), c["y"]), mirrored
        c = C.wide_wgrad_case(mirrored)
        assert not _same(emulate_wgrad(c["x"], c["gy"], chained=False, operand=cut), c["dw"]), mirrored
    for s in C.POINTWISE_CASES:
        c = C.pointwise_case(*s)
        assert torch.equal(E.conv_ref(cut(c["x"]), cut(c["w"]), c["bias"]), c["y"]), s
    for s in C.POINTWISE_WGRAD_CASES:
        c = C.pointwise_wgrad_case(*s)
        assert torch.equal(E.pointwise_wgrad_ref(cut(c["x"]), cut(c["gy"])).view_as(c["dw"]), c["dw"]), s
    c = C.wide_pointwise_case(True)
    assert not torch.equal(E.conv_ref(cut(c["x"]), cut(c["w"])), c["y"])
    c = C.wide_pointwise_wgrad_case(True)
    assert not torch.equal(E.pointwise_wgrad_ref(cut(c["x"]), cut(c["gy"])).view_as(c["dw"]), c["dw"])


def test_wide_operands_need_their_bits():
    for mirrored, (dense, sparse) in ((False, E.WIDE_PLAIN), (True, E.WIDE_MIRRORED)):
        c = C.wide_forward_case(mirrored)
        assert 2 ** (dense - 1) < float(c["x"].abs().max()) < 2 ** dense and 2 ** (sparse - 1) < float(c["w"].abs().max()) < 2 ** sparse
        assert int((c["w"] != 0).sum()) == c["w"].shape[0] and bool((c["w"] != 0).flatten(1).sum(1).eq(1).all())
        assert bool((c["w"] != 0).sum((0, 2, 3)).eq(1).all()), "the adjoint bank must be as sparse"
        c = C.wide_wgrad_case(mirrored)
        assert bool((c["gy"] != 0).flatten(2).sum(2).eq(1).all())
