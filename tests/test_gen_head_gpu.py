"""The generator head kernels (csrc/gen_small_ops.hip) through the public ``sis_hip`` functions against the float64 references
of gen_head_cases.py: the exact tier bit for bit (integer operands, power-of-two scalars: no rounding can excuse a differing
element), the bound tier per element within K u32 A + B with the K measured on the CPU restatement (test_gen_head_cases_cpu.py,
which also shows that flipped or transposed taps, an exchanged skip height and width, a dropped last K chunk, latent row 0 for
row i, a bias without lr_mul and one element from the row above break these checks).

Every EqualLinear and ToRGB case names the kernel it must run and the test asserts it through ``sis_last_kernel()`` BEFORE it
compares a value: all four EqualLinear routes and both ToRGB routes are reached in-process by shape and alignment alone."""
import pytest
import torch

import gen_head_cases as C

pytestmark = pytest.mark.gpu


def _last_kernel():
    import sis_hip
    return sis_hip.lib().sis_last_kernel().decode()


def _one_float_in(t, device):
    """``t`` on the device, contiguous, its first element one float into a fresh buffer: 4 bytes off every 16-byte boundary."""
    flat = torch.full((t.numel() + 4,), float("nan"), dtype=torch.float32, device=device)
    view = flat[1:1 + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


@pytest.mark.parametrize("shape_id", [s.id for s in C.EL_SHAPES])
def test_equal_linear(device, shape_id):
    """Exact tier with every combination of bias / activation / lr_mul, one bound-tier combination; the strided form
    (x = latent[:, i] read in place) additionally bit for bit against the same call on contiguous rows."""
    import sis_hip as S
    s = C.EL_SHAPE[shape_id]
    rep = C.Report()
    for tier in ("exact", "randn"):
        op = C.el_operands(shape_id, tier)
        w, bias = op["w"].to(device), op["bias"].to(device)
        if s.strided:
            i, misaligned = s.strided
            latent = _one_float_in(op["latent"], device) if misaligned else op["latent"].to(device)
            x = latent[:, i]
            assert (x.data_ptr() % 16 != 0) == misaligned
            rows = dict(row_stride=C.N_LATENT * s.k, batch=s.batch)
        else:
            x, rows = op["x"].to(device), {}
        for combo in (C.COMBOS if tier == "exact" else [C.EL_BOUND_COMBO[shape_id]]):
            has_bias, act, lr_mul = combo
            args = (w, bias if has_bias else None, C.el_scale(shape_id, tier, combo), lr_mul, act)
            y = S.equal_linear(x, *args, **rows)
            assert _last_kernel() == s.route, f"{C.el_id(shape_id, tier, combo)} ran {_last_kernel()}, not {s.route}"
            assert tuple(y.shape) == (s.batch, s.out) and y.dtype == torch.float32
            rep.add(C.el_check(shape_id, tier, combo, y))
            if s.strided:
                dense = S.equal_linear(x.contiguous(), *args)
                assert _last_kernel() == s.route
                assert torch.equal(y, dense), f"{C.el_id(shape_id, tier, combo)}: rows read in place differ from contiguous rows"
    rep.finish()


@pytest.mark.parametrize("tier", ["exact", "randn"])
@pytest.mark.parametrize("batch,dim", C.MOD_CASES)
def test_modulation_and_demodulation(device, batch, dim, tier):
    """``modulation_batch`` (exact tier: bit for bit) and ``demod_batch`` / ``modconv_demod`` on tables laid out as
    Generator._modulate_all does: latent indices out of layer order, a ToRGB layer without a demodulation row, a row without
    demodulation (the scale itself, inside its own slice only).  The flat buffers are born NaN with a NaN tail."""
    import sis_hip as S
    assert S.head_gemm_tile() == C.HEAD_TILE
    op = C.mod_operands(batch, dim, tier)
    rows, (s_total, d_total, mblocks, dblocks) = C.layout(batch)
    dev = [{k: v.to(device) for k, v in L.items()} for L in op["layers"]]
    wsq = []
    for L, D in zip(op["layers"], dev):
        wpk_d, wsq_d = S.modconv_prepack(D["weight"])
        if tier == "exact":
            wpk_ref, wsq_ref = C.prepack_ref(L["weight"])
            assert torch.equal(wpk_d.cpu(), wpk_ref) and torch.equal(wsq_d.cpu(), wsq_ref)
        wsq.append(wsq_d)
    mod, dem = C.tables(batch, [(D["mw"].data_ptr(), D["mb"].data_ptr(), q.data_ptr()) for D, q in zip(dev, wsq)], tier)
    mod, dem = mod.to(device), dem.to(device)
    latent = op["latent"].to(device)
    tail = 256
    s_flat = torch.full((s_total + tail,), float("nan"), dtype=torch.float32, device=device)
    S.modulation_batch(s_flat, latent, mod, mod.shape[0], mblocks, C.mod_scale(dim, tier))
    s_in = torch.full((s_total + tail,), float("nan"), dtype=torch.float32, device=device)
    for (cin, _, _, _), (s_off, _, _, _), D in zip(C.LAYERS, rows, dev):
        s_in[s_off:s_off + batch * cin] = D["s_in"].reshape(-1)
    d_flat = torch.full((d_total + tail,), float("nan"), dtype=torch.float32, device=device)
    S.demod_batch(d_flat, s_in, dem, dem.shape[0], dblocks, batch)
    assert bool(s_flat[s_total:].isnan().all()) and bool(d_flat[d_total:].isnan().all()), "a store past the last slice"
    rep = C.Report()
    for li, ((cin, cout, lat, d), (s_off, d_off, _, _), D, q) in enumerate(zip(C.LAYERS, rows, dev, wsq)):
        rep.add(C.mod_check(batch, dim, tier, li, s_flat[s_off:s_off + batch * cin].view(batch, cin)))
        if d is None:
            continue
        rep.add(C.dem_check(batch, dim, tier, li, C.HG2, d_flat[d_off:d_off + batch * cout].view(batch, cout), q))
        rep.add(C.dem_check(batch, dim, tier, li, C.DEM, S.modconv_demod(D["s_in"], q, C.dem_scale(cin, tier), d), q))
    rep.finish()


RGB_SHAPE_IDS = list(dict.fromkeys(c.shape_id for c in C.RGB_CASES))


@pytest.mark.parametrize("shape_id", RGB_SHAPE_IDS)
def test_to_rgb(device, shape_id):
    """Both tiers, without skip and with every kind of taps the map's size allows: k = 2, 3, 4 and the project's own blur on
    the fast route, k = 6 through ``skip_up2``."""
    import sis_hip as S
    rep = C.Report()
    for tier in ("exact", "randn"):
        op = C.rgb_operands(shape_id, tier)
        for case in [c for c in C.RGB_CASES if c.shape_id == shape_id]:
            x = _one_float_in(op["x"], device) if case.misaligned else op["x"].to(device)
            w, s, bias = op["w"].to(device), op["s"].to(device), op["bias"].to(device)
            if case.kind is None:
                y = S.to_rgb(x, w, s, bias, op["scale"])
            else:
                taps = C.taps_of(case.kind, tier)
                y = S.to_rgb(x, w, s, bias, op["scale"], op["skip"].to(device), taps.to(device), C.upsample_pad(taps.shape[0]))
            assert _last_kernel() == case.route, f"{case.id}-{tier} ran {_last_kernel()}, not {case.route}"
            assert tuple(y.shape) == (case.b, case.cout, case.h, case.w)
            rep.add(C.rgb_check(case, tier, y))
    rep.finish()


@pytest.mark.parametrize("dims", C.FIN_SHAPES, ids=["x".join(str(d) for d in dims) for dims in C.FIN_SHAPES])
def test_rgb_finish(device, dims):
    """``rgb_finish(part)`` against the reference sum of the same ``part``: no skip, a k = 4 skip and a k = 6 skip."""
    import sis_hip as S
    rep = C.Report()
    for tier in ("exact", "randn"):
        op = C.fin_operands(dims, tier)
        part, bias, skip = (op[k].to(device) for k in ("part", "bias", "skip"))
        for kind in C.FIN_KINDS:
            if kind is None:
                y = S.rgb_finish(part, bias)
            else:
                y = S.rgb_finish(part, bias, skip, C.taps_of(kind, tier).to(device), C.upsample_pad(kind))
            rep.add(C.fin_check(dims, kind, tier, y))
    rep.finish()


def test_pixel_norm(device):
    import sis_hip as S
    rep = C.Report()
    for shape in C.PN_SHAPES:
        for family in C.PN_FAMILIES:
            rep.add(C.pn_check(shape, family, S.pixel_norm(C.pn_input(shape, family).to(device))))
    rep.finish()


def test_truncate(device):
    import sis_hip as S
    rep = C.Report()
    for shape in C.TR_SHAPES:
        w, mean = C.tr_operands(shape, "exact")
        rep.add(C.tr_check(shape, C.TR_PSI_EXACT, "exact", S.truncate(w.to(device), mean.to(device), C.TR_PSI_EXACT)))
        w, mean = C.tr_operands(shape, "randn")
        for psi in C.TR_PSI:
            rep.add(C.tr_check(shape, psi, "randn", S.truncate(w.to(device), mean.to(device), psi)))
    rep.finish()


@pytest.mark.parametrize("dims", C.PREPACK_SHAPES, ids=["x".join(str(d) for d in dims) for dims in C.PREPACK_SHAPES])
def test_prepack(device, dims):
    """``wpk`` is the permutation and ``wsq`` the exact sum, bit for bit."""
    import sis_hip as S
    import exact_operands as X
    weight = C.prepack_weight(dims)
    wpk_ref, wsq_ref = C.prepack_ref(weight)
    wpk, wsq = S.modconv_prepack(weight.to(device))
    X.assert_bitwise(wpk, wpk_ref, f"wpk {dims}")
    X.assert_bitwise(wsq, wsq_ref, f"wsq {dims}")
