"""Guard-band cases (tests/guard_bands.py) of the generator head routes that tests/test_guard_bands_gpu.py does not reach, in the
manner of tests/test_wino44_guard_bands_gpu.py: every operand between 0xFF bands, every result born NaN between two more.  No
store outside a result (the bands stay 0xFF), no operand changed, and no load from outside reaches a result: the comparisons
are the exact tier's of gen_head_cases.py (bit for bit; one NaN from a band is a mismatch) and, for the demodulation scales, its
element-wise bound.  One case per route: head_gemm_kernel<0> at 33 x 1088 -> 130 (interior and edge tiles, 17 chunks),
equal_linear_full_kernel<4> at 5 x 256 -> 7 (the row clamp), to_rgb_kernel<4> at 10 x 26 (a partial last group) with skip,
rgb_finish at 36 x 36 (a partial second group), and the batch-33 modulation / demodulation tables."""
import pytest
import torch

import gen_head_cases as C
import guard_bands as G
from test_guard_bands_gpu import T

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _fresh_session():
    G.reset()
    yield
    G.reset()


def _last_kernel():
    import sis_hip
    return sis_hip.lib().sis_last_kernel().decode()


@pytest.mark.parametrize("shape_id,route", [("el-33x1088x130", C.HG0), ("el-5x256x7", C.EL4)])
def test_equal_linear(device, monkeypatch, shape_id, route):
    import sis_hip
    t = T(device, monkeypatch)
    op = C.el_operands(shape_id, "exact")
    x, w, bias = t.put(op["x"]), t.put(op["w"]), t.put(op["bias"])
    rep = C.Report()
    for combo in ((True, True, 0.5), (False, False, 1.0)):
        y = t.run(sis_hip.equal_linear, x, w, bias if combo[0] else None, C.el_scale(shape_id, "exact", combo), combo[2], combo[1])
        assert _last_kernel() == route
        rep.add(C.el_check(shape_id, "exact", combo, y))
    rep.finish()


@pytest.mark.parametrize("kind", [None, 3, 6])
def test_to_rgb_vec4(device, monkeypatch, kind):
    import sis_hip
    t = T(device, monkeypatch)
    case = C.RGB_CASE["rgb-1x100x3x10x26-" + ("noskip" if kind is None else f"k{kind}")]
    op = C.rgb_operands(case.shape_id, "exact")
    args = [t.put(op[k]) for k in ("x", "w", "s", "bias")] + [op["scale"]]
    if kind is not None:
        args += [t.put(op["skip"]), t.put(C.taps_of(kind, "exact")), C.upsample_pad(kind)]
    y = t.run(sis_hip.to_rgb, *args)
    assert _last_kernel() == C.RGB4
    rep = C.Report()
    rep.add(C.rgb_check(case, "exact", y))
    rep.finish()


@pytest.mark.parametrize("kind", C.FIN_KINDS)
def test_rgb_finish(device, monkeypatch, kind):
    import sis_hip
    t = T(device, monkeypatch)
    dims = (3, 1, 3, 36, 36)
    op = C.fin_operands(dims, "exact")
    args = [t.put(op["part"]), t.put(op["bias"])]
    if kind is not None:
        args += [t.put(op["skip"]), t.put(C.taps_of(kind, "exact")), C.upsample_pad(kind)]
    rep = C.Report()
    rep.add(C.fin_check(dims, kind, "exact", t.run(sis_hip.rgb_finish, *args)))
    rep.finish()


def test_modulation_and_demodulation_tables_batch_33(device, monkeypatch):
    """Both batched launches at batch 33 and style dim 192 (two row tiles, three chunks) on tables that point at banded weights;
    the flat style and scale buffers are banded results."""
    import sis_hip
    t = T(device, monkeypatch)
    batch, dim, tier = 33, 192, "exact"
    op = C.mod_operands(batch, dim, tier)
    rows, (s_total, d_total, mblocks, dblocks) = C.layout(batch)
    placed, wsq = [], []
    s_in = torch.zeros(s_total)
    for L, (cin, _, _, _), (s_off, _, _, _) in zip(op["layers"], C.LAYERS, rows):
        placed.append((t.put(L["mw"]), t.put(L["mb"])))
        wsq.append(t.run(sis_hip.modconv_prepack, t.put(L["weight"]))[1])
        s_in[s_off:s_off + batch * cin] = L["s_in"].reshape(-1)
    mod, dem = C.tables(batch, [(mw.data_ptr(), mb.data_ptr(), q.data_ptr()) for (mw, mb), q in zip(placed, wsq)], tier)
    mod, dem, latent, s_in = t.put(mod), t.put(dem), t.put(op["latent"]), t.put(s_in)

    def launch():
        s_flat = sis_hip.torch.empty(s_total, dtype=torch.float32, device=device)
        d_flat = sis_hip.torch.empty(d_total, dtype=torch.float32, device=device)
        sis_hip.modulation_batch(s_flat, latent, mod, mod.shape[0], mblocks, C.mod_scale(dim, tier))
        sis_hip.demod_batch(d_flat, s_in, dem, dem.shape[0], dblocks, batch)
        return s_flat, d_flat

    s_flat, d_flat = t.run(launch)
    rep = C.Report()
    for li, ((cin, cout, _, d), (s_off, d_off, _, _), q) in enumerate(zip(C.LAYERS, rows, wsq)):
        rep.add(C.mod_check(batch, dim, tier, li, s_flat[s_off:s_off + batch * cin].view(batch, cin)))
        if d is not None:
            rep.add(C.dem_check(batch, dim, tier, li, C.HG2, d_flat[d_off:d_off + batch * cout].view(batch, cout), q))
    rep.finish()
