"""GPU, bit for bit: the bf16 GEMMs (csrc/gemm_bf16.hip, csrc/gemm256_bf16.hip) and csrc/column_sum.hip on exactly summable
operands (tests/exact_operands.py).  Integer operands keep every partial sum an fp32 value, so an fp32 result IS the float64
CPU product and a bf16 result IS its round-to-nearest-even image, whatever the tile, the split-K slab order or the association
-- ``assert_bitwise`` has no tolerance.  The one exception, the GELU epilogue, is bounded per element around the exactly known
pre-activation (``test_gelu_epilogue_per_element``).

The case builders below run on the CPU only; tests/test_exact_operands_cpu.py imports them to check, from the references alone,
that the rounding path of every bf16-output case is exercised."""
import functools
import math

import pytest
import torch

import exact_operands as E

pytestmark = pytest.mark.gpu

BIAS_R, RESID_R = 64, 1024        # integer fp32 bias / residual: K * r * r < 2^23 leaves them room below 2^24

NT_CASES = [(130, 132, 192), (128, 384, 64), (256, 256, 128), (392, 768, 768)]
NN_CASES = [(200, 136, 64), (256, 256, 128), (392, 768, 2304)]
TN_CASES = [(256, 256, 128, 1), (136, 264, 200, 2), (768, 768, 320, 4), (768, 768, 784, 8), (768, 768, 1100, 16)]
WGRAD_BIAS_CASES = [(136, 264, 200, 2), (264, 72, 1000, 2), (768, 768, 784, 8)]
WGRAD_MULTI_CASES = [(136, 264, 200), (768, 768, 784)]     # (out, in, tokens): the smallest of the shapes above and the 784-token one
COLUMN_SUM_CASES = [(77, 3072, torch.bfloat16, 15), (513, 260, torch.float32, 1024), (8192, 768, torch.bfloat16, 15)]
G256_CASES = [(64, 96, 256), (256, 96, 128), (300, 100, 192), (260, 580, 2304)]
BATCHED_CASES = [(4, 64, 72, 256), (2, 128, 256, 1024)]
GELU_CASE = (300, 388, 192)       # ragged in the 128- and the 256-row tiles; k = 192 keeps the pre-activation in GELU's curved range
PRE_R = 3                         # the stored derivative factor of EPI_GELU_BWD as an integer in [-3, 3]


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(v) for i, v in enumerate(key)) + 17)


@functools.lru_cache(maxsize=None)
def nt_case(m, n, k):
    """Operands and the exact results of every exact NT epilogue."""
    gen, r = _gen(m, n, k), E.radius(k)
    E.check_operands(k, r, r, 2)
    x, w = E.integers((m, k), r, gen), E.integers((n, k), r, gen)
    bias = E.integers((n,), BIAS_R, gen, dtype=torch.float32)
    resid = E.integers((m, n), RESID_R, gen, dtype=torch.float32)
    pre = E.integers((m, n), PRE_R, gen)
    E.check_operands(k, r, r, PRE_R)
    y = E.gemm_ref(x, w, "NT")
    return dict(x=x, w=w, bias=bias, resid=resid, pre=pre, y=y, y_bias=y + bias.double(), y_resid=resid.double() + y + bias.double(),
                y_pre=y * pre.double())


@functools.lru_cache(maxsize=None)
def nn_case(m, n, k):
    gen, r = _gen(m, n, k, 1), E.radius(k)
    E.check_operands(k, r, r, PRE_R)
    g, w, pre = E.integers((m, k), r, gen), E.integers((k, n), r, gen), E.integers((m, n), PRE_R, gen)
    y = E.gemm_ref(g, w, "NN")
    return dict(g=g, w=w, pre=pre, y=y, y_pre=y * pre.double())


@functools.lru_cache(maxsize=None)
def tn_case(m, n, k):
    gen, r = _gen(m, n, k, 2), E.radius(k)
    E.check_operands(k, r, r)
    g, x = E.integers((k, m), r, gen), E.integers((k, n), r, gen)
    return dict(g=g, x=x, dw=E.exact_f32(E.gemm_ref(g, x, "TN")), db=E.exact_f32(g.double().sum(0)))


@functools.lru_cache(maxsize=None)
def batched_case(batch, cin, cout, hw):
    """The three GEMMs of a 1x1 convolution on NCHW tensors; the weight gradient contracts over batch * hw."""
    gen, r = _gen(batch, cin, cout, hw), E.radius(max(cin, cout, batch * hw))
    E.check_operands(max(cin, cout, batch * hw), r, r)
    x, w, gy = E.integers((batch, cin, hw), r, gen), E.integers((cout, cin), r, gen), E.integers((batch, cout, hw), r, gen)
    return dict(x=x, w=w, gy=gy, y=torch.einsum("oi,bip->bop", w.double(), x.double()),
                dx=torch.einsum("oi,bop->bip", w.double(), gy.double()), dw=torch.einsum("bop,bip->oi", gy.double(), x.double()))


@functools.lru_cache(maxsize=None)
def strided_case():
    gen, r = _gen(512, 2304), E.radius(768)
    E.check_operands(768, r, r)
    return dict(qkv=E.integers((512, 2304), r, gen), w=E.integers((768, 768), r, gen))


def bf16_output_references():
    """(label, float64 reference) of every bf16-output case of this file, for the rounding-path conditions."""
    for m, n, k in NT_CASES + G256_CASES:
        c = nt_case(m, n, k)
        for name in ("y", "y_bias") + (("y_pre",) if (m, n, k) in G256_CASES else ()):
            yield f"gemm NT {(m, n, k)} {name}", c[name]
    for m, n, k in NN_CASES:
        c = nn_case(m, n, k)
        for name in ("y", "y_pre"):
            yield f"gemm NN {(m, n, k)} {name}", c[name]
    for case in BATCHED_CASES:
        c = batched_case(*case)
        for name in ("y", "dx"):
            yield f"gemm batched {case} {name}", c[name]
    c = strided_case()
    for c0 in (0, 768, 1536):
        yield f"gemm strided views, columns from {c0}", E.gemm_ref(c["qkv"][:, c0:c0 + 768], c["w"], "NT")


@pytest.mark.parametrize("tile", [0, 1, 2, 3, 4, 5, 6, 7, 8])
@pytest.mark.parametrize("m,n,k", NT_CASES)
def test_gemm_nt_exact(device, m, n, k, tile):
    """x W^T with the exact epilogues: none, bias (one parameter and query | key | value segments), fp32, bias + residual with
    dropout off; whole and ragged tiles of every plan (tile 8, 128 x 96, exists for this layout only)."""
    import sis_hip as S
    c = nt_case(m, n, k)
    xd, wd, bd, rd = (c[name].to(device) for name in ("x", "w", "bias", "resid"))
    what = f"NT {(m, n, k)} tile {tile}"
    box = (128, 96 if tile == 8 else 128)
    E.assert_bitwise(S.gemm_bf16(xd, wd, S.GEMM_NT, S.EPI_NONE, tile=tile), E.expected_bf16(c["y"]), what + " EPI_NONE", box)
    want = E.expected_bf16(c["y_bias"])
    E.assert_bitwise(S.gemm_bf16(xd, wd, S.GEMM_NT, S.EPI_BIAS, bias=bd, tile=tile), want, what + " EPI_BIAS", box)
    if n % 12 == 0:
        seg = n // 3
        b3 = tuple(bd[i * seg:(i + 1) * seg].contiguous() for i in range(3))
        E.assert_bitwise(S.gemm_bf16(xd, wd, S.GEMM_NT, S.EPI_BIAS, bias=b3, tile=tile), want, what + " EPI_BIAS, three segments", box)
    E.assert_bitwise(S.gemm_bf16(xd, wd, S.GEMM_NT, S.EPI_F32, tile=tile), E.exact_f32(c["y"]), what + " EPI_F32", box)
    res = S.gemm_bf16(xd, wd, S.GEMM_NT, S.EPI_BIAS_DROP_RESID, bias=bd, resid=rd, drop_p=0.0, tile=tile)
    E.assert_bitwise(res, E.exact_f32(c["y_resid"]), what + " EPI_BIAS_DROP_RESID", box)


@pytest.mark.parametrize("tile", [0, 1, 2, 3, 4, 5, 6, 7])
@pytest.mark.parametrize("m,n,k", NN_CASES)
def test_gemm_nn_exact(device, m, n, k, tile):
    """g W (the data gradient, W read K-major) and its EPI_GELU_BWD form: the product times an integer factor stays exact, the
    output is its RNE image."""
    import sis_hip as S
    c = nn_case(m, n, k)
    gd, wd, pd = (c[name].to(device) for name in ("g", "w", "pre"))
    what = f"NN {(m, n, k)} tile {tile}"
    E.assert_bitwise(S.gemm_bf16(gd, wd, S.GEMM_NN, S.EPI_NONE, tile=tile), E.expected_bf16(c["y"]), what + " EPI_NONE", (128, 128))
    E.assert_bitwise(S.gemm_bf16(gd, wd, S.GEMM_NN, S.EPI_GELU_BWD, pre=pd, tile=tile), E.expected_bf16(c["y_pre"]), what + " EPI_GELU_BWD",
                     (128, 128))


@pytest.mark.parametrize("tile", [0, 1, 2, 3, 4, 5, 6, 7])
@pytest.mark.parametrize("m,n,k,splits", TN_CASES)
def test_gemm_tn_split_k_exact(device, m, n, k, splits, tile):
    """g^T x (the weight gradient) is the exact product for every split count, hence bitwise one result across split counts;
    token counts that are no multiple of the K step, slice counts that step down."""
    import sis_hip as S
    c = tn_case(m, n, k)
    gd, xd = c["g"].to(device), c["x"].to(device)
    for s in sorted({1, 2, splits}):
        E.assert_bitwise(S.gemm_bf16(gd, xd, S.GEMM_TN, S.EPI_F32, splits=s, tile=tile), c["dw"], f"TN {(m, n, k)} tile {tile} splits {s}",
                         (128, 128))


@pytest.mark.parametrize("tile", [0, 4, 6])
@pytest.mark.parametrize("m,n,k,splits", WGRAD_BIAS_CASES)
def test_gemm_wgrad_bias_exact(device, m, n, k, splits, tile):
    """sis_gemm_bf16_wgrad_bias: dW and the bias gradient (column sums by extra workgroups of the same launches) are exact."""
    import sis_hip as S
    c = tn_case(m, n, k)
    dw, db = S.gemm_bf16_wgrad_bias(c["g"].to(device), c["x"].to(device), splits, tile)
    E.assert_bitwise(dw, c["dw"], f"wgrad_bias {(m, n, k, splits)} tile {tile} dW", (128, 128))
    E.assert_bitwise(db, c["db"], f"wgrad_bias {(m, n, k, splits)} tile {tile} db", 256)


@pytest.mark.parametrize("jobs,tile", [(3, None), (17, None), (3, 0), (3, 6)])
@pytest.mark.parametrize("m,n,k", WGRAD_MULTI_CASES)
def test_gemm_wgrad_bias_multi_exact(device, m, n, k, jobs, tile):
    """The pointer-table form (one launch per 16 layers of one shape, every tile contracts all tokens): every job's dW and db are
    exact; 17 jobs take a second launch."""
    import sis_hip as S
    gen, r = _gen(m, n, k, jobs), E.radius(k)
    E.check_operands(k, r, r)
    gs, xs = [E.integers((k, m), r, gen) for _ in range(jobs)], [E.integers((k, n), r, gen) for _ in range(jobs)]
    table = [(g.to(device), x.to(device), torch.empty(m, n, device=device), torch.empty(m, device=device)) for g, x in zip(gs, xs)]
    S.gemm_bf16_wgrad_bias_multi(table, tile)
    for j, (g, x) in enumerate(zip(gs, xs)):
        E.assert_bitwise(table[j][2], E.exact_f32(E.gemm_ref(g, x, "TN")), f"wgrad_bias_multi {(m, n, k)} job {j} of {jobs} dW", (128, 128))
        E.assert_bitwise(table[j][3], E.exact_f32(g.double().sum(0)), f"wgrad_bias_multi {(m, n, k)} job {j} of {jobs} db", 256)


@pytest.mark.parametrize("rows,n,dtype,r", COLUMN_SUM_CASES)
def test_column_sum_exact(device, rows, n, dtype, r):
    import sis_hip as S
    E.check_operands(rows, r, 1)
    x = E.integers((rows, n), r, _gen(rows, n), dtype=dtype)
    E.assert_bitwise(S.column_sum(x.to(device)), E.exact_f32(x.double().sum(0)), f"column_sum {(rows, n)} {dtype}", 256)


@pytest.mark.parametrize("tile", [9, 10, 11])
@pytest.mark.parametrize("m,n,k", G256_CASES)
def test_gemm256_exact(device, m, n, k, tile):
    """The 256-row tiles: the exact epilogues of the NT case plus EPI_GELU_BWD (EPI_F32 is not theirs: ``sis_gemm256_ok``
    declines it); bitwise the exact result, and therefore bitwise tile 0's."""
    import sis_hip as S
    c = nt_case(m, n, k)
    xd, wd, bd, rd, pd = (c[name].to(device) for name in ("x", "w", "bias", "resid", "pre"))
    what = f"gemm256 {(m, n, k)} tile {tile}"
    box = (256, (96, 192, 288)[tile - 9])
    E.assert_bitwise(S.gemm_bf16(xd, wd, S.GEMM_NT, S.EPI_NONE, tile=tile), E.expected_bf16(c["y"]), what + " EPI_NONE", box)
    want = E.expected_bf16(c["y_bias"])
    got = S.gemm_bf16(xd, wd, S.GEMM_NT, S.EPI_BIAS, bias=bd, tile=tile)
    E.assert_bitwise(got, want, what + " EPI_BIAS", box)
    assert torch.equal(got, S.gemm_bf16(xd, wd, S.GEMM_NT, S.EPI_BIAS, bias=bd, tile=0))
    if n % 12 == 0:
        seg = n // 3
        b3 = tuple(bd[i * seg:(i + 1) * seg].contiguous() for i in range(3))
        E.assert_bitwise(S.gemm_bf16(xd, wd, S.GEMM_NT, S.EPI_BIAS, bias=b3, tile=tile), want, what + " EPI_BIAS, three segments", box)
    res = S.gemm_bf16(xd, wd, S.GEMM_NT, S.EPI_BIAS_DROP_RESID, bias=bd, resid=rd, drop_p=0.0, tile=tile)
    E.assert_bitwise(res, E.exact_f32(c["y_resid"]), what + " EPI_BIAS_DROP_RESID", box)
    E.assert_bitwise(S.gemm_bf16(xd, wd, S.GEMM_NT, S.EPI_GELU_BWD, pre=pd, tile=tile), E.expected_bf16(c["y_pre"]), what + " EPI_GELU_BWD", box)


@pytest.mark.parametrize("batch,cin,cout,hw", BATCHED_CASES)
def test_gemm_batched_exact(device, batch, cin, cout, hw):
    """sis_gemm_bf16_batched as a 1x1 convolution: forward (NN), data gradient (TN), weight gradient (NT, summed over the batch
    entries in fp32: exact)."""
    import sis_hip as S
    c = batched_case(batch, cin, cout, hw)
    xd, wd, gd = c["x"].to(device), c["w"].to(device), c["gy"].to(device)
    what = f"batched {(batch, cin, cout, hw)}"
    E.assert_bitwise(S.gemm_bf16_batched(wd, xd, S.GEMM_NN), E.expected_bf16(c["y"]), what + " NN", (128, 128))
    E.assert_bitwise(S.gemm_bf16_batched(wd, gd, S.GEMM_TN), E.expected_bf16(c["dx"]), what + " TN", (128, 128))
    dw = S.gemm_bf16_batched(gd, xd, S.GEMM_NT, S.EPI_F32, sum_over_batches=True)
    E.assert_bitwise(dw, E.exact_f32(c["dw"]), what + " NT summed over the batch", (128, 128))


def test_gemm_strided_views_exact(device):
    """The q | k | v column blocks of one fused-projection matrix as row-strided operands, NT and split-K TN."""
    import sis_hip as S
    c = strided_case()
    qd, wd = c["qkv"].to(device), c["w"].to(device)
    E.check_operands(512, E.radius(768), E.radius(768))
    for c0 in (0, 768, 1536):
        block = c["qkv"][:, c0:c0 + 768]
        E.assert_bitwise(S.gemm_bf16(qd[:, c0:c0 + 768], wd, S.GEMM_NT), E.expected_bf16(E.gemm_ref(block, c["w"], "NT")),
                         f"NT on columns from {c0}", (128, 128))
        E.assert_bitwise(S.gemm_bf16(qd[:, c0:c0 + 768], qd[:, :768], S.GEMM_TN, S.EPI_F32, splits=2),
                         E.exact_f32(E.gemm_ref(block, c["qkv"][:, :768], "TN")), f"TN on columns from {c0}", (128, 128))


# ---- the one epilogue that is not exactly summable

GELU_A = 6e-7     # four times the 1.5e-7 csrc/vit_common.h documents for its Abramowitz-Stegun 7.1.26 erf


@functools.lru_cache(maxsize=None)
def gelu_case():
    m, n, k = GELU_CASE
    gen, r = _gen(m, n, k, 3), 15
    E.check_operands(k, r, r, 2)
    x, w = E.integers((m, k), r, gen), E.integers((n, k), r, gen, shift=10)
    bias = E.integers((n,), BIAS_R, gen, shift=10, dtype=torch.float32)
    h = E.check_reference(E.gemm_ref(x, w, "NT") + bias.double(), unit=2.0 ** -10)   # the pre-activation, known exactly
    cdf = 0.5 * (1 + torch.erf(h / math.sqrt(2)))
    pdf = torch.exp(-0.5 * h * h) / math.sqrt(2 * math.pi)
    return dict(x=x, w=w, bias=bias, h=h, gelu=h * cdf, gelu_grad=cdf + h * pdf)


@pytest.mark.parametrize("tile", [0, 4, 9, 10])
def test_gelu_epilogue_per_element(device, tile, capsys):
    """EPI_BIAS_GELU_DROP with dropout off.  The pre-activation h is exact (integers times 2^-10, h in about [-4.5, 4], standard
    deviation 1.08), so both outputs are bounded PER ELEMENT around the float64 values:
        |got - f(h)| <= 2^-8 |f(h)| + A max(1, |h|),   f = gelu, gelu'
    one bf16 ulp plus the kernel's own approximation; A = 6e-7 is four times the bound documented for the erf approximation.
    The largest deviation beyond the ulp term, in units of max(1, |h|), is printed before the assertion.
    Measured on one MI355X, tiles 0, 4, 9 and 10 alike: 3.3e-10 for gelu, 0 for gelu' (largest |err| 1.56e-2 and 3.9e-3, all of
    it the output rounding), so A = 6e-7 stands as derived, with room."""
    import sis_hip as S
    c = gelu_case()
    out, dact = S.gemm_bf16(c["x"].to(device), c["w"].to(device), S.GEMM_NT, S.EPI_BIAS_GELU_DROP, bias=c["bias"].to(device), drop_p=0.0, tile=tile)
    h = c["h"]
    assert -6 < float(h.min()) < -3 and 3 < float(h.max()) < 6 and 0.9 < float(h.std()) < 1.3
    scale = h.abs().clamp(min=1.0)
    for name, got, want in (("gelu", out, c["gelu"]), ("gelu'", dact, c["gelu_grad"])):
        err = (got.double().cpu() - want).abs()
        beyond_ulp = ((err - 2.0 ** -8 * want.abs()).clamp(min=0) / scale).max().item()
        with capsys.disabled():
            print(f"\n[gelu epilogue] tile {tile} {name}: max (|err| - 2^-8 |f|)+ / max(1, |h|) = {beyond_ulp:.3e}, max |err| = {err.max().item():.3e}")
        bad = err > 2.0 ** -8 * want.abs() + GELU_A * scale
        assert not bool(bad.any()), (name, tile, int(bad.sum()), beyond_ulp)
