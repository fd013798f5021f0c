"""modconv_bf16_kernel (csrc/modconv_bf16.h): operand rounding against the emulation of tests/modconv_bf16_checks.py (bound and
its derivation there; tests/test_modconv_bf16_cpu.py shows from the reference alone that the bound sees five rounding defects),
declined shapes, batch independence, the profiler record, and the generator's precision switch.

The deviation of a bf16 image from the fp32 image is measured by tools/bench_gen_bf16.py (profiles/gen_bf16.json) and is not
asserted here."""
import functools

import pytest
import torch

import modconv_bf16_checks as M
from oracle import stylegan2_ref as R

pytestmark = pytest.mark.gpu

KERNEL = "modconv_bf16_kernel"

# randn operands at cin <= 40 only: at K = 4608 the worst-case bound no longer separates the rounding defects
SHAPES = [(2, 16, 64, 32, 32),     # one chunk of 16 channels, 64-channel tile, whole 8 x 32 tiles
          (1, 40, 192, 24, 40),    # half-empty last chunk, ragged 128-channel tile, 4 x 64 tiles partial in W
          (3, 8, 128, 10, 72)]     # half a chunk in all, partial tiles in H and in W, three samples


@functools.lru_cache(maxsize=None)
def _layer(b, cin, cout, h, w):
    """Operands, emulation and bound of one layer; computed once, shared, never modified."""
    L = M.operands(b, cin, cout, h, w)
    L["y"], L["bound"] = M.emulate(L["x"], L["w"], L["s"], L["dscale"])
    L["y_act"] = M.tail64(L["y"], L["noise"], L["nw"], L["bias"])
    L["bound_act"] = M.tail_bound(L["y"], L["bound"], L["noise"], L["nw"], L["bias"])
    return L


def _run(device, L, fuse, sl=slice(None), **kw):
    import sis_hip
    d = lambda t: t.to(device)
    wpk, _ = sis_hip.modconv_prepack(d(L["w"]).unsqueeze(0))
    y = sis_hip.modconv2d(d(L["x"][sl]), wpk, d(L["s"][sl]).contiguous(), d(L["dscale"][sl]).contiguous(), 3, d(L["noise"]) if fuse else None,
                          d(L["nw"]) if fuse else None, d(L["bias"]) if fuse else None, fuse_act=fuse, **kw)
    torch.cuda.synchronize()
    return y, sis_hip.lib().sis_last_kernel().decode()


@pytest.mark.parametrize("fuse", [False, True])
@pytest.mark.parametrize("b,cin,cout,h,w", SHAPES)
def test_operand_rounding(device, b, cin, cout, h, w, fuse):
    import sis_hip
    L = _layer(b, cin, cout, h, w)
    assert sis_hip.modconv_bf16_eligible(cin, cout, h, w)
    y, name = _run(device, L, fuse, bf16_w=sis_hip.modconv_prepack_bf16(L["w"].to(device).unsqueeze(0)))
    share, worst = M.over_bound_share(y.cpu(), L["y_act"] if fuse else L["y"], L["bound_act"] if fuse else L["bound"])
    print(f"modconv_bf16 B{b} {cin}->{cout} {h}x{w} fuse={int(fuse)}: worst error / bound = {worst:.4f}")
    assert name == KERNEL
    assert share == 0.0, (share, worst)


DECLINED = [(2, 16, 64, 16, 16),   # narrower than a tile row
            (2, 16, 32, 32, 32),   # Cout % 64
            (1, 16, 64, 32, 34)]   # W % 4


@pytest.mark.parametrize("b,cin,cout,h,w", DECLINED)
def test_declined_shapes_take_the_path_they_took(device, b, cin, cout, h, w):
    import sis_hip
    L = _layer(b, cin, cout, h, w)
    assert not sis_hip.modconv_bf16_eligible(cin, cout, h, w)
    packed = sis_hip.modconv_prepack_bf16(torch.randn(1, 64, 16, 3, 3, device=device))   # any image: it must not be read
    u16 = sis_hip.modconv_prepack_wino(L["w"].to(device).unsqueeze(0))
    for kw in ({}, {"wino_u": u16}):
        y, name = _run(device, L, True, bf16_w=packed, **kw)
        y0, name0 = _run(device, L, True, **kw)
        assert name == name0 and KERNEL not in name and torch.equal(y, y0)


def test_batch_independence(device):
    """Samples 2:4 of a B = 6 call against a B = 2 call on those samples: the same bits; so are B = 1, 4, 32, 33 calls on one
    repeated sample.  The eligibility query has no batch argument."""
    import sis_hip
    L = _layer(6, 16, 64, 12, 40)
    packed = sis_hip.modconv_prepack_bf16(L["w"].to(device).unsqueeze(0))
    y6, name = _run(device, L, True, bf16_w=packed)
    y2, name2 = _run(device, L, True, sl=slice(2, 4), bf16_w=packed)
    assert name == KERNEL and name2 == KERNEL and torch.equal(y6[2:4], y2)
    one = dict(L, x=L["x"][:1], s=L["s"][:1], dscale=L["dscale"][:1])
    for b in (1, 4, 32, 33):
        rep = dict(one, x=one["x"].expand(b, -1, -1, -1).contiguous(), s=one["s"].expand(b, -1).contiguous(),
                   dscale=one["dscale"].expand(b, -1).contiguous())
        yb, nameb = _run(device, rep, True, bf16_w=packed)
        assert nameb == KERNEL and torch.equal(yb[b - 1], y6[0]) and torch.equal(yb[0], y6[0])


def test_profiler_record_names_the_kernel(device):
    import sis_hip
    b, cin, cout, h, w = SHAPES[0]
    L = _layer(b, cin, cout, h, w)
    packed = sis_hip.modconv_prepack_bf16(L["w"].to(device).unsqueeze(0))
    rec = []
    sis_hip.set_profiler(rec)
    try:
        _run(device, L, True, bf16_w=packed)
        _run(device, _layer(*DECLINED[0]), True, bf16_w=packed)
    finally:
        sis_hip.set_profiler(None)
    convs = [r for r in rec if "modconv" in r[0] and "prepack" not in r[0]]
    assert len(convs) == 2 and convs[0][0] == KERNEL and KERNEL not in convs[1][0]
    assert convs[0][1] == 2.0 * b * cout * cin * 9 * h * w                              # direct form
    assert convs[0][2] == 4.0 * (b * cin * h * w + b * cout * h * w) + 2.0 * packed.numel()    # fp32 maps, bf16 weight image


# ---- the generator's switch: Generator(64, 512, 8, 2) at B = 2

def _forward(device, precision=None, want_latent=False):
    import sis_hip
    from networks.stylegan2.model import Generator
    sd = R.seeded_state_dict(64, 512, 8, 2, seed=21)
    z, noise = R.seeded_inputs(64, 2, 512, seed=22)
    g = Generator(64, 512, 8, channel_multiplier=2)
    g.load_state_dict(sd, strict=True)
    g = g.to(device).eval()
    if precision is not None:
        g.set_matrix_precision(precision)
    noise = [n.to(device) for n in noise]
    rec = []
    sis_hip.set_profiler(rec)
    try:
        with torch.no_grad():
            img, acts = g([z.to(device)], noise=noise, return_intermediate_activations=True)
        torch.cuda.synchronize()
    finally:
        sis_hip.set_profiler(None)
    return g, img, acts, [r[0] for r in rec], z.to(device), noise


def test_generator_fp32_mode_never_launches_the_kernel(device, monkeypatch):
    monkeypatch.delenv("SIS_GEN_PRECISION", raising=False)
    _, img, acts, names, _, _ = _forward(device)
    monkeypatch.setenv("SIS_GEN_PRECISION", "fp32")
    _, img1, acts1, names1, _, _ = _forward(device)
    assert KERNEL not in names and KERNEL not in names1 and names == names1
    assert torch.equal(img, img1) and all(torch.equal(acts[k], acts1[k]) for k in acts)


@pytest.mark.parametrize("how", ["environment", "method"])
def test_generator_bf16_mode(device, monkeypatch, how):
    monkeypatch.delenv("SIS_GEN_PRECISION", raising=False)
    _, img0, acts0, names0, _, _ = _forward(device)
    if how == "environment":
        monkeypatch.setenv("SIS_GEN_PRECISION", "bf16")
    g, img, acts, names, z, noise = _forward(device, "bf16" if how == "method" else None)
    assert names.count(KERNEL) == 2 and KERNEL not in names0            # the stride-1 3x3 layers at 32^2 and 64^2
    assert bool(torch.isfinite(img).all()) and all(bool(torch.isfinite(a).all()) for a in acts.values())
    # activation 7 is the 32^2 layer's, 9 the 64^2 layer's (0: the constant, 1: conv1, then up / conv per resolution)
    for k in range(7):
        assert torch.equal(acts[k], acts0[k]), k
    with torch.no_grad():
        _, latent = g([z], noise=noise, return_latents=True)
        s, d = g._modulate_all(latent)
    for r, k in ((2, 7), (3, 9)):
        layer, j = g.convs[2 * r + 1], 2 + 3 * r
        conv = layer.conv
        assert conv.bf16_takes(*acts[k].shape[2:])
        x = acts[k - 1]
        xm = M.rne(M.modulated(x, s[j + 1])).to(device)                # rounded on the CPU by the pinned helper
        y, bound = M.emulate(x, conv.weight[0].detach(), s[j + 1], d[j + 1], x_op=xm, w_op=M.rne(conv.weight[0]).to(device))
        nz, nw, bias = noise[2 + 2 * r], float(layer.noise.weight.detach()), layer.activate.bias.detach()
        share, worst = M.over_bound_share(acts[k], M.tail64(y, nz, nw, bias), M.tail_bound(y, bound, nz, nw, bias))
        print(f"Generator(64) {how}: activation {k}: worst error / bound = {worst:.4f}")
        assert share == 0.0, (k, share, worst)
