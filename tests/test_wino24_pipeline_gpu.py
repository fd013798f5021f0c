"""Workgroups of modconv_wino24_kernel (csrc/modconv_wino24.h) that walk several tiles, with the fused tail on and with shared
(1,1,H,W) and per-sample (B,1,H,W) noise: every walk must give the bits of the one-tile-per-workgroup walk -- the staging
order (which chunk's DMA is in flight under which MFMAs, which tile's style row, demodulation row and noise tile sit in LDS)
is all that differs, so a stale operand of the previous tile or a DMA piece that lands after its readers shows as a differing
bit.  The cases are the ones the tile-to-tile pipeline of DESIGN.md 3.2b was measured with (its schedule is not in the kernel:
no gain on the step); they hold for any walk.  Operands, oracle and the bound 2e-5 * max|ref| as tests/test_wino24_gpu.py."""
import functools

import pytest
import torch

from oracle import ops_ref
from test_wino24_gpu import NEW, _layer, _rel, _run

pytestmark = pytest.mark.gpu

CASES = [((4, 8, 64, 8, 64), (2, 4)),            # two chunks: the loop is nothing but "the last two chunks"; every next tile is another sample
         ((3, 16, 128, 32, 32), (2, 3, 6)),      # 16 x 32 tiles, two per sample, two output-channel blocks; next tile: same / next sample
         ((1, 24, 64, 44, 72), (2, 3, 4, 6, 12)),  # six chunks, partial tiles in H and W: the next tile's out-of-image float4 are zeros
         ((2, 512, 64, 32, 32), (2, 4)),         # 128 chunks: long loop, wrap of the weight prefetch
         ((5, 8, 64, 8, 64), (5,))]              # odd tile count per workgroup


@functools.lru_cache(maxsize=None)
def _noisy(shape, per_sample):
    """The layer of test_wino24_gpu._layer with shared or per-sample noise, and its fused-tail oracle; shared, never modified."""
    L = _layer(*shape)
    if not per_sample:
        return L
    b, _, _, h, w = shape
    noise = torch.randn(b, 1, h, w, generator=torch.Generator().manual_seed(77 + b + h))
    with torch.no_grad():
        ref_act = ops_ref.fused_leaky_relu(L["ref"] + L["nw"] * noise, L["bias"])
    return dict(L, noise=noise, ref_act=ref_act)


@functools.lru_cache(maxsize=None)
def _one_tile_walk(device, shape, per_sample):
    import sis_hip
    L = _noisy(shape, per_sample)
    u24 = sis_hip.modconv_prepack_wino24(L["weight"].to(device))
    y, name, sd = _run(device, L, True, wino24_u=u24, wino24_tiles_per_wg=1)
    assert name == NEW
    return u24, y, sd


@pytest.mark.parametrize("per_sample", [False, True], ids=["shared_noise", "per_sample_noise"])
@pytest.mark.parametrize("shape,tpw", [(s, n) for s, ns in CASES for n in ns])
def test_walk_vs_one_tile_and_oracle(device, shape, tpw, per_sample):
    L = _noisy(shape, per_sample)
    u24, y1, (s, ds) = _one_tile_walk(device, shape, per_sample)
    y, name, _ = _run(device, L, True, s=s, ds=ds, wino24_u=u24, wino24_tiles_per_wg=tpw)
    err = _rel(y, L["ref_act"])
    print(f"wino24 walk {shape} tiles_per_wg={tpw} per_sample={int(per_sample)}: {err:.3e}, equal={torch.equal(y, y1)}")
    assert name == NEW
    assert torch.equal(y, y1)
    assert err < 2e-5, err


def test_determinism(device):
    """10 launches of one walk into fresh outputs: the same bits; a race of the schedule would flicker."""
    shape = (3, 16, 128, 32, 32)
    L = _noisy(shape, True)
    u24, _, (s, ds) = _one_tile_walk(device, shape, True)
    ys = [_run(device, L, True, s=s, ds=ds, wino24_u=u24, wino24_tiles_per_wg=6)[0] for _ in range(10)]
    assert all(torch.equal(ys[0], y) for y in ys[1:])
