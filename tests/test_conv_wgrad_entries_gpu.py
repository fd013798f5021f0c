"""GPU: a convolution weight-gradient family's single-layer C entry, its ``_multi`` entry with one job and its public binding
called immediately return the same bits.  The binding launches through the ``_multi`` entries only (immediate: one job; queued:
the layers of a shape), and the single-layer entries forward to them: the plan for one job is the plan of the single layer and
the kernels add in a fixed order, so equality is bitwise -- no tolerance.  Shapes (batch, cin, cout, h, w): the smallest of the
families' own tests that reach each kernel form (unaligned maps, more than one K slice, both dW dtypes of the bf16 kernels).
What these launches compute is held to float64 elsewhere: the fp32 families bit for bit in test_conv_f32_exact_gpu.py, the bf16
families in test_conv_bf16_exact_gpu.py."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
CASES = {"f3": [((1, 128, 64, 16, 16), F32), ((4, 128, 64, 6, 20), F32)],
         "f1": [((1, 64, 128, 8, 8), F32), ((5, 192, 384, 8, 16), F32)],   # one K slice (no workspace) / five
         3: [((1, 16, 16, 8, 256), F32), ((1, 16, 16, 8, 256), BF16), ((1, 64, 64, 31, 33), F32)],   # ... the unaligned kernel form
         1: [((2, 72, 40, 20, 28), F32), ((2, 72, 40, 20, 28), BF16), ((1, 64, 64, 31, 33), F32)]}


@pytest.mark.parametrize("kind", list(CASES), ids=str)
def test_single_entry_multi_entry_and_binding_agree(device, kind):
    for shape, dw_dtype in CASES[kind]:
        _three_ways(device, kind, shape, dw_dtype)


def _three_ways(device, kind, shape, dw_dtype):
    import sis_hip
    L = sis_hip.lib()
    batch, cin, cout, h, w = shape
    gen = torch.Generator().manual_seed(batch * 7 + cin + cout + h)
    op_dtype = F32 if kind in ("f3", "f1") else BF16
    x = torch.randn(batch, cin, h, w, generator=gen).to(device, op_dtype)
    gy = torch.randn(batch, cout, h, w, generator=gen).to(device, op_dtype)
    k = 3 if kind in ("f3", 3) else 1

    # per family: capability, C entries (single, multi), operands behind dW, leading dW dtype code, shape arguments, the binding
    if kind == "f3":
        assert sis_hip.conv3x3_wgrad_supported(batch, cin, cout, h, w)
        single, multi, ops, code, dims = L.sis_conv3x3_wgrad, L.sis_conv3x3_wgrad_multi, (x, gy), (), (batch, cin, cout, h, w)
        bound = sis_hip.conv3x3_wgrad(x, gy)
    elif kind == "f1":
        assert sis_hip.conv1x1_wgrad_f32_supported(gy, x)
        single, multi, ops, code, dims = L.sis_conv1x1_wgrad_f32, L.sis_conv1x1_wgrad_f32_multi, (gy, x), (), (batch, cin, cout, h * w)
        bound = sis_hip.conv1x1_wgrad_f32(gy, x)
    elif kind == 3:
        assert sis_hip.conv_bf16_wgrad_supported(batch, cin, cout, h, w)
        single, multi, ops, code, dims = L.sis_conv_bf16_wgrad, L.sis_conv_bf16_wgrad_multi, (x, gy), (sis_hip._DTYPE_CODE[dw_dtype],), (batch, cin, cout, h, w)
        bound = sis_hip.conv_bf16_wgrad(x, gy, dw_dtype)
    else:
        assert sis_hip.conv1x1_bf16_wgrad_supported(batch, cin, cout, h * w)
        single, multi, ops, code, dims = (L.sis_conv1x1_bf16_wgrad, L.sis_conv1x1_bf16_wgrad_multi, (x, gy), (sis_hip._DTYPE_CODE[dw_dtype],),
                                         (batch, cin, cout, h * w))
        bound = sis_hip.conv1x1_bf16_wgrad(x, gy, dw_dtype)

    if kind == "f1":   # a scratch of exactly the planned slabs; none for a single K slice
        ws_bytes = int(L.sis_conv1x1_wgrad_f32_workspace(batch, cin, cout, h * w))
        assert (ws_bytes > 0) == (shape == (5, 192, 384, 8, 16))
        ws = torch.empty(ws_bytes // 4, dtype=F32, device=device) if ws_bytes else None
    else:
        ws = sis_hip._workspace(device)
        ws_bytes = ws.numel()

    def one(p):
        return (ctypes.c_void_p * 1)(p.data_ptr())

    dw_single = torch.full((cout, cin, k, k), float("nan"), dtype=dw_dtype, device=device)
    dw_multi = torch.full((cout, cin, k, k), float("nan"), dtype=dw_dtype, device=device)
    with torch.cuda.device(device):
        rc = single(sis_hip._ptr(dw_single), *code, sis_hip._ptr(ops[0]), sis_hip._ptr(ops[1]), *dims, sis_hip._ptr(ws), ws_bytes, sis_hip._stream())
        assert rc == 0, L.sis_last_error().decode()
        rc = multi(one(dw_multi), *code, one(ops[0]), one(ops[1]), 1, *dims, sis_hip._ptr(ws), ws_bytes, sis_hip._stream())
        assert rc == 0, L.sis_last_error().decode()
    assert bound.dtype == dw_dtype and tuple(bound.shape) == (cout, cin, k, k)
    assert not torch.isnan(dw_single.float()).any(), (shape, dw_dtype)
    assert torch.equal(dw_single, dw_multi), (shape, dw_dtype)
    assert torch.equal(dw_single, bound), (shape, dw_dtype)
