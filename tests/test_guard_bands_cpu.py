"""The guard-band harness (tests/guard_bands.py) checked on CPU tensors, and the coverage rule: every ``csrc/*.hip`` file has a
guarded case in tests/test_guard_bands_gpu.py, or a reasoned exemption here."""
import glob
import os

import pytest
import torch

import guard_bands as G

CPU = torch.device("cpu")


@pytest.fixture(autouse=True)
def _fresh_session():
    G.reset()
    yield
    G.reset()


def _past(view, elements):
    """The element ``elements`` places past the end (or, negative, before the start) of a banded view, same raw buffer."""
    off = view.storage_offset() + (view.numel() - 1 + elements if elements > 0 else elements)
    return view.as_strided((1,), (1,), off)


def test_placement():
    t = torch.arange(15, dtype=torch.float32).view(3, 5)
    v = G.banded(t, CPU)
    assert v.shape == t.shape and v.dtype == t.dtype and v.is_contiguous() and torch.equal(v, t)
    assert v.data_ptr() % G.ALIGN == 0
    buf = G._session.buffers[0]
    assert buf.nbytes == 60 and G.BAND_BYTES == 2 << 20
    before, after = buf.raw[:buf.start], buf.raw[buf.start + buf.nbytes:]
    assert before.numel() >= G.BAND_BYTES and after.numel() >= G.BAND_BYTES
    assert bool((before == 0xFF).all()) and bool((after == 0xFF).all())
    assert buf.raw.data_ptr() + buf.start + buf.nbytes == after.data_ptr()   # the trailing band starts at the first byte after
    G.check()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16, torch.float64])
def test_fill_is_nan_in_every_float_type(dtype):
    assert torch.isnan(torch.full((8,), 0xFF, dtype=torch.uint8).view(dtype)).all()


def test_fill_as_integers():
    raw = torch.full((8,), 0xFF, dtype=torch.uint8)
    assert raw.view(torch.int32).tolist() == [-1, -1] and raw.view(torch.int64).tolist() == [-1] and raw[0].item() == 255


def test_proxy_allocations(monkeypatch):
    import sis_hip
    with G.guarded(monkeypatch, CPU) as session:
        assert sis_hip.torch.float32 is torch.float32
        out = sis_hip._out_or_new(None, (3, 5, 7), CPU, "test")
        assert isinstance(out, sis_hip.torch.Tensor) and out.dtype == torch.float32 and tuple(out.shape) == (3, 5, 7)
        assert out.is_contiguous() and out.data_ptr() % 16 == 0 and torch.isnan(out).all()
        z = sis_hip.torch.zeros(5, dtype=torch.int32, device=CPU)
        assert z.tolist() == [0] * 5
        like = sis_hip.torch.empty_like(z)
        assert like.tolist() == [-1] * 5
        zl = sis_hip.torch.zeros_like(out, dtype=torch.bfloat16)
        assert zl.dtype == torch.bfloat16 and zl.shape == out.shape and not zl.any()
        assert len(session.buffers) == 4
        assert [b.kind for b in session.buffers] == ["empty", "zeros", "empty", "zeros"]
        assert all("test_guard_bands_cpu.py" in b.site or "__init__.py" in b.site for b in session.buffers)
    assert sis_hip.torch is torch
    G.check()


def test_caches_are_emptied_and_restored(monkeypatch):
    import sis_hip
    marker = torch.zeros(1)
    monkeypatch.setitem(sis_hip._workspaces, "marker", marker)
    monkeypatch.setitem(sis_hip._GROUP_COUNTERS, "marker", marker)
    before = sis_hip.WORKSPACE_BYTES
    with G.guarded(monkeypatch, CPU, workspace_bytes=4096):
        assert not sis_hip._workspaces and not sis_hip._GROUP_COUNTERS and not sis_hip._drop_seeds
        assert sis_hip.WORKSPACE_BYTES == 4096
        ws = sis_hip._workspace(CPU)
        assert ws.numel() == 4096 and bool((ws == 0xFF).all())
    assert sis_hip._workspaces["marker"] is marker and list(sis_hip._workspaces) == ["marker"]
    assert sis_hip._GROUP_COUNTERS["marker"] is marker and sis_hip.WORKSPACE_BYTES == before
    G.check()


def test_write_one_byte_before_the_view_fails():
    v = G.banded(torch.zeros(4, 6, dtype=torch.uint8), CPU)
    _past(v, -1).fill_(7)
    with pytest.raises(AssertionError, match=r"band before the view changed, first at byte offset -1 "):
        G.check()


def test_write_one_byte_after_the_view_fails(monkeypatch):
    import sis_hip
    with G.guarded(monkeypatch, CPU):
        v = sis_hip.torch.empty((4, 6), dtype=torch.uint8, device=CPU)
    _past(v, 1).fill_(7)
    with pytest.raises(AssertionError, match=r"empty from test_guard_bands_cpu.py:\d+ .*band after the view changed, first at byte offset 24 "):
        G.check()


def test_changed_input_element_fails():
    v = G.banded(torch.ones(3, 3, dtype=torch.int32), CPU)
    v[1, 1] = 2
    with pytest.raises(AssertionError, match="interior changed, first at byte offset 16"):
        G.check()


def test_empty_like_of_a_non_dense_tensor_is_counted(monkeypatch):
    import sis_hip
    with G.guarded(monkeypatch, CPU):
        dense = sis_hip.torch.empty((4, 6), dtype=torch.float32, device=CPU)
        out = sis_hip.torch.empty_like(dense.t())
    assert tuple(out.shape) == (6, 4)
    with pytest.raises(AssertionError, match="1 unguarded allocation"):
        G.check()


# ---- fake ops, allocating through the same sis_hip.torch proxy as the wrappers

def _fake_scale(x, weights, read_past=0, skip_last=False):
    """out[i] = sum_k weights[k] * x[i + k]; ``read_past``: a zero-weight tap that many elements past the end of x."""
    import sis_hip
    out = sis_hip.torch.empty_like(x)
    n = x.numel()
    flat = x.as_strided((n + read_past,), (1,), x.storage_offset())
    acc = flat[:n] * weights[0]
    if read_past:
        acc = acc + 0.0 * flat[read_past:n + read_past]
    m = n - 1 if skip_last else n
    out.view(-1)[:m] = acc[:m]
    return out


@pytest.mark.parametrize("fault,nan", [({}, False), ({"read_past": 1}, True), ({"skip_last": True}, True)])
def test_fake_ops_show_as_nan(monkeypatch, fault, nan):
    """A read one element past the input times zero, and one unwritten output element, are NaN in the result; the clean twin
    has none.  Neither touches a band: this is the caller's parity assertion, not ``check()``."""
    x = G.banded(torch.arange(1.0, 13.0), CPU)
    with G.guarded(monkeypatch, CPU):
        y = _fake_scale(x, [2.0], **fault)
    G.check()
    assert bool(torch.isnan(y).any()) == nan
    if not nan:
        assert torch.equal(y, 2 * torch.arange(1.0, 13.0))


# ---- coverage

EXEMPT = {
    "sis_core.hip": "no kernels: version, last-error and last-kernel strings",
}


def test_every_kernel_file_has_a_guarded_case():
    import test_guard_bands_gpu as cases
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    files = sorted(os.path.basename(p) for p in glob.glob(os.path.join(root, "synthesis-in-style_amd", "csrc", "*.hip")))
    assert len(files) > 30
    covered = {f for c in cases.CASES for f in c.files}
    assert covered <= set(files), sorted(covered - set(files))
    assert all(c.files for c in cases.CASES)
    assert all(EXEMPT.values()) and set(EXEMPT) <= set(files) and not (set(EXEMPT) & covered)
    missing = [f for f in files if f not in covered and f not in EXEMPT]
    assert not missing, f"no guarded case in tests/test_guard_bands_gpu.py for {missing}"
    names = [c.name for c in cases.CASES]
    assert len(set(names)) == len(names)
