"""Guard bands: do the kernels stay inside their operands, results and workspaces?

The parity tests feed tensors that live in torch's caching allocator, next to finite, unrelated numbers.  A kernel that reads
one row past an operand and multiplies it by a zero weight, or that stores one row past its result, passes them.  This helper
makes both visible, deterministically, on any device (CPU included):

* ``banded(t, device)`` copies ``t`` into the middle of a larger ``uint8`` buffer and returns a contiguous view of the same shape
  and dtype.  The view starts at a multiple of 512 bytes (as allocator blocks do, so the kernels' 16-byte alignment requirements
  hold); the trailing band starts at the first byte after the last element, with no rounding up, so a 16-byte read of a partial
  last vector hits the band.  Every byte outside the view is ``0xFF``: NaN as fp32 / bf16 / fp16 / fp64, -1 as int32 / int64,
  255 as uint8 -- one fill serves every dtype.
* ``guarded(monkeypatch)`` replaces the name ``torch`` inside ``sis_hip`` with a proxy module whose ``empty`` / ``empty_like`` /
  ``zeros`` / ``zeros_like`` (on the device under test) return banded views: results, scratch and the cached split-K workspace
  are then born ``0xFF`` (``empty``) or zero (``zeros``) between two ``0xFF`` bands.  The module-level caches of device buffers
  are emptied for the region and restored afterwards, so every buffer a wrapper touches inside it is a guarded one.
* ``check()`` (after ``torch.cuda.synchronize()``) asserts that every band byte is still ``0xFF``, that every banded input is
  bit-equal to what was put in, and that no allocation escaped the guard.  A load from a band is not seen here directly: it is a
  NaN (or -1 / 255), and if it can reach a stored result the caller's parity assertion sees a non-finite value.

Limits.  The bands are ``BAND_BYTES`` (2 MiB) on each side -- more than any operand footprint a tile spans at the shapes of
tests/test_guard_bands_gpu.py (the largest is 128 rows x 1024 pixels x 4 bytes).  A store that lands FURTHER out than the band
is not seen by this harness, nor is an allocation made through a tensor method (``x.new_empty``) or by torch itself (autograd
intermediates): only the direct ``sis_hip`` wrappers are guarded.
"""
import contextlib
import os
import traceback

import torch as _torch

BAND_BYTES = 2 << 20
ALIGN = 512
FILL = 0xFF

_HERE = os.path.abspath(__file__)
# module-level caches of device buffers in sis_hip (grep "^_[A-Za-z_]* = {" there): emptied inside ``guarded``
_CACHES = ("_workspaces", "_GROUP_COUNTERS", "_drop_seeds")


HELPER_FRAMES = set()   # (file name, function name) of callers' own placement helpers: not a creation site


def _site():
    for fr in reversed(traceback.extract_stack()):
        if os.path.abspath(fr.filename) != _HERE and "contextlib" not in fr.filename \
                and (os.path.basename(fr.filename), fr.name) not in HELPER_FRAMES:
            return f"{os.path.basename(fr.filename)}:{fr.lineno} ({fr.name})"
    return "?"


def _same_device(a, b):
    a, b = _torch.device(a), _torch.device(b)
    if a.type != b.type:
        return False
    if a.type != "cuda":
        return True
    cur = _torch.cuda.current_device() if _torch.cuda.is_available() else 0
    return (cur if a.index is None else a.index) == (cur if b.index is None else b.index)


class _Buffer:
    """One raw uint8 allocation: [leading band | interior | trailing band]."""

    def __init__(self, shape, dtype, device, interior, site, kind):
        shape = tuple(int(d) for d in shape)
        n = 1
        for d in shape:
            n *= d
        self.nbytes = n * _torch.empty((), dtype=dtype).element_size()
        self.raw = _torch.full((BAND_BYTES + ALIGN + self.nbytes + BAND_BYTES,), FILL, dtype=_torch.uint8, device=device)
        self.start = BAND_BYTES + (-(self.raw.data_ptr() + BAND_BYTES)) % ALIGN
        self.site, self.kind = site, kind
        inner = self.raw[self.start:self.start + self.nbytes]
        if interior is not None and self.nbytes:
            inner.fill_(interior)
        self.view = inner.view(dtype).view(shape)
        self.snapshot = None

    def bands(self):
        return (("before", self.raw[:self.start], -self.start), ("after", self.raw[self.start + self.nbytes:], self.nbytes))

    def problems(self):
        out = []
        for side, band, base in self.bands():
            bad = band != FILL
            if bool(bad.any()):
                first = int(bad.nonzero()[0].item())
                out.append(f"{self.kind} from {self.site} ({tuple(self.view.shape)} {self.view.dtype}): band {side} the view changed, "
                           f"first at byte offset {base + first} from the view's start ({int(bad.sum().item())} bytes in all)")
        if self.snapshot is not None:
            now = self.raw[self.start:self.start + self.nbytes]
            bad = now != self.snapshot
            if bool(bad.any()):
                out.append(f"{self.kind} from {self.site}: interior changed, first at byte offset {int(bad.nonzero()[0].item())}")
        return out


class Session:
    """The buffers one test placed and recorded."""

    def __init__(self):
        self.buffers = []
        self.unguarded = []

    def banded(self, t, device, inplace=False):
        """Copy ``t`` between two ``0xFF`` bands on ``device``; the result is contiguous, shaped and typed like ``t``.
        ``inplace``: an operand the op updates in place (its bands are checked, its contents are the caller's to compare)."""
        src = t.detach().contiguous()
        buf = _Buffer(src.shape, src.dtype, device, None, _site(), "input")
        if buf.nbytes:
            buf.view.copy_(src)
        if not inplace:
            buf.snapshot = buf.raw[buf.start:buf.start + buf.nbytes].clone()
        self.buffers.append(buf)
        return buf.view

    def _new(self, shape, dtype, device, interior):
        buf = _Buffer(shape, dtype, device, interior, _site(), "zeros" if interior == 0 else "empty")
        self.buffers.append(buf)
        return buf.view

    def check(self):
        problems = []
        for buf in self.buffers:
            problems += buf.problems()
        if self.unguarded:
            problems.append(f"{len(self.unguarded)} unguarded allocation(s): " + "; ".join(self.unguarded))
        assert not problems, "guard bands:\n  " + "\n  ".join(problems)


class _TorchProxy:
    """Stands in for the name ``torch`` inside sis_hip: everything is the real module's, except the four allocating functions
    on the device under test."""

    def __init__(self, session, device):
        self.__dict__["_session"] = session
        self.__dict__["_device"] = _torch.device(device)

    def __getattr__(self, name):
        return getattr(_torch, name)

    def _mine(self, device):
        return device is not None and _same_device(device, self._device)

    def _fresh(self, real, interior, size, kw):
        if len(size) == 1 and isinstance(size[0], (tuple, list, _torch.Size)):
            size = tuple(size[0])
        device = kw.get("device")
        if device is None or not self._mine(device):
            return real(*size, **kw) if size else real(size, **kw)
        extra = {k: v for k, v in kw.items() if k not in ("dtype", "device") and v not in (None, False)}
        if extra:
            self._session.unguarded.append(f"{real.__name__}({sorted(extra)}) at {_site()}")
            return real(size, **kw)
        dtype = kw.get("dtype") or _torch.get_default_dtype()
        return self._session._new(size, dtype, device, interior)

    def _like(self, real, interior, t, kw):
        device = kw.get("device") or t.device
        if not self._mine(device):
            return real(t, **kw)
        extra = {k: v for k, v in kw.items() if k not in ("dtype", "device") and v not in (None, False)}
        if extra or not t.is_contiguous():
            self._session.unguarded.append(f"{real.__name__} of a {tuple(t.shape)} tensor with strides {tuple(t.stride())} at {_site()}")
            return real(t, **kw)
        return self._session._new(t.shape, kw.get("dtype") or t.dtype, device, interior)

    def empty(self, *size, **kw):
        return self._fresh(_torch.empty, FILL, size, kw)

    def zeros(self, *size, **kw):
        return self._fresh(_torch.zeros, 0, size, kw)

    def empty_like(self, t, **kw):
        return self._like(_torch.empty_like, FILL, t, kw)

    def zeros_like(self, t, **kw):
        return self._like(_torch.zeros_like, 0, t, kw)


_session = Session()


def reset():
    """Forget every buffer placed so far (start of a test)."""
    global _session
    _session = Session()
    return _session


def banded(t, device, inplace=False):
    return _session.banded(t, device, inplace)


def check():
    _session.check()


@contextlib.contextmanager
def guarded(monkeypatch, device=None, workspace_bytes=None):
    """Inside the region ``sis_hip``'s own allocations on ``device`` (default: the device of the inputs placed so far) are
    banded and recorded; ``workspace_bytes`` sets ``sis_hip.WORKSPACE_BYTES`` for the region."""
    import sis_hip
    session = _session
    if device is None:
        device = session.buffers[0].raw.device if session.buffers else _torch.device("cpu")
    saved = {}
    with monkeypatch.context() as m:
        m.setattr(sis_hip, "torch", _TorchProxy(session, device))
        if workspace_bytes is not None:
            m.setattr(sis_hip, "WORKSPACE_BYTES", int(workspace_bytes))
        for name in _CACHES:
            cache = getattr(sis_hip, name)
            saved[name] = dict(cache)
            cache.clear()
        try:
            yield session
        finally:
            for name, old in saved.items():
                cache = getattr(sis_hip, name)
                cache.clear()
                cache.update(old)
