"""What tests/test_scan_margin_gpu.py and tests/test_scan_margin_guard_bands_gpu.py share: the device calls of one case, run
through a ``run`` / ``put`` pair (direct, or between guard bands), compared byte for byte with the restatement of DESIGN.md
§20 (tests/scan_margin_restatement.py).  The restatement's result of a case is computed once and shared."""
import ctypes

import numpy as np
import torch

import scan_margin_cases as K
import scan_margin_restatement as R

SENTINEL = -7
_CASES, _WANT = None, {}


def cases():
    global _CASES
    if _CASES is None:
        _CASES = dict(K.all_cases())
    return _CASES


def want(name):
    """The restatement's result of a case (computed once; not to be modified)."""
    if name not in _WANT:
        _WANT[name] = R.content_box(cases()[name])
    return _WANT[name]


def same(got, expected, what):
    got = got.cpu().numpy()
    expected = np.asarray(expected, dtype=got.dtype).reshape(got.shape)
    assert np.array_equal(got, expected), f"{what}: {int((got != expected).sum())} of {got.size} values differ; got {got.ravel()[:12]}, " \
                                          f"want {expected.ravel()[:12]}"


def check_case(run, put, name, outputs=True):
    """box and info (and with ``outputs`` the edge image and the whole contour table, two spare rows behind it) of one case."""
    import sis_hip
    expected = want(name)
    count = expected.info[0]
    page = put(torch.from_numpy(cases()[name]))
    got = run(sis_hip.scan_content_box, page, edges=outputs, max_contours=count + 2 if outputs else 0)
    same(got.box, expected.box, f"{name}: box")
    same(got.info, expected.info, f"{name}: info")
    if outputs:
        same(got.edges, expected.edges, f"{name}: edges")
        same(got.contours[:count], expected.contours, f"{name}: contours")
    else:
        assert got.edges is None and got.contours is None
    return got


def entry(page, max_contours, rows, edges=True, low=20, high=150):
    """The C entry itself on buffers filled with SENTINEL first: -> (box, info, edges, table of ``rows`` rows)."""
    import sis_hip
    h, w = int(page.shape[0]), int(page.shape[1])
    dev = page.device
    box = torch.full((4,), SENTINEL, dtype=torch.int32, device=dev)
    info = torch.full((8,), SENTINEL, dtype=torch.int32, device=dev)
    edge_image = torch.full((h, w), 0x5A, dtype=torch.uint8, device=dev) if edges else None
    table = torch.full((max(rows, 1), 6), SENTINEL, dtype=torch.int32, device=dev)
    ws_bytes = int(sis_hip.lib().sis_scan_content_box_workspace_bytes(h, w))
    ws = torch.full((ws_bytes // 4,), -1, dtype=torch.int32, device=dev)

    def ptr(t):
        return None if t is None else ctypes.c_void_p(t.data_ptr())

    rc = sis_hip.lib().sis_scan_content_box(ptr(box), ptr(info), ptr(edge_image), ptr(table), max_contours, ptr(page), h, w, low, high,
                                            ptr(ws), ws_bytes, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, sis_hip.lib().sis_last_error().decode()
    return box, info, edge_image, table


def check_truncated_table(device, name):
    """max_contours below the count: the stored rows are the prefix, the rows behind stay as they were, box and info do not move."""
    expected = want(name)
    count = expected.info[0]
    assert count >= 2, name
    page = torch.from_numpy(cases()[name]).to(device)
    for stored in sorted({1, count // 2, count - 1}):
        box, info, _, table = entry(page, stored, count, edges=False)
        same(box, expected.box, f"{name}: box with {stored} rows")
        same(info, expected.info, f"{name}: info with {stored} rows")
        same(table[:stored], expected.contours[:stored], f"{name}: the first {stored} rows")
        assert bool((table[stored:] == SENTINEL).all()), f"{name}: a row behind the first {stored} was written"
    box, info, _, table = entry(page, 0, count, edges=False)
    same(box, expected.box, f"{name}: box with no table")
    same(info, expected.info, f"{name}: info with no table")
    assert bool((table == SENTINEL).all())


def check_remove_margin(run, put, page, analysis_size=1000):
    """``scan_remove_margin`` against the restatement on Pillow's own thumbnail and Pillow's crop."""
    import sis_hip
    cropped, box, crop = R.remove_margin(page, analysis_size)
    got, got_box, got_crop = run(sis_hip.scan_remove_margin, put(torch.from_numpy(page)), analysis_size)
    assert (got_box, got_crop) == (box, crop), (got_box, got_crop, box, crop)
    assert got.is_contiguous()
    same(got, cropped, "the cropped page")
    return box, crop
