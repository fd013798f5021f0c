"""The PNG encoder without a device: the format's restatement against zlib and PIL, the closed-form run rule against the
greedy definition, the capacity formula at its worst case, the C ABI's declarations and argument checks, the tool's options."""
import ctypes
import io
import os
import re
import zlib

import numpy as np
import pytest

import png_cases as K
import png_restatement as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = {"sis_png_capacity", "sis_png_encode_pairs_workspace_bytes", "sis_png_encode_pairs"}
NEW_KERNELS = {"png_count_kernel", "png_offsets_kernel", "png_emit_kernel", "png_crc_kernel", "png_finish_kernel"}


def _shape_cases():
    """The inputs of tests/test_png_encode_gpu.py (the workload pair apart: it is restated there)."""
    cases = [("one pixel", np.array([[[[7, 200, 143]]]], dtype=np.uint8), None)]
    for h, w, wl in [(3, 5, 0), (2, 87, 0), (3, 5, 2), (2, 87, 87)]:
        cases.append((f"random {h}x{w}+{wl}", *K.random_pair(h * 100 + w + wl, 2, h, w, wl)))
    cases += [(f"flat {w}", K.flat_row(w), None) for w in K.FLAT_WIDTHS]
    cases += [("planted runs", K.planted_runs(), None), ("literal boundary", K.literal_boundary(), None), ("seams", *K.seam_batch())]
    cases += [(f"byte boundary {i}", image, None) for i, image in enumerate(K.byte_boundary_pair())]
    return cases


@pytest.mark.parametrize("name,image,label", _shape_cases(), ids=[c[0] for c in _shape_cases()])
def test_restatement_is_a_zlib_stream_and_a_png(name, image, label):
    from PIL import Image
    for i in range(image.shape[0]):
        lab = None if label is None else label[i]
        rows = P.filtered_rows(image[i], lab)
        stream = P.zlib_stream(rows)
        assert stream[:2] == b"\x78\x01" and zlib.decompress(stream) == b"".join(rows)
        assert stream == P.zlib_stream(rows, P.tokens_greedy)
        data = P.encode_png(image[i], lab)
        assert len(data) == 57 + len(stream) <= P.capacity(image.shape[1], image.shape[2] + (0 if lab is None else lab.shape[1]))
        assert data.count(b"IDAT") == 1
        decoded = Image.open(io.BytesIO(data))
        assert decoded.mode == "RGB"
        assert np.array_equal(np.asarray(decoded), image[i] if lab is None else np.concatenate([image[i], lab], axis=1))


def test_byte_boundary_cases_are_what_they_claim():
    on, off = K.byte_boundary_pair()
    assert P.stream_bits(P.filtered_rows(on[0])) % 8 == 0 and P.stream_bits(P.filtered_rows(off[0])) % 8 != 0


def test_flat_rows_have_the_stated_follower_counts():
    for w, followers in zip(K.FLAT_WIDTHS, (260, 518, 521, 524, 776)):
        row = P.filtered_rows(K.flat_row(w)[0])[0]
        assert row[4:] == bytes(followers + 1) and row[3] != 0
        rest = followers % 258
        assert P.tokens_closed_form(row)[-(1 if rest >= 3 else rest):] == ([("match", rest)] if rest >= 3 else [("lit", 0)] * rest)


def test_closed_form_equals_the_greedy_definition():
    rng = np.random.default_rng(0)
    for trial in range(60):
        n = int(rng.integers(1, 1400))
        row = rng.integers(0, 4 if trial % 2 else 256, n, dtype=np.uint8)
        for _ in range(int(rng.integers(0, 6))):   # planted runs, also longer than 258 and up to the row's end
            at, length = int(rng.integers(0, n)), int(rng.choice([2, 3, 4, 5, 258, 259, 260, 261, 262, 516, 517, 520, 700]))
            row[at:at + length] = rng.integers(0, 256)
        row = bytes(row)
        assert P.tokens_closed_form(row) == P.tokens_greedy(row)
    for length in list(range(1, 12)) + [258, 259, 260, 261, 262, 517, 518, 519, 520]:
        row = bytes([1] * length)   # the run takes the filter-type byte in
        assert P.tokens_closed_form(row) == P.tokens_greedy(row)


def test_length_codes():
    want = {3: (257, 0, 0), 10: (264, 0, 0), 11: (265, 1, 0), 12: (265, 1, 1), 114: (279, 4, 15), 115: (280, 4, 0), 130: (280, 4, 15),
            131: (281, 5, 0), 226: (283, 5, 31), 227: (284, 5, 0), 257: (284, 5, 30), 258: (285, 0, 0)}
    for length, triple in want.items():
        assert P.length_code(length) == triple, length
    assert P.fixed_code(143) == (0xBF, 8) and P.fixed_code(144) == (0x190, 9) and P.fixed_code(255) == (0x1FF, 9)
    assert P.fixed_code(256) == (0, 7) and P.fixed_code(279) == (23, 7) and P.fixed_code(280) == (0xC0, 8)


def test_capacity_at_the_worst_case():
    """Every filtered byte >= 144 (9 bits) and no runs: the file is within 16 bytes of the stride, and never above it."""
    import sis_hip
    L = sis_hip.lib()
    for h, w in [(1, 1), (3, 5), (4, 9), (7, 33)]:
        filtered = 144 + (37 * np.arange(3 * w)[None, :] + 11 * np.arange(h)[:, None]) % 112   # neighbours differ by 37
        assert not (filtered[:, 1:] == filtered[:, :-1]).any()
        image = K.image_from_filtered(filtered.astype(np.uint8))
        size = len(P.encode_png(image))
        f = h * (1 + 3 * w)
        assert size == 57 + 2 + (10 + 8 * h + 9 * (f - h) + 7) // 8 + 4   # the filter-type bytes cost 8 bits each
        assert size <= P.capacity(h, w) < size + 16 + h
        assert L.sis_png_capacity(h, w) == P.capacity(h, w) and P.capacity(h, w) % 16 == 0
    assert L.sis_png_capacity(256, 512) == P.capacity(256, 512) == (57 + 2 + (10 + 9 * 256 * 1537 + 7) // 8 + 4 + 15) // 16 * 16
    assert L.sis_png_capacity(0, 5) == 0 and L.sis_png_capacity(5, 0) == 0


def test_header_ctypes_table_and_library_agree():
    import sis_hip
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sis_hip.h")).read(), flags=re.S)
    assert NEW_SYMBOLS <= set(re.findall(r"\b(sis_[a-z0-9_]+)\s*\(", header)) and NEW_SYMBOLS <= set(sis_hip.exported_symbols())
    L = sis_hip.lib()
    for name in NEW_SYMBOLS:
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, header).group(1)
        assert decl.count(",") + 1 == len(sis_hip._SIGNATURES[name][0]), name
        assert hasattr(L, name)
    text = open(os.path.join(ROOT, "include", "sis_hip.h")).read()
    for name in NEW_SYMBOLS:   # every entry cites the reference's save_image
        assert re.search(r"%s \(.{0,40}:84-90, save_image" % name, text), name
    assert NEW_KERNELS <= sis_hip.own_kernel_names()


def test_entry_declines_bad_arguments_before_any_launch():
    import sis_hip
    L = sis_hip.lib()
    p = ctypes.c_void_p(4096)   # never dereferenced: every case returns at its check
    cap = L.sis_png_capacity(4, 6)
    ws = L.sis_png_encode_pairs_workspace_bytes(2, 4)
    assert ws == 2 * (3 * 4 + 4) * 4 and L.sis_png_encode_pairs_workspace_bytes(0, 4) == 0

    def call(n=2, h=4, w=4, wl=2, stride=cap, label=p, workspace_bytes=ws, out=p):
        return L.sis_png_encode_pairs(out, p, p, label, n, h, w, wl, stride, 0, p, workspace_bytes, None)

    for kw, text in [(dict(n=0), "n 0"), (dict(h=0), "height 0"), (dict(w=0), "widths 0"), (dict(wl=-1), "+ -1"),
                     (dict(stride=cap - 16), "out_stride"), (dict(stride=cap + 8), "multiple of 16"), (dict(label=None), "label"),
                     (dict(wl=0), "label"), (dict(w=4000, wl=200), "total width"), (dict(workspace_bytes=ws - 4), "workspace"),
                     (dict(out=ctypes.c_void_p(4100)), "aligned"), (dict(out=None), "null")]:
        assert call(**kw) != 0, kw
        assert text in L.sis_last_error().decode(), (kw, L.sis_last_error().decode())


def test_cli_options():
    import argparse
    import create_dataset_for_segmentation as cds
    assert cds.PNG_ENCODERS == ("pil", "device")
    assert [cds.png_writer_count(v) for v in (None, 4, 0, -3, 8, 9, 1000, "6")] == [4, 4, 1, 1, 8, 8, 8, 6]
    parser = cds.build_parser()
    defaults = parser.parse_args([])
    assert defaults.png_encoder == "pil" and defaults.png_writers == 4
    chosen = parser.parse_args(["--png-encoder", "device", "--png-writers", "64"])
    assert chosen.png_encoder == "device" and chosen.png_writers == 8 and parser.parse_args(["--png-writers", "0"]).png_writers == 1
    with pytest.raises(SystemExit):
        parser.parse_args(["--png-encoder", "zlib"])
    text = open(cds.__file__).read()
    assert "cpu_count" not in text
    assert "--png-encoder device" in cds.__doc__ and "--png-writers" in cds.__doc__
    with pytest.raises(ValueError, match="png-encoder"):   # checked before a device is touched
        cds.build_dataset(argparse.Namespace(png_encoder="zlib"), {})


def test_writer_pool_writes_and_raises_in_the_caller(tmp_path):
    import create_dataset_for_segmentation as cds
    pool = cds.PngWriterPool(3)
    for i in range(20):
        pool.submit(cds.image_path(i * 1000, tmp_path, "{id:06d}.png"), memoryview(bytes([i]) * 10))
    pool.drain(keep_in_flight=5)
    assert len(pool.futures) <= 5
    pool.close()
    assert sorted(p.name for p in tmp_path.rglob("*.png")) == [f"{i * 1000:06d}.png" for i in range(20)]
    assert (tmp_path / "0" / "19" / "019000.png").read_bytes() == bytes([19]) * 10
    pool = cds.PngWriterPool(2)
    (tmp_path / "file").write_text("not a directory")
    pool.submit(tmp_path / "file" / "x.png", b"1")
    with pytest.raises(OSError):
        pool.close()
