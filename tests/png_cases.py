"""Inputs of the PNG encoder tests (CPU and GPU): small uint8 images whose FILTERED rows hold planted content, and the
comparison of device files with tests/png_restatement.py."""
import functools
import io

import numpy as np

import png_restatement as P

# follower counts (run length - 1) at the bases of the length-code ranges whose extra-bit width changes, the 7-bit / 8-bit
# length-code boundary (114 / 115) and the 258 cap
BOUNDARY_FOLLOWERS = (3, 10, 11, 114, 115, 130, 131, 226, 227, 257, 258, 259)
FLAT_WIDTHS = (88, 174, 175, 176, 260)   # one flat row: 3 W - 4 followers = 260 / 518 / 521 / 524 / 776, remainders 2 / 2 / 5 / 8 / 2


def image_from_filtered(filtered):
    """uint8 [H, 3 W] filtered bytes (without the filter-type byte) -> uint8 [H, W, 3] pixels whose Sub filter gives them."""
    filtered = np.asarray(filtered, dtype=np.uint8)
    h, n = filtered.shape
    assert n % 3 == 0
    raw = np.cumsum(filtered.reshape(h, n // 3, 3).astype(np.int64), axis=1) & 255
    return raw.astype(np.uint8)


def planted_runs(followers=BOUNDARY_FOLLOWERS):
    """One row whose filtered bytes are runs with the given follower counts, neighbours differing, padded to whole pixels."""
    row = []
    for k, count in enumerate(followers):
        row += [10 + 2 * k] * (count + 1)
    pad = 200
    while len(row) % 3:
        row.append(pad)
        pad += 1
    return image_from_filtered(np.array([row], dtype=np.uint8))[None]


def literal_boundary():
    """Filtered bytes 143 / 144 / 255 (the 8-bit / 9-bit literal split) beside their neighbours, no runs."""
    row = [143, 144, 255, 0, 142, 145, 254, 143, 255, 144, 1, 2]
    return image_from_filtered(np.array([row, row[::-1]], dtype=np.uint8))[None]


def flat_row(width, value=200):
    return np.full((1, 1, width, 3), value, dtype=np.uint8)


def random_pair(seed, n, h, w, wl):
    rng = np.random.default_rng(seed)
    image = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    label = rng.integers(0, 3, (n, h, wl, 1), dtype=np.uint8).repeat(3, axis=3) * 100 if wl else None
    return image, label


def seam_batch():
    """Three different images in one call: dark (8-bit literals), bright (9-bit literals) and mixed with flat stretches, so
    that the sizes differ and the rows end on many bit phases."""
    rng = np.random.default_rng(11)
    h, w, wl = 5, 7, 4
    image = np.stack([rng.integers(0, 100, (h, w, 3)), rng.integers(160, 256, (h, w, 3)), rng.integers(0, 256, (h, w, 3))]).astype(np.uint8)
    image[2, 1:4] = 77
    label = np.zeros((3, h, wl, 3), dtype=np.uint8)
    label[0], label[1, :, :2], label[2, 2:] = (255, 0, 0), (0, 0, 255), (9, 9, 9)
    return image, label


def byte_boundary_pair():
    """(image whose deflate block ends exactly on a byte boundary, image whose block does not), found with the restatement."""
    on, off = None, None
    for seed in range(200):
        image = np.random.default_rng(1000 + seed).integers(0, 256, (1, 2, 3, 3), dtype=np.uint8)
        bits = P.stream_bits(P.filtered_rows(image[0]))
        if bits % 8 == 0 and on is None:
            on = image
        if bits % 8 != 0 and off is None:
            off = image
        if on is not None and off is not None:
            return on, off
    raise AssertionError("no pair found")


def workload_pair():
    """One 256 x 512 pair like the dataset's: a noisy light page on the left, flat class colours on the right."""
    rng = np.random.default_rng(5)
    page = np.clip(rng.normal(225, 12, (1, 256, 256, 3)), 0, 255).astype(np.uint8)
    page[0, 40:60, 30:220] = rng.integers(0, 90, (20, 190, 3), dtype=np.uint8)
    label = np.zeros((1, 256, 256, 3), dtype=np.uint8)
    label[0, 40:60, 30:220] = (255, 0, 0)
    label[0, 100:180, 20:130] = (0, 0, 255)
    return page, label


@functools.lru_cache(maxsize=None)
def workload_case():
    """(image, label, expected files) of the workload pair: restated once per process, shared by the tests that need it."""
    image, label = workload_pair()
    return image, label, tuple(expected_files(image, label))


def expected_files(image, label=None):
    return [P.encode_png(image[i], None if label is None else label[i]) for i in range(image.shape[0])]


def assert_files_equal(buffer, sizes, image, label=None, expected=None):
    """buffer uint8 [N, stride], sizes int32 [N] (numpy) against the restatement's bytes and, through PIL, the pixels."""
    from PIL import Image
    expected = expected if expected is not None else expected_files(image, label)
    assert buffer.shape[1] >= P.capacity(image.shape[1], image.shape[2] + (0 if label is None else label.shape[2]))
    for i, want in enumerate(expected):
        got = buffer[i, :sizes[i]].tobytes()
        assert int(sizes[i]) == len(want), (i, int(sizes[i]), len(want))
        if got != want:
            first = next(k for k in range(len(want)) if got[k] != want[k])
            raise AssertionError(f"file {i}: first differing byte at offset {first} of {len(want)}: {got[first]:#x} != {want[first]:#x}")
        assert not buffer[i, sizes[i]:].any(), f"file {i}: bytes behind the file are not zero"
        pixels = image[i] if label is None else np.concatenate([image[i], label[i]], axis=1)
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(got)).convert("RGB")), pixels), f"file {i}: PIL decodes other pixels"
