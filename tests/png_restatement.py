"""Restatement of the byte format of ``sis_hip.png_encode_pairs`` ("PNG pairs encoded on the device") in plain
Python / numpy; ``zlib`` is used for ``adler32`` and ``crc32`` only.  The device bytes must EQUAL these bytes.

One file per image: signature, IHDR (width = image width + label width, 8-bit RGB), ONE IDAT, IEND.  Scanline r is image
row r followed by label row r; every row has filter type 1 (Sub, bpp 3).  The IDAT payload is ``78 01``, one deflate block
with fixed Huffman codes (BFINAL = 1, BTYPE = 01), the end-of-block code, zero bits to the byte boundary and the Adler-32 of
the filtered bytes.  Tokens are defined per filtered row (``tokens_greedy``): at position i, L = the number of bytes from i on
that equal byte i - 1 (counted while L < 258, 0 at i = 0); L >= 3 is a match of length L at distance 1, anything else a literal.
``tokens_closed_form`` is the same rule per maximal run, which is what the kernels evaluate.
"""
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
MAX_MATCH = 258

# RFC 1951 §3.2.5: (first length code, extra bits, first base) of the groups of four codes; 258 is code 285 on its own
_LEN_BASES = []
_base = 3
for _code in range(257, 285):
    _extra = 0 if _code < 265 else (_code - 261) // 4
    _LEN_BASES.append((_code, _extra, _base))
    _base += 1 << _extra
_LEN_BASES.append((285, 0, 258))


def length_code(length):
    """(code, number of extra bits, extra value): the code with the largest base <= length."""
    assert 3 <= length <= MAX_MATCH
    best = None
    for code, extra, base in _LEN_BASES:
        if base <= length:
            best = (code, extra, length - base)
    assert best[2] < (1 << best[1]) or best[1] == 0 and best[2] == 0
    return best


def fixed_code(symbol):
    """(code, bits) of a literal/length symbol under the fixed Huffman code (RFC 1951 §3.2.6)."""
    if symbol < 144:
        return 0x30 + symbol, 8
    if symbol < 256:
        return 0x190 + symbol - 144, 9
    if symbol < 280:
        return symbol - 256, 7
    return 0xC0 + symbol - 280, 8


def filtered_rows(image, label=None):
    """uint8 [H, W, 3] (+ [H, Wl, 3]) -> list of H ``bytes`` rows: 0x01, then raw[i] - raw[i - 3] mod 256."""
    pair = np.asarray(image, dtype=np.uint8)
    if label is not None:
        pair = np.concatenate([pair, np.asarray(label, dtype=np.uint8)], axis=1)
    h = pair.shape[0]
    raw = pair.reshape(h, -1).astype(np.int16)
    sub = raw.copy()
    sub[:, 3:] -= raw[:, :-3]
    sub = (sub & 255).astype(np.uint8)
    return [b"\x01" + sub[r].tobytes() for r in range(h)]


def tokens_greedy(row):
    """The definition: scan left to right; ("lit", value) and ("match", length) tokens."""
    out, i, n = [], 0, len(row)
    while i < n:
        run = 0
        if i > 0:
            while run < MAX_MATCH and i + run < n and row[i + run] == row[i - 1]:
                run += 1
        if run >= 3:
            out.append(("match", run))
            i += run
        else:
            out.append(("lit", row[i]))
            i += 1
    return out


def tokens_closed_form(row):
    """The same tokens per maximal run of R equal bytes: one literal, (R - 1) // 258 matches of 258, then the remainder
    r = (R - 1) % 258 as one match (r >= 3) or r literals (r < 3)."""
    out, i, n = [], 0, len(row)
    while i < n:
        j = i
        while j < n and row[j] == row[i]:
            j += 1
        followers = j - i - 1
        out.append(("lit", row[i]))
        out += [("match", MAX_MATCH)] * (followers // MAX_MATCH)
        rest = followers % MAX_MATCH
        out += [("match", rest)] if rest >= 3 else [("lit", row[i])] * rest
        i = j
    return out


class BitWriter:
    """Deflate's bit order: bits fill a byte from its least significant end; Huffman codes go in most significant bit first."""

    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def bits(self, value, count):   # least significant bit first
        self.acc |= value << self.n
        self.n += count
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, count):    # most significant bit first
        self.bits(int(format(code, f"0{count}b")[::-1], 2), count)

    def finish(self):
        if self.n:
            self.bits(0, 8 - self.n)
        return bytes(self.out)


def token_bits(token):
    """Number of bits a token takes in the stream."""
    kind, value = token
    if kind == "lit":
        return fixed_code(value)[1]
    code, extra, _ = length_code(value)
    return fixed_code(code)[1] + extra + 5


def zlib_stream(rows, tokens=tokens_closed_form):
    w = BitWriter()
    w.out += b"\x78\x01"
    w.bits(1, 1)   # BFINAL
    w.bits(1, 2)   # BTYPE = 01
    for row in rows:
        for kind, value in tokens(row):
            if kind == "lit":
                w.code(*fixed_code(value))
            else:
                code, extra, extra_value = length_code(value)
                w.code(*fixed_code(code))
                w.bits(extra_value, extra)
                w.code(0, 5)   # distance 1
    w.code(*fixed_code(256))
    return w.finish() + struct.pack(">I", zlib.adler32(b"".join(rows)))


def stream_bits(rows):
    """Bits of the deflate block up to and including the end-of-block code (the stream ends on a byte boundary when this is a
    multiple of 8)."""
    return 3 + sum(token_bits(t) for row in rows for t in tokens_closed_form(row)) + 7


def chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data))


def ihdr(width, height):
    return struct.pack(">IIBBBBB", width, height, 8, 2, 0, 0, 0)


def encode_png(image, label=None):
    """The file bytes of one [image | label] pair."""
    rows = filtered_rows(image, label)
    width = (len(rows[0]) - 1) // 3
    return SIGNATURE + chunk(b"IHDR", ihdr(width, len(rows))) + chunk(b"IDAT", zlib_stream(rows)) + chunk(b"IEND", b"")


def capacity(height, width_total):
    """Per-image stride of the output buffer: a literal costs at most 9 bits per byte, a match at most 18 for at least 3."""
    f = height * (1 + 3 * width_total)
    z = 2 + (10 + 9 * f + 7) // 8 + 4
    return (57 + z + 15) // 16 * 16
