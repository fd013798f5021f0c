"""NumPy restatement of Winograd F(4x4,3x3) as csrc/modconv_wino44.h uses it: the 6-point transform (points 0, +-1, +-2, inf) on
both axes.  Y = A^T [ (G g G^T) * (B^T d B) ] A for a 6 x 6 patch d and a 3 x 3 filter g (correlation, as the convolution layers)."""
import numpy as np

BT = np.array([[4, 0, -5, 0, 1, 0],
               [0, -4, -4, 1, 1, 0],
               [0, 4, -4, -1, 1, 0],
               [0, -2, -1, 2, 1, 0],
               [0, 2, -1, -2, 1, 0],
               [0, 4, 0, -5, 0, 1]], dtype=np.float64)
G = np.array([[1 / 4, 0, 0],
              [-1 / 6, -1 / 6, -1 / 6],
              [-1 / 6, 1 / 6, -1 / 6],
              [1 / 24, 1 / 12, 1 / 6],
              [1 / 24, -1 / 12, 1 / 6],
              [0, 0, 1]], dtype=np.float64)
AT = np.array([[1, 1, 1, 1, 1, 0],
               [0, 1, -1, 2, -2, 0],
               [0, 1, 1, 4, 4, 0],
               [0, 1, -1, 8, -8, 1]], dtype=np.float64)


def direct_tile(d, g):
    """4 x 4 outputs of the 3 x 3 correlation of the 6 x 6 patch d with g; leading axes broadcast."""
    out = np.zeros(d.shape[:-2] + (4, 4), dtype=np.result_type(d, g))
    for a in range(3):
        for b in range(3):
            out += g[..., a, b, None, None] * d[..., a:a + 4, b:b + 4]
    return out


def weight_planes(g, dtype=np.float64):
    """U = G g G^T, [..., 6, 6]."""
    Gm = G.astype(dtype)
    return np.einsum("ia,...ab,jb->...ij", Gm, g.astype(dtype), Gm).astype(dtype)


def data_planes(d, dtype=np.float64):
    """V = B^T d B, [..., 6, 6]."""
    Bm = BT.astype(dtype)
    return np.einsum("ia,...ab,jb->...ij", Bm, d.astype(dtype), Bm).astype(dtype)


def output_tile(m, dtype=np.float64):
    """Y = A^T M A, [..., 4, 4]."""
    Am = AT.astype(dtype)
    return np.einsum("ri,...ij,xj->...rx", Am, m.astype(dtype), Am).astype(dtype)


_F = np.float32


def _fma(a, b, c):
    """fp32 fused multiply-add: the product of two fp32 values is exact in float64, one rounding of the sum to fp32."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(_F)


def _six_point_data(x0, x1, x2, x3, x4, x5):
    """B6^T applied along one axis the way the kernel's t_col / t_row do it; fp32 in, fp32 out."""
    u, v = _fma(_F(-4), x2, x4), _fma(_F(-4), x1, x3)
    p, q = x4 - x2, x3 - x1
    return [_fma(_F(4), x0, _fma(_F(-5), x2, x4)), u + v, u - v, _fma(_F(2), q, p), _fma(_F(-2), q, p), _fma(_F(4), x1, _fma(_F(-5), x3, x5))]


def _six_point_weight(a, b, c):
    """G4 applied along one axis as wino44_prepack_kernel does it (separate products and sums, each rounded)."""
    s6, s24, s12 = _F(1) / _F(6), _F(1) / _F(24), _F(1) / _F(12)
    return [_F(0.25) * a, -s6 * ((a + b) + c), -s6 * ((a - b) + c), (s24 * a + s12 * b) + s6 * c, (s24 * a - s12 * b) + s6 * c, c]


def _four_point_out(m0, m1, m2, m3, m4, m5):
    """A4^T applied along one axis as the kernel's epilogue does it."""
    s12, d12, s34, d34 = m1 + m2, m1 - m2, m3 + m4, m3 - m4
    return [(m0 + s12) + s34, _fma(_F(2), d34, d12), _fma(_F(4), s34, s12), _fma(_F(8), d34, d12) + m5]


def emulate_fp32(d, g, s, fma_chain=False):
    """The kernel's arithmetic in fp32 for tiles d [T, Cin, 6, 6], filters g [Co, Cin, 3, 3], style s [Cin]: both transforms in
    the kernel's own order of operations, the style on the data planes, the products accumulated over Cin in ascending order, the
    output transform on rows, then on columns.  Returns [T, Co, 4, 4] fp32.

    The accumulation: in chunks of 4 channels (one MFMA step) -- the four products of a chunk summed in fp32, the sum added to the
    accumulator, one accumulator rounding per chunk; with ``fma_chain`` one FMA per channel instead, one accumulator rounding per
    channel, which is what a v_mfma_f32_16x16x4_f32 step is documented to equal bit for bit."""
    d, g, s = d.astype(_F), g.astype(_F), s.astype(_F)
    cols = np.stack(_six_point_data(*[d[..., j] for j in range(6)]), axis=-1)                # (d B6)[r][j]
    v = np.stack(_six_point_data(*[cols[..., r, :] for r in range(6)]), axis=-2)             # B6^T (d B6)
    v = v * s[None, :, None, None]
    t = np.stack(_six_point_weight(g[..., 0, :], g[..., 1, :], g[..., 2, :]), axis=-2)        # (G4 g)[i][c]
    u = np.stack(_six_point_weight(t[..., 0], t[..., 1], t[..., 2]), axis=-1)                 # (G4 g) G4^T
    m = np.zeros((d.shape[0], g.shape[0], 6, 6), dtype=_F)
    for c in range(0, d.shape[1], 4):
        if fma_chain:
            for k in range(c, c + 4):
                m = _fma(u[None, :, k], v[:, None, k], m)
        else:
            pr = [u[None, :, k] * v[:, None, k] for k in range(c, c + 4)]
            m = m + ((pr[0] + pr[1]) + (pr[2] + pr[3]))
    rows = np.stack(_four_point_out(*[m[..., i, :] for i in range(6)]), axis=-2)              # A4^T M
    return np.stack(_four_point_out(*[rows[..., j] for j in range(6)]), axis=-1)              # (A4^T M) A4


def plane(i, jj):
    """Plane a of (row i, column 3 q + jj) in a wave's 18: see the head of csrc/modconv_wino44.h."""
    n = 3 * (i % 3) + jj
    return 8 * (i // 3) + n if n < 8 else 16 + i // 3


def unshuffle_u(u):
    """The prepacked image [Cin, 9, Cout, 4] -> [Cout, Cin, 6, 6]."""
    cin, _, cout, _ = u.shape
    out = np.zeros((cout, cin, 6, 6), dtype=u.dtype)
    for i in range(6):
        for j in range(6):
            q, a = j // 3, plane(i, j % 3)
            row, k = (4 * q + a // 4, a % 4) if a < 16 else (8, 2 * q + a - 16)
            out[:, :, i, j] = u[:, row, :, k].T
    return out
