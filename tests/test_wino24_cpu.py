"""The transform triples of the Winograd F(2x4,3x3) kernel (csrc/modconv_wino24.h), in float64 on the CPU: F(2,3) on the row
axis, F(4,3) with the points 0, +-1, +-2, inf on the column axis, and the two nested as the kernel nests them."""
import numpy as np

G2 = np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]])
B2T = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=np.float64)
A2T = np.array([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=np.float64)
G4 = np.array([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6],
               [0, 0, 1]])
B4T = np.array([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0],
                [0, 4, 0, -5, 0, 1]], dtype=np.float64)
A4T = np.array([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]], dtype=np.float64)


def _unit(n, i):
    v = np.zeros(n)
    v[i] = 1.0
    return v


def _check_1d(g_mat, bt, at, m):
    """A^T [(G g) * (B^T d)] = the m outputs of correlating d (m + 2 samples) with g (3 taps), for every pair of unit vectors."""
    for a in range(3):
        for b in range(m + 2):
            g, d = _unit(3, a), _unit(m + 2, b)
            want = np.array([sum(d[o + k] * g[k] for k in range(3)) for o in range(m)])
            np.testing.assert_allclose(at @ ((g_mat @ g) * (bt @ d)), want, rtol=0, atol=1e-13)


def test_f23_rows():
    _check_1d(G2, B2T, A2T, 2)


def test_f43_columns():
    _check_1d(G4, B4T, A4T, 4)


def test_f2x4_nested():
    """Y = A2^T [(G2 g G4^T) * (B2^T d B4)] A4 for every unit tap against every unit patch element."""
    for a in range(9):
        for b in range(24):
            g, d = _unit(9, a).reshape(3, 3), _unit(24, b).reshape(4, 6)
            want = np.array([[sum(d[r + i, c + j] * g[i, j] for i in range(3) for j in range(3)) for c in range(4)] for r in range(2)])
            got = A2T @ ((G2 @ g @ G4.T) * (B2T @ d @ B4T.T)) @ A4T.T
            np.testing.assert_allclose(got, want, rtol=0, atol=1e-13)


def test_binding_declares_the_entries():
    import sis_hip
    assert {"sis_modconv_prepack_wino24", "sis_modconv_wino24_eligible", "sis_modconv2d_wino24"} <= set(sis_hip.exported_symbols())


def test_eligibility_rule():
    """The explicit cases of test_wino44_cpu.test_eligibility_rule, with the answers of the library before the two plans became
    one: H needs whole 2 x 4 tiles only, so 18 rows pass here."""
    import sis_hip
    ok = sis_hip.modconv_wino24_eligible
    assert ok(8, 64, 16, 32) and ok(8, 64, 8, 64) and ok(8, 64, 12, 64) and ok(128, 128, 256, 256)
    assert not ok(12, 64, 16, 32)    # Cin % 8
    assert not ok(8, 32, 16, 32)     # Cout % 64
    assert ok(8, 64, 18, 32)         # H % 4 is F(4x4)'s rule: H % 2 here
    assert ok(8, 64, 14, 64) and not ok(8, 64, 15, 64)   # H % 2
    assert not ok(8, 64, 16, 34)     # W % 4
    assert not ok(8, 64, 64, 16)     # W <= 16
    assert not ok(8, 64, 16, 16)     # fewer than 512 pixels


def test_the_two_forms_share_one_rule():
    """One plan serves both forms (csrc/modconv_wino_tile512.h): they differ in the H multiple, in a 2^31 bound and in an LDS
    total, and neither of the latter two is reached at these sizes."""
    import sis_hip
    ok24, ok44 = sis_hip.modconv_wino24_eligible, sis_hip.modconv_wino44_eligible
    seen = set()
    for cin in (8, 16):
        for cout in (64, 128):
            for h in range(2, 70, 2):
                for w in range(4, 140, 4):
                    assert ok44(cin, cout, h, w) == (ok24(cin, cout, h, w) and h % 4 == 0), (cin, cout, h, w)
                    seen.add((ok24(cin, cout, h, w), ok44(cin, cout, h, w)))
    assert seen == {(False, False), (True, False), (True, True)}   # the grid reaches every answer
