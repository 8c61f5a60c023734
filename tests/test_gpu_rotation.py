"""The rotation a randomized fit ends in (engine.cpp rotate_into_components: panel_gemm with ld != ldo, then flip_transpose),
through sapca_rotate_panel_* on the panels of tests/dense_tail_cases.py: integer panels whose product is exact in both dtypes,
columns whose two largest entries tie at the places the sign kernels' reductions meet, a zero column, a column of nan, and one
Gaussian panel per dtype.  tests/test_dense_tail_cases_cpu.py holds the cases to their conditions without a GPU."""
import numpy as np
import pytest
import torch  # noqa: F401  (first: one HIP runtime per process)

import dense_tail_cases as C
from sapca import ops

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]


@pytest.fixture(scope="module")
def session():
    return ops.Session()


def _exact(session, P, M, dtype):
    """rotate the integer pair and compare with the exact answer bit for bit; returns the signs"""
    Y = (P @ M).astype(np.float64)
    want, want_signs = C.flip_reference(Y)
    got, signs = session.rotate_panel(P.astype(dtype), M.astype(np.float64))
    assert got.dtype == np.dtype(dtype) and got.shape == want.shape
    assert np.array_equal(signs, want_signs), np.flatnonzero(signs != want_signs)
    assert got.tobytes() == want.astype(dtype).tobytes(), np.argwhere(got != want.astype(dtype))[:5]
    return signs


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("l,k,n", C.rotation_shapes())
def test_integer_panels_bit_for_bit(session, l, k, n, dtype):
    """components == (signs * (P64 @ M)).T bit for bit and signs == numpy's (argmax of |.| with the first index, then its sign):
    l = 16 .. 270 through the one-launch and the block-by-block panel product, 768 threads at 112 / 128 columns, 512 from 1024
    row tiles (n = 16369) at 64 columns; n either side of 16 rows a tile and of the 4096 rows from which the signs take two
    stages.  Random integer columns of this height tie by themselves: the tie rule is part of the comparison."""
    P, M = C.integer_rotation(l, k, n)
    _exact(session, P, M, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("l,k,n", C.TIE_SHAPES)
def test_ties_take_the_first_row(session, l, k, n, dtype):
    """Columns with exactly two entries of largest magnitude and opposite signs -- in rows of one thread, of two row groups (or
    threads) of a block in either order, of two blocks, the first and the last row, rows 4095 and 4096, the short last block --
    each in both orders of the two signs, on the two-stage route (ldk = 64 and 32: four and eight row groups) and the
    one-kernel route; and a zero column: sign +1, component row all +0."""
    for P, M, marks in C.tie_panels(l, k, n):
        signs = _exact(session, P, M, dtype)
        for c, (name, r1, r2, s) in marks.items():
            assert signs[c] == s, (name, r1, r2, s)
        zero = [c for c, m in marks.items() if m[0] == "zero"]
        if zero:
            got, _ = session.rotate_panel(P.astype(dtype), M.astype(np.float64))
            assert not got[zero[0]].any() and not np.signbit(got[zero[0]]).any()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("l,k,n", C.NAN_SHAPES)
def test_nan_column_keeps_plus_one(session, l, k, n, dtype):
    """a column of the factor set to nan: no entry of that product column compares greater than any other, the sign stays +1
    (both routes guard the read of the winning row), the component row is nan, every other row is exact"""
    P, M = C.integer_rotation(l, k, n)
    c = k // 2
    Mn = M.astype(np.float64)
    Mn[:, c] = np.nan
    want, want_signs = C.flip_reference((P @ M).astype(np.float64))
    got, signs = session.rotate_panel(P.astype(dtype), Mn)
    keep = np.arange(k) != c
    assert signs[c] == 1.0 and np.isnan(got[c]).all()
    assert np.array_equal(signs[keep], want_signs[keep])
    assert got[keep].tobytes() == want[keep].astype(dtype).tobytes()


@pytest.mark.parametrize("dtype", DTYPES)
def test_gaussian_panel_within_the_product_bound(session, dtype):
    """f64: |got - sign * (P @ M)| <= 2 l 2^-53 (|P| @ |M|) elementwise -- the gamma_l bound of a dot product, doubled for the
    reference's own error; f32 (the product is accumulated in f64 and rounded once): within one ulp of the f64 reference
    rounded to f32.  The signs are the reference's: every column's maximum is clear of the bound (CPU test)."""
    l, k, n = C.GAUSSIAN_SHAPE
    P, M, Y, absprod = C.gaussian_rotation(np.dtype(dtype).name)
    want, want_signs = C.flip_reference(Y)
    got, signs = session.rotate_panel(P, M)
    assert np.array_equal(signs, want_signs)
    bound = C.rotation_error_bound(np.dtype(dtype).name, l, Y, absprod).T
    ref = want.astype(dtype).astype(np.float64) if dtype == np.float32 else want
    err = np.abs(got.astype(np.float64) - ref)
    print(f"{np.dtype(dtype).name}: largest error / bound {float((err / bound).max()):.3f}")
    assert np.all(err <= bound)


def test_refusals(session):
    P, M = C.integer_rotation(16, 1, 17)
    with pytest.raises(Exception, match="rotate_panel"):
        session.rotate_panel(P[:, :1].astype(np.float32), np.ones((1, 2)))       # k > l
    got, _ = session.rotate_panel(P.astype(np.float32), M.astype(np.float64))   # (the handle still works)
    assert got.shape == (1, 17)
