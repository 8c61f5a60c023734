"""Engine::normalize with its extras filled in (sapca_normalize_panel_ex_*): the slab-summing, centring and column-summing read
pass of the fused Gram (gram.hip gramv_kernel<..., SRC = true>, 64 and 128 columns), materialize() ahead of the plain and the
wide Gram, the vector R^-T (P^T w) (chol.hip) and the factors R1 / R2 the f64 small SVD multiplies, on the integer panels of
tests/dense_tail_cases.py -- the sum of the slabs, mu sv^T, w^T P and the Gram are exact there in both dtypes, so a dropped
slab, row or tile is a change of bits (NONE) or of 1 / 200 in the Gram (QR), not something a tolerance could hide.

Margins of the two QR checks that compare with the returned Q (dense_tail_cases.MARGIN, measured on the reference, not on the
kernel: 8 x what numpy.linalg.qr in f64, rounded once to the dtype, leaves on the same panels):
    |P - Q (R2 R1)| <= margin * l eps (|Q| @ |R2 R1|):     numpy leaves 295.05 (f64), 0.012402 (f32)  ->  2361, 0.09922
    |vec - w^T Q|   <= margin * rows eps (|w| @ |Q|):      numpy leaves 0.020156 (f64), 0.00072228 (f32)  ->  0.1613, 0.005779
(rows eps: the gamma bound of a dot product over the rows, as l eps is that of one over the columns.)  R1 and R2 arrive as
l x l matrices: what lies outside l x l in the padded device buffers is not visible through the entry point, and the f64 small
SVD reads none of it either (engine.cpp small_svd_qr_jacobi multiplies the l x l corners)."""
import numpy as np
import pytest
import torch  # noqa: F401  (first: one HIP runtime per process)

import dense_tail_cases as C
from sapca import ops
from sapca import PowerIterationNormalizer as PIN

pytestmark = pytest.mark.gpu

DTYPES = [(np.float32, 5e-6), (np.float64, 1e-12)]     # (the bounds of test_normalizer_qr_orthonormal_same_span: 20 x these)


@pytest.fixture(scope="module")
def session():
    return ops.Session()


def _same(a, b):
    return all((a[key] is None and b[key] is None) or (np.asarray(a[key]).tobytes() == np.asarray(b[key]).tobytes())
               for key in ("panel", "vec", "r1", "r2", "regularised"))


def _upper_positive(R):
    return np.array_equal(np.triu(R), R) and np.all(np.diag(R) > 0)


def _check_qr(out, P, w, l, rows, dtype, tol, passes, tag):
    T = np.dtype(dtype)
    P64 = P.astype(np.float64)
    G = P64.T @ P64                                   # (exact: integers below 2^53, CPU test)
    R1, R2, Q = out["r1"], out["r2"], out["panel"].astype(np.float64)
    assert out["regularised"] == 0, tag
    assert np.isfinite(Q).all() and _upper_positive(R1), tag
    if passes == 1:
        assert not R2.any(), tag
        R = R1
    else:
        assert _upper_positive(R2), tag
        R = R2 @ R1
    d = np.sqrt(np.diag(G))
    chol = float((np.abs(R1.T @ R1 - G) / ((l + 1) * 2.0 ** -52 * np.outer(d, d))).max())
    orth = float(np.abs(Q.T @ Q - np.eye(l)).max())
    res = C.residual_ratio(P64, Q, R, T)
    w1 = np.ones(rows, np.int64) if w is None else w
    vec = C.vec_ratio(out["vec"].astype(np.float64), w1, Q, T)
    m_res, m_vec = C.MARGIN[T.name]
    print(f"{tag}: |R1^T R1 - G| / bound {chol:.3f}, |Q^T Q - I| {orth:.2e} (bound {20 * tol:.0e}), residual {res:.3e} "
          f"(margin {m_res}), vec {vec:.3e} (margin {m_vec})")
    assert chol <= 1.0, tag
    assert orth <= 20 * tol, tag
    assert res <= m_res, tag
    assert vec <= m_vec, tag


@pytest.mark.parametrize("dtype,tol", DTYPES)
@pytest.mark.parametrize("l,rows,nsplit", C.normalize_shapes())
def test_extras_on_integer_slabs(session, l, rows, nsplit, dtype, tol):
    """l = 60 / 128: the fused Gram (ld = 64; four waves, which materialises a panel staged in place first); l = 40 / 150: the
    plain and the wide-pair Gram behind materialize().  nsplit 1 .. 12 at 200 rows: with the f32 unroll of four slabs the head
    not full, full, remainders of one to three and one full group; with the f64 unroll of two every parity (of one at 128
    columns every count).  One slab is staged in the panel buffer, several in a buffer of their own.  rows 1 and 17: less
    than a row tile and one over; 8200: past the 512 x 16 rows the workgroups cover in one trip.  Each with and without
    mu sv^T, with and without weights.
    NONE: the panel and w^T P bit for bit.  QR with one pass and with its two, rows >= l: R1^T R1 against the exact Gram at
    Higham's bound with gamma doubled for the blocked order, (l + 1) 2^-52 sqrt(G_ii G_jj); triangular factors with positive
    diagonals, no floored pivot; Q^T Q = I; P = Q R2 R1 and vec = w^T Q at the margins of the module docstring.  rows < l: no l
    orthonormal columns exist (test_gpu_normaliser_chain.py): bytes between two calls only.  Every call twice: the same bytes."""
    case = C.normalize_case(l, rows, nsplit)
    slabs = case["slabs"].astype(dtype)
    for centred in (False, True):
        mu, sv = (case["mu"], case["sv"]) if centred else (None, None)
        P = C.panel_of(case, centred)
        for w in (None, case["w"]):
            tag = f"l {l} rows {rows} nsplit {nsplit} {np.dtype(dtype).name}{' centred' if centred else ''}{' weighted' if w is not None else ''}"
            none = session.normalize_panel_ex(slabs, PIN.NONE, mu=mu, sv=sv, w=w)
            assert none["panel"].tobytes() == P.astype(dtype).tobytes(), tag
            wsum = P.sum(0) if w is None else w @ P
            assert none["vec"].tobytes() == wsum.astype(dtype).tobytes(), tag
            assert none["regularised"] == 0 and not none["r1"].any() and not none["r2"].any(), tag
            assert _same(none, session.normalize_panel_ex(slabs, PIN.NONE, mu=mu, sv=sv, w=w)), tag
            for passes in (1, 0):
                out = session.normalize_panel_ex(slabs, PIN.QR, passes=passes, mu=mu, sv=sv, w=w)
                assert _same(out, session.normalize_panel_ex(slabs, PIN.QR, passes=passes, mu=mu, sv=sv, w=w)), tag
                if rows >= l:
                    _check_qr(out, P, w, l, rows, dtype, tol, 1 if passes == 1 else 2, f"{tag} passes {passes or 2}")


@pytest.mark.parametrize("dtype,tol", DTYPES)
def test_outputs_are_optional(session, dtype, tol):
    """without vec_out, r1 and r2 the same panel comes back (the factors then go to the normaliser's own scratch slot)"""
    case = C.normalize_case(60, 200, 3)
    slabs = case["slabs"].astype(dtype)
    full = session.normalize_panel_ex(slabs, PIN.QR, mu=case["mu"], sv=case["sv"], w=case["w"])
    bare = session.normalize_panel_ex(slabs, PIN.QR, mu=case["mu"], sv=case["sv"], w=case["w"], want_vec=False, want_r=False)
    assert bare["vec"] is None and bare["r1"] is None and bare["panel"].tobytes() == full["panel"].tobytes()
    with pytest.raises(Exception, match="mu and sv"):
        session.normalize_panel_ex(slabs, PIN.QR, mu=case["mu"])


@pytest.mark.parametrize("dtype,tol", DTYPES)
def test_rank_deficient_panel_is_regularised(session, dtype, tol):
    """two equal columns at l = 60: the factorisation floors a pivot and says so; every output stays finite; same bytes twice"""
    case = C.normalize_case(60, 200, 3, rank_deficient=True)
    slabs = case["slabs"].astype(dtype)
    out = session.normalize_panel_ex(slabs, PIN.QR, mu=case["mu"], sv=case["sv"], w=case["w"])
    assert out["regularised"] >= 1
    for key in ("panel", "vec", "r1", "r2"):
        assert np.isfinite(out[key]).all(), key
    assert _same(out, session.normalize_panel_ex(slabs, PIN.QR, mu=case["mu"], sv=case["sv"], w=case["w"]))
