"""The restatement of normalize / log1p / line statistics (tests/preproc_ref.py) against itself and against the data the
reference's own tests hold, and the preconditions of the fixtures the GPU test (test_gpu_preproc_edges.py) runs.  CPU only."""
import numpy as np
import pytest
import scipy.sparse as sp

import masked_stats_ref as M
import preproc_ref as P
import sapca_oracle as O

DTYPES = [np.float32, np.float64]


def _small_fixtures(dt):
    """(name, ptr, idx, val, m, n): every small matrix the GPU test uses, specials included"""
    out = [("special", *P.special_fixture(dt)), ("special, transposed", *P.special_fixture(dt, transposed=True))]
    ptr, idx, val, m, n, _ = P.normalize_special_values(dt)
    out.append(("normalize specials", ptr, idx, val, m, n))
    ptr, idx, val, m, n = P.ragged_fixture(dt)
    keep = np.flatnonzero(np.diff(ptr) < 200)            # (the literal loops are slow: the rows below 200 entries)
    lens = np.diff(ptr)[keep]
    sel = np.concatenate([np.arange(ptr[r], ptr[r + 1]) for r in keep]).astype(np.int64)
    out.append(("ragged, short rows", np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), idx[sel], val[sel], len(keep), n))
    z = np.zeros(0, np.int64)
    out.append(("nnz = 0", np.zeros(4, np.int64), z, np.zeros(0, dt), 3, 5))
    out.append(("one entry", np.array([0, 1]), np.array([2]), np.array([-2.5], dt), 1, 4))
    out.append(("n = 1", np.array([0, 1, 1, 2, 3]), np.array([0, 0, 0]), np.array([1.0, np.nan, 3.0], dt), 4, 1))
    return out


def test_long_double_is_wider_than_double():
    assert np.finfo(np.longdouble).nmant >= 63


@pytest.mark.parametrize("dt", DTYPES)
def test_vectorised_statistics_equal_the_literal_loops(dt):
    for name, ptr, idx, val, m, n in _small_fixtures(dt):
        for direction in (P.ROW, P.COLUMN):
            got, want = P.stats(ptr, idx, val, m, n, direction), P.ref_stats(ptr, idx, val, m, n, direction)
            for k, what in enumerate(("sum", "sum_squared", "nonzero")):
                assert P.same_bits(got[k], want[k]), f"{name}, direction {direction}: {what}"
            for k, what in ((3, "min"), (4, "max")):   # (a zero's sign is not specified: fmin may return either zero)
                assert P.same_values(got[k], want[k]), f"{name}, direction {direction}: {what}"


@pytest.mark.parametrize("dt", DTYPES)
def test_vectorised_normalize_and_log1p_equal_the_literal_loops(dt):
    rng = np.random.default_rng(0)
    for name, ptr, idx, val, m, n in _small_fixtures(dt):
        assert P.same_bits(P.log1p(val), P.ref_log1p_normalize(val)), name
        for direction, ln in ((P.ROW, m), (P.COLUMN, n)):
            sums = rng.uniform(-1.0, 50.0, ln)
            sums[::5] = [0.0, np.nan, np.inf, 5e-324, -np.inf, 1.7e308, -0.0][: len(sums[::5])] + [1.0] * max(0, len(sums[::5]) - 7)
            for target in (1e4, 1e-20, 0.0, -1.0, np.inf):
                got, want = P.normalize(ptr, idx, val, sums, target, direction), P.ref_normalize(ptr, idx, val, sums, target, direction)
                assert P.same_bits(got, want), f"{name}, direction {direction}, target {target}"
    ptr, idx, val, m, n, sums = P.normalize_special_values(dt)
    assert P.same_bits(P.normalize(ptr, idx, val, sums, 1.0, P.ROW), P.ref_normalize(ptr, idx, val, sums, 1.0, P.ROW))


@pytest.mark.parametrize("dt", DTYPES)
def test_the_corrected_restatements_agree(dt):
    """oracle.stats_csr, oracle.log1p_csr and the masked_stats_ref chunk functions carry the same semantics"""
    for name, ptr, idx, val, m, n in _small_fixtures(dt):
        assert P.same_bits(O.log1p_csr(val), P.log1p(val)), name
        for direction in (P.ROW, P.COLUMN):
            want = P.ref_stats(ptr, idx, val, m, n, direction)
            with np.errstate(all="ignore"):
                got = O.stats_csr(ptr, idx, val, m, n, direction)
            for k in (0, 1, 2):
                assert P.same_bits(np.asarray(got[k], want[k].dtype), want[k]), f"{name}, direction {direction}, output {k}"
            assert P.same_values(got[3], want[3]) and P.same_values(got[4], want[4]), f"{name}, direction {direction}"
        rng = np.random.default_rng(5)
        for fn, lit, ln in ((M.min_max_row_chunk, M.ref_min_max_row_chunk, m), (M.min_max_col_chunk, M.ref_min_max_col_chunk, n)):
            start = (rng.normal(0, 3, ln).astype(dt), rng.normal(0, 3, ln).astype(dt))
            start[0][::4], start[1][1::4] = np.nan, np.inf
            a, b = fn(ptr, idx, val, m, n, tuple(x.copy() for x in start)), lit(ptr, idx, val, m, n, tuple(x.copy() for x in start))
            assert P.same_values(a[0], b[0]) and P.same_values(a[1], b[1]), f"{name}: {fn.__name__}"


def test_the_reference_test_vectors(golden):
    g = golden("ref_pins_preproc.npz")
    A = sp.coo_matrix((g["norm_vals"], (g["norm_rows"], g["norm_cols"])), shape=(3, 3)).tocsr()
    A.sort_indices()
    ptr, idx, val = A.indptr.astype(np.int64), A.indices.astype(np.int64), A.data
    for fn in (P.normalize, P.ref_normalize):
        assert np.abs(fn(ptr, idx, val, g["norm_col_sums"], float(g["norm_target"]), P.COLUMN) - g["norm_expected_col"]).max() < float(g["norm_tol"])
        assert np.abs(fn(ptr, idx, val, g["norm_row_sums"], float(g["norm_target"]), P.ROW) - g["norm_expected_row"]).max() < float(g["norm_tol"])
    for fn in (P.stats, P.ref_stats):
        B = sp.csr_matrix(g["nz_dense"])
        args = (B.indptr.astype(np.int64), B.indices.astype(np.int64), B.data, *B.shape)
        np.testing.assert_array_equal(fn(*args, P.COLUMN)[2], g["nz_col"])
        np.testing.assert_array_equal(fn(*args, P.ROW)[2], g["nz_row"])
        B = sp.csr_matrix(g["sum_dense"])
        args = (B.indptr.astype(np.int64), B.indices.astype(np.int64), B.data, *B.shape)
        sc, _, _, loc, hic = fn(*args, P.COLUMN)
        sr, _, _, lor, hir = fn(*args, P.ROW)
        np.testing.assert_array_equal(sc, g["sum_col"])
        np.testing.assert_array_equal(sr, g["sum_row"])
        assert loc[0] == g["min_col0"] and hic[0] == g["max_col0"] and lor[2] == g["min_row2"] and hir[2] == g["max_row2"]


def test_min_max_semantics_in_words():
    nan, inf = np.nan, np.inf
    big = np.finfo(np.float32).max
    ptr, idx = np.array([0, 2, 4, 5, 7, 7]), np.array([0, 1, 0, 1, 0, 0, 1])
    val = np.array([nan, 1.0, 2.0, nan, inf, -inf, nan], np.float32)
    for fn in (P.min_max, lambda *a: P.ref_stats(*a)[3:]):
        lo, hi = fn(ptr, idx, val, 5, 2, P.ROW)
        assert np.isnan(lo[0]) and np.isnan(hi[0])                 # NaN first: the row is (NaN, NaN)
        assert (lo[1], hi[1]) == (2.0, 2.0)                        # NaN later: never wins
        assert (lo[2], hi[2]) == (inf, inf)                        # +inf alone: min is +inf in the ROW direction
        assert (lo[3], hi[3]) == (-inf, -inf)
        assert (lo[4], hi[4]) == (big, -big)                       # no entries
        ptr2, idx2, val2 = np.array([0, 1, 2, 3]), np.array([0, 0, 1]), np.array([nan, 3.0, inf], np.float32)
        lo, hi = fn(ptr2, idx2, val2, 3, 3, P.COLUMN)
        assert (lo[0], hi[0]) == (3.0, 3.0)                        # COLUMN: NaN first does not matter
        assert (lo[1], hi[1]) == (big, inf)                        # +inf alone: min stays T::MAX
        assert (lo[2], hi[2]) == (big, -big)


def test_ulp_distance():
    T = np.float32
    want = np.array([1.0, 1.0, np.inf, np.nan, 0.0, -np.inf], np.longdouble)
    got = np.array([1.0, np.nextafter(T(1), T(2)), np.inf, np.nan, 0.0, 5.0], T)
    np.testing.assert_array_equal(P.ulp_distance(got, want, T), [0, 1, 0, 0, 0, np.inf])
    w = np.longdouble(1) + np.longdouble(2.0) ** -25            # a quarter of an ulp above 1
    assert P.ulp_distance(np.array([1.0], T), np.array([w]), T)[0] == 0.25
    assert P.ulp_distance(np.array([np.nan], T), np.array([w]), T)[0] == np.inf


def test_log1p_reference_rounds_once():
    for T in DTYPES:
        eps = np.finfo(T).eps
        v = np.array([0.0, -0.0, eps / 4, -eps / 4, np.finfo(T).smallest_subnormal, -1.0, -2.0, np.inf, np.nan, 1.0], T)
        got = P.log1p(v)
        assert got[:5].tolist() == [0.0] * 5 and not np.signbit(got[1])      # ln(T(1) + v) with 1 + v == 1 in T, not a true log1p
        assert got[5] == -np.inf and np.isnan(got[6]) and got[7] == np.inf and np.isnan(got[8])
        assert P.ulp_distance(got, P.log1p_longdouble(v), T).max() <= 0.5


def test_stride_fixture_preconditions():
    ptr, idx, ival, m, n = P.stride_fixture()
    lens, nnz = np.diff(ptr), int(ptr[-1])
    assert m == 33_000 > 2 * P.ROW_WAVES and n == 3000
    assert nnz > 2 * P.ENTRY_THREADS and nnz % 256 != 0
    assert (lens[::97] == 0).all() and lens[-1] > 0 and lens[20_000] == 2500 == lens[32_900]
    body = np.delete(lens, np.r_[np.arange(0, m, 97), 20_000, 32_900])
    assert body.min() >= 110 and body.max() <= 170
    rows = np.repeat(np.arange(m), lens)
    assert idx.min() >= 0 and idx.max() < n
    inner = np.ones(nnz, bool)
    inner[ptr[:-1][lens > 0]] = False
    assert (np.diff(idx)[inner[1:]] > 0).all()                         # ascending, distinct columns within every row
    s, q = P.int_line_sums(ptr, idx, ival, m, n, P.ROW)
    assert q.max() < 2 ** 24 and (ival == 0).any() and (ival < 0).any()  # f32 holds every value, sum and sum of squares exactly
    sc, qc = P.int_line_sums(ptr, idx, ival, m, n, P.COLUMN)
    assert max(np.abs(sc).max(), qc.max()) < 2 ** 53
    np.testing.assert_array_equal(s, np.bincount(rows, weights=ival, minlength=m))
    turn = np.minimum(np.arange(nnz) // P.ENTRY_THREADS, 2)
    for j in (0, n // 2, n - 1):                                        # a column has entries in every turn of the per-entry kernels
        assert set(turn[idx == j].tolist()) == {0, 1, 2}
    for bounds, seed in ((P.STRIDE_ROW_TURNS, 1), (P.STRIDE_COL_THIRDS, 2)):
        sums = P.stride_sums(bounds, seed)
        assert (sums > 0).mean() > 0.9
        for lo, hi in zip(bounds[:-1], bounds[1:]):                     # every special class in every turn
            part = sums[lo:hi]
            with np.errstate(all="ignore"):
                assert (part == 0).any() and (part < 0).any() and np.isnan(part).any() and (part == np.inf).any()
                assert np.isinf(P.STRIDE_TARGETS[0] / part[part > 0]).any() and (P.STRIDE_TARGETS[1] / part[part > 0] == 0).sum() >= 2


def test_wide_fixture_preconditions():
    ptr, idx, ival, m, n = P.wide_fixture()
    assert m == 300 and n == 40_000 > 2 * P.ROW_WAVES
    cnt = np.bincount(idx, minlength=n)
    assert (cnt == 0).sum() >= n // 101 and cnt[12_345] == m and cnt.max() == m
    s, q = P.int_line_sums(ptr, idx, ival, m, n, P.COLUMN)
    assert max(np.abs(s).max(), q.max()) < 2 ** 24 and (ival == 0).any() and (ival < 0).any()


@pytest.mark.parametrize("dt", DTYPES)
def test_ragged_and_special_fixture_preconditions(dt):
    ptr, idx, val, m, n = P.ragged_fixture(dt)
    lens = np.diff(ptr)
    assert n == 6000 and sorted(set(lens.tolist())) == sorted(P.RAGGED_LENGTHS) and m == 3 * len(P.RAGGED_LENGTHS)
    assert np.isfinite(val).all() and (val < 0).any() and (val > 0).any() and np.abs(val).max() / np.abs(val).min() > 1e5
    fi = np.finfo(dt)
    for transposed in (False, True):
        ptr, idx, val, m, n = P.special_fixture(dt, transposed)
        lens = np.diff(ptr)
        pure = np.bincount(idx, minlength=n) if transposed else lens      # the lines that are special_rows: S's rows, S^T's columns
        assert (pure > 64).sum() >= 3 and (pure <= 5).sum() >= 24 and (pure == 0).any()
        inner = np.ones(len(val), bool)
        inner[ptr[:-1][lens > 0]] = False
        assert (np.diff(idx)[inner[1:]] > 0).all()
    rows = P.special_rows(dt)

    def some(pred):
        return any(len(r) and pred(r) for r in rows)
    assert some(lambda r: (r == np.inf).all()) and some(lambda r: (r == -np.inf).all()) and some(lambda r: np.isnan(r).all())
    assert some(lambda r: np.isnan(r[0]) and not np.isnan(r[1:]).all() and len(r) > 1)
    assert some(lambda r: not np.isnan(r[0]) and np.isnan(r[1:]).any())
    assert some(lambda r: (r == fi.max).any() and (r == -fi.max).any())
    assert some(lambda r: ((r != 0) & (np.abs(r) < fi.tiny)).all())
    assert some(lambda r: (r == 0).all() and np.signbit(r).any() and not np.signbit(r).all())
    for special in (np.isnan, lambda x: x == np.inf, lambda x: x == -np.inf, lambda x: x == fi.max, lambda x: (x == 0) & np.signbit(x)):
        for pos in (0, 64, 70):                                         # first value / lane 0's later share / another lane
            assert any(len(r) == 130 and special(r[pos]) and not special(np.delete(r, pos)).any() for r in rows)
    ptr, idx, val, m, k, sums = P.normalize_special_values(dt)
    with np.errstate(all="ignore"):
        out = P.normalize(ptr, idx, val, sums, 1.0, P.ROW)
    sub = (out != 0) & (np.abs(out) < fi.tiny) & ~((val != 0) & (np.abs(val) < fi.tiny))
    assert sub.sum() >= 5 and (np.isinf(out) & np.isfinite(val)).any()
    cls = P.log1p_classes(dt)
    assert (np.abs(cls["tiny"]) <= fi.eps / 4).all() and ((cls["subnormal"] != 0) & (np.abs(cls["subnormal"]) < fi.tiny)).all()
    assert ((cls["minus_one_to_zero"] >= -1) & (cls["minus_one_to_zero"] < 0)).all() and (cls["positive"] > 0).all()
