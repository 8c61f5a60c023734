"""The matrices of tests/lanczos_cases.py meet the conditions tests/test_gpu_lanczos_products.py relies on, checked without a GPU:
the gap sigma_k / sigma_k+1 of the operator each fit sees is at least 1.5 (the angle assertions have no escape clause), the
edited row lengths and the boundary columns are present, and the route predicates restated from the sources send every case
where its test says it goes."""
import numpy as np
import pytest

import exact_sums_ref
import lanczos_cases as C

# (case, centred, f32): every operator a fit of the GPU file sees
FITS = [("L", False, False), ("L", False, True), ("S", False, False), ("S", False, True), ("W2", False, False), ("W2", False, True),
        ("W2", True, False), ("W2", True, True), ("W3", False, False), ("T", False, False), ("P2", False, False), ("P2", False, True),
        ("P3m", False, False), ("P3m", False, True), ("LIM", False, False)]      # (Lsmall: statistics only, no angle is asserted)


@pytest.mark.parametrize("name,centred,f32", FITS)
def test_gap_is_at_least_one_and_a_half(name, centred, f32):
    k = C.k_of(name)
    s, _, gap = C.reference(name, centred, f32, vectors=not centred)
    print(f"{name}{' centred' if centred else ''}{' f32' if f32 else ''}: sigma_{k} / sigma_{k + 1} = {gap:.3f}")
    assert gap >= 1.5
    assert np.all(s[:k - 1] / s[1:k] > 1.02)      # (|C V^T| = I needs the leading values apart from each other as well)


def test_svds_agrees_with_the_dense_answer():
    A = C.matrix("S")
    s_gram, vt_gram = C.gram_svd(A, C.K)
    s_svds, vt_svds = C.svds_svd(A, C.K)
    np.testing.assert_allclose(s_svds, s_gram, rtol=1e-12)
    s_dense = np.linalg.svd(A.toarray(), compute_uv=False)
    np.testing.assert_allclose(s_gram, s_dense[:C.K + 1], rtol=1e-12)
    np.testing.assert_allclose(np.abs(vt_svds @ vt_gram.T), np.eye(C.K), atol=1e-9)


def test_fast_exact_sums_are_the_exact_sums():
    A = C.matrix("S")
    s, sq, cnt, sabs = C.exact_column_sums(A)
    want_s, want_sq = exact_sums_ref.exact_column_sums(A.indices, A.data, A.shape[1])
    assert np.array_equal(s, want_s) and np.array_equal(sq, want_sq)
    assert np.array_equal(cnt, np.bincount(A.indices, minlength=A.shape[1]))
    small = C.matrix("Lsmall")       # (values of very different magnitudes)
    s, sq, _, _ = C.exact_column_sums(small)
    keep = small.indices < 40
    want_s, want_sq = exact_sums_ref.exact_column_sums(small.indices[keep], small.data[keep], 40)
    assert np.array_equal(s[:40], want_s) and np.array_equal(sq[:40], want_sq)


@pytest.mark.parametrize("name,centred", [(name, False) for name in C.EDGE_ROW_CASES] + [("W2", True)])
def test_edited_rows(name, centred):
    A = C.matrix(name, centred)
    m, n = A.shape
    lens = np.diff(A.indptr)
    assert tuple(lens[:len(C.ROW_LENGTHS)]) == C.ROW_LENGTHS
    assert A.has_canonical_format and A.indices.min() >= 0 and A.indices.max() == n - 1
    assert C.ROW_LENGTHS == (0, 1, 63, 64, 65, 192, 193, 255, 256, 257, 320, 448, 449, 512, 513) and C.UNROLL_FROM == 193
    assert lens[C.empty_row(m)] == 0 and 0 < C.empty_row(m) < m - 1 and lens[m - 1] > 0
    row = A.indices[A.indptr[C.FULL_ROW]:A.indptr[C.FULL_ROW + 1]]
    if name == "W2":
        s, t = C.slices_of(n)
        assert (s, t) == (10000, 2)
        assert {0, 9999, 10000, n - 1} <= set(row.tolist())
    else:
        assert np.array_equal(row, np.arange(n))
    body = lens[C.FULL_ROW + 1:]
    body = body[body > 0]
    print(f"{name}: other rows hold {body.min()}..{body.max()} entries")
    assert body.min() >= C.UNROLL_FROM      # every other row runs the four-wide loop


def test_three_slices():
    A = C.matrix("W3")
    assert C.slices_of(40000) == (13334, 3) and 40000 - 2 * 13334 == 13332
    row = set(A.indices[A.indptr[C.FULL_ROW]:A.indptr[C.FULL_ROW + 1]].tolist())
    assert {13333, 13334, 26667, 26668, 0, 39999} <= row
    lens = np.diff(A.indptr)
    assert lens[C.empty_row(4200)] == 0 and lens[-1] > 0 and np.sort(lens)[1] >= C.UNROLL_FROM


@pytest.mark.parametrize("name,edges", [("P2", [3849, 3850]), ("P3m", [5333, 5334, 10667, 10668]), ("LIM", [6399, 6400, 12799, 12800])])
def test_pass_boundaries(name, edges):
    A = C.matrix(name)
    m, n = A.shape
    passes, nc = C.stats_passes(n)
    assert C.STATS_PASS_COLS == 7680 and passes == len(edges) // 2 + 1
    assert edges == [c for p in range(1, passes) for c in (p * nc - 1, p * nc)]
    cnt = np.bincount(A.indices, minlength=n)
    assert np.all(cnt[edges] > 0) and cnt[n - 1] > 0 and cnt[C.EMPTY_COLUMN] == 0
    assert np.count_nonzero(cnt == 0) == 1
    rows = [set(A.indices[A.indptr[r]:A.indptr[r + 1]].tolist()) for r in (5, 6, 7)]
    assert set(edges) <= rows[0]
    assert set(edges[1::2]) <= rows[1] and not set(edges[0::2]) & rows[1]
    assert set(edges[0::2]) <= rows[2] and not set(edges[1::2]) & rows[2]
    assert n - 1 in A.indices[A.indptr[m - 1]:A.indptr[m]]
    lens = np.diff(A.indptr)
    assert lens[C.empty_row(m)] == 0 and lens[m - 1] > 0
    if name == "P3m":
        mask = C.mask_of(name)
        kept = C.used(name)
        assert int(mask.sum()) == 4013 == kept.shape[1]
        klen = np.diff(kept.indptr)
        print(f"P3m: {klen[klen > 0].min()}..{klen.max()} kept entries a row")


def test_routes():
    """the kernels of the two products of a step, by the predicates restated in lanczos_cases.py"""
    def shape(name, centred=False):
        A = C.used(name, centred)
        return A.shape[0], A.shape[1], A.nnz
    assert (C.LDS_X_COLS, C.LDSX_MIN_ROWS, C.LONG_ROW_ENTRIES, C.SLICED_MIN_ROWS, C.SCATTER_MIN_ROWS) == (19200, 4096, 256, 1024, 4096)
    m, n, nnz = shape("L")
    assert nnz >= 256 * m and n * 8 <= 150 * 1024 and n <= m and m >= 4096
    assert C.products(m, n, nnz) == ("ldsx", "scatter")
    assert C.products(m, n, nnz, no_lds=True) == ("row", "scatter")
    assert C.products(m, n, nnz, transpose_switch=True) == ("ldsx", "sliced") and C.slices_of(m)[1] == 1 and C.sliced_rpw(n) == 1
    assert C.stats_passes(n) == (1, n)
    m, n, nnz = shape("S")
    assert m < 4096 and nnz >= 256 * m and nnz >= 256 * n and n >= 1024
    assert C.products(m, n, nnz) == ("sliced", "sliced") and C.slices_of(n)[1] == 1 and C.slices_of(m)[1] == 1
    assert C.products(m, n, nnz, no_lds=True) == ("row", "row")
    for centred in (False, True):
        m, n, nnz = shape("W2", centred)
        assert n > m and nnz >= 256 * m and n >= 4096 and m * 8 <= 150 * 1024
        assert C.products(m, n, nnz) == ("ldsx", "slice_grid") and C.slices_of(n) == (10000, 2)
        assert C.products(m, n, nnz, no_grid=True) == ("ldsx", "sliced") and C.sliced_rpw(m) == 2
        assert C.products(m, n, nnz, no_lds=True) == ("row", "row")
    m, n, nnz = shape("W3")
    assert nnz >= 256 * m
    assert C.products(m, n, nnz) == ("ldsx", "slice_grid") and C.products(m, n, nnz, no_grid=True) == ("ldsx", "sliced")
    assert C.sliced_rpw(m) * (3 + 1) <= 64
    m, n, nnz = shape("T")
    assert C.products(m, n, nnz) == ("ldsx", "scatter") and m / 4096 > 4.8
    assert C.products(m, n, nnz, transpose_switch=True) == ("ldsx", "slice_grid") and C.slices_of(m) == (10000, 2)
    assert C.products(m, n, nnz, transpose_switch=True, no_grid=True) == ("ldsx", "sliced") and C.sliced_rpw(n) == 2
    assert C.sliced_rpw(n) * (2 + 1) <= 64
    for name, passes in (("P2", 2), ("P3m", 3), ("LIM", 3)):
        m, n, nnz = shape(name)
        assert n <= m and m >= 4096 and n * 8 <= 150 * 1024
        assert C.products(m, n, nnz) == ("ldsx", "scatter")
        assert C.stats_passes(C.matrix(name).shape[1])[0] == passes
    m, n, nnz = shape("LIM")
    assert n == 19200 and m >= n and not C.scatter_route(m, n + 1, nnz + 1)
    A1 = C.matrix("LIM+1")
    assert A1.shape == (m, n + 1) and A1.nnz == nnz + 1 and A1[m - 1, n] == 2.0 ** -20
    assert C.products(m, n + 1, nnz + 1) == ("sliced", "slice_grid")


def test_the_small_columns_case():
    A, B = C.matrix("L"), C.matrix("Lsmall")
    assert np.array_equal(A.indices, B.indices) and np.abs(B.data).max() == 1e3
    small = B.indices < 10
    assert np.array_equal(B.data[small], A.data[small] * 1e-9) and np.count_nonzero(B.data != np.where(small, A.data * 1e-9, A.data)) == 1
