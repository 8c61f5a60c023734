"""Row selection on a device-resident matrix (-m gpu): sapca_select_rows_csr_device_* and ResidentCsr.select_rows.

The reference for the arrays is scipy's A[rows] on the host matrix (indices sorted as uploaded) and the comparison is
exact: offsets and indices equal, values equal as bit patterns.  Statistics of a selection are held to the bar of the
masked-statistics tests (counts exact, sums within 1e-12 relative); fits on a selection to the bars the same fits have
on a full matrix (f32 randomized: subspace angle < 1e-4, singular values 1e-4; f64 Lanczos: 1e-4, 1e-5; projection
2e-4 / 1e-9 of the largest coordinate)."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import masked_stats_ref as M
import sapca
import sapca_oracle as O
from sapca import _lib as L
from sapca import ops, synth
from sapca import PowerIterationNormalizer as PIN
from sapca import SVDMethod

pytestmark = pytest.mark.gpu

BITS = {np.dtype(np.float32): np.uint32, np.dtype(np.float64): np.uint64}


def _resident(A, sess=None):
    sess = sess or ops.Session()
    return sess, sess.upload(A.indptr, A.indices, A.data, A.shape[0], A.shape[1])


def _host(R):
    """(offsets, indices, values) of a ResidentCsr, copied to the host"""
    d = R.as_device_csr()
    return d.row_offsets.cpu().numpy(), d.col_indices.cpu().numpy(), d.values.cpu().numpy()


def _check_selection(S, A, rows, what):
    """S against scipy's A[rows], exactly"""
    rows = np.asarray(rows, dtype=np.int64)
    want = A[rows] if rows.size else sp.csr_matrix((0, A.shape[1]), dtype=A.dtype)
    ptr, idx, val = _host(S)
    assert S.shape == (rows.size, A.shape[1]) and S.nnz == want.nnz, what
    assert ptr.dtype == np.int64 and idx.dtype == np.int32 and val.dtype == A.dtype
    np.testing.assert_array_equal(ptr, want.indptr.astype(np.int64), err_msg=f"{what}: offsets")
    np.testing.assert_array_equal(idx, want.indices.astype(np.int32), err_msg=f"{what}: indices")
    bits = BITS[np.dtype(A.dtype)]
    np.testing.assert_array_equal(val.view(bits), np.ascontiguousarray(want.data).view(bits), err_msg=f"{what}: value bits")


def _mixed(m, n, density, seed, dtype):
    """like _mixed of test_gpu_masked_stats.py (stored zeros, negative values, an empty row 7, an empty column 3), with a
    few NaN (one with a payload), +-inf and -0.0 planted among the stored values"""
    rng = np.random.default_rng(seed)
    D = (rng.random((m, n)) < density) * rng.normal(1.5, 4.0, (m, n))
    stored = (D != 0) | (rng.random((m, n)) < 0.01)
    stored[7, :] = False
    stored[:, 3] = False
    r, c = np.nonzero(stored)
    data = D[r, c].astype(dtype)
    bits = BITS[np.dtype(dtype)]
    spots = rng.choice(data.size, 12, replace=False)
    data[spots[0:3]] = np.nan
    data[spots[3:5]] = np.inf
    data[spots[5:7]] = -np.inf
    data[spots[7:10]] = -0.0
    data.view(bits)[spots[10]] = bits(0x7FC00123) if dtype == np.float32 else bits(0x7FF8000000000123)   # a NaN with a payload
    data.view(bits)[spots[11]] = bits(0xFFC00001) if dtype == np.float32 else bits(0xFFF8000000000001)   # .. and a negative one
    A = sp.csr_matrix((data, (r, c)), shape=(m, n))
    A.sort_indices()
    assert A.nnz == data.size and np.diff(A.indptr)[7] == 0
    return A


# ------------------------------------------------------------------ 1. exact selection
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_exact_selection(dt):
    m, n = 2600, 900
    A = _mixed(m, n, 0.05, 11, dt)
    sess, R = _resident(A)
    rng = np.random.default_rng(3)
    src_before = [x.tobytes() for x in _host(R)]
    cases = {
        "a 50 % mask": rng.random(m) < 0.5,
        "all rows": np.arange(m),
        "no rows": np.zeros(0, np.int64),
        "an all-false mask": np.zeros(m, bool),
        "one row": [1234],
        "reversed order": np.arange(m)[::-1],
        "a random permutation": rng.permutation(m),
        "a bootstrap draw of 2m rows": rng.integers(0, m, 2 * m),
        "empty rows only": [7, 7, 7, 7, 7],
        "starts and ends with the empty row": np.concatenate([[7, 7], rng.integers(0, m, 300), [7]]),
    }
    for what, rows in cases.items():
        S = R.select_rows(rows)
        idx = np.flatnonzero(rows) if np.asarray(rows).dtype == np.bool_ else np.asarray(rows, dtype=np.int64)
        _check_selection(S, A, idx, what)
        if what == "a bootstrap draw of 2m rows":
            assert S.nnz > R.nnz
        if what == "all rows":
            for got, src in zip(_host(S), src_before):
                assert got.tobytes() == src                     # the output equals the source
            assert (S.d_ptr, S.d_idx, S.d_val) != (R.d_ptr, R.d_idx, R.d_val)
        if what in ("no rows", "an all-false mask"):
            assert S.nnz == 0 and _host(S)[0].tolist() == [0]
    assert [x.tobytes() for x in _host(R)] == src_before         # the source is byte-identical after all of them


# ------------------------------------------------------------------ 2. skew and span boundaries
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_one_long_row_among_short_and_empty_ones(dt):
    """one row of 60,000 entries (more than 7 spans of at most 8192 output positions; select.hip's is 4096) between rows of
    0-6 entries and a run of 301 empty rows: spans that start and end inside the long row, a long row that starts in the
    middle of a 16-byte group, runs of empty rows on either side of it"""
    m, n, long_row, long_len = 600, 70_000, 50, 60_000
    rng = np.random.default_rng(8)
    lens = rng.integers(0, 7, m)
    lens[100:401] = 0
    lens[long_row] = long_len
    cols = np.concatenate([np.sort(rng.choice(n, k, replace=False)) for k in lens])
    ptr = np.concatenate([[0], np.cumsum(lens)])
    A = sp.csr_matrix((rng.normal(0.5, 2.0, cols.size).astype(dt), cols, ptr), shape=(m, n))
    A.sort_indices()
    sess, R = _resident(A)
    short = np.concatenate([np.arange(0, 50), np.arange(401, 600)])
    empty = np.arange(100, 401)
    cases = {
        "the long row first": np.concatenate([[long_row], short]),
        "the long row last": np.concatenate([short, [long_row]]),
        "the long row twice in a row": np.concatenate([short[:37], [long_row, long_row], short[37:]]),
        "the long row between runs of empty rows": np.concatenate([short[:5], empty, [long_row], empty[::-1], short[5:9]]),
        "the long row after one entry, between empty rows": np.concatenate([[401 + int(np.argmax(lens[401:] == 1))], empty[:3], [long_row], empty]),
        "a random permutation": rng.permutation(m),
        "the long row alone": [long_row],
    }
    for what, rows in cases.items():
        _check_selection(R.select_rows(rows), A, rows, what)


def test_more_rows_than_one_workgroup_stages():
    """a span of output positions that crosses more rows than the fill stages in LDS at a time (2048): rows of 0 or 1
    entries, and 5000 empty rows in the middle of the list"""
    m, n = 9000, 64
    rng = np.random.default_rng(2)
    lens = (rng.random(m) < 0.5).astype(np.int64)
    lens[2000:7000] = 0
    cols = rng.integers(0, n, int(lens.sum()))
    A = sp.csr_matrix((rng.normal(size=cols.size).astype(np.float32), cols, np.concatenate([[0], np.cumsum(lens)])), shape=(m, n))
    sess, R = _resident(A)
    for what, rows in (("in order", np.arange(m)), ("permuted", rng.permutation(m)), ("a bootstrap", rng.integers(0, m, 3 * m))):
        _check_selection(R.select_rows(rows), A, rows, what)


# ------------------------------------------------------------------ 3. errors and lifetimes
def _raw_select(sess, R, rows_ptr, n_rows, outs):
    return L.load().sapca_select_rows_csr_device_f32(*R._args(), rows_ptr, C.c_uint64(n_rows), *outs)


def test_errors_leave_the_handle_usable():
    m, n = 300, 80
    A = _mixed(m, n, 0.1, 4, np.float32)
    sess, R = _resident(A)
    with pytest.raises(L.SapcaError) as e:
        R.select_rows([5, 299, 300, 1])
    assert e.value.status == L.ERR_ARG and str(e.value) == "select_rows: row index 300 at position 2 is out of range (m = 300)"
    nnz_out, dp, di, dv = C.c_uint64(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    outs = [C.byref(nnz_out), C.byref(dp), C.byref(di), C.byref(dv)]
    st = _raw_select(sess, R, None, 3, outs)                                     # rows == NULL with n_rows > 0
    assert st == L.ERR_ARG and b"rows is NULL" in L.load().sapca_last_error(sess._h)
    rows = np.array([1, 2], dtype=np.uint64)
    rp = rows.ctypes.data_as(C.POINTER(C.c_uint64))
    for missing in range(4):                                                    # each null output pointer
        o = list(outs)
        o[missing] = None
        st = _raw_select(sess, R, rp, 2, o)
        assert st == L.ERR_ARG and b"null output pointer" in L.load().sapca_last_error(sess._h)
    S = R.select_rows([10, 11, 12])                                             # a valid call on the same handle
    _check_selection(S, A, [10, 11, 12], "after the refused calls")
    with pytest.raises(L.SapcaError, match="own selection") as e:               # the selection cannot be its own source
        S.select_rows([0])
    assert e.value.status == L.ERR_ARG
    _check_selection(S, A, [10, 11, 12], "after the refused self-selection")     # .. and is left as it was
    with pytest.raises(ValueError, match="Row mask length"):
        R.select_rows(np.ones(m + 1, bool))
    with pytest.raises(ValueError, match="negative row index"):
        R.select_rows([0, -1])


def test_a_second_selection_replaces_the_first_and_the_source_stays():
    m, n = 1500, 400
    A = _mixed(m, n, 0.05, 9, np.float64)
    sess, R = _resident(A)
    before = [x.tobytes() for x in _host(R)]
    rng = np.random.default_rng(1)
    a, b = rng.permutation(m)[:700], rng.integers(0, m, 2000)
    S1 = R.select_rows(a)
    _check_selection(S1, A, a, "first")
    S2 = R.select_rows(b)                                                        # (larger: the buffers grow)
    _check_selection(S2, A, b, "second")
    S3 = R.select_rows(a[:10])                                                   # (smaller: they are reused)
    _check_selection(S3, A, a[:10], "third")
    assert (S3.d_ptr, S3.d_idx, S3.d_val) == (S2.d_ptr, S2.d_idx, S2.d_val)      # one set of buffers per handle
    assert [x.tobytes() for x in _host(R)] == before
    # the selection's values are its own: log1p on them leaves the source alone
    S3.log1p()
    assert [x.tobytes() for x in _host(R)] == before
    with np.errstate(invalid="ignore", divide="ignore"):
        want = O.log1p_csr(A[a[:10]].data)
    np.testing.assert_allclose(_host(S3)[2], want, rtol=1e-13, equal_nan=True)


class _InHandleOf:
    """a Session-shaped view of an estimator's handle (not owned): uploads and selections in the handle that fits"""

    def __init__(self, est):
        self._est, self._h = est, est._h

    _csr_args = ops.Session._csr_args
    upload = ops.Session.upload


def test_the_uploads_statistics_survive_a_selection():
    """the column statistics gathered during the upload are exact sums: a fit of the uploaded arrays that finds them gives
    the same mean_ bit for bit every time.  A selection in between -- and a fit of that selection -- must not drop them
    (the fit would fall back to the f64 sums of the transposed matrix, which round differently)."""
    m, n, k, p, q = 3000, 600, 6, 6, 2
    ptr, idx, val = (x.cpu().numpy() for x in synth.gapped_csr(m, n, 0.08, k, seed=42, dtype=torch.float32))
    A = sp.csr_matrix((val, idx.astype(np.int64), ptr.astype(np.int64)), shape=(m, n))
    om = synth.gaussian_panel(n, k + p, 42).numpy()
    est = sapca.SparsePCABuilder.new().n_components(k).svd_method(SVDMethod.Random(p, q, PIN.QR)).build().set_omega(om)
    R = _InHandleOf(est).upload(A.indptr, A.indices, A.data, m, n)
    est.fit(R.as_device_csr())
    mean0, sing0 = est.mean_(np.float64).copy(), est.singular_values_(np.float64).copy()
    rows = np.random.default_rng(0).permutation(m)[:2000]
    S = R.select_rows(rows)
    est.fit(R.as_device_csr())
    assert est.mean_(np.float64).tobytes() == mean0.tobytes()
    est.fit(S.as_device_csr())                                                  # a fit of the selection in between
    sub = A[rows]
    np.testing.assert_allclose(est.mean_(np.float64), np.asarray(sub.mean(0)).ravel(), rtol=1e-5, atol=1e-7)
    S = R.select_rows(rows[::-1])                                               # .. and the selection it prepared is replaced
    est.fit(R.as_device_csr())
    assert est.mean_(np.float64).tobytes() == mean0.tobytes()
    np.testing.assert_allclose(est.singular_values_(np.float64), sing0, rtol=1e-5)


# ------------------------------------------------------------------ 4. statistics agree across the two features
def _same_stats(got, want, what):
    np.testing.assert_array_equal(got[2], want[2], err_msg=f"{what}: count")
    for j, name in ((0, "sum"), (1, "sumsq")):
        scale = max(1.0, float(np.abs(want[j]).max(initial=0)))
        np.testing.assert_allclose(got[j], want[j], rtol=1e-12, atol=1e-12 * scale, err_msg=f"{what}: {name}")


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_statistics_of_a_selection_equal_the_masked_statistics_of_the_source(dt):
    m, n = 2600, 900
    rng = np.random.default_rng(11)
    D = (rng.random((m, n)) < 0.05) * rng.normal(1.5, 4.0, (m, n))               # (finite values: sums are compared)
    stored = (D != 0) | (rng.random((m, n)) < 0.01)
    stored[7, :] = False
    stored[:, 3] = False
    r, c = np.nonzero(stored)
    A = sp.csr_matrix((D[r, c].astype(dt), (r, c)), shape=(m, n))
    A.sort_indices()
    sess, R = _resident(A)
    mask = rng.random(m) < 0.5
    col_want = R.masked_stats(ops.COLUMN, mask)                                   # (sum, sumsq, count, var)
    row_all = R.stats(ops.ROW)                                                    # (sum, sumsq, nonzero, min, max)
    S = R.select_rows(mask)
    _same_stats(S.stats(ops.COLUMN), col_want, "COLUMN of the selection against the row-masked source")
    got_rows = S.stats(ops.ROW)
    _same_stats(got_rows, tuple(x[mask] for x in row_all), "ROW of the selection against the source's kept rows")
    np.testing.assert_array_equal(got_rows[3], row_all[3][mask])                  # min / max: the same values
    np.testing.assert_array_equal(got_rows[4], row_all[4][mask])
    # and against the host restatement, so that the two do not merely agree with each other
    ptr, idx, val = A.indptr.astype(np.int64), A.indices.astype(np.int64), A.data
    _same_stats(S.stats(ops.COLUMN), M.masked_stats(ptr, idx, val, m, n, M.COLUMN, mask), "COLUMN against the restatement")
    _same_stats(S.masked_stats(ops.COLUMN), col_want, "masked_stats of the selection, no mask")


# ------------------------------------------------------------------ 5. fit on the subset, project everything
@pytest.fixture(scope="module")
def mito():
    """the matrix of test_end_to_end_mito_fraction_then_gene_filter_then_masked_pca, preprocessed in HBM the same way"""
    m, n = 4000, 900
    ptr, idx, val = (x.cpu().numpy() for x in synth.gapped_csr(m, n, 0.05, 8, seed=21, dtype=torch.float32))
    ptr, idx = ptr.astype(np.int64), idx.astype(np.int64)
    sess, R = _resident(sp.csr_matrix((val, idx, ptr), shape=(m, n)))
    R.normalize(R.stats(ops.ROW)[0], 1e3, ops.ROW).log1p()
    v32 = R.values()
    return dict(m=m, n=n, ptr=ptr, idx=idx, sess=sess, R=R, v32=v32, A64=sp.csr_matrix((v32.astype(np.float64), idx, ptr), shape=(m, n)))


def _host_slice(A, rows):
    S = A[rows]
    S.sort_indices()
    return S.indptr.astype(np.int64), S.indices.astype(np.int64), S.data


def _gene_mask(var, top):
    order = np.argsort(-var, kind="stable")
    assert var[order[top - 1]] > var[order[top]] * (1 + 1e-6)                     # the cut is not a near tie
    genes = np.zeros(var.size, bool)
    genes[order[:top]] = True
    return genes


def _gap(A, rows, genes, k):
    """sigma_k / sigma_(k+1) of the centred operator a masked fit on A[rows][:, genes] sees (dense SVD on the host)"""
    D = A[rows].toarray()[:, genes]
    sv = np.linalg.svd(D - D.mean(0), compute_uv=False)
    return sv[k - 1] / sv[k]


def _subset_rows(name, mt):
    m, R = mt["m"], mt["R"]
    rng = np.random.default_rng(5)
    if name == "mito cells":
        mito_genes = np.zeros(mt["n"], bool)
        mito_genes[:40] = True
        frac = R.sum_row_masked(mito_genes) / np.maximum(R.stats(ops.ROW)[0], 1e-30)
        thr = np.quantile(frac, 0.8)
        assert np.abs(frac - thr).min() > 1e-9 * thr                              # no cell sits on the cut
        return frac < thr                                                         # a mask
    if name == "60 % mask":
        return rng.random(m) < 0.6
    assert name == "bootstrap of 3000"
    return rng.integers(0, m, 3000)


# k: the matrix has 9 planted clusters, so 8 centred directions stand above the background -- except under the mito cut,
# which drops the cells richest in columns 0..39, i.e. the cluster that owns those columns: 8 clusters, 7 directions
# are left there (the 8th singular value belongs to the background and has no gap behind it: nothing to compare).
@pytest.mark.parametrize("name,k", [("mito cells", 7), ("60 % mask", 8), ("bootstrap of 3000", 8)])
def test_randomized_fit_on_a_selection_then_projection_of_the_full_matrix(mito, name, k):
    mt, p, q, top = mito, 6, 2, 300
    m, n, R, A64 = mt["m"], mt["n"], mt["R"], mt["A64"]
    sel = _subset_rows(name, mt)
    rows = np.flatnonzero(sel) if sel.dtype == np.bool_ else sel
    S = R.select_rows(sel)
    sptr, sidx, sval = _host_slice(A64, rows)
    np.testing.assert_array_equal(_host(S)[0], sptr)
    gvar = S.var_col_masked(np.ones(rows.size, bool))
    if sel.dtype == np.bool_:                                                     # the same variances without the selection
        np.testing.assert_allclose(gvar, R.var_col_masked(sel), rtol=1e-12, atol=1e-12)
    genes = _gene_mask(gvar, top)
    np.testing.assert_array_equal(genes, _gene_mask(M.var_col_masked(sptr, sidx, sval, rows.size, n, np.ones(rows.size, bool)), top))
    assert _gap(A64, rows, genes, k) > 1.3, "the subset has no spectral gap behind its k-th direction"
    om = synth.gaussian_panel(top, k + p, 5).numpy()
    est = (sapca.MaskedSparsePCABuilder.new().n_components(k).mask(genes)
           .svd_method(SVDMethod.Random(p, q, PIN.QR)).build().set_omega(om))
    est.fit(S.as_device_csr())
    ref = O.fit(sptr, sidx, sval, rows.size, n, n_components=k, n_oversamples=p, n_power_iterations=q, omega=om, mask=genes)
    ang = O.subspace_angle(est.components_(np.float64), ref.components)
    print(f"{name}: {rows.size} rows, subspace angle {ang:.3e}, singular values off by "
          f"{np.abs(est.singular_values_(np.float64) / ref.singular_values - 1).max():.3e}")
    assert ang < 1e-4
    np.testing.assert_allclose(est.singular_values_(np.float64), ref.singular_values, rtol=1e-4)
    np.testing.assert_allclose(est.mean_(np.float64), ref.mean, atol=1e-5)
    # every cell through the model fitted on the subset
    t = est.transform(R.as_device_csr()).cpu().numpy()
    comps, mean = est.components_(np.float64), est.mean_(np.float64)
    tw = O.transform_masked_fast(mt["ptr"], mt["idx"], A64.data, m, n, comps, mean, True, genes)
    assert t.shape == (m, k)
    print(f"{name}: projection of all {m} rows off by {np.abs(t - tw).max() / max(1.0, float(np.abs(tw).max())):.3e} of the largest coordinate")
    np.testing.assert_allclose(t, tw, atol=2e-4 * max(1.0, float(np.abs(tw).max())))


def test_f64_lanczos_fit_on_a_permuted_selection_then_projection_of_the_full_matrix(mito):
    """Lanczos fits are uncentred (quirk Q1): the raw operator has 9 planted directions, so k = 9 is where its gap is"""
    mt, k = mito, 9
    m, n, A64 = mt["m"], mt["n"], mt["A64"]
    sess, R = _resident(A64)
    rows = np.random.default_rng(77).permutation(m)[:2500]
    S = R.select_rows(rows)
    sptr, sidx, sval = _host_slice(A64, rows)
    _check_selection(S, A64, rows, "permutation of 2500 rows")
    sv = np.linalg.svd(A64[rows].toarray(), compute_uv=False)
    assert sv[k - 1] / sv[k] > 1.3
    est = sapca.SparsePCABuilder.new().n_components(k).svd_method(SVDMethod.Lanczos()).build()
    est.fit(S.as_device_csr())
    ref = O.fit(sptr, sidx, sval, rows.size, n, n_components=k, method="LANCZOS")
    ang = O.subspace_angle(est.components_(np.float64), ref.components)
    print(f"f64 Lanczos on 2500 permuted rows: subspace angle {ang:.3e}")
    assert ang < 1e-4
    np.testing.assert_allclose(est.singular_values_(np.float64), ref.singular_values, rtol=1e-5)
    np.testing.assert_allclose(est.singular_values_(np.float64), sv[:k], rtol=1e-5)
    t = est.transform(R.as_device_csr()).cpu().numpy()
    tw = O.transform_sparse(mt["ptr"], mt["idx"], A64.data, m, n, est.components_(np.float64), est.mean_(np.float64), True)
    print(f"f64 Lanczos: projection of all {m} rows off by {np.abs(t - tw).max() / max(1.0, float(np.abs(tw).max())):.3e} of the largest coordinate")
    np.testing.assert_allclose(t, tw, atol=1e-9 * max(1.0, float(np.abs(tw).max())))
