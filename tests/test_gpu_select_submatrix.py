"""Row and column selection on a device-resident matrix (-m gpu): sapca_select_submatrix_csr_device_* and
ResidentCsr.select / select_cols.

The reference for the arrays is tests/submatrix_ref.py (numpy; held to scipy's A[rows][:, cols] and eliminate_zeros by the
CPU tests) and the comparison is exact: offsets and indices equal, values equal as bit patterns.  Statistics are held to
the bar of the masked-statistics tests (counts exact, sums within 1e-12 relative); fits on a selection to the bars the same
fits have in tests/test_gpu_select_rows.py (f32 randomized: subspace angle < 1e-4, singular values 1e-4; f64 Lanczos:
1e-4, 1e-5; projection 2e-4 / 1e-9 of the largest coordinate)."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import submatrix_ref as SR
import sapca
import sapca_oracle as O
from sapca import _lib as L
from sapca import ops, synth
from sapca import PowerIterationNormalizer as PIN
from sapca import SVDMethod

pytestmark = pytest.mark.gpu

BITS = {np.dtype(np.float32): np.uint32, np.dtype(np.float64): np.uint64}
# select.hip keeps the column map in LDS up to 3072 words (kSubMapWords): 98,304 columns; wider matrices read it from memory
MAP_LDS_COLUMNS = 98_304


def _resident(A, sess=None):
    sess = sess or ops.Session()
    return sess, sess.upload(A.indptr, A.indices, A.data, A.shape[0], A.shape[1])


def _host(R):
    """(offsets, indices, values) of a ResidentCsr, copied to the host"""
    d = R.as_device_csr()
    return d.row_offsets.cpu().numpy(), d.col_indices.cpu().numpy(), d.values.cpu().numpy()


def _bytes(R):
    return [x.tobytes() for x in _host(R)]


def _row_index(rows, m):
    if rows is None:
        return None
    rows = np.asarray(rows)
    return np.flatnonzero(rows) if rows.dtype == np.bool_ else rows.astype(np.int64)


def _check(S, A, rows, mask, drop, what):
    """S against the reference's A[rows][:, mask] (without stored zeros under `drop`), exactly"""
    ptr, idx, val, nc = SR.select_submatrix(A.indptr, A.indices, A.data, A.shape[1], _row_index(rows, A.shape[0]), mask, drop)
    gp, gi, gv = _host(S)
    assert S.shape == (ptr.size - 1, nc) and S.nnz == val.size, f"{what}: shape {S.shape}, nnz {S.nnz}; want {(ptr.size - 1, nc)}, {val.size}"
    assert gp.dtype == np.int64 and gi.dtype == np.int32 and gv.dtype == A.dtype
    np.testing.assert_array_equal(gp, ptr, err_msg=f"{what}: offsets")
    np.testing.assert_array_equal(gi, idx, err_msg=f"{what}: indices")
    bits = BITS[np.dtype(A.dtype)]
    np.testing.assert_array_equal(gv.view(bits), np.ascontiguousarray(val).view(bits), err_msg=f"{what}: value bits")


def _mixed(m, n, density, seed, dtype):
    """_mixed of test_gpu_select_rows.py: stored zeros, negative values, an empty row 7, an empty column 3, a few NaN (one
    with a payload), +-inf and -0.0 planted among the stored values"""
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
    m, n = 2600, 900                                                              # (900 is not a multiple of 32)
    A = _mixed(m, n, 0.05, 11, dt)
    sess, R = _resident(A)
    rng = np.random.default_rng(3)
    src_before = _bytes(R)
    perm = rng.permutation(m)
    row_cases = {
        "every row": None,
        "a 50 % row mask": rng.random(m) < 0.5,
        "a permutation": perm,
        "a bootstrap draw of 2m rows": rng.integers(0, m, 2 * m),
        "the empty row five times": [7] * 5,
        "no rows": np.zeros(0, np.int64),
    }
    col_cases = {
        "every column": None,
        "a 40 % mask": rng.random(n) < 0.4,
        "an all-true mask": np.ones(n, bool),
        "an all-false mask": np.zeros(n, bool),
        "only the empty column 3": np.arange(n) == 3,
        "one column": np.arange(n) == 517,
        "every 64th column": np.arange(n) % 64 == 0,
    }
    for rwhat, rows in row_cases.items():
        for cwhat, mask in col_cases.items():
            for drop in (False, True):
                what = f"{rwhat} x {cwhat}{' without stored zeros' if drop else ''}"
                S = R.select(rows, mask, drop_stored_zeros=drop)
                _check(S, A, rows, mask, drop, what)
                if mask is not None and not mask.any():
                    assert S.shape[1] == 0 and S.nnz == 0 and not _host(S)[0].any(), what
    # identity: the source's bytes at other addresses
    S = R.select()
    assert _bytes(S) == src_before and (S.d_ptr, S.d_idx, S.d_val) != (R.d_ptr, R.d_idx, R.d_val)
    # no mask, no flag: the bytes of select_rows; an all-true mask: the bytes of no mask
    want = _bytes(R.select_rows(perm))
    assert _bytes(R.select(perm)) == want
    assert _bytes(R.select(perm, np.ones(n, bool))) == want
    # the same arguments, the same bytes
    mask = col_cases["a 40 % mask"]
    first = _bytes(R.select(perm, mask, drop_stored_zeros=True))
    assert _bytes(R.select(perm, mask, drop_stored_zeros=True)) == first
    # select_cols, and integer columns
    assert _bytes(R.select_cols(mask)) == _bytes(R.select(cols=np.flatnonzero(mask)))
    assert _bytes(R) == src_before                                              # the source is byte-identical after all of them


# ------------------------------------------------------------------ 2. skew and span boundaries
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_one_long_row_among_short_and_empty_ones(dt):
    """the matrix and the row orders of test_gpu_select_rows.py's test of the same name: one row of 60,000 entries (more
    than 14 spans of 4096 gathered positions) between rows of 0-6 entries and a run of 301 empty rows"""
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
    row_cases = {
        "the long row first": np.concatenate([[long_row], short]),
        "the long row last": np.concatenate([short, [long_row]]),
        "the long row twice in a row": np.concatenate([short[:37], [long_row, long_row], short[37:]]),
        "the long row between runs of empty rows": np.concatenate([short[:5], empty, [long_row], empty[::-1], short[5:9]]),
        "the long row after one entry, between empty rows": np.concatenate([[401 + int(np.argmax(lens[401:] == 1))], empty[:3], [long_row], empty]),
        "a random permutation": rng.permutation(m),
        "the long row alone": [long_row],
        "every row": None,
    }
    long_cols = A.indices[A.indptr[long_row]:A.indptr[long_row + 1]]
    in_long = np.zeros(n, bool)
    in_long[long_cols] = True
    one_per_span = np.zeros(n, bool)
    one_per_span[long_cols[2048::4096]] = True                                    # one entry of the long row in every 4096
    col_cases = {
        "a 50 % mask": rng.random(n) < 0.5,
        "no column of the long row": ~in_long,
        "only the long row's columns": in_long,
        "one entry in every 4096 of the long row": one_per_span,
    }
    for rwhat, rows in row_cases.items():
        for cwhat, mask in col_cases.items():
            _check(R.select(rows, mask), A, rows, mask, False, f"{rwhat} x {cwhat}")
    _check(R.select(row_cases["a random permutation"], None, drop_stored_zeros=True), A, row_cases["a random permutation"], None, True,
           "a random permutation without stored zeros (there are none)")


def test_more_rows_than_one_workgroup_stages():
    """a span of gathered positions that crosses more rows than the two kernels stage in LDS at a time (1024): rows of 0 or
    1 entries, 5000 empty rows in the middle of the list; a third of the values are stored zeros"""
    m, n = 9000, 64
    rng = np.random.default_rng(2)
    lens = (rng.random(m) < 0.5).astype(np.int64)
    lens[2000:7000] = 0
    cols = rng.integers(0, n, int(lens.sum()))
    vals = rng.normal(size=cols.size).astype(np.float32) * (rng.random(cols.size) < 0.67)
    A = sp.csr_matrix((vals, cols, np.concatenate([[0], np.cumsum(lens)])), shape=(m, n))
    assert A.nnz == cols.size
    sess, R = _resident(A)
    mask = rng.random(n) < 0.5
    for what, rows in (("in order", None), ("permuted", rng.permutation(m)), ("a bootstrap", rng.integers(0, m, 3 * m))):
        _check(R.select(rows, mask), A, rows, mask, False, what)
        _check(R.select(rows, None, drop_stored_zeros=True), A, rows, None, True, what + " without stored zeros")
        _check(R.select(rows, mask, drop_stored_zeros=True), A, rows, mask, True, what + " masked, without stored zeros")


# ------------------------------------------------------------------ 3. wide matrices
@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("n", [MAP_LDS_COLUMNS, MAP_LDS_COLUMNS + 1, 400_000],
                         ids=["widest_lds_map", "narrowest_map_in_memory", "n400000"])
def test_wide_matrices(n, dt):
    m = 2000
    rng = np.random.default_rng(n % 1000)
    lens = rng.integers(4, 17, m)
    cols = np.concatenate([np.sort(rng.choice(n, k, replace=False)) for k in lens])
    cols[-1] = n - 1                                                               # (the last column is used: row m - 1's largest)
    A = sp.csr_matrix((rng.normal(size=cols.size).astype(dt), cols, np.concatenate([[0], np.cumsum(lens)])), shape=(m, n))
    sess, R = _resident(A)
    high = np.arange(n) > (2 ** 18 if n > 2 ** 18 + 3000 else n - 3000)              # (n = 400,000: every kept column above 2^18)
    masks = {"a 30 % mask": rng.random(n) < 0.3, "only high columns": high}
    assert masks["only high columns"][cols].any()
    rows = rng.permutation(m)[:1500]
    for what, mask in masks.items():
        _check(R.select(None, mask), A, None, mask, False, f"n = {n}, every row x {what}")
        _check(R.select(rows, mask), A, rows, mask, False, f"n = {n}, 1500 permuted rows x {what}")


# ------------------------------------------------------------------ 4. refusals
def _raw(R, suf, rows, n_rows, mask, mask_len, flags, outs):
    rp = None if rows is None else rows.ctypes.data_as(C.POINTER(C.c_uint64))
    mp = None if mask is None else mask.ctypes.data_as(C.POINTER(C.c_uint8))
    return getattr(L.load(), f"sapca_select_submatrix_csr_device_{suf}")(*R._args(), rp, n_rows, mp, mask_len, flags, *outs)


def test_refusals_leave_the_selection_and_the_handle_as_they_were():
    m, n = 300, 80
    A = _mixed(m, n, 0.1, 4, np.float32)
    sess, R = _resident(A)
    mask = np.random.default_rng(0).random(n) < 0.5
    S = R.select([10, 11, 12], mask)
    kept = _bytes(S)
    ncols, nnz_out, dp, di, dv = C.c_uint64(), C.c_uint64(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    outs = [C.byref(ncols), C.byref(nnz_out), C.byref(dp), C.byref(di), C.byref(dv)]
    rows = np.array([1, 2], dtype=np.uint64)
    m8 = np.ascontiguousarray(mask, dtype=np.uint8)

    def refused(status, fragment):
        assert status == L.ERR_ARG
        msg = L.load().sapca_last_error(sess._h).decode()
        assert fragment in msg, msg
        assert _bytes(S) == kept                                                  # the previous selection's bytes
        T = R.select([5, 4], mask, drop_stored_zeros=True)                      # .. and the next valid call succeeds
        _check(T, A, [5, 4], mask, True, f"after the refusal '{fragment}'")
        assert _bytes(R.select([10, 11, 12], mask)) == kept

    refused(_raw(R, "f32", rows, 2, m8[:-1], n - 1, 0, outs), f"select_submatrix: the column mask has {n - 1} entries, the matrix {n} columns")
    long_mask = np.ones(n + 1, np.uint8)
    refused(_raw(R, "f32", rows, 2, long_mask, n + 1, 0, outs), f"select_submatrix: the column mask has {n + 1} entries, the matrix {n} columns")
    bad = np.array([5, 299, 300, 1], dtype=np.uint64)
    refused(_raw(R, "f32", bad, 4, m8, n, 0, outs), "select_submatrix: row index 300 at position 2 is out of range (m = 300)")
    refused(_raw(R, "f32", None, m + 1, m8, n, 0, outs), "select_submatrix: rows is NULL with n_rows")
    refused(_raw(R, "f32", rows, 2, m8, n, 2, outs), "select_submatrix: unknown flag bits")
    refused(_raw(R, "f32", rows, 2, None, 0, 0x80000001, outs), "select_submatrix: unknown flag bits")
    for missing in range(5):                                                      # each null output pointer
        o = list(outs)
        o[missing] = None
        refused(_raw(R, "f32", rows, 2, m8, n, 0, o), "select_submatrix: null output pointer")
    S = R.select([10, 11, 12], mask)
    with pytest.raises(L.SapcaError, match="select_submatrix: the source is this handle's own selection") as e:
        S.select(cols=np.ones(S.shape[1], bool))
    assert e.value.status == L.ERR_ARG and _bytes(S) == kept
    with pytest.raises(L.SapcaError, match="select_rows: the source is this handle's own selection"):
        S.select_rows([0])                                                        # one selection per handle: select_rows refuses it too
    with pytest.raises(L.SapcaError, match=r"row index 300 at position 0 is out of range \(m = 300\)") as e:
        R.select([300], mask)
    assert e.value.status == L.ERR_ARG
    # the Python layer's own refusals reach no library call
    with pytest.raises(ValueError, match="Column mask length"):
        R.select(cols=np.ones(n + 1, bool))
    with pytest.raises(ValueError, match="strictly ascending"):
        R.select(cols=[3, 3])
    assert _bytes(S) == kept
    # n_rows <= m with rows == NULL is a prefix of the rows
    ok = _raw(R, "f32", None, 17, m8, n, 0, outs)
    assert ok == L.OK and ncols.value == int(mask.sum())
    T = ops.ResidentCsr(sess, (17, ncols.value), nnz_out.value, np.float32, dp.value, di.value, dv.value)
    _check(T, A, np.arange(17), mask, False, "rows == NULL, n_rows = 17")


# ------------------------------------------------------------------ 5. bookkeeping
class _InHandleOf:
    """a Session-shaped view of an estimator's handle (not owned): uploads and selections in the handle that fits"""

    def __init__(self, est):
        self._est, self._h = est, est._h

    _csr_args = ops.Session._csr_args
    upload = ops.Session.upload


def _gapped(m, n, k, seed):
    ptr, idx, val = (x.cpu().numpy() for x in synth.gapped_csr(m, n, 0.08, k, seed=seed, dtype=torch.float32))
    return sp.csr_matrix((val, idx.astype(np.int64), ptr.astype(np.int64)), shape=(m, n))


def _randomized(k, p, q, om):
    return sapca.SparsePCABuilder.new().n_components(k).svd_method(SVDMethod.Random(p, q, PIN.QR)).build().set_omega(om)


def test_the_uploads_statistics_survive_a_selection():
    """as in test_gpu_select_rows.py: a fit of the uploaded arrays that finds the upload's exact column sums gives the same
    mean_ bit for bit; a row-and-column selection in between, and a fit of it, must not drop them"""
    m, n, k, p, q = 3000, 600, 6, 6, 2
    A = _gapped(m, n, k, 42)
    est = _randomized(k, p, q, synth.gaussian_panel(n, k + p, 42).numpy())
    R = _InHandleOf(est).upload(A.indptr, A.indices, A.data, m, n)
    est.fit(R.as_device_csr())
    mean0, sing0, comp0 = est.mean_(np.float64).copy(), est.singular_values_(np.float64).copy(), est.components_(np.float64).copy()
    rng = np.random.default_rng(0)
    rows, mask = rng.permutation(m)[:2000], rng.random(n) < 0.5
    S = R.select(rows, mask)
    est.fit(R.as_device_csr())
    assert est.mean_(np.float64).tobytes() == mean0.tobytes()
    est2 = _randomized(k, p, q, synth.gaussian_panel(S.shape[1], k + p, 42).numpy())
    S2 = _InHandleOf(est2).upload(A.indptr, A.indices, A.data, m, n).select(rows, mask)
    est2.fit(S2.as_device_csr())                                                # (a fit of a selection, in a handle of its own)
    np.testing.assert_allclose(est2.mean_(np.float64), np.asarray(A[rows][:, np.flatnonzero(mask)].mean(0)).ravel(), rtol=1e-5, atol=1e-7)
    R.select(rows[::-1], mask, drop_stored_zeros=True)
    est.fit(R.as_device_csr())
    assert est.mean_(np.float64).tobytes() == mean0.tobytes()
    np.testing.assert_allclose(est.singular_values_(np.float64), sing0, rtol=1e-5)
    assert O.subspace_angle(est.components_(np.float64), comp0) < 1e-4


def test_a_new_selection_drops_the_preparation_made_of_the_previous_one():
    """fit_transform on a selection prepares it; a new selection of the same shape and entry count lands in the same
    buffers, and transform of it must see the new rows: the same numbers as on a fresh handle that never saw the first"""
    m, n, k, p, q = 3000, 600, 6, 6, 2
    A = _gapped(m, n, k, 17)
    rng = np.random.default_rng(1)
    rows, mask = rng.permutation(m)[:1800], rng.random(n) < 0.6
    om = synth.gaussian_panel(int(mask.sum()), k + p, 3).numpy()
    est = _randomized(k, p, q, om)
    R = _InHandleOf(est).upload(A.indptr, A.indices, A.data, m, n)
    S1 = R.select(rows, mask)
    t1 = est.fit_transform(S1.as_device_csr()).cpu().numpy()
    S2 = R.select(rows[::-1], mask)
    assert (S2.d_ptr, S2.d_idx, S2.d_val, S2.nnz, S2.shape) == (S1.d_ptr, S1.d_idx, S1.d_val, S1.nnz, S1.shape)
    t2 = est.transform(S2.as_device_csr()).cpu().numpy()
    fresh = _randomized(k, p, q, om)
    F = _InHandleOf(fresh).upload(A.indptr, A.indices, A.data, m, n)
    fresh.fit(F.select(rows, mask).as_device_csr())
    want = fresh.transform(F.select(rows[::-1], mask).as_device_csr()).cpu().numpy()
    scale = max(1.0, float(np.abs(want).max()))
    np.testing.assert_allclose(t2, want, atol=2e-4 * scale)
    assert np.abs(t1 - want).max() > 1e-2 * scale                                # (the stale preparation's answer is far away)
    np.testing.assert_allclose(t2, t1[::-1], atol=2e-4 * scale)


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_the_results_values_are_its_own(dt):
    m, n = 1500, 400
    A = _mixed(m, n, 0.05, 9, dt)
    sess, R = _resident(A)
    before = _bytes(R)
    rng = np.random.default_rng(1)
    rows, mask = rng.permutation(m)[:700], rng.random(n) < 0.5
    S = R.select(rows, mask, drop_stored_zeros=True)
    sub = SR.select_submatrix(A.indptr, A.indices, A.data, n, rows, mask, True)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        S.log1p()
        assert _bytes(R) == before
        np.testing.assert_allclose(_host(S)[2], O.log1p_csr(sub[2]), rtol=1e-6 if dt == np.float32 else 1e-13, equal_nan=True)
        S.normalize(np.ones(S.shape[0]), 10.0, ops.ROW)
    assert _bytes(R) == before
    S3 = R.select(rows[:10])                                                     # smaller: the same buffers
    assert (S3.d_ptr, S3.d_idx, S3.d_val) == (S.d_ptr, S.d_idx, S.d_val)
    _check(S3, A, rows[:10], None, False, "a third selection")


def test_a_handle_in_a_communicator_selects_locally():
    m, n = 500, 120
    A = _mixed(m, n, 0.08, 6, np.float32)
    calls = []

    def allreduce(sendbuf, recvbuf, count, dtype, user):
        calls.append(count)
        return 0

    est = _randomized(4, 4, 1, synth.gaussian_panel(n, 8, 1).numpy())
    est.comm_set_callback(1, 0, allreduce)
    R = _InHandleOf(est).upload(A.indptr, A.indices, A.data, m, n)
    seen = len(calls)
    rng = np.random.default_rng(2)
    rows, mask = rng.integers(0, m, 700), rng.random(n) < 0.5
    _check(R.select(rows, mask, drop_stored_zeros=True), A, rows, mask, True, "inside a 1-rank communicator")
    _check(R.select(rows), A, rows, None, False, "inside a 1-rank communicator, rows only")
    assert len(calls) == seen


# ------------------------------------------------------------------ 6. statistics agree across the features
def _same_stats(got, want, what):
    np.testing.assert_array_equal(got[2], want[2], err_msg=f"{what}: count")
    for j, name in ((0, "sum"), (1, "sumsq")):
        scale = max(1.0, float(np.abs(want[j]).max(initial=0)))
        np.testing.assert_allclose(got[j], want[j], rtol=1e-12, atol=1e-12 * scale, err_msg=f"{what}: {name}")


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_statistics_of_a_column_selection(dt):
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
    mask = rng.random(n) < 0.4
    mask[3] = True                                                                # (the empty column is kept)
    row_want = R.masked_stats(ops.ROW, mask)                                      # (sum, sumsq, count, var)
    col_all = R.stats(ops.COLUMN)                                                 # (sum, sumsq, nonzero, min, max)
    report = R.check()
    assert report.stored_zeros > 0
    S = R.select(cols=mask)
    assert S.shape == (m, int(mask.sum()))
    _same_stats(S.stats(ops.ROW), row_want, "ROW of the selection against the column-masked source")
    got_cols = S.stats(ops.COLUMN)
    _same_stats(got_cols, tuple(x[mask] for x in col_all), "COLUMN of the selection against the source's kept columns")
    np.testing.assert_array_equal(got_cols[3], col_all[3][mask])                  # min / max: the same values
    np.testing.assert_array_equal(got_cols[4], col_all[4][mask])
    assert S.check().canonical
    Z = R.select(drop_stored_zeros=True)
    zr = Z.check()
    assert zr.stored_zeros == 0 and zr.canonical and Z.nnz == R.nnz - report.stored_zeros and Z.shape == R.shape
    np.testing.assert_array_equal(Z.stats(ops.ROW)[2], np.asarray((A != 0).sum(1)).ravel())


# ------------------------------------------------------------------ 7. fits on a row-and-column selection
@pytest.fixture(scope="module")
def mito():
    """the matrix of test_gpu_select_rows.py's fit tests, preprocessed in HBM the same way"""
    m, n = 4000, 900
    ptr, idx, val = (x.cpu().numpy() for x in synth.gapped_csr(m, n, 0.05, 8, seed=21, dtype=torch.float32))
    ptr, idx = ptr.astype(np.int64), idx.astype(np.int64)
    sess, R = _resident(sp.csr_matrix((val, idx, ptr), shape=(m, n)))
    R.normalize(R.stats(ops.ROW)[0], 1e3, ops.ROW).log1p()
    v32 = R.values()
    return dict(m=m, n=n, ptr=ptr, idx=idx, sess=sess, R=R, v32=v32, A64=sp.csr_matrix((v32.astype(np.float64), idx, ptr), shape=(m, n)))


def _gene_mask(var, top):
    order = np.argsort(-var, kind="stable")
    assert var[order[top - 1]] > var[order[top]] * (1 + 1e-6)                     # the cut is not a near tie
    genes = np.zeros(var.size, bool)
    genes[order[:top]] = True
    return genes


def _sub(A, rows, genes):
    S = A[rows][:, np.flatnonzero(genes)]
    S.sort_indices()
    return S


@pytest.mark.parametrize("name,k", [("60 % mask", 8), ("bootstrap of 3000", 8)])
def test_randomized_fits_on_a_submatrix(mito, name, k):
    """SparsePCA on select(rows, cols = genes) and MaskedSparsePCA(genes) on select(rows) against ONE oracle fit: that of
    the host slice A[rows][:, genes] (a masked fit is the fit of the compacted matrix)"""
    mt, p, q, top = mito, 6, 2, 300
    m, n, R, A64 = mt["m"], mt["n"], mt["R"], mt["A64"]
    rng = np.random.default_rng(5)
    sel = rng.random(m) < 0.6 if name == "60 % mask" else rng.integers(0, m, 3000)
    rows = np.flatnonzero(sel) if sel.dtype == np.bool_ else sel
    S = R.select(sel)
    genes = _gene_mask(S.var_col_masked(np.ones(rows.size, bool)), top)
    H = _sub(A64, rows, genes)
    sv = np.linalg.svd(H.toarray() - H.toarray().mean(0), compute_uv=False)
    assert sv[k - 1] / sv[k] > 1.3, "the subset has no spectral gap behind its k-th direction"
    om = synth.gaussian_panel(top, k + p, 5).numpy()
    ref = O.fit(H.indptr.astype(np.int64), H.indices.astype(np.int64), H.data, rows.size, top, n_components=k, n_oversamples=p,
                n_power_iterations=q, omega=om)
    masked = (sapca.MaskedSparsePCABuilder.new().n_components(k).mask(genes)
              .svd_method(SVDMethod.Random(p, q, PIN.QR)).build().set_omega(om))
    masked.fit(S.as_device_csr())
    SC = R.select(sel, genes)
    _check(SC, sp.csr_matrix((mt["v32"], mt["idx"], mt["ptr"]), shape=(m, n)), sel, genes, False, name)
    plain = _randomized(k, p, q, om)
    plain.fit(SC.as_device_csr())
    for what, est in (("SparsePCA on select(rows, cols)", plain), ("MaskedSparsePCA on select(rows)", masked)):
        ang = O.subspace_angle(est.components_(np.float64), ref.components)
        print(f"{name}, {what}: subspace angle {ang:.3e}, singular values off by "
              f"{np.abs(est.singular_values_(np.float64) / ref.singular_values - 1).max():.3e}")
        assert ang < 1e-4, what
        np.testing.assert_allclose(est.singular_values_(np.float64), ref.singular_values, rtol=1e-4, err_msg=what)
        mean = est.mean_(np.float64)                                              # (a masked estimator's mean_ is n wide)
        np.testing.assert_allclose(mean[genes] if est is masked else mean, ref.mean, atol=1e-5, err_msg=what)
    # every cell's kept genes through the model fitted on the submatrix
    t = plain.transform(R.select_cols(genes).as_device_csr()).cpu().numpy()
    G = _sub(A64, np.arange(m), genes)
    tw = O.transform_sparse(G.indptr.astype(np.int64), G.indices.astype(np.int64), G.data, m, top, plain.components_(np.float64),
                            plain.mean_(np.float64), True)
    assert t.shape == (m, k)
    print(f"{name}: projection of all {m} rows off by {np.abs(t - tw).max() / max(1.0, float(np.abs(tw).max())):.3e} of the largest coordinate")
    np.testing.assert_allclose(t, tw, atol=2e-4 * max(1.0, float(np.abs(tw).max())))


def test_f64_lanczos_fit_on_a_submatrix(mito):
    """Lanczos fits are uncentred (quirk Q1): the raw operator has 9 planted directions; a 70 % column mask keeps them"""
    mt, k = mito, 9
    m, n, A64 = mt["m"], mt["n"], mt["A64"]
    sess, R = _resident(A64)
    rng = np.random.default_rng(77)
    rows, genes = rng.permutation(m)[:2500], rng.random(n) < 0.7
    S = R.select(rows, genes)
    _check(S, A64, rows, genes, False, "2500 permuted rows x a 70 % column mask")
    H = _sub(A64, rows, genes)
    nc = int(genes.sum())
    sv = np.linalg.svd(H.toarray(), compute_uv=False)
    assert sv[k - 1] / sv[k] > 1.3
    ref = O.fit(H.indptr.astype(np.int64), H.indices.astype(np.int64), H.data, rows.size, nc, n_components=k, method="LANCZOS")
    plain = sapca.SparsePCABuilder.new().n_components(k).svd_method(SVDMethod.Lanczos()).build()
    plain.fit(S.as_device_csr())
    masked = sapca.MaskedSparsePCABuilder.new().n_components(k).mask(genes).svd_method(SVDMethod.Lanczos()).build()
    masked.fit(R.select(rows).as_device_csr())
    for what, est in (("SparsePCA on select(rows, cols)", plain), ("MaskedSparsePCA on select(rows)", masked)):
        ang = O.subspace_angle(est.components_(np.float64), ref.components)
        print(f"f64 Lanczos, {what}: subspace angle {ang:.3e}")
        assert ang < 1e-4, what
        np.testing.assert_allclose(est.singular_values_(np.float64), ref.singular_values, rtol=1e-5, err_msg=what)
        np.testing.assert_allclose(est.singular_values_(np.float64), sv[:k], rtol=1e-5, err_msg=what)
    t = plain.transform(R.select_cols(genes).as_device_csr()).cpu().numpy()
    G = _sub(A64, np.arange(m), genes)
    tw = O.transform_sparse(G.indptr.astype(np.int64), G.indices.astype(np.int64), G.data, m, nc, plain.components_(np.float64),
                            plain.mean_(np.float64), True)
    print(f"f64 Lanczos: projection of all {m} rows off by {np.abs(t - tw).max() / max(1.0, float(np.abs(tw).max())):.3e} of the largest coordinate")
    np.testing.assert_allclose(t, tw, atol=1e-9 * max(1.0, float(np.abs(tw).max())))
