"""The check / canonicalise gate on device-resident arrays (-m gpu): sapca_check_csr_device_*,
sapca_canonicalize_csr_device_*, ResidentCsr.check / canonicalize / from_torch.

The reference for the canonical arrays is tests/canonical_ref.py (a stable sort per row, equal columns summed left to right
in the matrix's dtype) and the comparison is exact: offsets and indices equal, values equal as bit patterns.  scipy's
sum_duplicates serves only where every sum is exact (small integers).  The check's counts are compared with counts taken
on the host, exactly.  Fits on a canonical result are held to the bars tests/test_gpu_select_rows.py uses for the same
fits (f32 randomized singular values rtol 1e-4, mean atol 1e-5; f64 Lanczos singular values rtol 1e-5; subspace angle
1e-4), statistics to its 1e-12.

The shapes are the smallest at which the kernels can go wrong: canon.hip sorts rows of <= 64 entries in one wave, rows of
<= 4096 entries in one workgroup's LDS and longer rows in global memory; the check cuts the entries into spans of 4096
and stages at most 2048 rows of a span at a time."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import canonical_ref as R
import masked_stats_ref as M
import sapca
import sapca_oracle as O
from sapca import _lib as L
from sapca import ops, synth
from sapca import PowerIterationNormalizer as PIN
from sapca import SVDMethod

pytestmark = pytest.mark.gpu

BITS = {np.dtype(np.float32): np.uint32, np.dtype(np.float64): np.uint64}


def _adopt(sess, ptr, idx, val, shape):
    """host arrays -> the caller's own device tensors -> a ResidentCsr that merely points at them"""
    dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (np.asarray(ptr, np.int64), np.asarray(idx, np.int32), val)]
    return ops.ResidentCsr.from_torch(sess, *dev, shape)


def _host(X):
    d = X.as_device_csr()
    return d.row_offsets.cpu().numpy(), d.col_indices.cpu().numpy(), d.values.cpu().numpy()


def _same_arrays(got, want, what):
    """exactly: offsets, indices, value bit patterns"""
    assert got[0].dtype == np.int64 and got[1].dtype == np.int32 and got[2].dtype == want[2].dtype, what
    np.testing.assert_array_equal(got[0], want[0], err_msg=f"{what}: offsets")
    np.testing.assert_array_equal(got[1], want[1], err_msg=f"{what}: indices")
    bits = BITS[np.dtype(want[2].dtype)]
    np.testing.assert_array_equal(got[2].view(bits), np.ascontiguousarray(want[2]).view(bits), err_msg=f"{what}: value bits")


def _rows_from_lengths(lens, n, rng, dtype):
    """a canonical matrix without duplicates: row r has lens[r] distinct ascending columns; values never zero"""
    cols = [np.sort(rng.choice(n, int(k), replace=False)) for k in lens]
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    idx = (np.concatenate(cols) if len(cols) else np.zeros(0)).astype(np.int32)
    val = (rng.normal(0.0, 2.0, idx.size) + np.where(rng.random(idx.size) < 0.5, -5.0, 5.0)).astype(dtype)
    return ptr, idx, val


def _permute_rows(ptr, idx, val, how, rng):
    idx, val = idx.copy(), val.copy()
    for r in range(ptr.size - 1):
        a, b = int(ptr[r]), int(ptr[r + 1])
        p = np.arange(b - a)[::-1] if how == "reversed" else rng.permutation(b - a)
        idx[a:b], val[a:b] = idx[a:b][p], val[a:b][p]
    return idx, val


def _unsorted_rows(ptr, idx):
    """the rows that hold an entry whose column is below its predecessor's, ascending"""
    lens = np.diff(ptr)
    row = np.repeat(np.arange(ptr.size - 1), lens)
    desc = np.zeros(idx.size, bool)
    desc[1:] = (idx[1:] < idx[:-1]) & (row[1:] == row[:-1])
    return np.unique(row[desc])


# ------------------------------------------------------------------ 1. permutation round trip
def _ladder_lengths():
    lens = [0, 1, 2]
    p = 4
    while p <= 16384:
        lens += [p - 1, p, p + 1]
        p *= 2
    lens += [0, 60_000]                                    # (the class caps, 64 and 4096, are powers of two: in the ladder)
    return np.array(lens, dtype=np.int64)


@pytest.fixture(scope="module")
def ladder():
    """row lengths 0, 1, 2, every power of two from 4 to 16,384 minus one, exact and plus one, and one row of 60,000 entries
    with n = 70,000, in a scrambled row order; built once, never modified"""
    rng = np.random.default_rng(1)
    lens = rng.permutation(_ladder_lengths())
    out = {}
    for dt in (np.float32, np.float64):
        out[np.dtype(dt)] = _rows_from_lengths(lens, 70_000, rng, dt)
    return out


@pytest.mark.parametrize("how", ["shuffled", "reversed"])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_permuted_rows_come_back_byte_identical(ladder, dt, how):
    ptr, idx, val = ladder[np.dtype(dt)]
    m, n = ptr.size - 1, 70_000
    pidx, pval = _permute_rows(ptr, idx, val, how, np.random.default_rng(2))
    sess = ops.Session()
    X = _adopt(sess, ptr, pidx, pval, (m, n))
    Cn, rep = X.canonicalize()
    assert Cn is not X and Cn.nnz == X.nnz and Cn.shape == X.shape
    _same_arrays(_host(Cn), (ptr, idx, val), f"{how} {np.dtype(dt).name}")
    unsorted = _unsorted_rows(ptr, pidx)                    # (a short row can come out of the shuffle in order)
    assert rep.flags == ("UNSORTED",) and not rep.canonical
    assert unsorted.size >= 40 and rep.unsorted_rows == unsorted.size and rep.first_unsorted_row == int(unsorted[0])
    assert rep.duplicate_entries == 0 and rep.first_duplicate_row is None
    assert (X.d_ptr, X.d_idx, X.d_val) != (Cn.d_ptr, Cn.d_idx, Cn.d_val)
    src = _host(X)                                          # the caller's arrays are untouched
    np.testing.assert_array_equal(src[1], pidx)
    assert src[2].tobytes() == pval.tobytes()
    assert Cn.check().canonical and Cn.check().flags == ()


def test_many_tiny_rows_more_than_one_lds_turn_of_the_check():
    """9,000 rows of 0-3 entries with 5,000 empty rows in the middle: a span of 4,096 entries crosses more rows than the
    check stages at a time, and every sorted row is a wave row"""
    rng = np.random.default_rng(3)
    lens = rng.integers(0, 4, 9000)
    lens[2000:7000] = 0
    ptr, idx, val = _rows_from_lengths(lens, 64, rng, np.float32)
    pidx, pval = _permute_rows(ptr, idx, val, "reversed", rng)
    sess = ops.Session()
    Cn, rep = _adopt(sess, ptr, pidx, pval, (9000, 64)).canonicalize()
    _same_arrays(_host(Cn), (ptr, idx, val), "tiny rows")
    unsorted = _unsorted_rows(ptr, pidx)
    assert unsorted.size == int((lens >= 2).sum()) and rep.unsorted_rows == unsorted.size and rep.first_unsorted_row == int(unsorted[0])


# ------------------------------------------------------------------ 2. duplicates
def _with_duplicates(spec, n, rng, dtype, integers):
    """rows of (entries, distinct columns) in stored order: every chosen column at least once, the rest drawn among them,
    the row shuffled (so duplicates are mostly not adjacent)"""
    lens = np.array([s[0] for s in spec], dtype=np.int64)
    idx = []
    for length, distinct in spec:
        cols = rng.choice(n, distinct, replace=False)
        row = np.concatenate([cols, rng.choice(cols, length - distinct)]) if distinct else np.zeros(0, np.int64)
        idx.append(rng.permutation(row))
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    idx = np.concatenate(idx).astype(np.int32)
    val = (rng.integers(-8, 9, idx.size) if integers else rng.normal(0.0, 3.0, idx.size)).astype(dtype)
    return ptr, idx, val


# (entries, distinct): rows of one column only in every class; rows that leave their class by merging (70 -> 60 across the
# wave cap, 4200 -> 4000 across the LDS cap, 64 -> 40, 4096 -> 4095); rows at the caps; clean and empty rows between
DUP_SPEC = [(5, 1), (0, 0), (64, 1), (65, 1), (200, 1), (4096, 1), (4097, 1), (5000, 1), (70, 60), (4200, 4000), (64, 40),
            (4096, 4095), (65, 64), (4097, 4096), (3, 3), (1, 1), (0, 0), (300, 150), (9000, 700), (2, 1)]


@pytest.fixture(scope="module")
def dup_cases():
    out = {}
    for dt in (np.float32, np.float64):
        for integers in (True, False):
            rng = np.random.default_rng(17)
            src = _with_duplicates(DUP_SPEC, 12_000, rng, dt, integers)
            out[(np.dtype(dt), integers)] = (src, R.canonicalize(*src))
    return out


@pytest.mark.parametrize("integers", [True, False], ids=["small integers against scipy", "arbitrary values against canonical_ref"])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_duplicates_are_summed_left_to_right(dup_cases, dt, integers):
    (ptr, idx, val), want = dup_cases[(np.dtype(dt), integers)]
    m, n = ptr.size - 1, 12_000
    sess = ops.Session()
    X = _adopt(sess, ptr, idx, val, (m, n))
    Cn, rep = X.canonicalize()
    got = _host(Cn)
    _same_arrays(got, want, "against canonical_ref")
    if integers:                                            # every sum is exact: scipy's order does not matter
        A = sp.csr_matrix((val.copy(), idx.copy(), ptr.copy()), shape=(m, n))
        A.sum_duplicates()
        A.sort_indices()
        _same_arrays(got, (A.indptr.astype(np.int64), A.indices.astype(np.int32), A.data), "against scipy")
    distinct = np.array([s[1] for s in DUP_SPEC])
    np.testing.assert_array_equal(got[0], np.concatenate([[0], np.cumsum(distinct)]))
    assert Cn.nnz == int(distinct.sum()) and rep.duplicate_entries == X.nnz - Cn.nnz and "DUPLICATES" in rep.flags
    assert Cn.check().flags == ()
    again, rep2 = X.canonicalize()                          # deterministic, and the second result replaces the first
    _same_arrays(_host(again), want, "second run")
    assert rep2.duplicate_entries == rep.duplicate_entries and rep2.unsorted_rows == rep.unsorted_rows


def test_duplicates_only_sorted_input_and_hidden_duplicates():
    """a sorted row with adjacent duplicates: the check counts them all; the same entries with the duplicates apart in an
    unsorted row: the check cannot see them, canonicalize reports them"""
    ptr = np.array([0, 6, 9], np.int64)
    idx = np.array([1, 1, 1, 4, 7, 7, 0, 2, 5], np.int32)
    val = np.array([0.1, 0.2, 0.3, 1.0, 2.0, 3.0, 5.0, 6.0, 7.0], np.float32)
    sess = ops.Session()
    X = _adopt(sess, ptr, idx, val, (2, 9))
    rep = X.check()
    assert rep.flags == ("DUPLICATES",) and rep.duplicate_entries == 3 and rep.first_duplicate_row == 0 and rep.unsorted_rows == 0
    Cn, rep = X.canonicalize()
    _same_arrays(_host(Cn), R.canonicalize(ptr, idx, val), "sorted duplicates")
    assert rep.duplicate_entries == 3 and Cn.nnz == 6
    hidden = np.array([7, 1, 4, 1, 7, 1, 0, 2, 5], np.int32)              # no two equal columns next to each other
    Y = _adopt(sess, ptr, hidden, val, (2, 9))
    rep = Y.check()
    assert rep.flags == ("UNSORTED",) and rep.duplicate_entries == 0 and rep.unsorted_rows == 1
    Cn, rep = Y.canonicalize()
    _same_arrays(_host(Cn), R.canonicalize(ptr, hidden, val), "hidden duplicates")
    assert rep.duplicate_entries == 3 and set(rep.flags) == {"UNSORTED", "DUPLICATES"} and rep.first_duplicate_row is None


# ------------------------------------------------------------------ 3. bit patterns
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_bit_patterns_of_entries_that_do_not_merge_survive(dt):
    rng = np.random.default_rng(23)
    spec = [(40, 40), (300, 300), (5000, 5000), (70, 35), (10, 10)]       # (row 3 merges; its values stay ordinary)
    ptr, idx, val = _with_duplicates(spec, 9000, rng, dt, False)
    bits = BITS[np.dtype(dt)]
    nan_pos, nan_neg = (0x7FC00123, 0xFFC00001) if dt == np.float32 else (0x7FF8000000000123, 0xFFF8000000000001)
    vb = val.view(bits)
    for r in (0, 1, 2, 4):
        spots = int(ptr[r]) + rng.choice(int(ptr[r + 1] - ptr[r]), 8, replace=False)
        vb[spots[0]], vb[spots[1]] = bits(nan_pos), bits(nan_neg)
        vb[spots[2]] = bits(nan_pos + 0x40)                               # (a third payload)
        val[spots[3:5]] = -0.0
        val[spots[5:7]] = 0.0
        val[spots[7]] = np.inf
    want = R.canonicalize(ptr, idx, val)
    sess = ops.Session()
    X = _adopt(sess, ptr, idx, val, (len(spec), 9000))
    Cn, rep = X.canonicalize()
    _same_arrays(_host(Cn), want, "bit patterns")
    kept = _host(Cn)[2].view(bits)
    assert (kept == bits(nan_pos)).sum() == 4 and (kept == bits(nan_neg)).sum() == 4 and (kept == bits(nan_pos + 0x40)).sum() == 4
    assert (kept == bits(1) << bits(8 * np.dtype(dt).itemsize - 1)).sum() == 8          # -0.0
    assert (kept == 0).sum() == 8                                                        # stored zeros are not dropped
    assert rep.nonfinite_values == 16 and rep.stored_zeros == 16 and "NONFINITE" in rep.flags


# ------------------------------------------------------------------ 4. already canonical
def _clean(m, n, density, seed, dtype):
    rng = np.random.default_rng(seed)
    D = (rng.random((m, n)) < density) * (rng.normal(0.0, 2.0, (m, n)) + 5.0)
    D[7, :] = 0
    A = sp.csr_matrix(D.astype(dtype))
    A.sort_indices()
    assert (A.data != 0).all() and np.isfinite(A.data).all()
    return A


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_canonical_input_is_handed_back_as_it_is(dt):
    A = _clean(700, 300, 0.06, 5, dt)
    sess = ops.Session()
    X = sess.upload(A.indptr, A.indices, A.data, *A.shape)
    stats_before = X.stats(ops.COLUMN)
    Cn, rep = X.canonicalize()
    assert Cn is X and rep.canonical and rep.flags == () and rep.bits == 0
    assert (rep.unsorted_rows, rep.duplicate_entries, rep.cols_out_of_range, rep.nonfinite_values, rep.stored_zeros) == (0, 0, 0, 0, 0)
    # the raw call: the source's own pointers and nnz
    nnz_out, dp, di, dv = C.c_uint64(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    suf = "f32" if dt == np.float32 else "f64"
    st = getattr(L.load(), f"sapca_canonicalize_csr_device_{suf}")(*X._args(), C.byref(nnz_out), C.byref(dp), C.byref(di), C.byref(dv), None)
    assert st == L.OK and (dp.value, di.value, dv.value, nnz_out.value) == (X.d_ptr, X.d_idx, X.d_val, X.nnz)
    # the source afterwards: a selection and the statistics are what they were
    rows = np.arange(0, 700, 3)
    S = X.select_rows(rows)
    want = A[rows]
    got = _host(S)
    np.testing.assert_array_equal(got[0], want.indptr)
    np.testing.assert_array_equal(got[1], want.indices)
    assert got[2].tobytes() == want.data.tobytes()
    for a, b in zip(X.stats(ops.COLUMN), stats_before):
        np.testing.assert_allclose(a, b, rtol=1e-12)
    # a canonical selection is handed back too
    Cs, rep = S.canonicalize()
    assert Cs is S and rep.canonical


# ------------------------------------------------------------------ 5. the check, defect by defect
@pytest.fixture(scope="module")
def clean_host():
    A = _clean(300, 200, 0.1, 9, np.float32)
    return A.indptr.astype(np.int64), A.indices.astype(np.int32), A.data.copy()


def _report_fields(rep):
    return {f: getattr(rep, f) for f in ops.CsrReport._COUNTS + ops.CsrReport._FIRSTS} | {"bits": rep.bits}


NOTHING = dict(cols_out_of_range=0, unsorted_rows=0, duplicate_entries=0, nonfinite_values=0, stored_zeros=0,
               first_bad_offset_row=None, first_out_of_range_row=None, first_unsorted_row=None, first_duplicate_row=None,
               first_nonfinite_row=None, bits=0)


def _last_of_row(ptr, r):
    assert ptr[r + 1] - ptr[r] >= 3
    return int(ptr[r + 1]) - 1


def _plant(name, ptr, idx, val, n):
    """the defect `name` alone in copies of the clean arrays; returns (ptr, idx, val, expected report fields)"""
    ptr, idx, val = ptr.copy(), idx.copy(), val.copy()
    want = dict(NOTHING)
    if name == "clean":
        pass
    elif name == "a decreasing offset":                       # every offset stays inside [0, nnz]: the arrays remain valid
        assert ptr[11] + 1 <= ptr[-1] and ptr[10] > ptr[9]
        ptr[10] = ptr[11] + 1
        want.update(bits=L.CSR_BAD_OFFSETS, first_bad_offset_row=10)
    elif name == "ptr[0] != 0":
        assert ptr[1] >= 2
        ptr[0] = 1
        want.update(bits=L.CSR_BAD_OFFSETS, first_bad_offset_row=0)
    elif name == "a column equal to n":                       # at the end of its row: larger than its predecessor
        idx[_last_of_row(ptr, 42)] = n
        want.update(bits=L.CSR_COL_RANGE, cols_out_of_range=1, first_out_of_range_row=42)
    elif name == "a column of -1":                            # unsigned: the largest column there is
        idx[_last_of_row(ptr, 250)] = -1
        want.update(bits=L.CSR_COL_RANGE, cols_out_of_range=1, first_out_of_range_row=250)
    elif name == "two unsorted rows":
        for r in (17, 99):
            e = _last_of_row(ptr, r)
            idx[e - 1], idx[e] = idx[e], idx[e - 1]
        want.update(bits=L.CSR_UNSORTED, unsorted_rows=2, first_unsorted_row=17)
    elif name == "an adjacent duplicate":
        e = _last_of_row(ptr, 130)
        idx[e] = idx[e - 1]
        want.update(bits=L.CSR_DUPLICATES, duplicate_entries=1, first_duplicate_row=130)
    elif name == "three non-finite values":
        val[int(ptr[60])], val[int(ptr[60]) + 1], val[_last_of_row(ptr, 200)] = np.inf, np.nan, -np.inf
        want.update(bits=L.CSR_NONFINITE, nonfinite_values=3, first_nonfinite_row=60)
    elif name == "stored zeros":
        val[int(ptr[5])], val[int(ptr[80]) + 1], val[_last_of_row(ptr, 299)], val[int(ptr[150])] = 0.0, -0.0, 0.0, 0.0
        want.update(stored_zeros=4)
    else:
        raise AssertionError(name)
    return ptr, idx, val, want


DEFECTS = ["clean", "a decreasing offset", "ptr[0] != 0", "a column equal to n", "a column of -1", "two unsorted rows",
           "an adjacent duplicate", "three non-finite values", "stored zeros"]


@pytest.mark.parametrize("name", DEFECTS)
def test_check_reports_each_defect_alone(clean_host, name):
    n = 200
    ptr, idx, val, want = _plant(name, *clean_host, n)
    sess = ops.Session()
    for dt in (np.float32, np.float64):
        X = _adopt(sess, ptr, idx, val.astype(dt), (ptr.size - 1, n))
        rep = X.check()
        assert _report_fields(rep) == want, (name, np.dtype(dt).name)
        assert rep.canonical == ((want["bits"] & 15) == 0)
        assert _report_fields(X.check()) == want                # the same from call to call


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_check_counts_equal_host_counts_on_a_messy_skewed_matrix(dt):
    """everything at once, on rows of 0-6 entries around one row of 60,000 (fifteen spans see it; it is one unsorted row)
    and a run of empty rows: the counts against counts taken with numpy"""
    rng = np.random.default_rng(31)
    m, n = 3000, 70_000
    lens = rng.integers(0, 7, m)
    lens[400:900] = 0
    lens[1500] = 60_000
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    nnz = int(ptr[-1])
    idx = rng.integers(0, 40, nnz).astype(np.int32)           # few columns: descents and equal neighbours everywhere
    a, b = int(ptr[1500]), int(ptr[1501])
    idx[a:b] = rng.integers(0, n, b - a)
    val = rng.normal(0.0, 1.0, nnz).astype(dt)
    val[rng.choice(nnz, 50, replace=False)] = 0.0
    val[rng.choice(nnz, 30, replace=False)] = np.nan
    oor = rng.choice(nnz, 20, replace=False)
    idx[oor[:10]], idx[oor[10:]] = n, -7
    row = np.repeat(np.arange(m), lens)
    u = idx.view(np.uint32).astype(np.int64)
    inside = np.ones(nnz, bool)
    inside[ptr[:-1][lens > 0]] = False                        # row starts have no predecessor
    desc = np.zeros(nnz, bool)
    dup = np.zeros(nnz, bool)
    desc[1:], dup[1:] = u[1:] < u[:-1], u[1:] == u[:-1]
    desc &= inside
    dup &= inside
    nonfin, zero, out = ~np.isfinite(val), val == 0, u >= n
    sess = ops.Session()
    rep = _adopt(sess, ptr, idx, val, (m, n)).check()
    first = lambda mask: int(row[mask].min())                 # noqa: E731
    assert rep.bits == 2 | 4 | 8 | 16
    assert (rep.cols_out_of_range, rep.first_out_of_range_row) == (int(out.sum()), first(out))
    assert (rep.unsorted_rows, rep.first_unsorted_row) == (np.unique(row[desc]).size, first(desc))
    assert (rep.duplicate_entries, rep.first_duplicate_row) == (int(dup.sum()), first(dup))
    assert (rep.nonfinite_values, rep.first_nonfinite_row) == (int(nonfin.sum()), first(nonfin))
    assert rep.stored_zeros == int(zero.sum())


# ------------------------------------------------------------------ 6. refusals
def test_refusals_leave_the_handle_usable(clean_host):
    ptr, idx, val = clean_host
    m, n = ptr.size - 1, 200
    A = sp.csr_matrix((val, idx, ptr), shape=(m, n))
    sess = ops.Session()
    U = sess.upload(A.indptr, A.indices, A.data, m, n)
    before = [x.tobytes() for x in _host(U)]
    bad = _plant("a column equal to n", ptr, idx, val, n)
    with pytest.raises(L.SapcaError) as e:
        _adopt(sess, *bad[:3], (m, n)).canonicalize()
    assert e.value.status == L.ERR_ARG
    assert str(e.value).startswith("canonicalize: 1 column indices are out of range (n = 200), the first in row 42")
    bad = _plant("a decreasing offset", ptr, idx, val, n)
    with pytest.raises(L.SapcaError) as e:
        _adopt(sess, *bad[:3], (m, n)).canonicalize()
    assert e.value.status == L.ERR_ARG and str(e.value).startswith("canonicalize: the row offsets are broken at row 10")
    pidx, pval = _permute_rows(ptr, idx, val, "shuffled", np.random.default_rng(4))
    X = _adopt(sess, ptr, pidx, pval, (m, n))
    nnz_out, dp, di, dv = C.c_uint64(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    outs = [C.byref(nnz_out), C.byref(dp), C.byref(di), C.byref(dv)]
    fn = L.load().sapca_canonicalize_csr_device_f32
    for missing in range(4):                                    # each null output pointer
        o = list(outs)
        o[missing] = None
        assert fn(*X._args(), *o, None) == L.ERR_ARG and b"null output pointer" in L.load().sapca_last_error(sess._h)
    short = L.CsrReport()
    short.struct_size = 16                                      # a report of another size
    assert fn(*X._args(), *outs, C.byref(short)) == L.ERR_ARG and b"struct_size" in L.load().sapca_last_error(sess._h)
    assert L.load().sapca_check_csr_device_f32(*X._args(), None) == L.ERR_ARG
    assert L.load().sapca_check_csr_device_f32(*X._args(), C.byref(short)) == L.ERR_ARG
    Cn, rep = X.canonicalize()                                  # a correct call on the same handle
    _same_arrays(_host(Cn), (ptr, idx, val), "after the refused calls")
    with pytest.raises(L.SapcaError, match="own canonical result") as e:
        Cn.canonicalize()
    assert e.value.status == L.ERR_ARG
    _same_arrays(_host(Cn), (ptr, idx, val), "after the refused self-canonicalisation")
    assert Cn.check().canonical                                 # (the check takes the handle's own result)
    assert [x.tobytes() for x in _host(U)] == before            # the upload's arrays are unchanged throughout


# ------------------------------------------------------------------ 7 / 8. fits on a canonical result
class _InHandleOf:
    """a Session-shaped view of an estimator's handle (not owned): adoptions and uploads in the handle that fits"""

    def __init__(self, est):
        self._est, self._h = est, est._h

    _csr_args = ops.Session._csr_args
    upload = ops.Session.upload


def _messy_copy(ptr, idx, val, rng, dups):
    """the same matrix out of order: every row shuffled, and `dups` entries split in two (x -> x / 4 and 3 x / 4, exact in
    binary), the halves at random places of the row"""
    lens = np.diff(ptr)
    split = np.zeros(idx.size, bool)
    split[rng.choice(idx.size, dups, replace=False)] = True
    row = np.repeat(np.arange(ptr.size - 1), lens)
    idx2 = np.concatenate([idx, idx[split]])
    val2 = np.concatenate([np.where(split, val / 4, val), (3 * (val[split] / 4))]).astype(val.dtype)
    row2 = np.concatenate([row, row[split]])
    order = np.lexsort((rng.random(idx2.size), row2))
    ptr2 = np.concatenate([[0], np.cumsum(np.bincount(row2, minlength=ptr.size - 1))]).astype(np.int64)
    return ptr2, idx2[order].astype(np.int32), val2[order]


@pytest.fixture(scope="module")
def gapped():
    m, n, k = 3000, 600, 6
    out = {}
    for dt, tdt, centred in ((np.float32, torch.float32, True), (np.float64, torch.float64, False)):
        ptr, idx, val = (x.cpu().numpy() for x in synth.gapped_csr(m, n, 0.08, k, seed=42, centred=centred, dtype=tdt))
        rng = np.random.default_rng(6)
        messy = _messy_copy(ptr.astype(np.int64), idx.astype(np.int32), val, rng, 25)
        canon = R.canonicalize(*messy)                          # the host-canonical matrix both models are about
        out[np.dtype(dt)] = dict(m=m, n=n, k=k, messy=messy, canon=canon)
    return out


def _aligned(a, b):
    """rows of a with the signs of b's"""
    s = np.sign(np.sum(a * b, axis=1))
    s[s == 0] = 1
    return a * s[:, None]


def test_f32_randomized_fit_on_canonicalised_arrays_equals_the_fit_on_the_host_canonical_upload(gapped):
    g = gapped[np.dtype(np.float32)]
    m, n, k, p, q = g["m"], g["n"], g["k"], 6, 2
    om = synth.gaussian_panel(n, k + p, 42).numpy()
    new = lambda: sapca.SparsePCABuilder.new().n_components(k).svd_method(SVDMethod.Random(p, q, PIN.QR)).build().set_omega(om)   # noqa: E731
    a, b = new(), new()
    Cn, rep = _adopt(_InHandleOf(a), *g["messy"], (m, n)).canonicalize()
    assert rep.duplicate_entries == 25 and rep.unsorted_rows > 0
    _same_arrays(_host(Cn), g["canon"], "the canonical arrays")
    a.fit(Cn.as_device_csr())
    cp, ci, cv = g["canon"]
    U = _InHandleOf(b).upload(cp, ci.astype(np.int64), cv, m, n)
    b.fit(U.as_device_csr())
    np.testing.assert_allclose(a.singular_values_(np.float64), b.singular_values_(np.float64), rtol=1e-4)
    np.testing.assert_allclose(a.mean_(np.float64), b.mean_(np.float64), atol=1e-5)
    ca, cb = a.components_(np.float64), b.components_(np.float64)
    assert O.subspace_angle(ca, cb) < 1e-4
    np.testing.assert_allclose(_aligned(ca, cb), cb, atol=1e-4)
    # the statistics of the canonical result against the host restatement on the host-canonical matrix
    for direction in (ops.ROW, ops.COLUMN):
        got = Cn.masked_stats(direction)
        want = M.masked_stats(cp, ci.astype(np.int64), cv, m, n, direction)
        np.testing.assert_array_equal(got[2], want[2])
        for j in (0, 1):
            scale = max(1.0, float(np.abs(want[j]).max(initial=0)))
            np.testing.assert_allclose(got[j], want[j], rtol=1e-12, atol=1e-12 * scale)


def test_f64_lanczos_fit_on_canonicalised_arrays_equals_the_fit_on_the_host_canonical_upload(gapped):
    g = gapped[np.dtype(np.float64)]
    m, n, k = g["m"], g["n"], g["k"]
    new = lambda: sapca.SparsePCABuilder.new().n_components(k).svd_method(SVDMethod.Lanczos()).build()   # noqa: E731
    a, b = new(), new()
    Cn, rep = _adopt(_InHandleOf(a), *g["messy"], (m, n)).canonicalize()
    _same_arrays(_host(Cn), g["canon"], "the canonical arrays")
    a.fit(Cn.as_device_csr())
    cp, ci, cv = g["canon"]
    b.fit(_InHandleOf(b).upload(cp, ci.astype(np.int64), cv, m, n).as_device_csr())
    np.testing.assert_allclose(a.singular_values_(np.float64), b.singular_values_(np.float64), rtol=1e-5)
    # (f64 column sums of at most 3,000 values below 20 by two summation orders: they differ by less than 3000 * 20 * 2^-53)
    np.testing.assert_allclose(a.mean_(np.float64), b.mean_(np.float64), atol=1e-12)
    ca, cb = a.components_(np.float64), b.components_(np.float64)
    assert O.subspace_angle(ca, cb) < 1e-4
    np.testing.assert_allclose(_aligned(ca, cb), cb, atol=1e-4)


def test_a_second_canonicalisation_replaces_the_first_and_drops_its_preparation(gapped):
    """two matrices of one structure and different values: the second result has the first's addresses, shape and nnz, so a
    preparation kept from the first fit would pass for it"""
    g = gapped[np.dtype(np.float32)]
    m, n, k, p, q = g["m"], g["n"], g["k"], 6, 2
    ptr, idx, val = g["messy"]
    val_b = (val * np.where(idx % 2 == 0, 1.0, 0.25)).astype(np.float32)   # (exact scalings: the halves still add up)
    om = synth.gaussian_panel(n, k + p, 42).numpy()
    new = lambda: sapca.SparsePCABuilder.new().n_components(k).svd_method(SVDMethod.Random(p, q, PIN.QR)).build().set_omega(om)   # noqa: E731
    a, b = new(), new()
    sa = _InHandleOf(a)
    C1, _ = _adopt(sa, ptr, idx, val, (m, n)).canonicalize()
    a.fit(C1.as_device_csr())
    sing1 = a.singular_values_(np.float64).copy()
    C2, _ = _adopt(sa, ptr, idx, val_b, (m, n)).canonicalize()
    assert (C2.d_ptr, C2.d_idx, C2.d_val, C2.nnz) == (C1.d_ptr, C1.d_idx, C1.d_val, C1.nnz)
    want = R.canonicalize(ptr, idx, val_b)
    _same_arrays(_host(C2), want, "the second result")
    a.fit(C2.as_device_csr())
    b.fit(_InHandleOf(b).upload(want[0], want[1].astype(np.int64), want[2], m, n).as_device_csr())
    np.testing.assert_allclose(a.singular_values_(np.float64), b.singular_values_(np.float64), rtol=1e-4)
    assert np.abs(a.singular_values_(np.float64) / sing1 - 1).max() > 1e-2     # (and the two matrices do differ)


# ------------------------------------------------------------------ 9. degenerate shapes
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_one_row_and_no_entries(dt):
    sess = ops.Session()
    one = _adopt(sess, [0, 5], [4, 0, 2, 2, 1], np.array([1, 2, 3, 4, 5], dt), (1, 6))
    assert one.check().flags == ("UNSORTED", "DUPLICATES")
    Cn, rep = one.canonicalize()
    _same_arrays(_host(Cn), (np.array([0, 4]), np.array([0, 1, 2, 4], np.int32), np.array([2, 5, 7, 1], dt)), "m = 1")
    assert rep.duplicate_entries == 1 and rep.unsorted_rows == 1 and rep.first_unsorted_row == 0
    empty = _adopt(sess, np.zeros(6, np.int64), np.zeros(0, np.int32), np.zeros(0, dt), (5, 7))
    rep = empty.check()
    assert rep.canonical and rep.flags == () and rep.stored_zeros == 0
    Ce, rep = empty.canonicalize()
    assert Ce is empty and rep.canonical
    # a decreasing offset in a matrix of one entry: every offset stays inside [0, nnz] of arrays that exist
    bad = _adopt(sess, np.array([0, 0, 1, 0, 0, 1]), np.array([3], np.int32), np.array([2], dt), (5, 7))
    rep = bad.check()
    assert rep.flags == ("BAD_OFFSETS",) and rep.first_bad_offset_row == 2 and rep.unsorted_rows == 0
