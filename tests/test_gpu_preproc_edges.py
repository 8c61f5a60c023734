"""normalize, log1p and the line statistics of a device-resident matrix at their edges (-m gpu): sapca_normalize_csr_device_*,
sapca_log1p_csr_device_* and sapca_stats_csr_device_* against the host restatement in preproc_ref.py, on fixtures whose
preconditions test_preproc_ref_cpu.py checks.

Bars: integer fixtures exact; normalize bit for bit (NaNs by position); min / max / nonzero exact (zeros by value); sums
of real data within L * 2^-53 * sum|x| of the exact sum (L the line's length: the bound of any summation order in f64);
log1p within LOG1P_ULPS of the long-double ln(T(1) + v), exact where that is 0, +-inf or NaN."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (first, so the process carries one HIP runtime)

import preproc_ref as P
from sapca import _lib as L
from sapca import ops

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
# The reference's ln is the platform libm's (error below 1 ulp), so whatever it returns lies within 1 ulp of T of the
# correctly rounded long-double result: the bar for both types.  Not calibrated on the kernel.
LOG1P_ULPS = {np.float32: 1.0, np.float64: 1.0}


def _upload(ptr, idx, val, m, n, sess=None):
    sess = sess or ops.Session()
    return sess, sess.upload(np.asarray(ptr, np.int64), np.asarray(idx, np.int64), np.ascontiguousarray(val), m, n)


def _raw(R, name):
    suf, ct = ops._SUF[R.dtype]
    return getattr(L.load(), f"sapca_{name}_csr_device_{suf}"), ct


def _differ(got, want):
    """the first few positions where two arrays differ by value (NaN equal to NaN), for a message"""
    return np.flatnonzero(~((got == want) | (np.isnan(got) & np.isnan(want))))[:8]


def _check_log1p(got, val, what):
    T = val.dtype.type
    want = P.log1p_longdouble(val)
    want_t = want.astype(T)
    special = ~np.isfinite(want_t) | (want_t == 0)
    assert P.same_values(got[special], want_t[special]), f"{what}: an exact case (0, inf, NaN) differs"
    d = P.ulp_distance(got, want, T)
    worst = int(np.argmax(d)) if d.size else 0
    print(f"log1p {np.dtype(T).name} {what}: max distance {d.max(initial=0):.4f} ulp" + (f" at v = {val[worst]!r}" if d.size else ""))
    assert d.max(initial=0) <= LOG1P_ULPS[T], f"{what}: {d.max()} ulp at v = {val[worst]!r} (got {got[worst]!r})"


# ---- a. the stride fixture: every grid-stride loop takes two full turns and a ragged third -----------------------------------
@pytest.fixture(scope="module")
def stride():
    return P.stride_fixture()


@pytest.mark.parametrize("dt", DTYPES)
def test_stride_row_statistics_are_exact(stride, dt):
    ptr, idx, ival, m, n = stride
    val = ival.astype(dt)
    s, q = P.int_line_sums(ptr, idx, ival, m, n, P.ROW)
    lo, hi = P.min_max(ptr, idx, val, m, n, P.ROW)
    sess, R = _upload(ptr, idx, val, m, n)
    got = R.stats(ops.ROW)
    np.testing.assert_array_equal(got[0], s.astype(np.float64))
    np.testing.assert_array_equal(got[1], q.astype(np.float64))
    np.testing.assert_array_equal(got[2], np.diff(ptr).astype(np.uint64))
    np.testing.assert_array_equal(got[3], lo)
    np.testing.assert_array_equal(got[4], hi)


@pytest.mark.parametrize("direction", [ops.ROW, ops.COLUMN])
@pytest.mark.parametrize("dt", DTYPES)
def test_stride_normalize_is_bit_exact(stride, dt, direction):
    """two calls in a row (no single target makes one scale +inf and another underflow to 0), the second on the first's
    output; the sums carry zeros, negatives, NaN, +-inf in every turn of the kernel's loop"""
    ptr, idx, ival, m, n = stride
    val = ival.astype(dt)
    sums = P.stride_sums(P.STRIDE_ROW_TURNS if direction == ops.ROW else P.STRIDE_COL_THIRDS, 7 + direction)
    sess, R = _upload(ptr, idx, val, m, n)
    for target in P.STRIDE_TARGETS:
        want = P.normalize(ptr, idx, val, sums, target, direction)
        got = R.normalize(sums, target, direction).values()
        assert P.same_bits(got, want), f"target {target}: entries {_differ(got, want)}"
        alone = P.scales_not_positive(ptr, idx, sums, target, direction)
        assert alone.any() and got[alone].tobytes() == val[alone].tobytes()      # lines whose scale is not > 0: untouched
        val = want


@pytest.mark.parametrize("dt", DTYPES)
def test_stride_log1p(stride, dt):
    ptr, idx, ival, m, n = stride
    val = ival.astype(dt)
    sess, R = _upload(ptr, idx, val, m, n)
    got = R.log1p().values()
    zero = val == 0
    assert zero.any() and (got[zero] == 0).all() and not np.signbit(got[zero]).any()
    _check_log1p(got, val, "stride fixture")


# ---- b. the wide fixture: more than two turns of lines after the transposition --------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
def test_wide_column_statistics_are_exact(dt):
    ptr, idx, ival, m, n = P.wide_fixture()
    val = ival.astype(dt)
    s, q = P.int_line_sums(ptr, idx, ival, m, n, P.COLUMN)
    lo, hi = P.min_max(ptr, idx, val, m, n, P.COLUMN)
    sess, R = _upload(ptr, idx, val, m, n)
    got = R.stats(ops.COLUMN)
    np.testing.assert_array_equal(got[0], s.astype(np.float64))
    np.testing.assert_array_equal(got[1], q.astype(np.float64))
    np.testing.assert_array_equal(got[2], np.bincount(idx, minlength=n).astype(np.uint64))
    np.testing.assert_array_equal(got[3], lo)
    np.testing.assert_array_equal(got[4], hi)


# ---- c. ragged lines: the per-lane loop over a line takes 0, 1, 2, ... steps; sums held to the f64 bound ---------------------
@pytest.mark.parametrize("dt", DTYPES)
def test_ragged_lines_sums_within_the_f64_bound(dt):
    ptr, idx, val, m, n = P.ragged_fixture(dt)
    sess, R = _upload(ptr, idx, val, m, n)
    for direction in (ops.ROW, ops.COLUMN):
        got = R.stats(direction)
        want = P.stats(ptr, idx, val, m, n, direction)
        P.check_sum_bound(got[0], got[1], P.exact_line_sums(ptr, idx, val, m, n, direction), dt, f"ragged, direction {direction}")
        np.testing.assert_array_equal(got[2], want[2])
        np.testing.assert_array_equal(got[3], want[3])
        np.testing.assert_array_equal(got[4], want[4])
    sums = R.stats(ops.ROW)[0]
    got = R.normalize(sums, 1e4, ops.ROW).values()                 # every row length through normalize_rows_kernel
    assert P.same_bits(got, P.normalize(ptr, idx, val, sums, 1e4, ops.ROW))


# ---- d. special values ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("dt", DTYPES)
def test_special_values_in_the_statistics(dt, transposed):
    """S holds the special lines as its rows, S^T as its columns: both directions of both, against the literal loops"""
    ptr, idx, val, m, n = P.special_fixture(dt, transposed)
    sess, R = _upload(ptr, idx, val, m, n)
    for direction in (ops.ROW, ops.COLUMN):
        what = f"S{'^T' if transposed else ''}, direction {direction}"
        got = R.stats(direction)
        want = P.ref_stats(ptr, idx, val, m, n, direction)
        for k, name in ((3, "min"), (4, "max")):      # zeros by value, NaNs by position
            bad = _differ(got[k], want[k])
            assert P.same_values(got[k], want[k]), f"{what}: {name} of lines {bad}: {got[k][bad]} for {want[k][bad]}"
        np.testing.assert_array_equal(got[2], want[2], err_msg=what)          # stored zeros count
        exact = P.exact_line_sums(ptr, idx, val, m, n, direction)
        wild = np.array([e[0] is None for e in exact])
        assert wild.any() and (~wild).any()
        # an inf or a NaN in a line: +-inf, or NaN, whatever the order of the additions
        assert P.same_values(got[0][wild], want[0][wild]) and P.same_values(got[1][wild], want[1][wild]), what
        P.check_sum_bound(got[0], got[1], exact, dt, what)
        # lines of subnormals alone: not flushed, the exact sum
        lines = P.lines(ptr, idx, val, m, n, direction)
        tiny = np.finfo(dt).tiny
        sub = [j for j, l in enumerate(lines) if len(l) and ((l != 0) & (np.abs(l) < tiny)).all()]
        assert sub or direction != (ops.COLUMN if transposed else ops.ROW)   # (the direction whose lines are special_rows)
        for j in sub:
            assert got[0][j] == float(exact[j][0]) and (got[0][j] != 0 or exact[j][0] == 0), f"{what}: line {j} of subnormals"


@pytest.mark.parametrize("dt", DTYPES)
def test_special_values_in_normalize(dt):
    ptr, idx, val, m, k, sums = P.normalize_special_values(dt)
    sess, R = _upload(ptr, idx, val, m, k)
    for direction, s in ((ops.ROW, sums), (ops.COLUMN, np.resize(sums, k))):
        for target in (0.0, -0.0, -1.0, -np.inf, np.nan):                       # no scale is > 0: every byte stays
            assert R.normalize(s, target, direction).values().tobytes() == val.tobytes(), f"target {target}"
        want = P.normalize(ptr, idx, val, s, 1.0, direction)
        got = R.normalize(s, 1.0, direction).values()
        bad = _differ(got, want)
        assert P.same_bits(got, want), f"direction {direction}: entries {bad}: {got[bad]} for {want[bad]}"
        alone = P.scales_not_positive(ptr, idx, s, 1.0, direction)
        assert got[alone].tobytes() == val[alone].tobytes()
        sess, R = _upload(ptr, idx, val, m, k, sess)


@pytest.mark.parametrize("dt", DTYPES)
def test_log1p_special_and_small_inputs(dt):
    T = np.dtype(dt).type
    fi = np.finfo(dt)
    table = np.array([-1.0, -1.5, -np.inf, -float(fi.max), np.inf, np.nan, -0.0, 0.0], np.float64).astype(T)
    cls = P.log1p_classes(dt)
    names = list(cls)
    val = np.concatenate([table] + [cls[k] for k in names])
    ptr = np.array([0, len(val)], np.int64)
    sess, R = _upload(ptr, np.arange(len(val)), val, 1, len(val))
    got = R.log1p().values()
    t = got[: len(table)]
    assert t[0] == -np.inf and np.isnan(t[1]) and np.isnan(t[2]) and np.isnan(t[3]) and t[4] == np.inf and np.isnan(t[5])
    assert t[6] == 0 and not np.signbit(t[6]) and t[7] == 0 and not np.signbit(t[7])
    at = len(table)
    for k in names:
        g, v = got[at:at + len(cls[k])], cls[k]
        at += len(v)
        if k in ("tiny", "subnormal"):      # ln(1 + v) in T, where 1 + v is 1: exactly 0 (a true log1p would return v)
            assert (g == 0).all() and not np.signbit(g).any(), f"{k}: {g}"
        _check_log1p(g, v, k)


# ---- e. degenerate shapes and the ABI's small print -----------------------------------------------------------------------
def _degenerate(dt):
    rng = np.random.default_rng(6)
    z = np.zeros(0, np.int64)
    long_cols = np.sort(rng.choice(9000, 5000, replace=False))
    return [("nnz = 0", np.zeros(4, np.int64), z, np.zeros(0, dt), 3, 5),
            ("one row, one entry", np.array([0, 1]), np.array([2]), np.array([3.0], dt), 1, 4),
            ("m = 1, a long row", np.array([0, 5000]), long_cols, rng.integers(-9, 10, 5000).astype(dt), 1, 9000),
            ("n = 1", np.concatenate([[0], np.cumsum(np.arange(70) % 3 != 1)]), np.zeros(47, np.int64), rng.integers(-9, 10, 47).astype(dt), 70, 1)]


@pytest.mark.parametrize("dt", DTYPES)
def test_degenerate_shapes(dt):
    for name, ptr, idx, val, m, n in _degenerate(dt):
        assert int(ptr[-1]) == len(val) == len(idx), name
        sess, R = _upload(ptr, idx, val, m, n)
        for direction in (ops.ROW, ops.COLUMN):
            got, want = R.stats(direction), P.stats(ptr, idx, val, m, n, direction)
            for g, w in zip(got, want):
                np.testing.assert_array_equal(g, w, err_msg=f"{name}, direction {direction}")     # (integer data: exact)
        cur = val
        for direction in (ops.ROW, ops.COLUMN):
            sums = np.abs(P.stats(ptr, idx, cur, m, n, direction)[0]) + (np.arange(m if direction == ops.ROW else n) % 2)
            want = P.normalize(ptr, idx, cur, sums, 10.0, direction)
            got = R.normalize(sums, 10.0, direction).values()
            assert P.same_bits(got, want), f"{name}, normalize direction {direction}"
            cur = want
        got = R.log1p().values()
        assert got.shape == cur.shape
        _check_log1p(got, cur, name)


@pytest.mark.parametrize("dt", DTYPES)
def test_statistics_outputs_may_be_null_one_at_a_time(dt):
    ptr, idx, val, m, n = P.special_fixture(dt)
    sess, R = _upload(ptr, idx, val, m, n)
    fn, ct = _raw(R, "stats")
    types = (C.c_double, C.c_double, C.c_uint64, ct, ct)
    for direction, ln in ((ops.ROW, m), (ops.COLUMN, n)):
        full = R.stats(direction)
        for skip in range(5):
            out = [np.full(ln, 77, a.dtype) for a in full]
            args = [None if k == skip else ops._p(out[k], types[k]) for k in range(5)]
            L.check(sess._h, fn(*R._args(), C.c_int32(direction), *args))
            for k in range(5):
                want = np.full(ln, 77, full[k].dtype) if k == skip else full[k]
                assert out[k].tobytes() == want.tobytes(), f"direction {direction}, output {skip} NULL: output {k}"


@pytest.mark.parametrize("dt", DTYPES)
def test_argument_errors_leave_the_handle_usable(dt):
    ptr, idx, val, m, n = P.ragged_fixture(dt)
    sess, R = _upload(ptr, idx, val, m, n)
    before = R.stats(ops.ROW)
    norm, _ = _raw(R, "normalize")
    stat, _ = _raw(R, "stats")
    for direction, ln, msg in ((ops.ROW, m, "Length of sums must match number of rows"), (ops.COLUMN, n, "Length of sums must match number of columns")):
        for off in (-1, 1):
            sums = np.ones(ln + off)
            with pytest.raises(L.SapcaError) as e:
                L.check(sess._h, norm(*R._args(), ops._p(sums, C.c_double), C.c_uint64(sums.size), C.c_double(1.0), C.c_int32(direction)))
            assert str(e.value) == msg and e.value.status == L.ERR_ARG
    sums = np.ones(max(m, n))
    with pytest.raises(L.SapcaError, match="direction") as e:
        L.check(sess._h, norm(*R._args(), ops._p(sums, C.c_double), C.c_uint64(m), C.c_double(1.0), C.c_int32(2)))
    assert e.value.status == L.ERR_ARG
    with pytest.raises(L.SapcaError, match="direction") as e:
        L.check(sess._h, stat(*R._args(), C.c_int32(2), None, None, None, None, None))
    assert e.value.status == L.ERR_ARG
    assert R.values().tobytes() == val.tobytes()                                   # nothing was scaled on the way
    for a, b in zip(R.stats(ops.ROW), before):
        assert a.tobytes() == b.tobytes()
    want = P.stats(ptr, idx, val, m, n, ops.COLUMN)
    got = R.stats(ops.COLUMN)
    for k in (2, 3, 4):
        np.testing.assert_array_equal(got[k], want[k])


def test_statistics_after_an_edit_see_the_edited_values():
    """normalize and log1p change the uploaded values: the transposition a COLUMN call made before is stale, and so are the
    column statistics gathered during the upload (a fit on the same handle must take its mean from the values as they are)"""
    m, n = 400, 120
    rng = np.random.default_rng(8)
    stored = rng.random((m, n)) < 0.2
    r, c = np.nonzero(stored)
    ptr = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=m))]).astype(np.int64)
    val = rng.integers(1, 30, len(c)).astype(np.float32)
    sess, R = _upload(ptr, c, val, m, n)
    R.stats(ops.COLUMN)
    lib = L.load()
    for step in ("normalize", "log1p"):
        if step == "normalize":
            R.normalize(R.stats(ops.ROW)[0], 100.0, ops.ROW)
        else:
            R.log1p()
        edited = R.values()
        assert not np.array_equal(edited, val)
        got = R.stats(ops.COLUMN)
        s2, R2 = _upload(ptr, c, edited, m, n)
        for a, b in zip(got, R2.stats(ops.COLUMN)):
            assert a.tobytes() == b.tobytes(), step
        L.check(sess._h, lib.sapca_fit_csr_device_f32(*R._args()))
        mean = np.zeros(n, np.float32)
        L.check(sess._h, lib.sapca_get_mean_f32(sess._h, ops._p(mean, C.c_float), C.c_size_t(n)))
        want = np.bincount(c, weights=edited.astype(np.float64), minlength=n) / m
        np.testing.assert_allclose(mean, want, rtol=1e-5, atol=1e-7)
        val = edited
