"""Host restatements of the reference's Normalize, Log1P and line statistics (src/sparse/csr.rs:23-134, 259-392, 558-630,
917-1078) for the tests of sapca_normalize_csr_device_*, sapca_log1p_csr_device_* and sapca_stats_csr_device_*:

- `ref_*`: literal transliterations of the reference loops (the serial branches), one Python loop per Rust loop; slow,
  for small matrices.  The two min/max loops are the ones of masked_stats_ref.
- the same functions vectorised (`normalize`, `log1p`, `stats`, `min_max`) for the large fixtures; the CPU test holds
  them to the literal ones bit for bit on every small fixture.
- `log1p_longdouble`: one = T(1) + v in T (an IEEE addition: exact parity with the reference), then ln in long double.
  Rounded once to T it is the value a correctly rounded ln would return; the reference's libm ln stays within 1 ulp of it.
- `ulp_distance`, exact line sums (`exact_line_sums`: math.fsum and rational sums of squares; `int_line_sums`: integer
  arithmetic), and the fixtures the GPU test runs, each with the preconditions that make its checks mean something.

Semantics of min/max, which the library reproduces (csr.rs:917-1008): ROW starts from a row's FIRST stored value, so a
row that begins with a NaN is (NaN, NaN) and a NaN later in a row never wins a comparison; COLUMN starts from
(T::MAX, -T::MAX), a NaN never wins, and a column of +inf alone keeps min T::MAX.  Lines without entries keep (MAX, -MAX).
"""
import math
from fractions import Fraction

import numpy as np

from masked_stats_ref import ref_min_max_col_chunk, ref_min_max_row_chunk

ROW, COLUMN = 0, 1


def _rows(ptr):
    ptr = np.asarray(ptr, np.int64)
    return np.repeat(np.arange(len(ptr) - 1, dtype=np.int64), np.diff(ptr))


# ---- the reference loops, transliterated --------------------------------------------------------------------------------
def ref_normalize(ptr, idx, val, sums, target, direction):   # csr.rs:1013-1067, U = f64
    values = np.array(val, copy=True)
    T = values.dtype.type
    target = np.float64(target)
    scaling_factors = []
    with np.errstate(all="ignore"):
        for s in np.asarray(sums, np.float64):
            scaling_factors.append(target / s if s > 0.0 else np.float64(0.0))
        if direction == COLUMN:
            for e in range(len(values)):
                scale = scaling_factors[idx[e]]
                if scale > 0.0:
                    values[e] = T(np.float64(values[e]) * scale)
        else:
            for row in range(len(ptr) - 1):
                scale = scaling_factors[row]
                if scale > 0.0:
                    for e in range(ptr[row], ptr[row + 1]):
                        values[e] = T(np.float64(values[e]) * scale)
    return values


def ref_log1p_normalize(val):   # csr.rs:1070-1078; ln in long double, rounded once (the module docstring)
    values = np.array(val, copy=True)
    T = values.dtype.type
    with np.errstate(all="ignore"):
        for e in range(len(values)):
            values[e] = T(1) + values[e]
            values[e] = T(np.log(np.longdouble(values[e])))
    return values


def ref_sum_col(ptr, idx, val, m, n):   # csr.rs:259-312 (the serial branch), T = f64
    result = [0.0] * n
    for e in range(len(val)):
        result[idx[e]] += float(val[e])
    return np.array(result, np.float64)


def ref_sum_row(ptr, idx, val, m, n):   # csr.rs:314-392 (the serial branch: in storage order, whatever the row's length)
    result = []
    for row in range(m):
        s = 0.0
        for e in range(ptr[row], ptr[row + 1]):
            s += float(val[e])
        result.append(s)
    return np.array(result, np.float64)


def ref_sum_col_squared(ptr, idx, val, m, n):   # csr.rs:558-608 (the serial branch)
    result = [0.0] * n
    for e in range(len(val)):
        v = float(val[e])
        result[idx[e]] += v * v
    return np.array(result, np.float64)


def ref_sum_row_squared(ptr, idx, val, m, n):   # csr.rs:610-622 (its vector has ncols slots; one per row here)
    result = [0.0] * m
    for row in range(m):
        for e in range(ptr[row], ptr[row + 1]):
            v = float(val[e])
            result[row] += v * v
    return np.array(result, np.float64)


def ref_nonzero_col(ptr, idx, val, m, n):   # csr.rs:23-77
    result = [0] * n
    for c in idx:
        result[c] += 1
    return np.array(result, np.uint64)


def ref_nonzero_row(ptr, idx, val, m, n):   # csr.rs:79-122
    return np.array([ptr[row + 1] - ptr[row] for row in range(m)], np.uint64)


def _initial(ln, dtype):
    big = np.finfo(dtype).max
    return np.full(ln, big, dtype), np.full(ln, -big, dtype)


def ref_min_max_col(ptr, idx, val, m, n):   # csr.rs:917-926
    return ref_min_max_col_chunk(ptr, idx, val, m, n, _initial(n, np.asarray(val).dtype))


def ref_min_max_row(ptr, idx, val, m, n):   # csr.rs:928-937
    return ref_min_max_row_chunk(ptr, idx, val, m, n, _initial(m, np.asarray(val).dtype))


def ref_stats(ptr, idx, val, m, n, direction):
    """(sum, sum_squared, nonzero, min, max) from the literal loops"""
    if direction == COLUMN:
        lo, hi = ref_min_max_col(ptr, idx, val, m, n)
        return ref_sum_col(ptr, idx, val, m, n), ref_sum_col_squared(ptr, idx, val, m, n), ref_nonzero_col(ptr, idx, val, m, n), lo, hi
    lo, hi = ref_min_max_row(ptr, idx, val, m, n)
    return ref_sum_row(ptr, idx, val, m, n), ref_sum_row_squared(ptr, idx, val, m, n), ref_nonzero_row(ptr, idx, val, m, n), lo, hi


# ---- the same, vectorised -----------------------------------------------------------------------------------------------
def normalize(ptr, idx, val, sums, target, direction):
    sums = np.asarray(sums, np.float64)
    out = np.array(val, copy=True)
    with np.errstate(all="ignore"):
        scale = np.where(sums > 0, np.float64(target) / sums, 0.0)
        sc = scale[np.asarray(idx, np.int64)] if direction == COLUMN else np.repeat(scale, np.diff(np.asarray(ptr, np.int64)))
        hit = sc > 0
        out[hit] = (out[hit].astype(np.float64) * sc[hit]).astype(out.dtype)
    return out


def scales_not_positive(ptr, idx, sums, target, direction):
    """per stored entry: True where the reference leaves it alone (its line's scale is not > 0)"""
    sums = np.asarray(sums, np.float64)
    with np.errstate(all="ignore"):
        scale = np.where(sums > 0, np.float64(target) / sums, 0.0)
    sc = scale[np.asarray(idx, np.int64)] if direction == COLUMN else np.repeat(scale, np.diff(np.asarray(ptr, np.int64)))
    return ~(sc > 0)


def log1p_longdouble(val):
    """ln(T(1) + v) with the addition in T and the logarithm in long double, not yet rounded"""
    val = np.asarray(val)
    with np.errstate(all="ignore"):
        one = (val.dtype.type(1) + val).astype(val.dtype)
        return np.log(one.astype(np.longdouble))


def log1p(val):
    val = np.asarray(val)
    with np.errstate(all="ignore"):
        return log1p_longdouble(val).astype(val.dtype)


def min_max(ptr, idx, val, m, n, direction):
    """(min, max) with the reference's semantics (the module docstring)"""
    ptr, idx, x = np.asarray(ptr, np.int64), np.asarray(idx, np.int64), np.asarray(val)
    if direction == COLUMN:
        lo, hi = _initial(n, x.dtype)
        np.fmin.at(lo, idx, x)      # fmin / fmax skip a nan operand: a nan never wins, and +inf does not beat MAX
        np.fmax.at(hi, idx, x)
        return lo, hi
    lo, hi = _initial(m, x.dtype)
    has = np.flatnonzero(np.diff(ptr) > 0)
    if has.size:
        starts = ptr[has]
        first = x[starts]
        lo[has] = np.where(np.isnan(first), first, np.fmin.reduceat(x, starts))
        hi[has] = np.where(np.isnan(first), first, np.fmax.reduceat(x, starts))
    return lo, hi


def stats(ptr, idx, val, m, n, direction):
    """(sum, sum_squared, nonzero, min, max); the sums accumulate in f64 in storage order, like the literal loops"""
    ptr, idx, x = np.asarray(ptr, np.int64), np.asarray(idx, np.int64), np.asarray(val)
    ln, key = (n, idx) if direction == COLUMN else (m, _rows(ptr))
    d = x.astype(np.float64)
    with np.errstate(all="ignore"):
        sm = np.bincount(key, weights=d, minlength=ln)[:ln].astype(np.float64)
        sq = np.bincount(key, weights=d * d, minlength=ln)[:ln].astype(np.float64)
    nz = np.bincount(key, minlength=ln)[:ln].astype(np.uint64)
    lo, hi = min_max(ptr, idx, x, m, n, direction)
    return sm, sq, nz, lo, hi


# ---- helpers ------------------------------------------------------------------------------------------------------------
def same_bits(a, b):
    """equal bit for bit, except that NaNs need only sit at the same positions"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    na, nb = np.isnan(a), np.isnan(b)
    u = np.uint32 if a.dtype == np.float32 else np.uint64
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(u), b[~nb].view(u)))


def same_values(a, b):
    """equal by value (a zero's sign does not count), NaNs at the same positions"""
    a, b = np.asarray(a), np.asarray(b)
    return bool(a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True))


def ulp_distance(got, want_longdouble, T):
    """|got - want| in units of np.spacing(|T(want)|), per element.  Where want is not finite (or rounds to a non-finite
    T) the distance is 0 if got matches T(want) exactly (NaN for NaN) and inf otherwise."""
    got = np.asarray(got, T)
    want = np.asarray(want_longdouble, np.longdouble)
    with np.errstate(all="ignore"):
        want_t = want.astype(T)
        fin = np.isfinite(want_t)
        unit = np.spacing(np.abs(np.where(fin, want_t, T(1)))).astype(np.longdouble)
        d = np.abs(got.astype(np.longdouble) - want) / unit
    exact = (got == want_t) | (np.isnan(got) & np.isnan(want_t))
    return np.where(fin, np.where(np.isfinite(got), d, np.inf), np.where(exact, 0.0, np.inf)).astype(np.float64)


def lines(ptr, idx, val, m, n, direction):
    """the stored values of every row (ROW) or column (COLUMN), in storage order"""
    ptr, idx = np.asarray(ptr, np.int64), np.asarray(idx, np.int64)
    if direction == ROW:
        return [np.asarray(val)[ptr[r]:ptr[r + 1]] for r in range(m)]
    order = np.argsort(idx, kind="stable")
    bounds = np.searchsorted(idx[order], np.arange(n + 1))
    v = np.asarray(val)[order]
    return [v[bounds[j]:bounds[j + 1]] for j in range(n)]


def exact_line_sums(ptr, idx, val, m, n, direction):
    """per line, as Fractions: (sum, sum of squares, sum of |x|, length); None in the first three where the line holds a
    value that is not finite"""
    out = []
    for line in lines(ptr, idx, val, m, n, direction):
        if not np.isfinite(line).all():
            out.append((None, None, None, len(line)))
            continue
        fr = [Fraction(float(v)) for v in line]
        out.append((sum(fr, Fraction(0)), sum((f * f for f in fr), Fraction(0)), sum((abs(f) for f in fr), Fraction(0)), len(line)))
    return out


def fsum_line_sums(ptr, idx, val, m, n, direction):
    """(correctly rounded sums, sum |x| rounded up to the next f64) per line, by math.fsum; finite values only"""
    ls = lines(ptr, idx, np.asarray(val, np.float64), m, n, direction)
    s = np.array([math.fsum(l) for l in ls])
    a = np.array([np.nextafter(math.fsum(np.abs(l)), np.inf) for l in ls])
    return s, a


def int_line_sums(ptr, idx, ival, m, n, direction):
    """(sum, sum of squares) per line of integer data, in int64 arithmetic"""
    ptr, idx, v = np.asarray(ptr, np.int64), np.asarray(idx, np.int64), np.asarray(ival, np.int64)
    if direction == COLUMN:
        order = np.argsort(idx, kind="stable")
        v = v[order]
        ptr = np.searchsorted(idx[order], np.arange(n + 1)).astype(np.int64)
    c1 = np.concatenate([[0], np.cumsum(v)])
    c2 = np.concatenate([[0], np.cumsum(v * v)])
    return c1[ptr[1:]] - c1[ptr[:-1]], c2[ptr[1:]] - c2[ptr[:-1]]


_U53 = Fraction(1, 2 ** 53)


def check_sum_bound(got_sum, got_sq, exact, dt, what):
    """|got - exact| <= L * 2^-53 * sum|x| (sums) and (L [+ 1 in f64: each square is rounded once]) * 2^-53 * sum x^2 (+ L
    * 2^-1075 in f64, where a square may round in the subnormal range), in rational arithmetic.  Lines that hold a value
    that is not finite are the caller's; a finite line whose sum|x| passes DBL_MAX may overflow on the way in one order
    and not in another (skipped), and one whose squares pass DBL_MAX has sum of squares +inf."""
    big = Fraction(float(np.finfo(np.float64).max))
    worst = 0.0
    for j, (s, q, a, ln) in enumerate(exact):
        if s is None:
            continue
        if a <= big:
            assert np.isfinite(got_sum[j]), f"{what}: sum of line {j} is {got_sum[j]}"
            err, bound = abs(Fraction(float(got_sum[j])) - s), ln * _U53 * a
            worst = max(worst, float(err / bound) if bound else 0.0)
            assert err <= bound, f"{what}: sum of line {j} (length {ln}) off by {float(err):.3e}, bound {float(bound):.3e}"
        if q > big:
            assert got_sq[j] == np.inf, f"{what}: sum of squares of line {j} is {got_sq[j]}, squares pass DBL_MAX"
            continue
        err = abs(Fraction(float(got_sq[j])) - q)
        bound = (ln + 1) * _U53 * q + ln * Fraction(1, 2 ** 1075) if dt == np.float64 else ln * _U53 * q
        worst = max(worst, float(err / bound) if bound else 0.0)
        assert err <= bound, f"{what}: sum of squares of line {j} (length {ln}) off by {float(err):.3e}, bound {float(bound):.3e}"
    print(f"{what}: largest error / bound {worst:.3f}")


# ---- fixtures -----------------------------------------------------------------------------------------------------------
ROW_WAVES = 16_384          # normalize_rows_kernel, row_stats_kernel: 4096 workgroups of four waves, one wave per row
ENTRY_THREADS = 2_097_152   # normalize_cols_kernel, log1p_kernel: 8192 workgroups of 256 threads


def _spread_columns(lens, n, rng):
    """ascending distinct columns for every row: entry j of a row of length L sits in [j n / L, (j + 1) n / L)"""
    lens = np.asarray(lens, np.int64)
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    L = np.repeat(lens, lens)
    j = np.arange(ptr[-1], dtype=np.int64) - np.repeat(ptr[:-1], lens)
    return ptr, (j * n) // L + (rng.random(ptr[-1]) * (n // np.maximum(L, 1))).astype(np.int64)


def stride_fixture():
    """(ptr, idx, integer values as int64, m, n): every grid-stride loop takes two full turns and a partial third"""
    m, n = 33_000, 3000
    rng = np.random.default_rng(1701)
    lens = rng.integers(110, 171, m)
    lens[::97] = 0
    lens[20_000] = lens[32_900] = 2500
    ptr, idx = _spread_columns(lens, n, rng)
    ival = rng.integers(-40, 41, ptr[-1])
    return ptr, idx, ival, m, n


def stride_sums(bounds, seed):
    """`sums` for normalize on the stride fixture, of length bounds[-1]: mostly positive, with a zero, a negative, a NaN,
    a +inf, a value so small that 1e4 / sum is +inf and one so large that 1e-20 / sum is 0 in every [bounds[t], bounds[t + 1])"""
    rng = np.random.default_rng(seed)
    sums = rng.uniform(0.5, 200.0, bounds[-1])
    special = [0.0, -3.0, np.nan, np.inf, 5e-324, 1.7e308, -np.inf, -0.0]
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        sums[rng.choice(np.arange(lo, hi), len(special), replace=False)] = special
    return sums


STRIDE_ROW_TURNS = (0, ROW_WAVES, 2 * ROW_WAVES, 33_000)   # the rows each turn of the wave-per-row kernels takes
STRIDE_COL_THIRDS = (0, 1000, 2000, 3000)                  # (every column has entries in every turn of the per-entry kernels)
STRIDE_TARGETS = (1e4, 1e-20)   # 1e4 / 5e-324 = +inf; 1e-20 / 1.7e308 underflows to 0 (no single target does both)


def wide_fixture():
    """(ptr, idx, integer values, m, n): more than two turns of lines after the transposition, empty columns, one full"""
    m, n = 300, 40_000
    rng = np.random.default_rng(1702)
    stored = rng.random((m, n)) < 0.01
    stored[:, ::101] = False
    stored[:, 12_345] = True
    r, c = np.nonzero(stored)
    ptr = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=m))]).astype(np.int64)
    return ptr, c.astype(np.int64), rng.integers(-40, 41, len(c)), m, n


RAGGED_LENGTHS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 1000, 5000)


def ragged_fixture(dtype):
    n = 6000
    rng = np.random.default_rng(1703)
    lens = rng.permutation(np.repeat(RAGGED_LENGTHS, 3))
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    idx = np.concatenate([np.sort(rng.choice(n, k, replace=False)) for k in lens]).astype(np.int64)
    val = (rng.standard_normal(ptr[-1]) * 10.0 ** rng.uniform(-3, 3, ptr[-1])).astype(dtype)
    return ptr, idx, val, len(lens), n


def special_rows(dtype):
    """the rows of the special-value fixture, as lists of values.  Long rows (130 entries: lane 0 of the wave holds
    entries 0, 64 and 128) carry each special once at entry 0 (the first stored value), once at entry 64 (lane 0's
    share, later in the row) and once at entry 70 (another lane)."""
    T = np.dtype(dtype).type
    fi = np.finfo(dtype)
    big, tiny, sub = fi.max, fi.tiny, fi.smallest_subnormal
    nan, inf = np.nan, np.inf
    rng = np.random.default_rng(1704)
    rows = [[inf], [inf, inf, inf], [-inf], [-inf, -inf], [nan, 2.0, -3.0], [1.5, nan, -2.5], [1.5, -2.5, nan], [nan], [nan, nan, nan],
            [inf, nan, nan], [-inf, nan], [nan, inf], [nan, -inf], [inf, -inf], [-inf, 4.0, inf],
            [big, 1.0, -big], [-big, 2.0, big], [big], [-big],
            [sub, 3 * sub, -2 * sub], [-sub], [tiny / 2, tiny / 4, sub],
            [-0.0, 0.0], [0.0, -0.0], [-0.0], [0.0, 0.0, 0.0], [-0.0, -1.0], [0.0, 1.0], [], [7.0], [-7.0, 7.0]]
    for special in (nan, inf, -inf, big, -big, sub, -0.0):
        for pos in (0, 64, 70):
            row = rng.standard_normal(130) * 10.0 ** rng.uniform(-2, 2, 130)
            row[pos] = special
            rows.append(list(row))
    rows.append([inf] * 130)
    rows.append([-inf] * 70)
    rows.append([nan] * 130)
    rows.append([nan] * 64 + [5.0])
    rows.append([inf] + [nan] * 129)
    rows.append(list((rng.integers(1, 200, 130) * np.float64(sub))))
    rows.append([0.0, -0.0] * 65)
    return [np.array(r, np.float64).astype(T) for r in rows]


def special_fixture(dtype, transposed=False):
    """(ptr, idx, val, m, n) of the special-value matrix S: row i holds special_rows[i] in consecutive columns from a
    per-row offset, so S^T (transposed=True, again a canonical CSR) has the same lines as its columns"""
    rows = special_rows(dtype)
    n = 200
    r = np.concatenate([np.full(len(v), i) for i, v in enumerate(rows)]).astype(np.int64)
    c = np.concatenate([(7 * i) % (n - 130) + np.arange(len(v)) for i, v in enumerate(rows)]).astype(np.int64)
    v = np.concatenate(rows).astype(dtype)
    m = len(rows)
    if transposed:
        order = np.lexsort((r, c))
        r, c, v, m, n = c[order], r[order], v[order], n, m
    ptr = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=m))]).astype(np.int64)
    return ptr, c, v, m, n


def normalize_special_values(dtype):
    """one short matrix for the normalize specials: every row holds +-0.0, subnormals, T::MAX, +-inf, NaN and ordinary
    values; `sums` are chosen per row (with target 1) to scale into the subnormal range, to overflow, and to do nothing"""
    fi = np.finfo(dtype)
    base = np.array([0.0, -0.0, fi.smallest_subnormal, -3 * fi.smallest_subnormal, fi.tiny, fi.max, -fi.max, np.inf, -np.inf, np.nan,
                     1.0, -1.5, 3.0000001, 1 / 3, 12345.678, fi.tiny * 1.7, 1e-3, -2e5], np.float64).astype(dtype)
    # target 1: scale = 1 / sum
    sums = [1.0 / (float(fi.tiny) * 0.37), 1.0 / (float(fi.tiny) * 1e-3), 1.0 / (float(fi.smallest_subnormal) * 2.5),   # ordinary values land between subnormals
            1.0 / (float(fi.max) * 0.75), 1.0 / float(fi.max), 1e-300 if dtype == np.float64 else 1e-40,                # ordinary values overflow to inf
            1.0, 3.0, 0.1, 5e-324,                                                                                      # plain scales; scale = +inf
            0.0, -1.0, np.nan, np.inf]                                                                                  # scale not > 0: the row is left alone
    m, k = len(sums), len(base)
    ptr = np.arange(0, (m + 1) * k, k, dtype=np.int64)
    idx = np.tile(np.arange(k, dtype=np.int64), m)
    return ptr, idx, np.tile(base, m), m, k, np.array(sums, np.float64)


def log1p_classes(dtype):
    """{class: values} of the log1p inputs beyond the table of exact specials"""
    fi = np.finfo(dtype)
    T = np.dtype(dtype).type
    eps = float(fi.eps)
    rng = np.random.default_rng(1705)
    return {
        "tiny": np.array([eps / 4, -eps / 4, eps / 8, -eps / 1024, float(fi.tiny), -float(fi.tiny), 1e-30, -1e-30], np.float64).astype(T),
        "subnormal": np.array([float(fi.smallest_subnormal) * k for k in (1, -1, 2, 1000, -77777)], np.float64).astype(T),
        "near_eps": np.array([eps / 2, eps, 3 * eps, -eps / 2, -eps], np.float64).astype(T),
        "minus_one_to_zero": np.concatenate([-rng.random(4000), -(1 - 10.0 ** rng.uniform(-7, 0, 2000)), -(10.0 ** rng.uniform(-7, 0, 2000))]).astype(T),
        "positive": (10.0 ** rng.uniform(-12, 6, 8000)).astype(T),
    }
