"""Host restatements of the reference's masked and chunk statistics (src/sparse/csr.rs:124-252, 394-556, 728-1008) for the
tests:

- `masked_stats` and the fourteen method names below it: numpy restatements, vectorised, in f64, in the shape of the C ABI
  (sapca_masked_stats_csr_device_*) and of the Python `ResidentCsr` methods;
- `ref_*`: literal transliterations of the reference loops, slow, for small matrices only.  They check the
  restatements; the restatements check the library.
"""
import numpy as np

ROW, COLUMN = 0, 1


def _rows(ptr):
    ptr = np.asarray(ptr, np.int64)
    return np.repeat(np.arange(len(ptr) - 1, dtype=np.int64), np.diff(ptr))


def masked_stats(ptr, idx, val, m, n, direction, mask=None):
    """(sum, sum_squared, count, var): the contract of sapca_masked_stats_csr_device_*.  ROW: per row, over the stored
    entries whose column is kept; COLUMN: per column, over those whose row is kept.  var: ROW sum (x - mean)^2 / count,
    COLUMN sumsq / count - mean^2, 0 where count is 0.  A mask longer than the masked dimension: its tail is ignored."""
    idx = np.asarray(idx, np.int64)
    x = np.asarray(val, np.float64)
    rows = _rows(ptr)
    if direction == ROW:
        ln, key, other = m, rows, idx
    else:
        ln, key, other = n, idx, rows
    keep = np.ones(len(x), bool) if mask is None else np.asarray(mask, bool)[other]
    key, x = key[keep], x[keep]
    cnt = np.bincount(key, minlength=ln)[:ln]
    s = np.bincount(key, weights=x, minlength=ln)[:ln].astype(np.float64)   # (an empty selection gives int64 zeros)
    q = np.bincount(key, weights=x * x, minlength=ln)[:ln].astype(np.float64)
    c = cnt.astype(np.float64)
    with np.errstate(invalid="ignore"):   # (inf - inf in a line holding an inf: nan, as on the device)
        mean = np.divide(s, c, out=np.zeros(ln), where=cnt > 0)
        if direction == ROW:
            m2 = np.bincount(key, weights=(x - mean[key]) ** 2, minlength=ln)[:ln]
            var = np.divide(m2, c, out=np.zeros(ln), where=cnt > 0)
        else:
            var = np.where(cnt > 0, np.divide(q, c, out=np.zeros(ln), where=cnt > 0) - mean * mean, 0.0)
    return s, q, cnt.astype(np.uint64), var


# ---- the fourteen methods, restated ----------------------------------------------------------------------------------
def nonzero_col_masked(ptr, idx, val, m, n, mask):
    return masked_stats(ptr, idx, val, m, n, COLUMN, mask)[2]


def nonzero_row_masked(ptr, idx, val, m, n, mask):
    return masked_stats(ptr, idx, val, m, n, ROW, mask)[2]


def sum_col_masked(ptr, idx, val, m, n, mask):
    return masked_stats(ptr, idx, val, m, n, COLUMN, mask)[0]


def sum_row_masked(ptr, idx, val, m, n, mask):
    return masked_stats(ptr, idx, val, m, n, ROW, mask)[0]


def var_col_masked(ptr, idx, val, m, n, mask):
    return masked_stats(ptr, idx, val, m, n, COLUMN, mask)[3]


def var_row_masked(ptr, idx, val, m, n, mask):
    return masked_stats(ptr, idx, val, m, n, ROW, mask)[3]


def nonzero_col_chunk(ptr, idx, val, m, n, reference):
    k = min(len(reference), n)
    reference[:k] += masked_stats(ptr, idx, val, m, n, COLUMN)[2][:k].astype(reference.dtype)
    return reference


def nonzero_row_chunk(ptr, idx, val, m, n, reference):
    k = min(len(reference), m)
    reference[:k] += masked_stats(ptr, idx, val, m, n, ROW)[2][:k].astype(reference.dtype)
    return reference


def sum_col_chunk(ptr, idx, val, m, n, reference):
    k = min(len(reference), n)
    reference[:k] += masked_stats(ptr, idx, val, m, n, COLUMN)[0][:k].astype(reference.dtype)
    return reference


def sum_row_chunk(ptr, idx, val, m, n, reference):
    reference[:m] = masked_stats(ptr, idx, val, m, n, ROW)[0]
    return reference


def var_col_chunk(ptr, idx, val, m, n, reference):
    reference[:] = masked_stats(ptr, idx, val, m, n, COLUMN)[3]
    return reference


def var_row_chunk(ptr, idx, val, m, n, reference):
    reference[:] = masked_stats(ptr, idx, val, m, n, ROW)[3]
    return reference


def _min_max(ptr, idx, val, m, n, direction):
    """(has entries, min, max) per line over the stored values, compared as the reference compares (`<`, `>`: a NaN never
    wins).  COLUMN: from (+inf, -inf), so that narrowing the caller's arrays with the result is the reference's loop;
    ROW: from the row's first stored value -- a row that begins with a NaN is (NaN, NaN)."""
    ptr = np.asarray(ptr, np.int64)
    x = np.asarray(val)
    dt = x.dtype if x.dtype.kind == "f" else np.float64
    x = x.astype(dt)
    ln = m if direction == ROW else n
    lo, hi = np.full(ln, np.inf, dt), np.full(ln, -np.inf, dt)
    if direction == ROW:
        has = np.diff(ptr) > 0
        j = np.flatnonzero(has)
        if j.size:
            first = x[ptr[j]]
            lo[j] = np.where(np.isnan(first), first, np.fmin.reduceat(x, ptr[j]))
            hi[j] = np.where(np.isnan(first), first, np.fmax.reduceat(x, ptr[j]))
        return has, lo, hi
    key = np.asarray(idx, np.int64)
    np.fmin.at(lo, key, x)      # fmin / fmax skip a nan operand
    np.fmax.at(hi, key, x)
    return np.bincount(key, minlength=ln)[:ln] > 0, lo, hi


def min_max_col_chunk(ptr, idx, val, m, n, reference):
    mins, maxs = reference
    has, lo, hi = _min_max(ptr, idx, val, m, n, COLUMN)
    j = np.flatnonzero(has)
    mins[j] = np.where(lo[j] < mins[j], lo[j], mins[j])     # (a nan in the caller's arrays stays: nothing is < or > it)
    maxs[j] = np.where(hi[j] > maxs[j], hi[j], maxs[j])
    return reference


def min_max_row_chunk(ptr, idx, val, m, n, reference):
    mins, maxs = reference
    has, lo, hi = _min_max(ptr, idx, val, m, n, ROW)
    j = np.flatnonzero(has)
    mins[j], maxs[j] = lo[j], hi[j]
    return reference


# ---- the reference loops, transliterated ----------------------------------------------------------------------------
def ref_nonzero_col_masked(ptr, idx, val, m, n, mask):   # csr.rs:153-186
    if len(mask) < m:
        raise ValueError(f"Mask length ({len(mask)}) is less than number of rows ({m})")
    result = [0] * n
    for row in range(m):
        if not mask[row]:
            continue
        for e in range(ptr[row], ptr[row + 1]):
            result[idx[e]] += 1
    return result


def ref_nonzero_row_masked(ptr, idx, val, m, n, mask):   # csr.rs:188-252
    if len(mask) < n:
        raise ValueError(f"Mask length ({len(mask)}) is less than number of columns ({n})")
    result = []
    for row in range(m):
        count = 0
        for e in range(ptr[row], ptr[row + 1]):
            if mask[idx[e]]:
                count += 1
        result.append(count)
    return result


def ref_sum_col_masked(ptr, idx, val, m, n, mask):   # csr.rs:418-488 (the serial branch)
    if len(mask) < m:
        raise ValueError(f"Mask length ({len(mask)}) is less than number of rows ({m})")
    result = [0.0] * n
    for row, included in enumerate(mask):
        if included:
            for e in range(ptr[row], ptr[row + 1]):
                result[idx[e]] += float(val[e])
    return result


def ref_sum_row_masked(ptr, idx, val, m, n, mask):   # csr.rs:490-556 (the serial branch)
    if len(mask) < n:
        raise ValueError(f"Mask length ({len(mask)}) is less than number of columns ({n})")
    result = []
    for row in range(m):
        s = 0.0
        for e in range(ptr[row], ptr[row + 1]):
            if mask[idx[e]]:
                s += float(val[e])
        result.append(s)
    return result


def ref_var_col_masked(ptr, idx, val, m, n, mask):   # csr.rs:815-862
    if len(mask) < m:
        raise ValueError(f"Mask length ({len(mask)}) is less than number of rows ({m})")
    s = ref_sum_col_masked(ptr, idx, val, m, n, mask)
    count = ref_nonzero_col_masked(ptr, idx, val, m, n, mask)
    result, squared = [0.0] * n, [0.0] * n
    for row in range(m):
        if not mask[row]:
            continue
        for e in range(ptr[row], ptr[row + 1]):
            squared[idx[e]] += float(val[e]) * float(val[e])
    for c in range(n):
        if count[c] > 0:
            mean = s[c] / count[c]
            result[c] = squared[c] / count[c] - mean * mean
    return result


def ref_var_row_masked(ptr, idx, val, m, n, mask):   # csr.rs:864-914
    if len(mask) < n:
        raise ValueError(f"Mask length ({len(mask)}) is less than number of columns ({n})")
    s = ref_sum_row_masked(ptr, idx, val, m, n, mask)
    count = ref_nonzero_row_masked(ptr, idx, val, m, n, mask)
    result = [0.0] * m
    for row in range(m):
        if count[row] > 0:
            mean = s[row] / count[row]
            d2 = 0.0
            for e in range(ptr[row], ptr[row + 1]):
                if not mask[idx[e]]:
                    continue
                d2 += (float(val[e]) - mean) ** 2
            result[row] = d2 / count[row]
    return result


def ref_nonzero_col_chunk(ptr, idx, val, m, n, reference):   # csr.rs:124-134
    for c in idx:
        if c < len(reference):
            reference[c] += 1
    return reference


def ref_nonzero_row_chunk(ptr, idx, val, m, n, reference):   # csr.rs:136-150
    for i in range(m):
        if i < len(reference):
            reference[i] += ptr[i + 1] - ptr[i]
    return reference


def ref_sum_col_chunk(ptr, idx, val, m, n, reference):   # csr.rs:394-405
    for c, x in zip(idx, val):
        if c < len(reference):
            reference[c] += float(x)
    return reference


def ref_sum_row_chunk(ptr, idx, val, m, n, reference):   # csr.rs:407-416 (panics on a short reference)
    for row in range(m):
        reference[row] = sum(float(val[e]) for e in range(ptr[row], ptr[row + 1]))
    return reference


def ref_var_col_chunk(ptr, idx, val, m, n, reference):   # csr.rs:728-771
    if len(reference) != n:
        raise ValueError(f"Reference slice length {len(reference)} does not match number of columns {n}")
    s, count, squared = [0.0] * n, [0] * n, [0.0] * n
    for c, x in zip(idx, val):
        s[c] += float(x)
        count[c] += 1
        squared[c] += float(x) * float(x)
    for c in range(n):
        if count[c] > 0:
            mean = s[c] / count[c]
            reference[c] = squared[c] / count[c] - mean * mean
        else:
            reference[c] = 0.0
    return reference


def ref_var_row_chunk(ptr, idx, val, m, n, reference):   # csr.rs:773-813
    if len(reference) != m:
        raise ValueError(f"Reference slice length {len(reference)} does not match number of rows {m}")
    for row in range(m):
        xs = [float(val[e]) for e in range(ptr[row], ptr[row + 1])]
        if xs:
            mean = sum(xs) / len(xs)
            reference[row] = sum((x - mean) ** 2 for x in xs) / len(xs)
        else:
            reference[row] = 0.0
    return reference


def ref_min_max_col_chunk(ptr, idx, val, m, n, reference):   # csr.rs:939-973 (panics on a column past the arrays)
    mins, maxs = reference
    for row in range(m):
        for e in range(ptr[row], ptr[row + 1]):
            c, x = idx[e], val[e]
            if x < mins[c]:
                mins[c] = x
            if x > maxs[c]:
                maxs[c] = x
    return reference


def ref_min_max_row_chunk(ptr, idx, val, m, n, reference):   # csr.rs:975-1008
    mins, maxs = reference
    for row in range(m):
        if ptr[row] < ptr[row + 1]:
            lo = hi = val[ptr[row]]
            for e in range(ptr[row], ptr[row + 1]):
                if val[e] < lo:
                    lo = val[e]
                if val[e] > hi:
                    hi = val[e]
            mins[row], maxs[row] = lo, hi
    return reference


MASKED = ("nonzero_col_masked", "nonzero_row_masked", "sum_col_masked", "sum_row_masked", "var_col_masked", "var_row_masked")
CHUNK = ("nonzero_col_chunk", "nonzero_row_chunk", "sum_col_chunk", "sum_row_chunk", "var_col_chunk", "var_row_chunk",
         "min_max_col_chunk", "min_max_row_chunk")
