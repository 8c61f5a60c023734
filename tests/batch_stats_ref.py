"""Host restatements of the reference's last three CSR traits (src/sparse/csr.rs:1081-1376) for the tests:

- `batch_stats` / `sum_row_n_top`: numpy restatements, vectorised, in the shape of the C ABI (dense codes, f64);
- `ref_*`: literal transliterations of the reference loops (HashMap grouping, two passes, sort_by + take(n)), slow, for
  small matrices only.  They check the restatements; the restatements check the library.
"""
import numpy as np


def batch_stats(ptr, idx, val, m, n, grouped_axis, codes, n_batches):
    """(mean, var, count), each n_batches x (n if grouped_axis == 0 else m): the contract of sapca_batch_stats_csr_device_*.
    Over the stored entries of line j with code b: count, var = sum (x - mu)^2 / (count - 1) (0 when count <= 1);
    mean = their sum / (number of rows or columns with code b)."""
    ptr, idx = np.asarray(ptr, np.int64), np.asarray(idx, np.int64)
    x = np.asarray(val, np.float64)
    codes = np.asarray(codes, np.int64)
    rows = np.repeat(np.arange(m, dtype=np.int64), np.diff(ptr))
    if grouped_axis == 0:
        ln, key = n, codes[rows] * n + idx
    else:
        ln, key = m, codes[idx] * m + rows
    size = n_batches * ln
    cnt = np.bincount(key, minlength=size)[:size]
    s = np.bincount(key, weights=x, minlength=size)[:size]
    mu = np.divide(s, cnt, out=np.zeros(size), where=cnt > 0)
    m2 = np.bincount(key, weights=(x - mu[key]) ** 2, minlength=size)[:size]
    var = np.divide(m2, cnt - 1, out=np.zeros(size), where=cnt > 1)
    group = np.bincount(codes, minlength=n_batches)[:n_batches].astype(np.float64)
    g = np.repeat(group, ln)
    mean = np.divide(s, g, out=np.zeros(size), where=g > 0)
    return mean.reshape(n_batches, ln), var.reshape(n_batches, ln), cnt.astype(np.uint64).reshape(n_batches, ln)


def sum_row_n_top(ptr, val, n, rows=None):
    """per row (all rows, or those listed in `rows`): the sum of the min(n, len) largest stored values, in f64"""
    ptr = np.asarray(ptr, np.int64)
    rows = range(len(ptr) - 1) if rows is None else rows
    out = np.zeros(len(rows))
    for o, r in enumerate(rows):
        x = np.sort(np.asarray(val[ptr[r]:ptr[r + 1]], np.float64))[::-1]
        out[o] = x[:n].sum()
    return out


# ---- the reference loops, transliterated ----------------------------------------------------------------------------
def _row(ptr, idx, val, r):
    return [(int(idx[j]), float(val[j])) for j in range(ptr[r], ptr[r + 1])]


def ref_var_batch_row(ptr, idx, val, m, n, batches):   # csr.rs:1088-1163
    if len(batches) != m:
        raise ValueError(f"Batch vector length ({len(batches)}) doesn't match matrix row count ({m})")
    batch_indices = {}
    for i, b in enumerate(batches):
        batch_indices.setdefault(b, []).append(i)
    result = {}
    for b, indices in batch_indices.items():
        means, counts, sum_sq, var = [0.0] * n, [0] * n, [0.0] * n, [0.0] * n
        for r in indices:
            for c, x in _row(ptr, idx, val, r):
                means[c] += x
                counts[c] += 1
        for c in range(n):
            if counts[c] > 0:
                means[c] /= counts[c]
        for r in indices:
            for c, x in _row(ptr, idx, val, r):
                sum_sq[c] += (x - means[c]) ** 2
        for c in range(n):
            if counts[c] > 1:
                var[c] = sum_sq[c] / (counts[c] - 1)
        result[b] = var
    return result


def ref_var_batch_col(ptr, idx, val, m, n, batches):   # csr.rs:1165-1244
    if len(batches) != n:
        raise ValueError(f"Batch vector length ({len(batches)}) doesn't match matrix column count ({n})")
    batch_columns = {}
    for c, b in enumerate(batches):
        batch_columns.setdefault(b, []).append(c)
    result = {}
    for b, cols in batch_columns.items():
        var = [0.0] * m
        for r in range(m):
            values = [x for c, x in _row(ptr, idx, val, r) if c in cols]
            if len(values) > 1:
                mean = sum(values) / len(values)
                var[r] = sum((x - mean) ** 2 for x in values) / (len(values) - 1)
        result[b] = var
    return result


def ref_mean_batch_row(ptr, idx, val, m, n, batches):   # csr.rs:1251-1296
    if len(batches) != n:
        raise ValueError(f"Number of batch identifiers ({len(batches)}) must match number of columns ({n})")
    batch_indices = {}
    for c, b in enumerate(batches):
        batch_indices.setdefault(b, []).append(c)
    result = {}
    for b, cols in batch_indices.items():
        means = [0.0] * m
        for c in cols:
            for r in range(m):
                for cc, x in _row(ptr, idx, val, r):   # get_entry(row, col)
                    if cc == c:
                        means[r] += x
        result[b] = [s / len(cols) for s in means]
    return result


def ref_mean_batch_col(ptr, idx, val, m, n, batches):   # csr.rs:1299-1343
    if len(batches) != m:
        raise ValueError(f"Number of batch identifiers ({len(batches)}) must match number of rows ({m})")
    batch_indices = {}
    for r, b in enumerate(batches):
        batch_indices.setdefault(b, []).append(r)
    result = {}
    for b, rows in batch_indices.items():
        means = [0.0] * n
        for r in rows:
            for c, x in _row(ptr, idx, val, r):
                means[c] += x
        result[b] = [s / len(rows) for s in means]
    return result


def ref_sum_row_n_top(ptr, idx, val, m, n_top):   # csr.rs:1350-1375
    result = [0.0] * m
    for r in range(m):
        values = [x for _, x in _row(ptr, idx, val, r)]
        if len(values) <= n_top:
            result[r] = sum(values)
        else:
            values.sort(reverse=True)
            result[r] = sum(values[:n_top])
    return result


def dense_codes(batches):
    """labels in order of first appearance and the code of every entry (the wrapper's mapping, restated)"""
    lut = {}
    codes = np.array([lut.setdefault(b, len(lut)) for b in batches], dtype=np.int32)
    return list(lut), codes


def to_dict(labels, table):
    return {b: table[c] for c, b in enumerate(labels)}
