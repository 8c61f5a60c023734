"""The canonical form of a CSR matrix on the host, numpy only: the reference sapca_canonicalize_csr_device_* is held to.

Per row a STABLE sort by column (np.lexsort on (stored position, column)), then every run of equal columns becomes one
entry whose value is the plain left-to-right sum of the run, in the matrix's dtype, in stored order.  scipy's
sum_duplicates sorts with an unstable sort, so its sums can differ in the last bit; it is a reference only where the
values sum exactly.  An entry that does not merge is moved as its bit pattern (no arithmetic touches it).

    3 x 5, stored order:   row 0: (3, 1.0) (1, 2.0) (3, 4.0) (0, 8.0)      row 1: (empty)      row 2: (4, 0.5) (4, 0.25)
    ptr = [0, 4, 4, 6]     idx = [3, 1, 3, 0, 4, 4]     val = [1, 2, 4, 8, 0.5, 0.25]
    canonical:             row 0: (0, 8.0) (1, 2.0) (3, 1.0 + 4.0)         row 1: (empty)      row 2: (4, 0.5 + 0.25)
    ptr = [0, 3, 3, 4]     idx = [0, 1, 3, 4]           val = [8, 2, 5, 0.75]
"""
import numpy as np


def canonicalize(ptr, idx, val):
    """(ptr int64, idx int32, val) of the canonical form; inputs are host arrays with sound offsets"""
    ptr = np.asarray(ptr, dtype=np.int64)
    idx = np.asarray(idx)
    val = np.asarray(val)
    m = ptr.size - 1
    row = np.repeat(np.arange(m, dtype=np.int64), np.diff(ptr))
    pos = np.arange(idx.size, dtype=np.int64)
    order = np.lexsort((pos, idx.astype(np.int64), row))          # by row, then column, then stored position: stable
    c, v, r = idx[order], val[order], row[order]
    head = np.ones(c.size, dtype=bool)
    head[1:] = (c[1:] != c[:-1]) | (r[1:] != r[:-1])
    starts = np.flatnonzero(head)
    out_val = v[starts].copy()                                     # bit patterns of the heads, untouched
    run_len = np.diff(np.append(starts, c.size))
    for j in np.flatnonzero(run_len > 1):                          # the runs that merge: left to right, in the dtype
        s = v[starts[j]]
        for x in v[starts[j] + 1: starts[j] + run_len[j]]:
            s = val.dtype.type(s + x)
        out_val[j] = s
    out_ptr = np.zeros(m + 1, dtype=np.int64)
    np.cumsum(np.bincount(r[starts], minlength=m), out=out_ptr[1:])
    return out_ptr, c[starts].astype(np.int32), out_val
