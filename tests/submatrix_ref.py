"""Host restatement of sapca_select_submatrix_csr_device_* for the tests: A[rows][:, mask], optionally without stored
zeros, in pure numpy.  Output row i is source row rows[i]; its kept entries stay in stored order; a kept column becomes
the number of kept columns below it (MaskedCSRMatrix::new, sparse_masked/mod.rs:264-271, 455-466); values move as they
are (fancy indexing copies bytes: NaN payloads and -0.0 survive)."""
import numpy as np


def select_submatrix(ptr, idx, val, n, rows=None, mask=None, drop_stored_zeros=False):
    """(offsets int64, indices int32, values, n_cols) of A[rows][:, mask].  rows None: every row in order; mask None:
    every column.  drop_stored_zeros: entries whose value == 0 (either sign) are dropped; a NaN is kept."""
    ptr = np.asarray(ptr, np.int64)
    idx = np.asarray(idx)
    val = np.asarray(val)
    rows = np.arange(len(ptr) - 1, dtype=np.int64) if rows is None else np.asarray(rows, np.int64).reshape(-1)
    lens = ptr[rows + 1] - ptr[rows]
    goff = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    # the source entry of every gathered position: the row's base plus the position's place in the row
    src = np.repeat(ptr[rows] - goff[:-1], lens) + np.arange(goff[-1], dtype=np.int64)
    c, v = idx[src].astype(np.int64), val[src]
    keep = np.ones(src.size, bool)
    if mask is None:
        n_cols, rank = int(n), None
    else:
        mask = np.asarray(mask, bool)
        assert mask.size == n
        n_cols, rank = int(mask.sum()), np.cumsum(mask) - mask      # rank[c]: kept columns below c
        keep &= mask[c]
    if drop_stored_zeros:
        keep &= ~(v == 0)
    out_row = np.repeat(np.arange(rows.size, dtype=np.int64), lens)[keep]
    off = np.concatenate([[0], np.cumsum(np.bincount(out_row, minlength=rows.size))]).astype(np.int64)
    c = c[keep]
    return off, (c if rank is None else rank[c]).astype(np.int32), v[keep], n_cols
