"""Brute-force reference of the neighbour search (sapca_knn_device_*, Session.knn) in numpy, f64: every pairwise value by the
direct formula, np.lexsort on (value, index), self excluded by index.

values   euclidean: sqrt(sum (a - b)^2);  cosine: <a, b> / sqrt(|a|^2 |b|^2);  pearson: the cosine of the rows minus their
         own means (the reference's raw-moment expression, similarity/mod.rs:69-101, without its cancellation).
zero row a row whose norm (after centring, for pearson) is <= sqrt(eps_T) has similarity 0 to everything: the library's one
         deviation from the reference, which tests the pair's norm product against T::epsilon().  `T` is the dtype the
         library is run in; it enters nowhere else.
order    ascending distance / descending similarity, then ascending corpus index.
"""
import numpy as np

METRICS = ("euclidean", "cosine", "pearson")


def zero_norm(T):
    return float(np.sqrt(np.finfo(T).eps))


def _prepared(X, metric):
    """(rows as the similarity formulas use them, their norms), f64"""
    X = np.asarray(X, dtype=np.float64)
    if metric == "pearson":
        X = X - X.mean(axis=1, keepdims=True)
    return X, np.sqrt((X * X).sum(axis=1))


def pairwise(Q, C, metric, T=np.float64, chunk=64):
    """mq x mc values (f64) by the direct formulas"""
    assert metric in METRICS
    Q = np.asarray(Q, dtype=np.float64)
    C = np.asarray(C, dtype=np.float64)
    out = np.empty((Q.shape[0], C.shape[0]))
    if metric == "euclidean":
        for lo in range(0, Q.shape[0], chunk):
            df = Q[lo:lo + chunk, None, :] - C[None, :, :]
            out[lo:lo + chunk] = np.sqrt((df * df).sum(axis=2))
        return out
    Qp, nq = _prepared(Q, metric)
    Cp, nc = _prepared(C, metric)
    zq, zc = nq <= zero_norm(T), nc <= zero_norm(T)
    for lo in range(0, Q.shape[0], chunk):
        dot = (Qp[lo:lo + chunk, None, :] * Cp[None, :, :]).sum(axis=2)
        with np.errstate(divide="ignore", invalid="ignore"):
            out[lo:lo + chunk] = dot / np.sqrt((nq[lo:lo + chunk, None] ** 2) * (nc[None, :] ** 2))
    out[zq, :] = 0.0
    out[:, zc] = 0.0
    return out


def full_order(values, metric, exclude_self=False):
    """(order, sorted values): per query every admissible corpus row, best first; with exclude_self row i's list lacks i
    (one column shorter)"""
    mq, mc = values.shape
    key = values if metric == "euclidean" else -values
    idx = np.broadcast_to(np.arange(mc), (mq, mc))
    order = np.lexsort((idx, key), axis=1)
    if exclude_self:
        keep = order != np.arange(mq)[:, None]
        keep[mc:] = True                                     # (queries beyond the corpus have no self; they lose their last)
        keep[mc:, -1] = False
        order = order[keep].reshape(mq, mc - 1)
    return order, np.take_along_axis(values, order, axis=1)


def knn(Q, C, n_neighbors, metric, exclude_self=False, T=np.float64):
    """(indices int32, values f64), mq x n_neighbors"""
    order, vals = full_order(pairwise(Q, C, metric, T), metric, exclude_self)
    assert n_neighbors <= order.shape[1]
    return order[:, :n_neighbors].astype(np.int32), vals[:, :n_neighbors]


def values_at(Q, C, idx, metric, T=np.float64):
    """the values of the pairs (i, idx[i, j]) by the direct formulas in extended precision (np.longdouble), for the
    comparison of returned values to a few ulp of T; an index of -1 gives NaN"""
    LD = np.longdouble
    Q = np.asarray(Q, dtype=np.float64).astype(LD)
    C = np.asarray(C, dtype=np.float64).astype(LD)
    idx = np.asarray(idx)
    out = np.full(idx.shape, np.nan, dtype=LD)
    if metric != "euclidean":
        if metric == "pearson":
            Q = Q - Q.mean(axis=1, keepdims=True)
            C = C - C.mean(axis=1, keepdims=True)
        nq, nc = np.sqrt((Q * Q).sum(axis=1)), np.sqrt((C * C).sum(axis=1))
    for i in range(idx.shape[0]):
        ok = idx[i] >= 0
        B = C[idx[i][ok]]
        if metric == "euclidean":
            df = B - Q[i]
            out[i, ok] = np.sqrt((df * df).sum(axis=1))
        else:
            nb = nc[idx[i][ok]]
            v = (B * Q[i]).sum(axis=1) / np.sqrt(nq[i] ** 2 * nb ** 2) if nq[i] > 0 else np.zeros(B.shape[0], LD)
            v = np.where((nb <= zero_norm(T)) | (nq[i] <= zero_norm(T)), LD(0), v)
            out[i, ok] = v
    return out


def is_sorted(idx, val, metric):
    """every list ordered by (value, index): ascending distance / descending similarity, ties by ascending index"""
    key = np.asarray(val, dtype=np.float64)
    key = key if metric == "euclidean" else -key
    a, b = key[:, :-1], key[:, 1:]
    return bool(np.all((a < b) | ((a == b) & (idx[:, :-1] < idx[:, 1:]))))


def swap_bound(Q, C, T):
    """per query: what the rounding of the selection's inner products can cost, in squared-distance units:
    4 d eps_T (|a| + max |b|)^2 -- an FMA chain of length d on both sides of a swap"""
    Q = np.asarray(Q, dtype=np.float64)
    C = np.asarray(C, dtype=np.float64)
    d = Q.shape[1]
    na = np.sqrt((Q * Q).sum(axis=1))
    nb = np.sqrt((C * C).sum(axis=1)).max()
    return 4.0 * d * float(np.finfo(T).eps) * (na + nb) ** 2
