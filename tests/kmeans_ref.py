"""A numpy restatement in f64 of the k-means of include/sapca.h (sapca_kmeans_*): the k-means++ seeding under the library's
counter generator, the assignment by the direct formula, the update, and Lloyd's loop under scikit-learn's stopping rule.
tests/test_kmeans_cpu.py holds it to scikit-learn's own KMeans; the GPU tests hold the library to it.

Besides the results every stage reports how close it came to a decision that rounding could turn: an assignment its smallest
relative margin, (second - best) / (|x| + max |c|)^2, a seeding step the relative distance of u_t S from the nearest prefix
boundary, the loop the relative distance of every shift from tol_abs."""
import numpy as np

STREAM = 21          # the stream of the seeding's uniforms in the counter generator
_M64 = (1 << 64) - 1


def _mix64(z):
    z = (z + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def hash_u01(seed, stream, idx):
    """csrc/hash_u01.h in Python integers: the uniform in [0, 1) of (seed, stream, idx)."""
    key = (seed * 0xD1342543DE82EF95 + stream * 0x2545F4914F6CDD1D + 0x1234567) & _M64
    z = _mix64((idx ^ key) & _M64)
    z = _mix64((z + key) & _M64)
    return float(z >> 11) * (1.0 / 9007199254740992.0)


def uniforms(seed, k):
    return np.array([hash_u01(int(seed), STREAM, t) for t in range(k)])


def dist2(X, c):
    """|x_i - c|^2 for every row, the direct formula in f64"""
    df = np.asarray(X, dtype=np.float64) - np.asarray(c, dtype=np.float64)
    return (df * df).sum(axis=1)


def dist2_exact(X, Cl):
    """|x_i - Cl_i|^2 row by row in extended precision, rounded once to f64: what d_dist2 and the inertia are held to"""
    df = np.asarray(X, dtype=np.longdouble) - np.asarray(Cl, dtype=np.longdouble)
    return (df * df).sum(axis=1).astype(np.float64)


def seed(X, k, seed_):
    """(rows, boundary): the k chosen rows, and per step the distance of u_t S_{m-1} from the nearest S_i relative to S_{m-1}
    (inf for centre 0 and for the zero-total fallback, which do not search)."""
    X = np.asarray(X)
    m = X.shape[0]
    u = uniforms(seed_, k)
    rows = np.zeros(k, dtype=np.int64)
    boundary = np.full(k, np.inf)
    rows[0] = min(int(np.floor(u[0] * m)), m - 1)
    D = None
    for t in range(1, k):
        dt = dist2(X, X[rows[t - 1]])
        D = dt if D is None else np.minimum(D, dt)
        S = np.cumsum(D)
        if S[-1] == 0.0:
            rows[t] = min(int(np.floor(u[t] * m)), m - 1)
            continue
        thr = u[t] * S[-1]
        rows[t] = min(int(np.searchsorted(S, thr, side="right")), m - 1)    # the first i with S_i > thr
        boundary[t] = np.abs(S - thr).min() / S[-1]
    return rows, boundary


def assign(X, C):
    """(labels, dist2, margin): argmin_c |x_i - c|^2 with ties to the lower c, the squared distance to it (dist2_exact), and
    per row (second smallest - smallest) / (|x_i| + max_c |c|)^2 (inf for a single centroid)."""
    X = np.asarray(X, dtype=np.float64)
    C = np.asarray(C, dtype=np.float64)
    D = np.stack([dist2(X, c) for c in C], axis=1)
    labels = D.argmin(axis=1)
    best = D[np.arange(len(X)), labels]
    if C.shape[0] > 1:
        rest = D.copy()
        rest[np.arange(len(X)), labels] = np.inf
        scale = (np.sqrt((X * X).sum(axis=1)) + np.sqrt((C * C).sum(axis=1)).max()) ** 2
        with np.errstate(divide="ignore", invalid="ignore"):
            margin = np.where(scale > 0, (rest.min(axis=1) - best) / scale, 0.0)
    else:
        margin = np.full(len(X), np.inf)
    return labels.astype(np.int32), dist2_exact(X, C[labels]), margin


def update(X, labels, C, dtype=np.float64):
    """(centroids, counts): f64 sum / count rounded once to dtype; a cluster without rows keeps its row of C; a label outside
    [0, k) belongs to no cluster."""
    X = np.asarray(X, dtype=np.float64)
    out = np.array(C, dtype=dtype, copy=True)
    k = out.shape[0]
    counts = np.zeros(k, dtype=np.int64)
    for c in range(k):
        rows = X[np.asarray(labels) == c]
        counts[c] = len(rows)
        if len(rows):
            # (the sum in extended precision: the reference's own summation error stays far below an ulp of f64)
            out[c] = (rows.astype(np.longdouble).sum(axis=0).astype(np.float64) / len(rows)).astype(dtype)
    return out, counts


def tol_abs(X, tol):
    """tol x the mean over the columns of the column's population variance, two passes in f64"""
    X = np.asarray(X, dtype=np.float64)
    mean = X.sum(axis=0) / X.shape[0]
    return tol * ((((X - mean) ** 2).sum(axis=0) / X.shape[0]).sum() / X.shape[1])


def lloyd(X, C0, max_iter=300, tol=1e-4, dtype=np.float64):
    """Lloyd's loop of the header on X (held in `dtype`, arithmetic in f64, the centroids rounded to dtype at every update).
    Returns a dict: labels, centroids (dtype), update_labels (the labels the returned centroids are the update of; None when no
    update ran), inertia, n_iter, strict, min_margin (the smallest relative margin of any assignment along the run), tol_gap (the smallest |shift - tol_abs| / tol_abs met; inf when tol == 0)."""
    X = np.asarray(X, dtype=dtype)
    C = np.array(C0, dtype=dtype, copy=True)
    ta = tol_abs(X, tol) if tol > 0 else 0.0
    labels = prev = updated = None
    strict = False
    n_iter = 0
    min_margin, tol_gap = np.inf, np.inf
    for i in range(int(max_iter)):
        labels, _, margin = assign(X, C)
        min_margin = min(min_margin, margin.min())
        C_new, _ = update(X, labels, C, dtype)
        updated = labels
        shift = ((C_new.astype(np.float64) - C.astype(np.float64)) ** 2).sum()
        C = C_new
        n_iter = i + 1
        if i > 0 and np.array_equal(labels, prev):
            strict = True
            break
        if ta > 0:
            tol_gap = min(tol_gap, abs(shift - ta) / ta)
        if shift <= ta:
            break
        prev = labels
    if not strict:
        labels, _, margin = assign(X, C)
        min_margin = min(min_margin, margin.min())
    inertia = dist2_exact(X, C[labels]).sum() if len(X) else 0.0
    return dict(labels=labels, centroids=C, update_labels=updated, inertia=float(inertia), n_iter=n_iter, strict=strict, min_margin=float(min_margin),
                tol_gap=float(tol_gap))


def blobs(m, d, k, spread, seed_):
    """(X, truth): m rows around k standard-normal centres in d dimensions with N(0, spread^2) noise, every column centred"""
    rng = np.random.default_rng(seed_)
    centres = rng.normal(size=(k, d))
    truth = rng.integers(0, k, size=m)
    X = centres[truth] + spread * rng.normal(size=(m, d))
    return X - X.mean(axis=0), truth


def integer_case(m, d, k, seed_):
    """(X, C): integer coordinates in [-3, 3]; a fifth of the rows are copies of centroids or of other rows, and where k >= 2
    some centroids are copies of earlier ones, so that exact ties occur."""
    rng = np.random.default_rng(seed_)
    C = rng.integers(-3, 4, size=(k, d)).astype(np.float64)
    for c in range(1, k, 3):
        C[c] = C[rng.integers(0, c)]
    X = rng.integers(-3, 4, size=(m, d)).astype(np.float64)
    for i in range(0, m, 5):
        X[i] = C[rng.integers(0, k)] if (i // 5) % 2 == 0 else X[rng.integers(0, m)]
    return X, C
