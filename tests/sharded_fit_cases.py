"""Cases and a plain f64 reference for the row-sharded fit (sapca_multi_*, the members of a communicator inside Engine).

numpy and scipy only.  `partition` restates sapca_partition_rows plus the even-rows fallback of shard_bounds (multi.cpp);
`sharded_randomized_fit` is the algorithm of tests/test_dist_cpu.py as a loop over any number of shards in one process, with
its summation sites written out (statistics; the Gram of Y; the A^T panel together with 1^T Y; the per-column counts of the
reference projection).  Every matrix is small and integer-valued: column sums and sums of squares are exact in f64 and in f32,
whatever the order they are added in.  A planted block structure gives the gap the tolerances of tests/test_gpu_sharded_fit.py
rely on: k row and column clusters with distinct integer weights, one group of rows and columns outside every cluster (so the
centred operator keeps rank k), and sparse background entries of 1 and 2.  tests/test_sharded_fit_cases_cpu.py checks that
every case has the property it is listed for."""
import functools
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import scipy.linalg as sl
import scipy.sparse as sp
import torch

import sapca_oracle as O
from sapca import synth

EPS64 = float(np.finfo(np.float64).eps)


# ------------------------------------------------------------------------------------------ the partition
def nnz_bounds(indptr, nd):
    """sapca_partition_rows: boundary p is the first row whose prefix reaches floor(nnz p / nd), one row back where the earlier
    boundary is nearer, kept monotone; an empty matrix gets m p / nd"""
    ro = [int(x) for x in np.asarray(indptr).ravel()]
    m = len(ro) - 1
    nnz = ro[m] - ro[0]
    b = [0]
    for p in range(1, nd):
        target = ro[0] + nnz * p // nd
        r = int(np.searchsorted(np.asarray(ro, dtype=np.int64), target, side="left"))
        if 0 < r <= m and target - ro[r - 1] < ro[r] - target:
            r -= 1
        if nnz == 0:
            r = m * p // nd
        b.append(max(min(r, m), b[-1]))
    b.append(m)
    return np.asarray(b, dtype=np.int64)


def even_bounds(m, nd):
    return np.asarray([m * j // nd for j in range(nd + 1)], dtype=np.int64)


def partition(indptr, nd):
    """the row ranges sapca_multi_* give its members: nnz_bounds, or even row counts if a shard would have no rows"""
    b = nnz_bounds(indptr, nd)
    return even_bounds(len(np.asarray(indptr).ravel()) - 1, nd) if np.any(np.diff(b) == 0) else b


# ------------------------------------------------------------------------------------------ matrices
def planted(m, n, weights, d_in, d_bg, seed, gr=None, gc=None):
    """m x n, integer-valued f64 CSR.  Row i belongs to group i % (k + 1), column j to group j % (k + 1) (or to gr[i], gc[j]),
    k = len(weights); group k is outside every cluster.  A cell of cluster g (row and column group g < k) is stored with
    probability d_in and holds weights[g]; every other cell is stored with probability d_bg and holds 1 or 2."""
    k = len(weights)
    cell = torch.arange(m * n, dtype=torch.int64)
    u = synth.hash_u01(seed, 31, cell).numpy().reshape(m, n)
    two = synth.hash_u01(seed, 32, cell).numpy().reshape(m, n) < 0.5
    gr = np.arange(m) % (k + 1) if gr is None else np.asarray(gr)
    gc = np.arange(n) % (k + 1) if gc is None else np.asarray(gc)
    block = (gr[:, None] == gc[None, :]) & (gr[:, None] < k)
    w = np.asarray(list(weights) + [0], dtype=np.float64)[gr][:, None] * np.ones((1, n))
    D = np.where(block, np.where(u < d_in, w, 0.0), np.where(u < d_bg, np.where(two, 2.0, 1.0), 0.0))
    return _csr(D)


def _csr(D):
    A = sp.csr_matrix(np.asarray(D, dtype=np.float64))
    A.eliminate_zeros()
    A.sort_indices()
    A.indptr, A.indices = A.indptr.astype(np.int64), A.indices.astype(np.int64)
    return A


@functools.lru_cache(maxsize=None)
def matrix(key):
    if key == "balanced":        # (a): about 30 000 entries
        return planted(1500, 260, (12, 11, 10, 9, 8, 7), 0.6, 0.02, 3)
    if key == "empty_shard":     # (b): 60 planted rows, one full row of ones that holds two thirds of all entries, 1439 empty rows:
        # the last boundary is reached inside row 60, so the rows behind it are a shard of their own, with no entry
        D = np.zeros((1500, 2000))
        D[:60] = planted(60, 2000, (9, 7, 5), 0.9, 0.003, 21, gr=[0] * 20 + [1] * 20 + [2] * 20,
                         gc=[0] * 8 + [1] * 8 + [2] * 8 + [3] * 1976).toarray()
        D[60, :] = 1.0
        return _csr(D)
    if key == "short_30":        # (c)
        return planted(30, 200, (9, 7, 5, 3), 0.9, 0.03, 5)
    if key == "short_16":
        return planted(16, 120, (9, 6, 4), 0.9, 0.03, 7)
    if key == "short_10":        # l_req = 12 > m_global = 10
        return planted(10, 120, (9, 6, 4), 0.9, 0.03, 9)
    if key == "long_first_row":  # (d): row 0 holds more than two thirds of all entries
        D = planted(12, 240, (7, 4), 0.9, 0.01, 15, gr=[2] + [0] * 5 + [1] * 6, gc=[0] * 8 + [1] * 8 + [2] * 224).toarray()
        D[0, :] = 1.0
        return _csr(D)
    if key == "seven_rows":      # (d): m == nd == 7, and row 6 holds nothing
        D = planted(7, 120, (6, 5), 0.85, 0.05, 19, gr=[0, 0, 0, 1, 1, 2, 2], gc=[0] * 30 + [1] * 20 + [2] * 70).toarray()
        D[6, :] = 0.0
        return _csr(D)
    if key == "wide_panel":      # (i): n_used 2300, and about 1380 under the mask
        return planted(1200, 2300, (12, 11, 10, 9, 8, 7), 0.4, 0.01, 11)
    if key == "lanczos":         # (j): 900 x 400, tall; three shards of about 300 rows are wide
        return planted(900, 400, (12, 11, 10, 9, 8, 7), 0.5, 0.03, 13)
    if key == "lanczos_mask":    # ... and so are they over the 0.6 of 640 columns a mask keeps
        return planted(900, 640, (12, 11, 10, 9, 8, 7), 0.5, 0.03, 13)
    raise KeyError(key)


@functools.lru_cache(maxsize=None)
def mask_of(n, seed):
    return synth.bernoulli_mask(n, 0.6, seed).numpy()


@functools.lru_cache(maxsize=None)
def omega_of(n_used, l, seed):
    return synth.gaussian_panel(n_used, l, seed).numpy()


# ------------------------------------------------------------------------------------------ cases
@dataclass(frozen=True)
class Case:
    name: str
    edge: str                       # the letter of the edge it is listed for
    mat: str
    nd: int
    k: int
    p: int = 6
    q: int = 2
    center: bool = True
    normalizer: str = "QR"
    mask_seed: Optional[int] = None
    scale: Optional[str] = None
    method: str = "RANDOM"
    lanczos_center: bool = False
    dtypes: Tuple[str, ...] = ("float64", "float32")
    natural_order: bool = False     # (i): spmm_variant(2), rows in natural order
    why: str = ""

    @property
    def A(self):
        return matrix(self.mat)

    @property
    def mask(self):
        return None if self.mask_seed is None else mask_of(self.A.shape[1], self.mask_seed)

    @property
    def n_used(self):
        return self.A.shape[1] if self.mask is None else int(self.mask.sum())

    @property
    def l_req(self):
        return self.k + self.p

    @property
    def l(self):
        return min(self.l_req, self.A.shape[0], self.n_used)

    @property
    def omega(self):
        return omega_of(self.n_used, self.l_req, 5)

    @property
    def bounds(self):
        return partition(self.A.indptr, self.nd)


def _cases():
    out = []
    for nd in (2, 3, 4, 7):
        out.append(Case(f"a_balanced_nd{nd}", "a", "balanced", nd, 6, why="balanced shards; 7 members: an uneven last slice in sum_slice"))
    for nd in (3, 4):
        out.append(Case(f"b_empty_shard_nd{nd}", "b", "empty_shard", nd, 4, p=8, why="the last shard has 1439 rows and no entry"))
    out.append(Case("c_rows_below_l_30", "c", "short_30", 3, 4, p=8, why="10 rows per shard against l = 12"))
    out.append(Case("c_rows_below_l_16", "c", "short_16", 4, 3, p=9, why="4 rows per shard against l = 12"))
    # (uncentred: the centred operator of 10 rows has rank 9 < l = 10, and no Cholesky factor of its Gram exists to restate)
    out.append(Case("c_l_cut_to_m_global", "c", "short_10", 3, 3, p=9, center=False, why="l_req = 12 > m_global = 10: l is cut to 10"))
    out.append(Case("d_long_first_row", "d", "long_first_row", 3, 2, p=4, why="nnz bounds [0, 0, 1, m]: even row counts"))
    out.append(Case("d_m_equals_nd", "d", "seven_rows", 7, 2, p=2, why="one row per member; member 6 has a row and no entry"))
    out.append(Case("e_uncentred", "e", "balanced", 3, 6, center=False, why="the A^T all-reduce without the 1^T Y row"))
    out.append(Case("f_lu", "f", "balanced", 3, 6, normalizer="LU", why="PIN.LU"))
    out.append(Case("f_none", "f", "balanced", 3, 6, normalizer="NONE", why="PIN.NONE"))
    out.append(Case("g_mask", "g", "balanced", 3, 6, mask_seed=7, why="bernoulli_mask, keep 0.6"))
    out.append(Case("h_unit_variance", "h", "balanced", 3, 6, scale="unit_variance", why="unit variance, TRANSFORM_CENTERED"))
    for p, tag in ((6, "l12"), (64, "l70")):
        for nd in (2, 3):
            for ms in (None, 7):
                for center in (True, False):
                    out.append(Case(f"i_{tag}_nd{nd}_{'mask' if ms else 'all'}_{'centred' if center else 'raw'}", "i", "wide_panel", nd, 6,
                                    p=p, mask_seed=ms, center=center, dtypes=("float32",), natural_order=True,
                                    why="A^T sweep in two pieces" if p == 6 else "panel ld 128: one piece"))
    for dt in ("float64", "float32"):
        for ms in (None, 7):
            out.append(Case(f"j_lanczos_{dt}_{'mask' if ms else 'all'}", "j", "lanczos_mask" if ms else "lanczos", 3, 6, mask_seed=ms, method="LANCZOS",
                            dtypes=(dt,), why="tall overall, wide shards"))
    out.append(Case("j_lanczos_centred_all", "j", "lanczos", 3, 6, method="LANCZOS", lanczos_center=True, dtypes=("float64",),
                    why="lanczos_center"))
    out.append(Case("j_lanczos_centred_mask", "j", "lanczos_mask", 3, 6, mask_seed=7, method="LANCZOS", lanczos_center=True,
                    dtypes=("float64", "float32"), why="lanczos_center, masked"))
    return tuple(out)


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
RANDOMIZED = tuple(c for c in CASES if c.method == "RANDOM")
PLAIN = tuple(c for c in RANDOMIZED if not c.natural_order)       # every randomized case but the two-piece ones
TWO_PIECE = tuple(c for c in RANDOMIZED if c.natural_order)
LANCZOS = tuple(c for c in CASES if c.method == "LANCZOS")


# ------------------------------------------------------------------------------------------ the reference
def unit_variance_factors(s1, s2, m):
    """d of SAPCA_SCALE_UNIT_VARIANCE from the summed statistics (column_scaling_ref.unit_variance_factors)"""
    ss = s2 - s1 * s1 / m
    dead = ss <= 4.0 * m * EPS64 * s2
    d = np.zeros_like(s1)
    d[~dead] = 1.0 / np.sqrt(ss[~dead] / (m - 1))
    return d


@dataclass
class Fit:
    singular_values: np.ndarray
    components: np.ndarray
    mean: np.ndarray
    total_var: float
    scores: Optional[np.ndarray]    # the reference's transform semantics (Q2, masked: Q3); None for a scaled fit
    scores_centered: np.ndarray     # (A - 1 mu^T) [D] V^T
    scale: Optional[np.ndarray]     # d over the columns the fit used


def sharded_randomized_fit(A, bounds, k, p, q, omega, center, normalizer, mask=None, scale=None):
    A = sp.csr_matrix(A, dtype=np.float64)
    n = A.shape[1]
    shards = [A[int(a):int(b)] for a, b in zip(bounds[:-1], bounds[1:])]
    add = lambda parts: functools.reduce(np.add, parts)            # a summation site: rank order

    # site 1: column sums, sums of squares, stored entries per column and the row count
    s1 = add([np.asarray(S.sum(0)).ravel() for S in shards])
    s2 = add([np.asarray(S.multiply(S).sum(0)).ravel() for S in shards])
    cnt = add([np.bincount(S.indices, minlength=n).astype(np.float64) for S in shards])
    m = int(add([S.shape[0] for S in shards]))
    cols = np.arange(n) if mask is None else np.flatnonzero(np.asarray(mask, dtype=bool))
    mean = s1 / m if center else np.zeros(n)
    var = (s2 - (s1 / m) * s1) / (m - 1)
    d = None
    if isinstance(scale, str):
        assert scale == "unit_variance"
        d = unit_variance_factors(s1, s2, m)[cols]
    elif scale is not None:
        d = np.asarray(scale, dtype=np.float64)[cols]
    ops = [S[:, cols] for S in shards]
    mu = mean[cols] if center else None
    l = min(k + p, m, cols.size)
    X = np.array(omega[:, :l], dtype=np.float64)

    def sweep_a(X):                                     # local rows only
        Xs = X if d is None else d[:, None] * X
        return [S @ Xs - ((mu @ Xs)[None, :] if center else 0.0) for S in ops]

    def sweep_at(Ys):                                   # site 3: the panel and 1^T Y in one sum
        Z = add([S.T @ Y for S, Y in zip(ops, Ys)])
        if center:
            Z = Z - np.outer(mu, add([Y.sum(0) for Y in Ys]))
        return Z if d is None else d[:, None] * Z

    def orthonormal_rows(Ys, passes):                   # site 2: CholeskyQR on the summed Gram
        for _ in range(passes):
            R = np.linalg.cholesky(add([Y.T @ Y for Y in Ys])).T
            Ys = [sl.solve_triangular(R, Y.T, trans="T", lower=False).T for Y in Ys]
        return Ys

    passes = {"QR": 2, "LU": 1, "NONE": 0}[normalizer]
    for _ in range(q):
        Ys = orthonormal_rows(sweep_a(X), passes)
        X = O.normalize_panel(sweep_at(Ys), normalizer)
    B = sweep_at(orthonormal_rows(sweep_a(X), 2)).T
    _, s, vt = np.linalg.svd(B, full_matrices=False)
    _, vt = O.svd_flip_v(None, vt[:k])
    s = s[:k]
    if center:
        total_var = float(var[cols].sum() if d is None else (d * d * var[cols]).sum())
    else:
        total_var = float(np.sum(s ** 2 / (m - 1)))

    # the projection, shard by shard
    W = vt.T if d is None else d[:, None] * vt.T
    centred = np.vstack([S @ W - ((mu @ W)[None, :] if center else 0.0) for S in ops])
    scores = None
    if d is None and mask is None:                      # Q2: every column weighted by its stored entries, over all shards (site 4)
        Wc = cnt[:, None] * vt.T
        scores = np.vstack([S @ Wc - ((mu @ Wc)[None, :] if center else 0.0) for S in ops])
    elif d is None:                                     # Q3: the mean leaves stored, kept entries only
        scores = np.vstack([O.transform_masked_fast(S.indptr.astype(np.int64), S.indices.astype(np.int64), S.data, S.shape[0], n, vt, mean,
                                                    center, mask) for S in shards])
    return Fit(s, vt, mean, total_var, scores, centred, d)


def reference_fit(c):
    """sharded_randomized_fit of a case"""
    return sharded_randomized_fit(c.A, c.bounds, c.k, c.p, c.q, c.omega, c.center, c.normalizer, mask=c.mask, scale=c.scale)


def oracle_fit(c):
    """O.fit of the whole matrix with the l columns of Omega the fit uses (a scaled case: of A diag(d), d from dense numpy)"""
    A = c.A
    m, n = A.shape
    data = A.data
    if c.scale is not None:
        D = A.toarray()
        d = unit_variance_factors(D.sum(0), (D * D).sum(0), m)
        data = A.data * d[A.indices]
    return O.fit(A.indptr, A.indices, data, m, n, n_components=c.k, n_oversamples=c.l - c.k, n_power_iterations=c.q,
                 normalizer=c.normalizer, center=c.center, omega=c.omega[:, :c.l], mask=c.mask)


def dense_operator(c):
    """what the SVD of a case factors, dense: centred where the fit centres, over the kept columns, scaled where the case is"""
    D = c.A.toarray()
    centred = c.center and (c.method == "RANDOM" or c.lanczos_center)
    m = D.shape[0]
    d = unit_variance_factors(D.sum(0), (D * D).sum(0), m) if c.scale is not None else None
    if centred:
        D = D - D.mean(axis=0)
    if d is not None:
        D = D * d
    return D if c.mask is None else D[:, c.mask]


def _operator_key(c):
    return (c.mat, c.mask_seed, c.center and (c.method == "RANDOM" or c.lanczos_center), c.scale)


@functools.lru_cache(maxsize=None)
def _exact_svd(key):
    c = next(x for x in CASES if _operator_key(x) == key)
    _, s, vt = np.linalg.svd(dense_operator(c), full_matrices=False)
    return s, vt


def exact_svd(name):
    """(sigma, V^T) of dense_operator, all of them (computed once per operator: cases that differ in members or l share it)"""
    return _exact_svd(_operator_key(BY_NAME[name]))


def gap(c):
    s, _ = exact_svd(c.name)
    return float(s[c.k - 1] / s[c.k])
