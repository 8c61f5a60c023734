"""Host-only helper of tests/test_gpu_lanczos_products.py: the matrices that send a Lanczos fit through each of its product
kernels (csrc/lanczos.hip) and through the fixed-point scatter route (csrc/scatter.hip), the route each of them takes,
restated from the sources, and their f64 references.  Needs neither a GPU nor the library: tests/test_lanczos_cases_cpu.py holds
every case to its conditions (gap, row lengths, boundary columns, route) on the CPU.

Every matrix is synth.gapped_csr(m, n, density, k=6, seed=17, centred=False) in f64 as a scipy CSR with a few rows
edited (below); f32 cases round those values once, centred cases generate with centred=True (another matrix)."""
import functools
import math

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla
import torch

from sapca import synth

# ---- the route predicates, restated (file: the line each mirrors)
WAVE = 64                        # lanczos.hip: constexpr int WAVE = 64
UNROLL_FROM = 3 * WAVE + 1       # lanczos.hip / scatter.hip: for (; e + 3 * WAVE < e1; e += 4 * WAVE)  -- first trip at 193 entries
LDS_X_BYTES = 150 * 1024         # lanczos.hip spmv_plan: xbytes <= 150 * 1024  (x, or a slice of it, as doubles in LDS)
LDS_X_COLS = LDS_X_BYTES // 8    # = 19200
LDSX_MIN_ROWS = 4096             # lanczos.hip spmv_plan: A.rows >= 4096  (spmv_ldsx_kernel)
LONG_ROW_ENTRIES = 256           # lanczos.hip spmv_plan: A.nnz >= 256 * A.rows  (the sliced kernels)
SLICED_MIN_ROWS = 1024           # lanczos.hip spmv_plan: A.rows >= 1024
SLICE_WAVES, SLICE_MAX_RPW = 16, 8   # lanczos.hip: constexpr int SLICE_WAVES = 16, SLICE_MAX_RPW = 8
SCATTER_MIN_ROWS = 4096          # engine.cpp plan_preparation: n_used <= m && m >= 4096 && nnz > 0 && k::scatter_fits(n_used)
SCATTER_BYTES = 150 * 1024       # scatter.hip scatter_fits: cols * sizeof(long long) <= kScatterLds
STATS_PASS_COLS = SCATTER_BYTES // 20   # scatter.hip colstats_scatter: max_nc = kScatterLds / per_col (two int64 and a uint32) = 7680

K = 6
SEED = 17
# the lengths rows 0..14 are cut (or filled) to: first and last trips of the four-wide loop and every remainder count
ROW_LENGTHS = (0, 1, 63, 64, 65, 192, 193, 255, 256, 257, 320, 448, 449, 512, 513)
FULL_ROW = len(ROW_LENGTHS)      # row 15: every column (W2: an entry either side of every slice boundary)


def scatter_route(m, n_used, nnz, transpose_switch=False):
    """engine.cpp plan_preparation: lz_scatter"""
    return (not transpose_switch) and 0 < n_used <= m and m >= SCATTER_MIN_ROWS and nnz > 0 and n_used * 8 <= SCATTER_BYTES


def slices_of(cols):
    """lanczos.hip spmv_plan: (slice, nslices) of an x with `cols` elements"""
    nslices = -(-cols // LDS_X_COLS)
    return -(-cols // nslices), nslices


def spmv_kind(rows, cols, nnz, has_scratch, no_lds=False, no_grid=False):
    """lanczos.hip spmv_plan + spmv_launch: the kernel a product with a rows x cols operator takes"""
    if rows == 0 or no_lds:
        return "row"
    if cols * 8 <= LDS_X_BYTES and rows >= LDSX_MIN_ROWS:
        return "ldsx"
    if nnz >= LONG_ROW_ENTRIES * rows and rows >= SLICED_MIN_ROWS:
        _, nslices = slices_of(cols)
        if has_scratch and not no_grid and nslices > 1:
            return "slice_grid"
        rpw = max(1, -(-rows // (256 * SLICE_WAVES)))
        if rpw <= SLICE_MAX_RPW and rpw * (nslices + 1) <= WAVE:
            return "sliced"
    return "row"


def sliced_rpw(rows):
    return max(1, -(-rows // (256 * SLICE_WAVES)))


def stats_passes(n):
    """scatter.hip colstats_scatter: (passes, nc_pass) over the n columns of the matrix (masked-out ones included)"""
    passes = -(-n // STATS_PASS_COLS)
    return passes, -(-n // passes)


def products(m, n_used, nnz, transpose_switch=False, no_lds=False, no_grid=False):
    """the kernels of the two products of a Lanczos step, in order (lanczos.hip lanczos_fit, apply_B)"""
    if scatter_route(m, n_used, nnz, transpose_switch):
        return (spmv_kind(m, n_used, nnz, False, no_lds, no_grid), "scatter")
    if n_used <= m:     # right side: A v, then A^T y with the scratch buffer
        return (spmv_kind(m, n_used, nnz, False, no_lds, no_grid), spmv_kind(n_used, m, nnz, True, no_lds, no_grid))
    return (spmv_kind(n_used, m, nnz, False, no_lds, no_grid), spmv_kind(m, n_used, nnz, True, no_lds, no_grid))


# ---- the matrices
def _generate(m, n, density, k=K, centred=False):
    # (on the GPU where there is one: the generator is a pure function of (seed, row, column), bit-identical on either device)
    device = "cuda" if torch.cuda.is_available() else "cpu"
    ptr, idx, val = (t.cpu() for t in synth.gapped_csr(m, n, density, k, seed=SEED, centred=centred, dtype=torch.float64, device=device))
    return sp.csr_matrix((val.numpy(), idx.numpy().astype(np.int64), ptr.numpy()), shape=(m, n))


def _replace_rows(A, new):
    """A with the rows of `new` (row -> (ascending columns, values)) in place of its own"""
    m, n = A.shape
    cols, vals, counts = [], [], np.diff(A.indptr)
    for r in range(m):
        if r in new:
            c, v = new[r]
            counts[r] = len(c)
        else:
            c, v = A.indices[A.indptr[r]:A.indptr[r + 1]], A.data[A.indptr[r]:A.indptr[r + 1]]
        cols.append(np.asarray(c, np.int64))
        vals.append(np.asarray(v, np.float64))
    ptr = np.zeros(m + 1, np.int64)
    ptr[1:] = np.cumsum(counts)
    out = sp.csr_matrix((np.concatenate(vals), np.concatenate(cols), ptr), shape=(m, n))
    assert out.has_sorted_indices or not out.sort_indices()
    return out


def _row(A, r):
    return A.indices[A.indptr[r]:A.indptr[r + 1]].copy(), A.data[A.indptr[r]:A.indptr[r + 1]].copy()


def _resized(cols, vals, length, n, rng):
    """the row with exactly `length` entries: a random subset of its own, or its own and random new columns (U(0, 1) + 2^-20,
    the generator's background values)"""
    if length <= len(cols):
        keep = np.sort(rng.choice(len(cols), length, replace=False))
        return cols[keep], vals[keep]
    free = np.setdiff1d(np.arange(n), cols)
    add = rng.choice(free, length - len(cols), replace=False)
    c = np.concatenate([cols, add])
    v = np.concatenate([vals, rng.uniform(0.0, 1.0, len(add)) + 2.0 ** -20])
    o = np.argsort(c)
    return c[o], v[o]


def _with(cols, vals, extra, rng):
    add = np.setdiff1d(np.asarray(extra, np.int64), cols)
    c = np.concatenate([cols, add])
    v = np.concatenate([vals, rng.uniform(0.5, 1.0, len(add))])
    o = np.argsort(c)
    return c[o], v[o]


def empty_row(m):
    return m // 2


def _edge_rows(A, slice_boundaries=None):
    """rows 0..14 at ROW_LENGTHS, row 15 with every column (slice_boundaries: with an entry either side of each instead),
    row m // 2 empty; the last row stays as generated (non-empty)"""
    m, n = A.shape
    rng = np.random.default_rng(1000 + m + n)
    new = {r: _resized(*_row(A, r), length, n, rng) for r, length in enumerate(ROW_LENGTHS)}
    if slice_boundaries is None:
        new[FULL_ROW] = (np.arange(n), rng.uniform(0.0, 1.0, n) + 2.0 ** -20)
    else:
        new[FULL_ROW] = _with(*_row(A, FULL_ROW), [0, n - 1] + [c for b in slice_boundaries for c in (b - 1, b)], rng)
    new[empty_row(m)] = (np.zeros(0, np.int64), np.zeros(0))
    return _replace_rows(A, new)


def slice_boundaries(cols):
    s, t = slices_of(cols)
    return [i * s for i in range(1, t)]


EMPTY_COLUMN = 1234    # P2, P3m and the LDS-limit matrix


def _pass_edges(A):
    """entries in the columns either side of every statistics pass boundary p * nc_pass (row 5: both sides, row 6: the right-hand
    columns only -- the run of pass p starts exactly at its first entry -- row 7: the left-hand ones only), an entry in column
    n - 1 of the last row, column EMPTY_COLUMN without entries, row m // 2 empty"""
    m, n = A.shape
    rng = np.random.default_rng(2000 + m + n)
    passes, nc = stats_passes(n)
    edges = [p * nc for p in range(1, passes)]
    new = {5: _with(*_row(A, 5), [c for b in edges for c in (b - 1, b)], rng),
           6: _with(*_row(A, 6), edges, rng),
           7: _with(*_row(A, 7), [b - 1 for b in edges], rng),
           m - 1: _with(*_row(A, m - 1), [n - 1], rng),
           empty_row(m): (np.zeros(0, np.int64), np.zeros(0))}
    for r in (6, 7):      # (only the named side)
        c, v = new[r]
        drop = np.isin(c, [b - 1 for b in edges] if r == 6 else edges)
        new[r] = (c[~drop], v[~drop])
    out = _replace_rows(A, new).tocsc()
    out.data[out.indptr[EMPTY_COLUMN]:out.indptr[EMPTY_COLUMN + 1]] = 0.0
    out.eliminate_zeros()
    out = out.tocsr()
    out.sort_indices()
    return out


# name: (m, n, density); W3's density is the issue's 0.007 raised until the gap reaches 1.5 (0.007 gives 1.49)
SHAPES = {"L": (4200, 1500, 0.2), "S": (3000, 1200, 0.22), "W2": (4200, 20000, 0.0135), "W3": (4200, 40000, 0.0075),
          "T": (20000, 5000, 0.06), "P2": (8192, 7700, 0.02), "P3m": (4200, 16000, 0.03),
          "LIM": (19264, 19200, 0.014)}
K_OF = {"LIM": 2}
EDGE_ROW_CASES = ("L", "S", "T", "W2")


def k_of(name):
    return K_OF.get(name, K)


@functools.lru_cache(maxsize=None)
def matrix(name, centred=False, f32=False):
    """the case's matrix as a scipy CSR of f64 values (f32: values that an f32 holds exactly)"""
    if name == "LIM+1":      # the LDS-limit matrix with a 19201st column: one entry of 2^-20 in the last row
        A = matrix("LIM", centred, f32)
        m, n = A.shape
        extra = sp.csr_matrix((np.array([2.0 ** -20]), (np.array([m - 1]), np.array([n]))), shape=(m, n + 1))
        out = (sp.hstack([A, sp.csr_matrix((m, 1))]).tocsr() + extra).tocsr()
        out.sort_indices()
        return out
    if name == "Lsmall":     # L with columns 0..9 scaled by 1e-9 and one entry of 1e3: what the fixed-point resolution promises
        A = matrix("L", centred, f32).copy()
        A.data[A.indices < 10] *= 1e-9
        e = A.indptr[100] + 40
        assert A.indices[e] >= 10
        A.data[e] = 1e3
        return A
    if f32:
        A = matrix(name, centred, False).copy()
        A.data = A.data.astype(np.float32).astype(np.float64)
        return A
    m, n, density = SHAPES[name]
    A = _generate(m, n, density, k_of(name), centred)
    if name in EDGE_ROW_CASES:
        A = _edge_rows(A, slice_boundaries(n) if name == "W2" else None)
    elif name == "W3":
        A = _replace_rows(A, {FULL_ROW: _with(*_row(A, FULL_ROW), [0, n - 1] + [c for b in slice_boundaries(n) for c in (b - 1, b)],
                                               np.random.default_rng(3)),
                              empty_row(m): (np.zeros(0, np.int64), np.zeros(0))})
    else:
        A = _pass_edges(A)
    return A


def mask_of(name):
    return synth.bernoulli_mask(SHAPES[name][1], 0.25, 5).numpy() if name == "P3m" else None


def used(name, centred=False, f32=False):
    """the operator the fit sees: the kept columns"""
    A, mask = matrix(name, centred, f32), mask_of(name)
    return A if mask is None else A[:, np.flatnonzero(mask)].tocsr()


# ---- references (f64, host)
def gram_svd(A, k):
    """(sigma[:k + 1], Vt[:k]) from numpy.linalg.eigh of the Gram matrix of the smaller side, formed from the CSR"""
    m, n = A.shape
    tall = n <= m
    G = ((A.T @ A) if tall else (A @ A.T)).toarray()
    w, Q = np.linalg.eigh(G)
    w, Q = w[::-1], Q[:, ::-1]
    s = np.sqrt(np.maximum(w[:k + 1], 0.0))
    if tall:
        return s, Q[:, :k].T.copy()
    return s, ((A.T @ Q[:, :k]) / s[:k]).T.copy()


def svds_svd(A, k):
    """(sigma[:k + 1], Vt[:k]) from scipy.sparse.linalg.svds(k + 1, tol=0) (held to gram_svd on case S by the CPU test)"""
    _, s, vt = spla.svds(A, k=k + 1, tol=0, random_state=0)
    o = np.argsort(-s)
    return s[o], vt[o][:k]


def centred_svd(A, k, vectors=True):
    """(sigma[:k + 1], Vt[:k]) of D - D.mean(0) by numpy.linalg.svd, as tests/test_gpu_lanczos_centred.py has it"""
    D = A.toarray()
    if not vectors:
        return np.linalg.svd(D - D.mean(0), compute_uv=False)[:k + 1], None
    _, s, vt = np.linalg.svd(D - D.mean(0), full_matrices=False)
    return s[:k + 1], vt[:k]


SVDS_CASES = ("P2", "LIM", "LIM+1")     # (a 7700^2 or 19200^2 eigh takes too long)


@functools.lru_cache(maxsize=None)
def reference(name, centred=False, f32=False, vectors=True):
    """(sigma[:k + 1], Vt[:k], gap sigma_k / sigma_k+1) of the operator the fit sees (vectors=False: a centred case's sigma alone,
    a third of the time)"""
    base = "LIM" if name == "LIM+1" else name
    A, k = used(name, centred, f32), k_of(base)
    s, vt = centred_svd(A, k, vectors) if centred else svds_svd(A, k) if name in SVDS_CASES else gram_svd(A, k)
    return s, vt, float(s[k - 1] / s[k])


# ---- exact column sums
def _two_square(v):
    """v * v as three doubles whose exact sum it is (Veltkamp split: each half has at most 26 bits, each product is exact)"""
    t = v * 134217729.0
    hi = t - (t - v)
    lo = v - hi
    return hi * hi, 2.0 * hi * lo, lo * lo


def exact_column_sums(A):
    """per column of the CSR A: the correctly rounded sum and sum of squares of the stored values, the stored-entry count, and
    sum |a| (math.fsum per column; equal to tests/exact_sums_ref.py, which the CPU test checks on case S, without its Fractions)"""
    C = A.tocsc()
    n = C.shape[1]
    p0, p1, p2 = _two_square(C.data)
    s, sq, sabs = np.zeros(n), np.zeros(n), np.zeros(n)
    for j in range(n):
        lo, hi = C.indptr[j], C.indptr[j + 1]
        if hi > lo:
            s[j] = math.fsum(C.data[lo:hi])
            sabs[j] = math.fsum(np.abs(C.data[lo:hi]))
            sq[j] = math.fsum(np.concatenate([p0[lo:hi], p1[lo:hi], p2[lo:hi]]))
    return s, sq, np.diff(C.indptr).astype(np.int64), sabs
