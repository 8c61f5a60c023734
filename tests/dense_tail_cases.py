"""Host-only helper of tests/test_gpu_rotation.py and tests/test_gpu_normalize_extras.py: the panels that send the dense tail of
a randomized fit -- the normaliser with its extras (gram.hip, chol.hip, panel_gemm.hip) and the rotation into components
(panel_gemm.hip, panel_ops.hip) -- through each of its kernels and reductions, the geometry of those kernels restated from the
sources, and the exact references.  Needs neither a GPU nor the library: tests/test_dense_tail_cases_cpu.py holds every case to
its conditions on the CPU.

Every panel is built from small integers (|v| <= 8, weights 0..3), so that the sum of the slabs, mu sv^T, the weighted column
sums, the Gram matrix and P @ M for an integer M are exact in f32 and in f64: a dropped slab, row or tile changes bits."""
import functools

import numpy as np

# ---- the geometry, restated (file: the line each mirrors)
TWO_STAGE_MIN_ROWS = 4096    # panel_ops.hip flip_transpose: ld <= 256 && 256 % ld == 0 && n >= 4096
SIGN_THREADS = 256           # panel_ops.hip: both sign kernels run 256 threads
GEMM_WIDE_TILES = 1024       # panel_gemm.hip launch_panel_gemm: NTO == 4 && ntiles >= 1024 -> 512 threads


def pad(l):
    """api.cpp: ld = round_up(l, l > 128 ? 64 : 16)"""
    q = 64 if l > 128 else 16
    return -(-l // q) * q


def ldk_of(k):
    return -(-k // 16) * 16


def two_stage(n, k):
    ldk = ldk_of(k)
    return ldk <= 256 and 256 % ldk == 0 and n >= TWO_STAGE_MIN_ROWS


def sign_geometry(n, k):
    """(rows a block scans, row groups of a block, blocks): panel_ops.hip flip_transpose for the two-stage route; the one-kernel
    route is one block whose thread t scans rows t, t + 256, ..."""
    if not two_stage(n, k):
        return n, SIGN_THREADS, 1
    nblocks = min(256, (n + 63) // 64)
    rpb = -(-n // nblocks)
    return rpb, 256 // ldk_of(k), -(-n // rpb)


# ---- rotation
ROTATION_PAIRS = ((16, 1), (30, 17), (64, 50), (60, 40), (112, 100), (128, 100), (128, 128), (200, 150), (270, 270))
FULL_N = (1, 15, 16, 17, 4095, 4096, 4097, 16368, 16369, 16400)
SHORT_N = (17, 4097)
FULL_N_PAIRS = ((64, 50), (30, 17))


def rotation_shapes():
    return [(l, k, n) for l, k in ROTATION_PAIRS for n in (FULL_N if (l, k) in FULL_N_PAIRS else SHORT_N)]


def _rng(*key):
    return np.random.default_rng([20240, *key])


@functools.lru_cache(maxsize=None)
def integer_rotation(l, k, n):
    """(P, M): an n x l panel with entries in -8..8 and an l x k factor with entries in -3..3 (int64)"""
    rng = _rng(1, l, k, n)
    return rng.integers(-8, 9, (n, l)), rng.integers(-3, 4, (l, k))


def flip_reference(Y):
    """(components, signs) of the n x k product Y by the documented rule: the sign of the entry of largest |.| of every column,
    the first row on ties; a column without one (all nan) keeps +1"""
    A = np.abs(Y)
    A = np.where(np.isnan(A), -1.0, A)
    rows = np.argmax(A, axis=0)                       # (numpy: the first index of the maximum)
    top = Y[rows, np.arange(Y.shape[1])]
    signs = np.where(top < 0, -1.0, 1.0)
    return (Y * signs).T.copy(), signs


def tie_positions(n, k):
    """pairs of rows (r1 < r2) that one column's two equal maxima are put at, named by where the reductions of the sign kernels
    meet them (two-stage route: a block scans rpb rows, row r0 + g + i ng by thread group g; one-kernel route: thread t scans
    rows t + 256 i)"""
    rpb, ng, nblocks = sign_geometry(n, k)
    out = {}
    if two_stage(n, k):
        b = 2 * rpb                                   # block 2
        out["same thread"] = (b + 1, b + 1 + ng)
        out["row groups"] = (b + 2, b + 3)
        out["row groups, later group first"] = (b + ng - 1, b + ng + 1 + ng)   # group ng - 1, then group 1 one trip later
        out["blocks"] = (5, 3 * rpb + 7)
        last0 = (nblocks - 1) * rpb
        if n - last0 >= ng + 2:                       # (a last block of one row: the pairs below that end in row n - 1)
            out["short last block, same thread"] = (last0 + 1, last0 + 1 + ng)
            out["short last block, row groups"] = (last0 + 2, last0 + 3)
    else:
        out["same thread"] = (3, 3 + SIGN_THREADS)
        out["threads"] = (4, 5)
        out["threads, later thread first"] = (200, 256 + 7)   # thread 200, then thread 7 one trip later
        out["halves of the tree"] = (10, 128 + 10)
    out["first and last row"] = (0, n - 1)
    if n > 4096:
        out["rows 4095 and 4096"] = (4095, 4096)
    return {name: (r1, r2) for name, (r1, r2) in out.items() if r1 < r2 < n}


@functools.lru_cache(maxsize=None)
def tie_panels(l, k, n):
    """[(P, M, {column: (name, r1, r2, sign of the entry at r1)})]: integer panels in which every listed column of P @ M has
    exactly two entries of largest magnitude, of opposite signs, at rows r1 < r2 -- every pair of tie_positions in both orders
    of the two signs -- and one column is zero throughout (entry name "zero").  A panel holds pairs with disjoint rows, a
    column each; the other rows stay within -4..4, the paired rows are +-8 sign(M[:, column])."""
    rng = _rng(2, l, k, n)
    todo = [(name, r1, r2, s) for name, (r1, r2) in tie_positions(n, k).items() for s in (1, -1)]
    panels = []
    while todo:
        P, M = rng.integers(-4, 5, (n, l)), rng.integers(-3, 4, (l, k))
        M[M == 0] = 1                                  # (a paired row beats every other row in its column by a factor of two)
        used_rows, marks, rest = set(), {}, []
        free = list(range(k))
        zero_col = free.pop() if k > 1 and not panels else None
        for name, r1, r2, s in todo:
            if not free or r1 in used_rows or r2 in used_rows:
                rest.append((name, r1, r2, s))
                continue
            c = free.pop(0)
            used_rows |= {r1, r2}
            P[r1] = 8 * s * np.sign(M[:, c])
            P[r2] = -P[r1]
            marks[c] = (name, r1, r2, s)
        if zero_col is not None:
            M[:, zero_col] = 0
            marks[zero_col] = ("zero", -1, -1, 1)
        panels.append((P, M, marks))
        todo = rest
    return panels


TIE_SHAPES = ((64, 50, 4097), (64, 50, 16400), (30, 17, 4097), (30, 17, 16400),     # two-stage: ng = 4 / 8, rpb = 64 / 65
              (60, 40, 4097), (64, 50, 4095), (16, 1, 17))                          # one kernel: ldk = 48; n < 4096; one column
NAN_SHAPES = ((64, 50, 17), (64, 50, 4097), (60, 40, 17), (60, 40, 4097))
GAUSSIAN_SHAPE = (64, 50, 4097)


@functools.lru_cache(maxsize=None)
def gaussian_rotation(dtype_name):
    """(P in the dtype, M in f64, Y = P64 @ M, the elementwise product bound |P| @ |M|)"""
    l, k, n = GAUSSIAN_SHAPE
    rng = _rng(3, l, k, n)
    P = rng.standard_normal((n, l)).astype(dtype_name)
    M = rng.standard_normal((l, k))
    P64 = P.astype(np.float64)
    return P, M, P64 @ M, np.abs(P64) @ np.abs(M)


def rotation_error_bound(dtype_name, l, Y, absprod):
    """what a computed entry of P @ M may differ by from numpy's f64 product: f64, 2 l 2^-53 (|P| @ |M|) -- the gamma_l bound of
    a dot product, doubled for the reference's own error; f32, one ulp of the reference rounded to f32"""
    if np.dtype(dtype_name) == np.float64:
        return 2 * l * 2.0 ** -53 * absprod
    return np.spacing(np.abs(Y.astype(np.float32))).astype(np.float64)


# ---- normaliser with extras
NORMALIZE_L = (60, 128, 40, 150)       # fused ld = 64; fused, four waves; plain Gram behind materialize; wide pairs behind materialize
NSPLITS = (1, 2, 3, 4, 5, 6, 9, 12)    # at 200 rows
ROWS = (1, 17, 200, 8200)              # at nsplit 1 and 3


def normalize_shapes():
    return [(l, 200, ns) for l in NORMALIZE_L for ns in NSPLITS] + \
           [(l, rows, ns) for l in NORMALIZE_L for rows in ROWS if rows != 200 for ns in (1, 3)]


@functools.lru_cache(maxsize=None)
def normalize_case(l, rows, nsplit, rank_deficient=False):
    """dict of int64 arrays: slabs (nsplit x rows x l, entries -8..8), mu (rows, -1..1), sv (l, -1..1), w (rows, 0..3), and what
    follows from them exactly: P = sum of the slabs, Pc = P - mu sv^T, the weighted and plain column sums of either, the Grams"""
    rng = _rng(4, l, rows, nsplit, int(rank_deficient))
    slabs = rng.integers(-8, 9, (nsplit, rows, l))
    if rank_deficient:
        slabs[:, :, l - 1] = slabs[:, :, 3]
    mu, sv, w = rng.integers(-1, 2, rows), rng.integers(-1, 2, l), rng.integers(0, 4, rows)
    if rank_deficient:
        sv[l - 1] = sv[3]
    P = slabs.sum(0)
    Pc = P - np.outer(mu, sv)
    return {"slabs": slabs, "mu": mu, "sv": sv, "w": w, "P": P, "Pc": Pc}


def panel_of(case, centred):
    return case["Pc"] if centred else case["P"]


def qr_reference(P, w, dtype_name):
    """What numpy.linalg.qr in f64, rounded once to the dtype, leaves on the panel P (int64) with weights w, in the units of the
    two GPU checks: max |P - Q R| / (l eps (|Q| @ |R|)) and max |v - w^T Q| / (rows eps (|w| @ |Q|)), v = R^-T (P^T w)
    rounded once -- the quantities tests/test_gpu_normalize_extras.py bounds by 8 x these figures."""
    T = np.dtype(dtype_name)
    rows, l = P.shape
    P64 = P.astype(np.float64)
    Q, R = np.linalg.qr(P64)
    Qt = Q.astype(T).astype(np.float64)
    v = np.linalg.solve(R.T, P64.T @ w.astype(np.float64)).astype(T).astype(np.float64)
    return residual_ratio(P64, Qt, R, T), vec_ratio(v, w, Qt, T)


def residual_ratio(P64, Q64, R, T):
    l = P64.shape[1]
    unit = l * np.finfo(T).eps * (np.abs(Q64) @ np.abs(R))
    return float((np.abs(P64 - Q64 @ R) / np.maximum(unit, np.finfo(np.float64).tiny)).max())


def vec_ratio(v64, w, Q64, T):
    rows = Q64.shape[0]
    w64 = np.asarray(w, np.float64)
    unit = rows * np.finfo(T).eps * (np.abs(w64) @ np.abs(Q64))
    return float((np.abs(v64 - w64 @ Q64) / np.maximum(unit, np.finfo(np.float64).tiny)).max())


# 8 x the largest figure qr_reference leaves over normalize_shapes() with rows >= l, both centrings, both weightings: measured
# f64 residual 295.05, vec 0.020156; f32 residual 0.012402, vec 0.00072228.  (The f64 residual figure is numpy's at entries of
# column 0 where the integer panel holds a zero: Householder QR is accurate normwise, not entry by entry, and |Q| @ |R| is
# |P[i][0]| there.)  tests/test_dense_tail_cases_cpu.py::test_margins_are_eight_times_the_reference recomputes them.
MARGIN = {"float64": (2361.0, 0.1613), "float32": (0.09922, 0.005779)}    # dtype: (residual, vec)
