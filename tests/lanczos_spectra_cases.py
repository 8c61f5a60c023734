"""Host-only helper of tests/test_gpu_lanczos_spectra.py and tests/test_gpu_spectral_degenerate.py: matrices and graphs whose
spectra are hard for a single-vector Lanczos run (repeated, clustered, flat, rank-deficient, empty), and a numpy restatement of
the driver loop of lanczos_fit (csrc/lanczos.hip); the spectral driver's loop is restated in tests/spectral_ref.py.  The
restatements choose the fixtures and predict the branch each takes (tests/test_lanczos_spectra_cases_cpu.py holds every fixture
to what it is for); the GPU tests compare the library with numpy's svd and eigh of the dense f64 matrix, never with them.
Start vectors are numpy's, not the library's: step counts are predicted as a class (the check interval they end in)."""
import functools

import numpy as np
import scipy.sparse as sp

import spectral_ref as SR

KAPPA = 10e-6        # lanczos.hip: const double kappa = 10e-6
RANK_FLOOR = 1e-12   # lanczos.hip: rank_floor = 1e-12 theta_max (sigma <= 1e-6 sigma_1 is a zero)
TOL = 1e-8           # sapca_spectral_options_default: tol


# ------------------------------------------------------------------ the PCA driver, restated
def pca_jmax(m, n, k, masked=False):
    """lanczos.hip lanczos_fit: the iteration cap (the 12 GB cap on the basis does not bind at these sizes)"""
    length = n if n <= m else m
    ref_iters = max(2 * max(m, n), 100) if masked else max(m, n)
    return min(length, ref_iters, 20 * k + 600)


def step_class(steps):
    """the check interval a run ends in: 1 (every step, <= 64), 2 (<= 128), 4 (<= 256), 8"""
    return 1 if steps <= 64 else 2 if steps <= 128 else 4 if steps <= 256 else 8


def pca_lanczos(A, k, seed=42, every_step=False, masked=False):
    """lanczos_fit on the scipy matrix A (m x n) in f64: the side choice, jmax, CGS2, alpha = h1[j] + h2[j], the check schedule,
    the acceptance rule (theta > 1e-12 theta_max and |beta_j s_ji| <= kappa theta for the k largest) and the exhaustion rule
    (beta_j <= 1e-13 theta_max: "ok" with k values above the floor, else "rank").  dict: status ("ok" | "rank" | "not
    converged" | "jmax < k"), steps, right_side, rank (on exhaustion), sigma (k), Vt (k x n: the components before the sign
    flip; the wide side recovers v_i = A^T u_i / sigma_i)"""
    A = sp.csr_matrix(A, dtype=np.float64)
    m, n = A.shape
    right = n <= m
    B = A.T @ A if right else A @ A.T
    length = n if right else m
    jmax = pca_jmax(m, n, k, masked)
    out = dict(status="jmax < k", steps=0, right_side=right)
    if jmax < k:
        return out
    V = np.zeros((length, jmax + 1))
    w = np.random.default_rng(seed).normal(size=length)
    V[:, 0] = w / np.linalg.norm(w)
    alpha, beta = np.zeros(jmax), np.zeros(jmax)
    out["status"] = "not converged"
    for j in range(jmax):
        w = B @ V[:, j]
        h1 = V[:, :j + 1].T @ w
        w = w - V[:, :j + 1] @ h1
        h2 = V[:, :j + 1].T @ w
        w = w - V[:, :j + 1] @ h2
        alpha[j] = h1[j] + h2[j]
        beta[j] = np.linalg.norm(w)
        V[:, j + 1] = w / beta[j] if beta[j] > 0 else 0.0
        steps = out["steps"] = j + 1
        if not (steps >= k and (every_step or SR.check_due(steps) or steps == jmax)):
            continue
        T = np.diag(alpha[:steps]) + np.diag(beta[:steps - 1], 1) + np.diag(beta[:steps - 1], -1)
        theta, Z = np.linalg.eigh(T)
        top = slice(steps - k, steps)
        floor = RANK_FLOOR * abs(theta[-1])
        ok = np.isfinite(beta[j]) and np.all(theta[top] > floor) and np.all(np.abs(beta[j] * Z[-1, top]) <= KAPPA * np.abs(theta[top]))
        if ok:
            out["status"] = "ok"
            break
        if beta[j] <= 1e-13 * abs(theta[-1]):
            out["rank"] = int(np.sum(theta > floor))
            out["status"] = "ok" if out["rank"] >= k else "rank"
            break
    if out["status"] != "ok":
        return out
    steps = out["steps"]
    T = np.diag(alpha[:steps]) + np.diag(beta[:steps - 1], 1) + np.diag(beta[:steps - 1], -1)
    theta, Z = np.linalg.eigh(T)
    theta, Z = theta[::-1][:k], Z[:, ::-1][:, :k]
    sigma = np.sqrt(np.maximum(theta, 0.0))
    Y = V[:, :steps] @ Z
    if not right:
        Y = (A.T @ Y) / sigma[None, :]
    out["sigma"], out["Vt"] = sigma, Y.T
    return out


# ------------------------------------------------------------------ PCA fixtures (scipy CSR, f64; every value float32-exact)
def _f32_exact(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def p_flat(transposed=False):
    """sparse Gaussian 900 x 700 at density 0.05: no gap anywhere, so k pairs take many steps (the 2-, 4- and 8-step check
    intervals are reached)"""
    rng = np.random.default_rng(101)
    A = sp.random(900, 700, density=0.05, format="csr", random_state=rng, data_rvs=lambda s: _f32_exact(rng.normal(size=s)))
    A.sort_indices()
    return sp.csr_matrix(A.T) if transposed else A


P_FLAT_KS = (8, 30, 60, 100)     # the last one is the k "chosen on the CPU" whose step count exceeds 256
# the restatement's step counts (tall and transposed iterate on the same 700 x 700 Gram matrix): the 2-, 4-, 4- and 8-step intervals
P_FLAT_STEPS = {8: 94, 30: 184, 60: 252, 100: 344}


@functools.lru_cache(maxsize=None)
def p_all(wide=False):
    """30 x 12 (12 x 30) dense Gaussian: k = 11 and k = 12 = len need (nearly) the whole space"""
    A = _f32_exact(np.random.default_rng(102).normal(size=(30, 12)))
    return sp.csr_matrix(A.T if wide else A)


P_TINY_SHAPES = ((1, 1), (1, 5), (5, 1), (2, 2), (3, 2))


def p_tiny(shape):
    return sp.csr_matrix(_f32_exact(np.random.default_rng(103).normal(size=shape)))


P_RANK = 5


@functools.lru_cache(maxsize=None)
def p_rank(wide=False):
    """L R with integer factors in [-3, 3], 200 x 40 (40 x 200) of exact rank 5: every product and sum of the factors is an
    integer far below 2^24, so the matrix is exact in both dtypes"""
    rng = np.random.default_rng(104)
    L = rng.integers(-3, 4, size=(200, P_RANK)).astype(np.float64)
    R = rng.integers(-3, 4, size=(P_RANK, 40)).astype(np.float64)
    A = L @ R
    return sp.csr_matrix(A.T if wide else A)


def p_zero(stored):
    """60 x 20 with no entries (stored=False), or with 3 stored zeros a row (stored=True)"""
    if not stored:
        return sp.csr_matrix((60, 20))
    ptr = np.arange(0, 3 * 60 + 1, 3)
    idx = (np.arange(3 * 60) * 7) % 20
    A = sp.csr_matrix((np.zeros(3 * 60), np.sort(idx.reshape(60, 3), axis=1).ravel(), ptr), shape=(60, 20))
    return A


P_CAP_N = 5000


@functools.lru_cache(maxsize=None)
def p_cap(n=P_CAP_N):
    """n x n with 1 on the diagonal and the superdiagonal: A^T A is tridiag(1, 2, 1) (its first entry 1), whose largest
    eigenvalues crowd below 4 with gaps of pi^2 / n^2: k = 1 does not converge to kappa within the 20 k + 600 = 620 steps"""
    return sp.csr_matrix(sp.diags([np.ones(n), np.ones(n - 1)], [0, 1], format="csr"))


@functools.lru_cache(maxsize=None)
def p_mult(scale2=1.0):
    """blockdiag(M, scale2 M) with M 300 x 120 at density 0.1: every singular value twice (scale2 = 1), or twice within a
    relative 1e-7 (P-cluster: scale2 = 1 + 1e-7, a gap below kappa; f64 only, float32 cannot hold it)"""
    rng = np.random.default_rng(105)
    M = sp.random(300, 120, density=0.1, format="csr", random_state=rng, data_rvs=lambda s: _f32_exact(rng.normal(size=s)))
    A = sp.block_diag([M, M * scale2], format="csr")
    A.sort_indices()
    return A


P_MULT_KS = (2, 4, 6)


# ------------------------------------------------------------------ graphs (symmetric scipy CSR, unit weights unless said)
def _sym(rows, cols, m, w=None):
    w = np.ones(len(rows)) if w is None else w
    U = sp.csr_matrix((w, (rows, cols)), shape=(m, m))
    G = sp.csr_matrix(U + U.T)
    G.sort_indices()
    return G


def ring(n, neighbours=2, w=None):
    """vertex i joined to i +- 1 .. i +- neighbours / 2 (mod n)"""
    i = np.arange(n)
    rows = np.concatenate([i] * (neighbours // 2))
    cols = np.concatenate([(i + d) % n for d in range(1, neighbours // 2 + 1)])
    return _sym(rows, cols, n, w)


def grid(a, b):
    """a x b lattice, 4 neighbours"""
    v = np.arange(a * b).reshape(a, b)
    rows = np.concatenate([v[:, :-1].ravel(), v[:-1, :].ravel()])
    cols = np.concatenate([v[:, 1:].ravel(), v[1:, :].ravel()])
    return _sym(rows, cols, a * b)


def complete(n):
    G = sp.csr_matrix(np.ones((n, n)) - np.eye(n))
    G.sort_indices()
    return G


def star(leaves):
    return _sym(np.zeros(leaves, dtype=np.int64), np.arange(1, leaves + 1), leaves + 1)


def two_rings(n):
    G = sp.block_diag([ring(n), ring(n)], format="csr")
    G.sort_indices()
    return sp.csr_matrix(G)


def perturbed_ring(n, rel, float32):
    """the n-ring with edge weights 1 + rel u, u uniform in (-1, 1); rounded to float32 where it can hold them"""
    w = 1.0 + rel * (2.0 * np.random.default_rng(106).random(n) - 1.0)
    return ring(n, 2, _f32_exact(w) if float32 else w)


GRAPHS = {
    "ring64": lambda: ring(64),
    "ring1000x6": lambda: ring(1000, 6),
    "grid12": lambda: grid(12, 12),
    "grid30": lambda: grid(30, 30),
    "k16": lambda: complete(16),
    "star200": lambda: star(200),
    "two_rings64": lambda: two_rings(64),
    "ring64_1e-6": lambda: perturbed_ring(64, 1e-6, True),
    "ring64_1e-10": lambda: perturbed_ring(64, 1e-10, False),
}
# the graphs whose leading eigenvalues are exactly repeated: a single run returns too few copies of them
DEGENERATE = ("ring64", "ring1000x6", "grid12", "grid30", "k16", "star200", "two_rings64")


@functools.lru_cache(maxsize=None)
def graph(name):
    return GRAPHS[name]()


@functools.lru_cache(maxsize=None)
def graph_spectrum(name, kind, dtype="float64"):
    """dict for the graph with its weights rounded to `dtype`: S (dense f64), U (the locked vectors), n_components, and the
    exact pairs of S in the complement of U by eigh: w (descending) and Q (columns, in the full space)"""
    G = graph(name)
    data = G.data.astype(dtype).astype(np.float64)
    W = SR.dense(G.indptr, G.indices, data)
    labels, ncomp = SR.components(G.indptr, G.indices)
    S, s = SR.operator(W, kind)
    U = SR.locked_vectors(SR.analytic(W, kind, s), labels, ncomp)
    m = W.shape[0]
    C = np.linalg.qr(U, mode="complete")[0][:, U.shape[1]:] if U.shape[1] else np.eye(m)
    T = C.T @ S @ C
    w, Z = np.linalg.eigh((T + T.T) / 2)
    return dict(S=S, U=U, n_components=ncomp, w=w[::-1].copy(), Q=C @ Z[:, ::-1])


def clusters(w, width=10 * TOL):
    """[(first, last + 1)] of the runs of the descending values w in which neighbours are within `width`"""
    out, a = [], 0
    for i in range(1, len(w) + 1):
        if i == len(w) or w[i - 1] - w[i] > width:
            out.append((a, i))
            a = i
    return out
