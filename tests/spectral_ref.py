"""A numpy restatement of the spectral section of include/sapca.h: the components of a graph's structure, the two scales,
the dense S = diag(s) W diag(s), the locked pairs, the eigenpairs of the deflated matrix by numpy's eigh, the sign rule and
UMAP's spectral start; and the Lanczos run and rounds of stage 5 (lanczos_run, lanczos_rounds), held to eigh on graphs with
repeated eigenvalues.  Dense and slow on purpose: test_spectral_cpu.py holds it to scipy and scikit-learn, the GPU tests hold
the library to it (to eigenpairs(), never to the restated iteration)."""
import numpy as np

NORMALIZED, DIFFMAP = "normalized", "diffmap"


def dense(indptr, indices, data, m=None):
    """the CSR as a dense f64 matrix; a column outside [0, m) is skipped, as the kernels skip it"""
    m = len(indptr) - 1 if m is None else m
    W = np.zeros((m, m), dtype=np.float64)
    for i in range(m):
        for e in range(indptr[i], indptr[i + 1]):
            j = int(indices[e])
            if 0 <= j < m:
                W[i, j] += float(data[e])
    return W


def components(indptr, indices):
    """labels (int32) and their count: every stored entry an edge, the components numbered in ascending order of their smallest
    vertex (the fixed point of hooking onto the smaller root is that vertex)"""
    m = len(indptr) - 1
    parent = np.arange(m)

    def root(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for i in range(m):
        for e in range(indptr[i], indptr[i + 1]):
            j = int(indices[e])
            if 0 <= j < m:
                a, b = root(i), root(j)
                if a != b:
                    parent[max(a, b)] = min(a, b)
    roots = np.array([root(i) for i in range(m)], dtype=np.int64)
    is_root = roots == np.arange(m)
    number = np.cumsum(is_root) - 1
    return number[roots].astype(np.int32), int(is_root.sum())


def _positive(x):
    return np.isfinite(x) & (x > 0)


def scale(W, kind):
    """s (m f64) of the kind; 0 where a sum is not finite and positive"""
    q = W.sum(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        if kind == NORMALIZED:
            s = np.where(_positive(q), 1.0 / np.sqrt(q), 0.0)
        elif kind == DIFFMAP:
            t = np.divide(W, np.broadcast_to(q[None, :], W.shape), out=np.zeros_like(W), where=W != 0).sum(axis=1)   # (stored entries only)
            t = np.where(np.isfinite(t), t, 0.0)
            z = t / q
            ok = _positive(q) & _positive(t) & _positive(z)
            s = np.where(ok, 1.0 / (q * np.sqrt(z)), 0.0)
        else:
            raise ValueError(kind)
    return np.where(_positive(s), s, 0.0)


def operator(W, kind):
    """(S, s): S_ij = W_ij (s_i s_j)"""
    s = scale(W, kind)
    return W * (s[:, None] * s[None, :]), s


def analytic(W, kind, s):
    """t (m f64): the eigenvector of eigenvalue 1 of S on every component, before it is cut to a component and normalised:
    1 / s = sqrt(d) for NORMALIZED, 1 / (s q) = sqrt(z) for DIFFMAP; 0 where s is 0"""
    with np.errstate(divide="ignore", invalid="ignore"):
        if kind == NORMALIZED:
            t = 1.0 / s
        else:
            t = 1.0 / (s * W.sum(axis=1))
    return np.where(s > 0, t, 0.0)


def locked_vectors(t, labels, n_components):
    """U (m x c): one unit column t 1_C / |t 1_C| per component with a vertex of t > 0, in label order"""
    cols = []
    for c in range(n_components):
        v = np.where(labels == c, t, 0.0)
        n2 = 0.0
        for x in v[v > 0]:          # (ascending vertex order, as the library adds them)
            n2 += x * x
        if n2 > 0:
            cols.append(v * (1.0 / np.sqrt(n2)))
    return np.stack(cols, axis=1) if cols else np.zeros((len(t), 0))


def fix_sign(V):
    """every column's entry of largest magnitude (lowest index on a tie) made positive"""
    V = V.copy()
    for c in range(V.shape[1]):
        at = int(np.argmax(np.abs(V[:, c])))   # (argmax: the first maximum)
        if V[at, c] < 0:
            V[:, c] = -V[:, c]
    return V


def eigenpairs(indptr, indices, data, kind, n_eigen):
    """dict: evals (n_eigen, descending), evecs (m x n_eigen), gaps (n_eigen; inf for a locked pair: the distance of a Ritz
    value to the nearest other eigenvalue of S in the complement of the locked vectors), n_components, n_locked (those among
    the n_eigen), labels, scale, S"""
    W = dense(indptr, indices, data)
    m = W.shape[0]
    labels, ncomp = components(indptr, indices)
    S, s = operator(W, kind)
    U = locked_vectors(analytic(W, kind, s), labels, ncomp)
    c = min(U.shape[1], n_eigen)
    evals = np.ones(n_eigen)
    evecs = np.zeros((m, n_eigen))
    gaps = np.full(n_eigen, np.inf)
    evecs[:, :c] = U[:, :c]
    k = n_eigen - c
    if k > 0:
        # S restricted to the complement: a basis Q of it, eigh of Q^T S Q
        Q = np.linalg.qr(U, mode="complete")[0][:, U.shape[1]:] if U.shape[1] else np.eye(m)
        T = Q.T @ S @ Q
        w, Z = np.linalg.eigh((T + T.T) / 2)
        order = np.argsort(-w, kind="stable")
        w, Z = w[order], Z[:, order]
        evals[c:] = w[:k]
        evecs[:, c:] = fix_sign(Q @ Z[:, :k])
        for i in range(k):
            others = np.delete(w, i)
            gaps[c + i] = np.min(np.abs(others - w[i])) if len(others) else np.inf
    return dict(evals=evals, evecs=evecs, gaps=gaps, n_components=ncomp, n_locked=c, labels=labels, scale=s, S=S)


def refined_pairs(r):
    """The free pairs of eigenpairs()'s result `r`, refined in longdouble until their error is far below f64's eps: dict with
    evals (n_eigen longdouble, the locked ones 1) and evecs (m x n_eigen longdouble, unit columns, sign rule applied).
    eigh's pairs (lambda, v) of S are accurate to a few eps; with the residual rho = S v - lambda v taken in longdouble,
    v <- v - sum_{j != i} q_j (q_j . rho) / (w_j - lambda) applies eigh's own approximate inverse to it, which leaves an error of
    (a few eps / gap) times the one before: three rounds end at longdouble's rounding.  lambda is the Rayleigh quotient."""
    LD = np.longdouble
    S = r["S"].astype(LD)
    w, Q = np.linalg.eigh(r["S"])
    QL = Q.astype(LD)
    c, n_eigen = r["n_locked"], len(r["evals"])
    evals = r["evals"].astype(LD)
    evecs = r["evecs"].astype(LD)
    for i in range(c, n_eigen):
        v = evecs[:, i] / np.sqrt(np.dot(evecs[:, i], evecs[:, i]))
        own = int(np.argmin(np.abs(w - r["evals"][i])))        # eigh's copy of this pair
        others = np.delete(np.arange(len(w)), own)
        Qo = QL[:, others]
        for _ in range(3):
            Sv = S @ v
            lam = np.dot(v, Sv)
            rho = Sv - lam * v
            v = v - Qo @ ((Qo.T @ rho) / (w[others].astype(LD) - lam))
            v = v / np.sqrt(np.dot(v, v))
        Sv = S @ v
        evals[i] = np.dot(v, Sv)
        at = int(np.argmax(np.abs(v)))
        evecs[:, i] = -v if v[at] < 0 else v
    return dict(evals=evals, evecs=evecs)


# ---- stage 5 restated: the Lanczos run and the rounds of csrc/spectral.cpp, in f64 with numpy's own start vectors (so the
# pairs, not the bytes, are the library's).  test_spectral_cpu.py holds it to eigh on graphs with repeated eigenvalues.
def check_due(j):
    """spectral.cpp / lanczos.hip check_due: the steps at which the host looks at T"""
    every = 1 if j <= 64 else 2 if j <= 128 else 4 if j <= 256 else 8
    return j % every == 0


def lanczos_run(S, X, want, jmax, tol, start, every_step=False, floor=0.0):
    """run_lanczos: one run on S in the complement of X's orthonormal columns for the `want` largest pairs.  dict: steps,
    converged, exhausted, theta (ascending), Y (m x steps: the Ritz vectors of theta).  floor: a lower bound of |S| (1 when a
    pair of eigenvalue 1 is locked), the least scale a beta_j is called zero against"""
    m = S.shape[0]
    B = np.zeros((m, X.shape[1] + jmax + 1))
    c = X.shape[1]
    B[:, :c] = X

    def cgs2(w, n):
        h1 = B[:, :n].T @ w
        w = w - B[:, :n] @ h1
        h2 = B[:, :n].T @ w
        return w - B[:, :n] @ h2, h1 + h2
    w, _ = cgs2(np.asarray(start, dtype=np.float64), c)
    B[:, c] = w / np.linalg.norm(w)
    alpha, beta = np.zeros(jmax), np.zeros(jmax)
    out = dict(steps=0, converged=False, exhausted=False)
    for j in range(jmax):
        w, h = cgs2(S @ B[:, c + j], c + j + 1)
        alpha[j] = h[c + j]
        beta[j] = np.linalg.norm(w)
        B[:, c + j + 1] = w / beta[j] if beta[j] > 0 else 0.0
        steps = out["steps"] = j + 1
        if steps >= want and not (every_step or check_due(steps) or steps == jmax):
            continue
        if steps < want:
            reach = max(floor, np.max(np.abs(alpha[:steps]) + 2.0 * np.abs(beta[:steps])))
            if not beta[j] <= 1e-13 * reach:
                continue
            if floor == 0.0:          # nothing locked: S is the zero matrix, refused
                raise RuntimeError(f"the Krylov space is exhausted after {steps} steps, {want} pairs were to be iterated")
            out["converged"] = out["exhausted"] = True
            break
        T = np.diag(alpha[:steps]) + np.diag(beta[:steps - 1], 1) + np.diag(beta[:steps - 1], -1)
        theta, Z = np.linalg.eigh(T)
        ok = np.isfinite(beta[j]) and np.all(np.abs(beta[j] * Z[-1, steps - want:]) <= tol)
        exhausted = steps == m - c or beta[j] <= 1e-13 * max(floor, np.max(np.abs(theta)))
        if ok or (exhausted and np.isfinite(beta[j])):
            out["converged"], out["exhausted"] = True, bool(exhausted)
            break
    steps = out["steps"]
    T = np.diag(alpha[:steps]) + np.diag(beta[:steps - 1], 1) + np.diag(beta[:steps - 1], -1)
    out["theta"], Z = np.linalg.eigh(T)
    out["Y"] = B[:, c:c + steps] @ Z
    return out


def lanczos_rounds(S, U, k, tol=1e-8, max_steps=None, seed=42, single_round=False):
    """spectral_device's rounds for the k largest pairs of S in the complement of U's columns (the locked vectors).  dict: evals
    (k, descending), evecs (m x k, sign rule applied), steps (the sum), rounds (the runs made), first (the values the first
    run alone would return: what a single run gives)"""
    m = S.shape[0]
    c = U.shape[1]
    max_steps = min(m, 1000) if max_steps is None else max_steps
    vals, vecs, steps, rounds, first = [], [], 0, 0, None
    while True:
        have = len(vals)
        lock = c + have
        checking = have >= k
        if lock == m or (checking and (single_round or c == 0 or have >= 2 * k)):    # (the k-th merge is the last one)
            break
        want = 1 if checking else k - have
        X = np.concatenate([U] + [v[:, None] for v in vecs], axis=1) if vecs else U
        run = lanczos_run(S, X, want, min(max_steps, m - lock), tol, np.random.default_rng([seed, rounds]).normal(size=m),
                          floor=1.0 if c else 0.0)
        rounds += 1
        steps += run["steps"]
        if not run["converged"]:
            raise RuntimeError(f"no convergence in round {rounds - 1} after {steps} steps")
        got = min(want, run["steps"]) if run["exhausted"] else want
        if first is None:
            first = run["theta"][::-1][:got].copy()
        if checking and not run["theta"][-1] > np.sort(vals)[::-1][k - 1] + tol:
            break
        for i in range(got):
            vals.append(run["theta"][-1 - i])
            vecs.append(run["Y"][:, -1 - i])
    order = np.argsort(-np.array(vals), kind="stable")[:k]
    return dict(evals=np.array(vals)[order], evecs=fix_sign(np.stack([vecs[i] for i in order], axis=1)), steps=steps, rounds=rounds,
                first=first)


def _mix64(z):
    z = (z + 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
    return z ^ (z >> 31)


def hash_u01(seed, stream, idx):
    """the library's counter generator (csrc/hash_u01.h) for one index"""
    key = (seed * 0xD1342543DE82EF95 + stream * 0x2545F4914F6CDD1D + 0x1234567) & 0xFFFFFFFFFFFFFFFF
    z = _mix64(idx ^ key)
    z = _mix64((z + key) & 0xFFFFFFFFFFFFFFFF)
    return float(z >> 11) * (1.0 / 9007199254740992.0)


def umap_spectral_init(E, output_dim, seed):
    """y[i][c] = 10 E[i][1 + c] / max|E[:, 1 .. output_dim]| + 1e-4 (2 hash_u01(seed, 51, i output_dim + c) - 1), every
    operation rounded as written in f64, the result rounded to E's dtype"""
    E64 = np.asarray(E, dtype=np.float64)
    m = E64.shape[0]
    top = np.max(np.abs(E64[:, 1:1 + output_dim])) if m else 0.0
    Y = np.zeros((m, output_dim), dtype=np.float64)
    for i in range(m):
        for c in range(output_dim):
            noise = 1e-4 * (2.0 * hash_u01(seed, 51, i * output_dim + c) - 1.0)
            lead = (10.0 * E64[i, 1 + c]) / top if top > 0 else 0.0
            Y[i, c] = lead + noise
    return Y.astype(np.asarray(E).dtype)
