"""numpy restatement, in f64, of the UMAP that include/sapca.h states (stages 2-5 of sapca_umap_* and the curve fit of
sapca_umap_find_ab): umap-learn's fuzzy simplicial set with local_connectivity = 1 and set_op_mix_ratio = 1, and a
synchronous, deterministic form of its optimize_layout_euclidean.  umap-learn itself is not a dependency; the curve fit is
held to scipy.optimize.curve_fit by tests/test_umap_cpu.py, the GPU tests are held to this file.

Dense m x m intermediates in the union: for the few hundred rows the tests use, not for data."""
import numpy as np
import scipy.sparse as sp

from tsne_ref import clusters, exp_exact, hub_lists, sort_classes   # noqa: F401  (the same synthetic clusters and hand-made lists, the correctly rounded exp)

MASK64 = (1 << 64) - 1


# ---------------------------------------------------------------- the counter generator (csrc/hash_u01.h, sapca.synth.hash_u01)
def _mix64(z):
    z = z + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def hash_u01(seed, stream, idx):
    """uniform [0, 1) f64 from (seed, stream, idx); idx: uint64 array (wrap-around arithmetic)"""
    with np.errstate(over="ignore"):
        key = np.uint64((int(seed) * 0xD1342543DE82EF95 + int(stream) * 0x2545F4914F6CDD1D + 0x1234567) & MASK64)
        z = _mix64(np.asarray(idx, dtype=np.uint64) ^ key)
        z = _mix64(z + key)
    return (z >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


# ---------------------------------------------------------------- stage 2
def valid_slots(indices):
    indices = np.asarray(indices)
    return (indices >= 0) & (indices < indices.shape[0])


def smooth(indices, dist, n_neighbors):
    """(sigma, rho, floored, margin): the search of stage 2 per row.  floored[i]: the floor governs sigma_i.  margin: the
    smallest distance of any decision of any search from its threshold (| |psum - target| - 1e-5 | and |psum - target|)."""
    indices = np.asarray(indices)
    m, K = indices.shape
    ok = valid_slots(indices)
    d = np.where(ok, np.asarray(dist, dtype=np.float64), 0.0)
    target = np.log2(float(n_neighbors))
    total = d.sum()
    sigma, rho, floored = np.ones(m), np.zeros(m), np.zeros(m, dtype=bool)
    margin = np.inf
    for i in range(m):
        di, oki = d[i], ok[i]
        pos = oki & (di > 0)
        rho[i] = di[pos].min() if pos.any() else 0.0
        x = di - rho[i]
        lo, hi, mid = 0.0, np.inf, 1.0
        for _ in range(64):
            with np.errstate(over="ignore"):
                p = np.where(oki, np.where(x > 0, np.exp(-np.where(x > 0, x, 0.0) / mid), 1.0), 0.0)
            psum = p.sum()
            gap = psum - target
            margin = min(margin, abs(abs(gap) - 1e-5))
            if abs(gap) < 1e-5:
                break
            margin = min(margin, abs(gap))
            if gap > 0:
                hi = mid
                mid = (lo + hi) / 2.0
            else:
                lo = mid
                mid = mid * 2.0 if hi == np.inf else (lo + hi) / 2.0
        floor_at = 1e-3 * (di.sum() / n_neighbors) if rho[i] > 0 else 1e-3 * (total / (float(m) * n_neighbors))
        floored[i] = floor_at > mid
        sigma[i] = max(mid, floor_at)
    return sigma, rho, floored, margin


def memberships(indices, dist, sigma, rho):
    """a[i, k]: 1 where d_k - rho_i <= 0, else exp(-(d_k - rho_i) / sigma_i) correctly rounded; 0 in a slot that does not count"""
    indices = np.asarray(indices)
    m, K = indices.shape
    ok = valid_slots(indices)
    d = np.where(ok, np.asarray(dist, dtype=np.float64), 0.0)
    a = np.zeros((m, K))
    for i in range(m):
        for k in range(K):
            if ok[i, k]:
                x = d[i, k] - rho[i]
                a[i, k] = exp_exact(-x / sigma[i]) if x > 0 else 1.0
    return a


# ---------------------------------------------------------------- stage 3
def union(indices, a, dtype=np.float64):
    """G = (A + A^T) - A o A^T in f64, a missing direction counting 0, rounded once to dtype: a canonical scipy CSR that keeps
    every listed pair (a membership that underflowed to 0 stays stored)"""
    indices = np.asarray(indices)
    m, K = indices.shape
    ok = valid_slots(indices)
    rows = np.repeat(np.arange(m), K).reshape(m, K)[ok]
    cols = indices[ok]
    A = np.zeros((m, m))
    has = np.zeros((m, m), dtype=bool)
    A[rows, cols] = np.asarray(a, dtype=np.float64)[ok]
    has[rows, cols] = True
    G = (A + A.T) - A * A.T
    mask = has | has.T
    indptr = np.concatenate([[0], np.cumsum(mask.sum(axis=1))]).astype(np.int64)
    return sp.csr_matrix((G[mask].astype(dtype), np.nonzero(mask)[1].astype(np.int32), indptr), shape=(m, m))


def graph(indices, dist, n_neighbors, dtype=np.float64):
    """stages 2-3: (G, sigma, rho)"""
    sigma, rho, _, _ = smooth(indices, dist, n_neighbors)
    return union(indices, memberships(indices, dist, sigma, rho), dtype), sigma, rho


# ---------------------------------------------------------------- stage 4
def curve_points(spread, min_dist):
    x = 3.0 * spread * np.arange(300, dtype=np.float64) / 299.0
    y = np.where(x < min_dist, 1.0, np.exp(-(x - min_dist) / spread))
    return x, y


def curve(x, a, b):
    return 1.0 / (1.0 + a * x ** (2.0 * b))


def find_ab(spread=1.0, min_dist=0.1, steps=500):
    """least squares of curve() to curve_points() from (1, 1): damped steps while far, plain Gauss-Newton once a step is small,
    until a step is below 1e-14 relative (or cannot shrink further)"""
    x, y = curve_points(spread, min_dist)
    lx = np.log(np.where(x > 0, x, 1.0))

    def system(a, b):
        xb = np.where(x > 0, x ** (2.0 * b), 0.0)
        f = 1.0 / (1.0 + a * xb)
        r = f - y
        J = np.stack([-xb * f * f, -2.0 * a * xb * lx * f * f], axis=1)
        return J, r, float(r @ r)

    a, b, lam = 1.0, 1.0, 1e-3
    last = np.inf
    for _ in range(steps):
        J, r, cost = system(a, b)
        N, g = J.T @ J, J.T @ r
        step = np.linalg.solve(N, -g)
        size = max(abs(step[0] / a), abs(step[1] / b))
        if size <= 1e-4:
            a, b = a + step[0], b + step[1]
            if size <= 1e-14 or size >= last:
                return a, b
            last = size
            continue
        step = np.linalg.solve(N + lam * np.diag(np.diag(N)), -g)
        if a + step[0] > 0 and b + step[1] > 0 and system(a + step[0], b + step[1])[2] <= cost:
            a, b, lam = a + step[0], b + step[1], lam * 0.1
        else:
            lam *= 10.0
    raise RuntimeError("find_ab did not converge")


# ---------------------------------------------------------------- stage 5
def default_epochs(m):
    return 500 if m <= 10000 else 200


def init_panel(X, D):
    X = np.asarray(X, dtype=np.float64)[:, :D]
    lo, hi = X.min(axis=0), X.max(axis=0)
    rng = hi - lo
    return np.where(rng > 0, 10.0 * (X - lo) / np.where(rng > 0, rng, 1.0), 0.0)


def init_random(m, D, seed):
    return 10.0 * hash_u01(seed, 31, np.arange(m * D, dtype=np.uint64)).reshape(m, D)


def layout(G, Y0, n_epochs, a, b, negative_sample_rate=5, learning_rate=1.0, repulsion_strength=1.0, seed=42,
           storage=np.float64, reverse=False, return_stats=False):
    """stage 5 from the initial embedding Y0 (stored in `storage`): Y after n_epochs epochs.  Everything is evaluated in f64
    from the stored values and rounded once per epoch.  A vertex adds its terms in the order of its stored entries, an
    entry's attraction before its samples; reverse: in the opposite order, and s^b as exp(b ln s) -- a legitimately reordered
    evaluation.  return_stats: also {"qmax", "sampled": per-entry counts of epochs in which it was due}."""
    G = sp.csr_matrix(G)
    m = G.shape[0]
    nnz = G.nnz
    rate = int(negative_sample_rate)
    w = G.data.astype(np.float64)
    row = np.repeat(np.arange(m), np.diff(G.indptr))
    col = G.indices.astype(np.int64)
    wmax = w.max() if nnz else 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        used = (w > 0) & ~(w < wmax / float(n_epochs))
        eps = wmax / w
        epsn = eps / float(rate) if rate > 0 else np.full(nnz, np.inf)
    nxt, nxtn = eps.copy(), epsn.copy()
    Y = np.asarray(Y0).astype(storage)
    D = Y.shape[1]
    sampled = np.zeros(nnz, dtype=np.int64)
    qmax = 0

    def power(s):
        return np.exp(b * np.log(s)) if reverse else s ** b

    def force(delta, coef_of):
        s = (delta * delta).sum(axis=1)
        c = np.zeros_like(s)
        pos = s > 0
        c[pos] = coef_of(s[pos])
        return np.clip(c[:, None] * delta, -4.0, 4.0)

    for n in range(int(n_epochs)):
        alpha = learning_rate * (1.0 - float(n) / float(n_epochs))
        Yd = Y.astype(np.float64)
        due = np.nonzero(used & (nxt <= n))[0]
        sampled[due] += 1
        keys = [due * 65]
        vert = [row[due]]
        terms = [force(Yd[row[due]] - Yd[col[due]], lambda s: -2.0 * a * b * (power(s) / s) / (a * power(s) + 1.0))]
        nxt[due] += eps[due]
        if rate > 0 and due.size:
            q = np.floor((n - nxtn[due]) / epsn[due])
            qmax = max(qmax, int(q.max()))
            assert q.min() >= 0 and q.max() < 64
            for p in range(int(q.max())):
                e = due[q > p]
                ctr = (np.uint64(n) * np.uint64(nnz) + e.astype(np.uint64)) * np.uint64(64) + np.uint64(p)
                k = np.minimum(np.floor(hash_u01(seed, 32, ctr) * m).astype(np.int64), m - 1)
                keys.append(e * 65 + 1 + p)
                vert.append(row[e])
                terms.append(force(Yd[row[e]] - Yd[k],
                                   lambda s: 2.0 * repulsion_strength * b / ((0.001 + s) * (a * power(s) + 1.0))))
            nxtn[due] += q * epsn[due]
        keys, vert, terms = np.concatenate(keys), np.concatenate(vert), np.concatenate(terms)
        order = np.argsort(keys, kind="stable")
        if reverse:
            order = order[::-1]
        acc = np.zeros((m, D))
        np.add.at(acc, vert[order], terms[order])
        Y = np.where(acc == 0.0, Y, (Yd + alpha * acc).astype(storage))
    if return_stats:
        return Y, dict(qmax=qmax, sampled=sampled, used=used)
    return Y


def same_cluster_share(Y, labels):
    """the share of points whose nearest embedded neighbour carries their own label"""
    Y = np.asarray(Y, dtype=np.float64)
    d2 = ((Y[:, None, :] - Y[None, :, :]) ** 2).sum(axis=2)
    np.fill_diagonal(d2, np.inf)
    return float((labels[d2.argmin(axis=1)] == labels).mean())
