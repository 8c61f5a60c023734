"""numpy restatement, in f64, of the Louvain clustering that include/sapca.h states (sapca_louvain_*): hashed half-active
synchronous sweeps with anchored targets, keep or undo by the modularity, aggregation between levels.  networkx is not a
dependency of this file; tests/test_louvain_cpu.py holds it to networkx's louvain_communities / modularity, the GPU tests are
held to this file.

The order in which a sum is added is not restated (numpy and scipy choose their own): the GPU tests compare exactly only where
every sum is exact in any order (dyadic weights) or where every decision of the run clears its threshold by far more than
a reordering can move it (the margins reported here)."""
import numpy as np
import scipy.sparse as sp

from umap_ref import hash_u01   # the counter generator (csrc/hash_u01.h, sapca.synth.hash_u01)

MISSES = 4


def as_csr(A, dtype=np.float64):
    A = sp.csr_matrix(A).astype(dtype)
    A.sum_duplicates()
    A.sort_indices()
    return A


def active_mask(n, seed, level, t):
    idx = (np.uint64((int(level) * 4096 + int(t)) << 32) + np.arange(n, dtype=np.uint64))
    return hash_u01(seed, 41, idx) < 0.5


def degrees(A, dtype=np.float64):
    A = sp.csr_matrix(A)
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    k = np.zeros(A.shape[0], dtype=dtype)
    np.add.at(k, rows, A.data.astype(dtype))
    return k


def modularity(A, c, gamma=1.0, dtype=np.float64):
    """Q(c) = (sum_i s_i) / S - gamma sum_C (tot_C / S)^2; a vertex whose label is outside [0, n) is left out of s and tot"""
    A = sp.csr_matrix(A)
    n = A.shape[0]
    c = np.asarray(c, dtype=np.int64)
    k = degrees(A, dtype)
    S = k.sum()
    if not S > 0:
        return 0.0
    ok = (c >= 0) & (c < n)
    rows = np.repeat(np.arange(n), np.diff(A.indptr))
    cols = A.indices
    same = ok[rows] & ok[cols] & (c[rows] == c[cols])
    sum_s = A.data.astype(dtype)[same].sum()
    tot = np.zeros(n, dtype=dtype)
    np.add.at(tot, c[ok], k[ok])
    return sum_s / S - dtype(gamma) * ((tot / S) ** 2).sum()


def gains(A, c, seed, level, t, gamma, dtype=np.float64):
    """Everything a sweep decides from: per active vertex g_C, and the candidates (row, D, g_D) as flat arrays."""
    A = sp.csr_matrix(A)
    n = A.shape[0]
    c = np.asarray(c, dtype=np.int64)
    ok = (c >= 0) & (c < n)
    k = degrees(A, dtype)
    S = k.sum()
    tot = np.zeros(n, dtype=dtype)
    np.add.at(tot, c[ok], k[ok])
    active = active_mask(n, seed, level, t) & ok
    anchored = np.zeros(n, dtype=bool)
    anchored[c[ok & ~active]] = True
    rows = np.repeat(np.arange(n), np.diff(A.indptr))
    cols = A.indices.astype(np.int64)
    use = (cols != rows) & active[rows] & ok[cols]
    r_, d_, a_ = rows[use], c[cols[use]], A.data.astype(dtype)[use]
    # w_iD: the entries of a row grouped by the community of their column
    order = np.lexsort((d_, r_))
    r_, d_, a_ = r_[order], d_[order], a_[order]
    head = np.ones(len(r_), dtype=bool)
    head[1:] = (r_[1:] != r_[:-1]) | (d_[1:] != d_[:-1])
    seg = np.cumsum(head) - 1
    w = np.zeros(int(head.sum()), dtype=dtype)
    np.add.at(w, seg, a_)
    wr, wd = r_[head], d_[head]
    with np.errstate(invalid="ignore", divide="ignore"):
        r = (dtype(gamma) * k) / S
    own = wd == c[wr]
    w_own = np.zeros(n, dtype=dtype)
    w_own[wr[own]] = w[own]
    g_c = w_own - r * (tot[np.where(ok, c, 0)] - k)
    cand = ~own & anchored[wd]
    cr, cd = wr[cand], wd[cand]
    cg = w[cand] - r[cr] * tot[cd]
    return dict(n=n, active=active, g_c=g_c, rows=cr, D=cd, g=cg, k=k, S=S, tot=tot, r=r)


def sweep(A, c, seed, level, t, gamma):
    """one sweep, no keep / undo: (c', n_moved, margin); margin = the smallest gap between a vertex's best gain and its
    second-best distinct gain (g_C counted among the gains)"""
    c = np.asarray(c, dtype=np.int64)
    G = gains(A, c, seed, level, t, gamma)
    out = c.copy()
    margin = np.inf
    cr, cd, cg = G["rows"], G["D"], G["g"]
    if len(cr):
        order = np.lexsort((cd, -cg, cr))   # per row: the largest gain first, ties by the lowest label
        cr, cd, cg = cr[order], cd[order], cg[order]
        first = np.ones(len(cr), dtype=bool)
        first[1:] = cr[1:] != cr[:-1]
        br, bd, bg = cr[first], cd[first], cg[first]
        move = bg > G["g_c"][br]
        out[br[move]] = bd[move]
        # margins: all gains of a row, g_C among them
        ar = np.concatenate([cr, br])
        ag = np.concatenate([cg, G["g_c"][br]])
        o2 = np.lexsort((-ag, ar))
        ar, ag = ar[o2], ag[o2]
        top = np.maximum.reduceat(ag, np.flatnonzero(np.r_[True, ar[1:] != ar[:-1]]))
        top_of = top[np.cumsum(np.r_[True, ar[1:] != ar[:-1]]) - 1]
        below = ag < top_of
        if below.any():
            margin = float((top_of[below] - ag[below]).min())
    return out, int((out != c).sum()), margin


def aggregate(A, c):
    """(A', renumbered): communities renumbered in ascending order of label; a vertex whose label is out of range is left out"""
    A = sp.csr_matrix(A).astype(np.float64)
    n = A.shape[0]
    c = np.asarray(c, dtype=np.int64)
    ok = (c >= 0) & (c < n)
    labels, inv = np.unique(c[ok], return_inverse=True)
    ren = c.copy()
    ren[ok] = inv
    P = sp.csr_matrix((np.ones(int(ok.sum())), (np.flatnonzero(ok), inv)), shape=(n, len(labels)))
    C = (P.T @ A @ P).tocsr()
    C.sum_duplicates()
    C.sort_indices()
    return C, ren


def run(A, seed=42, gamma=1.0, tol=1e-7, max_sweeps=256, max_levels=32):
    """the whole run: dict(labels, n_communities, Q, n_levels, levels=[dict(labels, Q, kept, sweeps)], margin_gain, margin_q)"""
    A = as_csr(A)
    m = A.shape[0]
    final = np.arange(m, dtype=np.int64)
    out = dict(labels=final.astype(np.int32), n_communities=m, Q=0.0, n_levels=0, levels=[], margin_gain=np.inf, margin_q=np.inf)
    if m == 0:
        return out
    level = 0
    while True:
        n = A.shape[0]
        c = np.arange(n, dtype=np.int64)
        if not degrees(A).sum() > 0:
            break
        Q = modularity(A, c, gamma)
        if level == 0:
            out["Q"] = float(Q)
        misses, kept, t = 0, 0, 0
        while t < max_sweeps and misses < MISSES:
            c2, moved, margin = sweep(A, c, seed, level, t, gamma)
            out["margin_gain"] = min(out["margin_gain"], margin)
            if moved == 0:
                misses += 1
            else:
                Q2 = modularity(A, c2, gamma)
                out["margin_q"] = min(out["margin_q"], abs(Q2 - (Q + tol)))
                if Q2 > Q + tol:
                    c, Q, misses, kept = c2, Q2, 0, kept + 1
                else:
                    misses += 1
            t += 1
        info = dict(labels=c.astype(np.int32), Q=float(Q), kept=kept, sweeps=t)
        if kept == 0:
            out["levels"].append(info)
            break
        A, ren = aggregate(A, c)
        final = ren[final]
        info["labels"] = final.astype(np.int32)
        out["levels"].append(info)
        out.update(labels=final.astype(np.int32), n_communities=A.shape[0], Q=float(Q), n_levels=out["n_levels"] + 1)
        level += 1
        if A.shape[0] <= 1 or level >= max_levels:
            break
    return out


# ---------------------------------------------------------------- fixtures
def ring(n):
    i = np.arange(n)
    return as_csr(sp.coo_matrix((np.ones(2 * n), (np.r_[i, i], np.r_[(i + 1) % n, (i - 1) % n])), shape=(n, n)))


def grid(a, b):
    idx = np.arange(a * b).reshape(a, b)
    r = np.r_[idx[:, :-1].ravel(), idx[:-1, :].ravel()]
    c = np.r_[idx[:, 1:].ravel(), idx[1:, :].ravel()]
    return as_csr(sp.coo_matrix((np.ones(2 * len(r)), (np.r_[r, c], np.r_[c, r])), shape=(a * b, a * b)))


def planted(groups, size, seed=3, p_in=0.2, p_out=0.01):
    """a planted partition with weights k / 8 (k = 1 .. 8): every sum of them is exact in any order"""
    n = groups * size
    i, j = np.triu_indices(n, 1)
    u = hash_u01(seed, 51, (i * n + j).astype(np.uint64))
    v = hash_u01(seed, 52, (i * n + j).astype(np.uint64))
    keep = u < np.where(i // size == j // size, p_in, p_out)
    w = (np.floor(v[keep] * 8) + 1) / 8.0
    i, j = i[keep], j[keep]
    return as_csr(sp.coo_matrix((np.r_[w, w], (np.r_[i, j], np.r_[j, i])), shape=(n, n)))


def matching(n):
    i = np.arange(0, n, 2)
    return as_csr(sp.coo_matrix((np.ones(n), (np.r_[i, i + 1], np.r_[i + 1, i])), shape=(n, n)))


def clique(n):
    return as_csr(sp.csr_matrix(np.ones((n, n)) - np.eye(n)))


def star(n):
    j = np.arange(1, n)
    z = np.zeros(n - 1, dtype=np.int64)
    return as_csr(sp.coo_matrix((np.ones(2 * (n - 1)), (np.r_[z, j], np.r_[j, z])), shape=(n, n)))


def two_cliques(size=8):
    B = np.zeros((2 * size, 2 * size))
    B[:size, :size] = 1
    B[size:, size:] = 1
    np.fill_diagonal(B, 0)
    B[size - 1, size] = B[size, size - 1] = 1
    return as_csr(sp.csr_matrix(B))


def comb(hub_degrees, n_leaves=20000):
    """hubs of the given degrees over a shared pool of leaves (hub h takes the leaves (h * 977 + t * 1) mod n_leaves ...), the
    weights k / 8: vertices 0 .. n_hubs - 1 are the hubs, the rest the leaves"""
    nh = len(hub_degrees)
    rows, cols, vals = [], [], []
    for h, d in enumerate(hub_degrees):
        leaves = (h * 977 + np.arange(d)) % n_leaves
        rows.append(np.full(d, h))
        cols.append(nh + leaves)
        vals.append(((h + np.arange(d)) % 8 + 1) / 8.0)
    r, c, v = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
    n = nh + n_leaves
    return as_csr(sp.coo_matrix((np.r_[v, v], (np.r_[r, c], np.r_[c, r])), shape=(n, n)))


def knn_fuzzy_blob(m=2000, d=10, n_neighbors=15, seed=5):
    """the fuzzy union (tests/umap_ref.py) of the exact neighbour lists of one structureless Gaussian blob"""
    import knn_ref as KR
    import umap_ref as UR
    X = np.random.default_rng(seed).standard_normal((m, d))
    idx, dist = KR.knn(X, X, n_neighbors - 1, "euclidean", exclude_self=True)
    sigma, rho, _, _ = UR.smooth(idx, dist, n_neighbors)
    return as_csr(UR.union(idx, UR.memberships(idx, dist, sigma, rho)))
