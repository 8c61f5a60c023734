"""A numpy restatement in f64 of the Harmony of include/sapca.h (sapca_harmony_*), items 1-6, literally: dense one-hot design
matrices and numpy.linalg.solve for the ridge (NOT the closed form the library runs, so the two check each other), the update
order from sapca.synth.hash_u01 on the CPU.  tests/test_harmony_cpu.py holds it to scikit-learn's Ridge and scipy's softmax;
the GPU tests hold the library to it.

Besides the results a whole run reports its convergence margins, |ratio - epsilon| / epsilon of every test of items 4 and 6:
a run whose smallest margin is large decides every stop the same way under rounding."""
import numpy as np
import torch

from sapca.synth import hash_u01

STREAM = 61   # the stream of the update order in the counter generator


def normalise_rows(X):
    """rows scaled to unit L2 norm, a row of norm 0 stays 0"""
    X = np.asarray(X, dtype=np.float64)
    n = np.sqrt((X * X).sum(axis=1, keepdims=True))
    return np.divide(X, n, out=np.zeros_like(X), where=n > 0)


def design(batch, B):
    """Phi (B x m one-hot) and Phi~ (an intercept row over it)"""
    batch = np.asarray(batch)
    Phi = np.zeros((B, batch.shape[0]))
    Phi[batch, np.arange(batch.shape[0])] = 1.0
    return Phi, np.vstack([np.ones((1, batch.shape[0])), Phi])


def order(seed, c, m):
    """the update order of pass c: the rows sorted by (hash_u01(seed, 61, c m + i), i)"""
    u = hash_u01(int(seed), STREAM, torch.arange(m, dtype=torch.int64) + int(c) * m).numpy()
    return np.lexsort((np.arange(m), u))


def blocks(seed, c, m, n_blocks):
    return np.array_split(order(seed, c, m), n_blocks)


def distances(Zc, Y):
    return 2.0 * (1.0 - np.asarray(Zc, dtype=np.float64) @ np.asarray(Y, dtype=np.float64).T)


def soft(dist, sigma):
    """exp(-(dist - the row's minimum) / sigma)"""
    return np.exp(-(dist - dist.min(axis=1, keepdims=True)) / sigma)


def init_R(Zc, Y, sigma):
    S = soft(distances(Zc, Y), sigma)
    return S / S.sum(axis=1, keepdims=True)


def centroids(R, Zc):
    return normalise_rows(np.asarray(R, dtype=np.float64).T @ np.asarray(Zc, dtype=np.float64))


def objective(R, dist, O, E, batch, sigma, theta):
    """the three terms of item 3"""
    with np.errstate(divide="ignore", invalid="ignore"):
        ent = np.where(R > 0, R * np.log(R), 0.0)
    return np.array([(R * dist).sum(), sigma * ent.sum(), sigma * theta * (R * np.log((O + 1.0) / (E + 1.0))[batch]).sum()])


def one_pass(Zc, batch, B, Y, R, theta, sigma, n_blocks, seed, c, recompute=True):
    """item 2: (Y, R, O, rs, E, dist) after pass c from the R given (not modified)"""
    Zc = np.asarray(Zc, dtype=np.float64)
    R = np.array(R, dtype=np.float64)
    m = Zc.shape[0]
    Phi, _ = design(batch, B)
    Pr = Phi.sum(axis=1) / m
    Y = centroids(R, Zc) if recompute else np.asarray(Y, dtype=np.float64)
    dist = distances(Zc, Y)
    S = soft(dist, sigma)
    rs = R.sum(axis=0)
    O = Phi @ R
    E = np.outer(Pr, rs)
    for blk in blocks(seed, c, m, n_blocks):
        if blk.size == 0:
            continue
        rs = rs - R[blk].sum(axis=0)
        O = O - Phi[:, blk] @ R[blk]
        E = np.outer(Pr, rs)
        new = S[blk] * (((E + 1.0) / (O + 1.0)) ** theta)[batch[blk]]
        R[blk] = new / new.sum(axis=1, keepdims=True)
        rs = rs + R[blk].sum(axis=0)
        O = O + Phi[:, blk] @ R[blk]
        E = np.outer(Pr, rs)
    return Y, R, O, rs, E, dist


def ridge(Z, R, batch, B, lam):
    """item 5 by the dense solve: (Zcorr, W) with W[k] the (B + 1) x d coefficients of cluster k, intercept row zeroed"""
    Z = np.asarray(Z, dtype=np.float64)
    R = np.asarray(R, dtype=np.float64)
    _, Pt = design(batch, B)
    K = R.shape[1]
    Zcorr = Z.copy()
    W = np.zeros((K, B + 1, Z.shape[1]))
    pen = np.diag(np.r_[0.0, np.full(B, lam)])
    for k in range(K):
        if R[:, k].sum() == 0.0:
            continue
        PR = Pt * R[:, k]
        W[k] = np.linalg.solve(PR @ Pt.T + pen, PR @ Z)
        W[k][0] = 0.0
        Zcorr -= (PR.T @ W[k])
    return Zcorr, W


def ridge_closed(Z, R, batch, B, lam, ft=np.float64):
    """item 5 by the closed form of the arrow matrix: (Zcorr, beta) with beta K x B x d.  ft = numpy.longdouble evaluates it in
    extended precision (rounded once to f64 at the end): what the GPU's coefficients are held to, with an error of its own far
    below an f64 sum's."""
    Z = np.asarray(Z, dtype=ft)
    R = np.asarray(R, dtype=ft)
    Phi = design(batch, B)[0].astype(ft)
    lam = ft(lam)
    K = R.shape[1]
    beta = np.zeros((K, B, Z.shape[1]), dtype=ft)
    for k in range(K):
        o = Phi @ R[:, k]
        if o.sum() == 0.0:
            continue
        t = (Phi * R[:, k]) @ Z
        cb = o / (o + lam)
        a = ((1.0 - cb)[:, None] * t).sum(axis=0) / ((1.0 - cb) * o).sum()
        beta[k] = (t - np.outer(o, a)) / (o + lam)[:, None]
    Zcorr = Z.copy()
    for k in range(K):
        Zcorr -= R[:, k:k + 1] * beta[k][batch]
    return Zcorr.astype(np.float64), beta.astype(np.float64)


def run(Z, batch, B, Y0, theta=2.0, sigma=0.1, lam=1.0, n_blocks=20, max_iter_harmony=10, max_iter_cluster=20, epsilon_cluster=1e-5,
        epsilon_harmony=1e-4, seed=42, dtype=np.float64):
    """items 1-6 from given centroids Y0 (K x d).  `dtype`: what the library stores Zc, Y, R and the corrected panel in (the values
    are rounded to it where the library rounds them; all arithmetic stays f64).  Returns a dict: Zcorr, R, Y, objectives, passes,
    n_iter, converged, margin (the smallest |ratio - epsilon| / epsilon over every convergence test of the run)."""
    rnd = lambda a: np.asarray(a, dtype=dtype).astype(np.float64)
    Z = rnd(Z)
    batch = np.asarray(batch)
    Zc = rnd(normalise_rows(Z))
    Y = rnd(normalise_rows(rnd(Y0)))
    R = rnd(init_R(Zc, Y, sigma))
    objectives, passes, margins = [], [], []
    c = 0
    converged = False
    Zcorr = Z
    for it in range(1, max_iter_harmony + 1):
        obj = []
        for i in range(max_iter_cluster):
            Y, R, O, rs, E, dist = one_pass(Zc, batch, B, Y, R, theta, sigma, n_blocks, seed, c)
            Y, R = rnd(Y), rnd(R)
            c += 1
            obj.append(objective(R, dist, O, E, batch, sigma, theta).sum())
            if i > 3:
                new, old = obj[i - 2] + obj[i - 1] + obj[i], obj[i - 3] + obj[i - 2] + obj[i - 1]
                ratio = (old - new) / abs(old)
                if epsilon_cluster > 0:
                    margins.append(abs(ratio - epsilon_cluster) / epsilon_cluster)
                if ratio < epsilon_cluster:
                    break
        objectives.append(obj[-1])
        passes.append(len(obj))
        Zcorr = rnd(ridge(Z, R, batch, B, lam)[0])
        Zc = rnd(normalise_rows(Zcorr))
        if it >= 2:
            ratio = (objectives[-2] - objectives[-1]) / abs(objectives[-2])
            if epsilon_harmony > 0:
                margins.append(abs(ratio - epsilon_harmony) / epsilon_harmony)
            if ratio < epsilon_harmony:
                converged = True
                break
    return dict(Zcorr=Zcorr, R=R, Y=Y, objectives=np.array(objectives), passes=np.array(passes), n_iter=len(passes),
                converged=converged, margin=min(margins) if margins else np.inf)


def two_batch_fixture(m_per=300, d=10, n_types=3, seed=7):
    """Two batches of n_types cell types each: type centres, a batch shift along a direction of its own, unit-variance noise.
    Returns (Z float64 (2 m_per) x d, batch int32, cell type int32)."""
    rng = np.random.default_rng(seed)
    centres = rng.normal(size=(n_types, d)) * 6.0
    shift = rng.normal(size=(2, d)) * 2.5
    rows, batch, kind = [], [], []
    for b in range(2):
        t = rng.integers(0, n_types, size=m_per)
        rows.append(centres[t] + shift[b] + rng.normal(size=(m_per, d)))
        batch.append(np.full(m_per, b))
        kind.append(t)
    return np.vstack(rows), np.concatenate(batch).astype(np.int32), np.concatenate(kind).astype(np.int32)


def same_label_share(idx, labels):
    """the share of neighbour slots (idx: m x k) whose row carries the label of the query row"""
    labels = np.asarray(labels)
    return float((labels[idx] == labels[:, None]).mean())


def knn_bruteforce(X, k):
    X = np.asarray(X, dtype=np.float64)
    g = X @ X.T
    sq = np.diag(g)
    d2 = sq[:, None] + sq[None, :] - 2.0 * g
    np.fill_diagonal(d2, np.inf)
    return np.argsort(d2, axis=1, kind="stable")[:, :k]
