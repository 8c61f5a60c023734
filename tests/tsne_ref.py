"""numpy / scipy restatement, in f64, of the t-SNE that include/sapca.h states (stages 2-5 of sapca_tsne_*): van der Maaten's
bh_tsne with the repulsive term evaluated exactly.  tests/test_tsne_cpu.py holds it to scikit-learn's own t-SNE gradient
and Kullback-Leibler divergence (tests/golden/g8_tsne.npz); the GPU tests are held to it.

Dense m x m intermediates: for the few thousand rows the tests use, not for data."""
import decimal
import math

import numpy as np
import scipy.sparse as sp

DBL_MIN = np.finfo(np.float64).tiny


def neighbours_of(perplexity):
    return int(np.floor(3.0 * perplexity))


_CTX = decimal.Context(prec=50)


def exp_exact(x):
    """exp(x) rounded to nearest: 50 decimal digits, then one rounding to f64"""
    return float(_CTX.exp(decimal.Decimal(x)))


def entropy_gap(D, ok, beta, perplexity, exact=True):
    """H - ln(perplexity) and p_k|i of one row at beta (D: squared distances, ok: the slots that count).  The two sums are
    correctly rounded (math.fsum) and so is exp (exp_exact), so that p_k|i carries one rounding of exp, one of the sum and one
    of the division, and no summation order: P is compared to 2 ulp, and a single addend whose exp is one ulp off can
    already use up 4 (its quotient and its scaling by 1 / 2m may each double the error counted in ulp).  Measured against
    mpmath, numpy's vectorised exp is off the correctly rounded value for 6 arguments in 100 and libm's for 6 in 10 000.
    exact=False: libm's exp, for the steps of the search, where only the sign of the gap matters."""
    ex = exp_exact if exact else math.exp
    p = np.array([ex(-beta * d) if o else 0.0 for d, o in zip(D.tolist(), np.asarray(ok).tolist())])
    s = math.fsum(p) + DBL_MIN
    H = np.log(s) + beta * math.fsum(D * p) / s
    return H - np.log(perplexity), p / s


def conditional(indices, dist, perplexity):
    """stage 2: (p, beta); p[i, k] = p_{indices[i, k] | i}.  A slot whose index is outside [0, m) contributes nothing."""
    indices = np.asarray(indices)
    m, K = indices.shape
    D = np.asarray(dist, dtype=np.float64) ** 2
    ok = (indices >= 0) & (indices < m)
    p = np.zeros((m, K))
    beta = np.ones(m)
    for i in range(m):
        b, lo, hi = 1.0, -np.inf, np.inf
        for _ in range(200):
            gap, _p = entropy_gap(D[i], ok[i], b, perplexity, exact=False)
            if abs(gap) < 1e-5:
                break
            if gap > 0:
                lo = b
                b = b * 2.0 if hi == np.inf else 0.5 * (b + hi)
            else:
                hi = b
                b = b * 0.5 if lo == -np.inf else 0.5 * (b + lo)
        beta[i] = b
        p[i] = entropy_gap(D[i], ok[i], b, perplexity)[1]
    return p, beta


def symmetrise(indices, p, dtype=np.float64):
    """stage 3: (C + C^T) / (2 m) as a canonical scipy CSR (the sum in f64, rounded once to dtype)"""
    indices = np.asarray(indices)
    m, K = indices.shape
    ok = (indices >= 0) & (indices < m)
    rows = np.repeat(np.arange(m), K).reshape(m, K)[ok]
    C = sp.csr_matrix((np.asarray(p, dtype=np.float64)[ok], (rows, indices[ok])), shape=(m, m))
    C.sum_duplicates()
    S = (C + C.T).tocsr()
    S.sum_duplicates()
    S.sort_indices()
    S.data = (S.data * (1.0 / (2.0 * m))).astype(dtype)
    return S


def gradient(P, Y, exaggeration=1.0, reverse=False, arith=np.float64):
    """stage 4: (g, Z, KL).  reverse: the sums over j run in the opposite order.  arith = float32: the pair arithmetic and the
    sums of the repulsion in f32 (what an all-f32 implementation computes); the attraction and the rest stay f64."""
    P = sp.csr_matrix(P)
    Y64 = np.asarray(Y, dtype=np.float64)
    m, D = Y64.shape
    Ya = Y64.astype(arith)
    order = np.arange(m)[::-1] if reverse else np.arange(m)
    diff = Ya[:, None, :] - Ya[None, order, :]                       # (i, j, c)
    q = (arith(1) / (arith(1) + (diff * diff).sum(axis=2, dtype=arith))).astype(arith)
    q[order, np.arange(m)] = 0                                        # the pair i == j, by index
    zrow = q.sum(axis=1, dtype=arith)
    Z = float(zrow.astype(np.float64).sum()) if arith is np.float64 else float(zrow.sum(dtype=arith))
    rep = ((q * q)[:, :, None] * diff).sum(axis=1, dtype=arith).astype(np.float64)
    coo = P.tocoo()
    r, c, v = coo.row, coo.col, coo.data.astype(np.float64)
    if reverse:
        r, c, v = r[::-1], c[::-1], v[::-1]
    d = Y64[r] - Y64[c]
    qe = 1.0 / (1.0 + (d * d).sum(axis=1))
    attr = np.stack([np.bincount(r, weights=v * qe * d[:, k], minlength=m) for k in range(D)], axis=1)
    pos = v > 0
    kl = float((v[pos] * np.log(v[pos] * Z / qe[pos])).sum())
    return exaggeration * attr - rep / Z, Z, kl


DEFAULTS = dict(stop_lying_epoch=250, momentum_switch_epoch=250, exaggeration=12.0, learning_rate=200.0, momentum=0.5,
                final_momentum=0.8)


def embed(P, Y0, epochs, reverse=False, return_gains=False, **constants):
    """stage 5 from the initial embedding Y0 (re-centred first): (Y, KL of Y)"""
    c = dict(DEFAULTS, **constants)
    Y = np.array(Y0, dtype=np.float64)
    Y -= Y.mean(axis=0)
    v = np.zeros_like(Y)
    gain = np.ones_like(Y)
    for t in range(epochs):
        e = c["exaggeration"] if t < c["stop_lying_epoch"] else 1.0
        mu = c["momentum"] if t < c["momentum_switch_epoch"] else c["final_momentum"]
        g = gradient(P, Y, e, reverse)[0]
        gain = np.where(np.sign(g) != np.sign(v), gain + 0.2, gain * 0.8)
        gain = np.maximum(gain, 0.01)
        v = mu * v - c["learning_rate"] * gain * g
        Y = Y + v
        Y -= Y.mean(axis=0)
    kl = gradient(P, Y, 1.0, reverse)[2]
    return (Y, kl, gain) if return_gains else (Y, kl)


def initial_embedding(m, D, seed):
    """1e-4 N(0, 1): the library's generator (sapca.synth.gaussian_panel is the same function as rng.hip)"""
    from sapca import synth
    return 1e-4 * synth.gaussian_panel(m, D, seed).numpy().astype(np.float64)


def hub_lists(m=4200, hub=300, seed=5):
    """(indices, dist), K = 3, that take the row sort of stage 3 through every length class: every row lists row 0, rows
    2 .. hub + 1 list row 1, the other slots are a ring over rows 2 .. m - 1; rows 0 and 1 list 1, 2, 3 and 0, 2, 3, so that
    the hub rows hold mutual pairs.  No row lists itself or a row twice; the distances are f32-representable."""
    i = np.arange(m)
    ring = lambda s: 2 + (i - 2 + s) % (m - 2)   # noqa: E731
    idx = np.stack([np.zeros(m, dtype=np.int64), np.where((i >= 2) & (i < 2 + hub), 1, ring(1)), ring(2)], axis=1)
    idx[0], idx[1] = (1, 2, 3), (0, 2, 3)
    dist = np.random.default_rng(seed).uniform(0.5, 1.5, size=(m, 3)).astype(np.float32)
    return idx.astype(np.int32), dist


def sort_classes(indices, wave=64, lds=4096):
    """(rows per length class, merged entries) of the raw rows stage 3 emits (a row's own valid slots in slot order, then an
    entry per row that lists it, in any order), counting a row only where it needs the sort in whatever order the second part
    arrives: its own part is not strictly ascending, or a row that lists it does not lie above its last own entry."""
    indices = np.asarray(indices)
    m, K = indices.shape
    ok = (indices >= 0) & (indices < m)
    listed_by = sp.csr_matrix((np.ones(int(ok.sum())), (indices[ok], np.repeat(np.arange(m), K).reshape(m, K)[ok])), shape=(m, m))
    counts = [0, 0, 0]
    for r in range(m):
        own = indices[r][ok[r]]
        inc = listed_by.indices[listed_by.indptr[r]:listed_by.indptr[r + 1]]
        if (np.diff(own) <= 0).any() or (own.size and inc.size and inc.min() <= own[-1]):
            n = own.size + inc.size
            counts[0 if n <= wave else 1 if n <= lds else 2] += 1
    pairs = listed_by + listed_by.T
    return counts, 2 * int(ok.sum()) - pairs.nnz


def clusters(m, d, seed, centres=3, spread=8.0):
    """(X, labels): `centres` separated Gaussian clusters in d dimensions"""
    rng = np.random.default_rng(seed)
    labels = np.arange(m) % centres
    mu = rng.normal(size=(centres, d)) * spread
    return mu[labels] + rng.normal(size=(m, d)), labels
