"""Reference for the implicit column scaling (sapca_set_column_scaling), numpy f64.

The library fits S = (A - 1 mu^T) diag(d) (center) or A diag(d) without forming it.  Because (A - 1 mu^T) D = A D - 1 (mu D)^T,
the expected fit is the existing oracle (oracle/sapca_oracle.py) run on the CSR whose values are multiplied by d[column] in
f64, with the same center, mask, normaliser and injected Omega: nothing is densified.  With covariates it is
covariates_ref.expected_fit of that matrix.  d itself comes from dense numpy with the library's rule."""
import numpy as np
import scipy.sparse as sp
import torch

import sapca_oracle as O
from sapca import synth

EPS64 = float(np.finfo(np.float64).eps)
K = 4


def column_gains(n, seed):
    """10^(4 u - 2), u = hash_u01(seed, 21, j): four decades of column scales"""
    u = synth.hash_u01(seed, 21, torch.arange(n, dtype=torch.int64)).numpy()
    return 10.0 ** (4.0 * u - 2.0)


def scaled_case(m, n, seed, *, centred=True, gains=None):
    """synth.gapped_csr(m, n, 0.3, 4, seed) with column j multiplied by column_gains (or `gains`): scipy CSR, f64"""
    ptr, idx, val = (x.numpy() for x in synth.gapped_csr(m, n, 0.3, K, seed=seed, centred=centred, dtype=torch.float64))
    g = column_gains(n, seed) if gains is None else np.asarray(gains, dtype=np.float64)
    A = sp.csr_matrix((val * g[idx], idx.astype(np.int64), ptr), shape=(m, n))
    A.sort_indices()
    return A


def edge_case():
    """320 x 208, seed 4, with column 3 emptied, column 10 stored in every row as 3.0, column 11 stored in every row as 0.1f
    and column 12 holding the single entry 2.5 in row 17"""
    A = scaled_case(320, 208, 4).tolil()
    m = A.shape[0]
    A[:, 3] = 0.0
    A[:, 12] = 0.0
    A = A.tocsr()
    A.eliminate_zeros()
    D = A.toarray()
    S = D != 0
    D[:, 10] = 3.0
    D[:, 11] = float(np.float32(0.1))
    S[:, 10] = S[:, 11] = True
    D[17, 12] = 2.5
    S[17, 12] = True
    r, c = np.nonzero(S)
    A = sp.csr_matrix((D[r, c], (r, c)), shape=(m, D.shape[1]))
    A.sort_indices()
    return A


def column_sums(A):
    """(sum, sumsq) of every column over the stored entries, f64 (numpy's own sums)"""
    D = np.asarray(A.toarray(), dtype=np.float64)
    return D.sum(axis=0), (D * D).sum(axis=0)


def unit_variance_factors(A):
    """d of SAPCA_SCALE_UNIT_VARIANCE for every column of A (dense or scipy sparse, taken to f64): ss = sumsq - sum^2 / m,
    d = 1 / sqrt(ss / (m - 1)), and 0 where ss <= 4 m eps sumsq.  Also returns (ss, sumsq) for the derived bound on d."""
    D = np.asarray(A.toarray() if sp.issparse(A) else A, dtype=np.float64)
    m = D.shape[0]
    s1, s2 = D.sum(axis=0), (D * D).sum(axis=0)
    ss = s2 - s1 * s1 / m
    dead = ss <= 4.0 * m * EPS64 * s2
    d = np.zeros(D.shape[1])
    d[~dead] = 1.0 / np.sqrt(ss[~dead] / (m - 1))
    return d, ss, s2


def factor_bound(m, ss, s2):
    """|d / d_ref - 1| <= 2 m eps sumsq / ss + 4 eps: the two sums carry at most m eps relative error each, which reaches ss
    amplified by sumsq / ss and d by half of that; the square root, the two divisions and the subtraction add the rest."""
    return 2.0 * m * EPS64 * s2 / ss + 4.0 * EPS64


def prescaled(A, d):
    """the CSR of A with every stored value multiplied by d[column], in f64"""
    A = sp.csr_matrix(A, dtype=np.float64)
    return sp.csr_matrix((A.data * np.asarray(d, dtype=np.float64)[A.indices], A.indices, A.indptr), shape=A.shape)


def expected_fit(A, d, *, center, n_components, n_oversamples, n_power_iterations, normalizer, omega, mask=None):
    """the oracle's fit of A diag(d) (d: full width)"""
    B = prescaled(A, d)
    m, n = B.shape
    return O.fit(B.indptr.astype(np.int64), B.indices.astype(np.int64), B.data, m, n, n_components=n_components,
                 n_oversamples=n_oversamples, n_power_iterations=n_power_iterations, normalizer=normalizer, center=center,
                 omega=omega, mask=mask)


def scaled_operator(A, d, center, mask=None):
    """S, dense: (A - 1 mu^T) diag(d) or A diag(d), over the columns the mask keeps"""
    D = np.asarray(A.toarray() if sp.issparse(A) else A, dtype=np.float64)
    if center:
        D = D - D.mean(axis=0)
    S = D * np.asarray(d, dtype=np.float64)
    return S if mask is None else S[:, np.asarray(mask, dtype=bool)]


def gap(S, k):
    sv = np.linalg.svd(S, compute_uv=False)
    return float(sv[k - 1] / sv[k])
